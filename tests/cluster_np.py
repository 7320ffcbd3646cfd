"""Pure-numpy restatement of the three clusterers of the reference's Dino/utils/DBSCAN.py (test code, not product; no scipy /
sklearn, so it also runs where only numpy is installed).  Ties are broken the way the kernels break them: mean-column ties by
cluster number / label order, region_cluster's sort is stable like the reference's.

  dbscan_idmap(mask)   DBSCAN_cluster   (DBSCAN.py:10-59)  sklearn DBSCAN(eps=1.5, min_samples=4) on the pixels > 0.1, restated:
                       core = >= 3 foreground 8-neighbours; clusters = 8-connected core components numbered by their first core
                       pixel; a border pixel joins the lowest-numbered neighbouring cluster; >= 30 pixels; 26 leftmost.
  label_idmap(mask)    label_cluster    (DBSCAN.py:61-103)
  region_boxes(mask)   region_cluster   (DBSCAN.py:106-141) -> list of (ymin, xmin, ymax, xmax), half-open
"""
from fractions import Fraction

import numpy as np

from oracle import ccl_np

BG, PLANES, MIN_AREA, MIN_BOX_AREA = 255, 26, 30, 100


def _neighbour_views(a, fill):
    h, w = a.shape
    p = np.pad(a, 1, constant_values=fill)
    return [p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]


def dbscan_assign(mask):
    """int64 [H,W]: cluster number (0, 1, .. in sklearn's discovery order) of every pixel, -1 = background or noise."""
    fg = np.asarray(mask, dtype=np.float32) > np.float32(0.1)
    nbrs = sum(v.astype(np.int32) for v in _neighbour_views(fg, False))
    core = fg & (nbrs >= 3)
    comp = ccl_np.components_8conn(core).astype(np.int64)           # 0 = not core, else root + 1
    big = np.iinfo(np.int64).max
    best = np.full(fg.shape, big)
    for v in _neighbour_views(np.where(core, comp, big), big):
        best = np.minimum(best, v)
    lab = np.where(core, comp, np.where(fg & (best != big), best, 0))
    roots = np.unique(lab[lab > 0])
    out = np.full(fg.shape, -1, dtype=np.int64)
    out[lab > 0] = np.searchsorted(roots, lab[lab > 0])
    return out


def dbscan_idmap(mask):
    ids = dbscan_assign(mask)
    kept = []                                                       # (mean column, cluster number)
    for c in range(ids.max() + 1):
        xs = np.nonzero(ids == c)[1]
        if xs.size >= MIN_AREA:
            kept.append((Fraction(int(xs.sum()), int(xs.size)), c))
    out = np.full(ids.shape, BG, dtype=np.uint8)
    for plane, (_, c) in enumerate(sorted(kept)[:PLANES]):
        out[ids == c] = plane
    return out


def label_idmap(mask):
    return ccl_np.label_idmap(np.asarray(mask) != 0)


def region_boxes(mask, reverse_ties=False):
    """reverse_ties: equal sort keys in reverse label order instead (not the reference: shows that a fixture pins the order)."""
    comp = ccl_np.components_8conn(np.asarray(mask) != 0)
    regions = []
    labels = np.unique(comp[comp > 0])                              # label order = raster order of the first pixel
    for lab in (labels[::-1] if reverse_ties else labels):
        ys, xs = np.nonzero(comp == lab)
        regions.append((int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1))
    regions = sorted(regions, key=lambda b: b[1] + b[3])[:PLANES]   # stable
    return [b for b in regions if (b[3] - b[1]) * (b[2] - b[0]) >= MIN_BOX_AREA]


def idmap_planes(idmap):
    """uint8 [..., H, W] id map -> uint8 [..., 26, H, W]."""
    idmap = np.asarray(idmap)
    return (idmap[..., None, :, :] == np.arange(PLANES, dtype=np.uint8)[:, None, None]).astype(np.uint8)


def box_planes(boxes, shape=(32, 128)):
    out = np.zeros((PLANES,) + tuple(shape), dtype=np.uint8)
    for k, (y0, x0, y1, x1) in enumerate(boxes):
        out[k, y0:y1, x0:x1] = 1
    return out


def dbscan_planes(mask):
    return idmap_planes(dbscan_idmap(mask))


def label_planes(mask):
    return idmap_planes(label_idmap(mask))


def region_planes(mask):
    return box_planes(region_boxes(mask), np.asarray(mask).shape)


CLUSTERERS = {"dbscan": dbscan_planes, "label": label_planes, "region": region_planes}


def load_cases(golden_dir):
    """-> names, float32 masks [N,32,128], {clusterer: uint8 planes [N,26,32,128]}, {clusterer: has_tie [N]}."""
    import os
    g = np.load(os.path.join(golden_dir, "cluster_cases.npz"))
    planes = {k: np.unpackbits(g[k], axis=-1) for k in CLUSTERERS}
    ties = {k: g["has_tie"][:, i] for i, k in enumerate(CLUSTERERS)}
    return list(g["names"]), g["masks"], planes, ties


def random_masks(n, seed):
    """Binary masks at several densities, dilated specks and float masks around DBSCAN's 0.1 threshold."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        kind = i % 3
        if kind == 0:
            m = (rs.uniform(size=(32, 128)) < rs.uniform(0.05, 0.75)).astype(np.float32)
        elif kind == 1:
            s = rs.uniform(size=(32, 128)) < rs.uniform(0.01, 0.08)
            d = s.copy()
            d[1:] |= s[:-1]; d[:, 1:] |= s[:, :-1]; d[1:, 1:] |= s[:-1, :-1]
            m = d.astype(np.float32)
        else:
            m = (rs.uniform(size=(32, 128)) * rs.uniform(0.12, 0.4)).astype(np.float32)
        out.append(m)
    return np.stack(out)
