"""numpy restatement of Dino/metric/eval_IOU.py for the tests, the loader of tests/golden/iou_cases.npz and seeded label maps.

The confusion matrix is one np.bincount over gt * 32 + eval; with t / n / d its row sums, column sums and diagonal,
G = {t > 0}, E = {n > 0}:
    pixel_accuracy = sum_G d / sum_G t                    mean_accuracy = (sum_G d / t) / |G|
    mean_IU = (sum_{G and E} d / (t + n - d)) / |G|       frequency_weighted_IU = (sum_{G and E} t d / (t + n - d)) / (H W)
    fore_IU = d_k / (t_k + n_k - d_k + 1e-6), k the second-smallest label of G or E (None when there is no such label)
The sums over the classes are numpy's (np.sum of float64 quotients), as in the reference."""
import os

import numpy as np

CLASSES = 32
NAMES = ("pixel_accuracy", "mean_accuracy", "mean_IU", "fore_IU", "frequency_weighted_IU")


def confusion(eval_segm, gt_segm):
    """int64 [32, 32] counts of one [H, W] (or flat) pair of maps with labels in [0, 32): cm[g, e]."""
    e = np.asarray(eval_segm).astype(np.int64).ravel()
    g = np.asarray(gt_segm).astype(np.int64).ravel()
    assert e.shape == g.shape and e.size and 0 <= min(e.min(), g.min()) and max(e.max(), g.max()) < CLASSES
    return np.bincount(g * CLASSES + e, minlength=CLASSES * CLASSES).reshape(CLASSES, CLASSES)


def scores_of(cm):
    """The five scores of one confusion matrix as a float64 [5] array; fore_IU is NaN when the union has fewer than two classes."""
    cm = np.asarray(cm, dtype=np.int64)
    t, n, d = cm.sum(1), cm.sum(0), np.diagonal(cm)
    G, E = t > 0, n > 0
    both = G & E
    union = np.flatnonzero(G | E)
    n_gt = int(G.sum())
    iu_den = (t + n - d)[both]
    out = np.full(5, np.nan)
    out[0] = d[G].sum() / t[G].sum()
    out[1] = np.sum(d[G] / t[G]) / n_gt
    out[2] = np.sum(d[both] / iu_den) / n_gt
    if len(union) > 1:
        k = union[1]
        out[3] = d[k] / (t[k] + n[k] - d[k] + 1e-6)
    out[4] = np.sum((t[both] * d[both]) / iu_den) / t.sum()
    return out


def scores(eval_segm, gt_segm):
    return scores_of(confusion(eval_segm, gt_segm))


def batch(evals, gts):
    """-> (cm int64 [B, 32, 32], scores float64 [B, 5]) of a batch of pairs."""
    cms = np.stack([confusion(e, g) for e, g in zip(evals, gts)])
    return cms, np.stack([scores_of(c) for c in cms])


def load_cases(golden_dir):
    """-> (names, {name: {eval, gt (uint8 [H, W]), scores (float64 [5], NaN where fore_IU raised), fore_raised, eval_classes,
    gt_classes, union_classes}}, the reference's public names)."""
    z = np.load(os.path.join(golden_dir, "iou_cases.npz"))
    names = [str(n) for n in z["names"]]
    cases = {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in names}
    return names, cases, [str(s) for s in z["api"]]


def random_maps(shape, classes, seed, flip=0.1):
    """(eval, gt) uint8 maps of `shape`: gt uniform over `classes` labels, eval = gt with a share `flip` of the pixels redrawn."""
    rs = np.random.RandomState(seed)
    gt = rs.randint(0, classes, size=shape).astype(np.uint8)
    redraw = rs.rand(*shape) < flip
    ev = np.where(redraw, rs.randint(0, classes, size=shape), gt).astype(np.uint8)
    return ev, gt


def text_like(shape, seed):
    """A binary (eval, gt) pair with box-shaped 'characters' in gt and a shifted, slightly eroded prediction."""
    rs = np.random.RandomState(seed)
    H, W = shape[-2:]
    gt = np.zeros(shape, dtype=np.uint8)
    flat = gt.reshape(-1, H, W)
    for img in flat:
        x = 2
        while x < W - 4:
            w = rs.randint(3, 9)
            y0 = rs.randint(0, max(1, H // 4))
            img[y0 + H // 4:H - rs.randint(1, max(2, H // 4)), x:min(x + w, W)] = 1
            x += w + rs.randint(1, 5)
    ev = np.roll(gt, 1, axis=-1) & (rs.rand(*shape) > 0.05)
    return ev.astype(np.uint8), gt
