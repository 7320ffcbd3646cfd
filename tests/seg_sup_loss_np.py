"""The supervised segmentation loss (ccd_amd/loss/seg_loss.py, kernels/seg_sup_loss.h) restated in numpy fp64: loss, parts,
gradient and confusion matrix.  z: logits [N, 2, H, W], gt: uint8 [N, H, W] (0 background, 1 text, anything else not scored)."""
import numpy as np


def scored(gt):
    return (gt == 0) | (gt == 1)


def edge_band(gt, r):
    """bool [N, H, W]: the pixel is scored and a scored pixel of the other class lies inside the image within the (2r + 1)^2 square
    around it.  Shifted copies, one per offset."""
    gt = np.asarray(gt)
    N, H, W = gt.shape
    near = {c: np.zeros((N, H, W), dtype=bool) for c in (0, 1)}        # a pixel of class c within the square
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            for c in (0, 1):
                near[c][:, yd, xd] |= gt[:, ys, xs] == c
    return ((gt == 0) & near[1]) | ((gt == 1) & near[0]) if r > 0 else np.zeros((N, H, W), dtype=bool)


def edge_band_brute(gt, r):
    """The same by the definition: a double loop over the pixels and their squares."""
    gt = np.asarray(gt)
    N, H, W = gt.shape
    out = np.zeros((N, H, W), dtype=bool)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                if gt[n, y, x] > 1 or r == 0:
                    continue
                for yy in range(max(0, y - r), min(H, y + r + 1)):
                    for xx in range(max(0, x - r), min(W, x + r + 1)):
                        if gt[n, yy, xx] <= 1 and gt[n, yy, xx] != gt[n, y, x]:
                            out[n, y, x] = True
    return out


def seg_sup_loss(z, gt, class_weight=(1.0, 1.0), dice_weight=0.0, edge_weight=0.0, edge_radius=0, d_loss=1.0):
    """-> dict: loss, parts [L, CE, Dice, Omega], grad [N, 2, H, W] (d_loss * dL/dz), confusion int64 [2, 2] = [gt, pred]."""
    z = np.asarray(z, dtype=np.float64)
    gt = np.asarray(gt)
    N = z.shape[0]
    valid = scored(gt)
    y = (gt == 1).astype(np.float64)
    d = z[:, 1] - z[:, 0]
    p = 1.0 / (1.0 + np.exp(-d))
    l = np.logaddexp(0.0, np.where(y > 0, -d, d))                      # -log softmax(z)[y]
    w = np.where(y > 0, class_weight[1], class_weight[0]) * (1.0 + edge_weight * edge_band(gt, edge_radius)) * valid
    omega = w.sum()
    ce = (w * l).sum() / omega if omega > 0 else 0.0
    has = valid.reshape(N, -1).any(axis=1)
    nv = int(has.sum())
    I = (p * y * valid).reshape(N, -1).sum(1)
    P = (p * valid).reshape(N, -1).sum(1)
    G = (y * valid).reshape(N, -1).sum(1)
    S = P + G + 1.0
    dice_n = 1.0 - (2.0 * I + 1.0) / S
    dice = dice_n[has].sum() / nv if nv else 0.0
    loss = ce + dice_weight * dice
    g1 = np.zeros_like(d)
    if omega > 0:
        g1 += w * (p - y) / omega
    if nv:
        g1 -= (dice_weight / nv) * ((2.0 * y * S[:, None, None] - (2.0 * I + 1.0)[:, None, None]) / (S * S)[:, None, None]) * p * (1.0 - p) * valid
    g1 *= d_loss
    pred = z[:, 1] > z[:, 0]
    cm = np.array([[int((valid & (gt == g) & (pred == e)).sum()) for e in (0, 1)] for g in (0, 1)], dtype=np.int64)
    return {"loss": loss, "parts": np.array([loss, ce, dice, omega]), "grad": np.stack([-g1, g1], axis=1), "confusion": cm}
