"""The segmentation metrics of the reference (Dino/metric/eval_IOU.py), on the GPU: `pixel_accuracy`, `mean_accuracy`, `mean_IU`,
`fore_IU`, `frequency_weighted_IU`, their helpers and `EvalSegErr` (also importable as `Dino.metric.eval_IOU`), plus the batched
entry points `confusion`, `segmentation_scores`, `seg_logits_scores` and the accumulator `SegMeter`.

    pixel_accuracy(eval_segm, gt_segm) etc.
        numpy [H, W] pair                  -> float64 scalar (the reference contract; computed on the current GPU, one host read)
        torch [H, W] / [B, H, W] pair      -> float64 0-dim / [B] tensor on the maps' device, no host synchronisation
    confusion(eval_segm, gt_segm)           -> int32 [B, 32, 32], cm[i, g, e] = pixels of image i with gt label g and eval label e
    segmentation_scores(eval_segm, gt_segm) -> SegScores: the five scores as float64 [B] tensors and `status`; two launches in all
    seg_logits_scores(logits, gt_segm)      -> the same with eval = argmax over the channels of fp32 [N, C, H, W] logits, e.g.
                                               seg_logits_scores(student_out['mask'][:B], masks): the view and the fp32 0/1 masks
                                               are read in place, the prediction is never written
    SegMeter().update(eval, gt) / .update_logits(logits, gt) / .compute() / .reset()

One launch builds the per-image 32 x 32 confusion matrix (`ccd_seg_confusion`, `ccd_seg_confusion_logits`), one more turns it into
the five scores (`ccd_seg_scores`).  With t_c / n_c / d_c the row sum, column sum and diagonal of an image's matrix,
G = {c: t_c > 0}, E = {c: n_c > 0}:
    pixel_accuracy = sum_G d_c / sum_G t_c                 mean_accuracy = (sum_G d_c / t_c) / |G|
    mean_IU = (sum_{G and E} d_c / (t_c + n_c - d_c)) / |G|
    fore_IU = d_k / (t_k + n_k - d_k + 1e-6), k the second-smallest label of G or E
    frequency_weighted_IU = (sum_{G and E} t_c d_c / (t_c + n_c - d_c)) / (H W)
`status` is an int32 per image: bit 0 = the image holds a label outside [0, 32), a non-integral value or a NaN (all five scores
NaN), bit 1 = fore_IU is undefined (fewer than two classes in the union of the two maps; that score is NaN).

Differences from the reference:
  * Labels are integers in [0, 32) (`ops.SEG_CLASSES`): uint8, bool, int32, int64, or float32 holding integral values.  The
    reference takes whatever np.unique can sort.  Other dtypes raise TypeError on the tensor path; numpy arrays of other dtypes are
    converted to int64 when that is exact (ValueError otherwise).
  * The GPU path also covers torch tensors, batched; CPU tensors raise RuntimeError (there is no host path).
  * On the tensor path a failure is a NaN, not an exception: raising would need a host synchronisation.  The numpy path raises as
    the reference does: EvalSegErr when the shapes differ, IndexError from fore_IU when the union has one class, and ValueError
    for labels this module does not take.
  * The class sums run in ascending class order in fp64; numpy's sum and mean use their own blocked order from 8 terms up.  The
    values differ from the reference's by a few ulp at most (a sum of at most 32 quotients in [0, 1]).
  * A 1-D or 0-d numpy input raises EvalSegErr (the reference: IndexError from segm_size).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import _lib, ops

SegScores = namedtuple("SegScores", ops.SEG_SCORES + ("status",))
_NP_DIRECT = (np.uint8, np.int32, np.int64, np.float32)


class EvalSegErr(Exception):
    def __init__(self, value):
        self.value = value

    def __str__(self):
        return repr(self.value)


# ------------------------------------------------------------------------------------------ the reference's helpers (host numpy)
def get_pixel_area(segm):
    return segm.shape[0] * segm.shape[1]


def segm_size(segm):
    return segm.shape[0], segm.shape[1]


def check_size(eval_segm, gt_segm):
    if segm_size(eval_segm) != segm_size(gt_segm):
        raise EvalSegErr("DiffDim: Different dimensions of matrices!")


def extract_classes(segm):
    cl = np.unique(segm)
    return cl, len(cl)


def union_classes(eval_segm, gt_segm):
    cl = np.union1d(extract_classes(eval_segm)[0], extract_classes(gt_segm)[0])
    return cl, len(cl)


def extract_masks(segm, cl, n_cl):
    h, w = segm_size(segm)
    masks = np.zeros((n_cl, h, w))
    for i, c in enumerate(cl):
        masks[i] = segm == c
    return masks


def extract_both_masks(eval_segm, gt_segm, cl, n_cl):
    return extract_masks(eval_segm, cl, n_cl), extract_masks(gt_segm, cl, n_cl)


# ------------------------------------------------------------------------------------------ inputs
def _device_for_numpy():
    if _lib._stream_override is not None:           # the C ABI is bound to a host executor (kernel tests)
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise RuntimeError("ccd_amd.metric.eval_IOU runs on an AMD GPU only; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _from_numpy(a, what):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    elif a.dtype.type not in _NP_DIRECT:
        if a.dtype.kind not in "iuf":
            raise ValueError(f"{what}: labels must be integers in [0, {ops.SEG_CLASSES}), got dtype {a.dtype}")
        with np.errstate(invalid="ignore"):
            i = a.astype(np.int64)
        if not np.array_equal(i, a):
            raise ValueError(f"{what}: labels must be integers in [0, {ops.SEG_CLASSES})")
        a = i
    return torch.from_numpy(np.ascontiguousarray(a)).to(_device_for_numpy())


def _check_tensor(x, what, logits=False):
    if logits and x.dtype != torch.float32:
        raise TypeError(f"{what}: logits must be float32, got {str(x.dtype)[6:]}")
    if not logits and x.dtype != torch.bool and x.dtype not in ops.SEG_DTYPES:
        raise TypeError(f"{what}: label maps are uint8, bool, int32, int64 or float32, got {str(x.dtype)[6:]}")
    if x.device.type != "cuda" and _lib._stream_override is None:
        raise RuntimeError(f"{what} runs on an AMD GPU only (move the tensors with .cuda() first); there is no CPU path")


def _pair(eval_segm, gt_segm, what):
    """-> (eval [B, H, W], gt [B, H, W], was_numpy, was_2d) on the device."""
    tensors = [isinstance(x, torch.Tensor) for x in (eval_segm, gt_segm)]
    if tensors[0] != tensors[1]:
        raise TypeError(f"{what}: expects two numpy arrays or two torch tensors")
    if not tensors[0]:
        e, g = np.asarray(eval_segm), np.asarray(gt_segm)
        if e.ndim != 2 or g.ndim != 2:
            raise EvalSegErr(f"{what}: the numpy path takes [H, W] maps, got {list(e.shape)} and {list(g.shape)}")
        check_size(e, g)
        return _from_numpy(e, what)[None], _from_numpy(g, what)[None], True, True
    e, g = eval_segm, gt_segm
    if e.dim() not in (2, 3) or e.dim() != g.dim() or tuple(e.shape) != tuple(g.shape):
        raise EvalSegErr(f"DiffDim: Different dimensions of matrices! ({what}: {list(e.shape)} and {list(g.shape)})")
    for x in (e, g):
        _check_tensor(x, what)
    if e.device != g.device:
        raise ValueError(f"{what}: the maps are on different devices")
    was_2d = e.dim() == 2
    return (e[None], g[None], False, True) if was_2d else (e, g, False, False)


def _scores(eval_segm, gt_segm, what):
    e, g, was_numpy, was_2d = _pair(eval_segm, gt_segm, what)
    if min(e.shape[1:], default=0) < 1:
        raise ValueError(f"{what}: empty maps {list(e.shape)}")
    cm, status = ops.seg_confusion(e, g)
    return cm, ops.seg_scores(cm, status), status, was_numpy, was_2d


def _metric(k, eval_segm, gt_segm):
    name = ops.SEG_SCORES[k]
    _, scores, status, was_numpy, was_2d = _scores(eval_segm, gt_segm, name)
    if not was_numpy:
        return scores[0, k] if was_2d else scores[:, k]
    host = torch.cat([scores[0], status.to(torch.float64)]).cpu().numpy()         # the one host read
    st = int(host[5])
    if st & 1:
        raise ValueError(f"{name}: labels must be integers in [0, {ops.SEG_CLASSES})")
    if k == 3 and st & 2:
        raise IndexError("index 1 is out of bounds for axis 0 with size 1")       # the reference's eval_mask[1] on a one-class union
    return host[k]


def pixel_accuracy(eval_segm, gt_segm):
    """sum_i(n_ii) / sum_i(t_i)"""
    return _metric(0, eval_segm, gt_segm)


def mean_accuracy(eval_segm, gt_segm):
    """(1/n_cl) sum_i(n_ii/t_i)"""
    return _metric(1, eval_segm, gt_segm)


def mean_IU(eval_segm, gt_segm):
    """(1/n_cl) * sum_i(n_ii / (t_i + sum_j(n_ji) - n_ii))"""
    return _metric(2, eval_segm, gt_segm)


def fore_IU(eval_segm, gt_segm):
    """n_ii / (t_i + sum_j(n_ji) - n_ii + 1e-6) of the second-smallest class of the union (the text class of a binary map)"""
    return _metric(3, eval_segm, gt_segm)


def frequency_weighted_IU(eval_segm, gt_segm):
    """sum_k(t_k)^(-1) * sum_i((t_i*n_ii)/(t_i + sum_j(n_ji) - n_ii))"""
    return _metric(4, eval_segm, gt_segm)


# ------------------------------------------------------------------------------------------ batched entry points
def confusion(eval_segm, gt_segm):
    """int32 [B, 32, 32] confusion matrices of a torch [H, W] / [B, H, W] pair (rows: gt label, columns: eval label)."""
    return _scores_of_maps(eval_segm, gt_segm, "confusion")[0]


def _scores_of_maps(eval_segm, gt_segm, what):
    if not (isinstance(eval_segm, torch.Tensor) and isinstance(gt_segm, torch.Tensor)):
        raise TypeError(f"{what}: expects torch tensors")
    cm, scores, status, _, _ = _scores(eval_segm, gt_segm, what)
    return cm, scores, status


def _gt_for_logits(logits, gt_segm, what):
    if not (isinstance(logits, torch.Tensor) and isinstance(gt_segm, torch.Tensor)):
        raise TypeError(f"{what}: expects torch tensors")
    if logits.dim() != 4:
        raise ValueError(f"{what}: expects [N, C, H, W] logits, got {list(logits.shape)}")
    g = gt_segm[:, 0] if gt_segm.dim() == 4 and gt_segm.shape[1] == 1 else gt_segm
    if g.dim() != 3 or tuple(g.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise EvalSegErr(f"DiffDim: Different dimensions of matrices! ({what}: logits {list(logits.shape)}, gt {list(gt_segm.shape)})")
    if min(logits.shape[2:]) < 1:
        raise ValueError(f"{what}: empty maps {list(logits.shape)}")
    _check_tensor(logits, what, logits=True)
    _check_tensor(g, what)
    if logits.device != g.device:
        raise ValueError(f"{what}: logits and gt are on different devices")
    return g


def _scores_of_logits(logits, gt_segm, what):
    g = _gt_for_logits(logits, gt_segm, what)
    cm, status = ops.seg_confusion_logits(logits, g)
    return cm, ops.seg_scores(cm, status), status


def _as_tuple(scores, status):
    return SegScores(*(scores[:, k] for k in range(5)), status)


def segmentation_scores(eval_segm, gt_segm):
    """All five scores of a torch [B, H, W] (or [H, W]: B = 1) pair from one pass: SegScores of float64 [B] tensors + status."""
    _, scores, status = _scores_of_maps(eval_segm, gt_segm, "segmentation_scores")
    return _as_tuple(scores, status)


def seg_logits_scores(logits, gt_segm):
    """The same with eval = argmax over C of fp32 [N, C, H, W] logits (first maximum; two classes: logit1 > logit0)."""
    _, scores, status = _scores_of_logits(logits, gt_segm, "seg_logits_scores")
    return _as_tuple(scores, status)


def _scores_of_matrix(cm):
    """The five scores of one [32, 32] matrix of Python ints on the host (the pooled matrix of SegMeter.compute), same order of
    operations as ccd_seg_scores.  -> list of 5 floats, NaN where undefined."""
    nan = float("nan")
    n = len(cm)
    t = [sum(cm[c]) for c in range(n)]
    e = [sum(cm[g][c] for g in range(n)) for c in range(n)]
    d = [cm[c][c] for c in range(n)]
    gt = [c for c in range(n) if t[c] > 0]
    union = [c for c in range(n) if t[c] > 0 or e[c] > 0]
    if not gt:
        return [nan] * 5
    both = [c for c in gt if e[c] > 0]
    acc = iu = fw = 0.0
    for c in gt:
        acc += d[c] / t[c]
    for c in both:
        iu += d[c] / (t[c] + e[c] - d[c])
        fw += (t[c] * d[c]) / (t[c] + e[c] - d[c])
    area = sum(t[c] for c in gt)
    k = union[1] if len(union) > 1 else None
    fore = d[k] / (t[k] + e[k] - d[k] + 1e-6) if k is not None else nan
    return [sum(d[c] for c in gt) / area, acc / len(gt), iu / len(gt), fore, fw / area]


class SegMeter:
    """Accumulates the scores over batches, on the device, without a host synchronisation:
        meter.update(eval_segm, gt_segm) / meter.update_logits(logits, gt_segm)
        meter.compute() -> {the five names: the mean over the images where the score is defined (as one would average the
                            reference's per-image values), 'n_images', 'n_fore_defined', 'dataset_<name>': the five scores of the
                            pooled confusion matrix}          (one host read)
    Images with invalid labels (status bit 0) count in n_images and nowhere else."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.sums = None          # fp64 [5]: per-score sums over the images where the score is defined
        self.counts = None        # int64 [5]: how many those are
        self.pooled = None        # int64 [32, 32]
        self.n_images = 0

    def _add(self, cm, scores, status):
        if self.sums is None:
            dev = scores.device
            self.sums = torch.zeros(5, dtype=torch.float64, device=dev)
            self.counts = torch.zeros(5, dtype=torch.int64, device=dev)
            self.pooled = torch.zeros((ops.SEG_CLASSES, ops.SEG_CLASSES), dtype=torch.int64, device=dev)
        defined = ~torch.isnan(scores)
        self.sums += torch.where(defined, scores, torch.zeros_like(scores)).sum(0)
        self.counts += defined.sum(0)
        valid = ((status & 1) == 0).to(torch.int64)
        self.pooled += (cm.to(torch.int64) * valid[:, None, None]).sum(0)
        self.n_images += scores.shape[0]

    def update(self, eval_segm, gt_segm):
        self._add(*_scores_of_maps(eval_segm, gt_segm, "SegMeter.update"))

    def update_logits(self, logits, gt_segm):
        self._add(*_scores_of_logits(logits, gt_segm, "SegMeter.update_logits"))

    def compute(self):
        nan = float("nan")
        out = {"n_images": self.n_images}
        if self.sums is None:
            out.update({name: nan for name in ops.SEG_SCORES}, n_fore_defined=0)
            out.update({f"dataset_{name}": nan for name in ops.SEG_SCORES})
            return out
        host = torch.cat([self.sums.view(torch.int64), self.counts, self.pooled.flatten()]).cpu()       # the one host read
        sums, counts, pooled = host[:5].view(torch.float64).tolist(), host[5:10].tolist(), host[10:].tolist()
        for k, name in enumerate(ops.SEG_SCORES):
            out[name] = sums[k] / counts[k] if counts[k] else nan
        out["n_fore_defined"] = counts[3]
        n = ops.SEG_CLASSES
        dataset = _scores_of_matrix([pooled[r * n:(r + 1) * n] for r in range(n)])
        out.update({f"dataset_{name}": dataset[k] for k, name in enumerate(ops.SEG_SCORES)})
        return out
