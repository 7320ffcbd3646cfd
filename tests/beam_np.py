"""The two rules the fp64 specifications of the beam decoders share (ctc_beam_np.py, nrtr_beam_np.py; kernels/beam_wave.h).
A case is only compared with an implementation where the gap `select` returns is >= MIN_GAP, nine orders above the rounding of the
fp64 arithmetic: there the implementation must reproduce the selection and its order exactly."""
import numpy as np

MIN_GAP = 1e-9


def log_softmax64(row):
    """An fp32 logits row -> x - max - log sum exp(x - max) in fp64, the sum over the classes in ascending order, as the kernels add.
    A -inf logit gives -inf; a row of nothing else is -inf everywhere."""
    x = np.asarray(row, dtype=np.float32).astype(np.float64)
    m = x.max()
    if m == -np.inf:
        return np.full(x.shape, -np.inf)
    with np.errstate(divide="ignore"):
        return (x - m) - np.log(np.cumsum(np.exp(x - m))[-1])    # (cumsum adds one by one, in ascending order)


def select(scores, W, ties=False):
    """scores fp64, any shape: candidate k is element k of the flattened array, -inf is no candidate -> (the k of the W best by
    (score descending, k ascending), at most W of them; the smallest difference of neighbouring scores among the W + 1 best, inf
    where there are fewer than two).  ties=True leaves exact ties (bit-identical scores, ordered by k) out of the gap."""
    flat = np.asarray(scores, dtype=np.float64).ravel()
    order = np.argsort(-flat, kind="stable")                     # score descending, k ascending among equals
    order = order[flat[order] > -np.inf]
    near = -np.diff(flat[order[:W + 1]])
    if ties:
        near = near[near > 0]
    return order[:W], float(near.min()) if near.size else np.inf
