"""Two-pass decoding (kernels/nrtr_twopass.h: ccd_nrtr_twopass_rows, ccd_nrtr_twopass_select) restated in numpy: the specification of
both kernels, and of the whole decoder given frame probabilities and a callable attention scorer.

  proposals  paths int32 [B, W, Tp], CTC classes (0 is the blank, never part of a word), -1-padded; lengths int32 [B, W], -1 for an unused
             slot.  CTC class c is decoder class d = c - class_offset.
  rows       slot k of image b is eligible iff 0 <= n <= min(Tp, seq_len - 2, Lmax) and every one of its n classes has c >= 1, 0 <= d <
             classes, d != end_idx, d != pad_idx.  seq row: <BOS> d1 .. dn <EOS> <PAD>.., targets row: c1 .. cn 0.., subset: b * W + k;
             an ineligible slot: <BOS> <PAD>.., zeros, -1.
  select     eligible iff subset >= 0, 0 <= n <= min(Tp, T) and both scores are finite; S = (1 - w) att + w ctc in fp64 with the fp32
             scores widened first, a term whose weight is exactly 0 left out; ranks by (S descending, slot ascending).
"""
import numpy as np

import ctc_beam_np as R
import ctc_lexicon_np as L


def rows(paths, lengths, class_offset, classes, start_idx, end_idx, pad_idx, seq_len, Lmax):
    """-> (seq int64 [B * W, seq_len], targets int64 [B * W, Lmax], subset int32 [B, W])."""
    paths, lengths = np.asarray(paths), np.asarray(lengths)
    B, W, Tp = paths.shape
    seq = np.full((B * W, seq_len), pad_idx, dtype=np.int64)
    seq[:, 0] = start_idx
    targets = np.zeros((B * W, Lmax), dtype=np.int64)
    subset = np.full((B, W), -1, dtype=np.int32)
    for b in range(B):
        for k in range(W):
            n = int(lengths[b, k])
            if not 0 <= n <= min(Tp, seq_len - 2, Lmax):
                continue
            c = paths[b, k, :n].astype(np.int64)
            d = c - class_offset
            if ((c < 1) | (d < 0) | (d >= classes) | (d == end_idx) | (d == pad_idx)).any():
                continue
            r = b * W + k
            seq[r, 1:1 + n] = d
            seq[r, 1 + n] = end_idx
            targets[r, :n] = c
            subset[b, k] = r
    return seq, targets, subset


def combine(att, ctc, w):
    """S of one slot, fp64: the fp32 scores widened, the zero-weighted term left out."""
    a, c, w = np.float64(np.float32(att)), np.float64(np.float32(ctc)), np.float64(w)
    if w == 0:
        return a
    if w == 1:
        return c
    return (1 - w) * a + w * c


def select(att, ctc, paths, lengths, subset, w, T, class_offset):
    """att fp32 [B * W], ctc fp32 [B, W] -> (out_paths int32 [B, W, T], out_lengths int32 [B, W], scores, att_scores, ctc_scores fp32
    [B, W], source int32 [B, W])."""
    paths, lengths, subset = np.asarray(paths), np.asarray(lengths), np.asarray(subset)
    B, W, Tp = paths.shape
    att, ctc = np.asarray(att, dtype=np.float32).reshape(B, W), np.asarray(ctc, dtype=np.float32).reshape(B, W)
    out_paths = np.full((B, W, T), -1, dtype=np.int32)
    out_lengths = np.full((B, W), -1, dtype=np.int32)
    scores, att_s, ctc_s = (np.full((B, W), -np.inf, dtype=np.float32) for _ in range(3))
    source = np.full((B, W), -1, dtype=np.int32)
    for b in range(B):
        cand = []
        for k in range(W):
            n = int(lengths[b, k])
            if subset[b, k] >= 0 and 0 <= n <= min(Tp, T) and np.isfinite(att[b, k]) and np.isfinite(ctc[b, k]):
                cand.append((-combine(att[b, k], ctc[b, k], w), k))
        for r, (neg, k) in enumerate(sorted(cand)):                            # S descending, slot ascending
            n = int(lengths[b, k])
            out_paths[b, r, :n] = paths[b, k, :n] - class_offset
            out_lengths[b, r], source[b, r] = n, k
            scores[b, r], att_s[b, r], ctc_s[b, r] = np.float32(-neg), att[b, k], ctc[b, k]
    return out_paths, out_lengths, scores, att_s, ctc_s, source


def ctc_score_paths(frames, paths, lengths, normalized=False, max_labels=31):
    """frames [B, T, C] -> fp64 [B, W]: the exact log p(word | frames) of every proposal by tests/ctc_lexicon_np.py, -inf for an unused
    slot and a path of more than max_labels characters."""
    paths, lengths = np.asarray(paths), np.asarray(lengths)
    B, W, _ = paths.shape
    out = np.full((B, W), -np.inf)
    for b in range(B):
        lp = R.log_probs(np.asarray(frames[b]), normalized)
        for k in range(W):
            n = int(lengths[b, k])
            if 0 <= n <= min(max_labels, paths.shape[2]):
                out[b, k] = L.word_score(lp, paths[b, k, :n].tolist())
    return out


def decode(frames, paths, lengths, att_scorer, w, classes, start_idx, end_idx, pad_idx, T, class_offset=1, normalized=True, Lmax=None):
    """The whole decoder: frames [B, Tc, Cc] of the CTC head, the proposals, att_scorer(seq int64 [B * W, T + 1]) -> fp32 [B * W] the
    attention decoder's log p(word <EOS> | image) of every row (-inf for a row without an <EOS>) -> select's six outputs."""
    paths, lengths = np.asarray(paths), np.asarray(lengths)
    Lmax = min(paths.shape[2], 31) if Lmax is None else Lmax
    seq, targets, subset = rows(paths, lengths, class_offset, classes, start_idx, end_idx, pad_idx, T + 1, Lmax)
    ctc = ctc_score_paths(frames, paths, lengths, normalized=normalized, max_labels=Lmax)
    ctc = np.where(subset >= 0, ctc, -np.inf).astype(np.float32)
    att = np.asarray(att_scorer(seq), dtype=np.float32)
    return select(att, ctc, paths, lengths, subset, w, T, class_offset)
