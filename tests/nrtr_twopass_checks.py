"""The checks of two-pass decoding (kernels/nrtr_twopass.h: ccd_nrtr_twopass_rows, ccd_nrtr_twopass_select; ops.ctc_score_paths;
DINO_Finetune.forward_twopass) that run on either backend: the CPU SIMT executor (tests/test_nrtr_twopass_sim.py) and the MI355X
(tests/test_nrtr_twopass_gpu.py).  `device` is where the tensors live.  check_wrapper_refusals launches nothing and runs without a
backend (tests/test_nrtr_twopass_cpu.py).

Oracle: tests/nrtr_twopass_np.py.  Gates:
  * both kernels: every output bit-equal to the numpy specification (integers, and fp32 numbers that are one rounding of an fp64
    expression both sides evaluate in the same order);
  * ops.ctc_score_paths against tests/ctc_lexicon_np.py: |score - oracle| <= 2^-23 |oracle| + 1e-9, the gate tests/ctc_lexicon_checks.py
    grants ops.ctc_lexicon_score against the same oracle (ctc_lexicon_checks.one_rounding), -inf exactly where the oracle says; the
    beam's own score never exceeds the exact one by more than 2^-23 |score|: both are fp64 sums rounded once to fp32, and the beam's sum
    runs over a subset of the alignments;
  * the model: scores within 1e-5 relative of (1 - w) forward_score + w ops.ctc_lexicon_score, the gate
    nrtr_joint_checks.check_joint_scores_are_the_two_exact_scorers derives for the same sum (three fp32 roundings of 6e-8 each, with
    margin); against the joint beam twice that (each side is within the gate of the same exact number)."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_checks as BK
import ctc_lexicon_checks as LK
import nrtr_joint_checks as J
import nrtr_twopass_np as P

TP, SEQ_LEN, T = 32, 26, 25                                # proposals of 32 frames, the decoder's 26 positions, max_seq_len
CLASSES, START, END, PAD, UKN = 92, 91, 91, 92, 90         # AttnConvertor(DICT90, with_unknown): the classifier's classes and the specials
SHAPES = [(B, W) for B in (1, 3, 5) for W in (1, 4, 16)]   # B = 5: a second workgroup with three idle waves
SCORE_GATE = 1e-5


def hand_made():
    """(name, length, the path's first entries, eligible): the slots the rows kernel must treat by rule, in CTC classes (decoder + 1).
    Entries behind the length are junk where given: the kernel reads nothing there."""
    word = lambda n: [1 + (i * 7) % 90 for i in range(n)]                                      # noqa: E731
    return [("unused", -1, [], False),
            ("empty", 0, [], True),
            ("max_seq_len - 1 characters", T - 1, word(T - 1), True),
            ("max_seq_len characters", T, word(T), False),
            ("Tp characters", TP, word(TP), False),
            ("<UKN>", 3, [11, UKN + 1, 12], True),
            ("a class behind the classifier's", 3, [11, CLASSES + 2, 12], False),
            ("a class on <EOS>", 3, [11, END + 1, 12], False),
            ("a class on <PAD>", 2, [PAD + 1, 12], False),
            ("the blank inside a word", 3, [11, 0, 12], False),
            ("padding inside a word", 2, [11, -1], False),
            ("a length behind the path", TP + 8, word(TP), False),
            ("junk behind the length", 2, [11, 12, 9999, -7, 1 << 30], True),
            ("a huge class", 1, [1 << 30], False),
            ("a negative length that is not -1", -5, word(4), False)]


@functools.lru_cache(maxsize=None)
def proposals(B, W, seed=5):
    """Random words of 0..24 characters of the classes 1..91 in every slot, then the hand-made slots over the first slots in flat
    order (as many as B * W holds) -> (paths int32 [B, W, TP], lengths int32 [B, W], [(flat slot, name, eligible)])."""
    rng = np.random.default_rng(seed * 131 + B * 17 + W)
    paths = np.full((B, W, TP), -1, dtype=np.int32)
    lengths = rng.integers(0, T, size=(B, W)).astype(np.int32)
    for b in range(B):
        for k in range(W):
            paths[b, k, :lengths[b, k]] = rng.integers(1, CLASSES, size=lengths[b, k])
    placed = []
    for i, (name, n, head, eligible) in enumerate(hand_made()[:B * W]):
        b, k = divmod(i, W)
        paths[b, k] = -1
        paths[b, k, :len(head)] = head
        lengths[b, k] = n
        placed.append((i, name, eligible))
    return paths, lengths, placed


def strided(device, paths):
    """The [B, W, Tp] view of a [B, W + 1, Tp + 5] buffer filled with junk: sample and slot strides that are not the dense ones."""
    B, W, Tp = paths.shape
    buf = torch.full((B, W + 1, Tp + 5), 12345, dtype=torch.int32)
    buf[:, :W, :Tp] = torch.from_numpy(paths)
    return buf.to(device)[:, :W, :Tp]


def run_rows(device, paths, lengths, **kw):
    from ccd_amd import ops
    seq, targets, subset = ops.nrtr_twopass_rows(strided(device, paths), torch.from_numpy(lengths).to(device), CLASSES, START, END, PAD,
                                                 SEQ_LEN, **kw)
    B, W, _ = paths.shape
    assert seq.dtype == targets.dtype == torch.int64 and subset.dtype == torch.int32
    assert tuple(seq.shape) == (B * W, SEQ_LEN) and tuple(subset.shape) == (B, W) and targets.shape[0] == B * W
    return seq.cpu().numpy(), targets.cpu().numpy(), subset.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the rows kernel
def check_rows(device):
    """seq, targets and subset bit-equal to the specification at every shape; the hand-made slots are (in)eligible as listed; seq is
    AttnConvertor.words2rows of every eligible word and holds no token outside the embedding table."""
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=T, with_unknown=True)
    assert (conv.start_idx, conv.end_idx, conv.padding_idx, conv.unknown_idx, conv.num_classes()) == (START, END, PAD, UKN, CLASSES + 1)
    seen = set()
    for B, W in SHAPES:
        paths, lengths, placed = proposals(B, W)
        for Lmax in (None, 7):
            got = run_rows(device, paths, lengths, **({} if Lmax is None else {"max_labels": Lmax}))
            want = P.rows(paths, lengths, 1, CLASSES, START, END, PAD, SEQ_LEN, 31 if Lmax is None else Lmax)
            for g, w, name in zip(got, want, ("seq", "targets", "subset")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (B, W, Lmax, name)
        seq, targets, subset = run_rows(device, paths, lengths)
        for i, name, eligible in placed:
            assert (subset.reshape(-1)[i] == i) == eligible and (eligible or subset.reshape(-1)[i] == -1), (B, W, name)
            seen.add(name)
        assert seq.min() >= 0 and seq.max() < conv.num_classes()               # every token indexes the embedding table
        assert (seq[:, 0] == START).all()
        words = [[(paths[b, k, :lengths[b, k]] - 1).tolist()] if subset[b, k] >= 0 else [] for b in range(B) for k in range(W)]
        rows, _, _ = conv.words2rows(words)
        assert np.array_equal(seq[subset.reshape(-1) >= 0], rows.numpy())
        bad = seq[subset.reshape(-1) < 0]
        assert (bad[:, 1:] == PAD).all() and (targets[subset.reshape(-1) < 0] == 0).all()
    assert seen == {name for name, _, _, _ in hand_made()}
    # class_offset 0 (the decoder's classes ARE the CTC classes; class 0 stays the blank) and the CTC side alone
    from ccd_amd import ops
    paths, lengths, _ = proposals(3, 4)
    dev_paths, dev_len = torch.from_numpy(paths).to(device), torch.from_numpy(lengths).to(device)
    got = ops.nrtr_twopass_rows(dev_paths, dev_len, CLASSES, START, END, PAD, SEQ_LEN, class_offset=0)
    want = P.rows(paths, lengths, 0, CLASSES, START, END, PAD, SEQ_LEN, 31)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    seq, targets, subset = ops.nrtr_twopass_rows(dev_paths, dev_len, 128, -1, -1, -1, 128, want_seq=False)
    want = P.rows(paths, lengths, 1, 128, -1, -1, -1, 128, 31)
    assert seq is None and np.array_equal(targets.cpu().numpy(), want[1]) and np.array_equal(subset.cpu().numpy(), want[2])


# ------------------------------------------------------------------------------------------------ 2. the select kernel
def select_case(B, W, seed):
    """Proposals with random scores: about a fifth of the slots ineligible by subset, a -inf in either score, a NaN, equal scores."""
    rng = np.random.default_rng(seed)
    paths, lengths, _ = proposals(B, W)
    _, _, subset = P.rows(paths, lengths, 1, CLASSES, START, END, PAD, SEQ_LEN, 31)
    att = (-rng.random((B, W)) * 60).astype(np.float32)
    ctc = (-rng.random((B, W)) * 90).astype(np.float32)
    for scores in (att, ctc):
        scores[rng.random((B, W)) < 0.12] = -np.inf
    att[rng.random((B, W)) < 0.05] = np.nan
    ctc[rng.random((B, W)) < 0.03] = np.inf
    if W >= 4:                                                                 # ties: slots 1 and 3 score as slot 2 does
        att[:, 1] = att[:, 3] = att[:, 2]
        ctc[:, 1] = ctc[:, 3] = ctc[:, 2]
    return paths, lengths, subset, att, ctc


def run_select(device, paths, lengths, subset, att, ctc, w):
    from ccd_amd import ops
    out = ops.nrtr_twopass_select(torch.from_numpy(att.reshape(-1)).to(device), torch.from_numpy(ctc).to(device), strided(device, paths),
                                  torch.from_numpy(lengths).to(device), torch.from_numpy(subset).to(device), w, T)
    B, W, _ = paths.shape
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int32]
    assert tuple(out[0].shape) == (B, W, T) and all(tuple(t.shape) == (B, W) for t in out[1:])
    return [t.cpu().numpy() for t in out]


def assert_select_equal(got, want, where):
    for g, w, name in zip(got, want, ("paths", "lengths", "scores", "att_scores", "ctc_scores", "source")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (where, name, g, w)


def check_select(device):
    """All six outputs bit-equal to the specification at every shape and w in {0, 0.3, 0.5, 1}; ties resolve by slot; a slot with a
    -inf (or NaN, or +inf) in either score is never selected, also where that term's weight is 0; `source` is a permutation of the
    eligible slots; an image without an eligible slot and W = 1."""
    ties = 0
    for B, W in SHAPES:
        for w in (0.0, 0.3, 0.5, 1.0):
            paths, lengths, subset, att, ctc = select_case(B, W, 1000 * B + 10 * W + int(10 * w))
            if B >= 3:
                subset[1] = -1                                                 # an image with no eligible slot
            got = run_select(device, paths, lengths, subset, att, ctc, w)
            assert_select_equal(got, P.select(att, ctc, paths, lengths, subset, w, T, 1), (B, W, w))
            out_paths, out_len, scores, att_s, ctc_s, source = got
            assert not np.isnan(scores).any()
            for b in range(B):
                eligible = [k for k in range(W) if subset[b, k] >= 0 and np.isfinite(att[b, k]) and np.isfinite(ctc[b, k])
                            and 0 <= lengths[b, k] <= T]
                n = len(eligible)
                assert sorted(source[b, :n].tolist()) == eligible and (source[b, n:] == -1).all(), (B, W, w, b)
                assert (out_len[b, n:] == -1).all() and (out_paths[b, n:] == -1).all()
                assert np.isneginf(scores[b, n:]).all() and np.isneginf(att_s[b, n:]).all() and np.isneginf(ctc_s[b, n:]).all()
                assert np.isfinite(scores[b, :n]).all() and (np.diff(scores[b, :n]) <= 0).all()
                for r in range(n):
                    k = source[b, r]
                    assert att_s[b, r] == att[b, k] and ctc_s[b, r] == ctc[b, k] and out_len[b, r] == lengths[b, k]
                    assert np.array_equal(out_paths[b, r, :out_len[b, r]], paths[b, k, :lengths[b, k]] - 1)
                    if w == 0.0:
                        assert scores[b, r] == att[b, k]                       # the attention score itself, not a product
                    if w == 1.0:
                        assert scores[b, r] == ctc[b, k]
                if W >= 4 and all(k in eligible for k in (1, 2, 3)):
                    at = source[b].tolist().index(1)
                    assert source[b, at:at + 3].tolist() == [1, 2, 3], (B, W, w, b)        # equal scores: the slots in order
                    ties += 1
            if B >= 3:
                assert (source[1] == -1).all()
    assert ties >= 4
    # w = 0 with -inf in every CTC score, w = 1 with -inf in every attention score: nothing is eligible, nothing is NaN
    paths, lengths, subset, att, ctc = select_case(3, 4, 77)
    for w, a, c in ((0.0, np.full_like(att, -1.0), np.full_like(ctc, -np.inf)), (1.0, np.full_like(att, -np.inf), np.full_like(ctc, -1.0))):
        got = run_select(device, paths, lengths, subset, a, c, w)
        assert_select_equal(got, P.select(a, c, paths, lengths, subset, w, T, 1), w)
        assert (got[5] == -1).all() and np.isneginf(got[2]).all()


# ------------------------------------------------------------------------------------------------ 3. ops.ctc_score_paths
def check_ctc_score_paths(device):
    """The paths of ops.ctc_beam_search on peaked frames (logits and probabilities) and hand-made slots, against the fp64 oracle."""
    from ccd_amd import ops
    compared = 0
    for seed, normalized, W in ((100, False, 8), (101, True, 16), (102, True, 1)):
        x = BK.peaked(seed, normalized)
        view = LK.frames_view(device, x)
        paths, lengths, beam = ops.ctc_beam_search(view, W, normalized=normalized)
        got = ops.ctc_score_paths(view, paths, lengths, normalized=normalized)
        assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0], W)
        want = P.ctc_score_paths(x, paths.cpu().numpy(), lengths.cpu().numpy(), normalized=normalized)
        g, s, n = got.cpu().numpy(), beam.cpu().numpy(), lengths.cpu().numpy()
        for b in range(x.shape[0]):
            LK.compare_scores(g[b], want[b], (seed, b))
            for k in range(W):
                if n[b, k] >= 0 and np.isfinite(want[b, k]):
                    assert float(s[b, k]) - float(g[b, k]) <= 2.0 ** -23 * abs(float(s[b, k])), (seed, b, k, s[b, k], g[b, k])
                    compared += 1
        # the table and subset of a rows call on the same proposals give the same bytes
        _, targets, subset = ops.nrtr_twopass_rows(paths, lengths, 128, -1, -1, -1, 128, want_seq=False)
        assert torch.equal(ops.ctc_score_paths(view, paths, lengths, normalized=normalized, rows=(targets, subset)), got)
    assert compared >= 100
    x = BK.peaked(100, True, B=3)
    paths, lengths, _ = proposals(3, 16)
    got = ops.ctc_score_paths(LK.frames_view(device, x), strided(device, paths), torch.from_numpy(lengths).to(device), normalized=True)
    want = P.ctc_score_paths(x, paths, lengths, normalized=True)
    for b in range(3):
        LK.compare_scores(got.cpu().numpy()[b], want[b], ("hand-made", b))
    flat = got.cpu().numpy().reshape(-1)
    names = {name: i for i, name, _ in proposals(3, 16)[2]}
    assert all(np.isneginf(flat[names[k]]) for k in ("unused", "Tp characters", "the blank inside a word", "a length behind the path"))
    assert all(np.isfinite(flat[names[k]]) for k in ("empty", "max_seq_len characters", "<UKN>", "junk behind the length"))


# ------------------------------------------------------------------------------------------------ 4. arguments
def check_wrapper_refusals(device="cpu"):
    """Bad dtypes and shapes are refused by the two wrappers and ops.ctc_score_paths before any launch (no backend is needed)."""
    from ccd_amd import ops
    paths, lengths, _ = proposals(3, 4)
    p, n = torch.from_numpy(paths).to(device), torch.from_numpy(lengths).to(device)
    ok = dict(paths=p, lengths=n, classes=CLASSES, start_idx=START, end_idx=END, pad_idx=PAD, seq_len=SEQ_LEN)
    for error, kw in ((TypeError, dict(paths=p.long())), (TypeError, dict(lengths=n.long())), (TypeError, dict(paths=None)),
                      (ValueError, dict(paths=p[0])), (ValueError, dict(paths=p.transpose(1, 2))), (ValueError, dict(lengths=n[:, :3])),
                      (ValueError, dict(lengths=n.t().contiguous().t())), (ValueError, dict(paths=p[:, :0])),
                      (ValueError, dict(paths=torch.zeros(3, 17, TP, dtype=torch.int32, device=device))),
                      (ValueError, dict(paths=torch.zeros(3, 4, 129, dtype=torch.int32, device=device))),
                      (ValueError, dict(classes=0)), (ValueError, dict(classes=129)), (ValueError, dict(seq_len=1)), (ValueError, dict(seq_len=129)),
                      (ValueError, dict(max_labels=0)), (ValueError, dict(max_labels=32)), (ValueError, dict(class_offset=2)),
                      (ValueError, dict(class_offset=True)), (ValueError, dict(end_idx=-1)), (ValueError, dict(pad_idx=65536)),
                      (ValueError, dict(start_idx=-1))):
        with pytest.raises(error, match="nrtr_twopass_rows"):
            ops.nrtr_twopass_rows(**{**ok, **kw})
    att, ctc = torch.zeros(12, device=device), torch.zeros(3, 4, device=device)
    subset = torch.zeros(3, 4, dtype=torch.int32, device=device)
    ok = dict(att=att, ctc=ctc, paths=p, lengths=n, subset=subset, weight=0.5, max_seq_len=T)
    for error, kw in ((TypeError, dict(att=att.double())), (TypeError, dict(ctc=ctc.half())), (TypeError, dict(subset=subset.long())),
                      (TypeError, dict(paths=p.long())), (ValueError, dict(att=att.view(3, 4))), (ValueError, dict(ctc=ctc.view(-1))),
                      (ValueError, dict(att=att[:8])), (ValueError, dict(subset=subset[:2])), (ValueError, dict(ctc=torch.zeros(4, 3, device=device).t())),
                      (ValueError, dict(weight=-0.1)), (ValueError, dict(weight=1.5)), (ValueError, dict(weight=float("nan"))),
                      (ValueError, dict(weight=True)), (ValueError, dict(weight="0.3")), (ValueError, dict(max_seq_len=0)),
                      (ValueError, dict(max_seq_len=129)), (ValueError, dict(class_offset=-1))):
        with pytest.raises(error, match="nrtr_twopass_select"):
            ops.nrtr_twopass_select(**{**ok, **kw})
    frames = torch.zeros(3, 32, 92, device=device)
    for error, args in ((ValueError, (frames[0], p, n)), (ValueError, (frames.transpose(1, 2), p, n)), (ValueError, (frames[:2], p, n)),
                        (TypeError, (frames, p.long(), n)), (ValueError, (frames, p, n[:2]))):
        with pytest.raises(error, match="ctc_score_paths"):
            ops.ctc_score_paths(*args)
    with pytest.raises(ValueError, match="rows must be nrtr_twopass_rows'"):
        ops.ctc_score_paths(frames, p, n, rows=(torch.zeros(12, 40, dtype=torch.int64, device=device), subset))


def check_abi(device):
    """ABI 30; the entry points refuse what the wrappers let through - CCD_EINVAL (-1) / CCD_ESHAPE (-2) - and launch nothing."""
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() == 30 and ops.NRTR_TWOPASS_MAX_PATH == 128
    B, W = 3, 4
    paths, lengths, _ = proposals(B, W)
    p, n = torch.from_numpy(paths).to(device), torch.from_numpy(lengths).to(device)
    seq = torch.full((B * W, SEQ_LEN), 7, dtype=torch.int64, device=device)
    targets = torch.full((B * W, 31), 7, dtype=torch.int64, device=device)
    subset = torch.full((B, W), 7, dtype=torch.int32, device=device)
    st = _lib.stream()
    rows = [p, W * TP, TP, n, B, W, TP, 1, CLASSES, START, END, PAD, seq, SEQ_LEN, targets, 31, subset, st]
    for i, v, code in ((0, None, -1), (3, None, -1), (14, None, -1), (16, None, -1), (1, -1, -1), (2, -1, -1), (4, -1, -1), (5, 0, -2),
                       (5, 17, -2), (6, 0, -2), (6, 129, -2), (7, 2, -2), (7, -1, -2), (8, 0, -2), (8, 129, -2), (9, -1, -2), (9, 65536, -2),
                       (10, -1, -2), (11, -1, -2), (11, 65536, -2), (13, 1, -2), (13, 129, -2), (15, 0, -2), (15, 32, -2)):
        call = list(rows)
        call[i] = v
        assert lib.ccd_nrtr_twopass_rows(*call) == code, (i, v)
    assert int(seq.min()) == int(seq.max()) == 7 and int(targets.min()) == int(targets.max()) == 7 and int(subset.min()) == 7      # untouched
    assert lib.ccd_nrtr_twopass_rows(None, 0, 0, None, 0, W, TP, 1, CLASSES, START, END, PAD, None, SEQ_LEN, None, 31, None, st) == 0
    call = list(rows)
    call[10], call[11], call[12] = -1, -1, None                                # without seq, -1 is "no such class"
    assert lib.ccd_nrtr_twopass_rows(*call) == 0 and int(seq.min()) == 7 and int(subset.min()) == -1
    att, ctc = torch.zeros(B * W, device=device), torch.zeros(B, W, device=device)
    outs = [torch.full((B, W, T), 7, dtype=torch.int32, device=device), torch.full((B, W), 7, dtype=torch.int32, device=device),
            torch.full((B, W), 7.0, device=device), torch.full((B, W), 7.0, device=device), torch.full((B, W), 7.0, device=device),
            torch.full((B, W), 7, dtype=torch.int32, device=device)]
    select = [p, W * TP, TP, n, B, W, TP, 1, att, ctc, subset, 0.5, T] + outs + [st]
    for i, v, code in ([(i, None, -1) for i in (0, 3, 8, 9, 10, 13, 14, 15, 16, 17, 18)] +
                       [(1, -1, -1), (4, -1, -1), (5, 0, -2), (5, 17, -2), (6, 0, -2), (6, 129, -2), (7, 2, -2), (11, -0.01, -2), (11, 1.01, -2),
                        (11, float("nan"), -2), (11, float("inf"), -2), (12, 0, -2), (12, 129, -2)]):
        call = list(select)
        call[i] = v
        assert lib.ccd_nrtr_twopass_select(*call) == code, (i, v)
    assert all(float(t.double().min()) == 7.0 and float(t.double().max()) == 7.0 for t in outs)
    assert lib.ccd_nrtr_twopass_select(*([None, 0, 0, None, 0, W, TP, 1, None, None, None, 0.5, T] + [None] * 6 + [st])) == 0


# ------------------------------------------------------------------------------------------------ 5. the model
def words_of(paths, lengths, b):
    return [paths[b, r, :lengths[b, r]].tolist() for r in range(paths.shape[1]) if lengths[b, r] >= 0]


def check_model(device, B=4, W=8, w=0.3):
    """DINO_Finetune.forward_twopass of nrtr_joint_checks.build_model (vit_tiny, one decoder layer, the <EOS> and blank biases).
    -> (the largest relative difference to the two exact scorers, the words compared with the joint beam)."""
    from ccd_amd import ops
    model = J.build_model(device)
    img = J.model_images(B, device)
    with torch.no_grad():
        out = model.forward_twopass(img, beam=W, ctc_weight=w)
        parts = (model.last_att_scores.clone(), model.last_ctc_scores.clone(), model.last_sources.clone())
        again = model.forward_twopass(img, beam=W, ctc_weight=w)
        probs = model.forward_ctc(img)
        prop = ops.ctc_beam_search(probs, W, normalized=True)
        fed = model.forward_twopass(img, ctc_weight=w, proposals=prop[:2])
        fed_parts = (model.last_att_scores, model.last_ctc_scores, model.last_sources)
        zero = model.forward_twopass(img, beam=W, ctc_weight=0.0)
        zero_sources, zero_att = model.last_sources.cpu().numpy(), model.last_att_scores.clone()
        joint = model.forward_beam(img, W, joint_ctc_weight=w)
    assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, again))                # a second call: the same bytes
    assert all(torch.equal(a, b) for a, b in zip(out, fed)) and all(torch.equal(a, b) for a, b in zip(parts, fed_parts))
    paths, lengths, scores = (t.cpu().numpy() for t in out)
    assert paths.dtype == lengths.dtype == np.int32 and scores.dtype == np.float32
    assert paths.shape == (B, W, T) and lengths.shape == scores.shape == (B, W)
    att, ctc, source = (t.cpu().numpy() for t in parts)
    pp, pn = prop[0].cpu().numpy(), prop[1].cpu().numpy()
    _, _, subset = P.rows(pp, pn, 1, CLASSES, START, END, PAD, SEQ_LEN, 31)
    worst, compared, with_joint = 0.0, 0, 0
    jp, jn, js = (t.cpu().numpy() for t in joint)
    for b in range(B):
        eligible = [k for k in range(W) if subset[b, k] >= 0]
        n = len(eligible)
        assert n >= 1 and sorted(source[b, :n].tolist()) == eligible and (source[b, n:] == -1).all(), (b, source[b], eligible)
        assert (lengths[b, n:] == -1).all() and np.isneginf(scores[b, n:]).all() and (np.diff(scores[b, :n]) <= 0).all()
        words = words_of(paths, lengths, b)
        assert words == [(pp[b, k, :pn[b, k]] - 1).tolist() for k in source[b, :n]]            # the proposals, shifted by the offset
        exact = model.forward_score(img[b:b + 1], [words])["score"].double().cpu().numpy()
        table = torch.zeros((n, max(1, max(len(x) for x in words))), dtype=torch.int64)
        for i, x in enumerate(words):
            table[i, :len(x)] = torch.tensor(x, dtype=torch.int64) + 1
        exact_ctc = ops.ctc_lexicon_score(probs[b:b + 1], ops.ctc_lexicon(table), normalized=True).double().cpu().numpy()[0]
        for r in range(n):
            want = (1 - w) * exact[r] + w * exact_ctc[r]
            worst = max(worst, abs(scores[b, r] - want) / abs(want))
            assert abs(scores[b, r] - want) <= SCORE_GATE * abs(want), (b, r, scores[b, r], want)
            assert abs(att[b, r] - exact[r]) <= SCORE_GATE * abs(exact[r]), (b, r, att[b, r], exact[r])
            assert abs(ctc[b, r] - exact_ctc[r]) <= SCORE_GATE * abs(exact_ctc[r]), (b, r, ctc[b, r], exact_ctc[r])
            compared += 1
        # w = 0: rank 0 is the arg-max of forward_score over the proposals (first of equals; `exact` is in the order of `source`)
        best = max(exact)
        first = min(int(source[b, r]) for r in range(n) if exact[r] == best)
        assert zero_sources[b, 0] == first, (b, zero_sources[b], exact, source[b])
        # where the joint beam finished the same word, the two S agree within twice the gate
        finished = {tuple(jp[b, r, :jn[b, r]].tolist()): float(js[b, r]) for r in range(W) if 0 <= jn[b, r] < T}
        for r, word in enumerate(words):
            if tuple(word) in finished:
                s = finished[tuple(word)]
                assert abs(scores[b, r] - s) <= 2 * SCORE_GATE * abs(s), (b, r, word, scores[b, r], s)
                with_joint += 1
    assert torch.equal(zero[2], zero_att)                                      # w = 0: S is the attention score itself
    print(f"two-pass scores against (1 - w) forward_score + w ctc_lexicon_score: largest relative difference {worst:.3e} over {compared} "
          f"words; {with_joint} words compared with the joint beam")
    return worst, with_joint


def check_model_refusals(device):
    model = J.build_model(device)
    img = J.model_images(1, device)
    for kw, match in ((dict(beam=0), "beam must lie in 1..16"), (dict(beam=17), "beam must lie in 1..16"), (dict(), "decoder.twopass_beam"),
                      (dict(beam=4, ctc_weight=1.5), r"ctc_weight must lie in \[0, 1\]"), (dict(beam=4, ctc_weight=True), "ctc_weight")):
        with pytest.raises(ValueError, match=match):
            model.forward_twopass(img, **kw)
    with pytest.raises(ValueError, match="decoder.aux_ctc_weight"):
        J.build_model(device, aux=None).forward_twopass(img, beam=4)


def build_twopass_model(device, beam, weight=None, seed=2):
    """nrtr_joint_checks.build_model with the two-pass keys set."""
    from ccd_amd import finetune as ft
    torch.manual_seed(seed)
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=1)
    cfg.decoder_aux_ctc_weight, cfg.decoder_twopass_beam = J.AUX, beam
    if weight is not None:
        cfg.decoder_twopass_ctc_weight = weight
    model = ft.build_model(cfg, device).eval()
    with torch.no_grad():
        model.arena.w("decoder.classifier.bias")[91] += J.END_BIAS
        model.arena.w("ctc_decoder.fc.bias")[0] += J.BLANK_BIAS
    model.arena.refresh_mirrors()
    return model


def check_text_accuracy(device, B=3, W=4, batches=3):
    """TextAccuracy.compute on a model configured with decoder.twopass_beam: the totals of update() on the strings of rank 0 of
    paths2nbest on forward_twopass' outputs (the host path), over a few synthetic batches."""
    from ccd_amd.metric.eval_acc import TextAccuracy
    model = build_twopass_model(device, W)
    conv = model.label_convertor
    assert conv.twopass_beam == W and conv.twopass_ctc_weight == 0.5 and conv.beam_width == 0
    loader, host = [], TextAccuracy()
    for i in range(batches):
        img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(40 + i))
        with torch.no_grad():
            out = model.forward_twopass(img.to(device))
            if i == 0:                                                         # the configured defaults are the width and the weight
                assert torch.equal(out[2], model.forward_twopass(img.to(device), beam=W, ctc_weight=0.5)[2])
        nbest = conv.paths2nbest(*out)[0]
        pred = conv.idx2str([words[0] if words else [] for words in nbest])
        truth = [p if (b + i) % 2 == 0 and p else "Abc1" for b, p in enumerate(pred)]
        host.update(truth, pred)
        loader.append((img, (truth,)))
    got, want = TextAccuracy().compute(model, loader), host.result()
    assert want["words"] == batches * B
    assert all(got[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(got["ned"] - want["ned"]) < 1e-12, (got, want)
