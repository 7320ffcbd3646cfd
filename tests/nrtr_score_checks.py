"""The checks of scoring given words with the NRTR decoder (kernels/nrtr_score.h: ccd_xattn_rows_fwd, ccd_nrtr_word_score) that run on
either backend: the CPU SIMT executor (tests/test_nrtr_score_sim.py) and the MI355X (tests/test_nrtr_score_gpu.py).  `device` is where
the tensors live.

Gates:
  * rows attention: `out` is torch.equal to ops.dec_attn_fwd on K / V gathered per row - the arithmetic of a row is that kernel's;
  * moments: ops.dec_attn_fwd(want_probs=True) on the gathered inputs returns the fp32 probabilities the new kernel holds in registers.
    Their fp64 moments M bound the kernel's fp32 sums by 256 * 2^-24 * M + 1e-12: 256 non-negative terms, each rounded once as a
    product and at most 255 times inside partial sums.  (The kernel's tree is 23 roundings deep - nrtr_score.h - so it sits well
    inside; the gate stays the plain loop's.)  A one-hot map (one key with a score 512 above the rest: exp2(-738) is 0 in fp32) gives
    the key's coordinates exactly and std 0;
  * word scores: char_logp within 1e-6 of tests/nrtr_score_np.py (one fp32 rounding of a number below 16 in magnitude: 2^-24 * 16 =
    9.5e-7), score within 2^-24 |score| + 1e-9 (tests/test_nrtr_beam_gpu.py: rescore_tol with RESCORE_BASE = 0), length exact."""
import numpy as np
import pytest
import torch

import nrtr_score_np as S

BF16 = torch.bfloat16
SCALE = 64 ** -0.5


def rescore_tol(exact):
    return 2.0 ** -24 * np.abs(exact) + 1e-9


def rows_case(H):
    """The smallest row count at which a chunk holds two rows on this backend -> (counts per sample, CH): an empty sample, a
    single-row sample, a sample one row longer than a chunk (the row loop and the chunk seam), and the rest."""
    from ccd_amd import ops
    R = 8
    while ops.xattn_rows_chunk(R, H) < 2:
        R += 1
    CH = ops.xattn_rows_chunk(R, H)
    assert CH == 2 and R - (CH + 2) >= 1
    return [0, 1, CH + 1, R - (CH + 2)], CH


def _inputs(counts, H, Tq, seed):
    """q as the middle columns of a wider buffer, k | v as the column halves of one buffer (encoder_kv's layout)."""
    gen = torch.Generator().manual_seed(seed)
    B, R, D = len(counts), sum(counts), 64 * H
    qbuf = torch.randn(R * Tq, 3 * D, generator=gen).to(BF16)
    kv = torch.randn(B * 256, 2 * D, generator=gen).to(BF16)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    owner = torch.from_numpy(np.repeat(np.arange(B), counts))
    return qbuf, kv, ptr, owner


def _replicated(q, kv, owner, B, H, Tq, want_probs):
    """ops.dec_attn_fwd on K / V gathered per row: the yardstick."""
    from ccd_amd import ops
    D = 64 * H
    rep = kv.view(B, 256, 2 * D)[owner.to(kv.device)].reshape(-1, 2 * D)
    out, _, probs = ops.dec_attn_fwd(q, rep[:, :D], rep[:, D:], len(owner), H, Tq, 256, SCALE, want_probs=want_probs)
    return out, probs


_CASES = {}


def rows_results(device, Tq):
    """One run of both kernels per (backend, Tq), shared by the checks below and left unchanged."""
    from ccd_amd import ops
    key = (str(device), Tq)
    if key not in _CASES:
        H = 2
        counts, CH = rows_case(H)
        qbuf, kv, ptr, owner = _inputs(counts, H, Tq, seed=10 + Tq)
        qbuf, kv = qbuf.to(device), kv.to(device)
        D = 64 * H
        q = qbuf[:, D:2 * D]
        out, mom = ops.xattn_rows_fwd(q, kv[:, :D], kv[:, D:], ptr, H, Tq, SCALE, want_moments=True)
        plain, none = ops.xattn_rows_fwd(q, kv[:, :D], kv[:, D:], ops.csr_rows(ptr), H, Tq, SCALE)
        want, probs = _replicated(q, kv, owner, len(counts), H, Tq, True)
        _CASES[key] = dict(H=H, counts=counts, CH=CH, ptr=ptr, q=q, kv=kv, out=out, mom=mom, plain=plain, none=none, want=want, probs=probs)
    return _CASES[key]


def check_rows_equal_replicated(device, Tq):
    from ccd_amd import _lib, ops
    c = rows_results(device, Tq)
    R, H, D = sum(c["counts"]), c["H"], 64 * c["H"]
    assert c["out"].dtype == BF16 and tuple(c["out"].shape) == (R * Tq, D) and c["none"] is None
    assert torch.equal(c["out"].view(torch.int16), c["want"].view(torch.int16))
    assert torch.equal(c["plain"].view(torch.int16), c["want"].view(torch.int16))           # the moments change nothing
    # the grid does not matter: one chunk slot per (sample, head) - every workgroup walks all of its sample's chunks - and one too many
    for max_rows in (1, R):
        out = torch.zeros_like(c["out"])
        rc = _lib.get().ccd_xattn_rows_fwd(c["q"], c["q"].stride(0), c["kv"][:, :D], 2 * D, c["kv"][:, D:], 2 * D,
                                           torch.from_numpy(c["ptr"]).to(device), out, D, None, R, len(c["counts"]), H, Tq, max_rows, SCALE,
                                           _lib.stream())
        assert rc == 0 and torch.equal(out.view(torch.int16), c["want"].view(torch.int16)), max_rows


def check_moments(device, Tq):
    c = rows_results(device, Tq)
    R, H = sum(c["counts"]), c["H"]
    assert c["mom"].dtype == torch.float32 and tuple(c["mom"].shape) == (R, H, Tq, 4)
    want = S.moments_of(c["probs"].double().cpu().numpy())
    got = c["mom"].double().cpu().numpy()
    err, gate = np.abs(got - want), 256 * 2.0 ** -24 * want + 1e-12
    print(f"Tq = {Tq}: largest moment error / gate = {(err / gate).max():.3f} (relative error {(err / np.maximum(want, 1e-30)).max():.2e})")
    assert (err <= gate).all()


def check_one_hot(device):
    """Every query of sample b looks at one key alone, in both heads: the moments are its coordinates and their squares, exactly, and
    ops.nrtr_word_score turns them into that position with std 0."""
    from ccd_amd import ops
    H, T, keys = 2, 7, (37, 255, 0)
    B, D = len(keys), 128
    k = torch.zeros(B * 256, D)
    for b, j in enumerate(keys):
        k[b * 256 + j] = 8.0
    v = torch.randn(B * 256, D, generator=torch.Generator().manual_seed(3))
    counts = [2, 1, 1]
    R = sum(counts)
    q = torch.full((R * T, D), 8.0)
    q, k, v = (t.to(BF16).to(device) for t in (q, k, v))
    out, mom = ops.xattn_rows_fwd(q, k, v, np.array([0, 2, 3, 4]), H, T, SCALE, want_moments=True)
    owner = [0, 0, 1, 2]
    for r in range(R):
        j = keys[owner[r]]
        x, y = float(j & 31), float(j >> 5)
        assert torch.equal(mom[r].cpu(), torch.tensor([x, y, x * x, y * y]).expand(H, T, 4)), r
        want = v[owner[r] * 256 + j].float().cpu().expand(T, D)                              # P is the one-hot row: out = V[j]
        assert torch.equal(out[r * T:(r + 1) * T].float().cpu(), want), r
    C = 9
    seq = torch.full((R, T), C, dtype=torch.int64)
    seq[:, 0] = C - 1
    seq[:, 1:3] = 4
    seq[:, 3] = C - 1
    logits = torch.zeros(R * T, C)
    _, _, length, pos = ops.nrtr_word_score(logits.to(device), C, seq.to(device), C - 1, C, moments=mom, H=H)
    assert length.tolist() == [2] * R
    for r in range(R):
        j = keys[owner[r]]
        assert torch.equal(pos[r, :3].cpu(), torch.tensor([float(j & 31), float(j >> 5), 0.0, 0.0]).expand(3, 4)), r
        assert not pos[r, 3:].any()


# ------------------------------------------------------------------------------------------------ word scores
C_WS, T_WS, LD_WS, END, PAD = 92, 7, 128, 91, 92


def word_rows():
    """Six rows of T = 7: a word with junk behind its <EOS>, the empty word, a word of T - 2 characters, and one infeasible row of
    each kind - no <EOS>, a class >= C, <PAD> among the characters."""
    seq = np.full((6, T_WS), PAD, dtype=np.int64)
    seq[:, 0] = END
    seq[0, 1:6] = [5, 0, 90, END, 200]
    seq[1, 1] = END
    seq[2, 1:7] = [1, 2, 3, 4, 5, END]
    seq[3, 1:7] = [1, 2, 3, 4, 5, 6]
    seq[4, 1:4] = [7, 100, END]
    seq[5, 1:4] = [7, PAD, END]
    return seq


def check_word_scores(device):
    from ccd_amd import ops
    seq = word_rows()
    R, H = len(seq), 2
    gen = torch.Generator().manual_seed(7)
    logits = torch.full((R * T_WS, LD_WS), float("nan"))
    logits[:, :C_WS] = 4.0 * torch.randn(R * T_WS, C_WS, generator=gen)
    probs = torch.softmax(3.0 * torch.randn(R, H, T_WS, 256, generator=gen), dim=-1)
    moments = torch.from_numpy(S.moments_of(probs.numpy())).float()
    want_lp, want_score, want_len, want_pos = S.word_score(logits.numpy(), C_WS, seq, END, PAD, moments.numpy())
    assert want_len.tolist() == [3, 0, 5, -1, -1, -1]
    seq_d = torch.from_numpy(seq).to(device)
    lp, score, length, pos = ops.nrtr_word_score(logits.to(device), C_WS, seq_d, END, PAD, moments=moments.to(device), H=H)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (R, T_WS - 1) and score.dtype == torch.float32 and tuple(score.shape) == (R,)
    assert length.dtype == torch.int32 and tuple(pos.shape) == (R, T_WS - 1, 4)
    assert length.tolist() == want_len.tolist()
    lp, score, pos = lp.double().cpu().numpy(), score.double().cpu().numpy(), pos.double().cpu().numpy()
    print(f"largest |char_logp - numpy| {np.abs(lp - want_lp).max():.3e}, scores {score[:3]} against {want_score[:3]}")
    assert np.abs(lp - want_lp).max() <= 1e-6
    assert np.isneginf(score[3:]).all() and not lp[3:].any() and not pos[3:].any()           # -inf, -1 and zeros
    assert (np.abs(score[:3] - want_score[:3]) <= rescore_tol(want_score[:3])).all()
    assert score[1] == np.float32(want_lp[1, 0]) and not lp[1, 1:].any()                     # the empty word: the first position's <EOS>
    assert (np.abs(pos - want_pos) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want_pos))).all()
    for r in range(3):
        assert not pos[r, want_len[r] + 1:].any() and pos[r, :want_len[r] + 1, 2:].min() > 0
    # without moments there is no char_pos, and the rest is the same bits; a class that equals a pad_idx inside [0, C) is refused too
    lp2, score2, length2, none = ops.nrtr_word_score(logits.to(device), C_WS, seq_d, END, PAD)
    assert none is None and torch.equal(score2.cpu().double(), torch.from_numpy(score)) and torch.equal(length2, length)
    _, score3, length3, _ = ops.nrtr_word_score(logits.to(device), C_WS, seq_d, END, 90)
    assert length3.tolist() == [-1, 0, 5, -1, -1, -1] and np.isneginf(float(score3[0])) and float(score3[2]) == float(score2[2])


# ------------------------------------------------------------------------------------------------ arguments
def check_arguments(device):
    from ccd_amd import _lib, ops
    lib, st = _lib.get(), _lib.stream()
    assert lib.ccd_abi_version() >= 28
    H, Tq, D = 2, 5, 128
    ptr = [0, 2, 2, 3]
    q = torch.zeros(3 * Tq, D, dtype=BF16, device=device)
    kv = torch.zeros(3 * 256, 2 * D, dtype=BF16, device=device)
    ok = dict(q=q, k=kv[:, :D], v=kv[:, D:], row_ptr=ptr, H=H, Tq=Tq, scale=SCALE)
    for kw, err in ((dict(Tq=0), ValueError), (dict(Tq=33), ValueError), (dict(row_ptr=[0, 2, 1, 3]), ValueError),
                    (dict(row_ptr=[0, 2, 2, 4]), ValueError), (dict(row_ptr=[0, 1, 2]), ValueError), (dict(row_ptr=[1, 2, 2, 3]), ValueError),
                    (dict(row_ptr=[0, 2, 2]), ValueError), (dict(row_ptr=[0.0, 2.0, 3.0]), TypeError), (dict(q=q.float()), TypeError),
                    (dict(k=kv[:, :D].float()), TypeError), (dict(v=kv[:, D:].half()), TypeError), (dict(q=q[:, :64]), ValueError),
                    (dict(k=kv[:256, :D]), ValueError), (dict(q=q.view(3, Tq, D)), ValueError), (dict(H=0), ValueError)):
        with pytest.raises(err, match="xattn_rows_fwd|csr_rows"):
            ops.xattn_rows_fwd(**{**ok, **kw})
    if device.type != "cpu":
        with pytest.raises(TypeError, match="host integers"):
            ops.xattn_rows_fwd(**{**ok, "row_ptr": torch.tensor(ptr, dtype=torch.int32, device=device)})
    out, mom = ops.xattn_rows_fwd(**ok, want_moments=True)
    assert tuple(out.shape) == (3 * Tq, D) and tuple(mom.shape) == (3, H, Tq, 4)
    # empty R, empty B: empty outputs, nothing launched (null pointers reach no kernel)
    out, mom = ops.xattn_rows_fwd(q[:0], kv[:, :D], kv[:, D:], [0, 0, 0, 0], H, Tq, SCALE, want_moments=True)
    assert tuple(out.shape) == (0, D) and tuple(mom.shape) == (0, H, Tq, 4)
    out, mom = ops.xattn_rows_fwd(q[:0], kv[:0, :D], kv[:0, D:], [0], H, Tq, SCALE)
    assert tuple(out.shape) == (0, D) and mom is None
    assert lib.ccd_xattn_rows_fwd(None, D, None, D, None, D, None, None, D, None, 0, 3, H, Tq, 0, SCALE, st) == 0
    assert lib.ccd_xattn_rows_fwd(None, D, None, D, None, D, None, None, D, None, 3, 0, H, Tq, 0, SCALE, st) == 0
    dptr = torch.tensor(ptr, dtype=torch.int32).to(device)
    res = torch.full((3 * Tq, D), 7.0, dtype=BF16, device=device)
    args = [q, D, kv[:, :D], 2 * D, kv[:, D:], 2 * D, dptr, res, D, None, 3, 3, H, Tq, 2, SCALE, st]
    for i, v, code in ((0, None, -1), (2, None, -1), (4, None, -1), (6, None, -1), (7, None, -1), (10, -1, -1), (11, -1, -1), (12, 0, -1),
                       (14, 4, -1), (14, -1, -1), (13, 0, -2), (13, 33, -2), (1, D + 4, -2), (3, 64, -2), (8, 100, -2)):
        call = list(args)
        call[i] = v
        assert lib.ccd_xattn_rows_fwd(*call) == code, (i, v)
    assert bool((res == 7.0).all())                                                          # nothing ran
    assert lib.ccd_xattn_rows_chunk(-1, 2) < 0 and lib.ccd_xattn_rows_chunk(5, 0) < 0 and ops.xattn_rows_chunk(0, 8) == 1
    assert ops.xattn_rows_chunk(10 ** 6, 8) > ops.xattn_rows_chunk(10 ** 5, 8) >= 1

    C, T, R = 12, 6, 3
    seq = torch.full((R, T), C, dtype=torch.int64, device=device)
    seq[:, 0], seq[:, 1] = C - 1, C - 1
    logits = torch.zeros(R * T, C + 4, device=device)
    mom = torch.zeros(R, H, T, 4, device=device)
    ok = dict(logits=logits, C=C, seq=seq, end_idx=C - 1, pad_idx=C)
    for kw, err in ((dict(seq=seq.int()), TypeError), (dict(logits=logits.double()), TypeError), (dict(seq=seq.view(-1)), ValueError),
                    (dict(seq=seq.t()), ValueError), (dict(logits=logits[:-1]), ValueError), (dict(logits=logits[:, :C - 1]), ValueError),
                    (dict(C=0), ValueError), (dict(C=129), ValueError), (dict(end_idx=C), ValueError), (dict(end_idx=-1), ValueError),
                    (dict(moments=mom), ValueError), (dict(moments=mom, H=3), ValueError), (dict(moments=mom[:, :, :-1], H=H), ValueError),
                    (dict(moments=mom.double(), H=H), TypeError), (dict(seq=seq[:, :1]), ValueError)):
        with pytest.raises(err, match="nrtr_word_score"):
            ops.nrtr_word_score(**{**ok, **kw})
    lp, score, length, pos = ops.nrtr_word_score(logits[:0], C, seq[:0], C - 1, C, moments=mom[:0], H=H)
    assert tuple(lp.shape) == (0, T - 1) and tuple(score.shape) == (0,) and tuple(length.shape) == (0,) and tuple(pos.shape) == (0, T - 1, 4)
    lp = torch.full((R, T - 1), 7.0, device=device)
    sc, ln, cp = torch.zeros(R, device=device), torch.zeros(R, dtype=torch.int32, device=device), torch.zeros(R, T - 1, 4, device=device)
    args = [logits, C + 4, C, seq, R, T, C - 1, C, None, 0, lp, sc, ln, None, st]
    for i, v, code in ((0, None, -1), (3, None, -1), (10, None, -1), (11, None, -1), (12, None, -1), (4, -1, -1), (8, mom, -1), (13, cp, -1),
                       (2, 0, -2), (2, 129, -2), (1, C - 1, -2), (5, 1, -2), (5, 129, -2), (6, C, -2), (6, -1, -2)):
        call = list(args)
        call[i] = v
        assert lib.ccd_nrtr_word_score(*call) == code, (i, v)
    call = list(args)
    call[8], call[13] = mom, cp                                                               # moments with 0 heads
    assert lib.ccd_nrtr_word_score(*call) == -2
    assert bool((lp == 7.0).all())                                                            # nothing ran
    assert lib.ccd_nrtr_word_score(None, C, C, None, 0, T, C - 1, C, None, 0, None, None, None, None, st) == 0
    _, score, length, _ = ops.nrtr_word_score(**ok)
    assert length.tolist() == [0] * R and torch.allclose(score.cpu(), torch.full((R,), -float(np.log(C))), atol=1e-6)


# ------------------------------------------------------------------------------------------------ the decoder end to end
def check_decoder_end_to_end(device):
    """A 1-layer decoder of 6 steps, B = 2 (tests/test_nrtr_trie_sim.py builds the same): the three hypotheses of forward_beam per
    sample, fed back through forward_score in another order, score what the beam gave them - the incremental decoder and the
    teacher-forced pass run the same kernels on the same rows, and the rows attention is bit-equal to the attention the beam used -
    and scores2words, forward_words' second half, returns them in the beam's order."""
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.decoder.nrtr_decoder import NRTRDecoder
    torch.manual_seed(2)
    dec = NRTRDecoder(n_layers=1, max_seq_len=6, num_classes=93, start_idx=91, padding_idx=92).eval().to(device)
    with torch.no_grad():
        dec.classifier.bias[91] += 1.5                                         # (the hypotheses finish within the six steps)
    out_enc = torch.randn(2, 256, 512, generator=torch.Generator().manual_seed(1)).to(device)
    with torch.no_grad():
        paths, lengths, scores = dec.forward_beam(None, out_enc, 3)
    assert int(lengths.min()) >= 0 and int(lengths.max()) < 6
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=6, with_unknown=True)
    order = (2, 0, 1)                                                          # list position k holds the beam's rank order[k]
    words = [[paths[b, r, :lengths[b, r]].tolist() for r in order] for b in range(2)]
    assert any(len(w) == 0 for w in words[0])                                  # the empty word is among them
    seq, row_ptr, rows = conv.words2rows(words)
    assert tuple(seq.shape) == (6, 7) and row_ptr.tolist() == [0, 3, 6] and rows == conv.idx2str(words[0] + words[1])
    with torch.no_grad():
        res = dec.forward_score(None, out_enc, seq, row_ptr)
    assert res["length"].tolist() == [len(w) for w in words[0] + words[1]] and res["row_ptr"].tolist() == [0, 3, 6]
    got = res["score"].double().cpu().numpy().reshape(2, 3)
    want = scores.double().cpu().numpy()[:, list(order)]
    print(f"forward_score against the beam: largest difference {np.abs(got - want).max():.3e}, bit-equal: {bool((got == want).all())}")
    assert (np.abs(got - want) <= rescore_tol(want)).all()
    pos = res["char_pos"].cpu().numpy()
    assert (pos[..., 0] >= 0).all() and (pos[..., 0] <= 31).all() and (pos[..., 1] >= 0).all() and (pos[..., 1] <= 7).all()
    index, best = conv.scores2words(res["score"], row_ptr, nbest=3)
    assert index.tolist() == [[1, 2, 0]] * 2                                   # rank 0 sits at list position 1, ..
    assert torch.equal(best, res["score"].view(2, 3)[:, [1, 2, 0]])
    assert len(dec._graphs) == 0 and len(dec._beam_graphs) == 0 or device.type != "cpu"


def check_best_of_lists(device):
    """AttnConvertor.scores2words against tests/nrtr_score_np.py: lists of different lengths (one empty, one of nothing but infeasible
    words), ties - the lower index first - and -inf never selected; the slots left over are (-1, -inf)."""
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(max_seq_len=25)
    ninf = float("-inf")
    lists = [[-3.0, -1.0, -1.0, ninf, -2.0], [], [ninf, ninf], [-5.0], [-2.0, -2.0, -2.0, -2.0]]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    score = torch.tensor([v for s in lists for v in s], dtype=torch.float32).to(device)
    for nbest in (1, 3):
        index, best = conv.scores2words(score, torch.from_numpy(ptr), nbest=nbest)
        want_index, want_best = S.best_of_lists(score.cpu().numpy(), ptr, nbest)
        assert index.dtype == torch.int32 and tuple(index.shape) == (5, nbest) and best.dtype == torch.float32
        assert index.cpu().tolist() == want_index.tolist() and np.array_equal(best.cpu().numpy().astype(np.float64), want_best)
    assert index.cpu().tolist() == [[1, 2, 4], [-1, -1, -1], [-1, -1, -1], [0, -1, -1], [0, 1, 2]]
    index, best = conv.scores2words(score[:0], [0, 0, 0], nbest=2)                          # no words at all
    assert index.cpu().tolist() == [[-1, -1]] * 2 and bool(torch.isneginf(best).all())
    with pytest.raises(ValueError, match="scores2words"):
        conv.scores2words(score[:-1], ptr)
    with pytest.raises(ValueError, match="nbest must lie in"):
        conv.scores2words(score, ptr, nbest=17)
