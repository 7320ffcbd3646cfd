"""Beam search over the NRTR decoder on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of
tests/test_nrtr_beam_sim.py (gates: tests/nrtr_beam_checks.py), then the model - DINO_Finetune.forward_beam against forward_test at
width 1 and against a teacher-forced rescoring by the uncached decoder at widths 4 and 8, the HIP graph against eager launches, and
TextAccuracy.compute with a beam.

The model is vit_tiny with a 2-layer decoder at its random initialisation.  Such a model barely looks at its input, so the images
carry a strong offset per sample and channel and a column profile (`images`), and END_BIAS is added to the classifier's bias of
<EOS>: 0.5 was chosen from a scan of 0 .. 1.2 as the value at which, over the two batches, some hypotheses finish early and some
run to max_seq_len at every width used here (5 / 16 at width 1, 39 / 45 at width 4, 78 / 90 at width 8).  The tests assert both.

The rescoring gate.  A returned (path, score) is compared with the fp64 log-softmax of the UNCACHED decoder's logits (fe.decoder_states
on the whole sequence, dropout 0, as greedy_decode_full calls it) summed along the path and its <EOS>.  What the two decoders may
differ by was measured on the code before this feature, with this model and these images, as the largest
|sum log p_incremental - sum log p_full| along the greedy paths of greedy_decode against greedy_decode_full (tools/nrtr_beam_bench.py,
case `rescore`; profiles/nrtr_beam.json, "rescore_base"): RESCORE_BASE = 0.0 - the incremental decoder computes every row with the
same kernels in the same order as the full one, and the probabilities along all 21 greedy paths agree bit for bit.  Four times
that is still 0, and the returned score is an fp32: the gate is 4 x RESCORE_BASE plus the one rounding of the fp64 score to fp32,
2^-24 |score| (round to nearest: half an ulp), plus 1e-9 for the fp64 arithmetic of two log-softmax implementations (1e-13 at
|score| ~ 100).  Measured with the feature: the largest difference is 3.8e-6 at |score| ~ 100, where half an fp32 ulp is 3.8e-6."""
import numpy as np
import pytest
import torch

from backends import Backend
import nrtr_beam_checks as K

pytestmark = pytest.mark.gpu

END_IDX, PAD_IDX, T = 91, 92, 25
END_BIAS = 0.5
RESCORE_BASE = 0.0


def rescore_tol(exact):
    return 4 * RESCORE_BASE + 2.0 ** -24 * np.abs(exact) + 1e-9


BATCHES = (5, 16)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_paths_parents_and_scores_equal_the_oracle(hip):
    K.check_oracle(hip.device)


def test_finished_slots_compete_with_live_ones(hip):
    K.check_end_heavy(hip.device)


def test_width_one_is_the_arg_max_chain(hip):
    K.check_width_one_is_greedy(hip.device)


def test_a_wide_beam_equals_brute_force(hip):
    K.check_exhaustive(hip.device)


def test_equal_scores_rank_the_lower_flat_index_first(hip):
    K.check_ties(hip.device)


def test_cache_permutation_is_exact_in_place(hip):
    K.check_reorder(hip.device)


def test_argument_validation(hip):
    K.check_arguments(hip.device)


def test_convertor_nbest_and_path_scoring(hip):
    K.check_convertor(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def build(device, end_bias=END_BIAS, beam_width=None):
    from ccd_amd import finetune as ft
    torch.manual_seed(2)
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2)
    if beam_width is not None:
        cfg.decoder_beam_width = beam_width
    model = ft.build_model(cfg, device).eval()
    with torch.no_grad():
        model.arena.w("decoder.classifier.bias")[END_IDX] += end_bias
    model.arena.refresh_mirrors()
    return model


def images(B, device):
    """(tools/nrtr_beam_bench.py, case `rescore`, builds the same.)"""
    x = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(5 + B))
    g = torch.Generator().manual_seed(50 + B)
    x = x * 0.25 + 2.0 * torch.randn(B, 3, 1, 1, generator=g) + torch.randn(B, 3, 1, 128, generator=g)
    return x.to(device)


@pytest.fixture(scope="module")
def model(hip):
    return build(hip.device)


def greedy_words(probs):
    """forward_test's probabilities [B, 25, 92] -> (arg-max words up to the first <EOS>, sum of log probs along them with the <EOS>)."""
    p = probs.double().cpu().numpy()
    words, scores = [], []
    for b in range(p.shape[0]):
        word, score = [], 0.0
        for t in range(p.shape[1]):
            c = int(np.argmax(p[b, t]))
            score += np.log(p[b, t, c])
            if c == END_IDX:
                break
            word.append(c)
        words.append(word)
        scores.append(score)
    return words, np.asarray(scores)


def rescore(model, img, paths, lengths):
    """Teacher forcing by the uncached decoder: fp64 log-softmax of its logits along every path and its <EOS> -> [B, W] (nan for an
    unused slot)."""
    from ccd_amd import finetune_engine as fe, ops
    dec = model.decoder
    B, W, _ = paths.shape
    with torch.no_grad():
        feat = model.extract_feat(img)
        out_enc = model.encoder(feat).to(torch.bfloat16)
        dec._ready()
        arena, pre, spec, packed = dec.arena, dec.arena_prefix, dec.dec_spec, dec.packed
        packed.refresh(arena, pre, spec)
        kv = fe.encoder_kv(arena, pre, spec, out_enc.repeat_interleave(W, 0).reshape(-1, spec.D))
        p, n = paths.cpu().numpy(), lengths.cpu().numpy()
        seq = np.full((B * W, T + 1), PAD_IDX, dtype=np.int64)
        seq[:, 0] = END_IDX
        for b in range(B):
            for r in range(W):
                if n[b, r] >= 0:
                    seq[b * W + r, 1:1 + n[b, r]] = p[b, r, :n[b, r]]
                    if n[b, r] < T:
                        seq[b * W + r, 1 + n[b, r]] = END_IDX
        seq_d = torch.from_numpy(seq).to(img.device)
        y, _, _ = fe.decoder_states(arena, pre, spec, dec.pos_table, seq_d, kv, 0.0, fe._Seeds(0), False, want_attn=False)
        logits = ops.gemm_nt(y, packed.cls, epilogue=ops.EPI_F32, bias=packed.cls_bias)
        lp = torch.log_softmax(logits[:, :spec.C].double(), dim=-1).view(B * W, T + 1, spec.C).cpu().numpy()
    out = np.full((B, W), np.nan)
    for b in range(B):
        for r in range(W):
            if n[b, r] >= 0:
                row = b * W + r
                steps = min(n[b, r] + 1, T)
                out[b, r] = sum(lp[row, t, seq[row, t + 1]] for t in range(steps))
    return out


def test_width_one_is_forward_test(model, hip):
    finished = 0
    for B in BATCHES:
        img = images(B, hip.device)
        with torch.no_grad():
            probs = model.forward_test(img)
            paths, lengths, scores = model.forward_beam(img, 1)
        assert tuple(paths.shape) == (B, 1, T) and paths.dtype == torch.int32 and scores.dtype == torch.float32
        words, want = greedy_words(probs)
        got = model.label_convertor.paths2nbest(paths, lengths, scores)[0]
        assert [w[0] for w in got] == words
        err = np.abs(scores[:, 0].double().cpu().numpy() - want).max()
        print(f"B = {B}: width 1 against forward_test, largest score difference {err:.3e}")
        assert err <= 1e-3
        finished += sum(len(w) < T for w in words)
    assert 0 < finished < sum(BATCHES)                                         # some words end early, some run to max_seq_len


@pytest.mark.parametrize("W", [4, 8])
def test_beam_agrees_with_teacher_forced_rescoring(model, hip, W):
    worst, early, full, within = 0.0, 0, 0, True
    for B in BATCHES:
        img = images(B, hip.device)
        with torch.no_grad():
            paths, lengths, scores = model.forward_beam(img, W)
        p, n, s = paths.cpu().numpy(), lengths.cpu().numpy(), scores.double().cpu().numpy()
        assert (n >= 0).all() and np.isfinite(s).all()                         # 92 classes fill any beam at step 0
        assert (np.diff(s, axis=1) <= 0).all()                                 # by rank
        for b in range(B):
            words = [tuple(p[b, r, :n[b, r]].tolist()) for r in range(W)]
            assert len(set(words)) == W, (b, words)
            for r in range(W):
                assert (p[b, r, n[b, r]:] == -1).all() and (p[b, r, :n[b, r]] >= 0).all() and not (p[b, r, :n[b, r]] == END_IDX).any()
        again = rescore(model, img, paths, lengths)
        worst = max(worst, float(np.abs(again - s).max()))
        within = within and bool((np.abs(again - s) <= rescore_tol(again)).all())
        early += int((n < T).sum())
        full += int((n == T).sum())
    print(f"W = {W}: largest |beam score - teacher-forced score| {worst:.3e} (gate {float(rescore_tol(100.0)):.3e} at |score| = 100); "
          f"{early} finished, {full} at max_seq_len")
    assert early > 0 and full > 0
    assert within


def test_beam_hip_graph_matches_eager(hip, monkeypatch):
    """forward_beam replays its steps from a captured HIP graph: identical to issuing the kernels one by one, also after the weights
    changed in place and for a second batch size; every width has a graph of its own."""
    model = build(hip.device)
    for B in (16, 16, 5):
        img = images(B, hip.device)
        for W in (4, 8):
            with torch.no_grad():
                monkeypatch.setenv("CCD_DECODE_GRAPH", "1")
                graphed = model.forward_beam(img, W)
                monkeypatch.setenv("CCD_DECODE_GRAPH", "0")
                eager = model.forward_beam(img, W)
            assert all(torch.equal(a, b) for a, b in zip(graphed, eager)), (B, W)
        with torch.no_grad():
            model.arena.flat.mul_(1.01)
        model.arena.refresh_mirrors()
    assert len(model.decoder._beam_graphs) == 4 and {k[-1] for k in model.decoder._beam_graphs} == {4, 8}
    assert len(model.decoder._graphs) == 0


def _loader(B, device):
    gen = torch.Generator().manual_seed(4)
    imgs = [torch.randn(B, 3, 32, 128, generator=gen) for _ in range(2)]
    return imgs


def test_text_accuracy_scores_the_best_word_of_the_beam(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    model = build(hip.device, beam_width=4)
    conv = model.label_convertor
    assert conv.beam_width == 4 and model.decoder.beam_width == 4
    imgs = _loader(6, hip.device)
    decoded = []
    with torch.no_grad():
        for img in imgs:
            best = [w[0] for w in conv.paths2nbest(*model.forward_beam(img.to(hip.device)), nbest=1)[0]]
            decoded.append(conv.idx2str(best))
    truth = [decoded[0], [s[:-1] + "Q" if b % 2 else s for b, s in enumerate(decoded[1])]]
    loader = [(img, (gt,)) for img, gt in zip(imgs, truth)]
    host = TextAccuracy()
    for gt, pt in zip(truth, decoded):
        host.update(gt, pt)
    metric = TextAccuracy()
    res, want = metric.compute(model, loader), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12
    assert res["words"] == 12.0 and metric._totals is not None                 # (the device path ran)
    # beam_width = 0: today's result - the records of ops.text_score on forward_test's probabilities
    from ccd_amd import ops
    from ccd_amd.metric.eval_acc import encode_truth
    conv.beam_width = 0
    greedy = TextAccuracy()
    greedy.compute(model, loader)
    totals = ops.text_totals(hip.device)
    raw, norm = (torch.from_numpy(t).to(hip.device) for t in conv.score_table())
    with torch.no_grad():
        for img, gt in zip(imgs, truth):
            codes, lens = (torch.from_numpy(a).to(hip.device) for a in encode_truth(gt))
            probs = model(img.to(hip.device), text=None, return_loss=False, test_speed=False).float()
            ops.text_accumulate(ops.text_score(probs, raw, norm, conv.end_idx, conv.padding_idx, codes, lens), totals)
    assert torch.equal(greedy._totals, totals)


def test_scoring_the_beam_does_not_synchronise(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    model = build(hip.device, beam_width=4)
    img = images(5, hip.device)
    with torch.no_grad():
        model.forward_beam(img)                                                # (capture the graph outside the guarded region)
        metric = TextAccuracy()
        metric.update_paths(model.forward_beam(img)[0][:, 0], ["a"] * 5, model.label_convertor)      # tables and totals in place
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            paths, _, _ = model.forward_beam(img)
            metric.update_paths(paths[:, 0], ["ab", "c", "", "d", "e"], model.label_convertor)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert metric.result()["words"] == 10.0


def test_absent_beam_width_is_todays_model(hip):
    """An NRTR configuration without decoder.beam_width: forward_test as before, nothing of the beam is allocated."""
    plain = build(hip.device)
    assert plain.label_convertor.beam_width == 0 and plain.decoder.beam_width == 0
    wide = build(hip.device, beam_width=8)
    img = images(5, hip.device)
    with torch.no_grad():
        a, b = plain.forward_test(img), wide.forward_test(img)
        c = plain(img, None, return_loss=False)
    assert torch.equal(a, b) and torch.equal(a, c) and tuple(a.shape) == (5, T, 92)
    assert len(plain.decoder._beam_graphs) == 0 and len(wide.decoder._beam_graphs) == 0 and len(plain.decoder._graphs) == 1
    with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
        plain.forward_beam(img)
