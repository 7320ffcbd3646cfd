"""The checks of joint CTC / attention decoding (kernels/nrtr_joint.h: ccd_nrtr_joint_begin, ccd_nrtr_beam_step_joint) that run on
either backend: the CPU SIMT executor (tests/test_nrtr_joint_sim.py) and the MI355X (tests/test_nrtr_joint_gpu.py).  `device` is
where the tensors live.

Oracle: tests/nrtr_joint_np.py, the specification in fp64 numpy, itself checked against the enumeration of all alignments and brute
force in tests/test_nrtr_joint_cpu.py.  As in tests/nrtr_beam_checks.py the logits of a step come from a random Markov table gathered
with torch, NaN in the rows of slots that are not live and behind column C; the frames are 2 * standard_normal with 5 added to the
blank logit and NaN behind column Cc in a padded row stride.
Gates (those of nrtr_beam_checks):
  * paths, lengths and the parents of every step equal the oracle's - on samples where the oracle's smallest gap between
    neighbouring candidates is >= 1e-9; at most 2 % of the samples may miss that;
  * |score - oracle| <= 1e-6 |oracle| for scores and att_scores (the one rounding to fp32 is 6e-8)."""
import functools

import numpy as np
import pytest
import torch

import nrtr_beam_checks as K
import nrtr_beam_np as R
import nrtr_joint_np as J

LD_PAD = K.LD_PAD
SEED = 7


def device_frames(device, frames, Cc, normalized):
    """numpy fp32 [B, Tc, Cc + pad] (NaN behind Cc) -> (what the oracle reads [B, Tc, Cc], the strided device view [B, Tc, Cc])."""
    f = torch.from_numpy(frames)
    if normalized:
        f = f.clone()
        f[:, :, :Cc] = torch.softmax(f[:, :, :Cc], dim=-1)
    return f[:, :, :Cc].numpy().copy(), f.to(device)[:, :, :Cc]


def drive(device, tab, frames, W, weight, class_offset=1, normalized=False, plain=False):
    """tab fp32 [B, T, C + 1, C], frames a device view fp32 [B, Tc, Cc] -> (paths [B, W, T], lengths [B, W], scores [B, W], att_scores
    [B, W], parents [B, T, W], prefix [B, W, 2, Tc]) as numpy: ops.nrtr_joint_state, then T calls of ops.nrtr_beam_step_joint.
    plain=True drives ops.nrtr_beam_step instead (no att_scores, no prefix: None)."""
    from ccd_amd import ops
    B, T, _, C = tab.shape
    end, pad = C - 1, C
    seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, end, pad, device)
    joint = None if plain else ops.nrtr_joint_state(frames, W, normalized=normalized)
    table = torch.from_numpy(tab).to(device)
    sample = torch.arange(B, device=device).repeat_interleave(W)
    buf = torch.full((B * W, C + LD_PAD), float("nan"), device=device)
    parents, out = [], None
    for s in range(T):
        rows = table[sample, s, seq[:, s]]
        rows[state.view(-1) != ops.NRTR_LIVE] = float("nan")
        buf[:, :C] = rows
        if plain:
            out = ops.nrtr_beam_step(buf, C, s, end, pad, seq, score, state, parent, final=s == T - 1)
        else:
            out = ops.nrtr_beam_step_joint(buf, C, s, end, pad, seq, score, state, parent, joint, weight, class_offset=class_offset,
                                           final=s == T - 1)
        assert (out is None) == (s < T - 1)
        parents.append(parent.cpu().numpy().copy())
    if plain:
        out = out + (None,)
    paths, lengths, scores, att_scores = out
    assert paths.dtype == lengths.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(paths.shape) == (B, W, T) and tuple(lengths.shape) == tuple(scores.shape) == (B, W)
    assert (seq[:, 0] == end).all() and (scores.double() - score).abs().nan_to_num(0.0).max() <= 1e-4
    if not plain:
        assert att_scores.dtype == torch.float32 and tuple(att_scores.shape) == (B, W)
        assert (att_scores.double() - joint.att).abs().nan_to_num(0.0).max() <= 1e-4
    return (paths.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy(), None if plain else att_scores.cpu().numpy(),
            np.stack(parents, axis=1), None if plain else joint.prefix.cpu().numpy())


@functools.lru_cache(maxsize=None)
def case_frames(seed, B, Tc, Cc):
    return J.frames_of(seed * 31 + Tc, B, Tc, Cc)


@functools.lru_cache(maxsize=None)
def oracle(seed, B, W, C, T, mode, Tc, weight, normalized):
    """The oracle's result of every sample, computed once per process."""
    tab = K.case_tables(seed, B, T, C, mode)
    seen, _ = device_frames("cpu", case_frames(seed, B, Tc, C), C, normalized)
    return [J.beam_search(tab[b], seen[b], W, C - 1, C - 1, C, weight, normalized=normalized) for b in range(B)]


def compare(got, want, where):
    """One sample: got = (paths [W, T], lengths [W], scores [W], att_scores [W], parents [T, W], prefix [W, 2, Tc]) against the oracle's."""
    paths, lengths, scores, att, parents, prefix = got
    w_paths, w_lengths, w_scores, w_att, w_parents, _, w_prefix = want
    np.testing.assert_array_equal(parents, w_parents, err_msg=str(where))
    np.testing.assert_array_equal(lengths, w_lengths, err_msg=str(where))
    np.testing.assert_array_equal(paths, w_paths, err_msg=str(where))
    for r in range(len(lengths)):
        if w_lengths[r] < 0:
            assert scores[r] == -np.inf and att[r] == -np.inf, (where, r)
        else:
            assert abs(float(scores[r]) - w_scores[r]) <= 1e-6 * abs(w_scores[r]), (where, r, float(scores[r]), w_scores[r])
            assert abs(float(att[r]) - w_att[r]) <= 1e-6 * abs(w_att[r]), (where, r, float(att[r]), w_att[r])
    # the prefix states the kernel leaves behind: -inf where the oracle's are, else within fp64 rounding of a Tc-step recursion
    assert np.array_equal(np.isneginf(prefix), np.isneginf(w_prefix)), where
    fin = np.isfinite(w_prefix)
    assert np.all(np.abs(prefix[fin] - w_prefix[fin]) <= 1e-9 * np.maximum(1.0, np.abs(w_prefix[fin]))), where


def dropped_fraction(seed=SEED):
    """The share of samples whose oracle gap misses MIN_GAP, over all kernel cases."""
    gaps = [want[5] for case in J.CASES for want in oracle(seed, *case)]
    return sum(g < J.MIN_GAP for g in gaps) / len(gaps)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
def check_oracle(device):
    """The cases of nrtr_joint_np.CASES: the 64-lane class boundary, a full (Tc = 64) and a one-frame state, Tc = 33, W > C, a repeated
    last character (C = 3), w in {0.3, 0.7}, logits and probabilities."""
    total = compared = finished = live = 0
    for case in J.CASES:
        B, W, C, T, mode, Tc, weight, normalized = case
        want = oracle(SEED, *case)
        _, frames = device_frames(device, case_frames(SEED, B, Tc, C), C, normalized)
        got = drive(device, K.case_tables(SEED, B, T, C, mode), frames, W, weight, normalized=normalized)
        for b in range(B):
            total += 1
            if want[b][5] >= J.MIN_GAP:
                compare(tuple(a[b] for a in got), want[b], (case, b))
                compared += 1
            finished += int(((want[b][1] >= 0) & (want[b][1] < T)).sum())
            live += int((want[b][1] == T).sum())
    assert compared >= 0.98 * total, (compared, total)
    assert finished > 0 and live > 0                                           # finished words next to live ones behind the last step


# ------------------------------------------------------------------------------------------------ 2. w = 0
def check_weight_zero(device):
    """weight 0 is ops.nrtr_beam_step on the same inputs, bit for bit: paths, lengths, score bytes, the parents of every step - and
    att_scores are the scores.  A class without a CTC class (C = 128 against Cc = 92 frames) is a candidate here."""
    for (B, W, C, T, mode), Tc, Cc in (((5, 8, 92, 25, "end"), 32, 92), ((5, 16, 65, 25, "end"), 1, 65), ((5, 3, 128, 25, "end"), 33, 92)):
        tab = K.case_tables(SEED, B, T, C, mode)
        _, frames = device_frames(device, case_frames(SEED, B, Tc, Cc), Cc, False)
        got = drive(device, tab, frames, W, 0.0)
        want = drive(device, tab, None, W, 0.0, plain=True)
        for k in (0, 1, 4):
            assert np.array_equal(got[k], want[k]), (C, k)
        assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[2].tobytes(), C


# ------------------------------------------------------------------------------------------------ 3. ties
def check_ties(device):
    """nrtr_beam_checks.tie_table (decoder classes 0 and 1 are twins) with frames whose columns 1 and 2 - their CTC classes - are
    equal: twin hypotheses carry the same joint score bits and come in the order of k ascending."""
    tab = K.tie_table()
    frames = J.frames_of(5, 1, 8, 6)
    frames[:, :, 2] = frames[:, :, 1]
    seen, dev = device_frames(device, frames, 6, False)
    for W in (1, 2, 3, 4, 8, 16):
        want = J.beam_search(tab[0], seen[0], W, 5, 5, 6, 0.3, ties=True)
        assert want[5] >= J.MIN_GAP
        got = drive(device, tab, dev, W, 0.3)
        compare(tuple(a[0] for a in got), want, ("ties", W))
        paths, lengths, scores = got[0][0], got[1][0], got[2][0]
        words = [tuple(paths[r, :lengths[r]].tolist()) for r in range(W) if lengths[r] >= 0]
        plain = lambda w: tuple(0 if c == 1 else c for c in w)                                 # noqa: E731
        repeats = lambda w: [a == b for a, b in zip(w, w[1:])]                                 # noqa: E731
        pairs = 0
        for r in range(len(words)):
            for q in range(r + 1, len(words)):
                if plain(words[r]) == plain(words[q]) and repeats(words[r]) == repeats(words[q]):
                    # (twins whose repeats differ are no twins on the CTC side: 0 0 needs a blank in between, 0 1 does not)
                    assert np.asarray(scores[r]).tobytes() == np.asarray(scores[q]).tobytes() and words[r] < words[q], (words[r], words[q])
                    pairs += 1
        assert W < 16 or pairs >= 1, (W, words)


# ------------------------------------------------------------------------------------------------ 4. arguments
def check_arguments(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 29 and ops.NRTR_JOINT_MAX_STEPS == 64
    B, W, C, T, Tc = 2, 4, 12, 5, 7
    seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, device)
    frames = torch.randn(B, Tc, C + 2, generator=torch.Generator().manual_seed(2)).to(device)[:, :, :C]
    joint = ops.nrtr_joint_state(frames, W)
    assert joint.log_probs.dtype == joint.prefix.dtype == joint.att.dtype == torch.float64
    assert tuple(joint.log_probs.shape) == (B, Tc, C) and tuple(joint.prefix.shape) == (B, W, 2, Tc) and tuple(joint.att.shape) == (B, W)
    lp = joint.log_probs.cpu().numpy()
    for b in range(B):
        want = J.frame_log_probs(frames[b].cpu().numpy())
        assert np.abs(lp[b] - want).max() <= 1e-12
        rn, rb = J.root_state(want)
        for r in range(W):
            assert np.isneginf(joint.prefix[b, r, 0].cpu().numpy()).all() and np.abs(joint.prefix[b, r, 1].cpu().numpy() - rb).max() <= 1e-12
    assert joint.att.cpu().tolist() == [[0.0] + [float("-inf")] * (W - 1)] * B
    logits = torch.randn(B * W, C + 3, generator=torch.Generator().manual_seed(1)).to(device)
    ok = dict(logits=logits, C=C, step=0, end_idx=C - 1, pad_idx=C, seq=seq, score=score, state=state, parent=parent, joint=joint, weight=0.5)
    tensors = (seq, score, state, parent, joint.prefix, joint.att)

    def bad(error=ValueError, **kw):
        before = [t.clone() for t in tensors]
        with pytest.raises(error):
            ops.nrtr_beam_step_joint(**{**ok, **kw})
        assert all(torch.equal(a, b) for a, b in zip(tensors, before))

    for width in (0, 17):
        with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
            ops.nrtr_joint_state(frames, width)
    for f in (frames.double(), frames[0], torch.zeros(B, 65, C, device=device), torch.zeros(B, Tc, 129, device=device),
              torch.zeros(B, 0, C, device=device), frames.transpose(1, 2)):
        with pytest.raises(ValueError, match="nrtr_joint_state"):
            ops.nrtr_joint_state(f, W)
    bad(TypeError, joint=None)                                                 # a foreign handle
    bad(TypeError, joint=joint.prefix)
    bad(weight=-0.1)                                                           # the weight
    bad(weight=1.5)
    bad(weight=float("nan"))
    bad(weight=True)
    bad(weight="0.3")
    bad(class_offset=2)
    bad(class_offset=-1)
    bad(joint=ops.nrtr_joint_state(frames, 3))                                 # made for another width
    bad(joint=ops.nrtr_joint_state(frames[:1], W))
    bad(score=score.float())                                                   # what nrtr_beam_step refuses
    bad(state=state.long())
    bad(seq=seq[:-1])
    bad(logits=logits[:, :C - 1])
    bad(step=T)
    bad(end_idx=C)
    # the entry points themselves refuse what the wrappers let through, and launch nothing
    st = _lib.stream()
    att_out = torch.zeros(B, W, device=device)
    args = [logits, C + 3, B, W, C, 0, C - 1, C, seq, T + 1, score, state, parent, None, None, None, joint.log_probs, Tc, C, 1, 0.5,
            joint.prefix, joint.att, None, st]
    for i, v, code in ((0, None, -1), (8, None, -1), (12, None, -1), (16, None, -1), (21, None, -1), (22, None, -1), (1, -1, -1),
                       (5, -1, -1), (3, 0, -2), (3, 17, -2), (4, 0, -2), (4, 129, -2), (9, 129, -2), (5, T, -2), (6, C, -2), (7, 65536, -2),
                       (17, 0, -2), (17, 65, -2), (18, 0, -2), (18, 129, -2), (19, 2, -2), (19, -1, -2), (20, -0.01, -2), (20, 1.01, -2),
                       (20, float("nan"), -2), (20, float("inf"), -2)):
        call = list(args)
        call[i] = v
        assert lib.ccd_nrtr_beam_step_joint(*call) == code, (i, v)
    call = list(args)
    call[23] = att_out                                                         # att_scores without the paths
    assert lib.ccd_nrtr_beam_step_joint(*call) == -1
    call = list(args)                                                          # the paths without att_scores
    call[13], call[14], call[15] = (torch.zeros(B, W, T, dtype=torch.int32, device=device), torch.zeros(B, W, dtype=torch.int32, device=device),
                                    torch.zeros(B, W, device=device))
    assert lib.ccd_nrtr_beam_step_joint(*call) == -1
    assert int(state.sum()) == B and int(parent.min()) == -1 and int(parent.max()) == -1       # nothing ran
    assert joint.att.cpu().tolist() == [[0.0] + [float("-inf")] * (W - 1)] * B
    assert lib.ccd_nrtr_beam_step_joint(None, C, 0, W, C, 0, C - 1, C, None, T + 1, None, None, None, None, None, None, None, Tc, C, 1, 0.5,
                                        None, None, None, st) == 0                            # the empty batch
    lp_out, pre_out = torch.full((B, Tc, C), 7.0, dtype=torch.float64, device=device), torch.full((B, W, 2, Tc), 7.0, dtype=torch.float64,
                                                                                                  device=device)
    begin = [frames, frames.stride(0), frames.stride(1), B, Tc, C, 0, W, lp_out, pre_out, st]
    for i, v, code in ((0, None, -1), (8, None, -1), (9, None, -1), (1, -1, -1), (2, -1, -1), (3, -1, -1), (4, 0, -2), (4, 65, -2), (5, 0, -2),
                       (5, 129, -2), (6, 2, -2), (7, 0, -2), (7, 17, -2)):
        call = list(begin)
        call[i] = v
        assert lib.ccd_nrtr_joint_begin(*call) == code, (i, v)
    assert float(lp_out.min()) == 7.0 and float(pre_out.min()) == 7.0 and float(pre_out.max()) == 7.0      # untouched
    assert lib.ccd_nrtr_joint_begin(None, 0, 0, 0, Tc, C, 0, W, None, None, st) == 0
    ops.nrtr_beam_step_joint(**ok)
    assert int(parent.min()) == 0 and int(parent.max()) == 0 and int((state == ops.NRTR_UNUSED).sum()) == 0
    assert bool(torch.isfinite(joint.att).all()) and bool(torch.isfinite(score).all())
    # class_offset 0: decoder class 0 would be the blank - it is a character of its own here, CTC class 0
    seq2, score2, state2, parent2 = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, device)
    ops.nrtr_beam_step_joint(logits, C, 0, C - 1, C, seq2, score2, state2, parent2, ops.nrtr_joint_state(frames, W), 0.5, class_offset=0)
    assert int((state2 == ops.NRTR_UNUSED).sum()) == 0


# ------------------------------------------------------------------------------------------------ 5. the hybrid model
AUX, END_BIAS, BLANK_BIAS = 0.3, 0.5, 5.0
MODEL_WORDS = ["hello", "Wor1d!", "", "0123456789abcdefghijklmnopqrstuvwxyz"]       # (the last: cut at max_seq_len, no <EOS>)


def build_model(device, aux=AUX, joint=None, beam_width=None, seed=2):
    """vit_tiny, a 1-layer decoder, eval() - dropout and drop-path off; the <EOS> bias raised so that hypotheses finish, and the blank
    bias of the auxiliary head: at its initialisation every frame is uniform over the 92 classes, and a word of n characters pays
    (32 - n) log 92 for its blanks - no hypothesis would finish within 25 steps."""
    from ccd_amd import finetune as ft
    torch.manual_seed(seed)
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=1)
    if aux:
        cfg.decoder_aux_ctc_weight = aux
    if joint is not None:
        cfg.decoder_joint_ctc_weight, cfg.decoder_beam_width = joint, beam_width
    model = ft.build_model(cfg, device).eval()
    with torch.no_grad():
        model.arena.w("decoder.classifier.bias")[91] += END_BIAS
        if aux:
            model.arena.w("ctc_decoder.fc.bias")[0] += BLANK_BIAS
    model.arena.refresh_mirrors()
    return model


def model_images(B, device):
    return torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(100 + B)).to(device)


def _grads(model, loss):
    model.arena.grad.zero_()
    loss.backward()
    return {k: model.arena.g(k).detach().clone() for k in model.state_dict() if k in model.arena.params}


def check_hybrid_loss_and_gradients(device):
    """forward_train of the hybrid model is (1 - a) TFLoss + a CTCLoss of the two heads on the same tokens, last_losses holds the two
    parts, and the arena gradients of its backward are the weighted sum of the two single-loss backward passes - per tensor within
    the gates tests/model_checks.py applies to finetune gradients: |norm ratio - 1| < 8e-2, cosine > 0.97 (norms below 1e-7: < 1e-4).
    -> the largest |norm ratio - 1| and the smallest cosine seen."""
    model = build_model(device)
    img = model_images(4, device)
    targets = model.label_convertor.str2tensor(MODEL_WORDS).to(device)
    ctc_targets = model.ctc_targets(targets)
    assert tuple(ctc_targets.shape) == (4, 24) and ctc_targets[0].tolist()[:6] == [18, 15, 22, 22, 25, 0] and int(ctc_targets[2].sum()) == 0
    names = [k for k in model.state_dict() if k in model.arena.params]
    assert "ctc_decoder.fc.weight" in names and "ctc_decoder.fc.bias" in names

    def parts():
        feat = model.extract_feat(img)
        out_dec, _ = model.decoder(feat, model.encoder(feat), {"padded_targets": targets}, train_mode=True)
        tf = model.loss(out_dec, {"padded_targets": targets})
        ctc = model.ctc_loss(model.ctc_decoder.forward_train(feat), {"padded_targets": ctc_targets})
        return tf, ctc

    tf, _ = parts()
    g_tf = _grads(model, tf)
    _, ctc = parts()
    g_ctc = _grads(model, ctc)
    assert int(model.ctc_loss.last_infeasible) == 0                            # (24 distinct characters still align to 32 frames)
    loss, _ = model(img, targets, return_loss=True)
    got = _grads(model, loss)
    tf, ctc, part = tf.detach(), ctc.detach(), model.last_losses
    # the loss is the weighted sum of the two parts it reports (fp32: a rounding per product and one for the sum) ...
    want_loss = (1 - AUX) * float(part["tf"]) + AUX * float(part["ctc"])
    assert abs(float(loss.detach()) - want_loss) <= 1e-6 * abs(want_loss), (float(loss.detach()), want_loss)
    # ... and the parts are the two losses computed alone, within the 2e-3 tests/model_checks.py grants a finetune loss (a second
    # forward pass on the GPU is not bit-reproducible: some products accumulate with atomics)
    assert abs(float(part["tf"]) - float(tf)) <= 2e-3 and abs(float(part["ctc"]) - float(ctc)) <= 2e-3, (part, float(tf), float(ctc))
    assert float(ctc) > 0 and float(tf) > 0 and part["tf"].device == loss.device and not part["tf"].requires_grad
    worst_ratio, worst_cos = 0.0, 1.0
    for k in names:
        want = (1 - AUX) * g_tf[k].double() + AUX * g_ctc[k].double()
        nr = float(want.norm())
        if nr < 1e-7:
            assert float(got[k].norm()) < 1e-4, k
            continue
        ratio, cos = abs(float(got[k].double().norm()) / nr - 1), float((got[k].double().flatten() @ want.flatten()) / (got[k].double().norm() * nr))
        worst_ratio, worst_cos = max(worst_ratio, ratio), min(worst_cos, cos)
        assert ratio < 8e-2 and cos > 0.97, (k, ratio, cos)
    assert float(g_ctc["ctc_decoder.fc.weight"].norm()) > 0 and float(g_tf["ctc_decoder.fc.weight"].norm()) == 0
    assert float(g_ctc["decoder.classifier.weight"].norm()) == 0 and float(g_ctc["backbone.blocks.0.attn.qkv.weight"].norm()) > 0
    print(f"hybrid gradients against the weighted sum of two backward passes: largest |norm ratio - 1| {worst_ratio:.3e}, smallest cosine "
          f"{worst_cos:.6f} over {len(names)} tensors")
    return worst_ratio, worst_cos


def check_joint_weight_zero_is_the_plain_beam(device, B=4, W=4):
    """forward_beam with joint_ctc_weight = 0 returns the bytes of the plain forward_beam, and the attention parts are the scores."""
    model = build_model(device)
    img = model_images(B, device)
    with torch.no_grad():
        plain = model.forward_beam(img, W)
        joint = model.forward_beam(img, W, joint_ctc_weight=0.0)
    assert len(plain) == len(joint) == 3 and all(torch.equal(a, b) for a, b in zip(plain, joint))
    assert torch.equal(model.last_att_scores, plain[2])
    with pytest.raises(ValueError, match="aux_ctc_weight"):
        build_model(device, aux=None).forward_beam(img, W, joint_ctc_weight=0.3)
    with pytest.raises(ValueError, match="no auxiliary CTC head"):
        build_model(device, aux=None).forward_ctc(img)


def check_joint_scores_are_the_two_exact_scorers(device, B=4, W=8, w=0.3):
    """Every FINISHED hypothesis of the joint beam scores (1 - w) forward_score(its word) + w ops.ctc_lexicon_score of that word on
    forward_ctc(img), within 1e-5 relative (three fp32 roundings of 6e-8 each, with margin); the configured weight and width are the
    defaults, and a second call replays the graph (where there is one) and returns the same bytes.
    -> (the largest relative difference, the finished hypotheses compared)."""
    from ccd_amd import ops
    model = build_model(device, joint=w, beam_width=W)
    assert model.joint_ctc_weight == w and model.decoder.beam_width == W
    img = model_images(B, device)
    T = model.label_convertor.max_seq_len
    with torch.no_grad():
        paths, lengths, scores = model.forward_beam(img)
        att = model.last_att_scores.clone()
        again = model.forward_beam(img)
        probs = model.forward_ctc(img)
    assert all(torch.equal(a, b) for a, b in zip((paths, lengths, scores), again)) and torch.equal(att, model.last_att_scores)
    if torch.device(device).type == "cuda":
        assert len(model.decoder._joint_graphs) == 1 and len(model.decoder._beam_graphs) == 0 and len(model.decoder._trie_graphs) == 0
    assert tuple(probs.shape) == (B, 32, 92) and tuple(paths.shape) == (B, W, T)
    p, n, s, a = paths.cpu().numpy(), lengths.cpu().numpy(), scores.double().cpu().numpy(), att.double().cpu().numpy()
    worst, compared = 0.0, 0
    for b in range(B):
        done = [r for r in range(W) if 0 <= n[b, r] < T]
        if not done:
            continue
        words = [p[b, r, :n[b, r]].tolist() for r in done]
        exact = model.forward_score(img[b:b + 1], [words])["score"].double().cpu().numpy()
        rows = torch.zeros((len(words), max(1, max(len(x) for x in words))), dtype=torch.int64)
        for i, x in enumerate(words):
            rows[i, :len(x)] = torch.tensor(x, dtype=torch.int64) + 1
        ctc = ops.ctc_lexicon_score(probs[b:b + 1], ops.ctc_lexicon(rows), normalized=True).double().cpu().numpy()[0]
        for i, r in enumerate(done):
            want = (1 - w) * exact[i] + w * ctc[i]
            worst = max(worst, abs(s[b, r] - want) / abs(want))
            assert abs(s[b, r] - want) <= 1e-5 * abs(want), (b, r, s[b, r], want, exact[i], ctc[i])
            assert abs(a[b, r] - exact[i]) <= 1e-5 * abs(exact[i]), (b, r, a[b, r], exact[i])
            compared += 1
    assert compared >= B                                                       # (the <EOS> bias: most hypotheses finish)
    print(f"joint beam against (1 - w) forward_score + w ctc_lexicon_score: largest relative difference {worst:.3e} over {compared} "
          f"finished hypotheses")
    return worst, compared
