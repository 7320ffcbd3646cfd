"""The checks of the CTC head's kernels (kernels/ctc.h, ccd_text_score_ctc) that run on either backend: the CPU SIMT executor
(tests/test_ctc_sim.py) and the MI355X (tests/test_ctc_gpu.py).  `device` is where the tensors live.

Oracle: F.ctc_loss(F.log_softmax(logits.double(), -1), ..., reduction='none', zero_infinity=True) on the CPU, with autograd down to
the logits (ctc_np.torch_oracle).  Gates:
  * the infeasible samples (nll 0, zero gradient, acc[2]) are exactly torch's inf set;
  * max |nll - fp64| over the whole case set <= 2 x the same figure of torch's own fp32 CPU result (a different summation order);
  * every d_logits element is the fp64 gradient rounded to bf16, or its bf16 neighbour;
  * the pad columns are exactly zero, two runs give identical bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_np as R

LD = 128


def _padded(logits, C):
    """[B, T, C] -> [B * T, 128] fp32 on the CPU with NaN behind column C."""
    B, T, _ = logits.shape
    buf = torch.full((B * T, LD), float("nan"))
    buf[:, :C] = logits.reshape(B * T, C)
    return buf


def run_loss(device, logits, targets, upstream=None):
    """ops.ctc_loss_fwd + _bwd on [B, T, C] logits laid out with ld = 128 and NaN pads -> (nll [B], acc [3], d_logits bf16 [B, T, 128])."""
    from ccd_amd import ops
    B, T, C = logits.shape
    buf, tg = _padded(logits, C).to(device), targets.to(device)
    nll, acc, ws = ops.ctc_loss_fwd(buf, C, tg, T)
    d = ops.ctc_loss_bwd(buf, C, tg, T, ws, None if upstream is None else upstream.to(device), LD)
    assert nll.dtype == torch.float32 and d.dtype == torch.bfloat16 and tuple(d.shape) == (B * T, LD)
    return nll.cpu(), acc.cpu(), d.cpu().view(B, T, LD)


def _ordered(bits16):
    """bf16 bit patterns -> integers in value order (+0 and -0 both 0): neighbours differ by 1."""
    b = bits16.astype(np.int64) & 0xFFFF
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def check_gradient(d, ref64, where):
    """d bf16 [.., C] against the fp64 gradient: the rounded value or its bf16 neighbour, every element."""
    got = _ordered(d.contiguous().view(torch.int16).numpy())
    want = _ordered(ref64.to(torch.float32).to(torch.bfloat16).contiguous().view(torch.int16).numpy())
    off = np.abs(got - want) > 1
    assert not off.any(), (where, int(off.sum()), [(tuple(int(v) for v in i), float(d[tuple(i)]), float(ref64[tuple(i)]))
                                                   for i in np.argwhere(off)[:5]])


def _check_batch(device, logits, targets, where, worst):
    B, T, C = logits.shape
    raw64, nll64, grad64 = R.torch_oracle(logits, targets, torch.float64)
    _, nll32, _ = R.torch_oracle(logits, targets, torch.float32)
    nll, acc, d = run_loss(device, logits, targets)
    inf = torch.isinf(raw64)
    L = torch.from_numpy(R.label_lengths(targets.numpy()))
    assert torch.equal(nll == 0, inf | (nll64 == 0)) and int(acc[2]) == int(inf.sum()) and int(acc[1]) == B, (where, nll, raw64)
    worst["kernel"] = max(worst["kernel"], float((nll.double() - nll64).abs().max()))
    worst["torch_fp32"] = max(worst["torch_fp32"], float((nll32.double() - nll64).abs().max()))
    want0 = float((nll64 / L.clamp_min(1)).sum())
    assert abs(float(acc[0]) - want0) <= 2.0 ** -22 * max(1.0, abs(want0)), (where, float(acc[0]), want0)
    check_gradient(d[:, :, :C], grad64, where)
    assert (d[:, :, C:].view(torch.int16) == 0).all(), where                  # the pad columns: +0 bits
    assert (d[inf].view(torch.int16) == 0).all(), where
    nll2, acc2, d2 = run_loss(device, logits, targets)
    assert nll.numpy().tobytes() == nll2.numpy().tobytes() and acc.numpy().tobytes() == acc2.numpy().tobytes() and \
        d.view(torch.int16).numpy().tobytes() == d2.view(torch.int16).numpy().tobytes(), where
    return inf


def check_loss(device):
    """Every named case (one sample each), the random batches B in {1, 5, 67}, and the named T = 32, C = 92 cases as one batch."""
    worst = {"kernel": 0.0, "torch_fp32": 0.0}
    cases = R.named_cases()
    verdict = {}
    for c in cases:
        inf = _check_batch(device, c["logits"][None], R.pad_targets(c["target"]), c["name"], worst)
        verdict[c["name"]] = bool(inf[0])
    infeasible = sorted(k for k, v in verdict.items() if v)
    assert infeasible == ["05_17_equal", "08_L25_8_repeats", "10b_L31_two_repeats"], infeasible
    same = [c for c in cases if (c["T"], c["C"]) == (32, 92)]
    _check_batch(device, torch.stack([c["logits"] for c in same]), torch.cat([R.pad_targets(c["target"]) for c in same]), "named batch", worst)
    for B in (1, 5, 67):
        logits, targets = R.random_batch(B, seed=200 + B)
        _check_batch(device, logits, targets, f"random B={B}", worst)
    print(f"max |nll - fp64|: kernel {worst['kernel']:.3e}, torch fp32 CPU {worst['torch_fp32']:.3e}")
    assert worst["kernel"] <= 2.0 * worst["torch_fp32"], worst
    return worst


def check_upstream(device):
    """upstream: a device scalar multiplied in; NULL means 1."""
    logits, targets = R.random_batch(5, seed=31)
    _, _, d1 = run_loss(device, logits, targets)
    _, _, d3 = run_loss(device, logits, targets, upstream=torch.tensor([0.375]))
    _, _, grad64 = R.torch_oracle(logits, targets, torch.float64)
    check_gradient(d3[:, :, :92], grad64 * 0.375, "upstream")
    assert not torch.equal(d1, d3)


def check_loss_module(device):
    """CTCLoss on a user's own tensors: a [B, T, C] view of a 128-wide leaf gets its gradient back (nothing is parked for it), as
    does a dense tensor; both equal the oracle's to bf16."""
    from ccd_amd import finetune_engine as fe
    from ccd_amd.loss.ctc_loss import CTCLoss
    logits, targets = R.random_batch(3, seed=41)
    _, nll64, grad64 = R.torch_oracle(logits, targets, torch.float64)
    L = torch.from_numpy(R.label_lengths(targets.numpy()))
    want = float((nll64 / L.clamp_min(1)).mean())
    crit = CTCLoss()
    leaf = torch.zeros(3, 32, LD)
    leaf[:, :, :92] = logits
    leaf = leaf.to(device).requires_grad_(True)
    dense = logits.clone().to(device).requires_grad_(True)
    for x, view in ((leaf, leaf[:, :, :92]), (dense, dense)):
        loss = crit(view, {"padded_targets": targets.to(device)})
        loss.backward()
        assert abs(loss.item() - want) <= 2.0 ** -21 * want and int(crit.last_infeasible) == 0
        check_gradient(x.grad.cpu()[:, :, :92].to(torch.bfloat16), grad64, "module")
    assert float(leaf.grad[:, :, 92:].abs().max()) == 0.0 and not fe._PARKED_LOGIT_GRADS
    with pytest.raises(ValueError, match="contiguous classes"):
        from ccd_amd import ops
        ops.ctc_greedy(logits.to(device).transpose(1, 2))


def check_numpy_restatement():
    """ctc_np.ctc_reference against torch on the named cases (CPU only)."""
    for c in R.named_cases():
        raw64, _, grad64 = R.torch_oracle(c["logits"][None], R.pad_targets(c["target"]), torch.float64)
        nll, grad = R.ctc_reference(c["logits"].numpy(), c["target"])
        if torch.isinf(raw64[0]):
            assert np.isinf(nll), c["name"]
            continue
        assert abs(nll - float(raw64[0])) <= 1e-9 * max(1.0, abs(nll)), (c["name"], nll, float(raw64[0]))
        got = grad / max(len(c["target"]), 1)
        assert np.abs(got - grad64[0].numpy()).max() <= 1e-9, (c["name"], np.abs(got - grad64[0].numpy()).max())


# ------------------------------------------------------------------------------------------------ pooling
def check_pool(device):
    from ccd_amd import ops
    g = torch.Generator().manual_seed(5)
    for N, E in ((1, 64), (3, 192), (2, 8)):
        tokens = torch.randn(N, 256, E, generator=g).to(torch.bfloat16)
        frames = ops.ctc_pool_fwd(tokens.to(device)).cpu()
        want = tokens.float().view(N, 8, 32, E).sum(1) / 8.0                   # fp32 sums in row order, as the kernel adds them
        assert torch.equal(frames.view(N, 32, E), want.to(torch.bfloat16)), (N, E)
        d_frames = torch.randn(N * 32, E, generator=g).to(torch.bfloat16)
        d_tokens = ops.ctc_pool_bwd(d_frames.to(device)).cpu()
        want = (d_frames.float() / 8.0).to(torch.bfloat16).view(N, 1, 32, E).expand(N, 8, 32, E).reshape(N, 256, E)
        assert torch.equal(d_tokens, want), (N, E)
    assert tuple(ops.ctc_pool_fwd(torch.zeros(0, 256, 64, dtype=torch.bfloat16, device=device)).shape) == (0, 64)
    with pytest.raises(RuntimeError, match="ccd_ctc_pool_fwd failed: unsupported shape"):
        ops.ctc_pool_fwd(torch.zeros(1, 256, 12, dtype=torch.bfloat16, device=device))
    with pytest.raises(TypeError, match="ccd_ctc_pool_fwd: tokens expects bfloat16, got float32"):
        ops.ctc_pool_fwd(torch.zeros(1, 256, 64, device=device))


# ------------------------------------------------------------------------------------------------ greedy decoding and scoring
def greedy_case():
    """Logits [9, 32, 92] with ties (first maximum), an all-equal frame, an all-blank sample, 32 kept characters, repeats."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(9, 32, 92, generator=g) * 3.0
    x[1, :, :] = -4.0
    x[1, :, 0] = 2.0                                                           # all blank
    x[2, :, :] = -3.0
    for t in range(32):
        x[2, t, 1 + (t % 90)] = 5.0                                            # 32 different characters in a row: 32 kept
    x[3, 4, :] = 0.25                                                          # an all-equal frame: class 0, the blank
    x[3, 5, :] = -1.0
    x[3, 5, [7, 3, 80]] = 6.0                                                  # a three-way tie: class 3
    x[4, :, :] = -2.0
    for t, c in enumerate([5, 5, 0, 5, 5, 6, 6, 0, 0, 6] + [0] * 22):          # "5 5 _ 5 5 6 6 _ _ 6" -> 5 5 6 6
        x[4, t, c] = 3.0
    x[5, :, :] = 0.0                                                           # every frame all-equal: all blank
    x[6, :, 91] += 20.0                                                        # one class everywhere: a single <UKN>
    x[7, 0, :] = -1.0
    x[7, 0, [0, 9]] = 4.0                                                      # blank ties with a character: the blank wins
    return x


GREEDY_TRUTH = ["", "", "0123456789abcdefghijklmnopqrstuv", "3", "4455", "anything", "<UKN>", "k", "Kİ"]


def check_greedy(device):
    from ccd_amd import ops
    x = greedy_case()
    path, length, conf = (t.cpu().numpy() for t in ops.ctc_greedy(x.to(device)))
    want_path, want_len, want_conf = R.greedy(x.numpy())
    np.testing.assert_array_equal(path, want_path)
    np.testing.assert_array_equal(length, want_len)
    assert want_len[1] == 0 and want_len[2] == 32 and want_len[5] == 0 and want_len[6] == 1 and want_len[7] < 32
    assert want_path[4, :want_len[4]].tolist() == [5, 5, 6, 6] and 3 in want_path[3].tolist() and 7 not in want_path[3, :2].tolist()
    np.testing.assert_allclose(conf, want_conf, rtol=64 * 2.0 ** -23, atol=0)    # a 92-term fp32 sum of exp: a few ulp
    # a strided view is read in place
    wide = torch.full((9, 40, 100), 50.0)
    wide[:, :32, :92] = x
    p2, l2, _ = ops.ctc_greedy(wide.to(device)[:, :32, :92])
    np.testing.assert_array_equal(p2.cpu().numpy(), want_path)
    np.testing.assert_array_equal(l2.cpu().numpy(), want_len)


def check_score(device):
    """Records of ops.text_score_ctc and the totals of TextAccuracy.update_scores against the host path (tensor2idx + update)."""
    from ccd_amd import ops
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth
    conv = CTCConvertor()
    x = greedy_case()
    gts = list(GREEDY_TRUTH)
    idx, scores = conv.tensor2idx(x)
    path, length, _ = R.greedy(x.numpy())
    assert idx == [path[b, :length[b]].tolist() for b in range(9)]               # the host decode is the same rule
    host = TextAccuracy()
    host.update(gts, conv.idx2str(idx))
    want = host.result()
    dev = TextAccuracy()
    rec = dev.update_scores(x.to(device), gts, conv).cpu().numpy()
    got = dev.result()
    for k in ("ccr", "cwr", "ted", "ted/w", "words"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["ned"] - want["ned"]) <= 9 * 2.0 ** -52 * max(1.0, want["ned"])
    for b in range(9):                                                          # record by record
        one = TextAccuracy()
        one.update([gts[b]], conv.idx2str([idx[b]]))
        assert rec[b].tolist() == [int(one.total_ed), int(one.correct_num_char), len(gts[b]), int(one.correct_num_word)], (b, rec[b])
    # the wrapper on a strided view
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(gts))
    wide = torch.full((9, 40, 92), 50.0)
    wide[:, :32] = x
    np.testing.assert_array_equal(ops.text_score_ctc(wide.to(device)[:, :32], raw, norm, codes, lens).cpu().numpy(), rec)


# ------------------------------------------------------------------------------------------------ the ABI's contract
def check_abi_contract(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 20
    st = _lib.stream()
    B, T, C = 3, 32, 92
    logits, targets = R.random_batch(B, seed=77, Lmax=25)
    buf, tg = _padded(logits, C).to(device), targets.to(device)
    nll = torch.zeros(B, device=device)
    acc = torch.zeros(3, device=device)
    nbytes = lib.ccd_ctc_loss_ws_bytes(B, T)
    assert nbytes > 0 and nbytes % 8 == 0 and lib.ccd_ctc_loss_ws_bytes(0, T) == 0
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=device)
    d = torch.zeros(B * T, LD, dtype=torch.bfloat16, device=device)
    fwd = [buf, LD, B, T, C, tg, 25, nll, acc, ws, st]
    bwd = [buf, LD, B, T, C, tg, 25, ws, None, d, LD, st]
    assert lib.ccd_ctc_loss_fwd(*fwd) == 0 and lib.ccd_ctc_loss_bwd(*bwd) == 0
    for call, args, pointers in ((lib.ccd_ctc_loss_fwd, fwd, (0, 5, 7, 8, 9)), (lib.ccd_ctc_loss_bwd, bwd, (0, 5, 7, 9))):
        for i in pointers:                                                     # a missing pointer
            bad = list(args)
            bad[i] = None
            assert call(*bad) == -1, (call.__name__, i)
        for i, v in ((1, -1), (2, -1), (6, -1)):                               # a negative stride, batch or size
            bad = list(args)
            bad[i] = v
            assert call(*bad) == -1, (call.__name__, i, v)
        for i, v in ((4, 0), (4, 129), (3, 0), (3, 65), (6, 32), (1, 91)):     # C outside 1..128, T outside 1..64, Lmax > 31, ldl < C
            bad = list(args)
            bad[i] = v
            assert call(*bad) == -2, (call.__name__, i, v)
        empty = list(args)
        empty[2] = 0
        assert call(*[None if isinstance(a, torch.Tensor) else a for a in empty]) == 0      # B = 0 is a no-op
    assert lib.ccd_ctc_loss_bwd(*(bwd[:10] + [91, st])) == -2 and lib.ccd_ctc_loss_bwd(*(bwd[:10] + [-1, st])) == -1      # ldd
    # labels outside [1, C): infeasible, never an index (C = 3 at the end of a small buffer; a huge, a negative and the label C itself)
    small = torch.randn(4, 2, 3)
    bad_targets = torch.tensor([[1, 3, 0], [2, -1, 0], [1, 2 ** 40, 0], [1, 2, 0]])
    n4, a4, d4 = run_loss(device, small, bad_targets)
    assert (n4[:3] == 0).all() and n4[3] > 0 and a4.tolist()[1:] == [4.0, 3.0] and (d4[:3].view(torch.int16) == 0).all()
    raw64, _, grad64 = R.torch_oracle(small[3:], bad_targets[3:], torch.float64)
    assert abs(float(n4[3]) - float(raw64[0])) < 1e-5
    check_gradient(d4[3:, :, :3], grad64 / 4.0, "valid sample beside bad labels")
    # greedy
    x = torch.randn(B, T, C).to(device)
    path = torch.zeros(B, T, dtype=torch.int32, device=device)
    length = torch.zeros(B, dtype=torch.int32, device=device)
    conf = torch.zeros(B, T, device=device)
    ok = [x, T * C, C, B, T, C, path, length, conf, st]
    assert lib.ccd_ctc_greedy(*ok) == 0
    for i in (0, 6, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_greedy(*bad) == -1, i
    for i, v in ((1, -1), (2, -1), (3, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_greedy(*bad) == -1, (i, v)
    for i, v in ((4, 0), (4, 65), (5, 0), (5, 129)):
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_greedy(*bad) == -2, (i, v)
    assert lib.ccd_ctc_greedy(None, 0, 0, 0, T, C, None, None, None, st) == 0
    # pooling
    tok = torch.zeros(1, 256, 64, dtype=torch.bfloat16, device=device)
    fr = torch.zeros(32, 64, dtype=torch.bfloat16, device=device)
    assert lib.ccd_ctc_pool_fwd(tok, fr, 1, 8, 32, 64, st) == 0 and lib.ccd_ctc_pool_bwd(fr, tok, 1, 8, 32, 64, st) == 0
    assert lib.ccd_ctc_pool_fwd(None, fr, 1, 8, 32, 64, st) == -1 and lib.ccd_ctc_pool_fwd(tok, fr, -1, 8, 32, 64, st) == -1
    assert lib.ccd_ctc_pool_fwd(tok, fr, 1, 8, 32, 60, st) == -2 and lib.ccd_ctc_pool_fwd(None, None, 0, 8, 32, 64, st) == 0
    # text_score_ctc: the error codes of ccd_text_score
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import encode_truth
    conv = CTCConvertor()
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(["ab", "c", ""]))
    rec = torch.zeros(B, 4, dtype=torch.int32, device=device)
    ok = [x, T * C, C, B, T, C, raw, raw.shape[1], norm, norm.shape[1], codes, codes.shape[1], codes.shape[1], lens, rec, st]
    assert lib.ccd_text_score_ctc(*ok) == 0
    for i in (0, 6, 8, 13, 14):
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_text_score_ctc(*bad) == -1, i
    for i, v in ((1, -1), (3, -1), (11, -1), (4, 43), (4, 0), (5, 0), (7, 65), (9, 0)):
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_text_score_ctc(*bad) == (-1 if v == -1 else -2), (i, v)
    # the wrappers
    with pytest.raises(TypeError, match=r"^ccd_ctc_loss_fwd: targets expects int64, got int32$"):
        ops.ctc_loss_fwd(buf, C, tg.int(), T)
    with pytest.raises(RuntimeError, match="ccd_ctc_loss_fwd failed: unsupported shape"):
        ops.ctc_loss_fwd(buf, C, torch.zeros(B, 32, dtype=torch.long, device=device), T)


# ------------------------------------------------------------------------------------------------ the model
# A long word, a short one and one of medium length.  The loss is the mean of nll / L, so the short word weighs most.
WORDS = ["text-recognition", "aab", "Wor1d!"]


def ctc_model(device, arch="vit_test2"):
    from ccd_amd import finetune as ft
    from model_checks import _register_test_arch
    _register_test_arch()
    cfg = ft.FinetuneConfig(arch=arch, drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    return ft.build_model(cfg, device, dropout=0.0)


def _cpu_loss(P, spec, img, targets):
    """The restatement: the oracle's encoder, mean over the 8 token rows, one linear layer, F.ctc_loss (mean, zero_infinity)."""
    from oracle import ccd_oracle as O
    feat, _ = O.backbone_forward(P, "backbone.", img, spec)
    B, _, E = feat.shape
    logits = F.linear(feat.view(B, 8, 32, E).mean(1), P["decoder.fc.weight"], P["decoder.fc.bias"])
    L = torch.from_numpy(R.label_lengths(targets.numpy())).long()
    flat = torch.cat([targets[b, :L[b]] for b in range(B)])
    return F.ctc_loss(F.log_softmax(logits, -1).transpose(0, 1), flat, torch.full((B,), 32, dtype=torch.long), L, blank=0,
                      reduction="mean", zero_infinity=True)


def check_model_parity(device):
    """Tiny arch, B = 3, two AdamW iterations: the loss within the project's 1e-3 of the CPU restatement, which takes its own AdamW
    steps (the oracle's) from the same initial weights."""
    from ccd_amd import finetune as ft
    from oracle import ccd_oracle as O
    torch.manual_seed(5)
    model = ctc_model(device)
    spec = O.Spec(embed_dim=192, depth=2, heads=3)
    P = {k: v.detach().cpu().float().clone() for k, v in model.state_dict().items()}
    unused = set(model.unused_parameter_names())
    trainable = [k for k in P if k not in unused]
    for k in trainable:
        P[k].requires_grad_(True)
    net, o_opt = O.Net(spec, P, trainable), O.AdamWState()
    opt = ft.make_optimizer(model)
    targets = model.label_convertor.str2tensor(WORDS)
    gen = torch.Generator().manual_seed(77)
    for step in range(2):
        img = torch.randn(3, 3, 32, 128, generator=gen)
        want = _cpu_loss(net.P, spec, img, targets)
        grads = torch.autograd.grad(want, [net.P[k] for k in trainable], allow_unused=True)
        o_opt.step(net, {k: g for k, g in zip(trainable, grads) if g is not None}, 3e-4, 0.05)
        loss, _ = ft.training_iteration(model, opt, img.to(device), targets.to(device), 3e-4)
        print(f"step {step}: loss {loss.item():.6f}, CPU restatement {want.item():.6f}")
        assert abs(loss.item() - want.item()) < 1e-3, (step, loss.item(), want.item())
    assert int(model.loss.last_infeasible.item()) == 0


def check_model_trains(device, iterations=21):
    from ccd_amd import finetune as ft
    torch.manual_seed(6)
    model = ctc_model(device)
    opt = ft.make_optimizer(model)
    targets = model.label_convertor.str2tensor(WORDS).to(device)
    img = torch.randn(3, 3, 32, 128, generator=torch.Generator().manual_seed(3)).to(device)
    loss, attn = model(img, targets, return_loss=True)
    assert attn is None and loss.dim() == 0
    opt.zero_grad()
    loss.backward()
    for name in ("decoder.fc.weight", "decoder.fc.bias", "backbone.blocks.0.attn.qkv.weight", "backbone.blocks.0.mlp.fc1.weight"):
        g = model.arena.g(name)
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, name
    first = None
    for it in range(iterations):
        loss, _ = ft.training_iteration(model, opt, img, targets, 5e-4)
        first = loss.item() if first is None else first
    assert torch.isfinite(loss) and loss.item() < first, (first, loss.item())
    # inference: probabilities, and fwd alone under no_grad
    model.eval()
    with torch.no_grad():
        probs = model(img, None, return_loss=False)
        assert tuple(probs.shape) == (3, 32, 92) and (probs.sum(-1) - 1).abs().max() < 1e-5
        again, _ = model(img, targets, return_loss=True)
    assert torch.isfinite(again)
