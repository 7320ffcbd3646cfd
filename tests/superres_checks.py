"""Checks of the text super-resolution finetuning path, shared by test_superres_cpu.py (no kernels), test_superres_sim.py (the
kernels under the CPU SIMT executor) and test_superres_gpu.py (-m gpu): the fused loss and the upsample kernel against their
numpy restatement (tests/sr_np.py), the image head against the module's own torch layers, DINO_SuperRes.
The gates of the loss are the ones kernel_checks.check_seg_loss applies to the pretraining loss: loss and parts rtol 1e-5 / atol
1e-6, gradient rtol 1e-3 / atol 1e-9; the head's are check_seghead's 3e-2 / 3e-2; the upsample's atol 2e-6 is 16 fp32 roundings
on values <= 1.4."""
import numpy as np
import torch

import sr_np as R

LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-3, atol=1e-9)
UP_ATOL = 2e-6
PARAM_SETS = {"mse": 0.0, "tsrn": 1e-4, "gp_heavy": 1.0}      # gp_weight; at 1e-4 the MSE gradient hides any error in the stencil
SHAPES = ((3, 3, 32, 128), (1, 3, 8, 32), (300, 3, 4, 8))      # the last: more images than one finish chunk
SIGN_MARGIN = 1e-3
_CASES = {}


def _separate(fixed, free, rng, keep=None):
    """Redraw pixels of `free` (fp32, in place) until |g(fixed) - g(free)| >= 2 SIGN_MARGIN everywhere (outside the images of `keep`):
    a pixel that is too close gets a new right (or, on the border, left) neighbour in `free`, which moves its gradient map."""
    W = free.shape[-1]
    for _ in range(200):
        bad = np.abs(R.gradient_map(fixed) - R.gradient_map(free)) < 2 * SIGN_MARGIN
        if keep is not None:
            bad[keep] = False
        if not bad.any():
            return
        n, c, y, x = np.nonzero(bad)
        x = np.where(x + 1 < W, x + 1, x - 1)
        free[n, c, y, x] = rng.random_sample(len(n)).astype(np.float32)
    raise AssertionError("the generator did not separate the gradient maps")


def loss_case(shape, kind="random", seed=60):
    """(sr, hr) fp32 [N, 3, H, W] in [0, 1], built once per (shape, kind) and shared, with min |g(sr) - g(hr)| >= SIGN_MARGIN (fp64):
    the sign in the gradient does not depend on a rounding.  special (N = 3): image 0 has sr == hr (left out of the margin: its sign
    is exactly 0), image 1 an all-zero sr, image 2 a constant sr."""
    key = (tuple(shape), kind, seed)
    if key not in _CASES:
        N = shape[0]
        rng = np.random.RandomState(seed + 7 * N + shape[2])
        sr = rng.random_sample(shape).astype(np.float32)
        hr = rng.random_sample(shape).astype(np.float32)
        keep = None
        if kind == "special":
            assert N == 3
            sr[0] = hr[0]
            sr[1], sr[2] = 0.0, 0.625
            keep = np.zeros(shape, bool)
            keep[0] = True
        _separate(sr, hr, rng, keep)
        if kind == "special":
            sr[0] = hr[0]
        sr.setflags(write=False)
        hr.setflags(write=False)
        _CASES[key] = (sr, hr)
    return _CASES[key]


def assert_margin(sr, hr, kind):
    lo = 1 if kind == "special" else 0
    margin = R.sign_margin(sr[lo:], hr[lo:])
    assert margin >= SIGN_MARGIN, f"min |g(sr) - g(hr)| = {margin:.3g}: the sign of the gradient-profile term hangs on a rounding"


def _run(dev, sr, hr, gp_weight, d_loss=1.0):
    from ccd_amd import ops
    st, ht = torch.from_numpy(np.array(sr)).to(dev), torch.from_numpy(np.array(hr)).to(dev)
    out = ops.sr_loss_fwd(st, ht, gp_weight)
    return out, ops.sr_loss_bwd(st, ht, gp_weight, grad_scale=d_loss)


def _compare(out, grad, want, what):
    loss, parts, per = out
    print(f"{what}: loss {float(loss):.9g} want {want['loss']:.9g}; parts {parts.cpu().numpy()} want {want['parts']}; "
          f"max |grad err| {np.abs(grad.cpu().numpy() - want['grad']).max():.3g} of max |grad| {np.abs(want['grad']).max():.3g}")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and parts.dtype == torch.float64 and per.dtype == torch.float64
    np.testing.assert_allclose(float(loss), want["loss"], err_msg=what + "/loss", **LOSS_TOL)
    np.testing.assert_allclose(parts.cpu().numpy(), want["parts"], err_msg=what + "/parts", **LOSS_TOL)
    np.testing.assert_allclose(per.cpu().numpy(), np.stack([want["mse"], want["gp"]], axis=1), err_msg=what + "/per image", **LOSS_TOL)
    np.testing.assert_allclose(grad.cpu().numpy().astype(np.float64), want["grad"], err_msg=what + "/grad", **GRAD_TOL)
    assert np.isfinite(grad.cpu().numpy()).all()


def check_loss(dev, shape, kind, pname, d_loss=1.0):
    sr, hr = loss_case(shape, kind)
    assert_margin(sr, hr, kind)
    gpw = PARAM_SETS[pname]
    want = R.sr_loss(sr, hr, gpw, d_loss=d_loss)
    out, grad = _run(dev, sr, hr, gpw, d_loss)
    _compare(out, grad, want, f"sr_loss/{shape}/{kind}/{pname}")
    if kind == "special":
        assert float(grad[0].abs().max()) == 0.0, "sr == hr: the gradient is exactly zero (sign(0) = 0)"
        assert float(out[2][0, 0]) == 0.0 and float(out[2][0, 1]) == 0.0


def check_loss_repeatable(dev):
    sr, hr = loss_case(SHAPES[0], "random")
    a, ga = _run(dev, sr, hr, 1.0)
    b, gb = _run(dev, sr, hr, 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a.ws, b.ws) and torch.equal(ga, gb)


def check_loss_empty(dev):
    from ccd_amd import ops
    from ccd_amd.loss.sr_loss import SRLoss
    e = torch.zeros((0, 3, 8, 32)).to(dev)
    out = ops.sr_loss_fwd(e, e, 1.0)
    assert float(out[0]) == 0.0 and out[1].cpu().tolist() == [0.0, 0.0, 0.0] and tuple(out[2].shape) == (0, 2)
    assert tuple(ops.sr_loss_bwd(e, e, 1.0).shape) == (0, 3, 8, 32)
    z = e.clone().requires_grad_(True)
    loss = SRLoss(1.0)(z, e)
    loss.backward()
    assert float(loss.detach()) == 0.0 and tuple(z.grad.shape) == (0, 3, 8, 32)


def check_loss_autograd(dev):
    """SRLoss through autograd: the gradient scales with the incoming one, last_parts / last_mse are device tensors; with
    ssim_weight the term ssim_weight (1 - SSIM) is added on top of the fused part."""
    from ccd_amd.loss.sr_loss import SRLoss
    from ccd_amd.metric.eval_superpixel import SSIM
    sr, hr = loss_case(SHAPES[1], "random")
    crit = SRLoss(gp_weight=1.0)
    st = torch.from_numpy(np.array(sr)).to(dev).requires_grad_(True)
    ht = torch.from_numpy(np.array(hr)).to(dev)
    loss = crit(st, ht)
    (loss * 3.0).backward()
    want = R.sr_loss(sr, hr, 1.0, d_loss=3.0)
    assert loss.dim() == 0 and crit.last_parts.device == st.device and crit.last_mse.device == st.device
    np.testing.assert_allclose(float(loss.detach()), want["loss"], **LOSS_TOL)
    np.testing.assert_allclose(crit.last_mse.cpu().numpy(), want["mse"], **LOSS_TOL)
    np.testing.assert_allclose(st.grad.cpu().numpy().astype(np.float64), want["grad"], **GRAD_TOL)
    both = SRLoss(gp_weight=1.0, ssim_weight=0.25)
    s2 = st.detach().clone().requires_grad_(True)
    total = both(s2, ht)
    with torch.no_grad():
        term = 0.25 * (1.0 - SSIM()(st.detach(), ht))
    np.testing.assert_allclose(float(total.detach()), float(loss.detach()) + float(term), rtol=1e-5)
    total.backward()
    assert bool(torch.isfinite(s2.grad).all()) and not torch.equal(s2.grad * 3.0, st.grad)


def check_loss_abi(dev):
    """The entry points return -1 (CCD_EINVAL) / -2 (CCD_ESHAPE) for what they do not take and leave canary-filled outputs alone; the
    wrapper refuses a non-contiguous input."""
    import pytest
    from ccd_amd import _lib, ops
    lib = _lib.get()
    N, H, W = 2, 8, 32
    sr, hr = torch.zeros((N, 3, H, W)).to(dev), torch.zeros((N, 3, H, W)).to(dev)
    nws = lib.ccd_sr_loss_ws_doubles(N)
    assert nws == N * 6 and lib.ccd_sr_loss_ws_doubles(0) == 0
    ws, per = torch.full((nws,), 7.0, dtype=torch.float64).to(dev), torch.full((N, 2), 7.0, dtype=torch.float64).to(dev)
    loss, parts = torch.full((1,), 7.0).to(dev), torch.full((3,), 7.0, dtype=torch.float64).to(dev)
    dsr = torch.full((N, 3, H, W), 7.0).to(dev)
    s = _lib.stream()
    fwd = [sr, hr, N, H, W, 1.0, ws, per, loss, parts, s]
    bwd = [sr, hr, N, H, W, 1.0, 1.0, None, dsr, s]

    def untouched():
        return (bool((ws == 7.0).all()) and bool((per == 7.0).all()) and float(loss) == 7.0 and bool((parts == 7.0).all())
                and bool((dsr == 7.0).all()))
    for i, v, want in ((0, None, -1), (1, None, -1), (6, None, -1), (7, None, -1), (8, None, -1), (9, None, -1), (5, -1.0, -1),
                       (5, float("nan"), -1), (2, -1, -2), (3, 0, -2), (3, 33, -2), (4, 30, -2), (4, 132, -2), (4, 0, -2)):
        bad = list(fwd)
        bad[i] = v
        assert lib.ccd_sr_loss_fwd(*bad) == want, (i, v)
        assert untouched(), (i, v)
    for i, v, want in ((0, None, -1), (1, None, -1), (8, None, -1), (5, -2.0, -1), (3, 40, -2), (4, 6, -2), (2, -3, -2)):
        bad = list(bwd)
        bad[i] = v
        assert lib.ccd_sr_loss_bwd(*bad) == want, (i, v)
        assert untouched(), (i, v)
    off = torch.zeros(N * 3 * H * W + 1).to(dev)[1:]                  # a plane that does not start on 16 bytes
    bad = list(fwd)
    bad[0] = off
    assert lib.ccd_sr_loss_fwd(*bad) == -1 and untouched()
    assert lib.ccd_sr_loss_fwd(*fwd) == 0 and lib.ccd_sr_loss_bwd(*bwd) == 0
    assert not untouched() and float(loss) == 0.0 and float(dsr.abs().max()) == 0.0
    # images == 0 is OK: L = 0, nothing else is written
    loss.fill_(7.0)
    assert lib.ccd_sr_loss_fwd(None, None, 0, H, W, 1.0, None, None, loss, parts, s) == 0 and float(loss) == 0.0
    assert lib.ccd_sr_loss_bwd(None, None, 0, H, W, 1.0, 1.0, None, None, s) == 0
    # the upsample and the image tail
    lr, base, xin = torch.zeros((1, 3, 4, 6)).to(dev), torch.full((1, 3, 8, 12), 7.0).to(dev), torch.full((1, 3, 8, 12), 7.0).to(dev)
    up = [lr, 1, 4, 6, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, base, xin, s]
    for i, v, want in ((0, None, -1), (10, None, -1), (11, None, -1), (7, 0.0, -1), (9, float("nan"), -1), (3, 5, -2), (2, 0, -2),
                       (2, 1024, -2), (1, -1, -2)):
        bad = list(up)
        bad[i] = v
        assert lib.ccd_sr_upsample(*bad) == want, (i, v)
        assert bool((base == 7.0).all()) and bool((xin == 7.0).all()), (i, v)
    assert lib.ccd_sr_upsample(*up) == 0 and float(base.abs().max()) == 0.0 and bool((xin == -2.0).all())
    z = torch.zeros((32, 64)).to(dev)
    assert lib.ccd_img_gather_fwd(z, 10, torch.zeros(3).to(dev), torch.zeros(64).to(dev), torch.zeros(64).to(dev), 1, 4, 16, s) == -2
    assert lib.ccd_img_gather_fwd(z, 64, None, None, None, 1, 4, 16, s) == -1
    assert lib.ccd_img_grad_cols(None, None, 1, 4, 16, s) == -1
    # the wrappers' host-side checks
    with pytest.raises(ValueError, match="contiguous"):
        ops.sr_loss_fwd(torch.zeros((N, 3, W, H)).to(dev).transpose(2, 3), hr)
    with pytest.raises(ValueError, match="contiguous"):
        ops.sr_loss_bwd(sr, torch.zeros((N, 6, H, W)).to(dev)[:, ::2])
    with pytest.raises(ValueError, match="W % 4"):
        ops.sr_loss_fwd(torch.zeros((1, 3, 4, 6)).to(dev), torch.zeros((1, 3, 4, 6)).to(dev))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        ops.sr_loss_fwd(torch.zeros((1, 2, 4, 8)).to(dev), torch.zeros((1, 2, 4, 8)).to(dev))
    with pytest.raises(TypeError, match="float32"):
        ops.sr_loss_fwd(sr.double(), hr.double())
    with pytest.raises(ValueError, match="even w"):
        ops.sr_upsample(torch.zeros((1, 3, 4, 5)).to(dev), (0.5,) * 3, (0.25,) * 3)


# ------------------------------------------------------------------------------------------------ torch restatement (CPU, fp64)
def torch_loss(sr, hr, gp_weight):
    """The formula composed from torch ops with autograd: sr a leaf tensor [N, 3, H, W] -> the loss."""
    import torch.nn.functional as F

    def gmap(x):
        p = F.pad(x, (1, 1, 1, 1))
        a = 0.5 * (p[..., 1:-1, 2:] - p[..., 1:-1, :-2])
        b = 0.5 * (p[..., :-2, 1:-1] - p[..., 2:, 1:-1])
        return torch.sqrt(a * a + b * b + R.GP_EPS)
    mse = ((sr - hr) ** 2).flatten(1).mean(1)
    gp = (gmap(sr) - gmap(hr)).abs().flatten(1).mean(1)
    return (mse + gp_weight * gp).mean()


# ------------------------------------------------------------------------------------------------ upsample
def upsample_case(N):
    """lr fp32 [N, 3, 16, 64] in [0, 1]: image 0 random; (N = 3) image 1 constant per channel, image 2 an impulse at each corner."""
    key = ("up", N)
    if key not in _CASES:
        rng = np.random.RandomState(80 + N)
        lr = rng.random_sample((N, 3, 16, 64)).astype(np.float32)
        if N >= 3:
            lr[1] = np.array([0.7, 0.1, 1.0], np.float32)[:, None, None]
            lr[2] = 0.0
            for c, (y, x) in enumerate(((0, 0), (0, 63), (15, 0))):
                lr[2, c, y, x] = 1.0
            lr[2, 0, 15, 63] = 1.0
        lr.setflags(write=False)
        _CASES[key] = (lr, R.bicubic_x2(lr))
    return _CASES[key]


def check_upsample(dev, N):
    from ccd_amd import ops
    from ccd_amd.dataset.datasetsupervised_kmeans import MEAN, STD
    lr, want = upsample_case(N)
    base, xin = ops.sr_upsample(torch.from_numpy(np.array(lr)).to(dev), MEAN, STD)
    assert base.dtype == xin.dtype == torch.float32 and tuple(base.shape) == tuple(xin.shape) == (N, 3, 32, 128)
    got = base.cpu().numpy()
    print(f"sr_upsample N={N}: max err {np.abs(got - want).max():.3g}, range [{got.min():.4f}, {got.max():.4f}]")
    np.testing.assert_allclose(got, want, rtol=0, atol=UP_ATOL)
    assert got.min() < 0.0 and got.max() > 1.0, "the result is not clamped: the fixture overshoots on both sides"
    norm = (got - np.array(MEAN, np.float32)[:, None, None]) / np.array(STD, np.float32)[:, None, None]
    np.testing.assert_allclose(xin.cpu().numpy(), norm, rtol=0, atol=1e-6)
    if N >= 3:
        assert (got[1] == lr[1][:, :1, :1]).all(), "a constant plane comes back constant, bit for bit"


# ------------------------------------------------------------------------------------------------ the image head
def _unit(got, want):
    s = float(want.abs().max())
    return got.detach().float().cpu() / s, want.detach().float().cpu() / s


def check_sr_head(dev, images=1, E=64, seed=27, train=True):
    """seghead.sr_head_forward (train: batch statistics, gradients) / sr_head_inference (eval: running statistics, nothing updated)
    against the module's own torch layers plus base on the CPU in fp32, random cls weights.  check_seghead's gate 3e-2 / 3e-2 on sr
    and on the gradients into the taps, cls.weight and cls.bias, which also get check_seghead's cosine / norm-ratio bounds."""
    import copy
    from ccd_amd import seghead as sh
    from ccd_amd.modules.segmentor import SegHead
    from kernel_checks import BF, _cos, close, rnd
    torch.manual_seed(seed)
    ref = SegHead(in_channels=E, num_classes=3).float()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
                m.momentum = 0.5
        if not train:                               # running statistics of three batches that are not the one under test
            ref.train()
            for _ in range(3):
                xs = [rnd((2, E, 8, 32), g, 1.3) + 0.2 for _ in range(3)]
                ref.cls(ref.unpool2(ref.unpool1(ref.mlahead(*xs))))
    ref.train(train)
    head = copy.deepcopy(ref).to(dev)
    taps = [rnd((images * 256, E), g).to(BF) for _ in range(3)]
    base = torch.rand((images, 3, 32, 128), generator=g)
    rin = [t.float().view(images, 8, 32, E).permute(0, 3, 1, 2).contiguous().detach().requires_grad_(train) for t in taps]
    if not train:
        head.train()                                # whatever mode the head is in
        before = {k: v.detach().clone() for k, v in head.named_buffers()}
        sr = sh.sr_head_inference(head, [t.to(dev) for t in taps], images, base.to(dev))
        with torch.no_grad():
            want = ref.cls(ref.unpool2(ref.unpool1(ref.mlahead(*rin)))) + base
        assert not sr.requires_grad and all(torch.equal(v, before[k]) for k, v in head.named_buffers()), "a statistic changed"
    else:
        tin = [t.to(dev).requires_grad_(True) for t in taps]
        sr = sh.sr_head_forward(head, tin, images, base.to(dev))
        want = ref.cls(ref.unpool2(ref.unpool1(ref.mlahead(*rin)))) + base
    assert sr.dtype == torch.float32 and tuple(sr.shape) == (images, 3, 32, 128)
    print(f"sr head ({'train' if train else 'eval'}): max err {(sr.detach().cpu() - want.detach()).abs().max().item():.4g} of residual max "
          f"{(want.detach() - base).abs().max().item():.4g}")
    close(sr, want, 3e-2, 3e-2, "sr head/sr")
    if not train:
        return
    dl = rnd(tuple(want.shape), g) / want[0].numel()
    want.backward(dl)
    sr.backward(dl.to(dev))
    refp = dict(ref.named_parameters())
    pairs = [(f"d_tap{i}", tin[i].grad, rin[i].grad.permute(0, 2, 3, 1).reshape(images * 256, E)) for i in range(3)]
    pairs += [(n, dict(head.named_parameters())[n].grad, refp[n].grad) for n in ("cls.weight", "cls.bias")]
    for name, got, wg in pairs:
        c, ratio = _cos(got, wg), float(got.float().norm().cpu() / wg.norm())
        print(f"{name}: cos {c:.5f} ratio {ratio:.4f}")
        close(got, wg, 3e-2, 3e-2, f"sr head/{name}")
        # these gradients are far below 3e-2, so the gate above says little: what binds is check_seghead's own bound on a gradient
        # (direction and norm; the bf16 chain under the taps reaches cos 0.995 on the two-class path as well), and for the
        # classifier, which sits on top of the chain, the gate on the gradient scaled to unit maximum
        assert c > 0.99 and (0.97 if name.startswith("d_tap") else 0.95) < ratio < (1.03 if name.startswith("d_tap") else 1.05), \
            f"sr head/{name}: cos {c}, norm ratio {ratio}"
        if name.startswith("cls."):
            close(*_unit(got, wg), 3e-2, 3e-2, f"sr head/{name} (unit maximum)")


# ------------------------------------------------------------------------------------------------ the model
def model_batch(B=2, seed=5):
    from ccd_amd import superres as su
    ds = su.SyntheticPairSet(B, seed=seed)
    return su.collate([ds[i] for i in range(B)])


def check_model(dev, B=2):
    from ccd_amd import ops, superres as su
    from ccd_amd.dataset.datasetsupervised_kmeans import MEAN, STD
    from seg_finetune_checks import SEG_ARCH, register_arch
    register_arch()
    torch.manual_seed(11)
    model = su.build_model(su.SuperResConfig(arch=SEG_ARCH, drop_path_rate=0.0, gp_weight=1e-4), dev)
    opt = su.make_optimizer(model, lr=1e-3, weight_decay=0.05)
    lr, hr = model_batch(B)
    lr, hr = lr.to(dev), hr.to(dev)
    base = ops.sr_upsample(lr, MEAN, STD)[0]
    # at initialisation the classifier is zero: sr is the bicubic base, bit for bit
    assert not model.segmentation.cls.weight.detach().any() and not model.segmentation.cls.bias.detach().any()
    first_sr = model.forward_sr(lr)
    assert first_sr.dtype == torch.float32 and tuple(first_sr.shape) == (B, 3, 32, 128) and model.training
    assert torch.equal(first_sr, base.clamp(0.0, 1.0)), "forward_sr at initialisation is clamp(base, 0, 1)"
    assert torch.equal(model(lr, return_loss=False), first_sr)
    # the loss of forward_train is SRLoss on the unclamped sr the model produced (= base at initialisation)
    tracked = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    loss = su.training_iteration(model, opt, lr, hr, 1e-3)
    assert torch.equal(model.last_sr, base) and not model.last_sr.requires_grad
    want = R.sr_loss(base.cpu().numpy(), hr.cpu().numpy(), 1e-4)
    np.testing.assert_allclose(float(loss), want["loss"], **LOSS_TOL)
    assert model.loss.last_mse.device == lr.device and tuple(model.loss.last_mse.shape) == (B,)
    assert any(not torch.equal(v, model.state_dict()[k]) for k, v in tracked.items()), "training updates the running statistics"
    # one iteration makes cls.weight non-zero and changes forward_sr
    assert bool(model.segmentation.cls.weight.detach().any())
    tracked = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    second_sr = model.forward_sr(lr)
    assert not torch.equal(second_sr, first_sr) and float(second_sr.min()) >= 0.0 and float(second_sr.max()) <= 1.0
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in tracked.items()), "forward_sr touched the BatchNorm statistics"
    # a second iteration reaches the backbone (the first one's zero classifier passes no gradient below itself)
    su.training_iteration(model, opt, lr, hr, 1e-3)
    for i in range(3):
        gq = model.arena.g(f"backbone.blocks.{i}.attn.qkv.weight")
        assert bool(torch.isfinite(gq).all()) and float(gq.abs().max()) > 0.0, f"block {i}: qkv.weight.grad"
    unused = model.unused_parameter_names()
    assert "backbone.cls_token" in unused and sum(n.startswith("segmentation.conv_mla.") for n in unused) == 18
    for n in unused:
        assert float(model.arena.g(n).abs().max()) == 0.0, n
    res = su.evaluate(model, [(lr, hr)], dev)
    assert res["n_images"] == B and all(np.isfinite(res[k]) for k in ("psnr", "ssim", "bicubic_psnr", "bicubic_ssim"))
    import pytest
    with pytest.raises(ValueError, match="TextZoom"):
        model.forward_sr(hr)
    with pytest.raises(ValueError, match="hr must be"):
        model(lr, lr)


def check_model_stops_at_last_tap(dev, B=1):
    """A backbone with a block behind its last tap: the block keeps its parameters, gets no gradient and is listed as unused."""
    from ccd_amd import superres as su
    from seg_finetune_checks import SEG_ARCH, register_arch4
    register_arch4()
    torch.manual_seed(12)
    deep = su.build_model(su.SuperResConfig(arch=SEG_ARCH + "_4", drop_path_rate=0.1, gp_weight=1.0), dev)
    assert deep.backbone.spec.depth == 3 and len(deep.backbone.blocks) == 4
    with torch.no_grad():
        deep.segmentation.cls.weight.normal_(0.0, 0.05)          # (a zero classifier passes no gradient below itself)
    deep.arena.stale = True
    deep.ensure_arena()
    lr, hr = model_batch(B, seed=9)
    opt = su.make_optimizer(deep, lr=1e-3)
    loss = deep(lr.to(dev), hr.to(dev))
    opt.zero_grad()
    loss.backward()
    assert bool(torch.isfinite(loss.detach()))
    unused = set(deep.unused_parameter_names())
    for n, _ in deep.named_parameters():
        behind = n.startswith("backbone.blocks.3.") or n.startswith("backbone.norm.")
        assert (n in unused) == (behind or n == "backbone.cls_token" or n.startswith("segmentation.conv_mla.")), n
        if behind:
            assert float(deep.arena.g(n).abs().max()) == 0.0, n
    assert float(deep.arena.g("backbone.blocks.2.attn.qkv.weight").abs().max()) > 0.0
