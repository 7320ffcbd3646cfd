"""Dino.metric.eval_superpixel on a real MI355X, through libccd_hip.so (run with -m gpu): the reference's recorded outputs, the fp64
restatement on uniform and text-like batches (values and gradients), repeatability, batch invariance and the in-place channel view.
Gates: SSIM / TRI_SSIM <= 2e-6 absolute, PSNR <= 1e-5 dB, input gradients <= 5e-5 relative L2."""
import functools

import numpy as np
import pytest
import torch

from backends import Backend
import superpixel_np as sp

pytestmark = pytest.mark.gpu

SSIM_TOL, PSNR_TOL, GRAD_TOL = 2e-6, 1e-5, 5e-5


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def _fixture_inputs(case, dev):
    return [(torch.from_numpy(case[k].astype(np.float32)) / 255.0).to(dev) for k in ("x1_u8", "x2_u8", "x3_u8")]


def test_superpixel_fixtures(hip, golden_dir):
    from ccd_amd.metric.eval_superpixel import SSIM, TRI_SSIM, calculate_psnr, ssim
    names, cases, _ = sp.load_cases(golden_dir)
    for name in names:
        c = cases[name]
        ws = int(c["ws"])
        x = _fixture_inputs(c, hip.device)
        assert abs(ssim(x[0], x[1], ws).item() - float(c["ssim_mean"])) <= SSIM_TOL, name
        np.testing.assert_allclose(ssim(x[0], x[1], ws, False).cpu().numpy(), c["ssim_img"], rtol=0, atol=SSIM_TOL, err_msg=name)
        assert abs(SSIM(ws)(x[0], x[1]).item() - float(c["SSIM_mean"])) <= SSIM_TOL, name
        np.testing.assert_allclose(SSIM(ws, False)(x[0], x[1]).cpu().numpy(), c["SSIM_img"], rtol=0, atol=SSIM_TOL, err_msg=name)
        assert abs(TRI_SSIM(ws)(*x).item() - float(c["tri_mean"])) <= SSIM_TOL, name
        np.testing.assert_allclose(TRI_SSIM(ws, False)(*x).cpu().numpy(), c["tri_img"], rtol=0, atol=SSIM_TOL, err_msg=name)
        p = calculate_psnr(x[0], x[1])
        assert isinstance(p, torch.Tensor) and p.shape == () and abs(p.item() - float(c["psnr"])) <= PSNR_TOL, name
        assert calculate_psnr(x[0], x[0].clone()) == float("inf")
        if "g_ssim_1" in c:
            leaves = [t.clone().requires_grad_(True) for t in x[:2]]
            ssim(*leaves, ws).backward()
            for i in range(2):
                assert sp.rel_l2(leaves[i].grad, torch.from_numpy(c[f"g_ssim_{i + 1}"])) <= GRAD_TOL, (name, i)
        if "g_tri_1" in c:
            leaves = [t.clone().requires_grad_(True) for t in x]
            TRI_SSIM(ws)(*leaves).backward()
            for i in range(3):
                assert sp.rel_l2(leaves[i].grad, torch.from_numpy(c[f"g_tri_{i + 1}"])) <= GRAD_TOL, (name, i)


@functools.lru_cache(maxsize=1)
def _batches():
    """(label, img1, img2, img3) on the CPU: uniform and text-like images at the issue's shapes."""
    out = []
    for shape in ((64, 4, 32, 128), (256, 3, 32, 128), (256, 3, 16, 64)):
        a = sp.uniform(shape, shape[0] + shape[2])
        out.append((f"uniform{list(shape)}", a, sp.perturbed(a, 3, 0.1), sp.uniform(shape, 4)))
        t = sp.text_like(*shape, seed=shape[2])
        out.append((f"text{list(shape)}", t, sp.perturbed(t, 5, 0.05), sp.perturbed(t, 6, 0.15)))
    return out


@pytest.mark.parametrize("k", range(6))
def test_values_against_restatement(hip, k):
    from ccd_amd.metric.eval_superpixel import SSIM, TRI_SSIM, calculate_psnr, ssim
    label, *x = _batches()[k]
    d = [t.to(hip.device) for t in x]
    C = x[0].shape[1]
    ref3 = [t[:, :3] for t in x]
    # SSIM module: the [:, :3] slice (read in place for the 4-channel batch)
    np.testing.assert_allclose(SSIM(11, False)(d[0], d[1]).cpu().numpy(), sp.ssim(ref3[:2], 11, False).numpy(), rtol=0, atol=SSIM_TOL,
                               err_msg=label)
    assert abs(SSIM()(d[0], d[1]).item() - sp.ssim(ref3[:2], 11).item()) <= SSIM_TOL, label
    # ssim / TRI_SSIM: every channel, size_average both ways
    for ws in (11, 7) if C == 3 else (11,):
        np.testing.assert_allclose(ssim(d[0], d[1], ws, False).cpu().numpy(), sp.ssim(x[:2], ws, False).numpy(), rtol=0,
                                   atol=SSIM_TOL, err_msg=f"{label} ws={ws}")
        assert abs(ssim(d[0], d[1], ws).item() - sp.ssim(x[:2], ws).item()) <= SSIM_TOL
    np.testing.assert_allclose(TRI_SSIM(11, False)(*d).cpu().numpy(), sp.ssim(x, 11, False).numpy(), rtol=0, atol=SSIM_TOL,
                               err_msg=label)
    assert abs(TRI_SSIM()(*d).item() - sp.ssim(x, 11).item()) <= SSIM_TOL
    assert abs(calculate_psnr(d[0], d[1]).item() - sp.psnr(x[0], x[1])[0].item()) <= PSNR_TOL, label


@pytest.mark.parametrize("k", [0, 1, 4, 5])
def test_gradients_against_restatement(hip, k):
    from ccd_amd.metric.eval_superpixel import SSIM, TRI_SSIM
    label, *x = _batches()[k]
    x = [t[:32] for t in x]                      # fp64 autograd of the restatement on the host: 32 images are plenty
    leaves = [t.to(hip.device).requires_grad_(True) for t in x]
    (1 - SSIM()(leaves[0], leaves[1])).backward()
    want = sp.grads(lambda v: 1 - sp.ssim([t[:, :3] for t in v], 11), x[:2])
    for i in range(2):
        assert sp.rel_l2(leaves[i].grad, want[i]) <= GRAD_TOL, (label, i)
    leaves = [t.to(hip.device).requires_grad_(True) for t in x]
    TRI_SSIM(7, False)(*leaves).sum().backward()
    want = sp.grads(lambda v: sp.ssim(v, 7, False).sum(), x)
    for i in range(3):
        assert sp.rel_l2(leaves[i].grad, want[i]) <= GRAD_TOL, (label, i)


def test_repeatable_batch_invariant_and_strided(hip):
    from ccd_amd.metric.eval_superpixel import SSIM, TRI_SSIM, calculate_psnr, ssim
    _, a, b, c = _batches()[0]                   # [64, 4, 32, 128]
    a, b, c = (t.to(hip.device) for t in (a, b, c))
    la, lb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    s1 = SSIM()(la, lb)
    s1.backward()
    g1 = la.grad.clone()
    la.grad = None
    s2 = SSIM()(la, lb)
    s2.backward()
    assert torch.equal(s1, s2) and torch.equal(g1, la.grad)
    # the [:, :3] view against a contiguous copy: forward and gradients bitwise
    ca, cb = a[:, :3].contiguous().requires_grad_(True), b[:, :3].contiguous().requires_grad_(True)
    s3 = ssim(ca, cb)
    s3.backward()
    assert torch.equal(s1, s3) and torch.equal(g1[:, :3], ca.grad) and not g1[:, 3].any()
    assert torch.equal(calculate_psnr(a, b), calculate_psnr(a[:, :3].contiguous(), b[:, :3].contiguous()))
    # per-image values of a batch == the same images one at a time, bitwise
    per = SSIM(size_average=False)(a, b)
    tri = TRI_SSIM(size_average=False)(a, b, c)
    for i in range(0, 64, 7):
        assert torch.equal(per[i:i + 1], SSIM(size_average=False)(a[i:i + 1], b[i:i + 1])), i
        assert torch.equal(tri[i:i + 1], TRI_SSIM(size_average=False)(a[i:i + 1], b[i:i + 1], c[i:i + 1])), i


def test_loss_use_and_no_host_sync(hip):
    from Dino.metric.eval_superpixel import SSIM, TRI_SSIM, ssim
    _, a, b, c = _batches()[0]
    sr = a.to(hip.device).requires_grad_(True)
    hr, c = b.to(hip.device), c.to(hip.device)
    torch.cuda.synchronize()
    # forward and backward of every SSIM variant without one host synchronisation (torch raises on a synchronising call)
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = 1 - SSIM()(sr, hr)
        loss.backward()
        ssim(sr, hr, 7, size_average=False).sum().backward()
        TRI_SSIM(3)(sr, hr, c).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sr.grad is not None and sr.grad.shape == sr.shape and sr.grad[:, :3].abs().sum().item() > 0
