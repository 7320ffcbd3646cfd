"""Dino.metric.eval_superpixel without a GPU: the fp64 restatement (tests/superpixel_np.py) against the reference's recorded outputs
(tests/golden/superpixel_cases.npz), the host-side windows bit-equal to the reference's, and the module's error contract."""
import numpy as np
import pytest
import torch

import superpixel_np as sp


def _inputs(case):
    return [torch.from_numpy(case[k].astype(np.float32)) / 255.0 for k in ("x1_u8", "x2_u8", "x3_u8")]


def test_restatement_matches_reference_fixtures(golden_dir):
    names, cases, _ = sp.load_cases(golden_dir)
    assert len(names) >= 8
    for name in names:
        case = cases[name]
        ws = int(case["ws"])
        x = _inputs(case)
        np.testing.assert_allclose(sp.ssim(x[:2], ws).item(), case["ssim_mean"], rtol=0, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(sp.ssim(x[:2], ws, False).numpy(), case["ssim_img"], rtol=0, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(sp.ssim([t[:, :3] for t in x[:2]], ws).item(), case["SSIM_mean"], rtol=0, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(sp.ssim([t[:, :3] for t in x[:2]], ws, False).numpy(), case["SSIM_img"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(sp.ssim(x, ws).item(), case["tri_mean"], rtol=0, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(sp.ssim(x, ws, False).numpy(), case["tri_img"], rtol=0, atol=2e-6, err_msg=name)
        p, _ = sp.psnr(x[0], x[1])
        np.testing.assert_allclose(float(p), case["psnr"], rtol=0, atol=1e-5, err_msg=name)
        assert sp.psnr(x[0], x[0].clone())[0] == float("inf") and case["psnr_same"] == np.inf
        if "g_ssim_1" in case:
            g = sp.grads(lambda v: sp.ssim(v, ws), x[:2])
            for i in range(2):
                assert sp.rel_l2(torch.from_numpy(case[f"g_ssim_{i + 1}"]), g[i]) < 2e-5, (name, i)
        if "g_tri_1" in case:
            g = sp.grads(lambda v: sp.ssim(v, ws), x)
            for i in range(3):
                assert sp.rel_l2(torch.from_numpy(case[f"g_tri_{i + 1}"]), g[i]) < 2e-5, (name, i)


def test_fixture_covers_the_issue_cases(golden_dir):
    names, cases, windows = sp.load_cases(golden_dir)
    shapes = {tuple(cases[n]["x1_u8"].shape) for n in names}
    assert {(2, 3, 32, 128), (2, 4, 16, 64), (1, 1, 7, 13)} <= shapes
    assert {3, 7, 11} <= {int(cases[n]["ws"]) for n in names}
    # the 4-channel case pins SSIM's [:, :3] slice: it differs from ssim over all four channels
    low = cases["lowres_ws11"]
    assert abs(float(low["SSIM_mean"]) - float(low["ssim_mean"])) > 1e-4
    # a plane smaller than the window
    tiny = cases["tiny_ws11"]
    assert min(tiny["x1_u8"].shape[2:]) < int(tiny["ws"])
    assert all(f"g_tri_{i}" in cases["lowres_ws11"] for i in (1, 2, 3))
    assert set(windows) >= {3, 7, 11}


def test_windows_bit_equal_to_reference(golden_dir):
    from ccd_amd.metric.eval_superpixel import create_window, gaussian
    _, _, windows = sp.load_cases(golden_dir)
    for ws, (g, w) in windows.items():
        got = gaussian(ws, 1.5)
        assert got.dtype == torch.float32 and got.shape == (ws,)
        np.testing.assert_array_equal(got.numpy(), g)
        win = create_window(ws, 3)
        assert win.dtype == torch.float32 and tuple(win.shape) == (3, 1, ws, ws)
        np.testing.assert_array_equal(win.numpy(), w)
        # the separable kernels rely on exactly symmetric taps
        np.testing.assert_array_equal(got.numpy(), got.numpy()[::-1])


def test_modules_have_no_state_and_import_paths():
    import Dino.metric.eval_superpixel as D
    from ccd_amd.metric import eval_superpixel as mine
    from Dino.metric.eval_superpixel import SSIM, TRI_SSIM, calculate_psnr, create_window, gaussian, ssim  # noqa: F401
    assert D is mine
    assert SSIM().state_dict() == {} and TRI_SSIM(7, False).state_dict() == {}
    assert list(SSIM().parameters()) == [] and SSIM(7).window_size == 7 and not SSIM(3, False).size_average


def test_contract_errors_before_any_device_work():
    from ccd_amd.metric.eval_superpixel import SSIM, TRI_SSIM, calculate_psnr, ssim
    a = torch.rand(2, 3, 16, 20)
    with pytest.raises(ValueError):
        ssim(a, torch.rand(2, 3, 16, 21))
    with pytest.raises(ValueError):
        SSIM()(a, torch.rand(1, 3, 16, 20))
    with pytest.raises(ValueError):
        TRI_SSIM()(a, a, torch.rand(2, 2, 16, 20))
    with pytest.raises(ValueError):
        calculate_psnr(a, torch.rand(2, 3, 16))
    with pytest.raises(ValueError):
        ssim(a[0], a[0])
    for ws in (0, 2, 10, 17, 11.0):
        with pytest.raises(ValueError):
            ssim(a, a, window_size=ws)
    with pytest.raises(TypeError):
        ssim(a.double(), a.double())
    with pytest.raises(TypeError):
        SSIM()(a.half(), a.half())
    with pytest.raises(TypeError):
        calculate_psnr(a, a.to(torch.bfloat16))
    with pytest.raises(TypeError):
        TRI_SSIM()(a, a, a.double())


def test_cpu_tensors_raise_runtime_error():
    from ccd_amd import _lib
    from ccd_amd.metric.eval_superpixel import SSIM, calculate_psnr, ssim
    assert _lib._stream_override is None
    a = torch.rand(1, 3, 16, 20)
    for f in (lambda: ssim(a, a), lambda: SSIM()(a, a), lambda: calculate_psnr(a, a)):
        with pytest.raises(RuntimeError, match="GPU"):
            f()
