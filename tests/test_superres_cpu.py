"""Text super-resolution finetuning, the parts that need neither a GPU nor a kernel: the numpy specification of the loss and of the
bicubic resampling against torch, the backward stencil against a double loop, the YAML, DINO_SuperRes's parameter tree and
checkpoint loading, the refusals, the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sr_np as R
import superres_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "Dino", "configs", "CCD_vision_model_SR.yaml")


@pytest.mark.parametrize("d_loss", [1.0, 0.5])
@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
@pytest.mark.parametrize("kind", ["random", "special"])
def test_specification_is_the_torch_composition(kind, pname, d_loss):
    sr, hr = C.loss_case(C.SHAPES[0], kind)
    C.assert_margin(sr, hr, kind)
    gpw = C.PARAM_SETS[pname]
    st = torch.from_numpy(np.array(sr)).double().requires_grad_(True)
    want = C.torch_loss(st, torch.from_numpy(np.array(hr)).double(), gpw)
    (want * d_loss).backward()
    got = R.sr_loss(sr, hr, gpw, d_loss=d_loss)
    np.testing.assert_allclose(got["loss"], float(want.detach()), rtol=1e-12)
    np.testing.assert_allclose(got["grad"], st.grad.numpy(), rtol=1e-9, atol=1e-16)
    np.testing.assert_allclose(got["parts"][0], got["parts"][1] + gpw * got["parts"][2], rtol=1e-14)
    if kind == "special":
        assert not got["grad"][0].any() and got["mse"][0] == 0.0 and got["gp"][0] == 0.0          # sr == hr: sign(0) = 0


@pytest.mark.parametrize("shape", C.SHAPES[1:])
def test_generated_cases_keep_the_sign_margin(shape):
    sr, hr = C.loss_case(shape, "random")
    C.assert_margin(sr, hr, "random")
    assert sr.dtype == hr.dtype == np.float32 and 0.0 <= min(sr.min(), hr.min()) and max(sr.max(), hr.max()) <= 1.0


def test_empty_batch_is_zero():
    got = R.sr_loss(np.zeros((0, 3, 4, 8)), np.zeros((0, 3, 4, 8)), 1.0)
    assert got["loss"] == 0.0 and got["grad"].shape == (0, 3, 4, 8)


def test_backward_stencil_against_the_double_loop():
    rng = np.random.RandomState(4)
    sr, hr = rng.random_sample((5, 8)), rng.random_sample((5, 8))
    hr[2, 3:6] = sr[2, 3:6]
    got, want = R.gp_backward(sr, hr), R.gp_backward_brute(sr, hr)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    assert np.abs(want).max() > 0.1
    same = R.gp_backward(sr[None], sr[None])
    assert not same.any()                              # sign(0) = 0


def test_numpy_bicubic_is_torch_interpolate():
    """F.interpolate(scale_factor=2, mode='bicubic', align_corners=False) on CPU fp32, atol 2e-6 (16 fp32 roundings on values <= 1.4);
    a constant image comes back constant, the corner impulses see the clamped border."""
    lr, got = C.upsample_case(3)
    want = F.interpolate(torch.from_numpy(np.array(lr)), scale_factor=2, mode="bicubic", align_corners=False).numpy()
    assert got.shape == want.shape == (3, 3, 32, 128)
    np.testing.assert_allclose(got, want, rtol=0, atol=C.UP_ATOL)
    np.testing.assert_allclose(got[1], np.broadcast_to(lr[1][:, :1, :1], (3, 32, 128)), rtol=0, atol=1e-14)
    assert got.min() < 0.0 and got.max() > 1.0           # not clamped
    assert abs(got[2, 0, 0, 0] - want[2, 0, 0, 0]) <= C.UP_ATOL and got[2, 0, 0, 0] > 1.0
    # the two fractions of x2 and their taps, exact multiples of 1/256
    np.testing.assert_array_equal(R.cubic_taps(0.25) * 256, [-27, 225, 67, -9])
    np.testing.assert_array_equal(R.cubic_taps(0.75) * 256, [-9, 67, 225, -27])


def test_yaml_parses():
    from ccd_amd.utils.utils import Config
    from ccd_amd import superres as su
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = Config(YAML)
    finally:
        os.chdir(cwd)
    assert (c.arch, c.patch_size, c.optimizer, c.dataset_scheme, c.model_pretrain_key) == ("vit_small", 4, "adamw", "synthetic", "teacher")
    assert c.sr_loss == {"gp_weight": 0.0001, "ssim_weight": 0.0}
    assert c.dataset_data_aug is False and c.dataset_multiscales is False
    assert su.check_config(c, 1) == "teacher"
    from ccd_amd.model.dino_vision import DINO_SuperRes
    loss = DINO_SuperRes(c).loss
    assert (loss.gp_weight, loss.ssim_weight, loss.ssim) == (1e-4, 0.0, None)


def test_model_builds_on_the_cpu_and_loads_a_pretraining_checkpoint(golden_dir):
    import json
    import Dino  # noqa: F401
    from Dino.model.dino_vision import DINO_SuperRes as Aliased
    from ccd_amd import superres as su
    from ccd_amd.model.dino_vision import DINO_Segment, DINO_SuperRes
    from ccd_amd.parallel import DataParallel
    assert Aliased is DINO_SuperRes
    keys = json.load(open(os.path.join(golden_dir, "state_keys.json")))["vit_small"]
    torch.manual_seed(0)
    model = DINO_SuperRes(su.SuperResConfig(arch="vit_small"))
    want = [[k, [3] + s[1:] if k.startswith("segmentation.cls.") else s, d] for k, s, d in keys["student"]
            if k.startswith(("backbone.", "segmentation."))]
    assert [[k, list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()] == want
    w = model.state_dict()["segmentation.cls.weight"]
    assert tuple(w.shape) == (3, 128, 3, 3) and not w.any() and not model.state_dict()["segmentation.cls.bias"].any()
    assert model.unused_parameter_names() == DINO_Segment(su.SuperResConfig(arch="vit_small")).unused_parameter_names()
    gen = torch.Generator().manual_seed(7)
    fab = lambda table: {"module." + k: (torch.randn(s, generator=gen) if d == "torch.float32" else torch.tensor(3, dtype=torch.int64))
                         for k, s, d in table}
    ckpt = {"student": fab(keys["student"]), "teacher": fab(keys["teacher"])}
    for key, net in (("teacher", model), ("student", DataParallel(model))):        # bare and `module.`-prefixed keys
        missing = su.load_pretrained(net, ckpt, key)
        pre = "module." if net is not model else ""
        assert missing == [pre + "segmentation.cls.weight", pre + "segmentation.cls.bias"]
        for name, v in net.state_dict().items():
            bare = name[len("module."):] if name.startswith("module.") else name
            if bare.startswith("segmentation.cls."):
                assert not v.any(), name
                continue
            src = ckpt["student"] if bare.startswith("segmentation.") else ckpt[key]
            assert torch.equal(v, src["module." + bare]), (key, name)
    with pytest.raises(RuntimeError, match="GPU"):
        model(torch.zeros(1, 3, 16, 64), torch.zeros(1, 3, 32, 128))
    with pytest.raises(RuntimeError, match="GPU"):
        model.forward_sr(torch.zeros(1, 3, 16, 64))


def test_refusals():
    from ccd_amd import ops, superres as su
    from ccd_amd.loss.sr_loss import SRLoss
    from ccd_amd.model.dino_vision import DINO_SuperRes

    class Cfg:
        dataset_scheme, dataset_data_aug, dataset_multiscales, model_pretrain_key = "synthetic", False, False, None
    assert su.check_config(Cfg(), 1) == "teacher"
    with pytest.raises(NotImplementedError, match="one rank.*SyncBatchNorm"):
        su.check_config(Cfg(), 8)
    for attr, value, msg in (("dataset_data_aug", True, "data_aug.*one theta.*follow-up"), ("dataset_multiscales", True, "multiscales"),
                             ("dataset_scheme", "supervised_mask", "superres_pair")):
        c = Cfg()
        setattr(c, attr, value)
        with pytest.raises(NotImplementedError, match=msg):
            su.check_config(c, 1)
    c = Cfg()
    c.dataset_scheme = "superres_pair"
    assert su.check_config(c, 1) == "teacher"
    c.model_pretrain_key = "ema"
    with pytest.raises(ValueError, match="pretrain_key"):
        su.check_config(c, 1)
    for kw, msg in ((dict(gp_weight=-1e-4), "gp_weight"), (dict(gp_weight=float("nan")), "gp_weight"), (dict(gp_weight="1"), "gp_weight"),
                    (dict(gp_weight=True), "gp_weight"), (dict(ssim_weight=-0.5), "ssim_weight"), (dict(ssim_weight=float("inf")), "ssim_weight"),
                    (dict(ssim_weight=None), "ssim_weight")):
        with pytest.raises(ValueError, match=msg):
            SRLoss(**kw)
    assert SRLoss().gp_weight == 1e-4 and SRLoss().ssim_weight == 0.0 and SRLoss(ssim_weight=0.1).ssim is not None
    model = DINO_SuperRes(su.SuperResConfig(arch="vit_tiny"))
    for bad in (torch.zeros(1, 3, 32, 128), torch.zeros(1, 1, 16, 64), torch.zeros(3, 16, 64)):
        with pytest.raises(ValueError, match="TextZoom"):
            model.forward_sr(bad)
    with pytest.raises(ValueError, match="hr must be"):
        model(torch.zeros(2, 3, 16, 64), torch.zeros(2, 3, 16, 64))
    with pytest.raises(ValueError, match="hr must be"):
        model(torch.zeros(2, 3, 16, 64), torch.zeros(1, 3, 32, 128))
    with pytest.raises(NotImplementedError, match="forward_sr"):
        model.forward_mask(torch.zeros(1, 3, 16, 64))
    with pytest.raises(ValueError, match="three taps"):
        from ccd_amd.modules import vision_transformer as vits
        vits.vit_sr_two_blocks = lambda patch_size=16, **kw: vits.VisionTransformer(patch_size=patch_size, embed_dim=128, depth=2,
                                                                                    num_heads=2, qkv_bias=True, **kw)
        try:
            su.build_model(su.SuperResConfig(arch="vit_sr_two_blocks"), "cpu")
        finally:
            del vits.vit_sr_two_blocks


def test_synthetic_pairs_are_seeded_and_sized():
    from ccd_amd import superres as su
    a, b = su.SyntheticPairSet(4, seed=3), su.SyntheticPairSet(4, seed=3)
    lr, hr, label = a[2]
    assert tuple(lr.shape) == (3, 16, 64) and tuple(hr.shape) == (3, 32, 128) and lr.dtype == hr.dtype == torch.float32 and label == ""
    assert torch.equal(lr, b[2][0]) and torch.equal(hr, b[2][1]) and not torch.equal(hr, a[1][1])
    assert 0.0 <= float(lr.min()) and float(lr.max()) <= 1.0 and 0.0 <= float(hr.min()) and float(hr.max()) <= 1.0
    lrs, hrs = su.collate([a[0], None, a[1]])
    assert tuple(lrs.shape) == (2, 3, 16, 64) and tuple(hrs.shape) == (2, 3, 32, 128)
    # LR is a degraded HR: the bicubic base is close to it and not equal
    base = torch.from_numpy(R.bicubic_x2(lrs.numpy())).float()
    mse = float(((base - hrs) ** 2).mean())
    assert 1e-5 < mse < 2e-2, mse


def test_pair_dataset_reads_textzoom_keys(tmp_path):
    import io
    from PIL import Image
    from ccd_amd import superres as su
    from ccd_amd.dataset import lmdb_file
    rng = np.random.RandomState(0)
    records = {b"num-samples": b"2"}
    for i in (1, 2):
        for kind, (h, w) in (("hr", (40, 150)), ("lr", (20, 75))):
            buf = io.BytesIO()
            Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(buf, format="PNG")
            records[f"image_{kind}-{i:09d}".encode()] = buf.getvalue()
        records[f"label-{i:09d}".encode()] = f"word{i}".encode()
    lmdb_file.write_lmdb(str(tmp_path), records)
    ds = su.PairDataset(str(tmp_path))
    lr, hr, label = ds[1]
    assert len(ds) == 2 and tuple(lr.shape) == (3, 16, 64) and tuple(hr.shape) == (3, 32, 128) and label == "word2"


def test_header_declares_and_library_exports_the_entry_points():
    from ccd_amd import _lib
    names = ("ccd_sr_upsample", "ccd_img_gather_fwd", "ccd_img_grad_cols", "ccd_sr_loss_ws_doubles", "ccd_sr_loss_fwd", "ccd_sr_loss_bwd")
    header = open(os.path.join(ROOT, "include", "ccd_hip.h")).read()
    for n in names:
        assert re.search(r"\b(?:int|long)\s+" + n + r"\s*\(", header), n
        assert n in _lib.PROTOTYPES
    assert "seven entry points were added WITHOUT raising ccd_abi_version" in " ".join(header.split()) or \
        "entry points were added WITHOUT raising ccd_abi_version" in " ".join(header.split())
    assert os.path.isfile(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH))           # loads without a GPU; only the host-side size query is called
    assert all(hasattr(lib, n) for n in names)
    assert lib.ccd_sr_loss_ws_doubles(224) == 224 * 6 and lib.ccd_sr_loss_ws_doubles.restype is ctypes.c_long
    impl = open(os.path.join(ROOT, "ccd_amd", "csrc", "abi_impl.h")).read()
    said = re.search(r"int\s+ccd_abi_version\s*\(\s*(?:void)?\s*\)\s*\{\s*return\s+(\w+)\s*;", impl)
    assert said, "ccd_abi_version() in abi_impl.h"
    value = said.group(1)
    if not value.isdigit():
        value = re.search(r"#define\s+" + value + r"\s+(\d+)", header + impl).group(1)
    assert lib.ccd_abi_version() == int(value)
    kinds = [t.elem if hasattr(t, "elem") else t.__name__ for t in _lib.SIGNATURES["ccd_sr_loss_fwd"]]
    assert kinds == ["float", "float", "c_int", "c_int", "c_int", "c_float", "double", "double", "float", "double", "void"]
