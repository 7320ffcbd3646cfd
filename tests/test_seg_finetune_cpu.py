"""Text segmentation finetuning, the parts that need neither a GPU nor a kernel: the numpy specification of the loss against torch,
the edge band against its definition, the YAML, DINO_Segment's parameter tree and checkpoint loading, the refusals, the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_finetune_checks as C
import seg_sup_loss_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "Dino", "configs", "CCD_vision_model_SEG.yaml")


@pytest.mark.parametrize("kind", ["random", "special"])
def test_specification_is_weighted_cross_entropy(kind):
    """edge_weight = 0, dice_weight = 0: F.cross_entropy(weight, ignore_index, reduction='mean') in fp64."""
    z, gt = C.loss_case(C.SHAPES[0], kind)
    for cw in ((1.0, 1.0), (0.3, 1.7)):
        zt = torch.from_numpy(np.array(z)).double().requires_grad_(True)
        want = F.cross_entropy(zt, torch.from_numpy(np.array(gt)).long(), weight=torch.tensor(cw, dtype=torch.float64), ignore_index=255)
        want.backward()
        got = R.seg_sup_loss(z, gt, cw)
        np.testing.assert_allclose(got["loss"], float(want.detach()), rtol=1e-12)
        np.testing.assert_allclose(got["grad"], zt.grad.numpy(), rtol=1e-10, atol=1e-16)
        assert got["parts"][2] > 0 and got["parts"][1] == got["loss"]          # the Dice part is reported, not added


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
@pytest.mark.parametrize("kind", ["random", "special"])
def test_specification_is_the_torch_composition(kind, pname):
    z, gt = C.loss_case(C.SHAPES[0], kind)
    cw, dw, ew, r = C.PARAM_SETS[pname]
    zt = torch.from_numpy(np.array(z)).double().requires_grad_(True)
    want = C.torch_loss(zt, np.array(gt), cw, dw, ew, r)
    (want * 0.5).backward()
    got = R.seg_sup_loss(z, gt, cw, dw, ew, r, d_loss=0.5)
    np.testing.assert_allclose(got["loss"], float(want.detach()), rtol=1e-12)
    np.testing.assert_allclose(got["grad"], zt.grad.numpy(), rtol=1e-9, atol=1e-16)
    pred = np.array(z)[:, 1] > np.array(z)[:, 0]
    assert got["confusion"].sum() == R.scored(gt).sum() and got["confusion"][1, 1] == ((gt == 1) & pred).sum()


def test_specification_without_a_scored_pixel_is_zero():
    z, gt = C.loss_case(C.SHAPES[1], "ignored")
    got = R.seg_sup_loss(z, gt, (0.3, 1.7), 0.5, 2.0, 2)
    assert got["loss"] == 0.0 and not got["grad"].any() and got["parts"].tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("r", [0, 1, 4])
def test_edge_band_against_the_double_loop(r):
    gt = np.zeros((1, 5, 8), np.uint8)
    gt[0, 1:4, 2:5] = 1
    gt[0, 2, 5] = 255                  # an ignored pixel right of the boundary: neither an edge nor a reason for one
    gt[0, 4, 7] = 1
    band = R.edge_band(gt, r)
    np.testing.assert_array_equal(band, R.edge_band_brute(gt, r))
    assert not band[0, 2, 5]
    if r == 0:
        assert not band.any()
    if r == 1:
        assert band[0, 2, 4] and not band[0, 2, 6]      # (2, 6) sees only the ignored pixel within one step, no text
        lone = np.zeros((1, 5, 8), np.uint8)
        lone[0, 2, 3] = 255
        assert not R.edge_band(lone, 1).any()           # an ignored pixel makes no edge
    # the generic case as well
    rnd = np.random.RandomState(3).randint(0, 3, (2, 5, 8)).astype(np.uint8)
    rnd[rnd == 2] = 255
    np.testing.assert_array_equal(R.edge_band(rnd, r), R.edge_band_brute(rnd, r))


def test_yaml_parses():
    from ccd_amd.utils.utils import Config
    from ccd_amd import segment as sg
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = Config(YAML)
    finally:
        os.chdir(cwd)
    assert (c.arch, c.patch_size, c.optimizer, c.dataset_scheme, c.model_pretrain_key) == ("vit_small", 4, "adamw", "synthetic", "teacher")
    assert c.seg_loss == {"class_weight": [1.0, 2.0], "ignore_index": 255, "dice_weight": 0.5, "edge_weight": 1.0, "edge_radius": 2}
    assert c.dataset_data_aug is False and c.dataset_multiscales is False and c.dataset_mask_path == ""
    assert (c.lr, c.min_lr, c.warmup_epochs, c.weight_decay, c.clip_grad) == (0.0005, 0.000001, 1, 0.05, None)
    assert sg.check_config(c, 1) == "teacher"
    from ccd_amd.model.dino_vision import DINO_Segment
    loss = DINO_Segment(c).loss
    assert (loss.class_weight, loss.ignore_index, loss.dice_weight, loss.edge_weight, loss.edge_radius) == ((1.0, 2.0), 255, 0.5, 1.0, 2)


def test_model_builds_on_the_cpu_and_loads_a_pretraining_checkpoint(golden_dir):
    import json
    import Dino  # noqa: F401
    from Dino.model.dino_vision import DINO_Segment as Aliased
    from ccd_amd import segment as sg
    from ccd_amd.model.dino_vision import DINO_Segment
    from ccd_amd.parallel import DataParallel
    assert Aliased is DINO_Segment
    keys = json.load(open(os.path.join(golden_dir, "state_keys.json")))["vit_small"]
    torch.manual_seed(0)
    model = DINO_Segment(sg.SegmentConfig(arch="vit_small"))
    want = [[k, s, d] for k, s, d in keys["student"] if k.startswith(("backbone.", "segmentation."))]
    assert [[k, list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()] == want
    unused = model.unused_parameter_names()
    assert "backbone.cls_token" in unused and sum(n.startswith("segmentation.conv_mla.") for n in unused) == 18
    assert "backbone.blocks.5.attn.qkv.weight" not in unused and "backbone.blocks.6.attn.qkv.weight" in unused   # taps behind blocks 2, 4, 6
    # a pretraining-style checkpoint: {student, teacher}, `module.` prefix; the teacher has no segmentation head
    gen = torch.Generator().manual_seed(7)
    fab = lambda table: {"module." + k: (torch.randn(s, generator=gen) if d == "torch.float32" else torch.tensor(3, dtype=torch.int64))
                         for k, s, d in table}
    ckpt = {"student": fab(keys["student"]), "teacher": fab(keys["teacher"])}
    for key, net in (("teacher", model), ("student", DataParallel(model))):        # bare and `module.`-prefixed keys
        missing = sg.load_pretrained(net, ckpt, key)
        assert missing == []
        for name, v in net.state_dict().items():
            bare = name[len("module."):] if name.startswith("module.") else name
            src = ckpt["student"] if bare.startswith("segmentation.") else ckpt[key]
            assert torch.equal(v, src["module." + bare]), (key, name)
    del ckpt["student"]                # a teacher-only file: the head is reported and stays as it was
    missing = sg.load_pretrained(model, ckpt, "teacher")
    assert missing and all(n.startswith("segmentation.") for n in missing)
    with pytest.raises(RuntimeError, match="GPU"):
        model(torch.zeros(1, 3, 32, 128), torch.zeros(1, 32, 128, dtype=torch.uint8))


def test_refusals():
    from ccd_amd import ops, segment as sg
    from ccd_amd.loss.seg_loss import SegSupLoss

    class Cfg:
        dataset_scheme, dataset_data_aug, dataset_multiscales, model_pretrain_key = "synthetic", False, False, None
    assert sg.check_config(Cfg(), 1) == "teacher"
    with pytest.raises(NotImplementedError, match="one rank.*SyncBatchNorm"):
        sg.check_config(Cfg(), 8)
    for attr, value, msg in (("dataset_data_aug", True, "data_aug.*one theta.*follow-up"), ("dataset_multiscales", True, "multiscales"),
                             ("dataset_scheme", "supervised", "supervised_mask")):
        c = Cfg()
        setattr(c, attr, value)
        with pytest.raises(NotImplementedError, match=msg):
            sg.check_config(c, 1)
    c = Cfg()
    c.model_pretrain_key = "ema"
    with pytest.raises(ValueError, match="pretrain_key"):
        sg.check_config(c, 1)
    for kw, msg in ((dict(class_weight=(1.0,)), "class_weight"), (dict(class_weight=(1.0, -2.0)), "class_weight"),
                    (dict(ignore_index=1), "ignore_index"), (dict(ignore_index=256), "ignore_index"),
                    (dict(dice_weight=-0.1), "dice_weight"), (dict(edge_weight=float("nan")), "edge_weight"),
                    (dict(edge_radius=5), "edge_radius"), (dict(edge_radius=1.5), "edge_radius")):
        with pytest.raises(ValueError, match=msg):
            SegSupLoss(**kw)
    assert ops.seg_sup_params() == (1.0, 1.0, 255, 0.0, 0.0, 0)
    with pytest.raises(ValueError, match="three taps"):
        from ccd_amd.modules import vision_transformer as vits
        vits.vit_seg_two_blocks = lambda patch_size=16, **kw: vits.VisionTransformer(patch_size=patch_size, embed_dim=128, depth=2,
                                                                                     num_heads=2, qkv_bias=True, **kw)
        try:
            sg.build_model(sg.SegmentConfig(arch="vit_seg_two_blocks"), "cpu")
        finally:
            del vits.vit_seg_two_blocks


def test_header_declares_and_library_exports_the_entry_points():
    from ccd_amd import _lib
    names = ("ccd_seg_sup_loss_ws_doubles", "ccd_seg_sup_loss_fwd", "ccd_seg_sup_loss_bwd")
    header = open(os.path.join(ROOT, "include", "ccd_hip.h")).read()
    for n in names:
        assert re.search(r"\b(?:int|long)\s+" + n + r"\s*\(", header), n
        assert n in _lib.PROTOTYPES
    assert "deliberately" in header or "WITHOUT raising ccd_abi_version" in header
    assert os.path.isfile(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH))           # loads without a GPU; only the host-side size query is called
    assert all(hasattr(lib, n) for n in names)
    assert lib.ccd_seg_sup_loss_ws_doubles(224) == 224 * 11 + 3 and lib.ccd_seg_sup_loss_ws_doubles.restype is ctypes.c_long
    kinds = [t.elem if hasattr(t, "elem") else t.__name__ for t in _lib.SIGNATURES["ccd_seg_sup_loss_fwd"]]
    assert kinds == ["float", "c_long", "c_long", "c_int", "uint8_t", "c_long", "c_int", "c_int", "c_int", "c_int", "c_float", "c_float",
                     "c_float", "c_float", "c_int", "double", "uint8_t", "float", "double", "long", "void"]
