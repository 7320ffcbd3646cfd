"""Checks of the text-segmentation finetuning path, shared by test_seg_finetune_cpu.py (no kernels), test_seg_finetune_sim.py (the
kernels under the CPU SIMT executor) and test_seg_finetune_gpu.py (-m gpu): the fused supervised loss against its numpy
restatement (tests/seg_sup_loss_np.py), the eval-mode segmentation head against the module's own torch layers, DINO_Segment.
The gates of the loss are the ones kernel_checks.check_seg_loss applies to the pretraining loss: loss and parts rtol 1e-5 / atol
1e-6, gradient rtol 1e-3 / atol 1e-9; the head's is check_seghead's 3e-2 / 3e-2."""
import ctypes

import numpy as np
import torch

import seg_sup_loss_np as R

LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-3, atol=1e-9)
# (class_weight, dice_weight, edge_weight, edge_radius)
PARAM_SETS = {"plain": ((1.0, 1.0), 0.0, 0.0, 0), "full": ((0.3, 1.7), 0.5, 2.0, 2), "r4": ((1.0, 1.0), 0.0, 1.0, 4)}
SHAPES = ((3, 32, 128), (1, 8, 32))
_CASES = {}


def loss_case(shape, kind="random", seed=40):
    """(logits fp32 [N, 2, H, W] ~ 2 N(0, 1) without an arg-max tie, gt uint8 [N, H, W]), built once per (shape, kind) and shared.
    random: 0 / 1 with about 5 % ignored; special: image 0 all ignored, image 1 all text, image 2 all background (N = 3)."""
    key = (tuple(shape), kind, seed)
    if key not in _CASES:
        N, H, W = shape
        rng = np.random.RandomState(seed + 7 * N + H)
        z = (2.0 * rng.standard_normal((N, 2, H, W))).astype(np.float32)
        assert not (z[:, 0] == z[:, 1]).any(), "an arg-max tie in continuous draws"
        gt = (rng.random_sample((N, H, W)) < 0.4).astype(np.uint8)
        gt[rng.random_sample((N, H, W)) < 0.05] = 255
        if kind == "special":
            assert N == 3
            gt[0], gt[1], gt[2] = 255, 1, 0
        elif kind == "ignored":
            gt[:] = 255
        z.setflags(write=False)
        gt.setflags(write=False)
        _CASES[key] = (z, gt)
    return _CASES[key]


def _run(dev, z, gt, params, d_loss=1.0):
    from ccd_amd import ops
    cw, dw, ew, r = params
    zt = z if torch.is_tensor(z) else torch.from_numpy(np.array(z)).to(dev)
    out = ops.seg_sup_loss(zt, torch.from_numpy(np.array(gt)).to(dev), cw, 255, dw, ew, r)
    grad = ops.seg_sup_loss_bwd(zt, out.code, out.ws, cw, dw, ew, grad_scale=d_loss)
    return out, grad


def _compare(out, grad, want, what):
    loss, parts, cm = out
    print(f"{what}: loss {float(loss):.9g} want {want['loss']:.9g}; parts {parts.cpu().numpy()} want {want['parts']}; "
          f"max |grad err| {np.abs(grad.cpu().numpy() - want['grad']).max():.3g} of max |grad| {np.abs(want['grad']).max():.3g}")
    assert loss.dtype == torch.float32 and parts.dtype == torch.float64 and cm.dtype == torch.int64 and tuple(cm.shape) == (2, 2)
    np.testing.assert_allclose(float(loss), want["loss"], err_msg=what + "/loss", **LOSS_TOL)
    np.testing.assert_allclose(parts.cpu().numpy(), want["parts"], err_msg=what + "/parts", **LOSS_TOL)
    np.testing.assert_allclose(grad.cpu().numpy().astype(np.float64), want["grad"], err_msg=what + "/grad", **GRAD_TOL)
    np.testing.assert_array_equal(cm.cpu().numpy(), want["confusion"], err_msg=what + "/confusion")
    assert np.isfinite(grad.cpu().numpy()).all()


def check_loss(dev, shape, kind, pname, d_loss=1.0):
    z, gt = loss_case(shape, kind)
    cw, dw, ew, r = PARAM_SETS[pname]
    want = R.seg_sup_loss(z, gt, cw, dw, ew, r, d_loss=d_loss)
    out, grad = _run(dev, z, gt, PARAM_SETS[pname], d_loss)
    _compare(out, grad, want, f"seg_sup_loss/{shape}/{kind}/{pname}")
    code = out.code.cpu().numpy()
    np.testing.assert_array_equal(code & 3, np.where(gt == 0, 1, np.where(gt == 1, 2, 0)))
    np.testing.assert_array_equal((code & 4) != 0, R.edge_band(gt, r))


def check_loss_channel_stride(dev, pname="full"):
    """Logits viewed with a channel stride - channels 1..2 of a [N, 4, H, W] buffer - are read in place and give the same result."""
    z, gt = loss_case(SHAPES[0], "random")
    wide = torch.full((z.shape[0], 4) + z.shape[2:], 9.0)
    wide[:, 1:3] = torch.from_numpy(np.array(z))
    wide = wide.to(dev)
    view = wide[:, 1:3]
    assert not view.is_contiguous()
    from ccd_amd import ops
    assert ops._seg_sup_logits(view, "t")[0].data_ptr() == view.data_ptr(), "the slice was copied"
    out, grad = _run(dev, view, gt, PARAM_SETS[pname])
    ref, ref_grad = _run(dev, z, gt, PARAM_SETS[pname])
    _compare(out, grad, R.seg_sup_loss(z, gt, *PARAM_SETS[pname]), "seg_sup_loss/channel stride")
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2]) and torch.equal(grad, ref_grad)


def check_loss_repeatable(dev):
    z, gt = loss_case(SHAPES[0], "random")
    a, ga = _run(dev, z, gt, PARAM_SETS["full"])
    b, gb = _run(dev, z, gt, PARAM_SETS["full"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ga, gb) and torch.equal(a.ws, b.ws)


def check_loss_all_ignored(dev):
    z, gt = loss_case(SHAPES[0], "ignored")
    for pname in PARAM_SETS:
        out, grad = _run(dev, z, gt, PARAM_SETS[pname])
        assert float(out[0]) == 0.0 and out[1].cpu().tolist() == [0.0, 0.0, 0.0, 0.0] and int(out[2].sum()) == 0
        assert not torch.isnan(grad).any() and float(grad.abs().max()) == 0.0


def check_loss_autograd(dev):
    """SegSupLoss through autograd: the gradient scales with the incoming one, last_parts / last_confusion are device tensors,
    values other than 0 / 1 / ignore_index are not scored."""
    from ccd_amd.loss.seg_loss import SegSupLoss
    z, gt = loss_case(SHAPES[1], "random")
    gt = np.array(gt)
    gt[0, 0, :3] = 7                                     # not a class and not ignore_index: treated as ignored
    cw, dw, ew, r = PARAM_SETS["full"]
    crit = SegSupLoss(cw, 255, dw, ew, r)
    zt = torch.from_numpy(np.array(z)).to(dev).requires_grad_(True)
    loss = crit(zt, torch.from_numpy(gt).to(dev))
    (loss * 3.0).backward()
    want = R.seg_sup_loss(z, gt, cw, dw, ew, r, d_loss=3.0)
    assert loss.dim() == 0 and crit.last_parts.device == zt.device and crit.last_confusion.device == zt.device
    np.testing.assert_allclose(float(loss.detach()), want["loss"], **LOSS_TOL)
    np.testing.assert_allclose(zt.grad.cpu().numpy().astype(np.float64), want["grad"], **GRAD_TOL)
    np.testing.assert_array_equal(crit.last_confusion.cpu().numpy(), want["confusion"])


def check_loss_abi(dev):
    """The entry points return -1 (CCD_EINVAL) / -2 (CCD_ESHAPE) for what they do not take and leave canary-filled outputs alone."""
    from ccd_amd import _lib
    lib = _lib.get()
    N, H, W = 2, 8, 32
    z = torch.zeros((N, 2, H, W)).to(dev)
    gt = torch.zeros((N, H, W), dtype=torch.uint8).to(dev)
    nws = lib.ccd_seg_sup_loss_ws_doubles(N)
    assert nws == N * 11 + 3 and lib.ccd_seg_sup_loss_ws_doubles(0) == 0
    ws = torch.full((nws,), 7.0, dtype=torch.float64).to(dev)
    code = torch.full((N, H, W), 9, dtype=torch.uint8).to(dev)
    loss, parts = torch.full((1,), 7.0).to(dev), torch.full((4,), 7.0, dtype=torch.float64).to(dev)
    cm = torch.full((2, 2), 7, dtype=torch.int64).to(dev)
    dz = torch.full((N, 2, H, W), 7.0).to(dev)
    s = _lib.stream()
    fwd = [z, 2 * H * W, H * W, 2, gt, H * W, N, H, W, 255, 1.0, 1.0, 0.0, 0.0, 0, ws, code, loss, parts, cm, s]
    bwd = [z, 2 * H * W, H * W, 2, code, N, H, W, 1.0, 1.0, 0.0, 0.0, ws, 1.0, None, dz, s]

    def untouched():
        return (bool((ws == 7.0).all()) and bool((code == 9).all()) and float(loss) == 7.0 and bool((parts == 7.0).all())
                and bool((cm == 7).all()) and bool((dz == 7.0).all()))
    big = torch.zeros((1, 2, 128, 128)).to(dev)
    for i, v, want in ((0, None, -1), (4, None, -1), (15, None, -1), (17, None, -1), (18, None, -1), (19, None, -1), (1, -4, -1),
                       (2, 6, -1), (9, 1, -1), (9, 256, -1), (10, -1.0, -1), (12, float("nan"), -1), (13, -0.5, -1),
                       (3, 3, -2), (6, 0, -2), (8, 30, -2), (14, 5, -2), (14, -1, -2)):
        bad = list(fwd)
        bad[i] = v
        assert lib.ccd_seg_sup_loss_fwd(*bad) == want, (i, v)
        assert untouched(), (i, v)
    bad = list(fwd)
    bad[0], bad[7], bad[8] = big, 128, 128                # H * W > 8192
    assert lib.ccd_seg_sup_loss_fwd(*bad) == -2 and untouched()
    for i, v, want in ((0, None, -1), (4, None, -1), (12, None, -1), (15, None, -1), (3, 1, -2), (7, 3, -2), (5, 0, -2)):
        bad = list(bwd)
        bad[i] = v
        assert lib.ccd_seg_sup_loss_bwd(*bad) == want, (i, v)
        assert untouched(), (i, v)
    assert lib.ccd_seg_sup_loss_fwd(*fwd) == 0 and lib.ccd_seg_sup_loss_bwd(*bwd) == 0
    assert not untouched() and cm.cpu().tolist() == [[N * H * W, 0], [0, 0]]
    np.testing.assert_allclose(float(loss), np.log(2.0), rtol=1e-6)
    # the wrapper's host-side checks
    from ccd_amd import ops
    import pytest
    with pytest.raises(TypeError, match="uint8"):
        ops.seg_sup_loss(z, gt.int())
    with pytest.raises(ValueError, match="W % 4"):
        ops.seg_sup_loss(torch.zeros((1, 2, 4, 6)).to(dev), torch.zeros((1, 4, 6), dtype=torch.uint8).to(dev))
    with pytest.raises(ValueError, match=r"\[N >= 1, 2, H, W\]"):
        ops.seg_sup_loss(torch.zeros((1, 3, 4, 8)).to(dev), torch.zeros((1, 4, 8), dtype=torch.uint8).to(dev))


# ------------------------------------------------------------------------------------------------ torch restatement (CPU, fp64)
def torch_loss(z, gt, class_weight, dice_weight, edge_weight, edge_radius):
    """The formula composed from torch ops with autograd (fp64): z a leaf tensor [N, 2, H, W], gt a uint8 array -> the loss."""
    import torch.nn.functional as F
    valid = torch.from_numpy(R.scored(gt))
    y = torch.from_numpy((gt == 1).astype(np.int64))
    logp = F.log_softmax(z, dim=1)
    l = -logp.gather(1, y[:, None]).squeeze(1)
    p = torch.softmax(z, dim=1)[:, 1]
    w = torch.tensor(class_weight, dtype=z.dtype)[y] * (1.0 + edge_weight * torch.from_numpy(R.edge_band(gt, edge_radius)).to(z.dtype))
    w = w * valid
    omega = w.sum()
    ce = (w * l).sum() / omega if float(omega) > 0 else z.sum() * 0.0
    yf, vf = y.to(z.dtype), valid.to(z.dtype)
    I, P, G = (p * yf * vf).flatten(1).sum(1), (p * vf).flatten(1).sum(1), (yf * vf).flatten(1).sum(1)
    has = valid.flatten(1).any(1)
    dice_n = 1.0 - (2.0 * I + 1.0) / (P + G + 1.0)
    dice = dice_n[has].mean() if bool(has.any()) else z.sum() * 0.0
    return ce + dice_weight * dice


# ------------------------------------------------------------------------------------------------ eval-mode segmentation head
def check_seghead_eval(dev, images=1, E=64, seed=23, train_flag=False):
    """seghead.seg_head_inference against the module's own torch layers in .eval() on the CPU in fp32 (check_seghead's
    construction and gate), with non-trivial BatchNorm affine parameters and running statistics; the statistics and the batch
    counters are unchanged afterwards, whatever mode the head is in."""
    import copy
    from ccd_amd import seghead as sh
    from ccd_amd.modules.segmentor import SegHead
    from kernel_checks import BF, close, rnd
    torch.manual_seed(seed)
    ref = SegHead(in_channels=E).float()
    g = torch.Generator().manual_seed(seed)
    bns = [m for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    with torch.no_grad():
        for m in bns:
            m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
            m.momentum = 0.5
    ref.train()
    with torch.no_grad():                       # running statistics of three batches that are not the one under test
        for _ in range(3):
            xs = [rnd((2, E, 8, 32), g, 1.3) + 0.2 for _ in range(3)]
            ref.cls(ref.unpool2(ref.unpool1(ref.mlahead(*xs))))
    ref.eval()
    head = copy.deepcopy(ref).to(dev)
    head.train(train_flag)
    before = {k: v.detach().clone() for k, v in head.named_buffers()}
    assert all(int(v) == 3 for k, v in before.items() if "num_batches" in k and not k.startswith("conv_mla"))
    taps = [rnd((images * 256, E), g).to(BF) for _ in range(3)]
    logits = sh.seg_head_inference(head, [t.to(dev) for t in taps], images)
    rin = [t.float().view(images, 8, 32, E).permute(0, 3, 1, 2).contiguous() for t in taps]
    with torch.no_grad():
        want = ref.cls(ref.unpool2(ref.unpool1(ref.mlahead(*rin))))
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (images, 2, 32, 128) and not logits.requires_grad
    print(f"seghead eval: max err {(logits.cpu() - want).abs().max().item():.4g} of max {want.abs().max().item():.4g}")
    close(logits, want, 3e-2, 3e-2, "seghead/eval logits")
    for k, v in head.named_buffers():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert head.training == train_flag


# ------------------------------------------------------------------------------------------------ the model
SEG_ARCH = "vit_segtest3"


def register_arch():
    """The smallest backbone shape tests/model_checks.py builds (vit_test128: E = 128, two heads) with the three blocks and a tap
    behind each that its tiny_networks has, under a name: DINO_Segment looks architectures up by name."""
    from functools import partial
    import torch.nn as nn
    from ccd_amd.modules import vision_transformer as vits
    if SEG_ARCH not in vits.__dict__:
        setattr(vits, SEG_ARCH, lambda patch_size=16, **kw: vits.VisionTransformer(
            patch_size=patch_size, embed_dim=128, depth=3, num_heads=2, mlp_ratio=4, qkv_bias=True, out_indices=[1, 2, 3],
            norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw))


def register_arch4():
    """The same with a fourth block behind the last tap, as the stock architectures have six."""
    from functools import partial
    import torch.nn as nn
    from ccd_amd.modules import vision_transformer as vits
    if SEG_ARCH + "_4" not in vits.__dict__:
        setattr(vits, SEG_ARCH + "_4", lambda patch_size=16, **kw: vits.VisionTransformer(
            patch_size=patch_size, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4, qkv_bias=True, out_indices=[1, 2, 3],
            norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw))


MODEL_LOSS = dict(class_weight=(0.5, 1.5), dice_weight=0.5, edge_weight=1.0, edge_radius=2)


def model_batch(B=2, seed=5):
    from ccd_amd import segment as sg
    ds = sg.SyntheticMaskSet(B, seed=seed)
    img, gt = sg.collate([ds[i] for i in range(B)])
    gt = gt.clone()
    gt[:, :2, :16] = 255                                  # a corner that is not scored
    return img, gt


def check_model(dev, B=2):
    from ccd_amd import segment as sg
    from ccd_amd.loss.seg_loss import SegSupLoss
    from ccd_amd.metric.eval_IOU import SegMeter
    register_arch()
    torch.manual_seed(11)
    model = sg.build_model(sg.SegmentConfig(arch=SEG_ARCH, drop_path_rate=0.0, **MODEL_LOSS), dev)
    opt = sg.make_optimizer(model, lr=1e-3, weight_decay=0.05)
    img, gt = model_batch(B)
    img, gt = img.to(dev), gt.to(dev)
    # forward_train = SegSupLoss on the logits the model produced
    loss = model(img, gt, return_loss=True)
    logits = model.last_logits
    assert tuple(logits.shape) == (B, 2, 32, 128) and logits.dtype == torch.float32 and not logits.requires_grad
    again = SegSupLoss(**MODEL_LOSS)(logits, gt)
    assert torch.equal(loss.detach(), again), (float(loss), float(again))
    first = float(loss.detach())
    opt.zero_grad()
    loss.backward()
    want = R.seg_sup_loss(logits.cpu().numpy(), gt.cpu().numpy(), MODEL_LOSS["class_weight"], MODEL_LOSS["dice_weight"],
                          MODEL_LOSS["edge_weight"], MODEL_LOSS["edge_radius"])
    np.testing.assert_allclose(first, want["loss"], **LOSS_TOL)
    db = model.segmentation.cls.bias.grad.detach().cpu().numpy().astype(np.float64)
    print("cls.bias.grad", db, "want", want["grad"].sum(axis=(0, 2, 3)))
    np.testing.assert_allclose(db, want["grad"].sum(axis=(0, 2, 3)), err_msg="cls.bias.grad", **GRAD_TOL)
    arena = model.arena
    for i in range(3):
        gq = arena.g(f"backbone.blocks.{i}.attn.qkv.weight")
        assert bool(torch.isfinite(gq).all()) and float(gq.abs().max()) > 0.0, f"block {i}: qkv.weight.grad"
    unused = model.unused_parameter_names()
    assert "backbone.cls_token" in unused and sum(n.startswith("segmentation.conv_mla.") for n in unused) == 18
    for n in unused:
        assert float(arena.g(n).abs().max()) == 0.0, n
    opt.step()
    # three AdamW iterations on the one batch lower the loss
    for _ in range(2):
        sg.training_iteration(model, opt, img, gt, 1e-3)
    with torch.no_grad():
        last = float(model(img, gt, return_loss=True))
    print(f"loss {first:.5f} -> {last:.5f} after three AdamW iterations")
    assert last < first, (first, last)
    # inference: eval-mode logits, the mask rule, the meter
    tracked = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    test_logits = model(img, return_loss=False)           # (dispatches to forward_test)
    assert tuple(test_logits.shape) == (B, 2, 32, 128) and test_logits.dtype == torch.float32 and model.training
    mask, prob = model.forward_mask(img)
    assert mask.dtype == torch.uint8 and prob.dtype == torch.float32 and tuple(mask.shape) == tuple(prob.shape) == (B, 32, 128)
    assert torch.equal(mask.long(), test_logits.argmax(dim=1))
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in tracked.items()), "forward_test touched the BatchNorm statistics"
    meter = SegMeter()
    meter.update_logits(test_logits, torch.where(gt == 255, torch.zeros_like(gt), gt))
    assert meter.sums.device == test_logits.device and meter.pooled.device == test_logits.device
    scores = meter.compute()
    assert scores["n_images"] == B and 0.0 <= scores["pixel_accuracy"] <= 1.0
    fore = sg.fore_iou(model.loss.last_confusion)
    assert fore.device == test_logits.device and 0.0 <= float(fore) <= 1.0


def check_model_stops_at_last_tap(dev, B=1):
    """A backbone with a block behind its last tap: the passes stop at the tap - the logits are those of the same weights without
    that block, bit for bit - the block keeps its parameters (state dict), gets no gradient and is listed as unused."""
    from ccd_amd import segment as sg
    register_arch()
    register_arch4()
    torch.manual_seed(12)
    deep = sg.build_model(sg.SegmentConfig(arch=SEG_ARCH + "_4", drop_path_rate=0.1, **MODEL_LOSS), dev)
    flat = sg.build_model(sg.SegmentConfig(arch=SEG_ARCH, drop_path_rate=0.1, **MODEL_LOSS), dev)
    assert deep.backbone.spec.depth == 3 and len(deep.backbone.blocks) == 4 and flat.backbone.spec.depth == 3
    assert deep.backbone.spec.dpr == [x.item() for x in torch.linspace(0, 0.1, 4)][:3]        # the rates of the full depth
    sd = deep.state_dict()
    assert any(k.startswith("backbone.blocks.3.") for k in sd)
    flat.load_state_dict({k: v for k, v in sd.items() if not k.startswith("backbone.blocks.3.")})
    flat.ensure_arena()
    img, gt = model_batch(B, seed=9)
    img, gt = img.to(dev), gt.to(dev)
    assert torch.equal(deep.forward_test(img), flat.forward_test(img))
    opt = sg.make_optimizer(deep, lr=1e-3)
    loss = deep(img, gt)
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
