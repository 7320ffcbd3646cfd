"""ccd_attention_probs and VisionTransformer's inspection methods (get_last_selfattention, get_intermediate_layers) on the MI355X."""
import os

import numpy as np
import pytest
import torch

import selfattn_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "selfattn_cases.npz")))


@pytest.mark.parametrize("views", [1, 7, 512])
@pytest.mark.parametrize("heads", [3, 6, 8, 12])
def test_attention_probs_kernel(heads, views):
    """Against torch's softmax of the same bf16 q, k (<= 1e-5, row sums within 2e-5); two launches bitwise equal; a view alone
    bitwise equal to the same view inside the batch."""
    from ccd_amd import ops
    qkv = R.probs_case(views, heads, seed=heads * 1000 + views).to(DEV)
    got = ops.attention_probs(qkv, heads, 64 ** -0.5)
    R.check_probs(got, R.probs_torch(qkv, heads))
    assert torch.equal(got, ops.attention_probs(qkv, heads, 64 ** -0.5))
    for i in sorted({0, views // 2, views - 1}):
        assert torch.equal(ops.attention_probs(qkv[i:i + 1].contiguous(), heads, 64 ** -0.5)[0], got[i])


def _fixture_model(fx):
    return R.fixture_model(fx).to(DEV).eval()


def test_fixture_from_reference(fx):
    """vit_small at seed 0 with the fixture's qkv perturbation against what the reference recorded (bf16 kernels vs fp32 reference).
    Measured on the MI355X: attn 7.4e-3, x_last 3.8e-3, intermediate layers 4.1e-3 relative L2 (a bf16 restatement on the host
    predicts 7.2e-3 / 3.7e-3: bf16 rounding of the kernels' operands, not the kernels)."""
    m = _fixture_model(fx)
    x = torch.from_numpy(fx["images"]).to(DEV)
    rows = torch.from_numpy(fx["rows"]).long()
    pos = m.interpolate_pos_encoding(m.prepare_tokens(x), 32, 128)
    x_last, attn = m.get_last_selfattention(x)
    inter = m.get_intermediate_layers(x, n=4)
    assert float((pos[0, fx["pos_rows"]].cpu() - torch.from_numpy(fx["pos"])).abs().max()) <= 1e-5
    rel = {"attn": R.rel_l2(attn[:, :, rows], torch.from_numpy(fx["attn"])),
           "x_last": R.rel_l2(x_last[:, rows], torch.from_numpy(fx["x_last"]))}
    for j, t in enumerate(inter):
        rel[f"inter{j}"] = R.rel_l2(t[:, rows].float(), torch.from_numpy(fx["inter"][j]))
    print("fixture relative L2:", rel)
    assert rel["attn"] <= 2e-2, rel
    assert all(v <= 1e-2 for k, v in rel.items() if k != "attn"), rel


def test_attention_is_the_kernel_on_the_engine_qkv(fx, monkeypatch):
    """The model's attention is exactly ccd_attention_probs of the engine's own qkv of the last block: <= 1e-5 against torch's
    softmax of that qkv (measured 4.1e-8)."""
    from ccd_amd import ops
    m = _fixture_model(fx)
    seen = []
    real = ops.attention_probs
    monkeypatch.setattr(ops, "attention_probs", lambda qkv, *a: (seen.append(qkv.clone()), real(qkv, *a))[1])
    _, attn = m.get_last_selfattention(torch.from_numpy(fx["images"]).to(DEV))
    assert len(seen) == 1
    err, _ = R.check_probs(attn, R.probs_torch(seen[0], 6))
    print("kernel vs torch softmax of the engine's qkv:", err)


def test_intermediate_layers_equal_forward(fx):
    m = _fixture_model(fx)
    x = torch.randn((5, 3, 32, 128), generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        tokens = m(x)[0]
    assert torch.equal(m.get_intermediate_layers(x, 1)[0], tokens)
    assert torch.equal(m.get_intermediate_layers(x, 3)[-1], tokens)


def test_no_droppath_in_train_mode():
    """train() with drop_path_rate = 0.1 gives bitwise the eval-mode results, and the DropPath seed stream does not move."""
    from ccd_amd import engine
    from ccd_amd.modules import vision_transformer as vits
    torch.manual_seed(0)
    m = vits.vit_small(patch_size=4, drop_path_rate=0.1).to(DEV)
    R.perturb_qkv(m.named_parameters(), 5, 0.06)
    x = torch.randn((3, 3, 32, 128), generator=torch.Generator().manual_seed(4)).to(DEV)
    outs = []
    for train in (False, True):
        m.train(train)
        calls = engine._DROPPATH_SEED["calls"]
        outs.append(list(m.get_last_selfattention(x)) + m.get_intermediate_layers(x, 2))
        assert engine._DROPPATH_SEED["calls"] == calls
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_training_unaffected_by_inspection(monkeypatch):
    """Two pretraining iterations from the same seed (DropPath on), twice without and once with a get_last_selfattention call between
    them: the DropPath masks of every iteration are bitwise those of the plain runs and the call does not advance the seed stream.
    The losses are not bitwise repeatable even WITHOUT the call - two plain runs measured 7.1026549 / 7.1026559 and 6.297233 /
    6.297277, the run with the call 6.297010 (fp32 atomics in the gradient reductions) - so the second loss is held to that
    run-to-run spread, 1e-3 relative; the DropPath masks, which an advanced seed stream would change, are compared bitwise."""
    from ccd_amd import engine, ops, pretrain
    from ccd_amd.loss.Dino_loss import DINOLoss
    from ccd_amd.synthetic import make_batch
    drawn = []                # the DropPath scales of every run
    real = ops.droppath_scales
    monkeypatch.setattr(ops, "droppath_scales", lambda *a, **k: (lambda out: (drawn[-1].append(out.clone()), out)[1])(real(*a, **k)))
    runs = []
    for inspect in (False, False, True):
        drawn.append([])
        torch.manual_seed(3)
        np.random.seed(3)
        engine._DROPPATH_SEED.update(base=987654, calls=0)
        student, teacher = pretrain.build_networks(arch=None, out_dim=512, drop_path_rate=0.1, norm_last_layer=False, seg_channel=192,
                                                   backbone_kwargs=dict(embed_dim=192, depth=3, num_heads=3, out_indices=[1, 2, 3]),
                                                   head_kwargs=dict(hidden_dim=256, bottleneck_dim=64), device=DEV)
        dino_loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(DEV)
        opt = pretrain.make_optimizer(student, clip_grad=3.0)
        losses = []
        for it in range(2):
            images, masks, metrics = make_batch(8, seed=40 + it, device=DEV)
            losses.append(pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 2e-4, 0.05, 0.99))
            if inspect and it == 0:
                calls = engine._DROPPATH_SEED["calls"]
                _, attn = student.backbone.get_last_selfattention(images[:, 0].contiguous())
                assert attn.shape == (8, 3, 256, 256) and engine._DROPPATH_SEED["calls"] == calls
        torch.cuda.synchronize()
        runs.append([float(l) for l in losses])
    engine._DROPPATH_SEED.update(base=None, calls=0)
    print("losses (plain, plain, with get_last_selfattention):", runs)
    assert len(drawn[0]) >= 2 and all(len(d) == len(drawn[0]) for d in drawn)
    assert all(torch.equal(a, b) for d in drawn[1:] for a, b in zip(drawn[0], d))
    assert abs(runs[2][1] - runs[0][1]) <= 1e-3 * abs(runs[0][1]), runs


@pytest.mark.parametrize("arch", ["vit_tiny", "vit_base", "vit_base_768"])
def test_other_architectures(arch):
    """B = 4 against tests/selfattn_ref.py with the same gates as the fixture (measured attn 7.5e-3 / 9.0e-3 / 8.9e-3, x_last and
    intermediate layers 3.3e-3 .. 5.6e-3 for vit_tiny / vit_base / vit_base_768)."""
    from ccd_amd.modules import vision_transformer as vits
    E, depth, heads = {"vit_tiny": (192, 12, 3), "vit_base": (512, 12, 8), "vit_base_768": (768, 12, 12)}[arch]
    torch.manual_seed(0)
    m = getattr(vits, arch)(patch_size=4)
    R.perturb_qkv(m.named_parameters(), 4321, 0.06 * (384 / E) ** 0.5)     # the same logit scale as vit_small's fixture
    sp = R.spec(E, depth, heads)
    P = R.state_table(m)
    m = m.to(DEV).eval()
    x = torch.randn((4, 3, 32, 128), generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        xl_w, attn_w = R.get_last_selfattention(P, x, sp)
        inter_w = R.get_intermediate_layers(P, x, sp, n=3)
    xl, attn = m.get_last_selfattention(x.to(DEV))
    inter = m.get_intermediate_layers(x.to(DEV), n=3)
    rel = {"attn": R.rel_l2(attn, attn_w), "x_last": R.rel_l2(xl, xl_w)}
    for j, (a, b) in enumerate(zip(inter, inter_w)):
        rel[f"inter{j}"] = R.rel_l2(a.float(), b)
    print(arch, "relative L2:", rel)
    assert rel["attn"] <= 2e-2, rel
    assert all(v <= 1e-2 for k, v in rel.items() if k != "attn"), rel


def test_user_sized_batch():
    """vit_small at B = 256: shapes, finite values, row sums."""
    from ccd_amd.modules import vision_transformer as vits
    torch.manual_seed(0)
    m = vits.vit_small(patch_size=4).to(DEV).eval()
    x = torch.randn((256, 3, 32, 128), generator=torch.Generator().manual_seed(1)).to(DEV)
    xl, attn = m.get_last_selfattention(x)
    assert xl.shape == (256, 256, 384) and xl.dtype == torch.float32 and attn.shape == (256, 6, 256, 256)
    assert bool(torch.isfinite(xl).all()) and bool(torch.isfinite(attn).all())
    assert float((attn.sum(-1) - 1).abs().max()) <= 2e-5 and float(attn.min()) >= 0.0
    inter = m.get_intermediate_layers(x, n=4)
    assert len(inter) == 4 and all(t.shape == (256, 256, 384) and t.dtype == torch.bfloat16 and bool(torch.isfinite(t).all())
                                   for t in inter)
