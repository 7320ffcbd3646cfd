"""VisionTransformer's inspection methods (get_last_selfattention, get_intermediate_layers, prepare_tokens, interpolate_pos_encoding;
Dino/modules/vision_transformer.py:182-271) on the host: the torch restatement against the reference's recorded outputs, the fixture's
information content, the methods' signatures and input contract."""
import inspect
import os

import numpy as np
import pytest
import torch

import selfattn_ref as R


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "selfattn_cases.npz")))


def test_restatement_reproduces_fixture(fx):
    """tests/selfattn_ref.py (the oracle's pieces) reproduces what the reference recorded, to fp32 rounding."""
    sp = R.spec(384, 12, 6)
    P = R.state_table(R.fixture_model(fx))
    x = torch.from_numpy(fx["images"])
    rows = torch.from_numpy(fx["rows"]).long()
    with torch.no_grad():
        pos = R.interpolate_pos_encoding(P, sp)
        x_last, attn = R.get_last_selfattention(P, x, sp)
        inter = R.get_intermediate_layers(P, x, sp, n=4)
    assert pos.shape == (1, 256, 384) and attn.shape == (2, 6, 256, 256) and len(inter) == 4
    errs = {
        "pos": float((pos[0, fx["pos_rows"]] - torch.from_numpy(fx["pos"])).abs().max()),
        "x_last": float((x_last[:, rows] - torch.from_numpy(fx["x_last"])).abs().max()),
        "attn": float((attn[:, :, rows] - torch.from_numpy(fx["attn"])).abs().max()),
        "inter": float((torch.stack([t[:, rows] for t in inter]) - torch.from_numpy(fx["inter"])).abs().max()),
    }
    assert all(e <= 1e-5 for e in errs.values()), errs


def test_fixture_is_informative(fx):
    """The recorded attention rows are far from uniform and from any other key order: a key permutation moves them by more than 25x
    the GPU gate (2e-2 relative L2), and their maxima are several times 1/256 (at the plain init every row is ~1/256)."""
    attn = torch.from_numpy(fx["attn"]).double()
    g = torch.Generator().manual_seed(0)
    perm = attn[..., torch.randperm(256, generator=g)]
    assert R.rel_l2(perm, attn) > 0.5, R.rel_l2(perm, attn)
    assert R.rel_l2(torch.full_like(attn, 1 / 256), attn) > 0.4
    mx = attn.max(-1).values          # recorded: median 0.0144 (3.7 / 256), 82 % of the rows above 2 / 256, largest 0.046
    assert float(mx.median()) > 3.0 / 256 and float((mx > 2.0 / 256).double().mean()) > 0.75, mx
    assert torch.allclose(attn.sum(-1), torch.ones_like(mx), atol=1e-5)


# (reference: Dino/modules/vision_transformer.py:182, 225, 253, 262)
REFERENCE_SIGNATURES = {
    "interpolate_pos_encoding": [("x", inspect.Parameter.empty), ("w", inspect.Parameter.empty), ("h", inspect.Parameter.empty)],
    "prepare_tokens": [("x", inspect.Parameter.empty)],
    "get_last_selfattention": [("x", inspect.Parameter.empty)],
    "get_intermediate_layers": [("x", inspect.Parameter.empty), ("n", 1)],
}


def test_method_names_and_signatures_match_reference():
    from ccd_amd.modules.vision_transformer import VisionTransformer
    assert sorted(REFERENCE_SIGNATURES) == sorted(R.METHODS)
    for name, want in REFERENCE_SIGNATURES.items():
        params = list(inspect.signature(getattr(VisionTransformer, name)).parameters.values())[1:]
        assert [(p.name, p.default) for p in params] == want, name


def test_input_contract_on_host():
    """Anything but fp32 [N, 3, 32, 128] images on the module's device is a ValueError, before any kernel or arena."""
    from functools import partial
    from ccd_amd.modules import vision_transformer as vits
    m = vits.VisionTransformer(patch_size=4, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), out_indices=[1, 2])
    bad = [torch.zeros(1, 3, 32, 64), torch.zeros(1, 3, 32, 128, dtype=torch.float64), torch.zeros(3, 32, 128),
           torch.zeros(2, 1, 32, 128), np.zeros((1, 3, 32, 128), np.float32)]
    for x in bad:
        for call in (m.get_last_selfattention, m.get_intermediate_layers, m.prepare_tokens):
            with pytest.raises(ValueError):
                call(x)
    with pytest.raises(ValueError):
        m.interpolate_pos_encoding(torch.zeros(1, 256, 128), 64, 128)
    with pytest.raises(ValueError):
        m.interpolate_pos_encoding(torch.zeros(1, 128, 128), 32, 128)
