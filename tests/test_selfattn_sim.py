"""ccd_attention_probs and VisionTransformer.get_last_selfattention / get_intermediate_layers on the CPU SIMT executor."""
from functools import partial

import pytest
import torch

import selfattn_ref as R
from backends import Backend


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("heads", [2, 3, 6])
def test_attention_probs_vs_torch_sim(sim, heads, views):
    from ccd_amd import ops
    qkv = R.probs_case(views, heads, seed=heads * 10 + views)
    got = ops.attention_probs(qkv, heads, 64 ** -0.5)
    R.check_probs(got, R.probs_torch(qkv, heads))


def test_attention_probs_rejects_shapes_sim(sim):
    from ccd_amd import _lib, ops
    qkv = torch.zeros((1, 256, 3 * 64 * 4), dtype=torch.bfloat16)
    probs = torch.empty((1, 4, 256, 256), dtype=torch.float32)
    for heads in (1, 4, 5, 16):           # E = heads * 64 outside the backbone's widths 128 / 192 / 384 / 512 / 768
        assert _lib.get().ccd_attention_probs(qkv.data_ptr(), probs.data_ptr(), 1, heads, 0.125, _lib.stream()) == -2, heads
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.attention_probs(qkv, 4, 0.125)
    with pytest.raises(ValueError):       # head_dim 32: the width does not match 3 * 64 * heads
        ops.attention_probs(torch.zeros((1, 256, 3 * 32 * 2), dtype=torch.bfloat16), 2, 32 ** -0.5)


def test_whole_model_against_restatement_sim(sim, monkeypatch):
    """E = 128, depth 2, 2 heads, B = 2 (test_model_sim.py's small architecture), qkv perturbed: the four methods against
    tests/selfattn_ref.py, and the attention against the torch softmax of the engine's own qkv of the last block."""
    from ccd_amd import engine, ops
    from ccd_amd.modules import vision_transformer as vits
    torch.manual_seed(7)
    m = vits.VisionTransformer(patch_size=4, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, drop_path_rate=0.2,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), out_indices=[1, 2])
    R.perturb_qkv(m.named_parameters(), 11, 0.1)
    sp = R.spec(128, 2, 2)
    P = R.state_table(m)
    x = torch.randn((2, 3, 32, 128), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        pos_w = R.interpolate_pos_encoding(P, sp)
        tok_w = R.prepare_tokens(P, x, sp)
        xl_w, attn_w = R.get_last_selfattention(P, x, sp)
        inter_w = R.get_intermediate_layers(P, x, sp, n=5)
    seen = []
    real = ops.attention_probs
    monkeypatch.setattr(ops, "attention_probs", lambda qkv, *a: (seen.append(qkv.clone()), real(qkv, *a))[1])
    calls = engine._DROPPATH_SEED["calls"]
    m.train()                                              # no DropPath in either mode
    pos = m.interpolate_pos_encoding(tok_w, 32, 128)
    tok = m.prepare_tokens(x)
    xl, attn = m.get_last_selfattention(x)
    inter = m.get_intermediate_layers(x, n=5)
    assert engine._DROPPATH_SEED["calls"] == calls
    assert pos.shape == (1, 256, 128) and tok.shape == (2, 256, 128) and xl.shape == (2, 256, 128) and attn.shape == (2, 2, 256, 256)
    assert len(inter) == 2 and all(t.shape == (2, 256, 128) and t.dtype == torch.bfloat16 for t in inter)
    assert not any(t.requires_grad for t in [pos, tok, xl, attn] + inter)
    assert float((pos - pos_w).abs().max()) <= 1e-5
    assert R.rel_l2(tok, tok_w) <= 1e-5
    assert R.rel_l2(attn, attn_w) <= 2e-2 and R.rel_l2(xl, xl_w) <= 1e-2
    for a, b in zip(inter, inter_w):
        assert R.rel_l2(a.float(), b) <= 1e-2
    assert m.get_intermediate_layers(x, 0) == [] and m.get_intermediate_layers(x, -3) == []
    # the kernel alone: the engine's own qkv of the last block through torch's softmax
    assert len(seen) == 1
    R.check_probs(attn, R.probs_torch(seen[0], 2))
