"""Host logic of the parallel attention head: the numpy specification against the reference's own `Attention`
(tests/golden/parallel_attn.npz, written by tools/gen_parallel_attn_golden.py), DINO_Finetune's wiring of decoder.type
'ParallelAttnDecoder' (parameter names, the reference's state dict, refusals, the YAML) and the Dino alias.  No GPU."""
import os

import numpy as np
import torch

import parallel_attn_checks as K
import parallel_attn_np as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parallel_attn.npz")


def test_dino_alias():
    import Dino.decoder.parallel_attn_decoder
    from ccd_amd.decoder import parallel_attn_decoder
    assert Dino.decoder.parallel_attn_decoder is parallel_attn_decoder and parallel_attn_decoder.ParallelAttnDecoder


def test_model_wiring_refusals_and_yaml():
    K.check_refusals_and_loading()


def _golden(case):
    g = np.load(GOLDEN)
    w = {k: g[f"{case}_{k}"] for k in ("F", "W0", "b0", "Wv", "bv", "We", "be")}
    return g, w


def test_specification_reproduces_the_reference():
    """The numpy specification against the reference's `Attention` (fp32, torch on the CPU) on N = 2, E = 64, T = 25, at the default
    initialisation and with we.weight scaled until the maps are peaked (median peak probability 0.24; 0.009 at the default scale).
    Outputs: the gate of tests/test_oracle_golden.py for fp32 reference outputs, rtol 1e-4 / atol 1e-5 (observed: |dG_out| 1.9e-6 of
    2.55, |da| 5.9e-7).  Gradients: that file gates per-parameter statistics, which fits no element-wise comparison of a gradient
    whose entries span six decades, so the gate is 8 x the largest difference observed here relative to the largest entry of the
    gradient - observed 1.0e-6 * max |reference| (fp32 rounding of the reference's sums), gate 8e-6 * max |reference|.  d we.bias is
    analytically zero (the reference holds rounding noise of 1.7e-6 there): it is gated against d we.weight's scale."""
    for case in ("default", "peaked"):
        g, w = _golden(case)
        f = S.forward(g["x"], w)
        attn = g[f"{case}_attn"].reshape(2, 25, 256)
        peak = float(np.median(attn.max(axis=2)))
        assert peak > 0.1 if case == "peaked" else peak < 0.05
        np.testing.assert_allclose(f["a"], attn, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(f["G"], g[f"{case}_g_output"], rtol=1e-4, atol=1e-5)
        b = S.backward(g["dG"], g["x"], w)
        for k in ("F", "W0", "b0", "Wv", "bv", "We", "x"):
            ref = g[f"{case}_d_{k}"]
            got = b["dX" if k == "x" else "d" + k]
            assert np.abs(got - ref).max() <= 8e-6 * np.abs(ref).max(), (case, k, np.abs(got - ref).max(), np.abs(ref).max())
        assert np.abs(b["dbe"] - g[f"{case}_d_be"]).max() <= 8e-6 * np.abs(g[f"{case}_d_We"]).max()


def test_core_formulas_are_the_whole_head_split_at_the_kernel_boundary():
    g, w = _golden("peaked")
    f = S.forward(g["x"], w)
    a, G = S.core_forward(f["P"], g["x"], f["Q0"], w["We"], w["be"])
    assert np.array_equal(a, f["a"]) and np.array_equal(G, f["G"]) and np.allclose(a.sum(-1), 1.0, atol=1e-12)


def test_a_state_dict_of_the_reference_attention_loads():
    m = K.check_refusals_and_loading()
    g, _ = _golden("peaked")
    names = [str(n) for n in g["state_dict_names"]]
    assert ["attention." + n for n in names] == K.NAMES[:7]
    sd = {n: torch.zeros_like(p) for n, p in m.decoder.attention.state_dict().items()}
    assert list(sd) == names                                           # the reference's keys, in its order
    att = __import__("ccd_amd.decoder.parallel_attn_decoder", fromlist=["x"]).ParallelAttnDecoder(64, 93, 25)
    short = {"f0_embedding.weight": "F", "w0.weight": "W0", "w0.bias": "b0", "wv.weight": "Wv", "wv.bias": "bv", "we.weight": "We", "we.bias": "be"}
    att.attention.load_state_dict({n: torch.from_numpy(g["peaked_" + short[n]]) for n in names}, strict=True)
    assert torch.equal(att.attention.we.weight.detach(), torch.from_numpy(g["peaked_We"]))


def test_initialisation_is_torchs_in_the_reference_order():
    """torch's defaults, drawn in the reference's construction order (Embedding, w0, wv, we, then cls): the same seed gives the weights a
    plain torch construction in that order gives."""
    import torch.nn as nn
    from ccd_amd.decoder.parallel_attn_decoder import ParallelAttnDecoder
    torch.manual_seed(4)
    dec = ParallelAttnDecoder(64, 93, 25)
    torch.manual_seed(4)
    ref = [nn.Embedding(25, 64), nn.Linear(25, 256), nn.Linear(64, 64), nn.Linear(64, 25), nn.Linear(64, 93)]
    want = [ref[0].weight] + [t for m in ref[1:] for t in (m.weight, m.bias)]
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(dec.parameters(), want)) and len(list(dec.parameters())) == 9
