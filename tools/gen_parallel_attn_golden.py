#!/usr/bin/env python3
"""Generate tests/golden/parallel_attn.npz by running the REAL reference's `Attention` (Dino/modules/attention.py:5-30, read-only
reference tree) on the CPU, as tools/gen_golden.py does for the other fixtures.  Nothing of the reference is copied: only its numerical
outputs for seeded inputs are recorded - weights, one input of N = 2, E = 64, T = 25, `g_output`, `attn`, and the autograd gradients of
every parameter and of the input under a fixed random dG.

Two cases: `default_*` at torch's default initialisation (the maps are nearly uniform there: the largest probability is ~0.012 against
1 / 256), and `peaked_*` with we.weight scaled by WE_GAIN so that the reference's maps have a median peak probability above 0.1
(asserted) - a broken softmax or a wrong token order cannot pass within tolerance.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_parallel_attn_golden.py [--reference /path/to/reference]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True
N, E, T, TOKENS = 2, 64, 25, 256
WE_GAIN = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "parallel_attn.npz"))
    a = ap.parse_args()
    # REPO is NOT put on sys.path: its `Dino/` alias package (a regular package) would shadow the reference's namespace package
    sys.path.insert(0, os.path.join(HERE, "oracle_stubs"))
    sys.path.insert(0, a.reference)
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or os.getcwd()) != REPO]
    import torch
    from Dino.modules.attention import Attention

    out = {}
    for case, gain in (("default", 1.0), ("peaked", WE_GAIN)):
        torch.manual_seed(17)
        att = Attention(in_channels=E, max_length=T, n_feature=TOKENS)
        with torch.no_grad():
            att.we.weight.mul_(gain)
        gen = torch.Generator().manual_seed(23)
        x = torch.randn(N, TOKENS, E, generator=gen).requires_grad_(True)       # tokens, s = row * 32 + col
        dG = torch.randn(N, T, E, generator=gen)
        g_output, attn = att(x.transpose(1, 2).reshape(N, E, 8, 32))
        (g_output * dG).sum().backward()
        peak = float(attn.detach().reshape(N, T, TOKENS).max(dim=2).values.median())
        print(f"{case}: median peak probability {peak:.4f} (uniform: {1 / TOKENS:.4f})")
        assert (peak > 0.1) if case == "peaked" else (peak < 0.05)
        out["x"], out["dG"] = x.detach().numpy(), dG.numpy()            # (the same seed: one input and one dG for both cases)
        rec = dict(g_output=g_output, attn=attn, d_x=x.grad, F=att.f0_embedding.weight, W0=att.w0.weight, b0=att.w0.bias,
                   Wv=att.wv.weight, bv=att.wv.bias, We=att.we.weight, be=att.we.bias, d_F=att.f0_embedding.weight.grad,
                   d_W0=att.w0.weight.grad, d_b0=att.w0.bias.grad, d_Wv=att.wv.weight.grad, d_bv=att.wv.bias.grad,
                   d_We=att.we.weight.grad, d_be=att.we.bias.grad)
        out.update({f"{case}_{k}": v.detach().numpy().astype(np.float32) for k, v in rec.items()})
    out["state_dict_names"] = np.array(list(att.state_dict().keys()))
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
