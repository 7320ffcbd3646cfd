#!/usr/bin/env python3
"""Times the inspection path of VisionTransformer (vit_small, patch 4) with HIP events after warm-up:
  ops.attention_probs alone, get_last_selfattention and get_intermediate_layers(n=4) end to end, and a torch eager restatement of the
  probabilities (bf16 q k^T + fp32 softmax) - at B = 64 and 256.  The kernel's bandwidth (P written + Q, K read) is set against
  6.2 TB/s, the rate of plain full-shape stores on the MI355X; the floor below is computed from that rate, not measured.

    python tools/selfattn_bench.py [--batches 64 256] [--iters 20] [--json out.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ccd_amd import ops  # noqa: E402
from ccd_amd.modules import vision_transformer as vits  # noqa: E402

STORE_TBS = 6.2


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def eager_probs(qkv, heads):
    n = qkv.shape[0]
    q, k, _ = qkv.reshape(n, 256, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return torch.softmax((q @ k.transpose(-2, -1)).float() * 64 ** -0.5, dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = vits.vit_small(patch_size=4).to(dev).eval()
    heads = 6
    rows = []
    for B in a.batches:
        x = torch.randn((B, 3, 32, 128), device=dev)
        qkv = (1.5 * torch.randn((B, 256, 3 * 384), device=dev)).to(torch.bfloat16)
        p_bytes, qk_bytes = 4.0 * B * heads * 256 * 256, 2.0 * B * 256 * 2 * 384
        floor_us = (p_bytes + qk_bytes) / (STORE_TBS * 1e12) * 1e6
        k_ms = timed(lambda: ops.attention_probs(qkv, heads, 0.125), a.iters)
        e_ms = timed(lambda: eager_probs(qkv, heads), a.iters)
        gls_ms = timed(lambda: m.get_last_selfattention(x), max(3, a.iters // 4))
        gil_ms = timed(lambda: m.get_intermediate_layers(x, 4), max(3, a.iters // 4))
        fwd_ms = timed(lambda: m(x), max(3, a.iters // 4))
        row = {"batch": B, "probs_MB": p_bytes / 1e6, "qk_MB": qk_bytes / 1e6, "floor_us": round(floor_us, 1),
               "attention_probs_us": round(k_ms * 1e3, 1), "attention_probs_TBs": round((p_bytes + qk_bytes) / (k_ms * 1e-3) / 1e12, 2),
               "of_store_rate": round((p_bytes + qk_bytes) / (k_ms * 1e-3) / 1e12 / STORE_TBS, 3), "x_floor": round(k_ms * 1e3 / floor_us, 2),
               "eager_torch_us": round(e_ms * 1e3, 1), "get_last_selfattention_ms": round(gls_ms, 3),
               "get_intermediate_layers4_ms": round(gil_ms, 3), "forward_no_grad_ms": round(fwd_ms, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    with torch.no_grad():
        main()
