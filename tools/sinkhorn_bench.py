#!/usr/bin/env python3
"""Time the Sinkhorn-Knopp teacher assignment (ccd_amd/csrc/kernels/sinkhorn.h) on the GPU with HIP events on the current stream.

    python tools/sinkhorn_bench.py [--iters 20] [--rounds 5] [--steps 10] [--out profiles/sinkhorn.json]

Three figures:
  potentials    ops.sinkhorn_potentials on fp32 [3584, 65536] logits (256 images per GPU: about 7 selected rows per image and view)
                at temp 0.04, 3 iterations, against the reference's formula composed from torch ops on the same device
                (exp(t / temp)^T and its alternating normalisations, Dino_loss.py:157-184, written for this tool; the logits are
                clamped cosine products, so its fp32 exp stays finite);
  share_of_hbm  (2n - 1) * rows * K * 4 bytes, the passes' algorithmic traffic, over the fused time, against the measured HBM rate
                of 6.29 TB/s;
  step          one ViT-Small pretraining iteration at 256 images (bench.py's workload: synthetic batch, AdamW, epoch 0) with
                teacher_centering="sinkhorn_knopp" and with the default "center"; configurations alternate round by round.
Every call is bracketed by its own pair of events; a round is the median over its calls, and the figure reported is the median of
the round medians with their lowest and highest value (the run-to-run spread).  Prints one JSON line and, with --out, writes it to
that file."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ccd_amd import ops, pretrain  # noqa: E402
from ccd_amd.loss.Dino_loss import DINOLoss  # noqa: E402
from ccd_amd.synthetic import make_batch  # noqa: E402

HBM_TBS = 6.29
ROWS, K, TEMP, N_ITER = 3584, 65536, 0.04, 3


def call_times(fn, iters, warm=3):
    """ms of each of `iters` calls (events around every call, read after one synchronise)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(rounds):
    return {"median_ms": round(statistics.median(rounds), 4), "lowest_ms": round(min(rounds), 4), "highest_ms": round(max(rounds), 4)}


def torch_sinkhorn(t, temp, n_iterations):
    """The [rows, K] assignment from torch ops, one process."""
    q = torch.exp(t / temp).t()
    k, b = q.shape
    q = q / q.sum()
    for _ in range(n_iterations):
        q = q / q.sum(dim=1, keepdim=True) / k
        q = q / q.sum(dim=0, keepdim=True) / b
    return (q * b).t()


def cosine_logits(rows, k, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(rows, 64, device=dev, generator=g), dim=1)
    w = torch.nn.functional.normalize(torch.randn(k, 64, device=dev, generator=g), dim=1)
    return (2.5 * (a @ w.t())).clamp_(-1.0, 1.0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sinkhorn_bench needs an MI355X"
    dev = torch.device("cuda")
    out = {"iters": a.iters, "rounds": a.rounds, "unit": "ms per call (median of round medians; lowest and highest round)",
           "hbm_tbs": HBM_TBS}

    # ---- the potentials against the torch composition
    t = cosine_logits(ROWS, K, dev, 1)
    d_rows = torch.tensor([ROWS // 2], dtype=torch.int32, device=dev)
    fused = lambda: ops.sinkhorn_potentials(t, d_rows, TEMP, N_ITER, rows_mul=2)
    composed = lambda: torch_sinkhorn(t, TEMP, N_ITER)
    q_ref = composed()
    q_ours = torch.softmax((t - fused()[None, :]) / TEMP, dim=1)
    live = q_ref >= 1e-12
    agree = float(((q_ours - q_ref).abs()[live] / q_ref[live]).max())
    del q_ref, q_ours, live
    f_rounds, c_rounds = [], []
    for _ in range(a.rounds):
        f_rounds.append(statistics.median(call_times(fused, a.iters)))
        c_rounds.append(statistics.median(call_times(composed, max(3, a.iters // 4), warm=1)))
    f, c = summary(f_rounds), summary(c_rounds)
    nbytes = (2 * N_ITER - 1) * ROWS * K * 4
    out[f"potentials fp32 [{ROWS}, {K}] temp {TEMP} n {N_ITER}"] = {
        "fused": f, "torch_composition": c, "speedup": round(c["median_ms"] / f["median_ms"], 2),
        "fused_beats_composition_beyond_spread": f["highest_ms"] < c["lowest_ms"],
        "largest_relative_difference_of_the_assignments": agree, "pass_bytes": nbytes,
        "fused_gbs": round(nbytes / (f["median_ms"] * 1e-3) / 1e9, 1),
        "share_of_hbm": round(nbytes / (f["median_ms"] * 1e-3) / (HBM_TBS * 1e12), 4)}
    del t

    # ---- one ViT-Small step with the key on and off
    B = a.batch
    images, masks, metrics = make_batch(B, seed=1000, device=dev)
    lr, wd, mom = 0.0005 * B / 256.0, 0.04, 0.9995
    runs = {}
    for key in ("center", "sinkhorn_knopp"):
        torch.manual_seed(0)
        student, teacher = pretrain.build_networks(arch="vit_small", out_dim=K, drop_path_rate=0.1, norm_last_layer=False, device=dev)
        loss = DINOLoss(K, 2, 0.04, 0.04, 0, 100, teacher_centering=key).to(dev)
        opt = pretrain.make_optimizer(student, clip_grad=3.0)
        runs[key] = (student, teacher, loss, opt)

    def step_of(key):
        student, teacher, loss, opt = runs[key]
        return lambda: pretrain.training_iteration(student, teacher, loss, opt, images, masks, metrics, epoch=0, lr=lr, wd=wd, momentum=mom)

    rounds = {key: [] for key in runs}
    for _ in range(a.rounds):
        for key in runs:
            rounds[key].append(statistics.median(call_times(step_of(key), a.steps, warm=2)))
    s_off, s_on = summary(rounds["center"]), summary(rounds["sinkhorn_knopp"])
    losses = {key: float(runs[key][2].last_losses["Dino_loss"]) for key in runs}
    out[f"vit_small step, {B} images"] = {
        "teacher_centering=center": s_off, "teacher_centering=sinkhorn_knopp": s_on,
        "overhead_ms": round(s_on["median_ms"] - s_off["median_ms"], 4),
        "overhead_beyond_spread": s_on["lowest_ms"] > s_off["highest_ms"], "last_dino_loss": losses}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
