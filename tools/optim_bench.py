#!/usr/bin/env python3
"""Time the device half of an optimizer step (`launch_step`: per-tensor clip + update + bf16 mirrors) of FusedClipAdamW,
FusedClipSGD and FusedClipLARS on the ViT-Small student arena, in one process, with HIP events on the current stream.

    python tools/optim_bench.py [--iters 20] [--repeats 9] [--out profiles/optim_step.json]

The yardstick is the AdamW step of the same run.  The three are measured in turn inside every repeat (AdamW, SGD, LARS, AdamW, ...)
so that drift of the machine lands on all of them; a repeat is `iters` back-to-back steps between two events.  Reported per
optimizer: median / min / max ms per step over the repeats, and the achieved GB/s of the optimizer's ALGORITHMIC bytes over the
median (the sweep reads every tensor, the update touches the active ones; the transposed-mirror refresh that closes every
launch_step is inside the time and not inside the bytes, so the rate is a lower bound):

    AdamW   sweep 4 B (g)      + update 16 B read (g, p, m, v) + 14 B written (p, m, v, mirror)
    SGD     sweep 4 B (g)      + update 12 B read (g, p, buf)  + 10 B written (p, buf, mirror)
    LARS    sweep 8 B (g, p)   + update 12 B read (g, p, mu)   + 10 B written (p, mu, mirror)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ccd_amd import pretrain  # noqa: E402

BYTES = {"adamw": (4, 30), "sgd": (4, 22), "lars": (8, 22)}          # (sweep, update) per element


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--arch", default="vit_small")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    student, _ = pretrain.build_networks(arch=a.arch, device=dev)
    arena = student.arena
    arena.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    arena.grad.mul_(1e-2)
    opts = {k: pretrain.make_optimizer(student, clip_grad=3.0, name=k) for k in BYTES}
    for k, opt in opts.items():
        for gi, g in enumerate(opt.param_groups):
            g["lr"], g["weight_decay"] = 1e-5, (0.04 if gi == 0 else 0.0)
        opt.stage_hyper()                                   # every used tensor active (the last layer is not frozen)
    active = sum(s.numel for n, s in arena.segments.items() if n not in opts["adamw"].never_used and arena.params[n].requires_grad)
    total = sum(s.numel for s in arena.segments.values())

    def timed(opt):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.iters):
            opt.launch_step()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / a.iters

    for opt in opts.values():                               # warm-up: code objects, the lazily built tables
        for _ in range(5):
            opt.launch_step()
    torch.cuda.synchronize()
    times = {k: [] for k in opts}
    for _ in range(a.repeats):
        for k, opt in opts.items():
            times[k].append(timed(opt))
    assert bool(torch.isfinite(arena.flat).all())
    out = {"arch": a.arch, "elements": total, "active_elements": active, "iters_per_repeat": a.iters, "repeats": a.repeats,
           "unit": "ms per launch_step", "optimizers": {}}
    for k, ts in times.items():
        med = statistics.median(ts)
        nbytes = BYTES[k][0] * total + BYTES[k][1] * active
        out["optimizers"][k] = {"median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
                                "bytes_per_element": list(BYTES[k]), "algorithmic_MB": round(nbytes / 1e6, 1),
                                "GBps_at_median": round(nbytes / med / 1e6, 1),
                                "vs_adamw_median": round(med / statistics.median(times["adamw"]), 3)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
