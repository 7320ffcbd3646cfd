#!/usr/bin/env python3
"""Time the text super-resolution finetuning path on the GPU.

    python tools/superres_bench.py [--iters 30] [--rounds 5] [--batch 224] [--out profiles/superres.json]

  loss      the fused loss (kernels/sr.h), forward plus backward, at N = `batch` images of 3 x 32 x 128, against the same formula
            composed from torch ops on the same GPU (pad, slices, sqrt, abs, means; autograd for its backward).  Two forms of the
            fused side: the two raw calls, and SRLoss through autograd (what training runs).  The two sides' loss and gradient are
            compared first.
  upsample  ops.sr_upsample (base and the normalised input in one launch) against F.interpolate(bicubic) followed by the
            normalisation in torch.
  model     DINO_SuperRes, vit_small, `batch` images: one training step (forward, backward, fused AdamW) and forward_sr, in images/s.
All sides run in one process; the rounds alternate between the sides of a comparison.  Warm-up first, HIP events around every timed
call; a figure is the median of the round medians with the lowest and highest round.  The comparison side is always torch on the
same GPU in the same process, never an earlier run.  No threshold is set: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GP_WEIGHT = 1e-4                      # the YAML's sr_loss block


def event_ms(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def summary(rounds):
    return {"median_ms": round(statistics.median(rounds), 4), "lowest_ms": round(min(rounds), 4), "highest_ms": round(max(rounds), 4)}


def alternate(sides, rounds, iters):
    for _ in range(rounds):
        for fn, times in sides.values():
            times.append(event_ms(fn, iters))
    return {name: summary(times) for name, (_, times) in sides.items()}


def torch_sr_loss(sr, hr, gp_weight):
    """SRLoss's formula from torch ops (fp32, on sr's device)."""
    import torch
    import torch.nn.functional as F

    def gmap(x):
        p = F.pad(x, (1, 1, 1, 1))
        a = 0.5 * (p[..., 1:-1, 2:] - p[..., 1:-1, :-2])
        b = 0.5 * (p[..., :-2, 1:-1] - p[..., 2:, 1:-1])
        return torch.sqrt(a * a + b * b + 1e-6)
    mse = ((sr - hr) ** 2).flatten(1).mean(1)
    gp = (gmap(sr) - gmap(hr)).abs().flatten(1).mean(1)
    return (mse + gp_weight * gp).mean()


def case_loss(a):
    import torch
    from ccd_amd import ops
    from ccd_amd.loss.sr_loss import SRLoss
    dev = torch.device("cuda")
    N, H, W = a.batch, 32, 128
    g = torch.Generator().manual_seed(1)
    hr = torch.rand(N, 3, H, W, generator=g).to(dev)
    sr = (hr.cpu() + 0.1 * torch.randn(N, 3, H, W, generator=g)).to(dev)
    crit = SRLoss(GP_WEIGHT)
    sl = sr.clone().requires_grad_(True)

    def fused_raw():
        return ops.sr_loss_fwd(sr, hr, GP_WEIGHT), ops.sr_loss_bwd(sr, hr, GP_WEIGHT)

    def fused_autograd():
        sl.grad = None
        loss = crit(sl, hr)
        loss.backward()
        return loss

    def torch_autograd():
        sl.grad = None
        loss = torch_sr_loss(sl, hr, GP_WEIGHT)
        loss.backward()
        return loss

    out, grad = fused_raw()
    want = torch_autograd()
    agree = {"loss_fused": float(out[0]), "loss_torch": float(want.detach()),
             "max_abs_grad_difference": float((grad - sl.grad).abs().max()), "max_abs_grad": float(grad.abs().max())}
    res = {"shape": {"N": N, "C": 3, "H": H, "W": W}, "gp_weight": GP_WEIGHT, "agreement": agree}
    res.update(alternate({"fused_two_raw_calls": (fused_raw, []), "fused_through_autograd": (fused_autograd, []),
                          "torch_composition_through_autograd": (torch_autograd, [])}, a.rounds, a.iters))
    res["torch_over_fused_autograd"] = round(res["torch_composition_through_autograd"]["median_ms"] / res["fused_through_autograd"]["median_ms"], 2)
    return res


def case_upsample(a):
    import torch
    import torch.nn.functional as F
    from ccd_amd import ops
    from ccd_amd.dataset.datasetsupervised_kmeans import MEAN, STD
    dev = torch.device("cuda")
    lr = torch.rand(a.batch, 3, 16, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    mean, std = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)

    def fused():
        return ops.sr_upsample(lr, MEAN, STD)

    def torch_side():
        base = F.interpolate(lr, scale_factor=2, mode="bicubic", align_corners=False)
        return base, (base - mean) / std

    (b0, x0), (b1, x1) = fused(), torch_side()
    res = {"shape": {"N": a.batch, "C": 3, "h": 16, "w": 64},
           "agreement": {"max_abs_base_difference": float((b0 - b1).abs().max()), "max_abs_input_difference": float((x0 - x1).abs().max())}}
    res.update(alternate({"fused_one_launch": (fused, []), "torch_interpolate_then_normalise": (torch_side, [])}, a.rounds, a.iters))
    res["torch_over_fused"] = round(res["torch_interpolate_then_normalise"]["median_ms"] / res["fused_one_launch"]["median_ms"], 2)
    return res


def case_model(a):
    import torch
    from ccd_amd import superres as su
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = su.build_model(su.SuperResConfig(arch="vit_small", gp_weight=GP_WEIGHT), dev)
    opt = su.make_optimizer(model, lr=5e-4, weight_decay=0.05)
    ds = su.SyntheticPairSet(a.batch, seed=3)
    lr, hr = su.collate([ds[i] for i in range(a.batch)])
    lr, hr = lr.to(dev), hr.to(dev)
    iters = max(3, a.iters // 6)
    res = {"batch": a.batch, "arch": "vit_small", "weights": "random initialisation (rates, not accuracies)"}
    res.update(alternate({"training_step": (lambda: su.training_iteration(model, opt, lr, hr, 5e-4), []),
                          "forward_sr": (lambda: model.forward_sr(lr), [])}, a.rounds, iters))
    for name in ("training_step", "forward_sr"):
        res[name + "_images_per_s"] = round(a.batch / (res[name]["median_ms"] * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=224)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "superres_bench needs an MI355X"
    out = {"iters": a.iters, "rounds": a.rounds, "unit": "ms per call, HIP events (median of round medians; lowest and highest round)",
           "loss": case_loss(a), "upsample": case_upsample(a), "model": case_model(a)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
