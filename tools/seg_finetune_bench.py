#!/usr/bin/env python3
"""Time the text-segmentation finetuning path on the GPU.

    python tools/seg_finetune_bench.py [--iters 30] [--rounds 5] [--batch 224] [--out profiles/seg_finetune.json]

  loss   the fused supervised loss (kernels/seg_sup_loss.h), forward plus backward, at N = `batch` logits of 2 x 32 x 128, against
         the same formula composed from torch ops on the same GPU (log_softmax, sigmoid, two max_pool2d for the edge band, the
         masked sums; autograd for its backward).  Three forms of the fused side: the two raw calls, and SegSupLoss through autograd
         (what training runs).  The two sides' loss and gradient are compared first.
  model  DINO_Segment, vit_small, `batch` images: one training step (forward, backward, fused AdamW) and forward_mask, in images/s.
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

LOSS = dict(class_weight=(1.0, 2.0), dice_weight=0.5, edge_weight=1.0, edge_radius=2)      # the YAML's seg_loss block


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


def torch_seg_sup_loss(z, gt, class_weight, dice_weight, edge_weight, edge_radius, ignore_index=255):
    """SegSupLoss's formula from torch ops (fp32, on z's device)."""
    import torch
    import torch.nn.functional as F
    valid = (gt == 0) | (gt == 1)
    y = gt == 1
    logp = F.log_softmax(z, dim=1)
    l = -torch.where(y, logp[:, 1], logp[:, 0])
    p = torch.sigmoid(z[:, 1] - z[:, 0])
    w = torch.where(y, class_weight[1], class_weight[0]) * valid
    if edge_radius > 0 and edge_weight != 0:
        k = 2 * edge_radius + 1
        near_text = F.max_pool2d((y & valid).float()[:, None], k, 1, edge_radius)[:, 0] > 0
        near_bg = F.max_pool2d((~y & valid).float()[:, None], k, 1, edge_radius)[:, 0] > 0
        w = w * (1.0 + edge_weight * (valid & ((y & near_bg) | (~y & near_text))))
    omega = w.sum()
    ce = (w * l).sum() / omega.clamp_min(1e-30)
    yf, vf = (y & valid).float(), valid.float()
    I, P, G = (p * yf).flatten(1).sum(1), (p * vf).flatten(1).sum(1), yf.flatten(1).sum(1)
    has = vf.flatten(1).sum(1) > 0
    dice = ((1.0 - (2.0 * I + 1.0) / (P + G + 1.0)) * has).sum() / has.sum().clamp_min(1)
    return ce + dice_weight * dice


def case_loss(a):
    import torch
    from ccd_amd import ops
    from ccd_amd.loss.seg_loss import SegSupLoss
    dev = torch.device("cuda")
    N, H, W = a.batch, 32, 128
    g = torch.Generator().manual_seed(1)
    z = (2.0 * torch.randn(N, 2, H, W, generator=g)).to(dev)
    gt = (torch.rand(N, H, W, generator=g) < 0.3).to(torch.uint8)
    gt[torch.rand(N, H, W, generator=g) < 0.05] = 255
    gt = gt.to(dev)
    cw, dw, ew, r = LOSS["class_weight"], LOSS["dice_weight"], LOSS["edge_weight"], LOSS["edge_radius"]
    crit = SegSupLoss(**LOSS)
    zl = z.clone().requires_grad_(True)

    def fused_raw():
        out = ops.seg_sup_loss(z, gt, cw, 255, dw, ew, r)
        return out, ops.seg_sup_loss_bwd(z, out.code, out.ws, cw, dw, ew)

    def fused_autograd():
        zl.grad = None
        loss = crit(zl, gt)
        loss.backward()
        return loss

    def torch_autograd():
        zl.grad = None
        loss = torch_seg_sup_loss(zl, gt, cw, dw, ew, r)
        loss.backward()
        return loss

    out, grad = fused_raw()
    want = torch_autograd()
    agree = {"loss_fused": float(out[0]), "loss_torch": float(want.detach()),
             "max_abs_grad_difference": float((grad - zl.grad).abs().max()), "max_abs_grad": float(grad.abs().max())}
    sides = {"fused_two_raw_calls": (fused_raw, []), "fused_through_autograd": (fused_autograd, []),
             "torch_composition_through_autograd": (torch_autograd, [])}
    for _ in range(a.rounds):
        for fn, rounds in sides.values():
            rounds.append(event_ms(fn, a.iters))
    res = {"shape": {"N": N, "C": 2, "H": H, "W": W}, "parameters": {k: list(v) if isinstance(v, tuple) else v for k, v in LOSS.items()},
           "agreement": agree}
    for name, (_, rounds) in sides.items():
        res[name] = summary(rounds)
    res["torch_over_fused_autograd"] = round(res["torch_composition_through_autograd"]["median_ms"] / res["fused_through_autograd"]["median_ms"], 2)
    return res


def case_model(a):
    import torch
    from ccd_amd import segment as sg
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = sg.build_model(sg.SegmentConfig(arch="vit_small", **LOSS), dev)
    opt = sg.make_optimizer(model, lr=5e-4, weight_decay=0.05)
    ds = sg.SyntheticMaskSet(a.batch, seed=3)
    img, gt = sg.collate([ds[i] for i in range(a.batch)])
    img, gt = img.to(dev), gt.to(dev)
    iters = max(3, a.iters // 6)
    sides = {"training_step": (lambda: sg.training_iteration(model, opt, img, gt, 5e-4), []),
             "forward_mask": (lambda: model.forward_mask(img), [])}
    for _ in range(a.rounds):
        for fn, rounds in sides.values():
            rounds.append(event_ms(fn, iters))
    res = {"batch": a.batch, "arch": "vit_small"}
    for name, (_, rounds) in sides.items():
        res[name] = summary(rounds)
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
    assert torch.cuda.is_available(), "seg_finetune_bench needs an MI355X"
    out = {"iters": a.iters, "rounds": a.rounds, "unit": "ms per call, HIP events (median of round medians; lowest and highest round)",
           "loss": case_loss(a), "model": case_model(a)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
