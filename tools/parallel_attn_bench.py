#!/usr/bin/env python3
"""Time the parallel attention recognition head on the GPU.

    python tools/parallel_attn_bench.py [--iters 20] [--rounds 5] [--batch 512] [--out profiles/parallel_attn_head.json]

  kernels  ccd_posattn_fwd and ccd_posattn_fwd + _bwd + _fold (kernels/posattn.h) at B = `batch`, E = 384, T = 25 on given P, X, Q0, We,
           against the same formula composed from torch ops on the same GPU in bf16 (tanh, the We product, softmax, bmm; autograd for
           its backward, which yields the same five gradients).  The two sides are compared first.
  model    DINO_Finetune, vit_small, `batch` images with the ParallelAttnDecoder: one training step (forward, backward, fused AdamW)
           and forward_test, in images/s, next to forward_test of the NRTR head (greedy) and of the CTC head (greedy) on the same box.
All sides run in one process; the rounds alternate between the sides of a comparison.  Warm-up first, HIP events around every timed
call; a figure is the median of the round medians with the lowest and highest round.  The comparison side is always the same GPU in
the same process, never an earlier run.  No threshold is set: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, T = 384, 25


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


def case_kernels(a):
    import torch
    from ccd_amd import ops
    dev = torch.device("cuda")
    N = a.batch
    g = torch.Generator().manual_seed(1)
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    P, X = bf(torch.randn(N * 256, E, generator=g)), bf(torch.randn(N * 256, E, generator=g))
    Q0 = bf(0.5 * torch.randn(256, E, generator=g))
    We = torch.zeros(32, E)
    We[:T] = torch.randn(T, E, generator=g) * 5.0 / E ** 0.5            # peaked maps (tests/parallel_attn_checks.py)
    We, be = bf(We), torch.randn(T, generator=g).to(dev)
    dG = torch.zeros(N, 32, E)
    dG[:, :T] = torch.randn(N, T, E, generator=g)
    dG = bf(dG.view(N * 32, E))
    leaves = [t.clone().requires_grad_(True) for t in (P, X, Q0, We[:T], be)]

    def torch_fwd(P, X, Q0, We, be):
        A = torch.tanh(P.view(N, 256, E) + Q0) @ We.t() + be.to(P.dtype)
        attn = A.float().softmax(dim=1).transpose(1, 2)                # [N, T, 256] fp32, as the kernel returns it
        return attn, attn.to(P.dtype) @ X.view(N, 256, E)

    def fused_fwd():
        return ops.posattn_fwd(P, X, Q0, We, be, T)

    def fused_fwd_bwd():
        attn, G = ops.posattn_fwd(P, X, Q0, We, be, T)
        return ops.posattn_bwd(dG, X, P, Q0, We, attn)

    def torch_fwd_only():
        with torch.no_grad():
            return torch_fwd(P, X, Q0, We[:T], be)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        _, G = torch_fwd(*leaves)
        G.backward(dG.view(N, 32, E)[:, :T])
        return leaves[0].grad

    attn, G = fused_fwd()
    ref_attn, ref_G = torch_fwd_only()
    dX1, dP, dQ0, dWe, dbe = fused_fwd_bwd()
    torch_fwd_bwd()
    agree = {"max_abs_attn_difference": float((attn - ref_attn).abs().max()),
             "max_abs_G_difference": float((G.view(N, 32, E)[:, :T].float() - ref_G.float()).abs().max()),
             "max_abs_dP_difference": float((dP.float() - leaves[0].grad.float()).abs().max()), "max_abs_dP": float(dP.float().abs().max()),
             "max_abs_dWe_difference": float((dWe[:T] - leaves[3].grad.float()).abs().max()), "max_abs_dWe": float(dWe.abs().max()),
             "median_peak_probability": float(attn.max(dim=2).values.median())}
    sides = {"fused_forward": (fused_fwd, []), "torch_forward": (torch_fwd_only, []),
             "fused_forward_backward": (fused_fwd_bwd, []), "torch_forward_backward": (torch_fwd_bwd, [])}
    for _ in range(a.rounds):
        for fn, rounds in sides.values():
            rounds.append(event_ms(fn, a.iters))
    res = {"shape": {"B": N, "E": E, "T": T, "tokens": 256}, "torch_side": "bf16 operands, fp32 softmax, autograd backward",
           "agreement": agree}
    for name, (_, rounds) in sides.items():
        res[name] = summary(rounds)
    res["torch_over_fused_forward"] = round(res["torch_forward"]["median_ms"] / res["fused_forward"]["median_ms"], 2)
    res["torch_over_fused_forward_backward"] = round(res["torch_forward_backward"]["median_ms"] / res["fused_forward_backward"]["median_ms"], 2)
    # algorithmic bytes of the forward: P, X, Q0 read once, attn and G written once
    nbytes = 2.0 * N * 256 * E * 2 + 256 * E * 2 + N * T * 256 * 4 + N * 32 * E * 2
    res["fused_forward_gigabytes_per_s"] = round(nbytes / (res["fused_forward"]["median_ms"] * 1e-3) / 1e9)
    return res


def case_model(a):
    import torch
    from ccd_amd import finetune as ft
    dev = torch.device("cuda")
    B = a.batch
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    iters = max(3, a.iters // 4)

    def build(kind):
        torch.manual_seed(0)
        cfg = ft.FinetuneConfig(arch="vit_small")
        if kind is not None:
            cfg.decoder_type = kind
        return ft.build_model(cfg, dev)

    par, nrtr, ctc = build("ParallelAttnDecoder"), build(None), build("CTCDecoder")
    words = ["recognition" if i % 3 else "text" for i in range(B)]
    targets = par.label_convertor.str2tensor(words).to(dev)
    opt = ft.make_optimizer(par)
    for m in (nrtr, ctc):
        m.eval()

    def par_eval():
        par.eval()
        with torch.no_grad():
            return par.forward_test(img)

    def par_train():
        par.train()
        return ft.training_iteration(par, opt, img, targets, 5e-4)

    def other_eval(m):
        def run():
            with torch.no_grad():
                return m.forward_test(img)
        return run

    sides = {"parallel_attn_training_step": (par_train, []), "parallel_attn_forward_test": (par_eval, []),
             "nrtr_greedy_forward_test": (other_eval(nrtr), []), "ctc_greedy_forward_test": (other_eval(ctc), [])}
    for _ in range(a.rounds):
        for fn, rounds in sides.values():
            rounds.append(event_ms(fn, iters))
    res = {"batch": B, "arch": "vit_small"}
    for name, (_, rounds) in sides.items():
        res[name] = summary(rounds)
        res[name + "_images_per_s"] = round(B / (res[name]["median_ms"] * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--only", choices=("kernels", "model"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "parallel_attn_bench needs an MI355X"
    out = {"iters": a.iters, "rounds": a.rounds, "unit": "ms per call, HIP events (median of round medians; lowest and highest round)"}
    if a.only != "model":
        out["kernels"] = case_kernels(a)
    if a.only != "kernels":
        out["model"] = case_model(a)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
