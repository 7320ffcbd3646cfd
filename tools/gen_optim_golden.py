#!/usr/bin/env python3
"""Generate tests/golden/optim_cases.npz: the reference's `optimizer: sgd` and `optimizer: lars` paths on a handful of small named
tensors, recorded on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_optim_golden.py --reference <checkout of the reference>

The reference is imported (with the stub third-party modules of tools/oracle_stubs/), nothing of it is copied.  Every iteration
runs its own functions in train.py:244-252's order,

    clip_gradients(model, 3.0) -> cancel_gradients_last_layer(epoch, model, 1) -> optimizer.step()

with `optimizer` = torch.optim.SGD(get_params_groups(model), lr=0, momentum=0.9) or utils.LARS(get_params_groups(model)), lr
written into both groups and weight decay into group 0 before the step (train.py:238-242).  The "model" is a bag of named
parameters (the three functions only call named_parameters()).

Recorded: the initial parameters, every iteration's raw gradients / lr / wd / epoch, the parameters and the momentum buffers
after every iteration (with a flag: does the optimizer hold state for the tensor), and the key layout of both state_dict()s.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True

# (name, shape, gradient scale, what it is there for)
TENSORS = [
    ("backbone.blocks.0.mlp.fc1.weight", (24, 20), 1.0, "2-D weight, clipped"),
    ("backbone.pos_embed", (1, 8, 24), 1.0, "[1, T, E]: decayed AND adapted by LARS (ndim != 1)"),
    ("backbone.blocks.0.mlp.fc1.bias", (48,), 1.0, "bias: no decay, not adapted"),
    ("backbone.norm.weight", (200,), 1.0, "1-D weight: no decay, not adapted"),
    ("backbone.blocks.0.attn.proj.weight", (15, 20), 1e-3, "gradient norm stays under the clip"),
    ("head.last_layer.weight", (40, 33), 1.0, "cancelled while epoch < freeze_last_layer; two optimizer chunks"),
    ("backbone.cls_token", (1, 1, 24), 0.0, "never used: .grad stays None"),
    ("segmentor.zero_init.weight", (10, 13), 1.0, "all-zero parameter: LARS's |p| = 0 branch on its first step"),
]
NEVER_USED = {"backbone.cls_token"}
ZERO_INIT = {"segmentor.zero_init.weight"}
ITERS = 5
LR = [0.05, 0.11, 0.02, 0.3, 0.07]
WD = [0.04, 0.1, 0.25, 0.0, 0.4]
EPOCH = [0, 0, 1, 1, 2]           # freeze_last_layer = 1: the last layer is cancelled on the first two iterations
CLIP, FREEZE = 3.0, 1


class Bag:
    """What clip_gradients / cancel_gradients_last_layer / get_params_groups need of a model: named_parameters()."""

    def __init__(self, named):
        self.named = named

    def named_parameters(self):
        return iter(self.named)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference (holds Dino/)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "optim_cases.npz"))
    a = ap.parse_args()
    # REPO is NOT put on sys.path: its `Dino/` alias package would shadow the reference's
    sys.path.insert(0, os.path.join(HERE, "oracle_stubs"))
    sys.path.insert(0, os.path.abspath(a.reference))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or os.getcwd()) != REPO]
    import torch
    import Dino
    assert all(os.path.realpath(p).startswith(os.path.realpath(a.reference)) for p in Dino.__path__), Dino.__path__
    from Dino.modules import utils as R

    rng = np.random.RandomState(20240607)
    p0 = {n: (np.zeros(s, np.float32) if n in ZERO_INIT else (rng.standard_normal(s) * 0.5).astype(np.float32))
          for n, s, _, _ in TENSORS}
    grads = [{n: (rng.standard_normal(s) * 1.5 * sc).astype(np.float32) for n, s, sc, _ in TENSORS if n not in NEVER_USED}
             for _ in range(ITERS)]
    out = {"names": np.array([n for n, _, _, _ in TENSORS]), "lr": np.array(LR), "wd": np.array(WD), "epoch": np.array(EPOCH),
           "clip": np.array(CLIP), "freeze_last_layer": np.array(FREEZE), "never_used": np.array(sorted(NEVER_USED)),
           "momentum": np.array(0.9), "eta": np.array(0.001)}
    for i, (n, _, _, _) in enumerate(TENSORS):
        out[f"p0/{i}"] = p0[n]
        for it in range(ITERS):
            if n in grads[it]:
                out[f"g/{it}/{i}"] = grads[it][n]
    layouts = {}
    for kind in ("sgd", "lars"):
        params = [(n, torch.nn.Parameter(torch.from_numpy(p0[n].copy()))) for n, _, _, _ in TENSORS]
        model = Bag(params)
        groups = R.get_params_groups(model)
        opt = torch.optim.SGD(groups, lr=0, momentum=0.9) if kind == "sgd" else R.LARS(groups)
        key = "momentum_buffer" if kind == "sgd" else "mu"
        for it in range(ITERS):
            for gi, g in enumerate(opt.param_groups):
                g["lr"] = LR[it]
                if gi == 0:
                    g["weight_decay"] = WD[it]
            for n, p in params:
                p.grad = torch.from_numpy(grads[it][n].copy()) if n in grads[it] else None
            norms = R.clip_gradients(model, CLIP)
            R.cancel_gradients_last_layer(EPOCH[it], model, FREEZE)
            opt.step()
            out[f"{kind}/gnorm/{it}"] = np.array(norms, np.float64)
            for i, (n, p) in enumerate(params):
                out[f"{kind}/p/{it}/{i}"] = p.detach().numpy().copy()
                st = opt.state.get(p, {})
                has = st.get(key) is not None
                out[f"{kind}/buf/{it}/{i}"] = st[key].numpy().copy() if has else np.zeros(p.shape, np.float32)
                out[f"{kind}/has_state/{it}/{i}"] = np.array(has)
        sd = opt.state_dict()
        layouts[kind] = {"group_keys": [sorted(g) for g in sd["param_groups"]],
                         "group_params": [g["params"] for g in sd["param_groups"]],
                         "state_ids": sorted(sd["state"]),
                         "state_keys": sorted({k for st in sd["state"].values() for k in st}),
                         "group_names": [[n for n, p in params if any(p is q for q in g["params"])] for g in opt.param_groups]}
    out["layouts"] = np.array(json.dumps(layouts))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    print(json.dumps(layouts, indent=1))


if __name__ == "__main__":
    main()
