#!/usr/bin/env python3
"""Generate tests/golden/sinkhorn_cases.npz by running the REAL reference's DINOLoss.sinkhorn_knopp_teacher
(/root/reference/Dino/loss/Dino_loss.py:157-184, read-only) on the CPU, the way tools/gen_golden.py runs the rest of it: only the
numbers it returns for our seeded inputs are recorded, nothing of it is copied.  The method needs no process group.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_sinkhorn_golden.py

Per case: the fp32 logits (clamped cosine products, entries in [-1, 1]), the temperature, the iteration count, the reference's
fp32 assignment, the float64 restatement of tests/sinkhorn_np.py and the reference's own noise - its largest relative deviation
from the float64 value over the entries >= 1e-12.  The tests gate our kernels at a multiple of that noise.

The cases are sized for the 1 MiB limit on a committed file (16 bytes per entry: input, reference, float64): few rows with
K = 512 and 1000, K = 250 (no multiple of 4: the kernels' one-element loads), 130 rows (more than one 128-row chunk of the column
pass), both temperatures of the shipped schedules, one single-iteration case.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True
# REPO is NOT put on sys.path: its `Dino/` alias package would shadow the reference's namespace package (see tools/gen_golden.py)
sys.path.insert(0, os.path.join(HERE, "oracle_stubs"))
sys.path.insert(0, "/root/reference")
sys.path = [p for p in sys.path if os.path.realpath(p or os.getcwd()) != REPO]

import torch

import Dino as _ref_dino
assert all(os.path.realpath(p).startswith("/root/reference") for p in _ref_dino.__path__), _ref_dino
from Dino.loss.Dino_loss import DINOLoss

_spec = importlib.util.spec_from_file_location("sinkhorn_np", os.path.join(REPO, "tests", "sinkhorn_np.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

#        name              rows  K     temp  n  seed
CASES = (("r6_k512_t04",     6,  512, 0.04, 3, 1),
         ("r6_k512_t07",     6,  512, 0.07, 3, 2),
         ("r6_k512_t04_n1",  6,  512, 0.04, 1, 3),
         ("r24_k1000_t04",  24, 1000, 0.04, 3, 4),
         ("r24_k250_t07",   24,  250, 0.07, 3, 5),
         ("r130_k96_t07",  130,   96, 0.07, 3, 6))


def main():
    torch.set_num_threads(1)
    loss = DINOLoss(16, 2, 0.04, 0.04, 0, 10)
    out = {"names": np.array([c[0] for c in CASES])}
    for name, rows, k, temp, n, seed in CASES:
        t = R.cosine_logits(rows, k, seed)
        ref = loss.sinkhorn_knopp_teacher(torch.from_numpy(t.copy()), temp, n_iterations=n).numpy().astype(np.float32)
        f64 = R.restatement(t, temp, n)
        lin = R.linear(t, temp, n)
        assert ref.shape == t.shape and np.isfinite(ref).all()
        assert np.abs(lin - f64).max() < 1e-13, np.abs(lin - f64).max()
        noise = R.deviation(ref, f64)
        out[name + "/t"], out[name + "/temp"], out[name + "/n"] = t, np.float64(temp), np.int64(n)
        out[name + "/ref"], out[name + "/f64"], out[name + "/noise"] = ref, f64, np.float64(noise)
        print(f"{name}: rows {rows} K {k} temp {temp} n {n}: reference noise {noise:.3e}, "
              f"linear vs log-domain float64 {np.abs(lin - f64).max():.1e}")
    path = os.path.join(REPO, "tests", "golden", R.FIXTURE)
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
