#!/usr/bin/env python3
"""Time one batched call of each Dino.utils.DBSCAN clusterer (label / plane kernels) with HIP events on the current stream.

    python tools/cluster_bench.py [--batch 256] [--iters 50]

Masks: text-like masks of ccd_amd.synthetic plus random masks (the mix the GPU tests use).  Prints one JSON line: per clusterer
the mean time of a whole forward (labelling launch + uint8 plane expansion) and of the labelling launch alone."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ccd_amd import ops  # noqa: E402
from ccd_amd.synthetic import make_text_like_batch  # noqa: E402
from ccd_amd.utils.DBSCAN import DBSCAN_cluster, label_cluster, region_cluster  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cluster_bench needs an MI355X"
    half = a.batch // 2
    _, text, _ = make_text_like_batch(half, seed=1)
    rs = np.random.RandomState(2)
    rnd = (rs.uniform(size=(a.batch - half, 32, 128)) < rs.uniform(0.05, 0.6, size=(a.batch - half, 1, 1))).astype(np.float32)
    masks = torch.cat([text.float(), torch.from_numpy(rnd)]).contiguous().cuda()
    out = {"batch": a.batch, "iters": a.iters, "unit": "ms per batched call"}
    for name, cls, label_only in (("DBSCAN_cluster", DBSCAN_cluster, ops.dbscan_label),
                                  ("label_cluster", label_cluster, ops.ccl_label),
                                  ("region_cluster", region_cluster, ops.region_boxes)):
        f = cls()
        out[name] = {"forward": round(timed(lambda: f(masks), a.iters), 4),
                     "labelling_launch": round(timed(lambda: label_only(masks), a.iters), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
