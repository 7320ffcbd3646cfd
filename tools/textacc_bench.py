#!/usr/bin/env python3
"""Time the scoring half of TextAccuracy (ccd_amd/metric/eval_acc.py) on the GPU: the host path (tensor2idx + idx2str + update:
a softmax, three device-to-host copies and a Python loop per batch) against the device path (update_scores: ccd_text_score +
ccd_text_accumulate, no host synchronisation) of the same commit.

    python tools/textacc_bench.py [--iters 30] [--rounds 5] [--batches 8] [--out profiles/text_accuracy.json]

Cases.  (1) and (2): scoring one resident fp32 [512, 25, 93] batch of decoder scores against 512 ground-truth words of 3..15
characters (one character in ten of the prediction differs) on the host and on the device path - wall time per call, a host clock
around --iters calls that end in a device synchronise (the host path synchronises by itself; for the device path the clock covers
the enqueue and the drain), and for the device path also the two kernels alone, bracketed by HIP events.  (3): a whole
`compute()` of the ViT-Small recogniser of Dino/configs/CCD_vision_model_ARD.yaml over an in-memory loader of --batches batches of
512 images, device path and host path (score_table() forced to None), wall time including the final read.  Rounds of the two
paths alternate; a figure is the median of the round medians with the lowest and highest round (the run-to-run spread).  Both
paths must give the same totals, which is recorded.  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ccd_amd import finetune as ft, ops  # noqa: E402
from ccd_amd.convertor.attn import AttnConvertor  # noqa: E402
from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth  # noqa: E402
from ccd_amd.parallel import DataParallel  # noqa: E402

B, T = 512, 25


def make_batch(conv, dev, seed):
    """(scores fp32 [B, T, C] on the device: log-probabilities with 0.9 on the predicted class, ground-truth words)."""
    rs = np.random.RandomState(seed)
    C = conv.num_classes()
    words, rows = [], np.full((B, T), conv.padding_idx, dtype=np.int64)
    for row in rows:
        n = int(rs.randint(3, 16))
        cls = rs.randint(0, 90, size=n)
        words.append("".join(conv.idx2char[c] for c in cls))
        wrong = rs.rand(n) < 0.1
        row[:n] = np.where(wrong, rs.randint(0, 90, size=n), cls)
        row[n] = conv.end_idx
    s = (np.log(0.1 / (C - 1)) + rs.uniform(-0.01, 0.01, size=(B, T, C))).astype(np.float32)
    np.put_along_axis(s, rows[..., None], np.float32(np.log(0.9)), axis=-1)
    return torch.from_numpy(s).to(dev), words


def wall_ms(fn, iters):
    """ms per call: a host clock around `iters` calls and the synchronise that ends them."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_ms(fn, iters):
    """median ms of one call on the device (HIP events around every call, read after one synchronise)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "textacc_bench needs an MI355X"
    dev = torch.device("cuda")
    conv = AttnConvertor(dict_type="DICT90", with_unknown=True, max_seq_len=T)
    scores, words = make_batch(conv, dev, 1)
    out = {"batch": [B, T, conv.num_classes()], "iters": a.iters, "rounds": a.rounds,
           "unit": "ms per call (median of round medians; lowest and highest round)"}

    # ---- (1), (2): scoring one resident batch
    host_metric, dev_metric = TextAccuracy(), TextAccuracy()

    def host_path():
        idx, _ = conv.tensor2idx(scores)
        host_metric.update(words, conv.idx2str(idx))

    def device_path():
        dev_metric.update_scores(scores, words, conv)

    raw, norm = (torch.from_numpy(t).to(dev) for t in conv.score_table())
    codes, lens = (torch.from_numpy(x).to(dev) for x in encode_truth(words))
    totals = ops.text_totals(dev)

    def kernels_only():
        ops.text_accumulate(ops.text_score(scores, raw, norm, conv.end_idx, conv.padding_idx, codes, lens), totals)

    one_host, one_dev = TextAccuracy(), TextAccuracy()
    idx, _ = conv.tensor2idx(scores)
    one_host.update(words, conv.idx2str(idx))
    one_dev.update_scores(scores, words, conv)
    rh, rd = one_host.result(), one_dev.result()
    out["same_totals"] = all(rh[k] == rd[k] for k in ("ccr", "cwr", "ted", "ted/w", "words")) and abs(rh["ned"] - rd["ned"]) <= B * 2.0 ** -52 * rh["ned"]
    out["cwr"] = rd["cwr"]
    h_rounds, d_rounds, k_rounds = [], [], []
    for _ in range(a.rounds):
        h_rounds.append(wall_ms(host_path, a.iters))
        d_rounds.append(wall_ms(device_path, a.iters))
        k_rounds.append(event_ms(kernels_only, a.iters))
    h, d = summary(h_rounds), summary(d_rounds)
    out["score_batch"] = {"host_path_wall": h, "device_path_wall": d, "device_kernels_events": summary(k_rounds),
                          "speedup_wall": round(h["median_ms"] / d["median_ms"], 2),
                          "device_beats_host_beyond_spread": d["highest_ms"] < h["lowest_ms"]}

    # ---- (3): compute() over an in-memory loader
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(), dev, dropout=0.0)
    model.eval()
    wrapped = DataParallel(model)
    gen = torch.Generator().manual_seed(2)
    loader = [(torch.randn(B, 3, 32, 128, generator=gen), [tuple(make_words(conv, 10 + i))]) for i in range(a.batches)]
    table = AttnConvertor.score_table

    def compute(on_device):
        AttnConvertor.score_table = table if on_device else (lambda self: None)
        try:
            t0 = time.perf_counter()
            res = TextAccuracy().compute(wrapped, loader)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res
        finally:
            AttnConvertor.score_table = table

    (_, res_d), (_, res_h) = compute(True), compute(False)                     # warm-up of both paths; their totals
    out["compute_same_totals"] = all(res_d[k] == res_h[k] for k in ("ccr", "cwr", "ted", "ted/w", "words"))
    c_dev, c_host = [], []
    for _ in range(a.rounds):
        c_dev.append(compute(True)[0])
        c_host.append(compute(False)[0])
    cd, ch = summary(c_dev), summary(c_host)
    images = B * a.batches
    out["compute"] = {"images": images, "device_path_wall": cd, "host_path_wall": ch,
                      "device_images_per_s": round(images / (cd["median_ms"] * 1e-3)), "host_images_per_s": round(images / (ch["median_ms"] * 1e-3)),
                      "speedup_wall": round(ch["median_ms"] / cd["median_ms"], 2),
                      "device_beats_host_beyond_spread": cd["highest_ms"] < ch["lowest_ms"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


def make_words(conv, seed):
    rs = np.random.RandomState(seed)
    return ["".join(conv.idx2char[c] for c in rs.randint(0, 90, size=int(rs.randint(3, 16)))) for _ in range(B)]


if __name__ == "__main__":
    main()
