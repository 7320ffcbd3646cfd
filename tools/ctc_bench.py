#!/usr/bin/env python3
"""Time the CTC recognition head (kernels/ctc.h, ccd_amd/decoder/ctc_decoder.py) on the GPU.

    python tools/ctc_bench.py [--iters 30] [--rounds 5] [--out profiles/ctc_head.json]
    python tools/ctc_bench.py --cases beam --out profiles/ctc_beam.json

The cases, each in a process of its own under its own time limit; the next one starts only if the one before ended well (by
default the first three):
  loss    ccd_ctc_loss_fwd + _bwd on logits fp32 [512 * 32, 128] (92 classes), words of 3..15 characters, against
          F.log_softmax + F.ctc_loss(reduction='mean', zero_infinity=True) forward + backward of torch on the same GPU (the yardstick);
  step    one finetune step (forward, backward, AdamW) at B = 512, vit_small: CTC head and NRTR head in the same process, rounds
          alternating;
  infer   inference images/s at B = 512, vit_small, eval mode: CTC head (one pass) against NRTR greedy decoding (25 steps);
  beam    ccd_ctc_beam_search (kernels/ctc_beam.h) on probabilities fp32 [512, 32, 92] read from a 128-wide buffer, beam widths
          1, 4, 8, 16, next to ccd_ctc_greedy on the same buffer; then evaluation images/s at B = 512, vit_small (forward +
          TextAccuracy.update_scores, what TextAccuracy.compute does per batch) with beam_width 8 against greedy decoding.
  lexicon ccd_ctc_lexicon_score / ccd_ctc_lexicon_best (kernels/ctc_lexicon.h) on the same probabilities: scoring at V = 1000 and
          V = 10 000 words drawn from LEXICON_LENGTHS, scoring with a 50-word subset per image, the selection at nbest 1 and 16; the
          yardstick in the same process: ccd_ctc_loss_fwd on the pairs of a 64-word slice with replicated rows (a 537 MB buffer), as
          time per pair; then evaluation images/s at B = 512, vit_small, greedy against a 1000-word lexicon.
    python tools/ctc_bench.py --cases lexicon --out profiles/ctc_lexicon.json
  lm      ccd_ctc_beam_search_lm (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_LM>) on the same probabilities with random normalised tables of
          order 2 (34 KB) and 3 (3.1 MB), weight 0.5, bonus 0.8, eos on, beam widths 1, 4, 8, 16; ccd_ctc_beam_search at the same
          widths in the same process and the same rounds is the thing to compare with.
    python tools/ctc_bench.py --cases lm --out profiles/ctc_beam_lm.json
  align   ccd_ctc_align (kernels/ctc_align.h) at B = 512, T = 32, C = 92, words of 2..15 characters, on logits in a 128-wide buffer;
          ccd_ctc_loss_fwd (the yardstick: the same lane mapping, a strictly heavier recursion) and ccd_ctc_greedy in the same process
          on the same buffer; the same kernel on the fp32 softmax (normalized = 1) and with `rows` mapping 8 targets to every sample;
          then evaluation images/s at B = 512, vit_small: forward + TextAccuracy.update_scores, without and with what test.py
          --alignments adds per batch (CTCConvertor.tensor2chars: decode, align, one copy to the host, the host-side records).
    python tools/ctc_bench.py --cases align --out profiles/ctc_align.json
  trie    ccd_ctc_beam_search_trie (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_TRIE>) and the two-stage ops.ctc_lexicon_search on the same
          probabilities with synthetic lexicons of 1 000 / 10 000 / 90 000 words of 2..15 characters: the trie kernel at beam widths 4,
          8, 16; the sort + subset rescoring + selection behind it; the whole search; in the same process and the same rounds the
          exhaustive ccd_ctc_lexicon_score + ccd_ctc_lexicon_best on the same inputs and ccd_ctc_beam_search at the same widths; the host
          build time and the size of each trie; the share of samples whose searched best word is the exhaustive best (recorded, not
          gated: synthetic frames are not a recogniser's); then evaluation images/s at B = 512, vit_small, with a 10 000-word lexicon,
          exhaustive against lexicon_beam 16.
    python tools/ctc_bench.py --cases trie --out profiles/ctc_lexicon_trie.json
Warm-up first, HIP events around every timed call, a figure is the median of the round medians with the lowest and highest
round.  No threshold is set; the file records what was measured.  `--case NAME` runs one case and prints its JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, C = 512, 32, 92
LIMITS = {"loss": 240, "step": 420, "infer": 300, "beam": 300, "lexicon": 420, "lm": 240, "align": 300, "trie": 540}           # seconds per case
# word length -> share in per cent of a lexicon of `lexicon`: the shape of an English word list (mode 5 - 7 characters, a tail to 15)
LEXICON_LENGTHS = {2: 2, 3: 6, 4: 11, 5: 14, 6: 15, 7: 14, 8: 12, 9: 9, 10: 7, 11: 4, 12: 3, 13: 1, 14: 1, 15: 1}


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


def _targets(conv, seed):
    import numpy as np
    rs = np.random.RandomState(seed)
    words = ["".join(conv.idx2char[1 + c] for c in rs.randint(0, 90, size=int(rs.randint(3, 16)))) for _ in range(B)]
    return conv.str2tensor(words)


def case_loss(a):
    import torch
    import torch.nn.functional as F
    from ccd_amd import ops
    from ccd_amd.convertor.ctc import CTCConvertor
    dev = torch.device("cuda")
    targets = _targets(CTCConvertor(), 1).to(dev)
    g = torch.Generator().manual_seed(2)
    buf = torch.zeros(B * T, 128)
    buf[:, :C] = torch.randn(B * T, C, generator=g) * 2.0
    buf = buf.to(dev)
    one = torch.ones(1, device=dev)

    def ours():
        _, _, ws = ops.ctc_loss_fwd(buf, C, targets, T)
        ops.ctc_loss_bwd(buf, C, targets, T, ws, one, 128)

    lengths = (targets != 0).sum(1)
    flat = targets[targets != 0]
    frames = torch.full((B,), T, dtype=torch.long, device=dev)
    x = buf[:, :C].reshape(B, T, C).contiguous().requires_grad_(True)

    def torchs():
        x.grad = None
        lp = F.log_softmax(x, -1).transpose(0, 1)
        F.ctc_loss(lp, flat, frames, lengths, blank=0, reduction="mean", zero_infinity=True).backward()

    # the two must agree before either is timed
    nll, acc, ws = ops.ctc_loss_fwd(buf, C, targets, T)
    torchs()
    d = ops.ctc_loss_bwd(buf, C, targets, T, ws, one, 128)[:, :C].float().view(B, T, C)
    ref = F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), flat, frames, lengths, blank=0, reduction="mean", zero_infinity=True)
    out = {"shape": [B, T, C], "loss_kernel": float(acc[0] / acc[1]), "loss_torch": float(ref),
           "max_gradient_difference": float((d - x.grad).abs().max())}
    ours_r, torch_r = [], []
    for _ in range(a.rounds):
        ours_r.append(event_ms(ours, a.iters))
        torch_r.append(event_ms(torchs, a.iters))
    o, t = summary(ours_r), summary(torch_r)
    out.update({"kernels_fwd_bwd": o, "torch_log_softmax_ctc_loss_fwd_bwd": t, "torch_over_kernels": round(t["median_ms"] / o["median_ms"], 2),
                "kernels_not_slower_beyond_spread": o["highest_ms"] <= t["lowest_ms"]})
    return out


def _models(dropout=None):
    import torch
    from ccd_amd import finetune as ft
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_type = "CTCDecoder"
    return ft.build_model(cfg, dev, dropout=dropout), ft.build_model(ft.FinetuneConfig(), dev, dropout=dropout)


def case_step(a):
    import torch
    from ccd_amd import finetune as ft
    dev = torch.device("cuda")
    ctc, nrtr = _models()
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(3)).to(dev)
    words = ["".join(ctc.label_convertor.idx2char[1 + (i * 7 + j) % 90] for j in range(3 + i % 13)) for i in range(B)]
    sides = []
    for model in (ctc, nrtr):
        sides.append((model, ft.make_optimizer(model), model.label_convertor.str2tensor(words).to(dev)))
    rounds = ([], [])
    iters = max(3, a.iters // 3)
    for _ in range(a.rounds):
        for k, (model, opt, tg) in enumerate(sides):
            rounds[k].append(event_ms(lambda: ft.training_iteration(model, opt, img, tg, 1e-4), iters))
    c, n = summary(rounds[0]), summary(rounds[1])
    return {"batch": B, "arch": "vit_small", "ctc_step": c, "nrtr_step": n, "nrtr_over_ctc": round(n["median_ms"] / c["median_ms"], 2)}


def case_infer(a):
    import torch
    dev = torch.device("cuda")
    ctc, nrtr = _models(dropout=0.0)
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    rounds = ([], [])
    iters = max(3, a.iters // 3)
    with torch.no_grad():
        for model in (ctc, nrtr):
            model.eval()
        for _ in range(a.rounds):
            for k, model in enumerate((ctc, nrtr)):
                rounds[k].append(event_ms(lambda: model(img, None, return_loss=False), iters))
    c, n = summary(rounds[0]), summary(rounds[1])
    return {"batch": B, "arch": "vit_small", "ctc_forward": c, "nrtr_greedy": n, "ctc_images_per_s": round(B / (c["median_ms"] * 1e-3)),
            "nrtr_images_per_s": round(B / (n["median_ms"] * 1e-3))}


def case_beam(a):
    import torch
    from ccd_amd import finetune as ft, ops
    from ccd_amd.metric.eval_acc import TextAccuracy
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, T, C, generator=g)                               # moderately peaked frames: 60 % a character, else the blank
    peak = torch.where(torch.rand(B, T, generator=g) < 0.6, torch.randint(0, C, (B, T), generator=g), torch.zeros(B, T, dtype=torch.long))
    logits.scatter_add_(2, peak[..., None], 2.0 + 6.0 * torch.rand(B, T, 1, generator=g))
    buf = torch.zeros(B * T, 128)
    buf[:, :C] = logits.softmax(-1).reshape(B * T, C)
    probs = buf.to(dev).view(B, T, 128)[:, :, :C]
    out = {"shape": [B, T, C], "input": "fp32 probabilities, normalized = 1"}
    widths = (1, 4, 8, 16)
    rounds = {w: [] for w in widths}
    greedy = []
    for _ in range(a.rounds):
        greedy.append(event_ms(lambda: ops.ctc_greedy(probs), a.iters))
        for w in widths:
            rounds[w].append(event_ms(lambda: ops.ctc_beam_search(probs, w, normalized=True), a.iters))
    out["ctc_greedy"] = summary(greedy)
    for w in widths:
        out[f"ctc_beam_search_w{w}"] = summary(rounds[w])
    best = ops.ctc_beam_search(probs, 16, normalized=True)
    path, length, _ = ops.ctc_greedy(probs)
    same = ((best[0][:, 0] == path).all(1) & (best[1][:, 0] == length)).sum()
    out["samples_whose_best_word_at_w16_is_not_the_greedy_word"] = int(B - same)
    # evaluation: forward + scoring, the body of TextAccuracy.compute
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_type = "CTCDecoder"
    model = ft.build_model(cfg, dev, dropout=0.0).eval()
    conv = model.label_convertor
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    words = ["".join(conv.idx2char[1 + (i * 7 + j) % 90] for j in range(3 + i % 13)) for i in range(B)]
    metric = TextAccuracy()

    def evaluate():
        metric.update_scores(model(img, text=None, return_loss=False, test_speed=False).float(), words, conv)

    sides = {0: [], 8: []}
    iters = max(3, a.iters // 3)
    with torch.no_grad():
        for _ in range(a.rounds):
            for width in sides:
                conv.beam_width = width
                sides[width].append(event_ms(evaluate, iters))
    g0, b8 = summary(sides[0]), summary(sides[8])
    out.update({"batch": B, "arch": "vit_small", "evaluate_greedy": g0, "evaluate_beam_width_8": b8,
                "greedy_images_per_s": round(B / (g0["median_ms"] * 1e-3)), "beam_width_8_images_per_s": round(B / (b8["median_ms"] * 1e-3))})
    return out


def _peaked_probs(seed):
    """fp32 probabilities [B, T, C] on the GPU, a view of a 128-wide buffer: moderately peaked frames, as case_beam's."""
    import torch
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, C, generator=g)
    peak = torch.where(torch.rand(B, T, generator=g) < 0.6, torch.randint(0, C, (B, T), generator=g), torch.zeros(B, T, dtype=torch.long))
    logits.scatter_add_(2, peak[..., None], 2.0 + 6.0 * torch.rand(B, T, 1, generator=g))
    buf = torch.zeros(B * T, 128)
    buf[:, :C] = logits.softmax(-1).reshape(B * T, C)
    return buf.to("cuda").view(B, T, 128)[:, :, :C]


def _lexicon_words(V, seed):
    """int64 [V, 15]: V distinct words of classes 1..90 whose lengths follow LEXICON_LENGTHS."""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed)
    lengths = rs.choice(list(LEXICON_LENGTHS), size=V, p=np.array(list(LEXICON_LENGTHS.values())) / 100.0)
    words = np.zeros((V, max(LEXICON_LENGTHS)), dtype=np.int64)
    seen = set()
    for row, n in zip(words, lengths):
        while True:
            w = tuple(rs.randint(1, 91, size=n))
            if w not in seen:
                seen.add(w)
                row[:n] = w
                break
    return torch.from_numpy(words)


def case_lexicon(a):
    import torch
    from ccd_amd import finetune as ft, ops
    from ccd_amd.metric.eval_acc import TextAccuracy
    dev = torch.device("cuda")
    probs = _peaked_probs(5)
    out = {"shape": [B, T, C], "input": "fp32 probabilities, normalized = 1", "word_length_per_cent": LEXICON_LENGTHS}
    lex = {V: ops.ctc_lexicon(_lexicon_words(V, 6)) for V in (1000, 10000)}
    subset = torch.stack([torch.randperm(1000, generator=torch.Generator().manual_seed(b))[:50] for b in range(B)]).to(torch.int32).to(dev)
    iters = max(3, a.iters // 3)
    score = {V: [] for V in lex}
    sub, pick1, pick16, yard = [], [], [], []
    scores = ops.ctc_lexicon_score(probs, lex[1000], normalized=True)
    # the yardstick: the loss kernel on the pairs (sample, word) of the lexicon's first 64 words, every pair with its own copy of the rows
    logp = probs.log()
    rows = torch.zeros(B * 64 * T, 128, device=dev)
    rows.view(B, 64, T, 128)[..., :C] = logp[:, None]
    targets = torch.zeros(B * 64, 31, dtype=torch.long, device=dev)
    targets[:, :15] = lex[1000].words[:64].to(dev).repeat(B, 1)
    nll = ops.ctc_loss_fwd(rows, C, targets, T)[0].view(B, 64)
    out["largest_difference_to_the_loss_kernel"] = float((scores[:, :64] + nll).abs().max())
    for _ in range(a.rounds):
        for V in lex:
            score[V].append(event_ms(lambda: ops.ctc_lexicon_score(probs, lex[V], normalized=True), iters))
        sub.append(event_ms(lambda: ops.ctc_lexicon_score(probs, lex[1000], normalized=True, subset=subset), a.iters))
        pick1.append(event_ms(lambda: ops.ctc_lexicon_best(scores, 1), a.iters))
        pick16.append(event_ms(lambda: ops.ctc_lexicon_best(scores, 16), a.iters))
        yard.append(event_ms(lambda: ops.ctc_loss_fwd(rows, C, targets, T), iters))
    for V in lex:
        r = summary(score[V])
        out[f"ctc_lexicon_score_v{V}"] = {**r, "pairs_per_s": round(B * V / (r["median_ms"] * 1e-3)), "ns_per_pair": round(r["median_ms"] * 1e6 / (B * V), 2)}
    out["ctc_lexicon_score_subset_50_of_1000"] = summary(sub)
    out["ctc_lexicon_best_nbest1_v1000"], out["ctc_lexicon_best_nbest16_v1000"] = summary(pick1), summary(pick16)
    y = summary(yard)
    out["yardstick_ctc_loss_fwd_64_words_replicated"] = {**y, "buffer_bytes": rows.numel() * 4, "ns_per_pair": round(y["median_ms"] * 1e6 / (B * 64), 2)}
    out["yardstick_over_lexicon_per_pair"] = round(out["yardstick_ctc_loss_fwd_64_words_replicated"]["ns_per_pair"] /
                                                    out["ctc_lexicon_score_v1000"]["ns_per_pair"], 2)
    del rows, targets, logp
    # evaluation: forward + scoring, the body of TextAccuracy.compute
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_type = "CTCDecoder"
    model = ft.build_model(cfg, dev, dropout=0.0).eval()
    conv = model.label_convertor
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    words = ["".join(conv.idx2char[1 + (i * 7 + j) % 90] for j in range(3 + i % 13)) for i in range(B)]
    table = lex[1000].words
    strings = conv.idx2str([row[row != 0].tolist() for row in table])
    metric = TextAccuracy()

    def evaluate():
        metric.update_scores(model(img, text=None, return_loss=False, test_speed=False).float(), words, conv)

    sides = {"greedy": [], "lexicon": []}
    with torch.no_grad():
        for _ in range(a.rounds):
            for name in sides:
                conv.set_lexicon(strings if name == "lexicon" else None)
                sides[name].append(event_ms(evaluate, iters))
    g0, l1 = summary(sides["greedy"]), summary(sides["lexicon"])
    out.update({"batch": B, "arch": "vit_small", "evaluate_greedy": g0, "evaluate_lexicon_1000": l1,
                "greedy_images_per_s": round(B / (g0["median_ms"] * 1e-3)), "lexicon_1000_images_per_s": round(B / (l1["median_ms"] * 1e-3))})
    return out


def case_lm(a):
    import torch
    from ccd_amd import ops
    probs = _peaked_probs(5)
    g = torch.Generator().manual_seed(9)
    lms = {order: ops.ctc_char_lm((1.5 * torch.randn(C ** (order - 1), C, generator=g)).log_softmax(-1), order) for order in (2, 3)}
    widths = (1, 4, 8, 16)
    out = {"shape": [B, T, C], "input": "fp32 probabilities, normalized = 1", "weight": 0.5, "bonus": 0.8, "eos": 1,
           "table_bytes": {f"order{o}": int(lm.table.numel() * 4) for o, lm in lms.items()}}
    plain = {w: [] for w in widths}
    fused = {(o, w): [] for o in lms for w in widths}
    for _ in range(a.rounds):
        for w in widths:
            plain[w].append(event_ms(lambda: ops.ctc_beam_search(probs, w, normalized=True), a.iters))
            for o, lm in lms.items():
                fused[o, w].append(event_ms(lambda: ops.ctc_beam_search_lm(probs, w, lm, 0.5, 0.8, True, normalized=True), a.iters))
    for w in widths:
        out[f"ctc_beam_search_w{w}"] = summary(plain[w])
        for o in lms:
            r = summary(fused[o, w])
            out[f"ctc_beam_search_lm_order{o}_w{w}"] = {**r, "over_plain": round(r["median_ms"] / out[f"ctc_beam_search_w{w}"]["median_ms"], 3)}
    best = ops.ctc_beam_search(probs, 16, normalized=True)
    for o, lm in lms.items():
        with_lm = ops.ctc_beam_search_lm(probs, 16, lm, 0.5, 0.8, True, normalized=True)
        same = ((best[0][:, 0] == with_lm[0][:, 0]).all(1) & (best[1][:, 0] == with_lm[1][:, 0])).sum()
        out[f"samples_whose_best_word_at_w16_changes_with_the_order{o}_table"] = int(B - same)
    return out


def case_align(a):
    import numpy as np
    import torch
    from ccd_amd import finetune as ft, ops
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy
    dev = torch.device("cuda")
    conv = CTCConvertor()
    rs = np.random.RandomState(1)
    K = 8
    strings = ["".join(conv.idx2char[1 + c] for c in rs.randint(0, 90, size=int(rs.randint(2, 16)))) for _ in range(B * K)]
    many = conv.str2tensor(strings)[:, :15].contiguous().to(dev)               # 8 targets per sample
    targets = many[::K].contiguous()                                           # one per sample
    rows = torch.arange(B, dtype=torch.int32).repeat_interleave(K).to(dev)
    g = torch.Generator().manual_seed(2)
    buf = torch.zeros(B * T, 128)
    buf[:, :C] = torch.randn(B * T, C, generator=g) * 2.0
    pbuf = torch.zeros(B * T, 128)
    pbuf[:, :C] = buf[:, :C].softmax(-1)
    buf, pbuf = buf.to(dev), pbuf.to(dev)
    logits, probs = buf.view(B, T, 128)[:, :, :C], pbuf.view(B, T, 128)[:, :, :C]
    # max <= sum before anything is timed
    score = ops.ctc_align(logits, targets)[3]
    nll = ops.ctc_loss_fwd(buf, C, targets, T)[0]
    out = {"shape": [B, T, C], "words": "2..15 characters", "largest_score_plus_nll": float((score + nll).max()),
           "rows_equal_replicated": bool(torch.equal(ops.ctc_align(logits, many, rows=rows)[3][::K], score))}
    assert out["largest_score_plus_nll"] <= 1e-4 and out["rows_equal_replicated"]
    sides = {"ctc_align_logits": lambda: ops.ctc_align(logits, targets),
             "ctc_loss_fwd_same_rows": lambda: ops.ctc_loss_fwd(buf, C, targets, T),
             "ctc_greedy_same_buffer": lambda: ops.ctc_greedy(logits),
             "ctc_align_probabilities": lambda: ops.ctc_align(probs, targets, normalized=True),
             "ctc_align_rows_8_per_sample": lambda: ops.ctc_align(probs, many, normalized=True, rows=rows)}
    rounds = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, fn in sides.items():
            rounds[name].append(event_ms(fn, a.iters))
    for name in sides:
        out[name] = summary(rounds[name])
    out["loss_fwd_over_align"] = round(out["ctc_loss_fwd_same_rows"]["median_ms"] / out["ctc_align_logits"]["median_ms"], 2)
    out["align_faster_than_loss_fwd_beyond_spread"] = out["ctc_align_logits"]["highest_ms"] < out["ctc_loss_fwd_same_rows"]["lowest_ms"]
    out["rows_8_ns_per_target"] = round(out["ctc_align_rows_8_per_sample"]["median_ms"] * 1e6 / (B * K), 1)
    # evaluation: forward + scoring, the body of TextAccuracy.compute, without and with the hook of test.py --alignments
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_type = "CTCDecoder"
    model = ft.build_model(cfg, dev, dropout=0.0).eval()
    conv = model.label_convertor
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    words = ["".join(conv.idx2char[1 + (i * 7 + j) % 90] for j in range(3 + i % 13)) for i in range(B)]
    metric = TextAccuracy()

    def evaluate(alignments):
        probs = model(img, text=None, return_loss=False, test_speed=False).float()
        metric.update_scores(probs, words, conv)
        if alignments:
            conv.tensor2chars(probs, nbest=1, normalized=True)

    ev = {False: [], True: []}
    iters = max(3, a.iters // 3)
    with torch.no_grad():
        for _ in range(a.rounds):
            for flag in ev:
                ev[flag].append(event_ms(lambda: evaluate(flag), iters))
    e0, e1 = summary(ev[False]), summary(ev[True])
    out.update({"batch": B, "arch": "vit_small", "evaluate_greedy": e0, "evaluate_greedy_with_alignments": e1,
                "greedy_images_per_s": round(B / (e0["median_ms"] * 1e-3)),
                "with_alignments_images_per_s": round(B / (e1["median_ms"] * 1e-3))})
    return out


def case_trie(a):
    import time
    import torch
    from ccd_amd import finetune as ft, ops
    from ccd_amd.metric.eval_acc import TextAccuracy
    dev = torch.device("cuda")
    probs = _peaked_probs(5)
    out = {"shape": [B, T, C], "input": "fp32 probabilities, normalized = 1", "word_length_per_cent": LEXICON_LENGTHS}
    widths = (4, 8, 16)
    sizes = (1000, 10000, 90000)
    last = torch.iinfo(torch.int32).max

    def rescore(ids, lexicon):
        ids = torch.where(ids < 0, last, ids).sort(dim=1).values
        ids = torch.where(ids == last, -1, ids).contiguous()
        return ops.ctc_lexicon_best(ops.ctc_lexicon_score(probs, lexicon, normalized=True, subset=ids), 1)

    def exhaustive(lexicon):
        return ops.ctc_lexicon_best(ops.ctc_lexicon_score(probs, lexicon, normalized=True), 1)

    plain = {w: [] for w in widths}
    tables = {}
    for V in sizes:
        lexicon = ops.ctc_lexicon(_lexicon_words(V, 6))
        build = []
        for _ in range(3):
            t0 = time.perf_counter()
            trie = ops.ctc_lexicon_trie(lexicon)
            build.append((time.perf_counter() - t0) * 1e3)
        tables[V] = trie
        trie.on(dev)
        iters = max(3, a.iters // (3 if V < 90000 else 6))
        kernel, behind, whole = ({w: [] for w in widths} for _ in range(3))
        full = []
        proposals = {w: ops.ctc_beam_search_trie(probs, w, trie, normalized=True)[3] for w in widths}
        for _ in range(a.rounds):
            for w in widths:
                kernel[w].append(event_ms(lambda: ops.ctc_beam_search_trie(probs, w, trie, normalized=True), a.iters))
                behind[w].append(event_ms(lambda: rescore(proposals[w], lexicon), a.iters))
                whole[w].append(event_ms(lambda: ops.ctc_lexicon_search(probs, trie, w, normalized=True), a.iters))
                if V == sizes[0]:
                    plain[w].append(event_ms(lambda: ops.ctc_beam_search(probs, w, normalized=True), a.iters))
            full.append(event_ms(lambda: exhaustive(lexicon), iters))
        rec = {"trie": {**trie.stats, "host_build_ms": round(statistics.median(build), 1)},
               "exhaustive_ctc_lexicon_score_plus_best": summary(full)}
        want = exhaustive(lexicon)[0][:, 0]
        for w in widths:
            ids, _ = ops.ctc_lexicon_search(probs, trie, w, normalized=True)
            rec[f"w{w}"] = {"ctc_beam_search_trie": summary(kernel[w]), "sort_subset_rescoring_selection": summary(behind[w]),
                            "ctc_lexicon_search": summary(whole[w]),
                            "exhaustive_over_search": round(rec["exhaustive_ctc_lexicon_score_plus_best"]["median_ms"] /
                                                            statistics.median(whole[w]), 2),
                            "search_faster_than_exhaustive_beyond_spread": max(whole[w]) < min(full),
                            "share_of_samples_whose_best_is_the_exhaustive_best": round(float((ids[:, 0] == want).float().mean()), 4),
                            "share_of_samples_with_a_word": round(float((ids[:, 0] >= 0).float().mean()), 4)}
        out[f"v{V}"] = rec
        del want
    for w in widths:
        out[f"ctc_beam_search_w{w}"] = summary(plain[w])
    # evaluation: forward + scoring, the body of TextAccuracy.compute, with the 10 000-word lexicon
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_type = "CTCDecoder"
    model = ft.build_model(cfg, dev, dropout=0.0).eval()
    conv = model.label_convertor
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    words = ["".join(conv.idx2char[1 + (i * 7 + j) % 90] for j in range(3 + i % 13)) for i in range(B)]
    strings = conv.idx2str([row[row != 0].tolist() for row in tables[10000].lexicon.words])
    metric = TextAccuracy()

    def evaluate():
        metric.update_scores(model(img, text=None, return_loss=False, test_speed=False).float(), words, conv)

    sides = {0: [], 16: []}
    iters = max(3, a.iters // 3)
    conv.set_lexicon(strings, beam=16)                                         # (builds the trie; the width is switched per side)
    with torch.no_grad():
        for _ in range(a.rounds):
            for beam in sides:
                conv.lexicon_beam = beam
                sides[beam].append(event_ms(evaluate, iters))
    e0, e16 = summary(sides[0]), summary(sides[16])
    out.update({"batch": B, "arch": "vit_small", "evaluate_lexicon_10000_exhaustive": e0, "evaluate_lexicon_10000_lexicon_beam_16": e16,
                "exhaustive_images_per_s": round(B / (e0["median_ms"] * 1e-3)),
                "lexicon_beam_16_images_per_s": round(B / (e16["median_ms"] * 1e-3))})
    return out


CASES = {"trie": case_trie, "align": case_align, "loss": case_loss, "step": case_step, "infer": case_infer, "beam": case_beam, "lexicon": case_lexicon, "lm": case_lm}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    ap.add_argument("--cases", default="loss,step,infer", help="comma-separated cases of a whole run, in order")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), "ctc_bench needs an MI355X"
        print(json.dumps({a.case: CASES[a.case](a)}))
        return
    out = {"iters": a.iters, "rounds": a.rounds, "unit": "ms per call, HIP events (median of round medians; lowest and highest round)"}
    names = [n for n in a.cases.split(",") if n]
    assert names and all(n in CASES for n in names), f"--cases takes names out of {sorted(CASES)}"
    for name in names:
        # a fresh process per case under its own time limit; a case that fails or runs out of time ends the run
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--iters", str(a.iters), "--rounds", str(a.rounds)],
                             capture_output=True, text=True, timeout=LIMITS[name])
        if run.returncode != 0:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            sys.exit(f"ctc_bench: case {name} ended with status {run.returncode}; nothing further was started")
        out.update(json.loads(run.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
