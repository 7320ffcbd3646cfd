#!/usr/bin/env python3
"""Time beam search over the NRTR decoder (kernels/nrtr_beam.h, finetune_engine.beam_decode) on the GPU.

    python tools/nrtr_beam_bench.py [--iters 30] [--rounds 5] [--out profiles/nrtr_beam.json]
    python tools/nrtr_beam_bench.py --cases trie --out profiles/nrtr_beam_trie.json
    python tools/nrtr_beam_bench.py --cases score --out profiles/nrtr_score.json
    python tools/nrtr_beam_bench.py --cases joint --out profiles/nrtr_beam_joint.json
    python tools/nrtr_beam_bench.py --cases twopass --out profiles/nrtr_twopass.json

The cases, each in a process of its own under its own time limit; the next one starts only if the one before ended well:
  kernels  ccd_nrtr_beam_step and ccd_nrtr_beam_reorder per launch at B = 512, T = 25, C = 92 (logits rows 128 wide), D = 512,
           L = 6, beam widths 1, 4, 8, 16.  The step kernel runs on a state some steps into a peaked random decode; the reorder
           kernel permutes positions 0..12 and 0..24 by a random permutation per sample, so every row moves (the worst case: in a
           decode the slots that keep their rank move nothing), with the bytes it reads and writes and the rate;
  eval     evaluation images/s at B = 512, vit_small, eval mode: forward_test (greedy, HIP graph) against forward_beam at widths
           1, 4, 8 (HIP graph), rounds alternating;
  rescore  the yardstick of tests/test_nrtr_beam_gpu.py: with that test's model (vit_tiny, 2 decoder layers, its seed, images and
           <EOS> bias) the largest |sum log p_incremental - sum log p_full| along the greedy paths of greedy_decode against
           greedy_decode_full ("rescore_base"; the test gates the beam's scores against teacher forcing at 4 x that).
  trie     (not part of a default run) the lexicon-constrained beam: ccd_nrtr_beam_step_trie per launch at widths 4, 8, 16 over
           synthetic lexicons of 1 000 / 10 000 / 90 000 words of 2..15 characters, next to ccd_nrtr_beam_step in the same process
           on the same logits, both on a state eight steps into their own decode (with how many of its slots are still live: a
           finished slot costs no log-softmax); then evaluation images/s at B = 512, vit_small: forward_lexicon with lexicon_beam
           8 and 16 (the 10 000-word lexicon) against forward_beam at widths 8 and 16, rounds alternating.
  score    (not part of a default run) scoring given words (kernels/nrtr_score.h): ccd_xattn_rows_fwd at B = 64 images with 50 words
           each (R = 3 200 rows of 26 queries, 8 heads) against ccd_dec_attn_fwd on K / V replicated per row - the same process, the same
           q, rounds alternating, the outputs compared bit for bit first - with the bytes each side has to move and the rate, and at
           B = 512 x 50 (R = 25 600) alone, with and without moments; ccd_nrtr_word_score at R = 25 600, T = 26, C = 92, per launch and
           per row; then evaluation images/s at B = 512, vit_small: forward_words with 50 words per image against forward_lexicon at
           lexicon_beam 16 over the same 50 words, rounds alternating.
  joint    (not part of a default run) joint CTC / attention decoding (kernels/nrtr_joint.h): ccd_nrtr_beam_step_joint per launch at
           widths 4, 8, 16 with Tc = 32 frames of Cc = 92 classes and weight 0.3, next to ccd_nrtr_beam_step in the same process on the
           same logits, both on a state eight steps into their own decode (with how many slots are still live); ccd_nrtr_joint_begin
           per launch; then evaluation images/s at B = 512, vit_small with an auxiliary CTC head: forward_beam with joint_ctc_weight
           0.3 against the plain forward_beam at widths 4, 8 and 16, rounds alternating.
  twopass  (not part of a default run) two-pass decoding (kernels/nrtr_twopass.h): at B = 512, vit_small with an auxiliary CTC head and
           widths 4, 8, 16, on the proposals ops.ctc_beam_search makes of the model's own frames: ccd_nrtr_twopass_rows and
           ccd_nrtr_twopass_select per launch (through their wrappers, allocations included), ops.ctc_score_paths, the teacher-forced
           pass (finetune_engine.score_words without moments over the B * W rows) and forward_twopass end to end; in the same process
           and rounds forward_beam plain and with joint_ctc_weight at the same widths.
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

B, T, C, D, L = 512, 25, 92, 512, 6
WIDTHS = (1, 4, 8, 16)
LIMITS = {"kernels": 240, "eval": 420, "rescore": 180, "trie": 600, "score": 420, "joint": 420, "twopass": 420}      # seconds per case
TRIE_WIDTHS, TRIE_LEXICONS = (4, 8, 16), (1000, 10000, 90000)


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
    out = {"shape": {"B": B, "T": T, "C": C, "D": D, "L": L}}
    for W in WIDTHS:
        g = torch.Generator().manual_seed(W)
        logits = torch.randn(B * W, 128, generator=g) * 2.0
        logits.scatter_add_(1, torch.randint(0, C, (B * W, 1), generator=g), torch.full((B * W, 1), 6.0))
        logits = logits.to(dev)
        seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, dev)
        for s in range(8):                                                    # eight steps in: every slot is in use
            ops.nrtr_beam_step(logits.roll(s, 0), C, s, C - 1, C, seq, score, state, parent)
        saved = [t.clone() for t in (seq, score, state)]

        def step():
            for t, keep in zip((seq, score, state), saved):
                t.copy_(keep)
            ops.nrtr_beam_step(logits, C, 8, C - 1, C, seq, score, state, parent)

        def restore():
            for t, keep in zip((seq, score, state), saved):
                t.copy_(keep)

        cache = torch.zeros((L, B * W * (T + 1), 3 * D), dtype=torch.bfloat16, device=dev)
        perm = torch.stack([torch.randperm(W, generator=g) for _ in range(B)]).int().to(dev)
        moved = float((perm != torch.arange(W, device=dev)).sum())
        entry = {}
        with_copy, copies = [], []
        reorder = {12: [], 24: []}
        for _ in range(a.rounds):
            with_copy.append(event_ms(step, a.iters))
            copies.append(event_ms(restore, a.iters))
            for s in reorder:
                reorder[s].append(event_ms(lambda: ops.nrtr_beam_reorder(cache, perm, T + 1, s), a.iters))
        entry["step_with_state_restore"] = summary(with_copy)
        entry["state_restore_alone"] = summary(copies)
        entry["step_kernel_ms"] = round(entry["step_with_state_restore"]["median_ms"] - entry["state_restore_alone"]["median_ms"], 4)
        for s, rounds in reorder.items():
            r = summary(rounds)
            nbytes = 2.0 * L * moved * (s + 1) * 2 * D * 2                     # read + write of the K | V columns that move
            r["gigabytes_moved"] = round(nbytes * 1e-9, 3)
            r["gigabytes_per_s"] = round(nbytes * 1e-9 / (r["median_ms"] * 1e-3), 1) if moved else 0.0
            entry[f"reorder_positions_0_to_{s}"] = r
        entry["rows_that_move"] = f"{int(moved)} of {B * W}"
        out[f"w{W}"] = entry
        del cache
    return out


def case_eval(a):
    import torch
    from ccd_amd import finetune as ft
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(), dev, dropout=0.0).eval()
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    sides = {0: [], 1: [], 4: [], 8: []}
    iters = max(3, a.iters // 6)
    with torch.no_grad():
        for _ in range(a.rounds):
            for width in sides:
                fn = (lambda: model.forward_test(img)) if width == 0 else (lambda: model.forward_beam(img, width))
                sides[width].append(event_ms(fn, iters))
    out = {"batch": B, "arch": "vit_small", "decode_graph": os.environ.get("CCD_DECODE_GRAPH", "1") != "0"}
    for width, rounds in sides.items():
        name = "greedy" if width == 0 else f"beam_width_{width}"
        out[name] = summary(rounds)
        out[name + "_images_per_s"] = round(B / (out[name]["median_ms"] * 1e-3))
    return out


def case_rescore(a):
    import numpy as np
    import torch
    from ccd_amd import finetune as ft, finetune_engine as fe
    dev = torch.device("cuda")
    out = {}
    for bias in a.end_bias:
        torch.manual_seed(2)
        model = ft.build_model(ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2), dev).eval()
        with torch.no_grad():
            model.arena.w("decoder.classifier.bias")[91] += bias
        model.arena.refresh_mirrors()
        worst, compared, lengths = 0.0, 0, []
        for n in (5, 16):
            img = torch.randn(n, 3, 32, 128, generator=torch.Generator().manual_seed(5 + n))      # tests/test_nrtr_beam_gpu.py: images()
            g = torch.Generator().manual_seed(50 + n)
            img = (img * 0.25 + 2.0 * torch.randn(n, 3, 1, 1, generator=g) + torch.randn(n, 3, 1, 128, generator=g)).to(dev)
            with torch.no_grad():
                feat = model.extract_feat(img)
                out_enc = model.encoder(feat).to(torch.bfloat16)
                model.decoder._ready()
                inc = fe.greedy_decode(model.decoder, out_enc).double().cpu().numpy()
                full = fe.greedy_decode_full(model.decoder, out_enc).double().cpu().numpy()
            for b in range(n):
                tok_i, tok_f = inc[b].argmax(-1), full[b].argmax(-1)
                ends = np.nonzero(tok_i == 91)[0]
                steps = int(ends[0]) + 1 if len(ends) else inc.shape[1]
                lengths.append(steps - 1 if len(ends) else steps)
                if (tok_i[:steps] == tok_f[:steps]).all():
                    t = np.arange(steps)
                    worst = max(worst, abs(float(np.log(inc[b, t, tok_i[:steps]]).sum() - np.log(full[b, t, tok_i[:steps]]).sum())))
                    compared += 1
        out[f"end_bias_{bias:g}"] = {"rescore_base": worst, "greedy_paths_compared": compared, "greedy_word_lengths": lengths}
    return out


def synthetic_lexicon(n, seed=0):
    """n distinct words of 2..15 of the classes 0..90, sorted -> a list of tuples."""
    import numpy as np
    rng = np.random.default_rng(seed)
    words = set()
    while len(words) < n:
        words.add(tuple(int(c) for c in rng.integers(0, 91, int(rng.integers(2, 16)))))
    return sorted(words)


def case_trie(a):
    import numpy as np
    import torch
    from ccd_amd import finetune as ft, ops
    dev = torch.device("cuda")
    out = {"shape": {"B": B, "T": T, "C": C, "D": D, "L": L}, "lexicons": {}}
    tries = {}
    for n in TRIE_LEXICONS:
        words = synthetic_lexicon(n, seed=n)
        rows = np.zeros((n, 15), dtype=np.int64)
        for row, w in zip(rows, words):
            row[:len(w)] = np.asarray(w) + 1                                      # AttnConvertor.set_lexicon's layout: class + 1
        tries[n] = ops.ctc_lexicon_trie(ops.ctc_lexicon(torch.from_numpy(rows)))
        out["lexicons"][str(n)] = dict(tries[n].stats)
    for W in TRIE_WIDTHS:
        g = torch.Generator().manual_seed(W)
        logits = torch.randn(B * W, 128, generator=g) * 2.0
        logits.scatter_add_(1, torch.randint(0, C, (B * W, 1), generator=g), torch.full((B * W, 1), 6.0))
        logits = logits.to(dev)
        sides = {}
        for name in ["plain"] + [str(n) for n in TRIE_LEXICONS]:
            trie = None if name == "plain" else tries[int(name)]
            seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, dev)
            node = ops.nrtr_beam_trie_state(B, W, dev)

            def launch(s, rows, seq=seq, score=score, state=state, parent=parent, node=node, trie=trie):
                if trie is None:
                    ops.nrtr_beam_step(rows, C, s, C - 1, C, seq, score, state, parent)
                else:
                    ops.nrtr_beam_step_trie(rows, C, s, C - 1, C, seq, score, state, parent, node, trie)

            for s in range(8):                                                    # eight steps into its own decode
                launch(s, logits.roll(s, 0))
            live = int((state == ops.NRTR_LIVE).sum())
            used = int((state != ops.NRTR_UNUSED).sum())
            tensors = (seq, score, state, node)
            saved = [t.clone() for t in tensors]

            def restore(tensors=tensors, saved=saved):
                for t, keep in zip(tensors, saved):
                    t.copy_(keep)

            def step(restore=restore, launch=launch):
                restore()
                launch(8, logits)

            sides[name] = {"step": step, "restore": restore, "with_copy": [], "copies": [], "live": live, "used": used}
        for _ in range(a.rounds):                                                 # rounds alternate between the sides
            for side in sides.values():
                side["with_copy"].append(event_ms(side["step"], a.iters))
                side["copies"].append(event_ms(side["restore"], a.iters))
        entry = {}
        for name, side in sides.items():
            e = {"step_with_state_restore": summary(side["with_copy"]), "state_restore_alone": summary(side["copies"])}
            e["step_kernel_ms"] = round(e["step_with_state_restore"]["median_ms"] - e["state_restore_alone"]["median_ms"], 4)
            e["slots_live_at_the_timed_step"] = f"{side['live']} of {B * W} ({side['used']} in use)"
            entry["ccd_nrtr_beam_step" if name == "plain" else f"ccd_nrtr_beam_step_trie_{name}_words"] = e
        out[f"w{W}"] = entry
    # evaluation images/s: the lexicon beam against the plain beam of the same width
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(), dev, dropout=0.0).eval()
    conv = model.label_convertor
    words = synthetic_lexicon(10000, seed=10000)
    conv.set_lexicon(["".join(conv.idx2char[c] if c < 90 else "\u00e9" for c in w) for w in words], beam=8)
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    sides = {("beam_width", 8): [], ("lexicon_beam", 8): [], ("beam_width", 16): [], ("lexicon_beam", 16): []}
    iters = max(3, a.iters // 6)
    with torch.no_grad():
        for _ in range(a.rounds):
            for kind, width in sides:
                fn = (lambda: model.forward_beam(img, width)) if kind == "beam_width" else (lambda: model.forward_lexicon(img, width))
                sides[(kind, width)].append(event_ms(fn, iters))
    ev = {"batch": B, "arch": "vit_small", "lexicon": dict(conv.lexicon_stats), "decode_graph": os.environ.get("CCD_DECODE_GRAPH", "1") != "0"}
    for (kind, width), rounds in sides.items():
        name = f"{kind}_{width}"
        ev[name] = summary(rounds)
        ev[name + "_images_per_s"] = round(B / (ev[name]["median_ms"] * 1e-3))
    out["eval"] = ev
    return out


def case_score(a):
    import numpy as np
    import torch
    from ccd_amd import finetune as ft, ops
    dev = torch.device("cuda")
    H, Tq, words_per_image = 8, T + 1, 50
    scale = 64 ** -0.5
    out = {"shape": {"H": H, "Tq": Tq, "words_per_image": words_per_image, "D": D}}

    def operands(n_img, seed):
        g = torch.Generator().manual_seed(seed)
        R = n_img * words_per_image
        q = torch.randn(R * Tq, D, generator=g).to(torch.bfloat16).to(dev)
        kv = torch.randn(n_img * 256, 2 * D, generator=g).to(torch.bfloat16).to(dev)
        rows = ops.csr_rows(np.arange(n_img + 1) * words_per_image)
        return q, kv, rows, R

    # ---- B = 64: against the replicated attention
    q, kv, rows, R = operands(64, 1)
    rep = kv.view(64, 256, 2 * D).repeat_interleave(words_per_image, 0).reshape(-1, 2 * D)
    new = lambda: ops.xattn_rows_fwd(q, kv[:, :D], kv[:, D:], rows, H, Tq, scale)
    old = lambda: ops.dec_attn_fwd(q, rep[:, :D], rep[:, D:], R, H, Tq, 256, scale)
    assert torch.equal(new()[0].view(torch.int16), old()[0].view(torch.int16)), "xattn_rows_fwd differs from the replicated attention"
    sides = {"xattn_rows_fwd": (new, []), "dec_attn_fwd_replicated": (old, [])}
    for _ in range(a.rounds):
        for fn, rounds in sides.values():
            rounds.append(event_ms(fn, a.iters))
    qo = 2.0 * R * Tq * D * 2                                                  # q read + out written
    nbytes = {"xattn_rows_fwd": qo + 64 * 256 * 2 * D * 2 * -(-words_per_image // ops.xattn_rows_chunk(R, H)),
              "dec_attn_fwd_replicated": qo + R * 256 * 2 * D * 2}
    entry = {"rows": R, "chunk": ops.xattn_rows_chunk(R, H), "replication_buffers_megabytes": round(rep.numel() * 2e-6, 1)}
    for name, (_, rounds) in sides.items():
        e = summary(rounds)
        e["megabytes_moved"] = round(nbytes[name] * 1e-6, 1)
        e["gigabytes_per_s"] = round(nbytes[name] * 1e-9 / (e["median_ms"] * 1e-3), 1)
        entry[name] = e
    entry["speedup"] = round(entry["dec_attn_fwd_replicated"]["median_ms"] / entry["xattn_rows_fwd"]["median_ms"], 2)
    out["b64_x_50"] = entry
    del rep, q, kv
    # ---- B = 512: the new kernel alone (the replicated K / V would be 2 x 6.7 GB)
    q, kv, rows, R = operands(512, 2)
    entry = {"rows": R, "chunk": ops.xattn_rows_chunk(R, H)}
    sides = {"xattn_rows_fwd": [], "xattn_rows_fwd_with_moments": []}
    for _ in range(a.rounds):
        for name, rounds in sides.items():
            rounds.append(event_ms(lambda: ops.xattn_rows_fwd(q, kv[:, :D], kv[:, D:], rows, H, Tq, scale, want_moments=name.endswith("moments")),
                                   a.iters))
    moved = 2.0 * R * Tq * D * 2 + 512 * 256 * 2 * D * 2 * -(-words_per_image // entry["chunk"])
    for name, rounds in sides.items():
        e = summary(rounds)
        e["megabytes_moved"] = round((moved + (R * H * Tq * 16 if name.endswith("moments") else 0)) * 1e-6, 1)
        e["gigabytes_per_s"] = round(e["megabytes_moved"] * 1e-3 / (e["median_ms"] * 1e-3), 1)
        entry[name] = e
    out["b512_x_50"] = entry
    del q, kv
    # ---- the word scores
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(R * Tq, 128, generator=g) * 2.0).to(dev)
    seq = torch.full((R, Tq), C, dtype=torch.int64)
    seq[:, 0] = C - 1
    lengths = torch.randint(2, 16, (R,), generator=g)
    for r in range(R):
        n = int(lengths[r])
        seq[r, 1:1 + n] = torch.randint(0, C - 1, (n,), generator=g)
        seq[r, 1 + n] = C - 1
    seq = seq.to(dev)
    moments = torch.rand(R, H, Tq, 4, generator=g).to(dev)
    rounds = [event_ms(lambda: ops.nrtr_word_score(logits, C, seq, C - 1, C, moments=moments, H=H), a.iters) for _ in range(a.rounds)]
    e = summary(rounds)
    e["rows"], e["mean_word_length"] = R, round(float(lengths.float().mean()), 2)
    e["nanoseconds_per_row"] = round(e["median_ms"] * 1e6 / R, 1)
    out["nrtr_word_score"] = e
    del logits, moments
    # ---- evaluation images/s: 50 words per image, the same 50 for every image so that forward_lexicon answers the same question
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(), dev, dropout=0.0).eval()
    conv = model.label_convertor
    lexicon = ["".join(conv.idx2char[c] if c < 90 else "\u00e9" for c in w) for w in synthetic_lexicon(words_per_image, seed=50)]
    conv.set_lexicon(lexicon, beam=16)
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    lists = [lexicon] * B
    sides = {"forward_words_50_per_image": (lambda: model.forward_words(img, lists), []),
             "forward_lexicon_beam_16": (lambda: model.forward_lexicon(img, 16), [])}
    iters = max(3, a.iters // 6)
    with torch.no_grad():
        a_idx = sides["forward_words_50_per_image"][0]()[0][:, 0]
        b_idx = sides["forward_lexicon_beam_16"][0]()[0][:, 0]
        agree = int((a_idx == b_idx).sum())
        for _ in range(a.rounds):
            for fn, rounds in sides.values():
                rounds.append(event_ms(fn, iters))
    ev = {"batch": B, "arch": "vit_small", "lexicon": dict(conv.lexicon_stats), "best_word_agrees": f"{agree} of {B}",
          "decode_graph": os.environ.get("CCD_DECODE_GRAPH", "1") != "0"}
    for name, (_, rounds) in sides.items():
        ev[name] = summary(rounds)
        ev[name + "_images_per_s"] = round(B / (ev[name]["median_ms"] * 1e-3))
    out["eval"] = ev
    return out


JOINT_WIDTHS, JOINT_TC, JOINT_WEIGHT = (4, 8, 16), 32, 0.3


def case_joint(a):
    import torch
    from ccd_amd import finetune as ft, ops
    dev = torch.device("cuda")
    out = {"shape": {"B": B, "T": T, "C": C, "Tc": JOINT_TC, "Cc": C, "weight": JOINT_WEIGHT}}
    g = torch.Generator().manual_seed(5)
    frames = torch.randn(B, JOINT_TC, 128, generator=g) * 2.0                     # rows of a 128-wide buffer, as the CTC head's logits
    frames[:, :, 0] += 5.0
    frames = frames.to(dev)[:, :, :C]
    for W in JOINT_WIDTHS:
        g = torch.Generator().manual_seed(W)
        logits = torch.randn(B * W, 128, generator=g) * 2.0
        logits.scatter_add_(1, torch.randint(0, C, (B * W, 1), generator=g), torch.full((B * W, 1), 6.0))
        logits = logits.to(dev)
        sides = {}
        for name in ("plain", "joint"):
            seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, dev)
            joint = ops.nrtr_joint_state(frames, W) if name == "joint" else None

            def launch(s, rows, seq=seq, score=score, state=state, parent=parent, joint=joint):
                if joint is None:
                    ops.nrtr_beam_step(rows, C, s, C - 1, C, seq, score, state, parent)
                else:
                    ops.nrtr_beam_step_joint(rows, C, s, C - 1, C, seq, score, state, parent, joint, JOINT_WEIGHT)

            for s in range(8):                                                    # eight steps into its own decode
                launch(s, logits.roll(s, 0))
            live = int((state == ops.NRTR_LIVE).sum())
            used = int((state != ops.NRTR_UNUSED).sum())
            tensors = (seq, score, state) + ((joint.prefix, joint.att) if joint is not None else ())
            saved = [t.clone() for t in tensors]

            def restore(tensors=tensors, saved=saved):
                for t, keep in zip(tensors, saved):
                    t.copy_(keep)

            def step(restore=restore, launch=launch):
                restore()
                launch(8, logits)

            sides[name] = {"step": step, "restore": restore, "with_copy": [], "copies": [], "live": live, "used": used}
        begin = []
        for _ in range(a.rounds):                                                 # rounds alternate between the sides
            for side in sides.values():
                side["with_copy"].append(event_ms(side["step"], a.iters))
                side["copies"].append(event_ms(side["restore"], a.iters))
            begin.append(event_ms(lambda: ops.nrtr_joint_state(frames, W), a.iters))
        entry = {}
        for name, side in sides.items():
            e = {"step_with_state_restore": summary(side["with_copy"]), "state_restore_alone": summary(side["copies"])}
            e["step_kernel_ms"] = round(e["step_with_state_restore"]["median_ms"] - e["state_restore_alone"]["median_ms"], 4)
            e["slots_live_at_the_timed_step"] = f"{side['live']} of {B * W} ({side['used']} in use)"
            entry["ccd_nrtr_beam_step" if name == "plain" else "ccd_nrtr_beam_step_joint"] = e
        entry["nrtr_joint_state (ccd_nrtr_joint_begin and three allocations)"] = summary(begin)
        out[f"w{W}"] = entry
    # evaluation images/s: the joint beam against the plain beam of the same width, on a model with the auxiliary head
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_aux_ctc_weight = 0.3
    model = ft.build_model(cfg, dev, dropout=0.0).eval()
    with torch.no_grad():
        model.arena.w("ctc_decoder.fc.bias")[0] += 5.0                            # (an untrained head is uniform: nothing would finish)
    model.arena.refresh_mirrors()
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    sides = {(kind, width): [] for width in JOINT_WIDTHS for kind in ("beam_width", "joint_beam_width")}
    iters = max(3, a.iters // 6)
    with torch.no_grad():
        for _ in range(a.rounds):
            for kind, width in sides:
                fn = (lambda: model.forward_beam(img, width)) if kind == "beam_width" else \
                     (lambda: model.forward_beam(img, width, joint_ctc_weight=JOINT_WEIGHT))
                sides[(kind, width)].append(event_ms(fn, iters))
    ev = {"batch": B, "arch": "vit_small", "joint_ctc_weight": JOINT_WEIGHT, "decode_graph": os.environ.get("CCD_DECODE_GRAPH", "1") != "0"}
    for (kind, width), rounds in sides.items():
        name = f"{kind}_{width}"
        ev[name] = summary(rounds)
        ev[name + "_images_per_s"] = round(B / (ev[name]["median_ms"] * 1e-3))
    out["eval"] = ev
    return out


TWOPASS_WIDTHS, TWOPASS_WEIGHT = (4, 8, 16), 0.5


def case_twopass(a):
    import torch
    from ccd_amd import finetune as ft, finetune_engine as fe, ops
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig()
    cfg.decoder_aux_ctc_weight = 0.3
    model = ft.build_model(cfg, dev, dropout=0.0).eval()
    with torch.no_grad():
        model.arena.w("ctc_decoder.fc.bias")[0] += 5.0                            # (an untrained head is uniform: nothing would finish)
    model.arena.refresh_mirrors()
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    dec, spec = model.decoder, model.decoder.dec_spec
    out = {"batch": B, "arch": "vit_small", "decoder_layers": spec.L, "ctc_weight": TWOPASS_WEIGHT,
           "decode_graph": os.environ.get("CCD_DECODE_GRAPH", "1") != "0"}
    iters = max(3, a.iters // 6)
    with torch.no_grad():
        feat = model.extract_feat(img)
        probs = model.ctc_decoder.forward_test(feat)
        out_enc = model.encoder(feat).to(torch.bfloat16)
        dec._ready()
        for W in TWOPASS_WIDTHS:
            paths, lengths, _ = ops.ctc_beam_search(probs, W, normalized=True)
            rows = lambda: ops.nrtr_twopass_rows(paths, lengths, spec.C, spec.start_idx, spec.start_idx, spec.padding_idx, T + 1)      # noqa: E731
            seq, targets, subset = rows()
            row_ptr = ops.csr_rows(list(range(0, (B + 1) * W, W)))
            att = fe.score_words(dec, out_enc, seq, row_ptr, want_moments=False)["score"]
            ctc = ops.ctc_score_paths(probs, paths, lengths, normalized=True, rows=(targets, subset))
            stages = {"ccd_nrtr_twopass_rows": rows,
                      "ccd_nrtr_twopass_select": lambda: ops.nrtr_twopass_select(att, ctc, paths, lengths, subset, TWOPASS_WEIGHT, T),
                      "ctc_score_paths (given the rows)": lambda: ops.ctc_score_paths(probs, paths, lengths, normalized=True, rows=(targets, subset)),
                      "ctc_score_paths (with its own rows launch)": lambda: ops.ctc_score_paths(probs, paths, lengths, normalized=True),
                      "ctc_beam_search (the proposals)": lambda: ops.ctc_beam_search(probs, W, normalized=True),
                      "teacher_forced_pass (score_words, no moments)": lambda: fe.score_words(dec, out_enc, seq, row_ptr, want_moments=False)}
            ends = {"forward_twopass": lambda: model.forward_twopass(img, beam=W, ctc_weight=TWOPASS_WEIGHT),
                    "forward_beam": lambda: model.forward_beam(img, W),
                    "forward_beam_joint": lambda: model.forward_beam(img, W, joint_ctc_weight=JOINT_WEIGHT)}
            times = {name: [] for name in list(stages) + list(ends)}
            for _ in range(a.rounds):                                             # rounds alternate between all sides
                for name, fn in stages.items():
                    times[name].append(event_ms(fn, a.iters))
                for name, fn in ends.items():
                    times[name].append(event_ms(fn, iters))
            entry = {"rows": B * W, "eligible_rows": int((subset >= 0).sum())}
            for name, rounds in times.items():
                entry[name] = summary(rounds)
                if name in ends:
                    entry[name + "_images_per_s"] = round(B / (entry[name]["median_ms"] * 1e-3))
            out[f"w{W}"] = entry
    return out


CASES = {"joint": case_joint, "twopass": case_twopass, "kernels": case_kernels, "eval": case_eval, "rescore": case_rescore, "trie": case_trie, "score": case_score}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    ap.add_argument("--cases", default="kernels,eval,rescore", help="comma-separated cases of a whole run, in order")
    ap.add_argument("--end_bias", type=float, nargs="+", default=[0.5], help="rescore: the <EOS> bias of tests/test_nrtr_beam_gpu.py (END_BIAS)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), "nrtr_beam_bench needs an MI355X"
        print(json.dumps({a.case: CASES[a.case](a)}))
        return
    out = {"iters": a.iters, "rounds": a.rounds, "unit": "ms per call, HIP events (median of round medians; lowest and highest round)"}
    names = [n for n in a.cases.split(",") if n]
    assert names and all(n in CASES for n in names), f"--cases takes names out of {sorted(CASES)}"
    for name in names:
        # a fresh process per case under its own time limit; a case that fails or runs out of time ends the run
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--iters", str(a.iters), "--rounds", str(a.rounds),
                              "--end_bias"] + [str(b) for b in a.end_bias], capture_output=True, text=True, timeout=LIMITS[name])
        if run.returncode != 0:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            sys.exit(f"nrtr_beam_bench: case {name} ended with status {run.returncode}; nothing further was started")
        out.update(json.loads(run.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
