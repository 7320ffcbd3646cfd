"""Word / character accuracy of a recogniser over a labelled dataset.

Same surface and the same arithmetic as `Dino.metric.eval_acc.TextAccuracy` (reference :10-64; driven by test.py:184-218):
`TextAccuracy(charset_path, case_sensitive, model_eval).compute(model, dataloader)` ->
    {'ccr', 'cwr', 'ted', 'ned', 'ted/w', 'words', 'time'}
* a word counts as correct (cwr) when ground truth and prediction agree after lower-casing and dropping every character
  outside [A-Za-z0-9 + CJK] (:39-46);
* ted / ned: edit distance of those normalised strings, ned divided by the RAW ground-truth length (:48-50);
* ccr: position-wise equal characters of the RAW strings over the raw ground-truth length (:53-56).
The scoring is `update(gt_text, pt_text)`, separated from the model loop so that it can be checked against the reference's
numbers without a model.  (`editdistance` is not in this image: the Levenshtein distance is computed here.)

On a GPU `compute` scores on the device instead: `update_scores(scores, gt_text)` hands the decoder's output and the ground truth
as code points (`encode_truth`) to ops.text_score / ops.text_accumulate - arg-max decoding, normalisation, edit distance and the
sums in two launches per batch, no host synchronisation - and `result()` reads the six totals back in one copy.  The values are
those of `update` on the decoded strings: the counts exactly, `ned` up to the order of its fp64 sum.  The device path needs
`AttnConvertor.score_table()` (None when max_seq_len steps of the longest class do not fit the kernel: host path) and takes the
first maximum of the scores themselves where `tensor2idx` takes the maximum of their softmax; the two differ only where two
classes of a step are closer than the softmax resolves.  With a CTCConvertor the same path decodes by the greedy CTC rule
(ops.text_score_ctc: repeats collapsed, blanks dropped); everything behind the decode step is shared.  A CTCConvertor configured
with a beam (`beam_width` > 0, with or without a language model) or a lexicon (with or without `lexicon_beam`) decodes the head's
probabilities itself - `CTCConvertor.best_paths`, the one place that picks the decoder - and the best word's -1-padded paths are
scored by ops.text_score_paths, still without a host synchronisation (host path: `CTCConvertor.tensor2best`).  An AttnConvertor with `beam_width` > 0
makes `compute` decode by beam search over the NRTR decoder (`DINO_Finetune.forward_beam`) and score the best word the same way
(`update_paths`; on the host path: `idx2str` of `paths2nbest`); `forward_test` itself stays greedy.
An AttnConvertor with a lexicon (and its `lexicon_beam`) makes `compute` decode over that closed vocabulary instead: rank 0 of
`DINO_Finetune.forward_lexicon`'s paths through `update_paths` - no host synchronisation (host path: `paths2lexicon`).
An AttnConvertor with `twopass_beam` > 0 makes `compute` score rank 0 of `DINO_Finetune.forward_twopass` - CTC proposals rescored by
the decoder - through `update_paths`, again without a host synchronisation (host path: `paths2nbest` on the same outputs).
"""
from __future__ import annotations

import re
import time

import numpy as np
import torch

from .. import ops
from ..convertor.ctc import is_ctc

_KEEP = re.compile("[^A-Z^a-z^0-9^一-龥]")      # the reference's pattern, verbatim semantics: '^' itself is kept too


def normalise(s: str) -> str:
    """What a word is compared as: lower case, everything outside [a-z0-9^ + CJK] dropped (`update`)."""
    return _KEEP.sub("", s.lower())


def encode_truth(strings):
    """['ab', 'c', ...] -> (code points int32 [B, L] zero-padded to the longest string (L >= 1), lengths int32 [B]): one encode of
    the joined batch, no per-character Python."""
    strings = list(strings)
    lens = np.fromiter((len(s) for s in strings), dtype=np.int32, count=len(strings))
    flat = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int32)
    codes = np.zeros((len(strings), max(1, int(lens.max(initial=0)))), dtype=np.int32)
    codes[np.arange(codes.shape[1], dtype=np.int32)[None, :] < lens[:, None]] = flat
    return codes, lens


def levenshtein(a: str, b: str) -> int:
    """Unit-cost edit distance (what `editdistance.eval` returns)."""
    if a == b:
        return 0
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, start=1):
        cur = [i]
        for j, cb in enumerate(b, start=1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


class TextAccuracy:
    def __init__(self, charset_path=None, case_sensitive=False, model_eval="vision"):
        assert model_eval in ("vision", "language", "alignment")
        self.charset_path, self.case_sensitive, self.model_eval = charset_path, case_sensitive, model_eval
        self._names = ["ccr", "cwr", "ted", "ned", "ted/w", "words", "time"]
        self.total_num_char = self.total_num_word = self.correct_num_char = self.correct_num_word = 0.0
        self.total_ed = self.total_ned = self.inference_time = 0.0
        self._totals = None          # device path: int64 [6] on the device (ops.TEXT_TOTALS), read by result()
        self._tables = None          # (convertor, device, raw table, normalised table) of the last update_scores
        self._path_tables = None     # the same for update_paths (AttnConvertor.path_score_table)
        self._spans = []             # device path of compute(): (start, end) events around each batch

    def update(self, gt_text, pt_text):
        """Score one batch of (ground truth, prediction) strings."""
        self._refuse_case_sensitive()
        for gt, pt in zip(gt_text, pt_text):
            gt_n, pt_n = _KEEP.sub("", gt.lower()), _KEEP.sub("", pt.lower())
            if gt_n == pt_n:
                self.correct_num_word += 1
            distance = levenshtein(gt_n, pt_n)
            self.total_ed += distance
            self.total_ned += float(distance) / max(len(gt), 1)
            self.total_num_word += 1
            self.correct_num_char += sum(1 for j in range(min(len(gt), len(pt))) if gt[j] == pt[j])
            self.total_num_char += len(gt)

    def _refuse_case_sensitive(self):
        # the reference only defines its normalised strings under `not case_sensitive` (:40-44) and fails otherwise
        if self.case_sensitive:
            raise NotImplementedError("TextAccuracy is defined for case_sensitive=False (eval_acc.py:40-46)")

    def _device_tables(self, who, slot, convertor, make, dev):
        """The convertor's (raw, normalised) tables `make()` on `dev`, uploaded once per (convertor, device) and kept in the
        attribute `slot` as (convertor, device, raw, normalised), which is returned.  convertor None: the one of the last call."""
        cached = getattr(self, slot)
        if convertor is not None and (cached is None or cached[0] is not convertor or cached[1] != dev):
            tables = make(convertor)
            if tables is None:
                raise ValueError(f"{who}: max_seq_len steps of the convertor's longest class exceed ops.TEXT_COLS characters; "
                                 "score on the host with update()")
            cached = (convertor, dev) + tuple(ops.upload(torch.from_numpy(t), dev) for t in tables)
            setattr(self, slot, cached)
        if cached is None:
            raise ValueError(f"{who}: pass the model's label convertor")
        return cached

    @staticmethod
    def _upload_truth(who, gt_text, samples, dev):
        """The ground-truth strings of a batch of `samples` -> (code points int32 [B, L], lengths int32 [B]) on `dev`."""
        codes, lens = encode_truth(gt_text)
        if len(lens) != samples:
            raise ValueError(f"{who}: {samples} samples but {len(lens)} ground-truth strings")
        both = ops.upload(torch.from_numpy(np.concatenate([codes.ravel(), lens])), dev)        # one host-to-device copy for both
        return both[:codes.size].view(codes.shape), both[codes.size:]

    def _accumulate(self, records):
        if self._totals is None:
            self._totals = ops.text_totals(records.device)
        ops.text_accumulate(records, self._totals)
        return records

    def update_scores(self, scores, gt_text, convertor=None):
        """Score one batch on the device: decoder scores fp32 [B, T, C] (a strided view is read in place) against the ground-truth
        strings.  Nothing is read back; the totals stay on the device until result().  convertor: the model's AttnConvertor
        (default: the one of the last call)."""
        self._refuse_case_sensitive()
        conv, _, raw, norm = self._device_tables("update_scores", "_tables", convertor, lambda c: c.score_table(), scores.device)
        gt, gt_len = self._upload_truth("update_scores", gt_text, scores.shape[0], scores.device)
        if is_ctc(conv):                                                      # frames, not decoding steps
            paths = conv.best_paths(scores)                                   # None: the greedy rule, applied by the scoring kernel
            records = ops.text_score_ctc(scores, raw, norm, gt, gt_len) if paths is None else ops.text_score_paths(paths, raw, norm, gt, gt_len)
        else:
            records = ops.text_score(scores, raw, norm, conv.end_idx, conv.padding_idx, gt, gt_len)
        return self._accumulate(records)

    def update_paths(self, paths, gt_text, convertor):
        """Score one batch of decoded words on the device: paths int32 [B, T] (any row stride: rank 0 of forward_beam's paths), the
        classes of an AttnConvertor, -1-padded.  Records and totals as update_scores; nothing is read back."""
        self._refuse_case_sensitive()
        _, _, raw, norm = self._device_tables("update_paths", "_path_tables", convertor, lambda c: c.path_score_table(), paths.device)
        gt, gt_len = self._upload_truth("update_paths", gt_text, paths.shape[0], paths.device)
        # class c in row c + 1; the -1 padding counts nothing
        return self._accumulate(ops.text_score_paths(paths + 1, raw, norm, gt, gt_len))

    def result(self):
        cc, tc, cw, words, ed, ned = self.correct_num_char, self.total_num_char, self.correct_num_word, self.total_num_word, \
            self.total_ed, self.total_ned
        if self._totals is not None:
            host = self._totals.cpu()                                         # the one device-to-host copy
            cc, tc, cw, words, ed = (a + float(b) for a, b in zip((cc, tc, cw, words, ed), host[:5].tolist()))
            ned += host[5:].view(torch.float64).item()
            self.inference_time += sum(e0.elapsed_time(e1) for e0, e1 in self._spans) * 1e-3
            self._spans = []
        mets = [cc / tc, cw / words, ed, ned, ed / words, words, self.inference_time]
        return dict(zip(self._names, mets))

    @torch.no_grad()
    def compute(self, model, dataloader, on_batch=None):
        """on_batch(out_dec, gt_strings): called behind the scoring of every batch of a head whose decoder output is scored directly
        (test.py --alignments); what it does is outside the timed span and changes nothing that is scored."""
        net = model.module if hasattr(model, "module") else model
        device = next(net.parameters()).device
        convertor = net.label_convertor
        attn_beam = not is_ctc(convertor) and getattr(convertor, "beam_width", 0) > 0     # beam search over the NRTR decoder, rank 0 scored
        attn_lexicon = not is_ctc(convertor) and getattr(convertor, "lexicon", None) is not None     # ... along the lexicon's prefix tree
        attn_twopass = not is_ctc(convertor) and getattr(convertor, "twopass_beam", 0) > 0     # CTC proposals rescored by the decoder, rank 0
        if device.type == "cuda" and not self.case_sensitive and convertor.score_table() is not None:
            for image_tensors, label_tensors in dataloader:
                image_tensors = image_tensors.to(device)
                span = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                span[0].record()
                if attn_twopass:
                    self.update_paths(net.forward_twopass(image_tensors)[0][:, 0], list(label_tensors[0]), convertor)
                elif attn_lexicon:
                    self.update_paths(net.forward_lexicon(image_tensors)[2][:, 0], list(label_tensors[0]), convertor)
                elif attn_beam:
                    self.update_paths(net.forward_beam(image_tensors, convertor.beam_width)[0][:, 0], list(label_tensors[0]), convertor)
                else:
                    out_dec = model(image_tensors, text=None, return_loss=False, test_speed=False)
                    self.update_scores(out_dec.float(), list(label_tensors[0]), convertor)
                span[1].record()
                self._spans.append(span)                                      # read in result(), behind its copy
                if on_batch is not None and not attn_beam and not attn_lexicon and not attn_twopass:
                    on_batch(out_dec.float(), list(label_tensors[0]))
            return self.result()
        for image_tensors, label_tensors in dataloader:
            image_tensors = image_tensors.to(device)
            start = time.time()
            if attn_twopass:
                nbest = convertor.paths2nbest(*net.forward_twopass(image_tensors))[0]
            elif attn_lexicon:
                nbest = convertor.paths2lexicon(*net.forward_lexicon(image_tensors)[:2], nbest=1)[0]
            elif attn_beam:
                nbest = convertor.paths2nbest(*net.forward_beam(image_tensors, convertor.beam_width))[0]
            else:
                nbest = None
                out_dec = model(image_tensors, text=None, return_loss=False, test_speed=False)
            # the best word of the configured decoder: a CTC beam or lexicon runs its kernels, on any device
            label_indexes = convertor.tensor2best(out_dec) if nbest is None else [words[0] if words else [] for words in nbest]
            pt_text = convertor.idx2str(label_indexes)
            self.inference_time += time.time() - start
            self.update(list(label_tensors[0]), pt_text)
            if on_batch is not None and not attn_beam and not attn_lexicon and not attn_twopass:
                on_batch(out_dec.float(), list(label_tensors[0]))
        return self.result()
