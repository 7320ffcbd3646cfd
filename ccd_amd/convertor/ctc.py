"""Label codec of the CTC recognition head: words <-> class indices <-> zero-padded target tensors.

Class layout: `<BLK>` (the CTC blank) is class 0, the alphabet occupies 1..n, `<UKN>` (when enabled) is last: DICT90 gives 92
classes.  A target row is the word's classes followed by zeros, cut to `max_seq_len` - a valid label is never 0, so the length of a
row is its count of leading non-zero entries (what ccd_ctc_loss_fwd reads on the device).  Decoding is the greedy CTC rule: the
arg-max class of every frame (first maximum), repeats collapsed, blanks dropped.  The reference has no CTC head; the codec shares
base.BaseConvertor with AttnConvertor and follows its surface, so that DINO_Finetune, TextAccuracy, train_finetune.py and test.py take
either.  Which decoder the configuration below selects is decided in one place: `_beam`, `_lexicon_pick`, `best_paths`.

`beam_width` > 0 asks for CTC prefix beam search (ops.ctc_beam_search) where words are scored (TextAccuracy) and in `tensor2nbest`,
which returns an n-best list with the log-probability of each word summed over its alignments; 0, the default, is the greedy rule
everywhere, and `tensor2idx` is the greedy rule whatever the width.

A `lexicon` (a list of words, or the path of a UTF-8 file with one word per line) asks for lexicon-constrained decoding instead: where
words are scored (TextAccuracy) and in `tensor2lexicon` the answer is the most probable word OF THE LEXICON, with the exact log of its
probability summed over all alignments (ops.ctc_lexicon_score / ops.ctc_lexicon_best).  The words are encoded as targets are (`lower`,
`<UKN>`); words of more than 31 classes and duplicates after encoding are dropped and counted in `lexicon_stats`.  A lexicon and a
beam exclude each other.

`lexicon_beam` = W in 1..16 makes the lexicon path a two-stage search instead of scoring every word: a beam of width W walks the
lexicon's prefix tree (ops.ctc_lexicon_trie, built with the lexicon), and the handful of words it proposes are scored exactly
(ops.ctc_lexicon_search).  The cost is a beam's whatever the size of the lexicon; the log-probabilities are the same exact numbers,
and the answer is the exhaustive path's whenever its best word is among the proposals.  0, the default, scores every word.

An `lm` (a char_lm.CharNGram, the path of an .npz it saved, or the path of a UTF-8 word list, which is estimated at `lm_order`) fuses a
character n-gram language model into the beam search (ops.ctc_beam_search_lm): where words are scored (TextAccuracy) and in
`tensor2nbest` every extension by a character adds lm_weight * log P(character | context) + lm_bonus, and with `lm_eos` the end of the
word adds lm_weight * log P(end | context) behind the last frame.  An LM needs beam_width >= 1 and excludes a lexicon.

`tensor2align` / `tensor2chars` say WHERE the characters of a word sit and how sure the network is of each: the best single alignment
(ops.ctc_align) of given transcriptions, or of the word(s) the convertor's own configuration decodes - greedy, beam, LM-fused beam or
lexicon alike, so the per-character confidences of the four decoders are comparable numbers.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .base import BaseConvertor, checked_beam_width, nbest_lists


def is_ctc(convertor):
    """True for the codec of the CTC head (targets are zero-padded classes, decoding is the greedy CTC rule)."""
    return isinstance(convertor, CTCConvertor)


class CTCConvertor(BaseConvertor):
    """CTCConvertor(dict_type='DICT90', with_unknown=True, max_seq_len=25, lower=False, beam_width=0, lexicon=None, lexicon_beam=0,
    lm=None, lm_order=2, lm_weight=1.0, lm_bonus=0.0, lm_eos=True) - see the module docstring."""

    def __init__(self, dict_type="DICT90", dict_file=None, dict_list=None, with_unknown=True, max_seq_len=25, lower=False, beam_width=0,
                 lexicon=None, lexicon_beam=0, lm=None, lm_order=2, lm_weight=1.0, lm_bonus=0.0, lm_eos=True, **_ignored):
        alphabet = self._alphabet(dict_type, dict_file, dict_list)
        self.with_unknown, self.max_seq_len, self.lower = bool(with_unknown), int(max_seq_len), bool(lower)
        from ..ops import CTC_MAX_BEAM
        self.beam_width = checked_beam_width(beam_width, CTC_MAX_BEAM)
        self.blank_idx = 0
        self.idx2char = ["<BLK>"] + alphabet
        self.unknown_idx = None
        if self.with_unknown:
            self.idx2char.append("<UKN>")
            self.unknown_idx = len(self.idx2char) - 1
        self._index_alphabet(alphabet, 1)                                    # the alphabet starts behind the blank
        self.lexicon, self.lexicon_words, self.lexicon_stats, self.lexicon_trie = None, None, None, None
        self.lexicon_beam = self._checked_lexicon_beam(lexicon_beam)
        if lexicon is not None:
            self.set_lexicon(lexicon)
        elif self.lexicon_beam > 0:
            raise ValueError(f"lexicon_beam = {self.lexicon_beam} needs a lexicon: it is the width of the search over the lexicon's trie")
        self.lm, self.lm_model, self.lm_stats = None, None, None
        self.lm_order, self.lm_weight, self.lm_bonus, self.lm_eos = int(lm_order), float(lm_weight), float(lm_bonus), bool(lm_eos)
        if lm is not None:
            self.set_lm(lm)

    def set_lm(self, lm, order=None, weight=None, bonus=None, eos=None):
        """The language model of tensor2nbest and TextAccuracy: a char_lm.CharNGram, the path of an .npz that CharNGram.save wrote, or
        the path of a UTF-8 word list (one word per line), estimated at `order` (default: lm_order); None removes it.  weight / bonus /
        eos replace lm_weight / lm_bonus / lm_eos where given.  Kept: `lm` (the ops.ctc_char_lm handle), `lm_model` (the CharNGram) and
        `lm_stats` = {'order', 'classes', 'rows', 'bytes'}."""
        from .. import ops
        from .char_lm import CharNGram
        if lm is None:
            self.lm, self.lm_model, self.lm_stats = None, None, None
            return None
        if self.lexicon is not None:
            raise ValueError("a language model and a lexicon exclude each other: lexicon decoding scores the words of a closed list "
                             "exactly, remove the lexicon (set_lexicon(None)) or the language model")
        if self.beam_width < 1:
            raise ValueError("a language model needs beam_width >= 1: it is fused into the beam search, and the convertor's beam_width "
                             "is 0 (greedy decoding)")
        if order is not None:
            self.lm_order = int(order)
        if isinstance(lm, CharNGram):
            model = lm
        elif isinstance(lm, (str, bytes)) or hasattr(lm, "__fspath__"):
            name = lm.decode() if isinstance(lm, bytes) else str(lm)
            model = CharNGram.load(name) if name.endswith(".npz") else CharNGram.from_words(self, name, order=self.lm_order)
        else:
            raise TypeError(f"set_lm expects a CharNGram, the path of an .npz or the path of a word list, got {type(lm).__name__}")
        model.check_alphabet(self)
        handle = ops.ctc_char_lm(model.table, model.order)
        for name, value, kind in (("lm_weight", weight, float), ("lm_bonus", bonus, float), ("lm_eos", eos, bool)):
            if value is not None:
                setattr(self, name, kind(value))
        if not (np.isfinite(self.lm_weight) and np.isfinite(self.lm_bonus)):
            raise ValueError(f"lm_weight and lm_bonus must be finite, got {self.lm_weight} and {self.lm_bonus}")
        self.lm, self.lm_model, self.lm_order, self.lm_stats = handle, model, model.order, model.stats
        return self.lm_stats

    @staticmethod
    def _checked_lexicon_beam(beam):
        from ..ops import CTC_MAX_BEAM
        if isinstance(beam, bool) or int(beam) != beam or not 0 <= int(beam) <= CTC_MAX_BEAM:
            raise ValueError(f"lexicon_beam must lie in 0..{CTC_MAX_BEAM} (0: every word of the lexicon is scored), got {beam!r}")
        return int(beam)

    def set_lexicon(self, strings_or_path, beam=None):
        """The closed vocabulary of tensor2lexicon and TextAccuracy: a list of words, or the path of a UTF-8 file with one word per line
        (empty lines skipped); None removes it.  Kept: `lexicon` (the ops.ctc_lexicon handle), `lexicon_words` (the kept strings, in
        order: column v of the scores is lexicon_words[v]) and `lexicon_stats` = {'read', 'kept', 'too_long', 'duplicates'}.  beam
        replaces lexicon_beam where given; with lexicon_beam > 0 the prefix tree is built here (`lexicon_trie`, the
        ops.ctc_lexicon_trie handle) and lexicon_stats gains 'nodes'."""
        from .. import ops
        if beam is not None:
            beam = self._checked_lexicon_beam(beam)
        if strings_or_path is None:
            if beam:
                raise ValueError(f"lexicon_beam = {beam} needs a lexicon: it is the width of the search over the lexicon's trie")
            self.lexicon, self.lexicon_words, self.lexicon_stats, self.lexicon_trie = None, None, None, None
            self.lexicon_beam = 0
            return None
        if getattr(self, "lm", None) is not None:
            raise ValueError("a lexicon and a language model exclude each other: remove the language model (set_lm(None)) first")
        if self.beam_width > 0:
            raise ValueError(f"a lexicon and beam_width = {self.beam_width} exclude each other: lexicon decoding scores every word of "
                             "the lexicon exactly, set beam_width to 0")
        words, self.lexicon_words, self.lexicon_stats = self._lexicon_rows(strings_or_path, ops.CTC_MAX_LABELS, 0)
        self.lexicon = ops.ctc_lexicon(torch.from_numpy(words))
        if beam is not None:
            self.lexicon_beam = beam
        self.lexicon_trie = None
        if self.lexicon_beam > 0:
            self.lexicon_trie = ops.ctc_lexicon_trie(self.lexicon)
            self.lexicon_stats["nodes"] = self.lexicon_trie.n_nodes
        return self.lexicon_stats

    # ------------------------------------------------------------------ encode
    def str2tensor(self, strings):
        """['hello', ...] -> int64 [N, max_seq_len]: the word's classes, zero-padded (longer words cut)."""
        if not isinstance(strings, list) or not all(isinstance(w, str) for w in strings):
            raise TypeError("str2tensor expects a list of strings")
        target = np.zeros((len(strings), self.max_seq_len), dtype=np.int64)
        for row, word in zip(target, strings):
            cls = self._classes_of(word)[:self.max_seq_len]
            row[:cls.size] = cls
        return torch.from_numpy(target)

    # ------------------------------------------------------------------ decode
    def score_table(self, steps=32):
        """The classes as code points for ops.text_score_ctc: the (raw, normalised) tables of BaseConvertor._code_point_tables, the
        blank's row empty.  None when `steps` frames of the longest normalised row would not fit the kernel's columns.  The tables
        are built once."""
        if not hasattr(self, "_tables"):
            self._tables = self._code_point_tables({self.blank_idx})
        from ..ops import TEXT_COLS
        return self._tables if steps * self._tables[1].shape[1] <= TEXT_COLS else None

    @torch.no_grad()
    def tensor2idx(self, outputs, img_metas=None):
        """[N, T, C] frame scores (logits or probabilities) -> (class indices, confidences) per sample by the greedy rule; the
        confidence of a character is the softmax probability (of `outputs` as given) of the first frame of its run."""
        probs = outputs.float().softmax(dim=-1)
        conf, cls = probs.max(dim=-1)                                        # [N, T]; the first maximum
        cls_np, conf_np = cls.cpu().numpy(), conf.cpu().numpy()
        new_run = np.ones_like(cls_np, dtype=bool)
        new_run[:, 1:] = cls_np[:, 1:] != cls_np[:, :-1]
        keep = new_run & (cls_np != self.blank_idx)
        indexes = [cls_np[i][keep[i]].tolist() for i in range(cls_np.shape[0])]
        scores = [conf_np[i][keep[i]].tolist() for i in range(cls_np.shape[0])]
        return indexes, scores

    @torch.no_grad()
    def tensor2nbest(self, outputs, beam_width=None, nbest=1, normalized=True):
        """[N, T, C] frame scores on the device - probabilities (normalized=True: what CTCDecoder.forward_test returns) or logits
        -> (indexes, log_probs) by CTC prefix beam search of width `beam_width` (default: the convertor's own, which must then be
        > 0): indexes[i] holds up to `nbest` index lists, best first; log_probs is a float tensor [N, nbest], the log of each word's
        probability summed over the alignments the beam kept, -inf where a slot is empty.  With a language model set (set_lm) the search
        is the fused one and log_probs are the fused scores: log p_ctc(word) + lm_weight * sum log P_lm + lm_bonus * len(word), with
        lm_eos the end-of-word term included - comparable with the plain beam's only after that sum is subtracted."""
        width = self.beam_width if beam_width is None else int(beam_width)
        if width < 1:
            raise ValueError("tensor2nbest: needs a beam_width >= 1 (the convertor's is 0: greedy decoding)")
        return nbest_lists("tensor2nbest", *self._beam(outputs.float(), width, normalized), nbest)

    @torch.no_grad()
    def tensor2lexicon(self, outputs, nbest=1, normalized=True, subset=None, beam=None):
        """[N, T, C] frame scores on the device - probabilities (normalized=True: what CTCDecoder.forward_test returns) or logits
        -> (indexes, log_probs, word_ids): the `nbest` most probable words of the lexicon, best first.  indexes[i] holds up to `nbest`
        index lists (fewer where fewer words have an alignment of finite probability); log_probs is a float tensor [N, nbest], the
        exact log of each word's probability summed over all alignments, -inf where a slot is empty; word_ids is an int64 tensor
        [N, nbest] of positions in `lexicon_words`, -1 where a slot is empty.  subset int32 [N, K] on the device restricts sample i
        to the words subset[i] (negative entries are padding).  beam (default: lexicon_beam) > 0 searches the lexicon's trie with a
        beam of that width and scores only the words it proposes (ops.ctc_lexicon_search; nbest <= beam) - the same exact
        log-probabilities at a cost that does not grow with the lexicon; it excludes a subset."""
        from .. import ops
        if self.lexicon is None:
            raise ValueError("tensor2lexicon: the convertor has no lexicon (set_lexicon)")
        width = self.lexicon_beam if beam is None else self._checked_lexicon_beam(beam)
        if width > 0:
            if subset is not None:
                raise ValueError("tensor2lexicon: a subset and a beam exclude each other - a per-image subset is small already, it is "
                                 "scored exhaustively (pass beam=0)")
            if not 1 <= int(nbest) <= width:
                raise ValueError(f"tensor2lexicon: nbest must lie in 1..beam = {width}, got {nbest}")
        elif not 1 <= int(nbest) <= ops.CTC_LEXICON_MAX_NBEST:
            raise ValueError(f"tensor2lexicon: nbest must lie in 1..{ops.CTC_LEXICON_MAX_NBEST}, got {nbest}")
        ids, best = self._lexicon_pick(outputs.float(), nbest, normalized, beam=width, subset=subset)
        ids = ids.long()
        if subset is not None and subset.shape[1]:                           # positions in the subset -> positions in the lexicon
            ids = torch.where(ids >= 0, subset.long().gather(1, ids.clamp(min=0)), ids)
        ids = ids.cpu()
        words, lengths = self.lexicon.words, self.lexicon.lengths
        indexes = [[words[v, :lengths[v]].tolist() for v in row if v >= 0] for row in ids.tolist()]
        return indexes, best.cpu(), ids

    def _trie(self):
        """The lexicon's prefix tree, built on first use where the convertor was configured without a lexicon_beam."""
        from .. import ops
        if self.lexicon_trie is None:
            self.lexicon_trie = ops.ctc_lexicon_trie(self.lexicon)
        return self.lexicon_trie

    # ------------------------------------------------------------------ the configured decoder: each choice is made here, once
    def _beam(self, scores, width, normalized):
        """(paths, lengths, hyp_scores) of the prefix beam search of `width`, fused with the language model where one is set."""
        from .. import ops
        if self.lm is not None:
            return ops.ctc_beam_search_lm(scores, width, self.lm, self.lm_weight, self.lm_bonus, self.lm_eos, normalized=normalized)
        return ops.ctc_beam_search(scores, width, normalized=normalized)

    def _lexicon_pick(self, scores, nbest, normalized, beam=None, subset=None):
        """(index int32 [N, nbest], log_probs fp32 [N, nbest]) of the lexicon's best words, -1 and -inf in an empty slot: by the search
        over the trie with beam (default: lexicon_beam) > 0, by scoring every word - of subset[i] where given - otherwise."""
        from .. import ops
        width = self.lexicon_beam if beam is None else beam
        if width > 0:
            return ops.ctc_lexicon_search(scores, self._trie(), width, nbest=nbest, normalized=normalized)
        return ops.ctc_lexicon_best(ops.ctc_lexicon_score(scores, self.lexicon, normalized=normalized, subset=subset), nbest)

    def _lexicon_paths(self, scores):
        """The best lexicon word of every sample as -1-padded int32 paths [B, max_len] (all -1 where no word has an alignment of finite
        probability): the pick and plain indexing, nothing is read back."""
        index, _ = self._lexicon_pick(scores, 1, True)
        words = self.lexicon.on(scores.device)[0]
        if not words.shape[0]:
            return torch.full((scores.shape[0], 1), -1, dtype=torch.int32, device=scores.device)
        best = index[:, 0].long()
        rows = words[best.clamp(min=0)]
        ended = (rows == 0).cumsum(dim=1) > 0                                 # behind the word's first zero
        return torch.where(ended | (best < 0)[:, None], -1, rows).to(torch.int32)

    def best_paths(self, scores):
        """What TextAccuracy scores on the device: the rank-0 word of the configured decoder for [N, T, C] probabilities, as -1-padded
        int32 paths [N, width] (any row stride) - of the lexicon, else of the beam (LM-fused where an LM is set); None at beam_width 0
        without a lexicon: the greedy rule, which ops.text_score_ctc applies to the frames itself.  No host synchronisation."""
        if self.lexicon is not None:
            return self._lexicon_paths(scores)
        if self.beam_width > 0:
            return self._beam(scores, self.beam_width, True)[0][:, 0]
        return None

    @torch.no_grad()
    def tensor2best(self, outputs):
        """The host-side counterpart of best_paths: the best word of every sample as a list of class indices ([] where the decoder
        returns no word), by the lexicon, else the beam, else the greedy rule."""
        if self.lexicon is not None:
            nbest = self.tensor2lexicon(outputs, nbest=1)[0]
        elif self.beam_width > 0:
            nbest = self.tensor2nbest(outputs, nbest=1)[0]
        else:
            return self.tensor2idx(outputs)[0]
        return [words[0] if words else [] for words in nbest]

    # ------------------------------------------------------------------ alignment
    @torch.no_grad()
    def tensor2align(self, outputs, words=None, nbest=1, normalized=True):
        """[N, T, C] frame scores on the device - probabilities (normalized=True: what CTCDecoder.forward_test returns) or logits -> the
        best single alignment (ops.ctc_align) of `nbest` words per sample, a dict of device tensors with N * nbest rows, row
        i * nbest + r = rank r of sample i: 'targets' int64 [rows, Lmax] zero-padded, 'frame_char' int32 [rows, T], 'spans' int32
        [rows, Lmax, 2], 'char_logp' fp32 [rows, Lmax], 'score' fp32 [rows], 'rows' int32 [rows] (the sample of every row; -1 where a
        slot holds no word - fewer hypotheses than nbest, a word of more than 31 classes - and the row is padding with score -inf).
        words: a list of N strings, encoded as targets are - the forced alignment of those transcriptions (nbest must be 1).
        words=None: the word(s) the convertor's configuration decodes - the greedy word at beam_width 0, the beam's `nbest` best
        otherwise (LM-fused if an LM is set), the lexicon's `nbest` best if a lexicon is set (those of the trie search with lexicon_beam
        > 0) - aligned against one copy of the scores;
        nothing in this case synchronises with the host."""
        from .. import ops
        scores = outputs.float()
        N, T = scores.shape[0], scores.shape[1]
        k = int(nbest)
        sample = torch.arange(N, dtype=torch.int32, device=scores.device)
        if words is not None:
            if k != 1 or not isinstance(words, list) or len(words) != N:
                raise ValueError(f"tensor2align: words must be a list of one string per sample ({N}) and nbest 1, got "
                                 f"{len(words) if isinstance(words, list) else type(words).__name__} and nbest {nbest}")
            targets = self.str2tensor(words)[:, :ops.CTC_MAX_LABELS].contiguous().to(scores.device)
            rows = sample
        elif self.lexicon is not None:
            if not 1 <= k <= ops.CTC_LEXICON_MAX_NBEST:
                raise ValueError(f"tensor2align: nbest must lie in 1..{ops.CTC_LEXICON_MAX_NBEST}, got {nbest}")
            if 0 < self.lexicon_beam < k:                                    # the trie search proposes lexicon_beam words
                raise ValueError(f"tensor2align: nbest must lie in 1..lexicon_beam = {self.lexicon_beam}, got {nbest}")
            index, _ = self._lexicon_pick(scores, k, normalized)
            table = self.lexicon.on(scores.device)[0]
            if table.shape[0]:
                targets = table[index.long().clamp(min=0).flatten()]
            else:
                targets = torch.zeros((N * k, 1), dtype=torch.int64, device=scores.device)
            rows = torch.where(index >= 0, sample[:, None], -1).flatten()
        elif self.beam_width > 0:
            if not 1 <= k <= self.beam_width:
                raise ValueError(f"tensor2align: nbest must lie in 1..beam_width = {self.beam_width}, got {nbest}")
            paths, lengths, _ = self._beam(scores, self.beam_width, normalized)
            lengths = lengths[:, :k]
            targets = ops.ctc_paths_to_targets(paths[:, :k]).flatten(0, 1)
            rows = torch.where((lengths >= 0) & (lengths <= ops.CTC_MAX_LABELS), sample[:, None], -1).flatten()
        else:
            if k != 1:
                raise ValueError(f"tensor2align: greedy decoding (beam_width 0, no lexicon) has one word per sample, got nbest {nbest}")
            path, length, _ = ops.ctc_greedy(scores)
            targets = ops.ctc_paths_to_targets(path)
            rows = torch.where(length <= ops.CTC_MAX_LABELS, sample, -1)
        rows = rows.to(torch.int32).contiguous()
        frame_char, spans, char_logp, score = ops.ctc_align(scores, targets.contiguous(), normalized=normalized, rows=rows)
        return {"targets": targets, "frame_char": frame_char, "spans": spans, "char_logp": char_logp, "score": score, "rows": rows}

    @torch.no_grad()
    def tensor2chars(self, outputs, words=None, nbest=1, normalized=True, image_width=128, boxes="emission"):
        """The host-side view of tensor2align (same arguments): per sample a list of up to `nbest` entries (word, log_prob, chars), best
        first, where log_prob is the log-probability of the word's best alignment and chars holds one (char, x0, x1, first_frame,
        last_frame, conf) per character: x0 = first * image_width / T, x1 = (last + 1) * image_width / T, and conf = exp(char_logp /
        n_frames), the geometric mean of the frame probabilities of the character.  A slot without a word or without an alignment
        gives no entry.
        boxes='emission' (the default): the span is where the network EMITS the character.  CTC is peaky - a character is often
        emitted on a single frame, somewhere inside its glyph - so this is NOT the character's inked extent.
        boxes='cells': every span is widened to the midpoints of the blank gaps to its neighbours, and to the image edges at the ends
        of the word; the cells tile the width (a segmentation of the line into characters, still no ink boxes)."""
        if boxes not in ("emission", "cells"):
            raise ValueError(f"tensor2chars: boxes must be 'emission' or 'cells', got {boxes!r}")
        res = self.tensor2align(outputs, words=words, nbest=nbest, normalized=normalized)
        N, T = outputs.shape[0], outputs.shape[1]
        packed = torch.cat([res["targets"].float(), res["spans"].flatten(1).float(), res["char_logp"], res["score"][:, None],
                            res["rows"][:, None].float()], dim=1).cpu().numpy()              # ONE device-to-host copy
        return self.chars_of(packed, N, T, res["targets"].shape[1], image_width=image_width, boxes=boxes)

    def chars_of(self, packed, N, T, Lmax, image_width=128, boxes="emission"):
        """The host half of tensor2chars: `packed` is the numpy array [rows, 4 * Lmax + 2] of (targets, spans, char_logp, score, rows)."""
        k = packed.shape[0] // max(N, 1)
        out = [[] for _ in range(N)]
        scale, table = float(image_width) / float(T), self.idx2char
        for n, rec in enumerate(packed.tolist()):                              # plain lists: no numpy call per row
            score, row = rec[4 * Lmax], int(rec[4 * Lmax + 1])
            if row < 0 or score == float("-inf"):
                continue
            cls = [int(c) for c in rec[:Lmax]]
            L = cls.index(0) if 0 in cls else Lmax
            first = [int(rec[Lmax + 2 * j]) for j in range(L)]
            last = [int(rec[Lmax + 2 * j + 1]) for j in range(L)]
            lo, hi = [float(f) for f in first], [float(e + 1) for e in last]
            if boxes == "cells" and L:
                cuts = [(hi[j] + lo[j + 1]) / 2.0 for j in range(L - 1)]
                lo, hi = [0.0] + cuts, cuts + [float(T)]
            chars = [(table[cls[j]], lo[j] * scale, hi[j] * scale, first[j], last[j],
                      math.exp(rec[3 * Lmax + j] / (last[j] - first[j] + 1))) for j in range(L)]
            out[n // k].append(("".join(c[0] for c in chars), score, chars))
        return out
