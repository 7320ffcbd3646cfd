"""Label codec of the recognition head: words <-> class indices <-> padded target tensors.

Behavioural contract (what `DINO_Finetune`, `train_finetune.py` and checkpoints rely on; reference:
Dino/convertor/base.py:3-110, Dino/convertor/attn.py:81-154): the DICT90 alphabet occupies classes 0..89, then
`<UKN>` (90, when enabled), `<BOS/EOS>` (91; one shared class unless start_end_same=False) and `<PAD>` (92);
a target row is `<BOS> chars <EOS> <PAD>...` cut to `max_seq_len`; decoding takes the arg-max class per position,
drops `<PAD>` and stops at the first `<EOS>`.

The alphabet, words <-> class indices and the reading of a lexicon's word list are base.BaseConvertor's; decoding is one arg-max +
one first-EOS scan on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from .base import ALPHABETS, BaseConvertor, _read_alphabet_file, checked_beam_width, nbest_lists  # noqa: F401 (the dataset and the tools import the alphabets from here)


class AttnConvertor(BaseConvertor):
    """AttnConvertor(dict_type='DICT90', max_seq_len=40, with_unknown=True, beam_width=0) - see the module docstring.  `beam_width` > 0
    asks for beam search over the decoder (DINO_Finetune.forward_beam) where words are scored (TextAccuracy.compute); 0, the default,
    is greedy decoding everywhere, and `tensor2idx` is the greedy rule whatever the width.  `lexicon` (a list of words or the path of
    a word list) TOGETHER WITH `lexicon_beam` in 1..16 asks for the closed vocabulary instead: a beam of that width over the decoder
    that walks the lexicon's prefix tree (DINO_Finetune.forward_lexicon); a finished hypothesis is a word of the lexicon and its score
    the exact log p(word <EOS> | image).  Either of the two alone is refused: exhaustive scoring of ONE lexicon for the whole batch
    exists for the CTC head only.  Words GIVEN per image - a 50-word lexicon for every image, an n-best to rescore, a transcription -
    need no configuration: words2rows / scores2words / scores2chars below, with DINO_Finetune.forward_score / forward_words.
    `twopass_beam` in 1..16 (with `twopass_ctc_weight` in [0, 1], default 0.5 - WeNet's, untuned here) asks for two-pass decoding where
    words are scored: the auxiliary CTC head's beam proposes, the decoder rescores (DINO_Finetune.forward_twopass); it excludes
    beam_width > 0 and a lexicon.  The two values are kept as attributes."""

    def __init__(self, dict_type="DICT90", dict_file=None, dict_list=None, with_unknown=True, max_seq_len=40, lower=False,
                 start_end_same=True, beam_width=0, lexicon=None, lm=None, lexicon_beam=0, twopass_beam=0, twopass_ctc_weight=None, **_ignored):
        if lm is not None:
            raise NotImplementedError("AttnConvertor: language-model fusion is for the CTC head only - the NRTR decoder conditions every "
                                      "character on the ones before it already, and its beam takes no additive table term (use "
                                      "decoder.type: 'CTCDecoder')")
        if (lexicon is not None) != bool(lexicon_beam):
            raise NotImplementedError("AttnConvertor: scoring every word of a lexicon is for the CTC head only - the probability of a word "
                                      "under the NRTR decoder takes one teacher-forced decoder pass per word, not a closed-form "
                                      "recursion over the frames (use decoder.type: 'CTCDecoder').  The NRTR head takes `lexicon` "
                                      "together with `lexicon_beam: N` (1..16): a beam of width N over the lexicon's prefix tree")
        alphabet = self._alphabet(dict_type, dict_file, dict_list)
        self.with_unknown, self.max_seq_len = bool(with_unknown), int(max_seq_len)
        self.lower, self.start_end_same = bool(lower), bool(start_end_same)
        from ..ops import NRTR_MAX_BEAM
        self.beam_width = checked_beam_width(beam_width, NRTR_MAX_BEAM)
        self.twopass_beam, self.twopass_ctc_weight = self._checked_twopass(twopass_beam, twopass_ctc_weight, NRTR_MAX_BEAM)
        if self.twopass_beam and (self.beam_width > 0 or lexicon is not None):
            raise ValueError(f"twopass_beam = {self.twopass_beam} excludes beam_width > 0 and lexicon / lexicon_beam: two-pass decoding "
                             "takes its proposals from the CTC prefix beam and ranks them itself")
        # special classes behind the alphabet, in the reference's order
        self.idx2char = list(alphabet)
        self.unknown_idx = self._append("<UKN>") if self.with_unknown else None
        self.start_idx = self._append("<BOS/EOS>")
        self.end_idx = self.start_idx if self.start_end_same else self._append("<BOS/EOS>")
        self.padding_idx = self._append("<PAD>")
        self._index_alphabet(alphabet, 0)
        self.lexicon, self.lexicon_words, self.lexicon_stats, self.lexicon_trie, self.lexicon_beam = None, None, None, None, 0
        if lexicon is not None:
            self.set_lexicon(lexicon, beam=lexicon_beam)

    TWOPASS_DEFAULT_WEIGHT = 0.5       # WeNet's default for attention rescoring; untuned here (no trained hybrid model exists)

    @staticmethod
    def _checked_twopass(beam, weight, limit):
        """(twopass_beam, 0: off; twopass_ctc_weight, None without a beam, absent: TWOPASS_DEFAULT_WEIGHT)."""
        beam = 0 if beam is None else beam
        if isinstance(beam, bool) or not isinstance(beam, (int, np.integer)) or not 0 <= int(beam) <= limit:
            raise ValueError(f"twopass_beam must lie in 1..{limit} (the width of the CTC beam that proposes; 0 or absent: off), got {beam!r}")
        if weight is not None and (isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) <= 1.0):
            raise ValueError(f"twopass_ctc_weight must lie in [0, 1], got {weight!r}")
        if not beam:
            if weight is not None:
                raise ValueError(f"twopass_ctc_weight = {weight!r} needs twopass_beam in 1..{limit}: it weighs the scores of its proposals")
            return 0, None
        return int(beam), AttnConvertor.TWOPASS_DEFAULT_WEIGHT if weight is None else float(weight)

    @staticmethod
    def _checked_lexicon_beam(beam):
        from ..ops import NRTR_MAX_BEAM
        if isinstance(beam, bool) or int(beam) != beam or not 1 <= int(beam) <= NRTR_MAX_BEAM:
            raise ValueError(f"lexicon_beam must lie in 1..{NRTR_MAX_BEAM} (the width of the beam over the lexicon's prefix tree), got {beam!r}")
        return int(beam)

    def set_lexicon(self, strings_or_path, beam=None):
        """The closed vocabulary of DINO_Finetune.forward_lexicon and TextAccuracy: a list of words, or the path of a UTF-8 file with
        one word per line (empty lines skipped); None removes it.  beam replaces lexicon_beam where given (a first lexicon needs one).
        Kept: `lexicon_words` (the kept strings: word id v is lexicon_words[v]), `lexicon` (the ops.ctc_lexicon handle whose rows are
        class + 1, zero-padded: class 0 is the character '0', and a row ends at its first zero), `lexicon_trie` (the
        ops.ctc_lexicon_trie handle of those rows) and `lexicon_stats` = {'read', 'kept', 'too_long', 'duplicates', 'nodes'}.  too_long
        counts the words of more than max_seq_len - 1 characters, which could never write their <EOS> (and of more than
        ops.CTC_MAX_LABELS, the widest row a lexicon handle takes): with finite logits and a lexicon that is not empty every slot that
        is still alive at the last step is then finished."""
        from .. import ops
        if strings_or_path is None:
            if beam:
                raise ValueError(f"lexicon_beam = {beam} needs a lexicon: it is the width of the search over the lexicon's trie")
            self.lexicon, self.lexicon_words, self.lexicon_stats, self.lexicon_trie, self.lexicon_beam = None, None, None, None, 0
            return None
        width = self._checked_lexicon_beam(self.lexicon_beam if beam is None else beam)
        if self.beam_width > 0:
            raise ValueError(f"a lexicon and beam_width = {self.beam_width} exclude each other: the lexicon's beam is lexicon_beam, set "
                             "beam_width to 0")
        if self.twopass_beam:
            raise ValueError(f"a lexicon and twopass_beam = {self.twopass_beam} exclude each other: two-pass decoding ranks the CTC beam's "
                             "proposals (a lexicon's proposals go through DINO_Finetune.forward_twopass(proposals=))")
        words, kept, stats = self._lexicon_rows(strings_or_path, min(self.max_seq_len - 1, ops.CTC_MAX_LABELS), 1)
        self.lexicon = ops.ctc_lexicon(torch.from_numpy(words))
        self.lexicon_words, self.lexicon_beam = kept, width
        self.lexicon_trie = ops.ctc_lexicon_trie(self.lexicon)
        self.lexicon_stats = dict(stats, nodes=self.lexicon_trie.n_nodes)
        return self.lexicon_stats

    def _append(self, token):
        self.idx2char.append(token)
        return len(self.idx2char) - 1

    def str2tensor(self, strings):
        """['hello', ...] -> int64 [N, max_seq_len]: <BOS> chars <EOS> <PAD>... (cut to max_seq_len)."""
        if not isinstance(strings, list) or not all(isinstance(w, str) for w in strings):
            raise TypeError("str2tensor expects a list of strings")
        T = self.max_seq_len
        target = np.full((len(strings), T), self.padding_idx, dtype=np.int64)
        for row, word in zip(target, strings):
            cls = self._classes_of(word)[:max(T - 1, 0)]
            row[0] = self.start_idx
            row[1:1 + cls.size] = cls
            if 1 + cls.size < T:
                row[1 + cls.size] = self.end_idx
        return torch.from_numpy(target)

    # ------------------------------------------------------------------ decode
    def score_table(self):
        """The classes as code points, for scoring on the device (ops.text_score): the (raw, normalised) tables of
        BaseConvertor._code_point_tables, the rows of the end and padding classes empty.  None when max_seq_len steps of the longest
        normalised row would not fit the kernel's columns (the caller scores on the host).  Built once."""
        if not hasattr(self, "_score_table"):
            from ..ops import TEXT_COLS
            tables = self._code_point_tables({self.end_idx, self.padding_idx})
            self._score_table = tables if self.max_seq_len * tables[1].shape[1] <= TEXT_COLS else None
        return self._score_table

    def path_score_table(self):
        """score_table() for classes that are already decoded (ops.text_score_paths, which never takes class 0 for an index - it is
        the CTC blank there): the same two tables behind one empty row, so that class c sits in row c + 1.  The caller hands the
        kernel `paths + 1`: the -1 padding becomes row 0 and counts nothing.  None where score_table() is None."""
        if not hasattr(self, "_path_score_table"):
            tables = self.score_table()
            self._path_score_table = None if tables is None else tuple(
                np.concatenate([np.full((1, t.shape[1]), -1, dtype=np.int32), t]) for t in tables)
        return self._path_score_table

    def tensor2align(self, *args, **kwargs):
        raise NotImplementedError("AttnConvertor: forced alignment (tensor2align / tensor2chars) is for the CTC head only - the NRTR "
                                  "decoder has no frame axis to align a word against (use decoder.type: 'CTCDecoder')")

    tensor2chars = tensor2align

    # ------------------------------------------------------------------ scoring given words (DINO_Finetune.forward_score / forward_words)
    def words2rows(self, words):
        """A list of N word lists - the words asked of image i; a word is a string or a list of class indices (what idx2str takes) ->
        (seq int64 [R, max_seq_len + 1], row_ptr int32 [N + 1], rows): one row `<BOS> chars <EOS> <PAD>..` per word in the layout of
        the decoder's sequences, the CSR table of which image owns which rows (image i: rows row_ptr[i] .. row_ptr[i + 1] - 1; a list
        may be empty), and the R words as strings.  Host tensors.  A word of more than max_seq_len - 1 characters cannot write its
        <EOS>: it STAYS, as a row of its first max_seq_len characters without one - an infeasible row, score -inf - so that index k
        of a result is word k of the list, whatever the words are."""
        if not isinstance(words, (list, tuple)) or not all(isinstance(w, (list, tuple)) for w in words):
            raise TypeError("words2rows expects a list of word lists, one per image")
        flat = [w for per_image in words for w in per_image]
        if not all(isinstance(w, str) or (isinstance(w, (list, tuple)) and all(isinstance(c, (int, np.integer)) for c in w)) for w in flat):
            raise TypeError("words2rows: a word is a string or a list of class indices")
        T = self.max_seq_len + 1
        seq = np.full((len(flat), T), self.padding_idx, dtype=np.int64)
        seq[:, 0] = self.start_idx
        rows = []
        for row, word in zip(seq, flat):
            cls = self._classes_of(word) if isinstance(word, str) else np.asarray(word, dtype=np.int64).reshape(-1)
            rows.append(word if isinstance(word, str) else self.idx2str([cls.tolist()])[0])
            n = min(cls.size, T - 1)
            row[1:1 + n] = cls[:n]
            if cls.size < T - 1:
                row[1 + cls.size] = self.end_idx
        row_ptr = np.zeros(len(words) + 1, dtype=np.int32)
        np.cumsum([len(per_image) for per_image in words], out=row_ptr[1:])
        return torch.from_numpy(seq), torch.from_numpy(row_ptr), rows

    @torch.no_grad()
    def scores2words(self, score, row_ptr, nbest=1):
        """score fp32 [R] (forward_score's, on any device), row_ptr as words2rows returns it (host integers, or an ops.csr_rows handle)
        -> (index int32 [N, nbest] into every image's OWN list, log_probs fp32 [N, nbest]), best first, on score's device: the scores
        are scattered to [N, longest list] padded with -inf and ops.ctc_lexicon_best picks per row - by (score descending, index
        ascending), -inf (an infeasible word, padding) never selected, a slot left over is (-1, -inf).  No host synchronisation."""
        from .. import ops
        rows = ops.csr_rows(row_ptr)
        if score.dim() != 1 or score.shape[0] != rows.R or score.dtype != torch.float32:
            raise ValueError(f"scores2words: expects score float32 [{rows.R}] (row_ptr ends there), got {score.dtype} {list(score.shape)}")
        N, K = rows.B, rows.max_rows
        table = torch.full((N, max(K, 1)), float("-inf"), dtype=torch.float32, device=score.device)
        if rows.R:
            counts = np.diff(rows.ptr)
            owner = np.repeat(np.arange(N, dtype=np.int64), counts)
            slot = owner * max(K, 1) + (np.arange(rows.R, dtype=np.int64) - rows.ptr[:-1].astype(np.int64)[owner])
            table.view(-1).index_copy_(0, torch.from_numpy(slot).to(score.device, non_blocking=True), score)
        return ops.ctc_lexicon_best(table, nbest)

    @torch.no_grad()
    def scores2chars(self, result, seq, img_hw=(32, 128), grid_hw=(8, 32)):
        """The host view of DINO_Finetune.forward_score: `result` its dict, `seq` the rows of words2rows -> one record per word,
        {'word', 'log_prob', 'eos_conf', 'chars': [{'char', 'conf', 'cx', 'cy', 'box': [x0, y0, x1, y1]}]}: conf = exp(char_logp), the
        probability of the character given the ones before it; (cx, cy) the centre of the decoder's attention when it emits the
        character, in pixels of the img_hw image - (mean + 0.5) cells of the grid_hw token grid; box that centre +- max(sqrt(3) std,
        0.5) cells per axis (a uniform extent of width w has std w / sqrt(12)), clipped to the image.  This is where the decoder LOOKS
        when it writes the character - the last layer's encoder-decoder attention, averaged over the heads - not the extent of the
        ink: a sharp map gives the half-cell floor, a map spread over the word a box as wide as the word.  An infeasible row gives
        {'word': None, 'log_prob': -inf, 'eos_conf': 0.0, 'chars': []}."""
        length = result["length"].cpu().numpy()
        logp, score = result["char_logp"].double().cpu().numpy(), result["score"].double().cpu().numpy()
        pos = result["char_pos"].double().cpu().numpy()
        seq = np.asarray(seq.cpu() if isinstance(seq, torch.Tensor) else seq)
        if seq.shape[0] != length.shape[0] or seq.shape[1] != logp.shape[1] + 1:
            raise ValueError(f"scores2chars: seq {list(seq.shape)} does not belong to a result of {length.shape[0]} rows of {logp.shape[1]} positions")
        cell_h, cell_w = img_hw[0] / grid_hw[0], img_hw[1] / grid_hw[1]
        records = []
        for r, n in enumerate(length.tolist()):
            if n < 0:
                records.append({"word": None, "log_prob": float("-inf"), "eos_conf": 0.0, "chars": []})
                continue
            chars = []
            for t in range(n):
                mean_x, mean_y, std_x, std_y = pos[r, t]
                cx, cy = (mean_x + 0.5) * cell_w, (mean_y + 0.5) * cell_h
                hx, hy = max(np.sqrt(3.0) * std_x, 0.5) * cell_w, max(np.sqrt(3.0) * std_y, 0.5) * cell_h
                chars.append({"char": self.idx2char[int(seq[r, t + 1])], "conf": float(np.exp(logp[r, t])), "cx": float(cx), "cy": float(cy),
                              "box": [float(max(cx - hx, 0.0)), float(max(cy - hy, 0.0)), float(min(cx + hx, img_hw[1])),
                                      float(min(cy + hy, img_hw[0]))]})
            records.append({"word": "".join(c["char"] for c in chars), "log_prob": float(score[r]), "eos_conf": float(np.exp(logp[r, n])),
                            "chars": chars})
        return records

    @torch.no_grad()
    def tensor2idx(self, outputs, img_metas=None):
        """[N, T, C] class scores -> (class indices, softmax confidences) per sample: positions up to the first <EOS>,
        <PAD> positions skipped."""
        probs = outputs.float().softmax(dim=-1)
        conf, cls = probs.max(dim=-1)                                        # [N, T]
        is_end = cls == self.end_idx
        before_end = torch.cumsum(is_end.int(), dim=1) == 0                  # strictly before the first <EOS>
        keep = (before_end & (cls != self.padding_idx)).cpu().numpy()
        cls_np, conf_np = cls.cpu().numpy(), conf.cpu().numpy()
        indexes = [cls_np[i][keep[i]].tolist() for i in range(cls_np.shape[0])]
        scores = [conf_np[i][keep[i]].tolist() for i in range(cls_np.shape[0])]
        return indexes, scores

    @torch.no_grad()
    def paths2nbest(self, paths, lengths, scores, nbest=1):
        """What DINO_Finetune.forward_beam returns - paths [N, W, T], lengths [N, W], scores [N, W] - -> (indexes, log_probs) as
        CTCConvertor.tensor2nbest returns them: indexes[i] holds up to `nbest` index lists, best first (an unused slot gives none);
        log_probs is a float tensor [N, nbest] on the host, the log-probability of each word with its <EOS>, -inf for an unused slot."""
        if paths.dim() != 3 or tuple(lengths.shape) != tuple(paths.shape[:2]) or tuple(scores.shape) != tuple(paths.shape[:2]):
            raise ValueError(f"paths2nbest: expects paths [N, W, T], lengths [N, W] and scores [N, W], got {list(paths.shape)}, "
                             f"{list(lengths.shape)}, {list(scores.shape)}")
        return nbest_lists("paths2nbest", paths, lengths, scores, nbest)

    @torch.no_grad()
    def paths2lexicon(self, word_ids, log_probs, nbest=1):
        """What DINO_Finetune.forward_lexicon returns - word_ids int32 [N, W] and log_probs fp32 [N, W], best first - -> (indexes,
        log_probs, word_ids) as CTCConvertor.tensor2lexicon returns them on the host: indexes[i] holds up to `nbest` index lists (the
        classes of lexicon_words[v]; fewer where the beam ended with fewer words), log_probs a float tensor [N, nbest], the exact
        log-probability of each word with its <EOS>, -inf where a slot is empty; word_ids an int64 tensor [N, nbest], -1 likewise."""
        if self.lexicon is None:
            raise ValueError("paths2lexicon: the convertor has no lexicon (set_lexicon)")
        if word_ids.dim() != 2 or tuple(log_probs.shape) != tuple(word_ids.shape):
            raise ValueError(f"paths2lexicon: expects word_ids [N, W] and log_probs [N, W], got {list(word_ids.shape)} and "
                             f"{list(log_probs.shape)}")
        if not 1 <= int(nbest) <= word_ids.shape[1]:
            raise ValueError(f"paths2lexicon: nbest must lie in 1..{word_ids.shape[1]}, got {nbest}")
        ids = word_ids[:, :int(nbest)].long().cpu()
        words, lengths = self.lexicon.words, self.lexicon.lengths
        indexes = [[(words[v, :lengths[v]] - 1).tolist() for v in row if v >= 0] for row in ids.tolist()]
        return indexes, log_probs[:, :int(nbest)].float().cpu(), ids
