"""What the label codecs of the two recognition heads (attn.AttnConvertor, ctc.CTCConvertor) share - the reference keeps the same
half in Dino/convertor/base.py: the alphabet and its code-point lookup table, words <-> class indices, the code-point tables a
decoded word is scored with on the device, and the reading of a lexicon's word list.  What a codec adds is its special classes,
its target layout (`str2tensor`), its decoding rule (`tensor2idx`) and what it allows next to a lexicon."""
from __future__ import annotations

import numpy as np

_DIGITS_LOWER = "0123456789abcdefghijklmnopqrstuvwxyz"
_UPPER_PUNCT = "ABCDEFGHIJKLMNOPQRSTUVWXYZ!\"#$%&'()*+,-./:;<=>?@[\\]_`~"
ALPHABETS = {
    "DICT36": _DIGITS_LOWER,
    "DICT37": _DIGITS_LOWER + " ",
    "DICT90": _DIGITS_LOWER + _UPPER_PUNCT,
    "DICT91": _DIGITS_LOWER + _UPPER_PUNCT + " ",
}
_NO_CLASS = -1


def _read_alphabet_file(path):
    chars = []
    with open(path, encoding="utf-8") as f:
        for number, raw in enumerate(f, start=1):
            entry = raw.rstrip("\r\n")
            if len(entry) > 1:
                raise ValueError(f"{path}:{number}: a dictionary line holds at most one character, found {len(entry)}")
            if entry:
                chars.append(entry)
    return chars


def checked_beam_width(beam_width, limit):
    """A constructor's `beam_width` (None counts as 0: greedy decoding) as an int in 0..limit, the decoder's widest beam."""
    width = int(beam_width or 0)
    if not 0 <= width <= limit:
        raise ValueError(f"beam_width must lie in 0..{limit} (0: greedy decoding), got {beam_width}")
    return width


def nbest_lists(who, paths, lengths, scores, nbest):
    """A beam decoder's paths [N, W, T] (-1-padded), lengths [N, W] (-1: unused slot) and scores [N, W], by rank -> (indexes,
    log_probs): indexes[i] holds up to `nbest` index lists, best first (an unused slot gives none); log_probs is a float tensor
    [N, nbest] on the host.  `who` names the caller in the error."""
    nbest = int(nbest)
    if not 1 <= nbest <= paths.shape[1]:
        raise ValueError(f"{who}: nbest must lie in 1..beam_width = {paths.shape[1]}, got {nbest}")
    paths, lengths = paths[:, :nbest].cpu().numpy(), lengths[:, :nbest].cpu().numpy()
    indexes = [[paths[i, r, :lengths[i, r]].tolist() for r in range(nbest) if lengths[i, r] >= 0] for i in range(paths.shape[0])]
    return indexes, scores[:, :nbest].float().cpu()


class BaseConvertor:
    """The alphabet of `dict_file` (one character per line), else `dict_list`, else `dict_type`, and the conversions that need
    nothing else.  A subclass lays out `idx2char` around the alphabet and calls `_index_alphabet` with the class of its first
    character; `unknown_idx` (None: a character outside the alphabet is an error) and `lower` are read when a word is encoded."""

    dicts = {name: tuple(chars) for name, chars in ALPHABETS.items()}      # same table name as the reference exposes
    unknown_idx = None
    lower = False

    @staticmethod
    def _alphabet(dict_type, dict_file, dict_list):
        if dict_file is not None:
            alphabet = _read_alphabet_file(dict_file)
        elif dict_list is not None:
            alphabet = list(dict_list)
        elif dict_type in ALPHABETS:
            alphabet = list(ALPHABETS[dict_type])
        else:
            raise NotImplementedError(f"unknown dictionary type {dict_type!r} (have {sorted(ALPHABETS)})")
        if len(set(alphabet)) != len(alphabet):
            raise AssertionError("dictionary holds a character twice")
        return alphabet

    def _index_alphabet(self, alphabet, first_class):
        """`char2idx` of the finished `idx2char`, and the code point -> class table: a word is encoded by three array operations, no
        Python loop per character.  A code point outside the table is _NO_CLASS: <UKN>, or an error."""
        self.char2idx = {c: i for i, c in enumerate(self.idx2char)}
        points = [ord(c) for c in alphabet if len(c) == 1]
        self._lut = np.full(max(points) + 1 if points else 1, _NO_CLASS, dtype=np.int64)
        for cls, c in enumerate(alphabet, start=first_class):
            if len(c) == 1:
                self._lut[ord(c)] = cls

    def num_classes(self):
        return len(self.idx2char)

    def _classes_of(self, word):
        if self.lower:
            word = word.lower()
        points = np.frombuffer(word.encode("utf-32-le"), dtype="<u4").astype(np.int64)
        inside = points < self._lut.size
        cls = np.where(inside, self._lut[np.minimum(points, self._lut.size - 1)], _NO_CLASS)
        missing = cls == _NO_CLASS
        if missing.any():
            if self.unknown_idx is None:
                bad = word[int(np.argmax(missing))]
                raise KeyError(f"character {bad!r} is not in the dictionary (pass with_unknown=True or a custom dict_file)")
            cls = np.where(missing, self.unknown_idx, cls)
        return cls

    def str2idx(self, strings):
        if not isinstance(strings, list):
            raise TypeError("str2idx expects a list of strings")
        return [self._classes_of(w).tolist() for w in strings]

    def idx2str(self, indexes):
        if not isinstance(indexes, list):
            raise TypeError("idx2str expects a list of index lists")
        table = self.idx2char
        return ["".join(table[i] for i in row) for row in indexes]

    def str2tensor(self, strings):
        raise NotImplementedError

    def tensor2idx(self, outputs, img_metas=None):
        raise NotImplementedError

    def tensor2best(self, outputs):
        """The best word of every sample as a list of class indices, decoded on the host from the decoder's [N, T, C] output (what
        TextAccuracy's host path scores): the codec's greedy rule, unless the codec has a decoder of its own configured."""
        return self.tensor2idx(outputs)[0]

    def _code_point_tables(self, silent):
        """(raw, normalised) int32 [num_classes, width]: row c = the code points of idx2char[c] as idx2str writes it / as
        TextAccuracy normalises it, padded with -1; the classes of `silent` never reach a decoded string: their rows are empty."""
        from ..metric.eval_acc import normalise
        raw = ["" if c in silent else s for c, s in enumerate(self.idx2char)]
        tables = []
        for rows in (raw, [normalise(s) for s in raw]):
            table = np.full((len(rows), max(1, max(map(len, rows)))), -1, dtype=np.int32)
            for row, s in zip(table, rows):
                row[:len(s)] = np.frombuffer(s.encode("utf-32-le"), dtype="<u4")
            tables.append(table)
        return tuple(tables)

    def _lexicon_rows(self, strings_or_path, longest, offset):
        """The word-list half of set_lexicon: a list of words, or the path of a UTF-8 file with one word per line (empty lines
        skipped) -> (rows int64 [V, width]: class + offset of every kept word, zero-padded; the kept words; {'read', 'kept',
        'too_long', 'duplicates'}).  The words are encoded as targets are (`lower`, <UKN>); a word of more than `longest` classes
        and a word that encodes as an earlier one are dropped and counted."""
        if isinstance(strings_or_path, (str, bytes)) or hasattr(strings_or_path, "__fspath__"):
            with open(strings_or_path, encoding="utf-8") as f:
                strings = [line.rstrip("\r\n") for line in f]
            strings = [w for w in strings if w]
        else:
            strings = list(strings_or_path)
            if not all(isinstance(w, str) for w in strings):
                raise TypeError("set_lexicon expects a list of strings or the path of a word list")
        kept, rows, seen, too_long, duplicates = [], [], set(), 0, 0
        for word, cls in zip(strings, self.str2idx(strings)):
            if len(cls) > longest:
                too_long += 1
            elif tuple(cls) in seen:
                duplicates += 1
            else:
                seen.add(tuple(cls))
                kept.append(word)
                rows.append(cls)
        words = np.zeros((len(rows), max(1, max(map(len, rows), default=1))), dtype=np.int64)
        for row, cls in zip(words, rows):
            row[:len(cls)] = np.asarray(cls, dtype=np.int64) + offset
        return words, kept, {"read": len(strings), "kept": len(kept), "too_long": too_long, "duplicates": duplicates}
