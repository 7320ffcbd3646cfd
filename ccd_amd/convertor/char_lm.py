"""A character n-gram language model for the CTC head's beam search (ops.ctc_beam_search_lm, CTCConvertor(lm=...)).

`CharNGram.from_words(convertor, strings_or_path, order=2, k=1.0)` estimates the table from a word list.  Words are encoded as targets
are (`lower`, `<UKN>`).  A word of classes c_1 .. c_L contributes L + 1 events - its characters and one end event, class 0 - each under
the context of the order - 1 classes in front of it, padded with 0 ("start of word") where the word is shorter.  Smoothing is additive,
by recursion over the order:
    P_n(e | ctx) = (count(ctx, e) + k * P_{n-1}(e | shorter ctx)) / (count(ctx) + k),      P_0 = 1 / C
over the C events (the C - 1 characters and the end), where the shorter context drops the oldest class.  The recursion runs in fp64, then
the log is taken and cast to fp32.  Every row is a distribution over the C columns, the rows of unseen contexts included (they hold the
lower order's distribution); a row whose context holds a 0 behind a non-zero class can never be addressed and is filled the same way.

The table's layout is the kernel's: fp32 [C^(order-1), C], the row of a context is its classes read as a number in base C (most recent
class last), column c >= 1 the log-probability of character c, column 0 that of the word ending.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_ORDER = 3                                             # ops.CTC_LM_MAX_ORDER


class CharNGram:
    """table fp32 numpy [C^(order-1), C], order, and the alphabet (the convertor's idx2char) the classes index."""

    def __init__(self, table, order, alphabet):
        table = np.ascontiguousarray(table, dtype=np.float32)
        order = int(order)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"CharNGram: order must lie in 1..{MAX_ORDER}, got {order}")
        alphabet = [str(c) for c in alphabet]
        if table.ndim != 2 or table.shape != (len(alphabet) ** (order - 1), len(alphabet)):
            raise ValueError(f"CharNGram: an order-{order} table over {len(alphabet)} classes has shape "
                             f"[{len(alphabet) ** (order - 1)}, {len(alphabet)}], got {list(table.shape)}")
        if np.isnan(table).any():
            raise ValueError("CharNGram: the table holds NaN")
        self._table, self.order, self.alphabet = table, order, alphabet

    @property
    def table(self):
        """The table as a host fp32 tensor, what ops.ctc_char_lm takes."""
        return torch.from_numpy(self._table)

    @property
    def stats(self):
        return {"order": self.order, "classes": len(self.alphabet), "rows": int(self._table.shape[0]), "bytes": int(self._table.nbytes)}

    # ------------------------------------------------------------------ estimation
    @classmethod
    def from_words(cls, convertor, strings_or_path, order=2, k=1.0):
        order, k = int(order), float(k)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"CharNGram.from_words: order must lie in 1..{MAX_ORDER}, got {order}")
        if not k > 0.0:
            raise ValueError(f"CharNGram.from_words: k must be > 0, got {k}")
        strings = read_words(strings_or_path, "CharNGram.from_words")
        C = convertor.num_classes()
        counts = [np.zeros((C ** n, C), dtype=np.float64) for n in range(order)]       # counts[n]: contexts of n classes
        for word in convertor.str2idx(strings):
            padded = [0] * (order - 1) + list(word)
            for pos, event in enumerate(list(word) + [0]):
                ctx = padded[pos:pos + order - 1]                                      # the order - 1 classes in front of the event
                for n in range(order):
                    row = 0
                    for c in ctx[len(ctx) - n:]:
                        row = row * C + c
                    counts[n][row, event] += 1.0
        prob = np.full((1, C), 1.0 / C)                                                # P_0, then P_1 .. P_order
        for n in range(order):
            shorter = np.tile(prob, (C ** n // prob.shape[0], 1))                      # row r of n classes -> its last n - 1: r mod C^(n-1)
            prob = (counts[n] + k * shorter) / (counts[n].sum(axis=1, keepdims=True) + k)
        with np.errstate(divide="ignore"):
            return cls(np.log(prob).astype(np.float32), order, convertor.idx2char)

    # ------------------------------------------------------------------ files
    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, table=self._table, order=np.int64(self.order), alphabet=np.array(self.alphabet, dtype=np.str_))

    @classmethod
    def load(cls, path, convertor=None):
        """The model of an .npz written by save(); with `convertor`, a table built for another alphabet is refused."""
        with np.load(path, allow_pickle=False) as f:
            model = cls(f["table"], int(f["order"]), [str(c) for c in f["alphabet"]])
        if convertor is not None:
            model.check_alphabet(convertor)
        return model

    def check_alphabet(self, convertor):
        if list(convertor.idx2char) != self.alphabet:
            raise ValueError(f"CharNGram: the table was built for another alphabet ({len(self.alphabet)} classes, the convertor has "
                             f"{len(convertor.idx2char)}; the classes must agree one by one)")


def read_words(strings_or_path, who):
    """A list of words, or the path of a UTF-8 file with one word per line (empty lines skipped) -> the list."""
    if isinstance(strings_or_path, (str, bytes)) or hasattr(strings_or_path, "__fspath__"):
        with open(strings_or_path, encoding="utf-8") as f:
            strings = [line.rstrip("\r\n") for line in f]
        return [w for w in strings if w]
    strings = list(strings_or_path)
    if not all(isinstance(w, str) for w in strings):
        raise TypeError(f"{who} expects a list of strings or the path of a word list")
    return strings
