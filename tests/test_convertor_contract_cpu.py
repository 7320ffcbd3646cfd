"""The behaviour of the two label codecs that every decoding mode builds on, pinned as literals: the alphabet, encoding and decoding,
the score tables and what set_lexicon keeps of a word list.  The expected values were recorded from the codecs as they stood before
their shared half moved into convertor/base.py; nothing here is computed by the code under test."""
import pytest

DICT90 = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ!\"#$%&'()*+,-./:;<=>?@[\\]_`~"
MAX_SEQ_LEN = 8
WORDS = ["hello",                                    # lower case
         "Hi-There!",                                # mixed case with punctuation; longer than max_seq_len
         "café",                                # a character outside the alphabet: <UKN>
         "",                                         # the empty word
         "abcdefghijkl",                             # longer than max_seq_len
         "0123456789abcdefghijklmnopqrstuvw",        # 33 characters: longer than any lexicon row
         "x€", "x£",                       # a pair that encodes identically (x <UKN>)
         "hello"]                                    # ... and a plain repeat

LOWER36 = "0123456789abcdefghijklmnopqrstuvwxyz"
RAW = list(DICT90) + ["<UKN>"]                       # a class as idx2str writes it
NORM = list(LOWER36) + list(LOWER36[10:]) + [""] * 28 + ["ukn"]      # ... and as TextAccuracy compares it: lower case, punctuation dropped
IDX_CTC = [[18, 15, 22, 22, 25], [44, 19, 75, 56, 18, 15, 28, 15, 63], [13, 11, 16, 91], [], list(range(11, 23)), list(range(1, 34)),
           [34, 91], [34, 91], [18, 15, 22, 22, 25]]
DECODED = ["hello", "Hi-There!", "caf<UKN>", "", "abcdefghijkl", "0123456789abcdefghijklmnopqrstuvw", "x<UKN>", "x<UKN>", "hello"]
ROWS_CTC = [[18, 15, 22, 22, 25, 0, 0, 0, 0, 0, 0, 0], [44, 19, 75, 56, 18, 15, 28, 15, 63, 0, 0, 0],
            [13, 11, 16, 91, 0, 0, 0, 0, 0, 0, 0, 0], [0] * 12, list(range(11, 23)), [34, 91, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
ROWS_ATTN = [[18, 15, 22, 22, 25], [13, 11, 16, 91, 0], [0, 0, 0, 0, 0], [34, 91, 0, 0, 0]]      # class + 1: class 0 is the character '0'

EXPECTED = {
    "ctc": {
        "num_classes": 92,
        "str2idx": IDX_CTC,
        "idx2str": DECODED,
        "str2tensor": [[18, 15, 22, 22, 25, 0, 0, 0], [44, 19, 75, 56, 18, 15, 28, 15], [13, 11, 16, 91, 0, 0, 0, 0],
                       [0, 0, 0, 0, 0, 0, 0, 0], [11, 12, 13, 14, 15, 16, 17, 18], [1, 2, 3, 4, 5, 6, 7, 8],
                       [34, 91, 0, 0, 0, 0, 0, 0], [34, 91, 0, 0, 0, 0, 0, 0], [18, 15, 22, 22, 25, 0, 0, 0]],
        "str2tensor_dtype": "torch.int64",
        "score_table": [([92, 5], "int32", [""] + RAW), ([92, 3], "int32", [""] + NORM)],          # the blank's row is empty
        "lexicon_list": {"stats": {"read": 9, "kept": 6, "too_long": 1, "duplicates": 2, "nodes": 33},
                         "words": ["hello", "Hi-There!", "café", "", "abcdefghijkl", "x€"],
                         "rows": ROWS_CTC, "rows_dtype": "torch.int64", "trie": [33, 8], "beam": 4},
        "lexicon_file": {"stats": {"read": 8, "kept": 5, "too_long": 1, "duplicates": 2, "nodes": 33},
                         "words": ["hello", "Hi-There!", "café", "abcdefghijkl", "x€"],
                         "rows": ROWS_CTC[:3] + ROWS_CTC[4:], "rows_dtype": "torch.int64", "trie": [33, 8], "beam": 4},
    },
    "attn": {
        "num_classes": 93,
        "str2idx": [[17, 14, 21, 21, 24], [43, 18, 74, 55, 17, 14, 27, 14, 62], [12, 10, 15, 90], [], list(range(10, 22)),
                    list(range(0, 33)), [33, 90], [33, 90], [17, 14, 21, 21, 24]],                 # no blank in front; <UKN> is 90
        "idx2str": DECODED,
        "str2tensor": [[91, 17, 14, 21, 21, 24, 91, 92], [91, 43, 18, 74, 55, 17, 14, 27], [91, 12, 10, 15, 90, 91, 92, 92],
                       [91, 91, 92, 92, 92, 92, 92, 92], [91, 10, 11, 12, 13, 14, 15, 16], [91, 0, 1, 2, 3, 4, 5, 6],
                       [91, 33, 90, 91, 92, 92, 92, 92], [91, 33, 90, 91, 92, 92, 92, 92], [91, 17, 14, 21, 21, 24, 91, 92]],
        "str2tensor_dtype": "torch.int64",
        "score_table": [([93, 5], "int32", RAW + ["", ""]), ([93, 3], "int32", NORM + ["", ""])],  # <EOS> and <PAD> are silent
        "path_score_table": [([94, 5], "int32", [""] + RAW + ["", ""]), ([94, 3], "int32", [""] + NORM + ["", ""])],
        "lexicon_list": {"stats": {"read": 9, "kept": 4, "too_long": 3, "duplicates": 2, "nodes": 12},
                         "words": ["hello", "café", "", "x€"],
                         "rows": ROWS_ATTN, "rows_dtype": "torch.int64", "trie": [12, 8], "beam": 4},
        "lexicon_file": {"stats": {"read": 8, "kept": 3, "too_long": 3, "duplicates": 2, "nodes": 12},
                         "words": ["hello", "café", "x€"],
                         "rows": ROWS_ATTN[:2] + ROWS_ATTN[3:], "rows_dtype": "torch.int64", "trie": [12, 8], "beam": 4},
    },
}


def make(codec, **kw):
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.convertor.ctc import CTCConvertor
    return {"ctc": CTCConvertor, "attn": AttnConvertor}[codec](dict_type="DICT90", with_unknown=True, max_seq_len=MAX_SEQ_LEN, **kw)


def rows_of(table):
    """An int32 code-point table, rows padded with -1 -> its rows as strings (the padding must be -1 to the end of the row)."""
    out = []
    for row in table.tolist():
        n = row.index(-1) if -1 in row else len(row)
        assert all(c == -1 for c in row[n:])
        out.append("".join(chr(c) for c in row[:n]))
    return out


def observe(codec, tmp_path):
    """Everything the test pins, as plain Python values."""
    conv = make(codec)
    idx = conv.str2idx(WORDS)
    seen = {"num_classes": conv.num_classes(), "str2idx": idx, "idx2str": conv.idx2str(idx),
            "str2tensor": conv.str2tensor(WORDS).tolist(), "str2tensor_dtype": str(conv.str2tensor(WORDS).dtype)}
    tables = conv.score_table()
    seen["score_table"] = [(list(t.shape), str(t.dtype), rows_of(t)) for t in tables]
    if codec == "attn":
        seen["path_score_table"] = [(list(t.shape), str(t.dtype), rows_of(t)) for t in conv.path_score_table()]
    path = tmp_path / "words.txt"
    path.write_text("\n".join(WORDS[:2] + [""] + WORDS[2:]) + "\n", encoding="utf-8")         # (WORDS holds an empty line of its own)
    for name, source in (("list", WORDS), ("file", str(path))):
        if codec == "ctc":                                                                    # through the constructor: lexicon_beam=4
            conv = make(codec, lexicon=source, lexicon_beam=4)
        else:                                                                                 # through set_lexicon: beam=4
            conv = make(codec)
            assert conv.set_lexicon(source, beam=4) is conv.lexicon_stats
        seen["lexicon_" + name] = {"stats": dict(conv.lexicon_stats),"words": conv.lexicon_words, "rows": conv.lexicon.words.tolist(),
                                   "rows_dtype": str(conv.lexicon.words.dtype), "trie": list(conv.lexicon_trie.nodes.shape),
                                   "beam": conv.lexicon_beam}
    return seen


@pytest.mark.parametrize("codec", ["ctc", "attn"])
def test_codec_contract(codec, tmp_path):
    seen = observe(codec, tmp_path)
    want = EXPECTED[codec]
    assert sorted(seen) == sorted(want)
    for key in want:
        assert seen[key] == want[key], key


@pytest.mark.parametrize("codec", ["ctc", "attn"])
def test_unknown_character_without_unknown_class(codec):
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.convertor.ctc import CTCConvertor
    conv = {"ctc": CTCConvertor, "attn": AttnConvertor}[codec](dict_type="DICT90", with_unknown=False, max_seq_len=MAX_SEQ_LEN)
    assert conv.num_classes() == {"ctc": 91, "attn": 92}[codec] and conv.unknown_idx is None
    for call in (conv.str2idx, conv.str2tensor):
        with pytest.raises(KeyError) as err:
            call(["café"])
        assert err.value.args == ("character 'é' is not in the dictionary (pass with_unknown=True or a custom dict_file)",)
