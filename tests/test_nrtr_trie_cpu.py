"""Lexicon-constrained beam search over the NRTR decoder without any device: the specification (tests/nrtr_trie_np.py) against brute
force over the lexicon, the share of samples its gap condition skips, and the Python surface - AttnConvertor with a lexicon and a
lexicon_beam, paths2lexicon, the config and the command lines."""
import os

import numpy as np
import pytest
import torch

import nrtr_beam_np as R
import nrtr_trie_checks as K
import nrtr_trie_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the specification
def test_a_wide_beam_of_the_specification_is_brute_force_over_the_lexicon():
    """Tiny cases, a beam at least as wide as the lexicon: every word of at most T - 1 classes, by its exact score, and each score is
    the plain beam's brute-force score of that hypothesis."""
    for C, T, mode in ((3, 4, "flat"), (4, 3, "flat"), (5, 4, "end")):
        tab = R.markov_table(17 + C, T, C, mode)
        plain = {w: s for w, s, finished in R.brute_force(tab, C - 1, C - 1) if finished}
        words = S.lexicon(C, tab, size=10)
        assert any(len(w) > T - 1 for w in words) and len(words) <= 16
        nodes = S.trie_of(words)
        paths, lengths, scores, ids, node, parents, gap = S.beam_search_trie(tab, 16, C - 1, C - 1, C, nodes)
        exact = S.exact_words(tab, words, C - 1, C - 1)
        assert gap >= S.MIN_GAP and len(exact) == sum(len(w) <= T - 1 for w in words)
        ranks = [r for r in range(16) if ids[r] >= 0]
        assert [int(ids[r]) for r in ranks] == [k for k, _ in exact]
        for r, (k, score) in zip(ranks, exact):
            assert tuple(paths[r, :lengths[r]].tolist()) == tuple(words[k]) and abs(scores[r] - score) <= 1e-12
            assert abs(score - plain[tuple(words[k])]) <= 1e-12 and int(nodes[node[r], 5]) == k


def test_a_full_lexicon_is_no_constraint_for_the_specification():
    """Every word of at most T - 1 classes, and every longer prefix: the constrained beam is the plain beam."""
    import itertools
    C, T = 4, 3
    tab = R.markov_table(5, T, C)
    words = [w for n in range(0, T + 1) for w in itertools.product(range(C - 1), repeat=n)]
    nodes = S.trie_of(words)
    for W in (1, 3, 16):
        want = R.beam_search(tab, W, C - 1, C - 1, C)
        got = S.beam_search_trie(tab, W, C - 1, C - 1, C, nodes)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and np.array_equal(got[5], want[3])
        for r in range(W):                                                     # a word where the slot finished, no word at T classes
            assert (got[3][r] >= 0) == (0 <= got[1][r] < T), (W, r)
            if got[3][r] >= 0:
                assert tuple(got[0][r, :got[1][r]].tolist()) == words[got[3][r]]


def test_word_score_and_the_offset():
    tab = R.markov_table(3, 5, 6)
    lp0 = S.log_softmax64(tab[0, 5])
    lp1 = S.log_softmax64(tab[1, 2])
    assert abs(S.word_score(tab, (2,), 5, 5) - (lp0[2] + lp1[5])) <= 1e-15 and S.word_score(tab, (), 5, 5) == lp0[5]
    assert S.word_score(tab, (1, 2, 3, 4, 0), 5, 5) == -np.inf                # five classes: the <EOS> has no step left
    rows = S.rows_of([(0, 4), (3,)])
    assert rows.tolist() == [[1, 5], [4, 0]] and S.rows_of([(0, 4)], 0).tolist() == [[0, 4]]
    smp = S.TrieSample(2, 5, S.trie_of([(0, 4), (3,)]))
    assert np.flatnonzero(smp.allowed(0, 6, 5)).tolist() == [0, 3]            # the root: classes 0 and 3, no <EOS>
    assert np.flatnonzero(smp.allowed(2, 6, 5)).tolist() == [5]               # behind (3,): the word ends


def test_the_lexicon_generator_is_what_the_checks_describe():
    tab = R.markov_table(1, 25, 92, "end")
    words = S.lexicon(4, tab)
    assert len(words) == 300 == len(set(words)) and all(91 not in w for w in words)
    assert sum(len(w) > 24 for w in words) == 1 and min(map(len, words)) >= 1
    prefixes = sum(any(v != w and v[:len(w)] == w for v in words) for w in words)
    assert prefixes >= 30                                                      # 30 % of the words bring a proper prefix along
    assert len(S.lexicon(4, R.markov_table(1, 4, 3))) == 6
    assert words == S.lexicon(4, tab)


def test_oracle_gap_condition_skips_at_most_two_percent():
    assert K.dropped_fraction() <= 0.02


# ------------------------------------------------------------------------------------------------ the convertor
def test_attn_convertor_takes_a_lexicon_with_a_lexicon_beam():
    from ccd_amd import ops
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=25, with_unknown=True, lexicon=["hello", "0a", "hell", "hello", "x" * 25, "y" * 24],
                         lexicon_beam=8)
    assert conv.lexicon_stats == {"read": 6, "kept": 4, "too_long": 1, "duplicates": 1, "nodes": 1 + 5 + 2 + 24}
    assert conv.lexicon_words == ["hello", "0a", "hell", "y" * 24] and conv.lexicon_beam == 8 and conv.beam_width == 0
    assert isinstance(conv.lexicon, ops.CTCLexicon) and isinstance(conv.lexicon_trie, ops.CTCLexiconTrie)
    assert conv.lexicon.words[1, :3].tolist() == [1, 11, 0]                   # '0' is class 0: the rows are class + 1
    assert conv.lexicon_trie.n_nodes == 32 and conv.lexicon_trie.stats["terminals"] == 4
    # the two refusals other tests pin, and what else is refused
    for kw in (dict(lexicon=["a"]), dict(lexicon_beam=4)):
        with pytest.raises(NotImplementedError, match="CTC head only"):
            AttnConvertor(**kw)
    with pytest.raises(NotImplementedError, match="lexicon_beam: N"):
        AttnConvertor(lexicon=["a"])
    with pytest.raises(NotImplementedError, match="CTC head only"):
        AttnConvertor(lm="words.txt", beam_width=4)
    for beam in (17, -1, 2.5):
        with pytest.raises(ValueError, match="lexicon_beam must lie in 1..16"):
            AttnConvertor(lexicon=["a"], lexicon_beam=beam)
    with pytest.raises(ValueError, match="lexicon.*beam_width|beam_width.*lexicon"):
        AttnConvertor(lexicon=["a"], lexicon_beam=4, beam_width=4)
    # set_lexicon: replaces, keeps the width, removes
    stats = conv.set_lexicon(["ab", "abc", "b"])
    assert stats == {"read": 3, "kept": 3, "too_long": 0, "duplicates": 0, "nodes": 5} and conv.lexicon_beam == 8
    assert conv.set_lexicon(["ab"], beam=16)["nodes"] == 3 and conv.lexicon_beam == 16
    conv.set_lexicon(None)
    assert conv.lexicon is None and conv.lexicon_trie is None and conv.lexicon_words is None and conv.lexicon_beam == 0
    with pytest.raises(ValueError, match="lexicon_beam must lie in 1..16"):
        conv.set_lexicon(["ab"])                                               # no width yet
    with pytest.raises(ValueError, match="needs a lexicon"):
        conv.set_lexicon(None, beam=4)
    plain = AttnConvertor()
    assert plain.lexicon is None and plain.lexicon_trie is None and plain.lexicon_beam == 0 and plain.lexicon_stats is None
    long_rows = AttnConvertor(max_seq_len=40, lexicon=["z" * 31, "z" * 32], lexicon_beam=2)      # a lexicon row holds 31 classes
    assert long_rows.lexicon_stats["too_long"] == 1 and long_rows.lexicon_stats["kept"] == 1


def test_set_lexicon_reads_a_word_list(tmp_path):
    from ccd_amd.convertor.attn import AttnConvertor
    path = tmp_path / "words.txt"
    path.write_text("hello\n\nworld\r\nhell\n", encoding="utf-8")
    conv = AttnConvertor(max_seq_len=25, lexicon=str(path), lexicon_beam=4)
    assert conv.lexicon_words == ["hello", "world", "hell"] and conv.lexicon_stats["read"] == 3 and conv.lexicon_stats["nodes"] == 11


def test_paths2lexicon_is_the_host_view():
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(max_seq_len=25, lexicon=["hello", "0a", "hell"], lexicon_beam=4)
    ids = torch.tensor([[1, 0, -1, -1], [2, -1, -1, -1], [-1, -1, -1, -1]], dtype=torch.int32)
    lp = torch.tensor([[-0.5, -2.0, float("-inf"), float("-inf")], [-1.0] + [float("-inf")] * 3, [float("-inf")] * 4])
    indexes, log_probs, word_ids = conv.paths2lexicon(ids, lp, nbest=2)
    assert indexes == [[[0, 10], conv.str2idx(["hello"])[0]], [conv.str2idx(["hell"])[0]], []]
    assert conv.idx2str([w[0] if w else [] for w in indexes]) == ["0a", "hell", ""]
    assert word_ids.dtype == torch.int64 and word_ids.tolist() == [[1, 0], [2, -1], [-1, -1]]
    assert log_probs.dtype == torch.float32 and tuple(log_probs.shape) == (3, 2) and float(log_probs[0, 1]) == -2.0
    assert conv.paths2lexicon(ids, lp)[0] == [[[0, 10]], [conv.str2idx(["hell"])[0]], []]
    with pytest.raises(ValueError, match="nbest must lie in 1..4"):
        conv.paths2lexicon(ids, lp, nbest=5)
    with pytest.raises(ValueError, match="expects word_ids"):
        conv.paths2lexicon(ids, lp[:, :2])
    with pytest.raises(ValueError, match="no lexicon"):
        AttnConvertor().paths2lexicon(ids, lp)


# ------------------------------------------------------------------------------------------------ the config and the command lines
def test_lexicon_and_lexicon_beam_reach_the_nrtr_convertor_from_the_config(tmp_path):
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    from ccd_amd.utils.utils import Config
    words = tmp_path / "words.txt"
    words.write_text("hello\nworld\nhell\n", encoding="utf-8")
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2)
    cfg.decoder_lexicon, cfg.decoder_lexicon_beam = str(words), 8
    model = DINO_Finetune(cfg)
    conv = model.label_convertor
    assert not model.ctc and conv.lexicon_beam == 8 and conv.lexicon_trie.n_nodes == 11 and conv.lexicon_words == ["hello", "world", "hell"]
    assert model.decoder.beam_width == 0 and len(model.decoder._beam_graphs) == 0 and len(model.decoder._trie_graphs) == 0
    absent = DINO_Finetune(ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2))
    assert absent.label_convertor.lexicon is None and absent.label_convertor.lexicon_trie is None
    with pytest.raises(ValueError, match="no lexicon"):
        absent.forward_lexicon(torch.zeros(1, 3, 32, 128))
    for key, value in (("decoder_lexicon", str(words)), ("decoder_lexicon_beam", 8)):      # either alone: the pinned refusal
        one = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2)
        setattr(one, key, value)
        with pytest.raises(NotImplementedError, match="CTC head only"):
            DINO_Finetune(one)
    ctc = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    ctc.decoder_type, ctc.decoder_lexicon = "CTCDecoder", str(words)
    with pytest.raises(NotImplementedError, match="tensor2lexicon"):
        DINO_Finetune(ctc).forward_lexicon(torch.zeros(1, 3, 32, 128))
    src = open(os.path.join(ROOT, "Dino", "configs", "CCD_vision_model_ARD.yaml")).read()
    assert Config(os.path.join(ROOT, "Dino", "configs", "CCD_vision_model_ARD.yaml")).decoder_lexicon_beam is None
    (tmp_path / "lex.yaml").write_text(src.replace("padding_idx: 92}", f"padding_idx: 92, lexicon: '{words}', lexicon_beam: 16}}"))
    config = Config(str(tmp_path / "lex.yaml"))
    assert config.decoder_lexicon == str(words) and config.decoder_lexicon_beam == 16 and config.decoder_type == "NRTRDecoder"
    config.decoder_n_layers = 1
    assert DINO_Finetune(config).label_convertor.lexicon_stats == {"read": 3, "kept": 3, "too_long": 0, "duplicates": 0, "nodes": 11}


def test_forward_beam_refuses_a_foreign_trie():
    from ccd_amd.decoder.nrtr_decoder import NRTRDecoder
    dec = NRTRDecoder(n_layers=1, max_seq_len=25)
    with pytest.raises(TypeError, match="trie must come from ops.ctc_lexicon_trie"):
        dec.forward_beam(None, torch.zeros(1, 256, 512), 4, trie=object())


def test_command_lines_describe_the_nrtr_lexicon():
    from decoding_flags import SCRIPTS, declared
    for name in SCRIPTS:
        assert "NRTR head" in declared(name)[0]["--lexicon_beam"], name
