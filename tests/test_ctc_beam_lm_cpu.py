"""The oracle of language-model fusion (tests/ctc_beam_lm_np.py) against brute force - where every word fits the beam nothing is
pruned, so the hypotheses are all the words with log p_ctc(word) + word_term(word), in that order -, the gap condition of the inputs
the executor / GPU tests use, the n-gram estimator (ccd_amd/convertor/char_lm.py) and the refusals of the convertors.  No GPU, no
kernel."""
import numpy as np
import pytest
import torch

import ctc_beam_lm_np as L
import ctc_beam_np as R


@pytest.mark.parametrize("T,C", R.EXHAUSTIVE)
@pytest.mark.parametrize("normalized", (False, True))
@pytest.mark.parametrize("order", (1, 2, 3))
@pytest.mark.parametrize("eos", (False, True))
def test_oracle_equals_brute_force_plus_the_word_term(T, C, normalized, order, eos):
    x = R.small_case(T, C, seed=10 * T + C)
    if normalized:
        x = R.softmax32(x)
    table = L.synthetic_table(40 + order, C, order)
    hyps, gap = L.beam_search_lm(x, 16, table, order, 0.7, 0.35, eos, normalized)
    exact = sorted([(w, s + L.word_term(w, table, order, 0.7, 0.35, eos)) for w, s in R.brute_force(x, normalized)],
                   key=lambda e: (-e[1], e[0]))
    assert gap >= R.MIN_GAP, gap
    assert [w for w, _ in hyps] == [w for w, _ in exact] and len(exact) == {(3, 3): 9, (4, 2): 3, (6, 2): 4}[(T, C)]
    assert max(abs(a - b) for (_, a), (_, b) in zip(hyps, exact)) <= 1e-12


def test_weight_zero_and_a_finite_table_are_the_plain_oracle():
    for seed, normalized in ((100, False), (101, True)):
        x = R.peaked_batch(seed)[:3]
        x = R.softmax32(x) if normalized else x
        for order in (1, 2, 3):
            table = L.synthetic_table(42, 92, order)
            for W in (1, 16):
                for b in range(3):
                    plain = R.beam_search(x[b], W, normalized)
                    for eos in (False, True):
                        assert L.beam_search_lm(x[b], W, table, order, 0.0, 0.0, eos, normalized)[0] == plain[0]


def test_peaked_inputs_meet_the_gap_condition_with_a_language_model():
    """The inputs of the executor / GPU tests: both modes, every width, orders 2 and 3, both tables - the oracle alone meets the
    condition on every sample (ctc_beam_lm_checks.oracle asserts it again where it is used)."""
    import ctc_beam_lm_checks as K
    worst = np.inf
    for seed in K.SEEDS[:1]:
        for normalized in (False, True):
            x = K.B.peaked(seed, normalized)
            for order in K.ORDERS:
                for W in K.WIDTHS:
                    for b in range(x.shape[0]):
                        worst = min(worst, L.beam_search_lm(x[b], W, K.table_of(42, 92, order), order, K.WEIGHT, K.BONUS, True, normalized)[1])
    print(f"smallest gap {worst:.3e}")
    assert worst >= R.MIN_GAP, worst


def test_masks_and_the_end_of_the_word():
    x = R.small_case(4, 3, seed=3)
    table = L.masked_table(41, 3, 2, (2,))
    hyps, _ = L.beam_search_lm(x, 16, table, 2, 0.0, 0.0)
    assert hyps and all(2 not in w for w, _ in hyps)
    plain = dict(R.brute_force(x))
    assert all(abs(s - plain[w]) <= 1e-12 for w, s in hyps) and len(hyps) == sum(2 not in w for w in plain)     # weight 0: a hard mask
    ends = L.masked_table(41, 3, 2, ())
    ends[1, 0] = -np.inf                                                       # no word may end behind class 1
    hyps, _ = L.beam_search_lm(x, 16, ends, 2, 1.0, 0.0, eos=True)
    assert hyps and all(not w or w[-1] != 1 for w, _ in hyps)
    assert L.row_of((), 3, 5) == 0 and L.row_of((3,), 3, 5) == 3 and L.row_of((1, 2, 4), 3, 5) == 14 and L.row_of((1, 2), 1, 5) == 0
    rows = L.row_masked_table(41, 4, 2)
    assert np.isneginf(rows).sum(axis=1).tolist() == [1, 1, 1, 1] and np.isneginf(rows[[0, 1, 2, 3], [1, 2, 3, 1]]).all()


# ------------------------------------------------------------------------------------------------ the estimator
SIX = ["ab", "ab", "ac", "b", "ba", "abc"]


def _abc():
    from ccd_amd.convertor.ctc import CTCConvertor
    return CTCConvertor(dict_list=["a", "b", "c"], with_unknown=False, beam_width=4)


@pytest.mark.parametrize("order", (1, 2, 3))
def test_every_row_of_the_estimated_table_is_a_distribution(order):
    from ccd_amd.convertor.char_lm import CharNGram
    model = CharNGram.from_words(_abc(), SIX, order=order)
    table = model.table
    assert table.dtype == torch.float32 and tuple(table.shape) == (4 ** (order - 1), 4) and model.order == order
    assert float((table.double().exp().sum(dim=1) - 1.0).abs().max()) <= 1e-6 and bool(torch.isfinite(table).all())


def test_a_bigram_row_by_hand():
    """ab ab ac b ba abc over (end, a, b, c): 18 events, end 6, a 5, b 5, c 2; behind `a`: end 1 (ba), b 3 (ab ab abc), c 1 (ac)."""
    from ccd_amd.convertor.char_lm import CharNGram
    conv = _abc()
    uni = (np.array([6.0, 5.0, 5.0, 2.0]) + 0.25) / 19.0
    after_a = (np.array([1.0, 0.0, 3.0, 1.0]) + uni) / 6.0
    start = (np.array([0.0, 4.0, 2.0, 0.0]) + uni) / 7.0                      # four words begin with a, two with b
    after_c = (np.array([2.0, 0.0, 0.0, 0.0]) + uni) / 3.0                    # ac and abc end there
    one = CharNGram.from_words(conv, SIX, order=1).table.numpy()
    two = CharNGram.from_words(conv, SIX, order=2).table.numpy()
    np.testing.assert_array_equal(one[0], np.log(uni).astype(np.float32))
    np.testing.assert_array_equal(two[1], np.log(after_a).astype(np.float32))
    np.testing.assert_array_equal(two[0], np.log(start).astype(np.float32))
    np.testing.assert_array_equal(two[3], np.log(after_c).astype(np.float32))
    three = CharNGram.from_words(conv, SIX, order=3, k=0.5).table.numpy()
    uni5 = (np.array([6.0, 5.0, 5.0, 2.0]) + 0.5 * 0.25) / 18.5
    after_b5 = (np.array([3.0, 1.0, 0.0, 1.0]) + 0.5 * uni5) / 5.5           # behind b: end (ab ab b), a (ba), c (abc)
    after_ab = (np.array([2.0, 0.0, 0.0, 1.0]) + 0.5 * after_b5) / 3.5       # behind ab: end twice, c once
    np.testing.assert_allclose(three[1 * 4 + 2], np.log(after_ab), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(three[2 * 4 + 0], three[3 * 4 + 0])         # never addressed: filled like any unseen context
    start5 = (np.array([0.0, 4.0, 2.0, 0.0]) + 0.5 * uni5) / 6.5              # its shorter context is 0, the start of a word
    np.testing.assert_allclose(np.exp(three[2 * 4 + 0].astype(np.float64)), start5, rtol=0, atol=1e-6)
    # the file of a word list, lower-casing and <UKN> go through the convertor's own encoding
    from ccd_amd.convertor.ctc import CTCConvertor
    low = CTCConvertor(lower=True, beam_width=1)
    a = CharNGram.from_words(low, ["Ab", "aé"], order=2).table
    b = CharNGram.from_words(low, ["ab", "aü"], order=2).table
    assert torch.equal(a, b)


def test_save_load_round_trip_and_an_alphabet_mismatch(tmp_path):
    from ccd_amd.convertor.char_lm import CharNGram
    from ccd_amd.convertor.ctc import CTCConvertor
    conv = _abc()
    model = CharNGram.from_words(conv, SIX, order=3)
    path = str(tmp_path / "lm.npz")
    model.save(path)
    back = CharNGram.load(path, conv)
    assert back.order == 3 and back.alphabet == list(conv.idx2char) and torch.equal(back.table, model.table)
    with np.load(path) as f:
        assert sorted(f.files) == ["alphabet", "order", "table"]
    assert conv.set_lm(path) == {"order": 3, "classes": 4, "rows": 16, "bytes": 256} and conv.lm_order == 3
    with pytest.raises(ValueError, match="another alphabet"):
        CharNGram.load(path, CTCConvertor(beam_width=4))
    with pytest.raises(ValueError, match="another alphabet"):
        CTCConvertor(beam_width=4, lm=path)
    with pytest.raises(ValueError, match="another alphabet"):
        CTCConvertor(dict_list=["a", "c", "b"], with_unknown=False, beam_width=4).set_lm(model)
    words = tmp_path / "words.txt"
    words.write_text("\n".join(SIX) + "\n\n", encoding="utf-8")
    conv.set_lm(str(words), order=2)
    assert torch.equal(conv.lm_model.table, CharNGram.from_words(conv, SIX, order=2).table) and conv.lm.order == 2
    assert conv.set_lm(None) is None and conv.lm is None and conv.lm_stats is None


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from ccd_amd import ops
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.convertor.char_lm import CharNGram
    from ccd_amd.convertor.ctc import CTCConvertor
    model = CharNGram.from_words(CTCConvertor(), ["hello", "world"], order=2)
    with pytest.raises(ValueError, match="needs beam_width >= 1"):
        CTCConvertor(beam_width=0, lm=model)
    with pytest.raises(ValueError, match="a language model and a lexicon exclude each other"):
        CTCConvertor(lexicon=["hello"], lm=model)
    conv = CTCConvertor(beam_width=4, lm=model, lm_weight=0.5, lm_bonus=0.25, lm_eos=False)
    assert (conv.lm_weight, conv.lm_bonus, conv.lm_eos, conv.lm_order) == (0.5, 0.25, False, 2) and isinstance(conv.lm, ops.CTCCharLM)
    with pytest.raises(ValueError, match="a lexicon and a language model exclude each other"):
        conv.set_lexicon(["hello"])
    with pytest.raises(NotImplementedError, match="CTC head only"):
        AttnConvertor(lm=model)
    with pytest.raises(ValueError, match="must be finite"):
        CTCConvertor(beam_width=4, lm=model, lm_weight=float("nan"))
    with pytest.raises(ValueError, match="order must lie in 1..3"):
        CharNGram.from_words(CTCConvertor(), ["a"], order=4)
    with pytest.raises(TypeError, match="set_lm expects"):
        CTCConvertor(beam_width=4, lm=3)


def test_the_language_model_reaches_the_convertor_from_the_config(tmp_path):
    """decoder.lm .. lm_eos of the YAML (config.decoder_lm ..) -> CTCConvertor; absent is today's behaviour; the NRTR head refuses."""
    import os
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    from ccd_amd.utils.utils import Config
    torch.manual_seed(0)
    words = tmp_path / "words.txt"
    words.write_text("hello\nworld\n", encoding="utf-8")
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    assert DINO_Finetune(cfg).label_convertor.lm is None
    cfg.decoder_lm = str(words)
    with pytest.raises(ValueError, match="needs beam_width >= 1"):
        DINO_Finetune(cfg)
    cfg.decoder_beam_width = 4
    conv = DINO_Finetune(cfg).label_convertor
    assert conv.lm_stats["order"] == 2 and (conv.lm_weight, conv.lm_bonus, conv.lm_eos) == (1.0, 0.0, True)
    cfg.decoder_lm_order, cfg.decoder_lm_weight, cfg.decoder_lm_bonus, cfg.decoder_lm_eos = 3, 0.0, 0.5, False
    conv = DINO_Finetune(cfg).label_convertor
    assert conv.lm_stats["rows"] == 92 * 92 and (conv.lm_weight, conv.lm_bonus, conv.lm_eos) == (0.0, 0.5, False)
    nrtr = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    nrtr.decoder_lm = str(words)
    with pytest.raises(NotImplementedError, match="CTC head only"):
        DINO_Finetune(nrtr)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).read()
    assert Config(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).decoder_lm is None
    (tmp_path / "lm.yaml").write_text(src.replace("max_seq_len: 25}", f"max_seq_len: 25, beam_width: 8, lm: '{words}', lm_weight: 0.7, lm_eos: false}}"))
    config = Config(str(tmp_path / "lm.yaml"))
    assert config.decoder_lm == str(words) and config.decoder_lm_weight == 0.7 and config.decoder_lm_eos is False
    assert config.decoder_lm_order is None and config.decoder_type == "CTCDecoder"
