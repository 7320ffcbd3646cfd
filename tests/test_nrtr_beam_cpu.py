"""The numpy specification of beam search over the NRTR decoder (tests/nrtr_beam_np.py) against the arg-max chain and brute force, and
the condition of the inputs the kernel checks use (tests/nrtr_beam_checks.py); then the configuration surface.  No kernel runs."""
import os

import numpy as np
import pytest

import nrtr_beam_checks as K
import nrtr_beam_np as R


def test_width_one_is_the_arg_max_chain():
    for C, T, bias in ((92, 25, "end"), (3, 4, "flat"), (65, 25, "flat")):
        tab = R.tables(11, 4, T, C, bias)
        for b in range(4):
            paths, lengths, scores, parents, _ = R.beam_search(tab[b], 1, C - 1, C - 1, C)
            word, score = R.greedy(tab[b], C - 1, C - 1)
            assert paths[0, :lengths[0]].tolist() == word and (paths[0, lengths[0]:] == -1).all()
            assert abs(scores[0] - score) <= 1e-12 * abs(score) and (parents == 0).all()


def test_a_wide_beam_equals_brute_force():
    for C, T in ((3, 2), (2, 4)):
        for seed in range(5):
            tab = R.markov_table(seed, T, C)
            exact = R.brute_force(tab, C - 1, C - 1)
            paths, lengths, scores, _, gap = R.beam_search(tab, 16, C - 1, C - 1, C)
            assert gap >= R.MIN_GAP and len(exact) <= 16
            for r, (word, score, finished) in enumerate(exact):
                assert paths[r, :lengths[r]].tolist() == list(word) and (lengths[r] < T) == finished
                assert abs(scores[r] - score) <= 1e-12
            assert (lengths[len(exact):] == -1).all() and np.isneginf(scores[len(exact):]).all() and (paths[len(exact):] == -1).all()
            assert abs(np.exp(scores[:len(exact)]).sum() - 1.0) <= 1e-12


def test_unused_slots_while_the_beam_exceeds_the_candidates():
    smp = R.Sample(16, 2)
    tab = R.markov_table(3, 3, 3)
    parent, _ = smp.step(np.stack([tab[0, 2]] * 16), 2, 3)
    assert parent[:3] == [0, 0, 0] and parent[3:] == [-1] * 13 and smp.state[3:] == [R.UNUSED] * 13 and np.isneginf(smp.score[3:]).all()
    assert sorted(smp.state[:3]) == [R.LIVE, R.LIVE, R.FINISHED]
    smp.step(np.stack([tab[1, s[-1]] for s in smp.seqs]), 2, 3)
    assert sum(st != R.UNUSED for st in smp.state) == 7                         # 2 live x 3 classes + the finished one


def test_the_chosen_seeds_keep_the_gap_condition():
    assert K.dropped_fraction(R.CASES, K.SEED) <= 0.02
    assert K.dropped_fraction(R.END_HEAVY, K.SEED) <= 0.02
    assert {c[0] for c in R.CASES} == {1, 5} and {c[3] for c in R.CASES} == {4, 25}
    assert {(c[1], c[2]) for c in R.CASES} == {(w, c) for w in R.WIDTHS for c in R.CLASSES}
    for B, W, C, T, mode in R.END_HEAVY[:2]:
        lengths = np.stack([w[1] for w in K.oracle(K.SEED, B, W, C, T, mode)])
        assert (lengths == T).any() and ((lengths >= 0) & (lengths < T - 8)).any()


def test_equal_scores_rank_by_the_flat_index():
    tab = K.tie_table()[0]
    paths, lengths, scores, parents, gap = R.beam_search(tab, 4, 5, 5, 6, ties=True)
    assert gap >= R.MIN_GAP
    words = [tuple(paths[r, :lengths[r]].tolist()) for r in range(4)]
    K.check_tied_order(words, scores)
    assert scores[0] == scores[1] == scores[2] == scores[3]                      # (three twin positions: eight tied words)
    assert R.beam_search(tab, 4, 5, 5, 6)[4] == 0.0                              # without ties=True the gap names the tie


def test_yaml_and_cli_width_reach_the_nrtr_head(tmp_path):
    """decoder.beam_width of an NRTR YAML gives the convertor and the decoder their width; absent, both are 0 (greedy)."""
    from Dino.utils.utils import Config
    from ccd_amd.model.dino_vision import DINO_Finetune
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shipped = os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD.yaml")
    text = open(shipped).read()
    assert "beam_width" not in text and "decoder: {type: 'NRTRDecoder'," in text
    wide = tmp_path / "beam.yaml"
    wide.write_text(text.replace("decoder: {type: 'NRTRDecoder',", "decoder: {type: 'NRTRDecoder', beam_width: 8,", 1))
    model = DINO_Finetune(Config(str(wide)))
    assert not model.ctc and model.label_convertor.beam_width == 8 and model.decoder.beam_width == 8
    plain = DINO_Finetune(Config(shipped))
    assert plain.label_convertor.beam_width == 0 and plain.decoder.beam_width == 0 and not plain.decoder._beam_graphs
    config = Config(shipped)
    config.decoder_beam_width = 17                                             # what --beam_width 17 sets
    with pytest.raises(ValueError, match="beam_width must lie in 0..16"):
        DINO_Finetune(config)
    from decoding_flags import SCRIPTS, declared
    for script in SCRIPTS:
        helps, configure = declared(script)
        assert "either head" in helps["--beam_width"] and not any(text.startswith("CTC head") for text in helps.values())
        assert configure(["--beam_width", "17"]) == {"decoder_beam_width": 17}
