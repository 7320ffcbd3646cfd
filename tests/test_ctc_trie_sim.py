"""CTC prefix beam search along a lexicon's prefix tree (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_TRIE>, ccd_ctc_beam_search_trie)
and the two-stage decoder ops.ctc_lexicon_search under the CPU SIMT executor (tests/hipsim), through the wrappers of ccd_amd.ops.  The
same checks run on the MI355X in tests/test_ctc_trie_gpu.py; gates: tests/ctc_trie_checks.py."""
import pytest
import torch

from backends import Backend
import ctc_trie_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_exhaustive_shapes_give_the_lexicons_feasible_words_sim(sim):
    K.check_exhaustive(CPU)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_paths_scores_and_word_ids_equal_the_oracle_sim(sim, seed):
    K.check_oracle(CPU, (seed,))


def test_longest_frames_and_classes_sim(sim):
    K.check_oracle_long(CPU)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_the_searched_best_word_is_the_exhaustive_best_sim(sim, seed):
    K.check_recall(CPU, (seed,))


def test_a_merge_inside_the_trie_sim(sim):
    K.check_merge(CPU)


def test_a_full_lexicon_is_the_plain_beam_byte_for_byte_sim(sim):
    K.check_full_lexicon(CPU)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)


def test_a_malformed_table_stays_inside_the_table_sim(sim):
    K.check_malformed_table(CPU)


def test_convertor_with_a_lexicon_beam_sim(sim):
    K.check_convertor(CPU)


def test_alignment_takes_the_searched_word_sim(sim):
    K.check_align(CPU)


def test_text_accuracy_with_a_lexicon_beam_sim(sim):
    K.check_update_scores(CPU)
