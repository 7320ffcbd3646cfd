"""Lexicon-constrained CTC decoding (kernels/ctc_lexicon.h: ccd_ctc_lexicon_score, ccd_ctc_lexicon_best) under the CPU SIMT executor
(tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on the MI355X in tests/test_ctc_lexicon_gpu.py; gates:
tests/ctc_lexicon_checks.py."""
import pytest
import torch

from backends import Backend
import ctc_lexicon_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_exhaustive_lexicons_equal_brute_force_sim(sim):
    K.check_exhaustive(CPU)


def test_scores_and_best_words_equal_the_oracle_sim(sim):
    K.check_oracle_batch(CPU)


def test_length_class_seams_give_identical_bits_sim(sim):
    K.check_seams(CPU)


def test_limits_of_frames_classes_and_labels_sim(sim):
    K.check_limits(CPU)


def test_masked_frames_and_classes_sim(sim):
    K.check_masks(CPU)


def test_subset_equals_the_gathered_columns_sim(sim):
    K.check_subset(CPU)


def test_a_word_listed_twice_ranks_the_lower_column_first_sim(sim):
    K.check_ties(CPU)


def test_scores_equal_the_loss_kernels_sim(sim):
    K.check_against_loss(CPU)


def test_beam_scores_are_lower_bounds_of_lexicon_scores_sim(sim):
    K.check_against_beam(CPU)


def test_random_lexicon_against_the_loss_kernel_sim(sim):
    K.check_property(CPU, B=3, V=300, n_pairs=200)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)


def test_convertor_lexicon_sim(sim, tmp_path):
    K.check_convertor(CPU, tmp_path)


def test_text_accuracy_with_a_lexicon_sim(sim):
    K.check_update_scores(CPU)
