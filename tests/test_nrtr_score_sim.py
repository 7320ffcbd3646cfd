"""Scoring given words with the NRTR decoder (kernels/nrtr_score.h: ccd_xattn_rows_fwd, ccd_nrtr_word_score) under the CPU SIMT
executor (tests/hipsim), through the wrappers of ccd_amd.ops, and the decoder end to end.  The same checks run on the MI355X in
tests/test_nrtr_score_gpu.py; gates: tests/nrtr_score_checks.py."""
import pytest
import torch

from backends import Backend
import nrtr_score_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


@pytest.mark.parametrize("Tq", [7, 32])
def test_rows_attention_equals_the_replicated_attention_bit_for_bit_sim(sim, Tq):
    K.check_rows_equal_replicated(CPU, Tq)


@pytest.mark.parametrize("Tq", [7, 32])
def test_moments_of_the_attention_maps_sim(sim, Tq):
    K.check_moments(CPU, Tq)


def test_a_one_hot_map_gives_the_key_and_std_zero_sim(sim):
    K.check_one_hot(CPU)


def test_word_scores_equal_numpy_sim(sim):
    K.check_word_scores(CPU)


def test_argument_validation_sim(sim):
    K.check_arguments(CPU)


def test_scores2words_ties_padding_and_empty_lists_sim(sim):
    K.check_best_of_lists(CPU)


def test_forward_score_reproduces_the_beam_and_forward_words_its_order_sim(sim):
    K.check_decoder_end_to_end(CPU)
