"""CTC prefix beam search (kernels/ctc_beam.h: ccd_ctc_beam_search) and ccd_text_score_paths under the CPU SIMT executor (tests/hipsim),
through the wrappers of ccd_amd.ops.  The same checks run on the MI355X in tests/test_ctc_beam_gpu.py; gates: tests/ctc_beam_checks.py."""
import pytest
import torch

from backends import Backend
import ctc_beam_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_exhaustive_shapes_equal_brute_force_sim(sim):
    K.check_exhaustive(CPU)


def test_paths_and_scores_equal_the_oracle_sim(sim):
    K.check_oracle(CPU)


def test_longest_frames_and_classes_sim(sim):
    K.check_oracle_long(CPU)


def test_equal_scores_rank_the_lower_class_first_sim(sim):
    K.check_ties(CPU)


def test_fewer_hypotheses_than_the_beam_sim(sim):
    K.check_fewer_than_beam(CPU)


def test_score_is_a_lower_bound_of_the_loss_kernels_probability_sim(sim):
    K.check_lower_bound(CPU)


def test_text_score_paths_sim(sim):
    K.check_score_paths(CPU)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)


def test_convertor_nbest_sim(sim):
    K.check_convertor(CPU)


def test_text_accuracy_with_a_beam_sim(sim):
    K.check_update_scores(CPU)
