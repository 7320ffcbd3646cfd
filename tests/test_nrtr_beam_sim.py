"""Beam search over the NRTR decoder (kernels/nrtr_beam.h: ccd_nrtr_beam_step, ccd_nrtr_beam_reorder) under the CPU SIMT executor
(tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on the MI355X in tests/test_nrtr_beam_gpu.py; gates:
tests/nrtr_beam_checks.py."""
import pytest
import torch

from backends import Backend
import nrtr_beam_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_paths_parents_and_scores_equal_the_oracle_sim(sim):
    K.check_oracle(CPU)


def test_finished_slots_compete_with_live_ones_sim(sim):
    K.check_end_heavy(CPU)


def test_width_one_is_the_arg_max_chain_sim(sim):
    K.check_width_one_is_greedy(CPU)


def test_a_wide_beam_equals_brute_force_sim(sim):
    K.check_exhaustive(CPU)


def test_equal_scores_rank_the_lower_flat_index_first_sim(sim):
    K.check_ties(CPU)


def test_cache_permutation_is_exact_in_place_sim(sim):
    K.check_reorder(CPU)


def test_argument_validation_sim(sim):
    K.check_arguments(CPU)


def test_convertor_nbest_and_path_scoring_sim(sim):
    K.check_convertor(CPU)
