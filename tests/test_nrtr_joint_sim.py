"""Joint CTC / attention decoding (kernels/nrtr_joint.h: ccd_nrtr_joint_begin, ccd_nrtr_beam_step_joint) under the CPU SIMT executor
(tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on the MI355X in tests/test_nrtr_joint_gpu.py; gates:
tests/nrtr_joint_checks.py."""
import pytest
import torch

from backends import Backend
import nrtr_joint_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_paths_parents_scores_and_prefix_states_equal_the_oracle_sim(sim):
    K.check_oracle(CPU)


def test_weight_zero_is_the_plain_beam_step_bit_for_bit_sim(sim):
    K.check_weight_zero(CPU)


def test_ties_resolve_by_flat_index_sim(sim):
    K.check_ties(CPU)


def test_argument_validation_sim(sim):
    K.check_arguments(CPU)


def test_hybrid_loss_is_the_weighted_sum_and_so_are_its_gradients_sim(sim):
    K.check_hybrid_loss_and_gradients(CPU)


def test_forward_beam_at_joint_weight_zero_is_the_plain_beam_sim(sim):
    K.check_joint_weight_zero_is_the_plain_beam(CPU, B=2, W=3)


def test_joint_scores_are_the_two_exact_scorers_sim(sim):
    K.check_joint_scores_are_the_two_exact_scorers(CPU, B=2, W=4)
