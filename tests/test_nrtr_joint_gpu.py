"""Joint CTC / attention decoding on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of
tests/test_nrtr_joint_sim.py (gates: tests/nrtr_joint_checks.py), then the hybrid model - loss and gradients of the auxiliary CTC
head, forward_beam at weight 0 against the plain beam, the joint scores against the project's two exact scorers, the HIP graph."""
import pytest
import torch

from backends import Backend
import nrtr_joint_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_paths_parents_scores_and_prefix_states_equal_the_oracle(hip):
    K.check_oracle(hip.device)


def test_weight_zero_is_the_plain_beam_step_bit_for_bit(hip):
    K.check_weight_zero(hip.device)


def test_ties_resolve_by_flat_index(hip):
    K.check_ties(hip.device)


def test_argument_validation(hip):
    K.check_arguments(hip.device)


def test_hybrid_loss_is_the_weighted_sum_and_so_are_its_gradients(hip):
    K.check_hybrid_loss_and_gradients(hip.device)


def test_forward_beam_at_joint_weight_zero_is_the_plain_beam(hip):
    K.check_joint_weight_zero_is_the_plain_beam(hip.device)


def test_joint_scores_are_the_two_exact_scorers_and_the_graph_replays(hip):
    K.check_joint_scores_are_the_two_exact_scorers(hip.device)
