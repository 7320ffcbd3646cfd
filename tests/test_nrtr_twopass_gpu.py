"""Two-pass decoding on a real MI355X, through libccd_hip.so (run with -m gpu): the checks of tests/test_nrtr_twopass_sim.py (gates:
tests/nrtr_twopass_checks.py) at the GPU's model shape, B = 4 and W = 8, and TextAccuracy.compute on its device path."""
import pytest
import torch

from backends import Backend
import nrtr_twopass_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_rows_equal_the_specification_and_words2rows(hip):
    K.check_rows(hip.device)


def test_select_equals_the_specification(hip):
    K.check_select(hip.device)


def test_ctc_score_paths_is_the_exact_word_probability(hip):
    K.check_ctc_score_paths(hip.device)


def test_entry_points_refuse_bad_arguments(hip):
    K.check_abi(hip.device)


def test_forward_twopass_ranks_the_proposals_by_the_two_exact_scores(hip):
    K.check_model(hip.device)


def test_forward_twopass_refusals(hip):
    K.check_model_refusals(hip.device)


def test_text_accuracy_scores_rank_zero_without_a_host_path(hip):
    K.check_text_accuracy(hip.device)
