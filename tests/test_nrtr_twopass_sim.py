"""Two-pass decoding (kernels/nrtr_twopass.h: ccd_nrtr_twopass_rows, ccd_nrtr_twopass_select; ops.ctc_score_paths;
DINO_Finetune.forward_twopass) under the CPU SIMT executor (tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on
the MI355X in tests/test_nrtr_twopass_gpu.py; gates: tests/nrtr_twopass_checks.py."""
import pytest
import torch

from backends import Backend
import nrtr_twopass_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_rows_equal_the_specification_and_words2rows_sim(sim):
    K.check_rows(CPU)


def test_select_equals_the_specification_sim(sim):
    K.check_select(CPU)


def test_ctc_score_paths_is_the_exact_word_probability_sim(sim):
    K.check_ctc_score_paths(CPU)


def test_entry_points_refuse_bad_arguments_sim(sim):
    K.check_abi(CPU)


def test_forward_twopass_ranks_the_proposals_by_the_two_exact_scores_sim(sim):
    K.check_model(CPU, B=2, W=4)


def test_forward_twopass_refusals_sim(sim):
    K.check_model_refusals(CPU)


def test_text_accuracy_scores_rank_zero_sim(sim):
    K.check_text_accuracy(CPU, B=2, W=4, batches=2)
