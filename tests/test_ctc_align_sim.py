"""CTC forced alignment (kernels/ctc_align.h: ccd_ctc_align) under the CPU SIMT executor (tests/hipsim), through the wrappers of
ccd_amd.ops.  The same checks run on the MI355X in tests/test_ctc_align_gpu.py; gates: tests/ctc_align_checks.py."""
import pytest
import torch

from backends import Backend
import ctc_align_checks as K

CPU = torch.device("cpu")
GROUPS = 6


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_seeded_rows_equal_the_oracle_sim(sim):
    K.check_seeded(CPU, GROUPS)


def test_limits_of_frames_classes_and_labels_sim(sim):
    K.check_limits(CPU)


def test_masked_frames_and_classes_sim(sim):
    K.check_masks(CPU)


def test_uniform_frames_follow_the_tie_rule_sim(sim):
    K.check_uniform(CPU)


def test_rows_equal_replicated_scores_sim(sim):
    K.check_rows(CPU)


def test_score_is_below_the_loss_kernels_sum_sim(sim):
    K.check_against_loss(CPU, GROUPS)


def test_a_single_alignment_scores_the_bits_of_the_lexicon_kernel_sim(sim):
    K.check_single_alignment_bits(CPU)


def test_the_greedy_word_aligns_on_the_arg_max_path_sim(sim):
    K.check_against_greedy(CPU, GROUPS)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)


def test_convertor_alignments_sim(sim):
    K.check_convertor(CPU)
