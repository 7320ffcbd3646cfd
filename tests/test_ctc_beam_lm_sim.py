"""CTC prefix beam search fused with a character n-gram language model (kernels/ctc_beam.h: ctc_beam_kernel<true>,
ccd_ctc_beam_search_lm) under the CPU SIMT executor (tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on the
MI355X in tests/test_ctc_beam_lm_gpu.py; gates: tests/ctc_beam_lm_checks.py."""
import pytest
import torch

from backends import Backend
import ctc_beam_lm_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_exhaustive_shapes_equal_brute_force_plus_the_word_term_sim(sim):
    K.check_exhaustive(CPU)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_paths_and_scores_equal_the_oracle_sim(sim, seed):
    K.check_oracle(CPU, (seed,))


def test_longest_frames_classes_and_order_sim(sim):
    K.check_oracle_long(CPU)


def test_weight_zero_is_the_plain_beam_byte_for_byte_sim(sim):
    K.check_weight_zero(CPU)


def test_a_merge_carries_the_absorbed_candidates_term_sim(sim):
    K.check_merge(CPU)


def test_end_of_word_reranks_and_empties_slots_sim(sim):
    K.check_eos(CPU)


def test_a_hard_mask_is_a_character_set_sim(sim):
    K.check_charset(CPU)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)


def test_convertor_nbest_with_a_language_model_sim(sim):
    K.check_convertor(CPU)


def test_text_accuracy_with_a_language_model_sim(sim):
    K.check_update_scores(CPU)
