"""The recognition-scoring kernels (kernels/textscore.h: ccd_text_score, ccd_text_accumulate) under the CPU SIMT executor
(tests/hipsim), through ops.text_score and TextAccuracy.update_scores: the pairs behind eval_acc.npz against the reference's
recorded values, adversarial batches against TextAccuracy.update record by record, strided views, bit-equal repeats and the
ABI's error codes.  The same checks run on the MI355X in tests/test_textscore_gpu.py; gates: tests/textscore_checks.py."""
import pytest
import torch

from backends import Backend
import textscore_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_fixture_pairs_sim(sim, golden_dir):
    K.check_fixture(CPU, golden_dir)


@pytest.mark.parametrize("T", [25, 40])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_adversarial_batches_sim(sim, B, T):
    K.check_adversarial(CPU, B, T)


def test_named_edge_cases_sim(sim):
    K.check_named_edges(CPU)


def test_strided_views_sim(sim):
    K.check_strided_views(CPU)


def test_repeatable_totals_sim(sim):
    K.check_repeatable(CPU)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)
