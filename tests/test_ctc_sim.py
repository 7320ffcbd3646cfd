"""The CTC head's kernels (kernels/ctc.h: frame pooling, CTC loss forward / backward, greedy decoding; ccd_text_score_ctc) under the
CPU SIMT executor (tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on the MI355X in tests/test_ctc_gpu.py;
gates: tests/ctc_checks.py."""
import pytest
import torch

from backends import Backend
import ctc_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_loss_named_and_random_cases_sim(sim):
    K.check_loss(CPU)


def test_loss_upstream_sim(sim):
    K.check_upstream(CPU)


def test_loss_module_sim(sim):
    K.check_loss_module(CPU)


def test_pool_sim(sim):
    K.check_pool(CPU)


def test_greedy_sim(sim):
    K.check_greedy(CPU)


def test_score_sim(sim):
    K.check_score(CPU)


def test_abi_contract_sim(sim):
    K.check_abi_contract(CPU)


def test_model_loss_parity_sim(sim):
    K.check_model_parity(CPU)


def test_model_gradients_sim(sim):
    """Finite, non-zero gradients down to the first block and a falling loss (a few iterations: the executor is slow)."""
    K.check_model_trains(CPU, iterations=3)

