"""The parallel attention head's kernels (kernels/posattn.h: ccd_posattn_fwd / _bwd / _fold) under the CPU SIMT executor
(tests/hipsim), through the wrappers of ccd_amd.ops, and ParallelAttnDecoder / DINO_Finetune on top of them.  The same checks run on
the MI355X in tests/test_parallel_attn_gpu.py; gates: tests/parallel_attn_checks.py."""
import pytest
import torch

from backends import Backend
import parallel_attn_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


@pytest.mark.parametrize("N,E,T", [(1, 64, 25), (1, 64, 32), (1, 64, 1), (3, 192, 25)])
def test_kernels_equal_the_specification_sim(sim, N, E, T):
    K.check_kernels(CPU, N, E, T)


def test_kernels_at_the_default_scale_sim(sim):
    K.check_default_scale(CPU)


def test_saturated_tanh_and_one_hot_maps_sim(sim):
    K.check_saturation(CPU)


def test_two_runs_give_the_same_bits_sim(sim):
    K.check_repeatable(CPU)


def test_unsupported_shapes_are_refused_before_a_launch_sim(sim):
    K.check_abi(CPU)


def test_module_gradients_equal_torch_autograd_sim(sim):
    K.check_module_autograd(CPU)


def test_module_under_tf_loss_sim(sim):
    K.check_module_tf_loss(CPU)
