"""The parallel attention head on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of
tests/test_parallel_attn_sim.py (gates: tests/parallel_attn_checks.py) plus the vit_small width once, then ParallelAttnDecoder and
DINO_Finetune on top of the kernels."""
import pytest
import torch

from backends import Backend
import parallel_attn_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


@pytest.mark.parametrize("N,E,T", [(1, 64, 25), (1, 64, 32), (1, 64, 1), (3, 192, 25), (2, 384, 25)])
def test_kernels_equal_the_specification(hip, N, E, T):
    K.check_kernels(hip.device, N, E, T)


def test_kernels_at_the_default_scale(hip):
    K.check_default_scale(hip.device)


def test_saturated_tanh_and_one_hot_maps(hip):
    K.check_saturation(hip.device)


def test_two_runs_give_the_same_bits(hip):
    K.check_repeatable(hip.device)


def test_unsupported_shapes_are_refused_before_a_launch(hip):
    K.check_abi(hip.device)


def test_module_gradients_equal_torch_autograd(hip):
    K.check_module_autograd(hip.device)


def test_module_under_tf_loss(hip):
    K.check_module_tf_loss(hip.device)


def test_model_trains_and_decodes(hip):
    K.check_model(hip.device)
