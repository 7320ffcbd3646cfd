"""Text super-resolution finetuning on a real MI355X (run with -m gpu): the checks of test_superres_sim.py through libccd_hip.so."""
import pytest
import torch

from backends import Backend
import kernel_checks as kc
import superres_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


@pytest.mark.parametrize("d_loss", [1.0, 0.5])
@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
@pytest.mark.parametrize("shape", C.SHAPES)
def test_loss_matches_specification(hip, shape, pname, d_loss):
    C.check_loss(hip.device, shape, "random", pname, d_loss)


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
def test_loss_identical_zero_and_constant_images(hip, pname):
    C.check_loss(hip.device, C.SHAPES[0], "special", pname, d_loss=0.5)


def test_loss_bit_repeatable(hip):
    C.check_loss_repeatable(hip.device)


def test_loss_empty_batch(hip):
    C.check_loss_empty(hip.device)


def test_loss_autograd(hip):
    C.check_loss_autograd(hip.device)


def test_abi_error_codes(hip):
    C.check_loss_abi(hip.device)


@pytest.mark.parametrize("N", [1, 3])
def test_upsample_matches_specification(hip, N):
    C.check_upsample(hip.device, N)


@pytest.mark.parametrize("images,train", [(1, True), (2, True), (1, False), (2, False)])
def test_sr_head(hip, images, train):
    C.check_sr_head(hip.device, images=images, train=train)


def test_seghead_two_class_path_untouched(hip):
    kc.check_seghead(hip.device, images=1, E=64)


def test_model(hip):
    C.check_model(hip.device)


def test_model_stops_at_last_tap(hip):
    C.check_model_stops_at_last_tap(hip.device)
