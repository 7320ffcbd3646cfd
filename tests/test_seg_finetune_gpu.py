"""Text segmentation finetuning on a real MI355X (run with -m gpu): the checks of test_seg_finetune_sim.py through libccd_hip.so."""
import pytest
import torch

from backends import Backend
import kernel_checks as kc
import seg_finetune_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
@pytest.mark.parametrize("shape", C.SHAPES)
def test_loss_matches_specification(hip, shape, pname):
    C.check_loss(hip.device, shape, "random", pname)


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
def test_loss_all_ignored_all_text_all_background_images(hip, pname):
    C.check_loss(hip.device, C.SHAPES[0], "special", pname, d_loss=0.5)


def test_loss_more_images_than_one_finish_chunk(hip):
    """300 images of 4 x 8: the finishing workgroup takes the rows 256 images at a time."""
    C.check_loss(hip.device, (300, 4, 8), "random", "full")


def test_loss_channel_stride(hip):
    C.check_loss_channel_stride(hip.device)


def test_loss_bit_repeatable(hip):
    C.check_loss_repeatable(hip.device)


def test_loss_batch_of_ignored_pixels(hip):
    C.check_loss_all_ignored(hip.device)


def test_loss_autograd(hip):
    C.check_loss_autograd(hip.device)


def test_loss_abi_error_codes(hip):
    C.check_loss_abi(hip.device)


@pytest.mark.parametrize("images,train_flag", [(1, False), (2, True)])
def test_seghead_eval_mode(hip, images, train_flag):
    C.check_seghead_eval(hip.device, images=images, train_flag=train_flag)


def test_seghead_train_mode_untouched(hip):
    kc.check_seghead(hip.device, images=1, E=64)


def test_model(hip):
    C.check_model(hip.device)


def test_model_stops_at_last_tap(hip):
    C.check_model_stops_at_last_tap(hip.device)
