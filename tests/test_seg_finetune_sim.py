"""Text segmentation finetuning under the CPU SIMT executor (tests/hipsim): the fused supervised loss kernels against the numpy
restatement, the eval-mode segmentation head, DINO_Segment on a three-block backbone.  The same checks run on the GPU in
test_seg_finetune_gpu.py."""
import pytest

from backends import Backend
import kernel_checks as kc
import seg_finetune_checks as C


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
@pytest.mark.parametrize("shape", C.SHAPES)
def test_loss_matches_specification_sim(sim, shape, pname):
    C.check_loss(sim.device, shape, "random", pname)


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
def test_loss_all_ignored_all_text_all_background_images_sim(sim, pname):
    C.check_loss(sim.device, C.SHAPES[0], "special", pname, d_loss=0.5)


def test_loss_more_images_than_one_finish_chunk_sim(sim):
    """300 images of 4 x 8: the finishing workgroup takes the rows 256 images at a time."""
    C.check_loss(sim.device, (300, 4, 8), "random", "full")


def test_loss_channel_stride_sim(sim):
    C.check_loss_channel_stride(sim.device)


def test_loss_bit_repeatable_sim(sim):
    C.check_loss_repeatable(sim.device)


def test_loss_batch_of_ignored_pixels_sim(sim):
    C.check_loss_all_ignored(sim.device)


def test_loss_autograd_sim(sim):
    C.check_loss_autograd(sim.device)


def test_loss_abi_error_codes_sim(sim):
    C.check_loss_abi(sim.device)


@pytest.mark.parametrize("images,train_flag", [(1, False), (2, True)])
def test_seghead_eval_mode_sim(sim, images, train_flag):
    C.check_seghead_eval(sim.device, images=images, train_flag=train_flag)


def test_seghead_train_mode_untouched_sim(sim):
    kc.check_seghead(sim.device, images=1, E=64)


def test_model_sim(sim):
    C.check_model(sim.device)


def test_model_stops_at_last_tap_sim(sim):
    C.check_model_stops_at_last_tap(sim.device)
