"""Text super-resolution finetuning under the CPU SIMT executor (tests/hipsim): the fused loss and upsample kernels against the
numpy restatement, the image head, DINO_SuperRes on a three-block backbone.  The same checks run on the GPU in
test_superres_gpu.py."""
import pytest

from backends import Backend
import kernel_checks as kc
import superres_checks as C


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


@pytest.mark.parametrize("d_loss", [1.0, 0.5])
@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
@pytest.mark.parametrize("shape", C.SHAPES)
def test_loss_matches_specification_sim(sim, shape, pname, d_loss):
    C.check_loss(sim.device, shape, "random", pname, d_loss)


@pytest.mark.parametrize("pname", list(C.PARAM_SETS))
def test_loss_identical_zero_and_constant_images_sim(sim, pname):
    C.check_loss(sim.device, C.SHAPES[0], "special", pname, d_loss=0.5)


def test_loss_bit_repeatable_sim(sim):
    C.check_loss_repeatable(sim.device)


def test_loss_empty_batch_sim(sim):
    C.check_loss_empty(sim.device)


def test_loss_autograd_sim(sim):
    C.check_loss_autograd(sim.device)


def test_abi_error_codes_sim(sim):
    C.check_loss_abi(sim.device)


@pytest.mark.parametrize("N", [1, 3])
def test_upsample_matches_specification_sim(sim, N):
    C.check_upsample(sim.device, N)


@pytest.mark.parametrize("images,train", [(1, True), (2, True), (1, False), (2, False)])
def test_sr_head_sim(sim, images, train):
    C.check_sr_head(sim.device, images=images, train=train)


def test_seghead_two_class_path_untouched_sim(sim):
    kc.check_seghead(sim.device, images=1, E=64)


def test_model_sim(sim):
    C.check_model(sim.device)


def test_model_stops_at_last_tap_sim(sim):
    C.check_model_stops_at_last_tap(sim.device)
