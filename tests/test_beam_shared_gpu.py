"""The code the two beam decoders share (kernels/beam_wave.h) on a real MI355X, through libccd_hip.so (run with -m gpu): the check of
tests/test_beam_shared_sim.py (what it compares: tests/beam_shared_checks.py)."""
import pytest
import torch

from backends import Backend
import beam_shared_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_one_ctc_frame_equals_one_nrtr_step(hip):
    K.check_one_frame_equals_one_step(hip.device)
