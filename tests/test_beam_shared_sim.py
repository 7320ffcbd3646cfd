"""The code the two beam decoders share (kernels/beam_wave.h) under the CPU SIMT executor (tests/hipsim), through the wrappers of
ccd_amd.ops.  The same check runs on the MI355X in tests/test_beam_shared_gpu.py; what it compares: tests/beam_shared_checks.py."""
import pytest
import torch

from backends import Backend
import beam_shared_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_one_ctc_frame_equals_one_nrtr_step_sim(sim):
    K.check_one_frame_equals_one_step(CPU)
