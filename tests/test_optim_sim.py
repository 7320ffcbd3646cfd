"""`optimizer: sgd` / `optimizer: lars` under the CPU SIMT executor (tests/hipsim): the three-sum sweep and the two update kernels on
odd sizes, the reference's recorded iterations through FusedClipSGD / FusedClipLARS, and the model-level behaviour (every step sees
its own lr / wd, checkpoint resume, the graphed step's bookkeeping) on the tiny networks."""
import pytest

from backends import Backend
import optim_checks as oc


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_moment_kernels_sim(sim):
    oc.check_moment_kernels(sim.device)


def test_fixture_replay_sim(sim, golden_dir):
    oc.check_fixture_replay(sim.device, golden_dir)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_optimizer_steps_sim(sim, kind):
    oc.check_host_runs_ahead(sim.device, kind, steps=3)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_checkpoint_resume_sim(sim, tmp_path, kind):
    oc.check_checkpoint_resume(sim.device, tmp_path, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_graphed_training_step_bookkeeping_sim(sim, monkeypatch, kind):
    """There is no HIP graph on the executor: `_record` is replaced by a stand-in whose replay() re-issues the captured launches
    with the launch-time constants of the capture (as tests/test_model_sim.py does for AdamW).  lr / wd / the frozen last layer
    must then reach the SGD / LARS kernel through the staged table for the run to agree with the eager one."""
    from ccd_amd import engine, pretrain

    def record(self, body):
        seeds = engine._DROPPATH_SEED
        at_capture, d_seed = seeds["calls"], seeds["device"]

        class Replay:
            def replay(_):
                now = seeds["calls"]
                seeds["calls"] = at_capture
                engine.set_device_droppath_seed(d_seed)
                try:
                    body()
                finally:
                    engine.set_device_droppath_seed(None)
                    seeds["calls"] = now
        return Replay(), 1

    monkeypatch.setattr(pretrain.GraphedTrainingStep, "_record", record)
    oc.check_graphed_step_matches_eager(sim.device, kind, steps=4, B=1, drop_path_rate=0.5)


def test_abi_contract_sim(sim):
    import torch
    from ccd_amd import _lib
    lib = _lib.get()
    t = torch.zeros(64)
    i32, i64 = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    P = _lib.ptr
    # a missing pointer or an empty chunk table: CCD_EINVAL, nothing launched; the mirror alone is optional
    assert lib.ccd_seg_moments(P(t), None, P(i32), P(i64), P(i32), 1, P(t), 0) == -1
    assert lib.ccd_seg_moments(P(t), P(t), P(i32), P(i64), P(i32), 0, P(t), 0) == -1
    assert lib.ccd_sgd_momentum(P(t), P(t), None, None, P(i32), P(i64), P(i32), 1, P(t), P(t), 3.0, 0.9, 0) == -1
    assert lib.ccd_lars(P(t), P(t), P(t), None, P(i32), P(i64), P(i32), 1, P(t), None, 3.0, 0.9, 0.001, 0) == -1
    assert lib.ccd_abi_version() >= 16
