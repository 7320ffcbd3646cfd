"""`optimizer: sgd` / `optimizer: lars` on a real MI355X, through libccd_hip.so (run with -m gpu): kernels, the reference's recorded
iterations, model-level behaviour, the graphed step, and the train.py command line with both values in the Tiny YAML."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from backends import Backend
import optim_checks as oc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_moment_kernels(hip):
    oc.check_moment_kernels(hip.device)


def test_fixture_replay(hip, golden_dir):
    oc.check_fixture_replay(hip.device, golden_dir)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_optimizer_host_runs_ahead(hip, kind):
    oc.check_host_runs_ahead(hip.device, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_checkpoint_resume(hip, tmp_path, kind):
    oc.check_checkpoint_resume(hip.device, tmp_path, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_graphed_training_step_matches_eager(hip, kind):
    oc.check_graphed_step_matches_eager(hip.device, kind, steps=8)


def test_launch_step_makes_no_host_sync(hip):
    """The device half of a step (what a HIP graph captures) never waits for the GPU: torch raises on a synchronising call."""
    import model_checks as mc
    from ccd_amd import pretrain
    student, _ = mc.tiny_networks(hip.device)
    for kind in oc.KINDS:
        opt = pretrain.make_optimizer(student, clip_grad=3.0, name=kind)
        student.arena.grad.normal_()
        opt.step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.launch_step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(student.arena.flat).all())


@pytest.mark.parametrize("kind,port", [("sgd", "29643"), ("lars", "29644")])
def test_train_cli_runs_checkpoints_and_resumes(tmp_path, kind, port):
    """tests/test_train_cli_gpu.py's recipe with `optimizer: sgd` / `optimizer: lars` in the Tiny YAML."""
    src = open(os.path.join(REPO, "Dino", "configs", "CCD_pretrain_ViT_Tiny.yaml")).read()
    assert "optimizer: adamw" in src
    cfg = (src.replace("scheme: selfsupervised_kmeans", "scheme: synthetic\n  synthetic_samples: 256")
              .replace("imgnet_based: 1000000", "imgnet_based: 128")          # pseudo-epoch boundary every 2 iterations
              .replace("training: {epochs: 3,", "training: {epochs: 2,")
              .replace("show_iters: 200", "show_iters: 2")
              .replace("optimizer: adamw", f"optimizer: {kind}")
              .replace("name: pre_tiny_65536", f"name: cli_{kind}"))
    path = tmp_path / f"cli_{kind}.yaml"
    path.write_text(cfg)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=port, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    cmd = [sys.executable, os.path.join(REPO, "train.py"), "--config", str(path)]

    def finite_losses(out, at_least):
        vals = [float(v) for pair in re.findall(r"loss: (\S+) \((\S+)\)", out) for v in pair]
        assert len(vals) >= at_least and all(math.isfinite(v) for v in vals), out[-1500:]

    first = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert first.returncode == 0, first.stdout[-2000:] + first.stderr[-2000:]
    assert "Starting DINO training" in first.stdout and "Training time" in first.stdout
    finite_losses(first.stdout, 2)
    ckpt = tmp_path / "saved_models" / f"cli_{kind}" / "checkpoint.pth"
    assert ckpt.is_file(), first.stdout[-1500:]
    sd = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert {"student", "teacher", "optimizer", "epoch", "iteration", "dino_loss"} <= set(sd) and sd["iteration"] > 0
    state, groups = sd["optimizer"]["state"], sd["optimizer"]["param_groups"]
    assert state and {k for st in state.values() for k in st} == {oc.STATE_KEY[kind]}
    assert all(torch.isfinite(st[oc.STATE_KEY[kind]]).all() for st in state.values())
    assert len(groups) == 2 and groups[0]["momentum"] == 0.9 and groups[1]["weight_decay"] == 0.0
    if kind == "lars":
        assert set(groups[0]) == {"lr", "weight_decay", "momentum", "eta", "weight_decay_filter", "lars_adaptation_filter", "params"}
    else:
        assert {"lr", "weight_decay", "momentum", "dampening", "nesterov", "params"} <= set(groups[0])
    second = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert second.returncode == 0, second.stdout[-2000:] + second.stderr[-2000:]
    assert "Found checkpoint" in second.stdout and f"continue to train:{sd['iteration']}" in second.stdout
    assert "=> loaded 'optimizer' from checkpoint" in second.stdout and "failed to load" not in second.stdout
    finite_losses(second.stdout, 0)          # (a resumed run may end before its first print)
