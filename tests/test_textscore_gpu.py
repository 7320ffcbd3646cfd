"""The recognition-scoring kernels on a real MI355X, through libccd_hip.so (run with -m gpu): the checks of
tests/test_textscore_sim.py (gates: tests/textscore_checks.py), then what only the device can show - TextAccuracy.compute on a
recogniser takes the device path, gives the host path's totals and never synchronises while it scores - and the finetune CLI
evaluating the benchmarks of dataset.test.roots while it trains."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from backends import Backend
import textscore_checks as K
import textscore_np as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_fixture_pairs(hip, golden_dir):
    K.check_fixture(hip.device, golden_dir)


@pytest.mark.parametrize("T", [25, 40])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_adversarial_batches(hip, B, T):
    K.check_adversarial(hip.device, B, T)


def test_named_edge_cases(hip):
    K.check_named_edges(hip.device)


def test_strided_views(hip):
    K.check_strided_views(hip.device)


def test_repeatable_totals(hip):
    K.check_repeatable(hip.device)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


def test_update_scores_does_not_synchronise(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    conv, scores, gts = R.adversarial_case(67, 25)
    dev_scores = torch.from_numpy(scores).to(hip.device)
    torch.cuda.synchronize()
    metric = TextAccuracy()
    torch.cuda.set_sync_debug_mode("error")              # torch raises on a synchronising call - the first update included
    try:
        metric.update_scores(dev_scores[:30], gts[:30], conv)
        metric.update_scores(dev_scores[30:], gts[30:], conv)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = metric.result()
    R.check_result(res, dict(R.host_result(conv, [(scores, gts)]), time=res["time"]), 67)


def test_compute_takes_the_device_path_and_matches_the_host_path(hip, monkeypatch, golden_dir):
    from ccd_amd import finetune as ft
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy
    from ccd_amd.parallel import DataParallel
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2), hip.device, dropout=0.0)
    model.eval()
    # the seeded recogniser and batches behind tests/golden/eval_acc.npz (tests/test_eval_interop_gpu.py)
    g = np.load(os.path.join(golden_dir, "eval_acc.npz"))
    gen = torch.Generator().manual_seed(4321)
    images = torch.cat([torch.randn(6, 3, 32, 128, generator=gen) for _ in range(3)])
    gts = [str(w) for w in g["gt"]]
    loader = [(images[a:b], [tuple(gts[a:b])]) for a, b in ((0, 6), (6, 12), (12, 18))]
    wrapped = DataParallel(model)
    calls = []
    monkeypatch.setattr(TextAccuracy, "update_scores",
                        lambda self, *a, _f=TextAccuracy.update_scores, **k: calls.append("device") or _f(self, *a, **k))
    monkeypatch.setattr(TextAccuracy, "update", lambda self, *a, _f=TextAccuracy.update, **k: calls.append("host") or _f(self, *a, **k))
    device_res = TextAccuracy().compute(wrapped, loader)
    assert calls == ["device"] * 3
    monkeypatch.setattr(AttnConvertor, "score_table", lambda self: None)
    host_res = TextAccuracy().compute(wrapped, loader)
    assert calls == ["device"] * 3 + ["host"] * 3
    assert device_res["words"] == 18.0 and device_res["time"] > 0 and host_res["time"] > 0
    R.check_result(device_res, dict(host_res, time=device_res["time"]), 18)
    assert device_res["ted"] == float(g["values"][2])                          # the reference's own run of these batches
    with pytest.raises(NotImplementedError):                                   # case_sensitive: the host path, which raises as before
        TextAccuracy(case_sensitive=True).compute(wrapped, loader)


def test_finetune_cli_evaluates_benchmarks_while_training(tmp_path):
    """train_finetune.py with dataset.test.roots set: every eval_iters iterations the report of test.py is appended to
    log_all_evaluation.txt and the best total keeps best_accuracy.pth; the one-batch accuracy line is still logged."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    root = os.path.join(REPO, "tests", "golden", "lmdb_handmade")
    src = open(os.path.join(REPO, "Dino", "configs", "CCD_vision_model_ARD.yaml")).read()
    cfg = (src.replace("scheme: supervised", "scheme: synthetic\n  synthetic_samples: 96")
              .replace("train: {roots: [], batch_size: 288}", "train: {roots: [], batch_size: 32}")
              .replace("test: {roots: [], batch_size: 288}", f"test: {{roots: ['{root}', '{root}'], batch_size: 2}}")
              .replace("training: {epochs: 35,", "training: {epochs: 2,")
              .replace("show_iters: 1000, eval_iters: 1000, save_iters: 100000", "show_iters: 2, eval_iters: 4, save_iters: 100")
              .replace("arch: 'vit_small'", "arch: 'vit_tiny'")
              .replace("num_workers: 8", "num_workers: 0")
              .replace("name: finetune_small_65536", "name: ft_eval"))
    assert cfg.count(root) == 2 and "eval_iters: 4" in cfg and "batch_size: 32" in cfg
    (tmp_path / "ft.yaml").write_text(cfg)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29643", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    run = subprocess.run([sys.executable, os.path.join(REPO, "train_finetune.py"), "--config", str(tmp_path / "ft.yaml")], cwd=tmp_path,
                         env=env, capture_output=True, text=True, timeout=600)
    log = run.stdout + run.stderr
    assert run.returncode == 0, log[-3000:]
    out = tmp_path / "saved_models" / "ft_eval"
    text = (out / "log_all_evaluation.txt").read_text()
    blocks = text.split("-" * 80 + "\n")
    assert blocks[0] == "" and len(blocks) == 3, text
    for block, iteration in zip(blocks[1:], (0, 4)):
        lines = block.splitlines()
        assert lines[0] == f"iteration: {iteration} ", block
        assert [ln.split(" --> ")[0] for ln in lines[1:3]] == ["dataset: IIIT5k_3000", "dataset: SVT"], block
        assert all(" --> word_num: 3.0 --> accuracy: " in ln for ln in lines[1:3]), block
        assert lines[3].startswith("total_accuracy: ") and len(lines) == 4, block
    sd = torch.load(out / "best_accuracy.pth", map_location="cpu", weights_only=False)
    assert set(sd) == {"net", "optimizer", "iteration"} and sd["iteration"] in (0, 4)
    assert all(k.startswith("module.") for k in sd["net"])
    assert "word accuracy" in log and "total_accuracy: " in log and "eval model" in log
