"""The CTC head on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of tests/test_ctc_sim.py (gates:
tests/ctc_checks.py), then the model - loss parity with a CPU restatement (the oracle's encoder, a torch head, F.ctc_loss), finite
non-zero gradients, a falling loss, no host synchronisation - and the finetune / test CLIs with the new YAML."""
import os
import subprocess
import sys

import pytest
import torch

from backends import Backend
import ctc_checks as K
import ctc_np as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = K.WORDS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_loss_named_and_random_cases(hip):
    K.check_loss(hip.device)


def test_loss_upstream(hip):
    K.check_upstream(hip.device)


def test_loss_module(hip):
    K.check_loss_module(hip.device)


def test_pool(hip):
    K.check_pool(hip.device)


def test_greedy(hip):
    K.check_greedy(hip.device)


def test_score(hip):
    K.check_score(hip.device)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def test_loss_parity_two_adamw_iterations(hip):
    K.check_model_parity(hip.device)


def test_gradients_finite_and_loss_decreases(hip):
    K.check_model_trains(hip.device)


def test_head_and_scoring_do_not_synchronise(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(7)
    model = K.ctc_model(hip.device)
    targets = model.label_convertor.str2tensor(WORDS).to(hip.device)
    tokens = torch.randn(3, 256, 192, device=hip.device).to(torch.bfloat16).requires_grad_(True)
    logits = model.decoder.forward_train(tokens)                               # warm-up: lazily built operands
    model.loss(logits, {"padded_targets": targets}).backward()
    model.eval()
    with torch.no_grad():
        probs = model.decoder.forward_test(tokens.detach())
    model.train()
    metric = TextAccuracy()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = model.decoder.forward_train(tokens)
        loss = model.loss(logits, {"padded_targets": targets})
        loss.backward()
        metric.update_scores(probs, WORDS, model.label_convertor)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and torch.isfinite(tokens.grad.float()).all() and float(tokens.grad.float().abs().max()) > 0
    res = metric.result()
    host = TextAccuracy()
    idx, _ = model.label_convertor.tensor2idx(probs)
    host.update(WORDS, model.label_convertor.idx2str(idx))
    want = host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12


def test_finetune_and_test_cli_with_the_ctc_yaml(tmp_path):
    """train_finetune.py on the new YAML (vit_tiny, synthetic data): trains, evaluates tests/golden/lmdb_handmade, saves
    module.decoder.fc.weight; test.py reads the checkpoint back."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    root = os.path.join(REPO, "tests", "golden", "lmdb_handmade")
    src = open(os.path.join(REPO, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).read()
    cfg = (src.replace("scheme: supervised", "scheme: synthetic\n  synthetic_samples: 96")
              .replace("train: {roots: [], batch_size: 288}", "train: {roots: [], batch_size: 32}")
              .replace("test: {roots: [], batch_size: 288}", f"test: {{roots: ['{root}', '{root}'], batch_size: 2}}")
              .replace("training: {epochs: 35,", "training: {epochs: 2,")
              .replace("show_iters: 1000, eval_iters: 1000, save_iters: 100000", "show_iters: 2, eval_iters: 4, save_iters: 4")
              .replace("arch: 'vit_small'", "arch: 'vit_tiny'")
              .replace("num_workers: 8", "num_workers: 0")
              .replace("name: finetune_small_65536_ctc", "name: ft_ctc"))
    assert cfg.count(root) == 2 and "eval_iters: 4" in cfg and "batch_size: 32" in cfg and "type: 'CTCDecoder'" in cfg
    (tmp_path / "ft.yaml").write_text(cfg)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29644", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    run = subprocess.run([sys.executable, os.path.join(REPO, "train_finetune.py"), "--config", str(tmp_path / "ft.yaml")], cwd=tmp_path,
                         env=env, capture_output=True, text=True, timeout=600)
    log = run.stdout + run.stderr
    assert run.returncode == 0, log[-3000:]
    assert "train loss" in log and "word accuracy" in log and "total_accuracy: " in log
    out = tmp_path / "saved_models" / "ft_ctc"
    text = (out / "log_all_evaluation.txt").read_text()
    assert text.count("dataset: IIIT5k_3000 --> word_num: 3.0 --> accuracy: ") == 2, text
    ck = out / "4.pth"
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert set(sd) == {"net", "optimizer", "iteration"} and sd["iteration"] == 4
    heads = sorted(k for k in sd["net"] if not k.startswith("module.backbone."))
    assert heads == ["module.decoder.fc.bias", "module.decoder.fc.weight"] and tuple(sd["net"]["module.decoder.fc.weight"].shape) == (92, 192)
    back = subprocess.run([sys.executable, os.path.join(REPO, "test.py"), "--config", str(tmp_path / "ft.yaml"), "--checkpoint", str(ck)],
                          cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    log = back.stdout + back.stderr
    assert back.returncode == 0, log[-3000:]
    assert "Read vision model from" in log and "dataset: SVT --> word_num: 3.0 --> accuracy: " in log and "total_accuracy: " in log
