"""CTC forced alignment on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of tests/test_ctc_align_sim.py
(gates: tests/ctc_align_checks.py) on more seeded rows, then the model - tensor2align does not synchronise, forward_chars agrees with
the oracle on the same probabilities, test.py --alignments writes what TextAccuracy scored."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from backends import Backend
import ctc_align_checks as K
import ctc_align_np as A
import ctc_checks as C

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = C.WORDS
GROUPS = 24


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_seeded_rows_equal_the_oracle(hip):
    K.check_seeded(hip.device, GROUPS)


def test_limits_of_frames_classes_and_labels(hip):
    K.check_limits(hip.device)


def test_masked_frames_and_classes(hip):
    K.check_masks(hip.device)


def test_uniform_frames_follow_the_tie_rule(hip):
    K.check_uniform(hip.device)


def test_rows_equal_replicated_scores(hip):
    K.check_rows(hip.device)


def test_score_is_below_the_loss_kernels_sum(hip):
    K.check_against_loss(hip.device, GROUPS)


def test_a_single_alignment_scores_the_bits_of_the_lexicon_kernel(hip):
    K.check_single_alignment_bits(hip.device)


def test_the_greedy_word_aligns_on_the_arg_max_path(hip):
    K.check_against_greedy(hip.device, GROUPS)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


def test_convertor_alignments(hip):
    K.check_convertor(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def _model(device, **decoder):
    from ccd_amd import finetune as ft
    from model_checks import _register_test_arch
    _register_test_arch()
    cfg = ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    for key, value in decoder.items():
        setattr(cfg, f"decoder_{key}", value)
    return ft.build_model(cfg, device, dropout=0.0).eval()


def test_tensor2align_does_not_synchronise(hip):
    torch.manual_seed(7)
    tokens = torch.randn(3, 256, 192, device=hip.device).to(torch.bfloat16)
    for decoder in ({}, {"beam_width": 4}):
        model = _model(hip.device, **decoder)
        conv = model.label_convertor
        with torch.no_grad():
            probs = model.decoder.forward_test(tokens)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = conv.tensor2align(probs, nbest=2 if decoder else 1)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        # (a word of more than 31 characters - an untrained head decodes such - has no row: it is padding, and checked as padding)
        assert K.check_result(res, probs.float().cpu().numpy()) == int((res["rows"] >= 0).sum()) >= 1


def test_forward_chars_agrees_with_the_oracle(hip):
    torch.manual_seed(8)
    model = _model(hip.device)
    img = torch.randn(3, 3, 32, 128, generator=torch.Generator().manual_seed(4)).to(hip.device)
    with torch.no_grad():
        probs = model(img, text=None, return_loss=False, test_speed=False).float().cpu().numpy()
    res = model.forward_chars(img)
    assert K.check_result(res, probs) == int((res["rows"] >= 0).sum()) >= 1 and tuple(res["frame_char"].shape) == (3, probs.shape[1])
    forced = model.forward_chars(img, words=list(WORDS))
    assert K.check_result(forced, probs) == 3
    assert K._words_of(model.label_convertor, forced) == [w[:25] for w in WORDS]
    from ccd_amd import finetune as ft
    nrtr = ft.build_model(ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0), hip.device, dropout=0.0).eval()
    with pytest.raises(NotImplementedError, match="CTC head"):
        nrtr.forward_chars(img)


def test_alignments_of_test_py_are_what_text_accuracy_scored(hip, tmp_path):
    from ccd_amd.metric.eval_acc import TextAccuracy
    spec = importlib.util.spec_from_file_location("ccd_test_script", os.path.join(REPO, "test.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    torch.manual_seed(9)
    model = _model(hip.device)
    gen = torch.Generator().manual_seed(5)
    images = [torch.randn(3, 3, 32, 128, generator=gen) for _ in range(2)]
    conv = model.label_convertor
    with torch.no_grad():
        classes = [conv.tensor2idx(model(img.to(hip.device), text=None, return_loss=False, test_speed=False))[0] for img in images]
    greedy = [conv.idx2str(c) for c in classes]
    truth = [greedy[0], list(WORDS)]                                           # the first batch right, the second as it comes
    loader = [(img, (gt,)) for img, gt in zip(images, truth)]
    config = types.SimpleNamespace(dataset_charset_path=None, dataset_eval_case_sensitive=False, dataset_image_width=128)
    plain_report, plain = script.evaluate(model, [loader], config, names=["synthetic"])
    with open(tmp_path / "align.jsonl", "w", encoding="utf-8") as f:
        report, results = script.evaluate(model, [loader], config, names=["synthetic"], alignments=f)
    assert report == plain_report and all(results[0][k] == plain[0][k] for k in ("ccr", "cwr", "ted", "ned", "ted/w", "words"))
    lines = [json.loads(line) for line in open(tmp_path / "align.jsonl", encoding="utf-8")]
    assert len(lines) == 6 and [r["index"] for r in lines] == list(range(6)) and [r["gt"] for r in lines] == truth[0] + truth[1]
    # a word of more than 31 classes (an untrained head decodes such) cannot be aligned: its line says null, every other line the word
    decoded = greedy[0] + greedy[1]
    lengths = [len(c) for batch in classes for c in batch]
    assert [r["pred"] for r in lines] == [w if n <= 31 else None for w, n in zip(decoded, lengths)] and min(lengths) <= 31
    host = TextAccuracy()
    host.update([r["gt"] for r in lines], decoded)
    want = host.result()
    assert all(results[0][k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(results[0]["ned"] - want["ned"]) < 1e-12
    assert results[0]["cwr"] >= 0.5
    lines = [r for r in lines if r["pred"] is not None]
    for r in lines:
        assert "".join(c["char"] for c in r["chars"]) == r["pred"] and np.isfinite(r["log_prob"])
        assert all(0.0 <= c["x0"] < c["x1"] <= 128.0 and c["first"] <= c["last"] and 0.0 < c["conf"] <= 1.0 for c in r["chars"])
