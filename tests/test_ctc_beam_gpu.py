"""CTC prefix beam search on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of tests/test_ctc_beam_sim.py
(gates: tests/ctc_beam_checks.py), then the model - TextAccuracy with a beam convertor does not synchronise and scores what the
oracle decodes from the same probabilities; beam_width = 0 is today's greedy path, bit for bit."""
import numpy as np
import pytest
import torch

from backends import Backend
import ctc_beam_checks as K
import ctc_beam_np as R
import ctc_checks as C

pytestmark = pytest.mark.gpu
WORDS = C.WORDS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_exhaustive_shapes_equal_brute_force(hip):
    K.check_exhaustive(hip.device)


def test_paths_and_scores_equal_the_oracle(hip):
    K.check_oracle(hip.device)


def test_longest_frames_and_classes(hip):
    K.check_oracle_long(hip.device)


def test_equal_scores_rank_the_lower_class_first(hip):
    K.check_ties(hip.device)


def test_fewer_hypotheses_than_the_beam(hip):
    K.check_fewer_than_beam(hip.device)


def test_score_is_a_lower_bound_of_the_loss_kernels_probability(hip):
    K.check_lower_bound(hip.device)


def test_text_score_paths(hip):
    K.check_score_paths(hip.device)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


def test_convertor_nbest(hip):
    K.check_convertor(hip.device)


def test_text_accuracy_with_a_beam(hip):
    K.check_update_scores(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def _model(device, beam_width):
    from ccd_amd import finetune as ft
    from model_checks import _register_test_arch
    _register_test_arch()
    cfg = ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0)
    cfg.decoder_type, cfg.decoder_beam_width = "CTCDecoder", beam_width
    model = ft.build_model(cfg, device, dropout=0.0)
    assert model.label_convertor.beam_width == beam_width
    return model.eval()


def test_scoring_with_a_beam_does_not_synchronise(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(7)
    model = _model(hip.device, 4)
    conv = model.label_convertor
    tokens = torch.randn(3, 256, 192, device=hip.device).to(torch.bfloat16)
    with torch.no_grad():
        probs = model.decoder.forward_test(tokens)
    metric = TextAccuracy()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metric.update_scores(probs, WORDS, conv)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host = TextAccuracy()
    host.update(WORDS, K.oracle_strings(conv, probs.float().cpu().numpy(), 4))
    res, want = metric.result(), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12


def test_compute_scores_the_oracles_words_and_width_zero_is_greedy(hip):
    from ccd_amd import ops
    from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth
    torch.manual_seed(8)
    model = _model(hip.device, 4)
    conv = model.label_convertor
    gen = torch.Generator().manual_seed(4)
    images = [torch.randn(3, 3, 32, 128, generator=gen) for _ in range(2)]
    with torch.no_grad():
        probs = [model(img.to(hip.device), text=None, return_loss=False, test_speed=False).float() for img in images]
    decoded = [K.oracle_strings(conv, p.cpu().numpy(), 4) for p in probs]
    truth = [decoded[0], list(WORDS)]                                          # the first batch right, the second as it comes
    loader = [(img, (gt,)) for img, gt in zip(images, truth)]
    host = TextAccuracy()
    for gt, pt in zip(truth, decoded):
        host.update(gt, pt)
    res, want = TextAccuracy().compute(model, loader), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12
    assert res["words"] == 6.0 and res["cwr"] >= 0.5
    # beam_width = 0: the greedy records and totals of ops.text_score_ctc, and the host's greedy words
    conv.beam_width = 0
    greedy = TextAccuracy()
    res0 = greedy.compute(model, loader)
    totals = ops.text_totals(hip.device)
    raw, norm = (torch.from_numpy(t).to(hip.device) for t in conv.score_table())
    host0 = TextAccuracy()
    for p, gt in zip(probs, truth):
        codes, lens = (torch.from_numpy(a).to(hip.device) for a in encode_truth(gt))
        ops.text_accumulate(ops.text_score_ctc(p, raw, norm, codes, lens), totals)
        host0.update(gt, conv.idx2str(conv.tensor2idx(p)[0]))
    assert torch.equal(greedy._totals, totals)
    want0 = host0.result()
    assert all(res0[k] == want0[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res0["ned"] - want0["ned"]) < 1e-12
