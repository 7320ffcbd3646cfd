"""Lexicon-constrained CTC decoding on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of
tests/test_ctc_lexicon_sim.py (gates: tests/ctc_lexicon_checks.py), a larger random lexicon, then the model - TextAccuracy with a
lexicon convertor does not synchronise and scores the word the oracle picks from the same probabilities."""
import pytest
import torch

from backends import Backend
import ctc_checks as C
import ctc_lexicon_checks as K

pytestmark = pytest.mark.gpu
WORDS = C.WORDS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_exhaustive_lexicons_equal_brute_force(hip):
    K.check_exhaustive(hip.device)


def test_scores_and_best_words_equal_the_oracle(hip):
    K.check_oracle_batch(hip.device)


def test_length_class_seams_give_identical_bits(hip):
    K.check_seams(hip.device)


def test_limits_of_frames_classes_and_labels(hip):
    K.check_limits(hip.device)


def test_masked_frames_and_classes(hip):
    K.check_masks(hip.device)


def test_subset_equals_the_gathered_columns(hip):
    K.check_subset(hip.device)


def test_a_word_listed_twice_ranks_the_lower_column_first(hip):
    K.check_ties(hip.device)


def test_scores_equal_the_loss_kernels(hip):
    K.check_against_loss(hip.device)


def test_beam_scores_are_lower_bounds_of_lexicon_scores(hip):
    K.check_against_beam(hip.device)


def test_random_lexicon_against_the_loss_kernel(hip):
    K.check_property(hip.device, B=33, V=1000, n_pairs=1500)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


def test_convertor_lexicon(hip, tmp_path):
    K.check_convertor(hip.device, tmp_path)


def test_text_accuracy_with_a_lexicon(hip):
    K.check_update_scores(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def _model(device):
    from ccd_amd import finetune as ft
    from ccd_amd.convertor.ctc import CTCConvertor
    from model_checks import _register_test_arch
    _register_test_arch()
    cfg = ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    cfg.decoder_lexicon = K.lexicon_strings(CTCConvertor(), 100) + list(WORDS)
    model = ft.build_model(cfg, device, dropout=0.0)
    assert model.label_convertor.lexicon_stats["kept"] >= 50
    return model.eval()


def test_scoring_with_a_lexicon_does_not_synchronise(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(7)
    model = _model(hip.device)
    conv = model.label_convertor
    tokens = torch.randn(3, 256, 192, device=hip.device).to(torch.bfloat16)
    with torch.no_grad():
        probs = model.decoder.forward_test(tokens)
    metric = TextAccuracy()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metric.update_scores(probs, WORDS, conv)                               # (the word list and the tables go up here, unsynchronised)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host = TextAccuracy()
    host.update(WORDS, K.oracle_strings(conv, probs.float().cpu().numpy()))
    res, want = metric.result(), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12


def test_compute_scores_the_oracles_lexicon_words(hip):
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(8)
    model = _model(hip.device)
    conv = model.label_convertor
    gen = torch.Generator().manual_seed(4)
    images = [torch.randn(3, 3, 32, 128, generator=gen) for _ in range(2)]
    with torch.no_grad():
        probs = [model(img.to(hip.device), text=None, return_loss=False, test_speed=False).float() for img in images]
    decoded = [K.oracle_strings(conv, p.cpu().numpy()) for p in probs]
    truth = [decoded[0], list(WORDS)]                                          # the first batch right, the second as it comes
    loader = [(img, (gt,)) for img, gt in zip(images, truth)]
    host = TextAccuracy()
    for gt, pt in zip(truth, decoded):
        host.update(gt, pt)
    res, want = TextAccuracy().compute(model, loader), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12
    assert res["words"] == 6.0 and res["cwr"] >= 0.5
    # the host path of compute (tensor2lexicon) decodes the same words
    for p, pt in zip(probs, decoded):
        assert conv.idx2str([w[0] for w in conv.tensor2lexicon(p, nbest=1)[0]]) == pt
