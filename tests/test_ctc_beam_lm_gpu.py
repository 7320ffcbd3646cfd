"""CTC prefix beam search fused with a character n-gram language model on a real MI355X, through libccd_hip.so (run with -m gpu): the
kernel checks of tests/test_ctc_beam_lm_sim.py (gates: tests/ctc_beam_lm_checks.py), then the model - TextAccuracy with a
language-model convertor does not synchronise and scores what the oracle decodes from the same probabilities."""
import pytest
import torch

from backends import Backend
import ctc_beam_lm_checks as K
import ctc_checks as C

pytestmark = pytest.mark.gpu
WORDS = C.WORDS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_exhaustive_shapes_equal_brute_force_plus_the_word_term(hip):
    K.check_exhaustive(hip.device)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_paths_and_scores_equal_the_oracle(hip, seed):
    K.check_oracle(hip.device, (seed,))


def test_longest_frames_classes_and_order(hip):
    K.check_oracle_long(hip.device)


def test_weight_zero_is_the_plain_beam_byte_for_byte(hip):
    K.check_weight_zero(hip.device)


def test_a_merge_carries_the_absorbed_candidates_term(hip):
    K.check_merge(hip.device)


def test_end_of_word_reranks_and_empties_slots(hip):
    K.check_eos(hip.device)


def test_a_hard_mask_is_a_character_set(hip):
    K.check_charset(hip.device)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


def test_convertor_nbest_with_a_language_model(hip):
    K.check_convertor(hip.device)


def test_text_accuracy_with_a_language_model(hip):
    K.check_update_scores(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def _model(device, tmp_path):
    from ccd_amd import finetune as ft
    from model_checks import _register_test_arch
    _register_test_arch()
    words = tmp_path / "words.txt"
    words.write_text("\n".join(K.LM_WORDS + list(WORDS)) + "\n", encoding="utf-8")
    cfg = ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0)
    cfg.decoder_type, cfg.decoder_beam_width = "CTCDecoder", 4
    cfg.decoder_lm, cfg.decoder_lm_order, cfg.decoder_lm_weight, cfg.decoder_lm_bonus = str(words), 3, 0.6, 0.4
    model = ft.build_model(cfg, device, dropout=0.0)
    conv = model.label_convertor
    assert conv.beam_width == 4 and conv.lm is not None and conv.lm_order == 3 and conv.lm_eos
    assert (conv.lm_weight, conv.lm_bonus) == (0.6, 0.4) and conv.lm_stats["rows"] == 92 * 92
    return model.eval()


def test_scoring_with_a_language_model_does_not_synchronise(hip, tmp_path):
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(7)
    model = _model(hip.device, tmp_path)
    conv = model.label_convertor
    tokens = torch.randn(3, 256, 192, device=hip.device).to(torch.bfloat16)
    with torch.no_grad():
        probs = model.decoder.forward_test(tokens)
    metric = TextAccuracy()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metric.update_scores(probs, WORDS, conv)                               # (the table goes up here, unsynchronised)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host = TextAccuracy()
    host.update(WORDS, K.oracle_strings(conv, probs.float().cpu().numpy(), 4))
    res, want = metric.result(), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12


def test_compute_scores_the_oracles_words_on_both_paths(hip, tmp_path):
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(8)
    model = _model(hip.device, tmp_path)
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
    # the host path of compute (tensor2nbest) decodes the same words
    for p, pt in zip(probs, decoded):
        assert conv.idx2str([w[0] for w in conv.tensor2nbest(p, nbest=1)[0]]) == pt
