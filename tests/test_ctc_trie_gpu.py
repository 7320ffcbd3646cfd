"""CTC prefix beam search along a lexicon's prefix tree and the two-stage decoder ops.ctc_lexicon_search on a real MI355X, through
libccd_hip.so (run with -m gpu): the kernel checks of tests/test_ctc_trie_sim.py (gates: tests/ctc_trie_checks.py), then the model - a
config with decoder_lexicon_beam builds the trie, and TextAccuracy scores the searched word without synchronising."""
import pytest
import torch

from backends import Backend
import ctc_checks as C
import ctc_trie_checks as K

pytestmark = pytest.mark.gpu
WORDS = C.WORDS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_exhaustive_shapes_give_the_lexicons_feasible_words(hip):
    K.check_exhaustive(hip.device)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_paths_scores_and_word_ids_equal_the_oracle(hip, seed):
    K.check_oracle(hip.device, (seed,))


def test_longest_frames_and_classes(hip):
    K.check_oracle_long(hip.device)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_the_searched_best_word_is_the_exhaustive_best(hip, seed):
    K.check_recall(hip.device, (seed,))


def test_a_merge_inside_the_trie(hip):
    K.check_merge(hip.device)


def test_a_full_lexicon_is_the_plain_beam_byte_for_byte(hip):
    K.check_full_lexicon(hip.device)


def test_abi_contract(hip):
    K.check_abi_contract(hip.device)


def test_convertor_with_a_lexicon_beam(hip):
    K.check_convertor(hip.device)


def test_alignment_takes_the_searched_word(hip):
    K.check_align(hip.device)


def test_text_accuracy_with_a_lexicon_beam_does_not_synchronise(hip):
    K.check_update_scores(hip.device, sync_debug=True)


# ------------------------------------------------------------------------------------------------ the model
def test_a_model_built_with_a_lexicon_beam_scores_the_searched_words(hip):
    from ccd_amd import finetune as ft
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy
    from model_checks import _register_test_arch
    import ctc_trie_np as N
    _register_test_arch()
    cfg = ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0)
    cfg.decoder_type, cfg.decoder_lexicon_beam = "CTCDecoder", 16
    cfg.decoder_lexicon = K.lexicon_strings(CTCConvertor(), N.batch_lexicon(100, True)[1]) + list(WORDS)
    torch.manual_seed(7)
    model = ft.build_model(cfg, hip.device, dropout=0.0).eval()
    conv = model.label_convertor
    assert conv.lexicon_beam == 16 and conv.lexicon_trie is not None and conv.lexicon_stats["nodes"] == conv.lexicon_trie.n_nodes > 10000
    gen = torch.Generator().manual_seed(4)
    images = [torch.randn(3, 3, 32, 128, generator=gen) for _ in range(2)]
    with torch.no_grad():
        probs = [model(img.to(hip.device), text=None, return_loss=False, test_speed=False).float() for img in images]
    decoded = [K.host_strings(conv, p) for p in probs]                         # tensor2lexicon -> idx2str: the host path
    truth = [decoded[0], list(WORDS)]                                          # the first batch right, the second as it comes
    host = TextAccuracy()
    for gt, pt in zip(truth, decoded):
        host.update(gt, pt)
    res, want = TextAccuracy().compute(model, [(img, (gt,)) for img, gt in zip(images, truth)]), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12
    assert res["words"] == 6.0 and res["cwr"] >= 0.5
