"""Scoring given words with the NRTR decoder on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of
tests/test_nrtr_score_sim.py (gates: tests/nrtr_score_checks.py), then the model - DINO_Finetune.forward_score against the scores of
forward_beam's own paths, forward_words against the host arg-max of forward_score, and forward_words against forward_lexicon.

The model and the images are those of tests/test_nrtr_beam_gpu.py (vit_tiny, a 2-layer decoder at its random initialisation, END_BIAS
0.5 on the classifier's <EOS>, B = 5; that file says why), and so is the gate: forward_beam's score and forward_score's are both the
fp64 sum of the log-softmax along the same path, of logits that the incremental decoder and the teacher-forced pass compute with the
same kernels on the same rows (RESCORE_BASE = 0 there), each rounded once to fp32: 2^-24 |score| + 1e-9.  Measured with the feature:
the scores of the 7 width-4 paths of the 5 images that end in front of max_seq_len agree bit for bit (the other 13 run to max_seq_len,
have no room for their <EOS> in a teacher-forced row and are infeasible by the rule), forward_lexicon and forward_words name the same
word with the same bits for 5 of 5 images, and the largest moment error is 1.3 % of its gate."""
import numpy as np
import pytest
import torch

from backends import Backend
import nrtr_score_checks as K

pytestmark = pytest.mark.gpu

END_IDX, PAD_IDX, T = 91, 92, 25
END_BIAS = 0.5
B = 5


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


@pytest.mark.parametrize("Tq", [7, 32])
def test_rows_attention_equals_the_replicated_attention_bit_for_bit(hip, Tq):
    K.check_rows_equal_replicated(hip.device, Tq)


@pytest.mark.parametrize("Tq", [7, 32])
def test_moments_of_the_attention_maps(hip, Tq):
    K.check_moments(hip.device, Tq)


def test_a_one_hot_map_gives_the_key_and_std_zero(hip):
    K.check_one_hot(hip.device)


def test_word_scores_equal_numpy(hip):
    K.check_word_scores(hip.device)


def test_argument_validation(hip):
    K.check_arguments(hip.device)


def test_scores2words_ties_padding_and_empty_lists(hip):
    K.check_best_of_lists(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def build(device, lexicon=None):
    from ccd_amd import finetune as ft
    torch.manual_seed(2)
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2)
    model = ft.build_model(cfg, device).eval()
    with torch.no_grad():
        model.arena.w("decoder.classifier.bias")[END_IDX] += END_BIAS
    model.arena.refresh_mirrors()
    if lexicon is not None:
        model.label_convertor.set_lexicon(lexicon, beam=16)
    return model


def images(n, device):
    x = torch.randn(n, 3, 32, 128, generator=torch.Generator().manual_seed(5 + n))
    g = torch.Generator().manual_seed(50 + n)
    x = x * 0.25 + 2.0 * torch.randn(n, 3, 1, 1, generator=g) + torch.randn(n, 3, 1, 128, generator=g)
    return x.to(device)


@pytest.fixture(scope="module")
def model(hip):
    return build(hip.device)


def test_forward_score_reproduces_the_scores_of_the_beam(model, hip):
    img = images(B, hip.device)
    with torch.no_grad():
        paths, lengths, scores = model.forward_beam(img, 4)
    p, n = paths.cpu().numpy(), lengths.cpu().numpy()
    assert (n >= 0).all() and (n < T).any() and (n == T).any()                 # words that end early and words that fill the decoder
    words = [[p[b, r, :n[b, r]].tolist() for r in range(4)] for b in range(B)]
    res = model.forward_score(img, words)
    assert res["row_ptr"].tolist() == [0, 4, 8, 12, 16, 20] and tuple(res["char_logp"].shape) == (20, T) and tuple(res["char_pos"].shape) == (20, T, 4)
    got, want = res["score"].double().cpu().numpy().reshape(B, 4), scores.double().cpu().numpy()
    length = res["length"].cpu().numpy().reshape(B, 4)
    # a path of max_seq_len characters never wrote its <EOS>: the beam scores the 25 characters, the teacher-forced row has no room for
    # the <EOS> and is infeasible - the closed-vocabulary rule (AttnConvertor.set_lexicon: too_long)
    full = n == T
    assert (length[~full] == n[~full]).all() and (length[full] == -1).all() and np.isneginf(got[full]).all()
    diff = np.abs(got[~full] - want[~full])
    print(f"forward_score against forward_beam (width 4): largest difference {diff.max():.3e} over {int((~full).sum())} words, "
          f"bit-equal: {bool((diff == 0).all())}; {int(full.sum())} paths at max_seq_len")
    assert (diff <= K.rescore_tol(want[~full])).all()
    lp = res["char_logp"].double().cpu().numpy().reshape(B, 4, T)
    assert (np.abs(lp.sum(-1)[~full] - got[~full]) <= 1e-4).all() and (lp <= 0).all()
    pos = res["char_pos"].cpu().numpy()
    assert (pos[..., 0] >= 0).all() and (pos[..., 0] <= 31).all() and (pos[..., 1] >= 0).all() and (pos[..., 1] <= 7).all() and (pos[..., 2:] >= 0).all()
    records = model.label_convertor.scores2chars(res, model.label_convertor.words2rows(words)[0])
    assert len(records) == 20 and [r["word"] is None for r in records] == full.reshape(-1).tolist()
    for r in records:
        assert all(0.0 <= c["box"][0] < c["box"][2] <= 128.0 and 0.0 <= c["box"][1] < c["box"][3] <= 32.0 and 0.0 < c["conf"] <= 1.0
                   for c in r["chars"])


def _lists():
    """A different 3-word list per image; one holds a word too long for the decoder, which stays in its place as an infeasible row."""
    return [["hello", "world", "a"], ["x" * 30, "0", "Hello"], ["abc", "abd", "ab"], ["", "zz", "q"], ["the", "of", "and"]]


def test_forward_words_is_the_host_arg_max_of_forward_score(model, hip):
    img = images(B, hip.device)
    words = _lists()
    res = model.forward_score(img, words)
    score = res["score"].double().cpu().numpy().reshape(B, 3)
    assert np.isneginf(score[1, 0]) and int(res["length"][3]) == -1 and np.isfinite(np.delete(score.reshape(-1), 3)).all()
    assert res["length"].cpu().tolist() == [len(w) if len(w) < T else -1 for ws in words for w in ws]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                    # nothing is read back, nothing waits
    try:
        index, best = model.forward_words(img, words, nbest=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    order = np.argsort(-score, axis=1, kind="stable")[:, :2]
    assert index.cpu().tolist() == order.tolist() and index.dtype == torch.int32
    assert np.array_equal(best.double().cpu().numpy(), np.take_along_axis(score, order, axis=1))
    one, _ = model.forward_words(img, words)
    assert one.cpu().tolist() == order[:, :1].tolist()


LEXICON = ["hello", "world", "a", "0", "Hello", "abc", "ab", "zz", "q", "the", "of", "and"]


def test_forward_words_agrees_with_forward_lexicon(hip):
    """A beam of 16 over the prefix tree of 12 words prunes nothing - no depth of the tree has more than 12 nodes - and every word is
    short enough to end: forward_lexicon's best word is the best of all 12 for EVERY image, none is empty."""
    model = build(hip.device, lexicon=LEXICON)
    assert model.label_convertor.lexicon_words == LEXICON
    img = images(B, hip.device)
    with torch.no_grad():
        word_ids, log_probs, _, _ = model.forward_lexicon(img)
    index, best = model.forward_words(img, [LEXICON] * B)
    ids, lp = word_ids[:, 0].cpu().numpy(), log_probs[:, 0].double().cpu().numpy()
    found = ids >= 0
    print(f"forward_lexicon returned a word for {int(found.sum())} of {B} images; largest |log p| difference "
          f"{np.abs(best[:, 0].double().cpu().numpy() - lp)[found].max():.3e}")
    assert int(found.sum()) == B
    assert index[:, 0].cpu().numpy()[found].tolist() == ids[found].tolist()
    assert (np.abs(best[:, 0].double().cpu().numpy() - lp)[found] <= K.rescore_tol(lp[found])).all()
