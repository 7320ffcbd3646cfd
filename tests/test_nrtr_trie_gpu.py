"""Lexicon-constrained beam search over the NRTR decoder on a real MI355X, through libccd_hip.so (run with -m gpu): the kernel checks of
tests/test_nrtr_trie_sim.py (gates: tests/nrtr_trie_checks.py), then the model - DINO_Finetune.forward_lexicon against a teacher-forced
rescoring by the uncached decoder, a small lexicon ranked exhaustively, the HIP graph against eager launches, TextAccuracy.compute
with a lexicon, and a model without the keys.

The model, the images and the rescoring gate are those of tests/test_nrtr_beam_gpu.py (vit_tiny, a 2-layer decoder, seed 2, END_BIAS
0.5; `rescore_tol` = 4 x RESCORE_BASE + 2^-24 |score| + 1e-9, derived there from a measurement on the code before the beam existed):
the trie changes which candidates exist, never what a candidate scores, so a returned (word, score) must agree with the fp64
log-softmax of the uncached decoder's logits summed along the word and its <EOS> exactly as the plain beam's do.
Measured with the feature (printed by the tests): see the docstring of test_lexicon_words_agree_with_teacher_forced_rescoring."""
import numpy as np
import pytest
import torch

from backends import Backend
import nrtr_trie_checks as K
from test_nrtr_beam_gpu import BATCHES, END_BIAS, END_IDX, T, images, rescore, rescore_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_paths_parents_word_ids_and_nodes_equal_the_oracle(hip):
    K.check_oracle(hip.device)


def test_a_beam_as_wide_as_the_lexicon_returns_every_word(hip):
    K.check_wide_beam(hip.device)


def test_width_one_is_the_constrained_arg_max_chain(hip):
    K.check_width_one(hip.device)


def test_masked_allowed_classes_leave_the_sample_unused(hip):
    K.check_masked_sample(hip.device)


def test_mask_bits_32_64_127_and_the_class_without_a_bit(hip):
    K.check_boundary_classes(hip.device)


def test_argument_validation(hip):
    K.check_arguments(hip.device)


# ------------------------------------------------------------------------------------------------ the model
def build(device, lexicon=None, lexicon_beam=None):
    """tests/test_nrtr_beam_gpu.py: build, with the two lexicon keys of the configuration."""
    from ccd_amd import finetune as ft
    torch.manual_seed(2)
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=2)
    if lexicon is not None:
        cfg.decoder_lexicon, cfg.decoder_lexicon_beam = lexicon, lexicon_beam
    model = ft.build_model(cfg, device).eval()
    with torch.no_grad():
        model.arena.w("decoder.classifier.bias")[END_IDX] += END_BIAS
    model.arena.refresh_mirrors()
    return model


@pytest.fixture(scope="module")
def model(hip):
    return build(hip.device)


def strings_of(conv, words):
    """Class sequences as strings that encode back to the same classes: class 90, <UKN>, is written as a character outside the alphabet."""
    assert conv.unknown_idx == 90
    strings = ["".join("é" if c == 90 else conv.idx2char[c] for c in w) for w in words]
    assert conv.str2idx(strings) == [list(w) for w in words]
    return strings


def plain_words(model, img, W=8):
    """The finished hypotheses of the plain beam, by sample and rank (None where a slot ran to max_seq_len)."""
    with torch.no_grad():
        paths, lengths, _ = model.forward_beam(img, W)
    p, n = paths.cpu().numpy(), lengths.cpu().numpy()
    return [[tuple(p[b, r, :n[b, r]].tolist()) if 0 <= n[b, r] < T else None for r in range(W)] for b in range(p.shape[0])]


def batch_lexicon(model, img, seed, size=300):
    """Every second hypothesis of the plain beam at W = 8, a dozen one-edit neighbours of each sample's best word and random words of
    2..15 classes up to `size` words, sorted."""
    rng = np.random.default_rng(seed)
    words = set()
    for hyps in plain_words(model, img):
        words |= {w for r, w in enumerate(hyps) if r % 2 == 1 and w}
        best = next((w for w in hyps if w), (10, 11))
        for _ in range(12):
            w, k = list(best), int(rng.integers(0, 3))
            if k == 0 and len(w) > 1:
                del w[int(rng.integers(0, len(w)))]
            elif k == 1 and w:
                w[int(rng.integers(0, len(w)))] = int(rng.integers(0, 91))
            else:
                w.insert(int(rng.integers(0, len(w) + 1)), int(rng.integers(0, 91)))
            if 1 <= len(w) <= T - 1:
                words.add(tuple(w))
    while len(words) < size:
        words.add(tuple(int(c) for c in rng.integers(0, 91, int(rng.integers(2, 16)))))
    return sorted(words)


@pytest.mark.parametrize("W", [4, 8])
def test_lexicon_words_agree_with_teacher_forced_rescoring(model, hip, W):
    """Every returned word is the lexicon row its id names, the scores descend by rank, and each is the teacher-forced score of that
    word within rescore_tol.  Measured on an MI355X: the largest difference is 2.9e-6 at W = 4 (84 words) and at W = 8 (168
    words); the gate is 6.0e-6 at |score| = 100."""
    conv = model.label_convertor
    worst, within, found = 0.0, True, 0
    try:
        for B in BATCHES:
            img = images(B, hip.device)
            words = batch_lexicon(model, img, 31 + B)
            stats = conv.set_lexicon(strings_of(conv, words), beam=W)
            assert stats["kept"] == len(words) >= 300 and stats["too_long"] == 0 and stats["duplicates"] == 0
            with torch.no_grad():
                ids, log_probs, paths, lengths = model.forward_lexicon(img)
            assert ids.dtype == torch.int32 and log_probs.dtype == torch.float32 and tuple(ids.shape) == tuple(log_probs.shape) == (B, W)
            assert tuple(paths.shape) == (B, W, T) and tuple(lengths.shape) == (B, W)
            k, s, p, n = ids.cpu().numpy(), log_probs.double().cpu().numpy(), paths.cpu().numpy(), lengths.cpu().numpy()
            assert (k >= 0).all() and np.isfinite(s).all()                     # 300 words fill the beam, and every one of them can end
            assert (np.diff(s, axis=1) <= 0).all()                             # by rank
            for b in range(B):
                assert len(set(k[b].tolist())) == W, (b, k[b])
                for r in range(W):
                    assert tuple(p[b, r, :n[b, r]].tolist()) == words[k[b, r]] and (p[b, r, n[b, r]:] == -1).all(), (b, r)
            again = rescore(model, img, paths, lengths)
            worst = max(worst, float(np.abs(again - s).max()))
            within = within and bool((np.abs(again - s) <= rescore_tol(again)).all())
            found += k.size
    finally:
        conv.set_lexicon(None)
    print(f"W = {W}: largest |lexicon beam score - teacher-forced score| {worst:.3e} (gate {float(rescore_tol(100.0)):.3e} at |score| = "
          f"100) over {found} words")
    assert within


def test_a_small_lexicon_is_ranked_as_teacher_forcing_ranks_it(model, hip):
    """12 words at W = 16: nothing can be dropped, so every sample returns all 12, ordered as the teacher-forced scores of the 12
    words order them - compared where two exact scores differ by more than twice rescore_tol."""
    conv = model.label_convertor
    B = 5
    img = images(B, hip.device)
    pool = [w for hyps in plain_words(model, img) for w in hyps if w]
    words = sorted(set(pool))[:8]
    rng = np.random.default_rng(3)
    while len(words) < 12:
        w = tuple(int(c) for c in rng.integers(0, 91, int(rng.integers(1, 6))))
        if w not in words:
            words.append(w)
    try:
        conv.set_lexicon(strings_of(conv, words), beam=16)
        with torch.no_grad():
            ids, log_probs, _, _ = model.forward_lexicon(img)
    finally:
        conv.set_lexicon(None)
    k, s = ids.cpu().numpy(), log_probs.double().cpu().numpy()
    every = torch.full((B, 12, T), -1, dtype=torch.int32)
    for v, w in enumerate(words):
        every[:, v, :len(w)] = torch.tensor(w, dtype=torch.int32)
    exact = rescore(model, img, every, torch.tensor([[len(w) for w in words]] * B, dtype=torch.int32))
    for b in range(B):
        assert sorted(k[b, :12].tolist()) == list(range(12)) and (k[b, 12:] == -1).all() and np.isneginf(s[b, 12:]).all(), (b, k[b])
        rank = {int(v): r for r, v in enumerate(k[b, :12])}
        for v in range(12):
            assert abs(s[b, rank[v]] - exact[b, v]) <= rescore_tol(exact[b, v]), (b, v)
            for u in range(12):
                if exact[b, v] - exact[b, u] > 2 * max(rescore_tol(exact[b, v]), rescore_tol(exact[b, u])):
                    assert rank[v] < rank[u], (b, v, u, exact[b, v], exact[b, u])


def test_lexicon_beam_hip_graph_matches_eager(model, hip, monkeypatch):
    """forward_lexicon replays its steps from a captured HIP graph: identical to issuing the kernels one by one, also after the
    weights changed in place and for a second batch size; the graphs of the trie path are kept apart from the plain beam's."""
    words = batch_lexicon(model, images(16, hip.device), 47)                   # (the plain beam runs on the shared model)
    model = build(hip.device)                                                  # this one only ever walks the trie
    conv = model.label_convertor
    conv.set_lexicon(strings_of(conv, words), beam=8)
    for B in (16, 16, 5):
        img = images(B, hip.device)
        for W in (4, 8):
            with torch.no_grad():
                monkeypatch.setenv("CCD_DECODE_GRAPH", "1")
                graphed = model.forward_lexicon(img, W)
                monkeypatch.setenv("CCD_DECODE_GRAPH", "0")
                eager = model.forward_lexicon(img, W)
            assert len(graphed) == 4 and all(torch.equal(a, b) for a, b in zip(graphed, eager)), (B, W)
        with torch.no_grad():
            model.arena.flat.mul_(1.01)
        model.arena.refresh_mirrors()
    graphs = model.decoder._trie_graphs
    assert len(model.decoder._beam_graphs) == 0 and len(model.decoder._graphs) == 0
    assert len(graphs) == 4 and {key[-2] for key in graphs} == {4, 8} and {key[-1] for key in graphs} == {conv.lexicon_trie}


def _words_file(tmp_path, model, hip):
    conv = model.label_convertor
    path = tmp_path / "words.txt"
    path.write_text("\n".join(strings_of(conv, batch_lexicon(model, images(6, hip.device), 5))) + "\n", encoding="utf-8")
    return str(path)


def test_text_accuracy_scores_the_best_word_of_the_lexicon(model, hip, tmp_path):
    from ccd_amd.metric.eval_acc import TextAccuracy
    lex = build(hip.device, lexicon=_words_file(tmp_path, model, hip), lexicon_beam=4)
    conv = lex.label_convertor
    assert conv.lexicon_beam == 4 and conv.beam_width == 0 and conv.lexicon_stats["kept"] >= 300
    imgs = [images(6, hip.device), images(6, hip.device).flip(0) * 0.5]
    decoded = []
    with torch.no_grad():
        for img in imgs:
            ids, log_probs, _, _ = lex.forward_lexicon(img)
            best = conv.paths2lexicon(ids, log_probs, nbest=1)[0]
            assert all(len(w) == 1 for w in best)
            decoded.append(conv.idx2str([w[0] for w in best]))
    truth = [decoded[0], [s[:-1] + "Q" if b % 2 else s for b, s in enumerate(decoded[1])]]
    loader = [(img, (gt,)) for img, gt in zip(imgs, truth)]
    host = TextAccuracy()
    for gt, pt in zip(truth, decoded):
        host.update(gt, pt)
    metric = TextAccuracy()
    res, want = metric.compute(lex, loader), host.result()
    assert all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12
    assert res["words"] == 12.0 and metric._totals is not None and 0 < want["cwr"] < 1       # (the device path ran)
    # a second pass under the synchronisation guard: the graph, the trie's device copy and the tables are in place
    guarded = TextAccuracy()
    with torch.no_grad():
        guarded.update_paths(lex.forward_lexicon(imgs[0])[2][:, 0], truth[0], conv)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            guarded.update_paths(lex.forward_lexicon(imgs[1])[2][:, 0], truth[1], conv)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    again = guarded.result()
    assert all(again[k] == want[k] for k in ("ccr", "cwr", "ted", "words"))


def test_absent_lexicon_keys_are_todays_model(model, hip, tmp_path):
    """An NRTR configuration without decoder.lexicon / decoder.lexicon_beam: forward_test and forward_beam as a model built with
    them, and no trie anywhere."""
    lex = build(hip.device, lexicon=_words_file(tmp_path, model, hip), lexicon_beam=8)
    plain = build(hip.device)
    conv = plain.label_convertor
    assert conv.lexicon is None and conv.lexicon_trie is None and conv.lexicon_beam == 0 and conv.lexicon_stats is None
    img = images(5, hip.device)
    with torch.no_grad():
        assert torch.equal(plain.forward_test(img), lex.forward_test(img))
        assert all(torch.equal(a, b) for a, b in zip(plain.forward_beam(img, 4), lex.forward_beam(img, 4)))
        assert len(plain.forward_beam(img, 4)) == 3
    assert len(plain.decoder._trie_graphs) == 0 and len(lex.decoder._trie_graphs) == 0 and len(plain.decoder._beam_graphs) == 1
    with pytest.raises(ValueError, match="no lexicon"):
        plain.forward_lexicon(img)
