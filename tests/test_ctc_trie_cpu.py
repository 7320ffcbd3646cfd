"""The oracle of the trie beam search (tests/ctc_trie_np.py) against brute force and the exact word scores, the gap and recall
conditions of the inputs the executor / GPU tests use, the vectorised trie builder (ops.ctc_lexicon_trie) against the plain-Python
one, and the host logic of the convertor and the config.  No GPU, no kernel."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_np as R
import ctc_lexicon_np as X
import ctc_trie_checks as K
import ctc_trie_np as N


def _built(words, max_len=None):
    """The node table of ops.ctc_lexicon_trie for a word list, as numpy."""
    return K.trie_of(words, max_len).nodes.numpy()


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("T,C", R.EXHAUSTIVE)
@pytest.mark.parametrize("normalized", (False, True))
def test_oracle_gives_the_lexicons_feasible_words_with_their_exact_scores(T, C, normalized):
    """Every prefix fits the beam: the hypotheses are the lexicon's feasible words, scored as ctc_lexicon_np.word_score and brute force
    score them, in order - for the four lexicons of each shape."""
    x = R.small_case(T, C, seed=10 * T + C)
    x = R.softmax32(x) if normalized else x
    exact = R.brute_force(x, normalized)
    total = dict(exact)
    for words in K.exhaustive_lexicons(T, C, exact):
        want = K.exact_hypotheses(x, normalized, words)
        hyps, gap = N.beam_search_trie(x, 16, N.build_trie(words), normalized)
        assert gap >= R.MIN_GAP and len(want) >= 1
        assert [(w, k) for w, _, k in hyps] == [(w, k) for w, _, k in want]
        assert all(abs(a[1] - b[1]) <= 1e-12 and abs(a[1] - total[a[0]]) <= 1e-12 for a, b in zip(hyps, want))


def test_a_merge_inside_the_trie_equals_brute_force():
    x, words = K.merge_case()
    exact = dict(R.brute_force(x))
    hyps, gap = N.beam_search_trie(x, 16, N.build_trie(words))
    assert gap >= R.MIN_GAP and sorted(w for w, _, _ in hyps) == sorted(words)
    assert all(abs(s - exact[w]) <= 1e-12 for w, s, _ in hyps)
    # without the merged mass (1, 1) would miss the alignments that reach it through the live prefix (1,)
    lp = R.log_probs(x, False)
    assert abs(dict((w, s) for w, s, _ in hyps)[(1, 1)] - X.word_score(lp, (1, 1))) <= 1e-12


def test_a_full_lexicon_is_the_plain_oracle():
    words = [()] + [(a,) for a in range(1, 4)] + [(a, c) for a in range(1, 4) for c in range(1, 4)]
    nodes = N.build_trie(words)
    for seed in (71, 72, 73):
        x = R.small_case(2, 4, seed=seed)
        for W in (1, 4, 16):
            assert [(w, s) for w, s, _ in N.beam_search_trie(x, W, nodes)[0]] == R.beam_search(x, W)[0]


@pytest.mark.parametrize("seed", K.SEEDS)
@pytest.mark.parametrize("normalized", (False, True))
def test_batch_lexicon_meets_the_gap_and_recall_conditions(seed, normalized):
    """The inputs of the executor / GPU tests: the oracle alone meets the gap condition at every width on every sample, and at W = 16
    the exactly rescored best proposal is the best of ALL words (every one of the 1 500 scored in numpy) for 9 of 9 samples."""
    x, words, trie = K.lexicon(seed, normalized)
    nodes = trie.nodes.numpy()
    assert len(words) == 1500 and 11000 <= nodes.shape[0] <= 14000
    runs = {W: [N.beam_search_trie(x[b], W, nodes, normalized) for b in range(9)] for W in K.WIDTHS}
    worst = min(gap for W in K.WIDTHS for _, gap in runs[W])
    found = [sum(1 for hyps, _ in runs[W] if hyps) for W in K.WIDTHS]
    hits = {W: 0 for W in (4, 16)}
    for b in range(9):
        exact = X.score(x[b], words, normalized)
        assert X.min_gap(exact, words) >= X.MIN_GAP
        top = X.best(exact, 1)[0]
        for W in hits:
            got, _ = N.search(x[b], W, nodes, words, normalized)
            hits[W] += bool(got) and got[0][0] == top[0] and got[0][1] == top[1]
    print(f"seed {seed}, normalized {normalized}: {nodes.shape[0]} nodes, smallest gap {worst:.3e}, samples with a word at W = 1 / 4 / 16 "
          f"{found}, recall at W = 4 {hits[4]} / 9, at W = 16 {hits[16]} / 9")
    assert worst >= R.MIN_GAP and hits[16] == 9 and found[0] < 9


def test_limits_of_the_abi_meet_the_gap_condition():
    for normalized in (False, True):
        hyps = K.oracle(K.LONG_SEED, 16, normalized, 5, 64, 128)              # (asserts the condition per sample)
        assert any(hyps)


# ------------------------------------------------------------------------------------------------ the builder
HAND = {"empty lexicon": [], "empty word": [()], "duplicate rows": [(4,), (2, 3), (4,), (2, 3), ()],
        "a prefix of another": [(5, 6, 7), (5, 6), (5,), (6,)], "classes >= 64": [(64,), (63, 127), (127, 1), (31, 32, 33, 95, 96)],
        "classes outside 1..127": [(3,), (3, 128, 4), (200,), (3, 5)]}


def check_invariants(nodes, words):
    """Breadth-first order, contiguous sorted children, popcount addressing, word ids."""
    n = nodes.shape[0]
    assert nodes.dtype == np.int32 and nodes.shape[1] == 8 and tuple(nodes[0, 6:]) == (-1, 0)
    depth = np.zeros(n, dtype=np.int64)
    at = 1
    for node in range(n):
        mask = N.mask_of(nodes, node)
        assert not mask & 1
        classes = [c for c in range(1, 128) if (mask >> c) & 1]
        if classes:
            assert nodes[node, 4] == at                                        # the children follow those of the node before: BFS
        for k, c in enumerate(classes):
            kid = N.child(nodes, node, c)
            assert kid == at + k and tuple(nodes[kid, 6:]) == (node, c)
            depth[kid] = depth[node] + 1
        at += len(classes)
    assert at == n and (np.diff(depth) >= 0).all()
    first = {}
    for row, w in enumerate(words):
        w = N._cut(w)
        if all(1 <= c <= 127 for c in w):
            first.setdefault(w, row)
    assert {w: int(nodes[N.node_of(nodes, w), 5]) for w in first} == first and int((nodes[:, 5] >= 0).sum()) == len(first)


@pytest.mark.parametrize("name", sorted(HAND))
def test_builder_equals_the_dictionary_builder_on_hand_cases(name):
    words = HAND[name]
    nodes = _built(words)
    assert np.array_equal(nodes, N.build_trie(words)), name
    check_invariants(nodes, words)
    if name == "empty lexicon":
        assert nodes.tolist() == [[0, 0, 0, 0, 0, -1, -1, 0]]
    if name == "empty word":
        assert nodes.tolist() == [[0, 0, 0, 0, 0, 0, -1, 0]]
    if name == "duplicate rows":
        assert sorted(nodes[:, 5].tolist()) == [-1, 0, 1, 4]


def test_builder_equals_the_dictionary_builder_on_the_batch_lexicon():
    from ccd_amd import ops
    _, words, trie = K.lexicon(100, False)
    nodes = trie.nodes.numpy()
    assert np.array_equal(nodes, N.build_trie(words))
    check_invariants(nodes, words)
    assert trie.stats == {"nodes": nodes.shape[0], "bytes": 32 * nodes.shape[0], "terminals": 1500} and trie.n_nodes == nodes.shape[0]
    padded = X.to_tensor(words, 31)
    padded[3, 20] = 9                                                          # behind the word's first zero: not a part of the word
    assert np.array_equal(ops.ctc_lexicon_trie(ops.ctc_lexicon(torch.from_numpy(padded))).nodes.numpy(), nodes)
    assert trie.on("cpu") is trie.on("cpu") and trie.on("cpu").dtype == torch.int32


# ------------------------------------------------------------------------------------------------ the convertor and the config
def test_lexicon_beam_reaches_the_convertor_from_the_config(tmp_path):
    """decoder.lexicon_beam of the YAML (config.decoder_lexicon_beam) -> CTCConvertor.lexicon_beam and the trie; absent is today's
    behaviour; without a lexicon it is refused, and the NRTR head refuses it."""
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    from ccd_amd.utils.utils import Config
    words = tmp_path / "words.txt"
    words.write_text("hello\nworld\nhell\n", encoding="utf-8")
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    cfg.decoder_type, cfg.decoder_lexicon = "CTCDecoder", str(words)
    conv = DINO_Finetune(cfg).label_convertor
    assert conv.lexicon_beam == 0 and conv.lexicon_trie is None and "nodes" not in conv.lexicon_stats
    cfg.decoder_lexicon_beam = 16
    conv = DINO_Finetune(cfg).label_convertor
    assert conv.lexicon_beam == 16 and conv.lexicon_trie.n_nodes == 11 and conv.lexicon_stats["nodes"] == 11
    assert conv.lexicon_trie.stats == {"nodes": 11, "bytes": 352, "terminals": 3}
    cfg.decoder_lexicon = None
    with pytest.raises(ValueError, match="lexicon_beam = 16 needs a lexicon"):
        DINO_Finetune(cfg)
    cfg.decoder_lexicon, cfg.decoder_beam_width = str(words), 4
    with pytest.raises(ValueError, match="lexicon"):
        DINO_Finetune(cfg)
    nrtr = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    nrtr.decoder_lexicon_beam = 16
    with pytest.raises(NotImplementedError, match="CTC head only"):
        DINO_Finetune(nrtr)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).read()
    assert Config(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).decoder_lexicon_beam is None
    (tmp_path / "trie.yaml").write_text(src.replace("max_seq_len: 25}", f"max_seq_len: 25, lexicon: '{words}', lexicon_beam: 16}}"))
    config = Config(str(tmp_path / "trie.yaml"))
    assert config.decoder_lexicon == str(words) and config.decoder_lexicon_beam == 16 and config.decoder_type == "CTCDecoder"


def test_command_lines_take_a_lexicon_beam():
    from decoding_flags import SCRIPTS, declared
    for name in SCRIPTS:
        helps, configure = declared(name)
        assert "--lexicon_beam" in helps and configure(["--lexicon_beam", "16"]) == {"decoder_lexicon_beam": 16}, name
        assert configure([]) == {}, name                                      # a flag that is absent leaves the YAML's value
