"""The lexicon oracle (tests/ctc_lexicon_np.py) against three independent references - tests/ctc_np.ctc_reference, torch's fp64
F.ctc_loss and brute force over every alignment - and the conditions its generator must meet.  No GPU, no kernel."""
import numpy as np
import pytest
import torch

import ctc_beam_np as R
import ctc_lexicon_np as L
import ctc_np as G


def test_oracle_equals_the_loss_reference_on_the_named_cases():
    for case in G.named_cases():
        x = case["logits"].numpy()
        got = L.score(x, [case["target"]])[0]
        nll, _ = G.ctc_reference(x, case["target"])
        if np.isinf(nll):
            assert got == -np.inf, case["name"]
        else:
            assert abs(got + nll) <= 1e-12 * max(1.0, abs(nll)), (case["name"], got, -nll)


def test_oracle_equals_torch_fp64_ctc_loss_on_the_named_cases():
    finite = 0
    for case in G.named_cases():
        x, target = case["logits"], case["target"]
        if len(target) > 31:
            continue
        loss, _, _ = G.torch_oracle(x[None], G.pad_targets(target), torch.float64)
        got = L.score(x.numpy(), [target])[0]
        if torch.isinf(loss[0]):
            assert got == -np.inf, case["name"]
        else:
            finite += 1
            assert abs(got + float(loss[0])) <= 1e-12 * max(1.0, abs(float(loss[0]))), (case["name"], got, -float(loss[0]))
    assert finite >= 5


@pytest.mark.parametrize("T,C", R.EXHAUSTIVE)
@pytest.mark.parametrize("normalized", (False, True))
def test_oracle_equals_brute_force(T, C, normalized):
    x = R.small_case(T, C, seed=10 * T + C)
    if normalized:
        x = R.softmax32(x)
    exact = R.brute_force(x, normalized)
    words = [w for w, _ in exact]
    got = L.score(x, words, normalized)
    assert max(abs(a - b) for a, (_, b) in zip(got, exact)) <= 1e-12
    assert abs(np.exp(got).sum() - 1.0) <= 1e-12
    assert [k for k, _ in L.best(got, 16)] == list(range(len(words)))
    # words brute force never sees have no alignment
    assert L.score(x, [(C,), (1,) * (T + 1), (0, 1)], normalized).tolist() == [-np.inf] * 3


def test_masks_give_minus_infinity_never_nan():
    x = R.small_case(4, 3, seed=3)
    x[:, 2] = -np.inf
    got = L.score(x, [(), (1,), (2,), (1, 2), (1, 1)])
    assert np.isfinite(got[[0, 1, 4]]).all() and np.isneginf(got[[2, 3]]).all()
    x[1, :] = -np.inf
    assert np.isneginf(L.score(x, [(), (1,), (2,)])).all()
    p = np.array([[0.5, 0.5, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    assert L.score(p[:1], [(1,)], normalized=True)[0] == pytest.approx(np.log(0.5))
    assert np.isneginf(L.score(p, [(), (1,)], normalized=True)).all()
    assert L.best([-np.inf, -3.0, -np.inf, -3.0, -1.0], 4) == [(4, -1.0), (1, -3.0), (3, -3.0)]
    assert L.min_gap(np.array([-1.0, -1.0, -2.5, -np.inf]), [(1,), (1,), (2,), (3,)]) == 1.5


def test_the_oracle_batch_meets_the_gap_condition():
    """The inputs of the executor / GPU tests, both kinds of input: per sample the smallest gap between two different words, the
    two words without an alignment, and how often the lexicon disagrees with greedy decoding."""
    worst, differ = np.inf, 0
    for seed in (100, 101, 102):
        logits = R.peaked_batch(seed)
        words = L.batch_lexicon(seed)
        assert len(words) == 70 and max(map(len, words)) == 31
        lengths = [len(w) for w in words]
        assert min(lengths) == 0 and any(8 <= n <= 15 for n in lengths) and any(n >= 16 for n in lengths)      # all three length classes
        greedy = G.greedy(logits)
        for x, normalized in ((logits, False), (R.softmax32(logits), True)):
            for b in range(x.shape[0]):
                exact = L.score(x[b], words, normalized)
                gap = L.min_gap(exact, words)
                assert gap >= L.MIN_GAP, (seed, normalized, b, gap)
                worst = min(worst, gap)
                bad = np.flatnonzero(np.isneginf(exact)).tolist()
                assert bad == [words.index((5,) * 17), words.index((3, 95, 4))], (seed, normalized, b, bad)
                if not normalized:
                    differ += tuple(greedy[0][b, :greedy[1][b]].tolist()) != tuple(words[L.best(exact, 1)[0][0]])
    print(f"smallest gap {worst:.3e}; the lexicon's best word differs from the greedy word on {differ} of 27 samples")
    assert differ >= 9


def test_lexicon_reaches_the_convertor_from_the_config(tmp_path):
    """decoder.lexicon of the YAML (config.decoder_lexicon) -> CTCConvertor.lexicon; absent is today's behaviour; the NRTR head refuses."""
    import os
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    from ccd_amd.utils.utils import Config
    torch.manual_seed(0)
    words = tmp_path / "words.txt"
    words.write_text("hello\nworld\n\nhello\n", encoding="utf-8")
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    assert DINO_Finetune(cfg).label_convertor.lexicon is None
    cfg.decoder_lexicon = str(words)
    conv = DINO_Finetune(cfg).label_convertor
    assert conv.lexicon_words == ["hello", "world"] and conv.lexicon_stats == {"read": 3, "kept": 2, "too_long": 0, "duplicates": 1}
    cfg.decoder_beam_width = 4
    with pytest.raises(ValueError, match="lexicon"):
        DINO_Finetune(cfg)
    nrtr = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    nrtr.decoder_lexicon = str(words)
    with pytest.raises(NotImplementedError, match="CTC head only"):
        DINO_Finetune(nrtr)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).read()
    assert Config(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")).decoder_lexicon is None
    (tmp_path / "lexicon.yaml").write_text(src.replace("max_seq_len: 25}", f"max_seq_len: 25, lexicon: '{words}'}}"))
    config = Config(str(tmp_path / "lexicon.yaml"))
    assert config.decoder_lexicon == str(words) and config.decoder_type == "CTCDecoder"
