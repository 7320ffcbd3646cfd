"""The host side of scoring given words with the NRTR head - no kernels: AttnConvertor.words2rows / scores2words / scores2chars, the
numpy specification (tests/nrtr_score_np.py) on hand-made cases, the CTC head's refusals, test.py --char_scores, and the refusals
pinned before this feature, which stay."""
import importlib.util
import io
import json
import os
import types

import numpy as np
import pytest
import torch

import nrtr_score_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("ccd_test_script_scores", os.path.join(ROOT, "test.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


# ------------------------------------------------------------------------------------------------ the specification
def test_numpy_word_score_on_a_uniform_row():
    C, T = 5, 4
    seq = np.array([[4, 1, 4, 5], [4, 4, 5, 5], [4, 1, 2, 3], [4, 7, 4, 5], [4, 5, 4, 5]])
    lp, score, length, pos = S.word_score(np.zeros((5 * T, C + 2), dtype=np.float32), C, seq, 4, 5)
    assert length.tolist() == [1, 0, -1, -1, -1] and pos is None
    assert np.allclose(score[:2], [-2 * np.log(5), -np.log(5)]) and np.isneginf(score[2:]).all()
    assert np.allclose(lp[0], [-np.log(5), -np.log(5), 0.0]) and not lp[2:].any()


def test_numpy_moments_and_positions():
    p = np.zeros((2, 256))
    p[0, 37] = 1.0                                                             # x = 5, y = 1
    p[1, 32 * 3 + 10], p[1, 32 * 3 + 12] = 0.5, 0.5                            # x = 10 | 12, y = 3
    m = S.moments_of(p)
    assert m.tolist() == [[5.0, 1.0, 25.0, 1.0], [11.0, 3.0, 122.0, 9.0]]
    assert S.char_pos_of(m[:1].astype(np.float32)).tolist() == [5.0, 1.0, 0.0, 0.0]
    assert S.char_pos_of(m[1:].astype(np.float32)).tolist() == [11.0, 3.0, 1.0, 0.0]
    both = S.char_pos_of(m.astype(np.float32))                                 # the average of the two heads' maps
    assert both[0] == 8.0 and both[1] == 2.0 and abs(both[2] - np.sqrt(73.5 - 64.0)) < 1e-12 and both[3] == 1.0


def test_numpy_best_of_lists():
    ninf = -np.inf
    index, best = S.best_of_lists(np.array([-1.0, -1.0, ninf, -0.5, ninf]), [0, 3, 3, 4, 5], 2)
    assert index.tolist() == [[0, 1], [-1, -1], [0, -1], [-1, -1]] and best[0].tolist() == [-1.0, -1.0] and np.isneginf(best[1]).all()


# ------------------------------------------------------------------------------------------------ the convertor
def test_words2rows_layout_too_long_words_and_row_ptr():
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=6, with_unknown=True)
    words = [["ab", "", "hello"], [], ["0a0", "hellos", [10, 90, 11]]]
    seq, row_ptr, rows = conv.words2rows(words)
    assert seq.dtype == torch.int64 and tuple(seq.shape) == (6, 7) and row_ptr.dtype == torch.int32 and row_ptr.tolist() == [0, 3, 3, 6]
    assert rows == ["ab", "", "hello", "0a0", "hellos", "a<UKN>b"]
    E, P = conv.end_idx, conv.padding_idx
    h = conv.str2idx(["hellos"])[0]
    assert seq.tolist() == [[E, 10, 11, E, P, P, P], [E, E, P, P, P, P, P], [E] + h[:5] + [E], [E, 0, 10, 0, E, P, P],
                            [E] + h,                                           # six characters: no room for the <EOS> - kept, infeasible
                            [E, 10, 90, 11, E, P, P]]
    assert [S.feasible(r, 92, E, P) for r in seq.numpy()] == [True, True, True, True, False, True]
    longer = conv.words2rows([["x" * 40]])[0]
    assert longer.tolist() == [[E] + [33] * 6]
    empty = conv.words2rows([[], []])
    assert tuple(empty[0].shape) == (0, 7) and empty[1].tolist() == [0, 0, 0] and empty[2] == []
    for bad in ("ab", ["ab"], [["ab", 3]], [[["a"]]]):
        with pytest.raises(TypeError, match="words2rows"):
            conv.words2rows(bad)
    with pytest.raises(KeyError):
        AttnConvertor(max_seq_len=6, with_unknown=False).words2rows([["é"]])


def test_scores2words_scatters_every_list_into_its_own_row(monkeypatch):
    """The table ops.ctc_lexicon_best receives (the kernel itself: tests/test_nrtr_score_sim.py): row i holds list i, -inf behind it."""
    from ccd_amd import ops
    from ccd_amd.convertor.attn import AttnConvertor
    seen = {}

    def best(table, nbest=1):
        seen["table"], seen["nbest"] = table.clone(), nbest
        index, score = S.best_of_lists(table.numpy().reshape(-1), np.arange(table.shape[0] + 1) * table.shape[1], nbest)
        return torch.from_numpy(index).int(), torch.from_numpy(score).float()

    monkeypatch.setattr(ops, "ctc_lexicon_best", best)
    conv = AttnConvertor(max_seq_len=25)
    score = torch.tensor([-3.0, -1.0, -1.0, -7.0, float("-inf")])
    index, log_probs = conv.scores2words(score, torch.tensor([0, 3, 3, 5], dtype=torch.int32), nbest=2)
    ninf = float("-inf")
    assert seen["nbest"] == 2 and seen["table"].tolist() == [[-3.0, -1.0, -1.0], [ninf, ninf, ninf], [-7.0, ninf, ninf]]
    assert index.tolist() == [[1, 2], [-1, -1], [0, -1]] and log_probs[0].tolist() == [-1.0, -1.0]           # the tie: lower index first
    conv.scores2words(score[:0], [0, 0], nbest=1)
    assert tuple(seen["table"].shape) == (1, 1) and seen["table"].tolist() == [[ninf]]
    for ptr in ([0, 3, 2, 5], [0, 3, 3, 4], [1, 3, 3, 5]):
        with pytest.raises(ValueError, match="csr_rows|scores2words"):
            conv.scores2words(score, ptr)
    with pytest.raises(ValueError, match="scores2words"):
        conv.scores2words(score.double(), [0, 3, 3, 5])


def test_scores2chars_boxes_on_hand_made_moments():
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=4, with_unknown=True)
    seq, row_ptr, rows = conv.words2rows([["ab", "hello"], ["0"]])             # "hello" is too long for 4 positions
    pos = torch.zeros(3, 4, 4)
    pos[0, 0] = torch.tensor([5.0, 1.0, 0.0, 0.0])                             # a sharp map: the half-cell floor
    pos[0, 1] = torch.tensor([10.0, 3.5, 2.0, 1.0])
    pos[2, 0] = torch.tensor([0.25, 7.0, 1.0, 4.0])                            # clipped on three sides
    logp = torch.zeros(3, 4)
    logp[0, :3] = torch.log(torch.tensor([0.5, 0.25, 0.125]))
    logp[2, :2] = torch.log(torch.tensor([1.0, 0.5]))
    result = {"score": torch.tensor([float(np.log(0.5 * 0.25 * 0.125)), float("-inf"), float(np.log(0.5))]),
              "length": torch.tensor([2, -1, 1], dtype=torch.int32), "char_logp": logp, "char_pos": pos, "row_ptr": row_ptr}
    rec = conv.scores2chars(result, seq)
    assert [r["word"] for r in rec] == ["ab", None, "0"] and rec[1] == {"word": None, "log_prob": float("-inf"), "eos_conf": 0.0, "chars": []}
    a, b = rec[0]["chars"]
    assert a["char"] == "a" and abs(a["conf"] - 0.5) < 1e-7 and (a["cx"], a["cy"]) == (22.0, 6.0) and a["box"] == [20.0, 4.0, 24.0, 8.0]
    r3 = np.sqrt(3.0)
    assert b["char"] == "b" and (b["cx"], b["cy"]) == (42.0, 16.0)
    assert np.allclose(b["box"], [42.0 - 8 * r3, 16.0 - 4 * r3, 42.0 + 8 * r3, 16.0 + 4 * r3]) and abs(b["conf"] - 0.25) < 1e-7
    assert abs(rec[0]["eos_conf"] - 0.125) < 1e-7 and abs(rec[0]["log_prob"] - np.log(0.5 * 0.25 * 0.125)) < 1e-6
    z, = rec[2]["chars"]
    assert z["char"] == "0" and (z["cx"], z["cy"]) == (3.0, 30.0) and np.allclose(z["box"], [0.0, 30.0 - 16 * r3, 3.0 + 4 * r3, 32.0])
    wide = conv.scores2chars(result, seq, img_hw=(64, 256))[0]["chars"][0]     # another crop size: cells of 8 x 8 pixels
    assert (wide["cx"], wide["cy"]) == (44.0, 12.0) and wide["box"] == [40.0, 8.0, 48.0, 16.0]
    with pytest.raises(ValueError, match="scores2chars"):
        conv.scores2chars(result, seq[:2])


# ------------------------------------------------------------------------------------------------ the model and the command line
def test_the_ctc_head_refuses_forward_score_and_forward_words():
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    ctc = DINO_Finetune(cfg)
    img = torch.zeros(1, 3, 32, 128)
    for call in (lambda: ctc.forward_score(img, [["a"]]), lambda: ctc.forward_words(img, [["a"]], nbest=2)):
        with pytest.raises(NotImplementedError, match=r"tensor2lexicon\(subset=\).*forward_chars"):
            call()
    nrtr = DINO_Finetune(ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=1))
    with pytest.raises(ValueError, match="one word list per image"):
        nrtr.forward_score(img, [["a"], ["b"]])
    dec = nrtr.decoder
    assert hasattr(dec, "forward_score") and hasattr(nrtr, "forward_words")


class _Stub(torch.nn.Module):
    """A model whose decoder returns 'ab' for the first image and nothing for the second."""

    def __init__(self, conv):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(1))
        self.label_convertor, self.ctc, self.calls = conv, False, []

    def forward_beam(self, img, beam_width=None):
        self.calls.append(("beam", beam_width))
        paths = torch.full((2, 1, 25), -1, dtype=torch.int32)
        paths[0, 0, :2] = torch.tensor([10, 11], dtype=torch.int32)
        return paths, torch.tensor([[2], [-1]], dtype=torch.int32), torch.tensor([[-1.5], [float("-inf")]])

    def forward_lexicon(self, img):
        self.calls.append(("lexicon", None))
        paths, lengths, scores = self.forward_beam(img)
        return torch.tensor([[0], [-1]], dtype=torch.int32), scores, paths, lengths

    def forward_score(self, img, words):
        self.calls.append(("score", words))
        pos = torch.zeros(1, 25, 4)
        pos[0, :2, 0] = torch.tensor([3.0, 9.0])
        logp = torch.zeros(1, 25)
        logp[0, :3] = -0.5
        return {"score": torch.tensor([-1.5]), "length": torch.tensor([2], dtype=torch.int32), "char_logp": logp, "char_pos": pos,
                "row_ptr": torch.tensor([0, 1, 1], dtype=torch.int32)}


def test_char_scores_of_test_py():
    from ccd_amd.convertor.attn import AttnConvertor
    script = _script()
    src = open(os.path.join(ROOT, "test.py")).read()
    assert '"--char_scores"' in src and "NRTR head only" in src[src.index('"--char_scores"'):][:700]
    with pytest.raises(ValueError, match="exclude each other"):
        script.check_arguments(types.SimpleNamespace(char_scores="a.jsonl", alignments="b.jsonl"))
    script.check_arguments(types.SimpleNamespace(char_scores="a.jsonl", alignments=None))
    script.check_arguments(types.SimpleNamespace(char_scores=None, alignments=None))                  # absent: today's run
    assert "--char_scores is for the NRTR head only" in src and "--alignments" in src[src.index("--char_scores is for the NRTR head only"):][:200]
    config = types.SimpleNamespace(dataset_image_height=32, dataset_image_width=128)
    loader = [(torch.zeros(2, 3, 32, 128), (["ab", "cd"],))]
    for kw, first in ((dict(), ("beam", 1)), (dict(beam_width=4), ("beam", 4)), (dict(lexicon=["ab", "b"], lexicon_beam=2), ("lexicon", None))):
        stub = _Stub(AttnConvertor(max_seq_len=25, **kw))
        out = io.StringIO()
        script.write_char_scores(stub, [loader], config, out, names=["synthetic"])
        assert stub.calls[0] == first and stub.calls[-1] == ("score", [[[10, 11]], []])
        lines = [json.loads(line) for line in out.getvalue().splitlines()]
        assert [(r["dataset"], r["index"], r["gt"], r["pred"]) for r in lines] == [("synthetic", 0, "ab", "ab"), ("synthetic", 1, "cd", None)]
        assert lines[0]["log_prob"] == -1.5 and [c["char"] for c in lines[0]["chars"]] == ["a", "b"] and lines[1]["chars"] == []
        assert [c["cx"] for c in lines[0]["chars"]] == [14.0, 38.0] and all(abs(c["conf"] - np.exp(-0.5)) < 1e-7 for c in lines[0]["chars"])
        assert lines[1]["log_prob"] is None


def test_pinned_refusals_stay():
    from ccd_amd import finetune as ft
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.model.dino_vision import DINO_Finetune
    conv = AttnConvertor(max_seq_len=25)
    for call in (conv.tensor2align, conv.tensor2chars):
        with pytest.raises(NotImplementedError, match="CTC head only - the NRTR decoder has no frame axis"):
            call(torch.zeros(1, 25, 92))
    with pytest.raises(NotImplementedError, match="one teacher-forced decoder pass per word"):
        AttnConvertor(max_seq_len=25, lexicon=["a"])
    with pytest.raises(NotImplementedError, match="one teacher-forced decoder pass per word"):
        AttnConvertor(max_seq_len=25, lexicon_beam=4)
    nrtr = DINO_Finetune(ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0, decoder_n_layers=1))
    with pytest.raises(NotImplementedError, match="forward_chars is the CTC head's"):
        nrtr.forward_chars(torch.zeros(1, 3, 32, 128))
    src = open(os.path.join(ROOT, "test.py")).read()
    assert "--alignments is for the CTC head only: the NRTR decoder has no frame axis to align a word against" in src


def test_row_tables_are_checked_on_the_host():
    from ccd_amd import ops
    rows = ops.csr_rows([0, 2, 2, 5])
    assert (rows.B, rows.R, rows.max_rows) == (3, 5, 3) and rows.ptr.dtype == np.int32 and ops.csr_rows(rows) is rows
    assert ops.csr_rows(torch.tensor([0, 1], dtype=torch.int32)).R == 1 and ops.csr_rows(np.array([0], dtype=np.int64)).B == 0
    for bad, err in (([0, 2, 1], ValueError), ([1, 2], ValueError), ([], TypeError), ([0.0, 1.0], TypeError), ([[0, 1]], TypeError),
                     (torch.tensor([0.0, 1.0]), TypeError)):
        with pytest.raises(err, match="csr_rows"):
            ops.csr_rows(bad)
