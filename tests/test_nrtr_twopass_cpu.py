"""Two-pass decoding without a GPU and without a launch: the numpy specification tests/nrtr_twopass_np.py on hand-made cases, the
configuration keys and every refusal, the command-line flags, the YAML keys, and the checks of the ops wrappers that come before a
launch."""
import os

import numpy as np
import pytest
import torch

import nrtr_twopass_checks as K
import nrtr_twopass_np as P
from decoding_flags import SCRIPTS, declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(**keys):
    from ccd_amd import finetune as ft
    cfg = ft.FinetuneConfig(arch="vit_tiny", decoder_n_layers=1)
    for k, v in keys.items():
        setattr(cfg, "decoder_" + k, v)
    return cfg


# ------------------------------------------------------------------------------------------------ the specification
def test_specification_rows_of_hand_made_proposals():
    paths = np.full((1, 4, 6), -1, dtype=np.int32)
    paths[0, 0, :2] = [11, 12]                                                 # 'ab' in CTC classes
    paths[0, 2, :3] = [11, 92, 12]                                             # a class on <EOS>
    lengths = np.array([[2, 0, 3, -1]], dtype=np.int32)
    seq, targets, subset = P.rows(paths, lengths, 1, 92, 91, 91, 92, 5, 4)
    assert seq.tolist() == [[91, 10, 11, 91, 92], [91, 91, 92, 92, 92], [91, 92, 92, 92, 92], [91, 92, 92, 92, 92]]
    assert targets.tolist() == [[11, 12, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and subset.tolist() == [[0, 1, -1, -1]]
    assert P.rows(paths, lengths, 1, 92, 91, 91, 92, 3, 4)[2].tolist() == [[-1, 1, -1, -1]]    # seq_len 3: one position for <EOS> only
    assert P.rows(paths, lengths, 1, 92, 91, 91, 92, 5, 1)[2].tolist() == [[-1, 1, -1, -1]]    # Lmax 1


def test_specification_select_ranks_by_score_then_slot_and_leaves_zero_weighted_terms_out():
    paths = np.full((1, 4, 6), -1, dtype=np.int32)
    for k in range(4):
        paths[0, k, :k] = 11 + k
    lengths = np.array([[0, 1, 2, 3]], dtype=np.int32)
    subset = np.array([[0, 1, 2, -1]], dtype=np.int32)
    att = np.array([-3.0, -1.0, -1.0, -0.5], dtype=np.float32)
    ctc = np.array([[-2.0, -4.0, -4.0, -0.5]], dtype=np.float32)
    out = P.select(att, ctc, paths, lengths, subset, 0.5, 5, 1)
    assert out[5].tolist() == [[0, 1, 2, -1]] and out[1].tolist() == [[0, 1, 2, -1]] and out[2].tolist() == [[-2.5, -2.5, -2.5, -np.inf]]
    assert out[0][0, 2].tolist() == [12, 12, -1, -1, -1] and out[3].tolist() == [[-3.0, -1.0, -1.0, -np.inf]]
    assert P.select(att, ctc, paths, lengths, subset, 0.0, 5, 1)[5].tolist() == [[1, 2, 0, -1]]
    ctc[0, 1] = -np.inf                                                        # never selected, also where its weight is 0
    out = P.select(att, ctc, paths, lengths, subset, 0.0, 5, 1)
    assert out[5].tolist() == [[2, 0, -1, -1]] and out[2].tolist() == [[-1.0, -3.0, -np.inf, -np.inf]] and not np.isnan(out[2]).any()
    assert P.combine(-1.0, -np.inf, 0.0) == -1.0 and P.combine(-np.inf, -2.0, 1.0) == -2.0


def test_specification_decode_combines_the_exact_ctc_score_with_the_callable_scorer():
    import ctc_beam_np as R
    import ctc_lexicon_np as L
    rng = np.random.default_rng(3)
    frames = R.softmax32(rng.standard_normal((1, 6, 5)).astype(np.float32))
    paths = np.array([[[1, 2, -1, -1, -1, -1], [2, -1, -1, -1, -1, -1], [4, 4, -1, -1, -1, -1]]], dtype=np.int32)
    lengths = np.array([[2, 1, 2]], dtype=np.int32)
    scorer = lambda seq: np.where((seq == 3).sum(axis=1) == 2, -(seq != 4).sum(axis=1).astype(np.float32), -np.inf)      # noqa: E731
    out = P.decode(frames, paths, lengths, scorer, 0.25, classes=4, start_idx=3, end_idx=3, pad_idx=4, T=5)
    lp = R.log_probs(frames[0], True)
    want = [0.75 * -4.0 + 0.25 * np.float32(L.word_score(lp, [1, 2])), 0.75 * -3.0 + 0.25 * np.float32(L.word_score(lp, [2]))]
    order = np.argsort(-np.array(want), kind="stable")
    assert out[5].tolist() == [order.tolist() + [-1]]                          # slot 2: class 4 maps onto <EOS> (3): dropped
    assert np.allclose(out[2][0, :2], np.array(want)[order], rtol=2e-7) and out[0][0, 0, :out[1][0, 0]].tolist() == (paths[0, order[0], :lengths[0, order[0]]] - 1).tolist()


# ------------------------------------------------------------------------------------------------ the wrappers, before any launch
def test_ops_wrappers_refuse_bad_dtypes_and_shapes_before_any_launch(monkeypatch):
    from ccd_amd import ops
    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a refusal came after a launch"))
    K.check_wrapper_refusals("cpu")


# ------------------------------------------------------------------------------------------------ configuration
def test_refusals_name_the_keys(tmp_path):
    from ccd_amd.model.dino_vision import DINO_Finetune
    words = tmp_path / "words.txt"
    words.write_text("hello\nworld\n", encoding="utf-8")
    for keys, match in ((dict(twopass_beam=4), "decoder.twopass_beam needs decoder.aux_ctc_weight > 0"),
                        (dict(twopass_beam=4, aux_ctc_weight=0), "decoder.twopass_beam needs decoder.aux_ctc_weight > 0"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, beam_width=4), "decoder.twopass_beam excludes decoder.beam_width"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, lexicon=str(words), lexicon_beam=4),
                         "decoder.twopass_beam excludes decoder.lexicon / decoder.lexicon_beam"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, lexicon_beam=4), "decoder.twopass_beam excludes decoder.lexicon / decoder.lexicon_beam"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, joint_ctc_weight=0.3), "decoder.twopass_beam excludes decoder.joint_ctc_weight"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, joint_ctc_weight=0.3, beam_width=4), "decoder.twopass_beam excludes"),
                        (dict(type="CTCDecoder", twopass_beam=4), "decoder.twopass_beam.*CTCDecoder"),
                        (dict(type="CTCDecoder", twopass_ctc_weight=0.3), "decoder.twopass_ctc_weight.*CTCDecoder"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=17), r"twopass_beam must lie in 1\.\.16"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=-1), r"twopass_beam must lie in 1\.\.16"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=True), r"twopass_beam must lie in 1\.\.16"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=2.5), r"twopass_beam must lie in 1\.\.16"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, twopass_ctc_weight=1.5), r"twopass_ctc_weight must lie in \[0, 1\]"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, twopass_ctc_weight=True), r"twopass_ctc_weight must lie in \[0, 1\]"),
                        (dict(aux_ctc_weight=0.2, twopass_beam=4, twopass_ctc_weight="0.5"), r"twopass_ctc_weight must lie in \[0, 1\]"),
                        (dict(aux_ctc_weight=0.2, twopass_ctc_weight=0.5), "twopass_ctc_weight = 0.5 needs twopass_beam")):
        with pytest.raises(ValueError, match=match):
            DINO_Finetune(_config(**keys))
    model = DINO_Finetune(_config())
    with pytest.raises(ValueError, match="decoder.aux_ctc_weight"):           # a model without the auxiliary head
        model.forward_twopass(torch.zeros(1, 3, 32, 128), beam=4)
    ctc = DINO_Finetune(_config(type="CTCDecoder"))
    with pytest.raises(NotImplementedError, match="forward_twopass is the NRTR head's"):
        ctc.forward_twopass(torch.zeros(1, 3, 32, 128), beam=4)


def test_pinned_refusals_stay():
    from ccd_amd.convertor.attn import AttnConvertor
    with pytest.raises(NotImplementedError, match="language-model fusion is for the CTC head only"):
        AttnConvertor(lm="words.txt", twopass_beam=4)
    with pytest.raises(NotImplementedError, match="scoring every word of a lexicon is for the CTC head only"):
        AttnConvertor(lexicon=["hello"], twopass_beam=4)


def test_keys_reach_the_convertor_and_absent_keys_change_nothing():
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.model.dino_vision import DINO_Finetune
    conv = AttnConvertor(twopass_beam=8, twopass_ctc_weight=0.25)
    assert (conv.twopass_beam, conv.twopass_ctc_weight) == (8, 0.25)
    assert (AttnConvertor(twopass_beam=8).twopass_ctc_weight, AttnConvertor.TWOPASS_DEFAULT_WEIGHT) == (0.5, 0.5)
    assert (AttnConvertor().twopass_beam, AttnConvertor().twopass_ctc_weight) == (0, None)
    assert AttnConvertor(twopass_beam=4, twopass_ctc_weight=0).twopass_ctc_weight == 0.0       # 0 is a value
    with pytest.raises(ValueError, match="twopass_beam = 4 excludes beam_width"):
        AttnConvertor(twopass_beam=4, beam_width=4)
    with pytest.raises(ValueError, match="twopass_beam = 4 excludes beam_width > 0 and lexicon"):
        AttnConvertor(twopass_beam=4, lexicon=["hello"], lexicon_beam=4)
    torch.manual_seed(0)
    hybrid = DINO_Finetune(_config(aux_ctc_weight=0.2))
    torch.manual_seed(0)
    model = DINO_Finetune(_config(aux_ctc_weight=0.2, twopass_beam=8, twopass_ctc_weight=0.3))
    conv = model.label_convertor
    assert (conv.twopass_beam, conv.twopass_ctc_weight, conv.beam_width, conv.lexicon) == (8, 0.3, 0, None)
    assert model.decoder.beam_width == 0 and model.joint_ctc_weight is None
    assert model.last_att_scores is None and model.last_ctc_scores is None and model.last_sources is None
    sd, want = model.state_dict(), hybrid.state_dict()
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)            # no parameter of its own
    for absent in (dict(), dict(twopass_beam=None), dict(twopass_beam=0), dict(twopass_beam=None, twopass_ctc_weight=None)):
        plain = DINO_Finetune(_config(**absent))
        assert (plain.label_convertor.twopass_beam, plain.label_convertor.twopass_ctc_weight) == (0, None), absent
    ctc = DINO_Finetune(_config(type="CTCDecoder", twopass_beam=0))             # 0 is "off" for either head
    assert ctc.ctc and not hasattr(ctc.label_convertor, "twopass_beam")


def test_shipped_configurations_have_no_two_pass_keys():
    from ccd_amd.utils.utils import Config
    from ccd_amd.model.dino_vision import DINO_Finetune
    for name in ("CCD_vision_model_ARD.yaml", "CCD_vision_model_ARD_CTC.yaml"):
        config = Config(os.path.join(ROOT, "Dino", "configs", name))
        assert config.decoder_twopass_beam is None and config.decoder_twopass_ctc_weight is None
        config.arch = "vit_tiny"
        model = DINO_Finetune(config)
        assert getattr(model.label_convertor, "twopass_beam", 0) == 0


def test_yaml_keys_reach_the_model(tmp_path):
    from ccd_amd.utils.utils import Config
    from ccd_amd.model.dino_vision import DINO_Finetune
    src = open(os.path.join(ROOT, "Dino", "configs", "CCD_vision_model_ARD.yaml")).read()
    assert "max_seq_len: 25" in src
    (tmp_path / "twopass.yaml").write_text(src.replace("max_seq_len: 25", "max_seq_len: 25, aux_ctc_weight: 0.2, twopass_beam: 8, twopass_ctc_weight: 0.3", 1))
    config = Config(str(tmp_path / "twopass.yaml"))
    assert config.decoder_aux_ctc_weight == 0.2 and config.decoder_twopass_beam == 8 and config.decoder_twopass_ctc_weight == 0.3
    config.arch = "vit_tiny"
    model = DINO_Finetune(config)
    assert (model.label_convertor.twopass_beam, model.label_convertor.twopass_ctc_weight) == (8, 0.3) and model.aux_ctc_weight == 0.2
    (tmp_path / "default.yaml").write_text(src.replace("max_seq_len: 25", "max_seq_len: 25, aux_ctc_weight: 0.2, twopass_beam: 4", 1))
    config = Config(str(tmp_path / "default.yaml"))
    config.arch = "vit_tiny"
    assert DINO_Finetune(config).label_convertor.twopass_ctc_weight == 0.5       # absent: WeNet's default, untuned


def test_command_lines_take_the_two_pass_flags():
    from ccd_amd import decoding_cli
    assert "twopass_beam" in decoding_cli.DECODING_FLAGS and "twopass_ctc_weight" in decoding_cli.DECODING_FLAGS
    for name in SCRIPTS:
        helps, configure = declared(name)
        assert "--twopass_beam" in helps and "--twopass_ctc_weight" in helps, name
        assert "aux_ctc_weight" in helps["--twopass_beam"] and "--joint_ctc_weight" in helps["--twopass_beam"]
        assert "untuned" in helps["--twopass_ctc_weight"]
        assert configure(["--twopass_beam", "8"]) == {"decoder_twopass_beam": 8}
        assert configure(["--twopass_beam", "4", "--twopass_ctc_weight", "0"]) == {"decoder_twopass_beam": 4, "decoder_twopass_ctc_weight": 0.0}
        assert configure([]) == {}


def test_evaluation_and_the_word_helper_take_the_two_pass_branch():
    """TextAccuracy.compute (host path: the stub lives on the CPU) and test.py's decoded_words score rank 0 of forward_twopass when the
    convertor has twopass_beam, and never call it otherwise."""
    import importlib.util
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=25, with_unknown=True, twopass_beam=4)
    paths = torch.full((2, 4, 25), -1, dtype=torch.int32)
    lengths = torch.full((2, 4), -1, dtype=torch.int32)
    scores = torch.full((2, 4), float("-inf"))
    for b, word in enumerate(conv.str2idx(["Hello", "ab"])):
        paths[b, 0, :len(word)] = torch.tensor(word, dtype=torch.int32)
        lengths[b, 0], scores[b, 0] = len(word), -1.0

    class Stub(torch.nn.Module):
        def __init__(self, convertor):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(1))
            self.label_convertor = convertor
            self.calls = []

        def forward_twopass(self, img, beam=None, ctc_weight=None, proposals=None):
            self.calls.append("twopass")
            return paths, lengths, scores

        def forward_beam(self, img, beam_width=None):
            self.calls.append(("beam", beam_width))
            return paths, lengths, scores

    stub = Stub(conv)
    res = TextAccuracy().compute(stub, [(torch.zeros(2, 3, 32, 128), (["hello", "abc"],))])
    assert stub.calls == ["twopass"] and res["words"] == 2 and res["cwr"] == 0.5
    spec = importlib.util.spec_from_file_location("ccd_test_script", os.path.join(ROOT, "test.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    assert script.decoded_words(stub, torch.zeros(2, 3, 32, 128)) == conv.str2idx(["Hello", "ab"]) and stub.calls == ["twopass"] * 2
    plain = Stub(AttnConvertor(dict_type="DICT90", max_seq_len=25, with_unknown=True, beam_width=4))
    script.decoded_words(plain, torch.zeros(2, 3, 32, 128))
    assert plain.calls == [("beam", 4)]
