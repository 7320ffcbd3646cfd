"""CPU-only checks of the CTC head: the convertor's round trip, the numpy restatement against torch, the class layout."""
import numpy as np
import pytest
import torch

import ctc_checks as K
import ctc_np as R


def test_numpy_restatement_against_torch():
    K.check_numpy_restatement()


def test_convertor_layout_and_round_trip():
    from ccd_amd.convertor.ctc import CTCConvertor
    conv = CTCConvertor(dict_type="DICT90", with_unknown=True, max_seq_len=25)
    assert conv.num_classes() == 92 and conv.blank_idx == 0 and conv.unknown_idx == 91
    assert conv.idx2char[0] == "<BLK>" and conv.idx2char[1] == "0" and conv.idx2char[90] == "~" and conv.idx2char[91] == "<UKN>"
    words = ["hello", "Wor1d!", "aab", "", "x" * 40, "café"]
    t = conv.str2tensor(words)
    assert t.dtype == torch.int64 and tuple(t.shape) == (6, 25)
    assert t[0].tolist() == conv.str2idx(["hello"])[0] + [0] * 20 and (t[3] == 0).all() and (t[4] != 0).all()
    assert t[5, 3].item() == 91 and R.label_lengths(t.numpy()).tolist() == [5, 6, 3, 0, 25, 4]
    # str -> tensor -> one-hot logits with a blank between equal neighbours -> tensor2idx -> str
    logits = torch.full((6, 64, 92), -5.0)
    for b, row in enumerate(t.tolist()):
        frames = []
        for c in row:
            if c:
                frames += [c, c, 0]
        frames += [0] * (64 - len(frames))
        for f, c in enumerate(frames[:64]):
            logits[b, f, c] = 5.0
    idx, scores = conv.tensor2idx(logits)
    assert conv.idx2str(idx) == ["hello", "Wor1d!", "aab", "", "x" * 22, "caf<UKN>"]       # (64 frames: 21 'x x _' triples and one more x)
    assert all(len(a) == len(b) for a, b in zip(idx, scores)) and all(0.99 < s <= 1.0 for row in scores for s in row)
    assert idx[:4] == conv.str2idx(words[:4])
    raw, norm = conv.score_table()
    assert raw.shape == (92, 5) and norm.shape == (92, 3) and (raw[0] == -1).all() and raw[1, 0] == ord("0") and \
        norm[91].tolist() == [ord(c) for c in "ukn"]
    with pytest.raises(KeyError):
        CTCConvertor(with_unknown=False).str2idx(["é"])
    assert CTCConvertor(lower=True).str2idx(["AbC"]) == conv.str2idx(["abc"])


def test_greedy_restatement_matches_tensor2idx():
    from ccd_amd.convertor.ctc import CTCConvertor
    x = K.greedy_case()
    path, length, conf = R.greedy(x.numpy())
    idx, scores = CTCConvertor().tensor2idx(x)
    assert idx == [path[b, :length[b]].tolist() for b in range(len(idx))]
    np.testing.assert_allclose(np.concatenate([conf[b, :length[b]] for b in range(len(idx))]),
                               np.concatenate([np.asarray(s, dtype=np.float32) for s in scores]), rtol=1e-5)


def test_dino_aliases():
    import Dino.convertor.ctc
    import Dino.decoder.ctc_decoder
    import Dino.loss.ctc_loss
    from ccd_amd.convertor import ctc
    assert Dino.convertor.ctc is ctc and Dino.decoder.ctc_decoder.CTCDecoder and Dino.loss.ctc_loss.CTCLoss


def test_head_initialisation_and_config():
    """CTCDecoder: fc.weight trunc-normal std 0.02, fc.bias zeros; decoder.type selects the head, any other value the NRTR recogniser."""
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    torch.manual_seed(0)
    cfg = ft.FinetuneConfig(arch="vit_tiny", drop_path_rate=0.0)
    cfg.decoder_type = "CTCDecoder"
    m = DINO_Finetune(cfg)
    names = [n for n, _ in m.named_parameters()]
    assert [n for n in names if not n.startswith("backbone.")] == ["decoder.fc.weight", "decoder.fc.bias"]
    w = m.decoder.fc.weight.detach()
    assert tuple(w.shape) == (92, 192) and float(w.abs().max()) <= 2.0 and 0.015 < float(w.std()) < 0.025
    assert float(m.decoder.fc.bias.abs().max()) == 0.0 and type(m.label_convertor).__name__ == "CTCConvertor"
    cfg = ft.FinetuneConfig(arch="vit_tiny", decoder_n_layers=1)
    cfg.decoder_type = "NRTRDecoder"
    assert type(DINO_Finetune(cfg).decoder).__name__ == "NRTRDecoder"
    import yaml
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    y = yaml.safe_load(open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_CTC.yaml")))
    ard = yaml.safe_load(open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD.yaml")))
    assert y["decoder"] == {"type": "CTCDecoder", "max_seq_len": 25}
    assert {k: v for k, v in y.items() if k not in ("decoder", "global")} == {k: v for k, v in ard.items() if k not in ("decoder", "global")}
