"""Joint CTC / attention decoding without a GPU: the specification tests/nrtr_joint_np.py against the enumeration of all alignments
and brute force, weight 0 against tests/nrtr_beam_np.py, the share of kernel cases the gap rule drops, and the host side - the
configuration keys, the command-line flag, the state-dict keys of a hybrid model and the CTC targets it derives."""
import itertools
import os

import numpy as np
import pytest
import torch

import nrtr_beam_np as R
import nrtr_joint_np as J
from decoding_flags import SCRIPTS, declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Tc,Cc", [(4, 3), (5, 3), (3, 4)])
def test_recursion_equals_the_enumeration_of_all_alignments(Tc, Cc):
    """psi (the output STARTS with the prefix) and full (the output IS the prefix) of every prefix of up to Tc characters, against
    the sums over all Cc^Tc alignments; difference at most 1e-12."""
    frames = J.frames_of(3, 1, Tc, Cc, pad=0)[0]
    lp = J.frame_log_probs(frames)
    exact = J.enumerate_alignments(lp)
    assert abs(J.lse(list(exact.values()))) <= 1e-12                           # the alignments are all of the probability
    checked = 0
    for n in range(Tc + 1):
        for word in itertools.product(range(1, Cc), repeat=n):
            psi, full = J.prefix_scores(lp, list(word))
            want_full = exact.get(word, -np.inf)
            want_psi = J.lse([p for w, p in exact.items() if w[:n] == word] or [-np.inf])
            for got, want in ((psi, want_psi), (full, want_full)):
                assert (got == want == -np.inf) or abs(got - want) <= 1e-12, (word, got, want)
            checked += 1
    assert checked == sum((Cc - 1) ** n for n in range(Tc + 1))
    long_word = [1] * (Tc // 2 + 1)                                            # repeats need blanks: 2 n - 1 frames
    assert J.prefix_scores(lp, [1] * (Tc + 1)) == (-np.inf, -np.inf) and (2 * len(long_word) - 1 <= Tc or J.prefix_scores(lp, long_word)[1] == -np.inf)


def test_normalized_frames_give_the_log_of_the_row():
    frames = J.frames_of(4, 1, 6, 5, pad=0)[0]
    p = torch.softmax(torch.from_numpy(frames), dim=-1).numpy()
    assert np.abs(J.frame_log_probs(p, normalized=True) - J.frame_log_probs(frames)).max() <= 1e-6
    p[2, 3] = 0.0
    assert J.frame_log_probs(p, normalized=True)[2, 3] == -np.inf


def test_a_wide_beam_returns_every_hypothesis_in_brute_force_order():
    """C = 3, T = 2, Tc = 3, w = 0.5 at W = 16: 7 hypotheses, fewer where the frames cannot spell a word (a repeat needs a blank)."""
    found = 0
    for seed in range(4):
        tab = R.tables(seed + 8, 1, 2, 3)[0]
        frames = J.frames_of(seed, 1, 3, 3, pad=0)[0]
        exact = J.brute_force(tab, frames, 2, 2, 0.5)
        assert 4 <= len(exact) <= 7
        paths, lengths, scores, att, _, gap, _ = J.beam_search(tab, frames, 16, 2, 2, 3, 0.5)
        assert gap >= J.MIN_GAP
        for r, (word, s, a, finished) in enumerate(exact):
            assert paths[r, :lengths[r]].tolist() == list(word) and (lengths[r] < 2) == finished, (seed, r)
            assert abs(scores[r] - s) <= 1e-12 * abs(s) and abs(att[r] - a) <= 1e-12 * abs(a)
        assert (lengths[len(exact):] == -1).all() and np.isneginf(scores[len(exact):]).all()
        found += len(exact)
    assert found >= 20


def test_weight_zero_is_the_plain_beam_bit_for_bit():
    tab = R.tables(7, 3, 25, 92, "end")
    frames = J.frames_of(1, 3, 32, 92, pad=0)
    for b in range(3):
        for W in (1, 4, 16):
            want = R.beam_search(tab[b], W, 91, 91, 92)
            got = J.beam_search(tab[b], frames[b], W, 91, 91, 92, 0.0)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[3])
            assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[2].tobytes() and got[5] == want[4]


def test_the_ctc_term_prunes_words_the_frames_cannot_align():
    """Tc = 1: one frame spells at most one character - every hypothesis of the joint beam has at most one, whatever the attention
    scores say; the plain beam on the same table keeps longer ones."""
    tab = R.tables(7, 1, 6, 5, "flat")[0]
    frames = J.frames_of(2, 1, 1, 5, pad=0)[0]
    paths, lengths, scores, _, _, _, _ = J.beam_search(tab, frames, 8, 4, 4, 5, 0.5)
    assert (lengths <= 1).all() and (lengths >= 0).sum() == 4 + 1              # the four characters and the empty word
    assert (R.beam_search(tab, 8, 4, 4, 5)[1] > 1).any()


def test_few_kernel_cases_are_dropped_by_the_gap_rule():
    import nrtr_joint_checks as K
    assert K.dropped_fraction() <= 0.02


# ------------------------------------------------------------------------------------------------ the host side
def _config(**keys):
    from ccd_amd import finetune as ft
    cfg = ft.FinetuneConfig(arch="vit_tiny", decoder_n_layers=1)
    for k, v in keys.items():
        setattr(cfg, "decoder_" + k, v)
    return cfg


def _keys(**keys):
    from ccd_amd.model.dino_vision import DINO_Finetune
    torch.manual_seed(0)
    return DINO_Finetune(_config(**keys)).state_dict()


def test_hybrid_config_adds_exactly_the_auxiliary_head():
    plain = _keys()
    for absent in (dict(aux_ctc_weight=None), dict(aux_ctc_weight=0), dict(aux_ctc_weight=0.0, joint_ctc_weight=None)):
        sd = _keys(**absent)
        assert list(sd) == list(plain) and all(torch.equal(sd[k], plain[k]) for k in plain), absent
    hybrid = _keys(aux_ctc_weight=0.2)
    assert sorted(set(hybrid) - set(plain)) == ["ctc_decoder.fc.bias", "ctc_decoder.fc.weight"] and not set(plain) - set(hybrid)
    assert tuple(hybrid["ctc_decoder.fc.weight"].shape) == (92, 192) and tuple(hybrid["ctc_decoder.fc.bias"].shape) == (92,)
    assert all(torch.equal(hybrid[k], plain[k]) for k in plain)                # the same init stream for everything else
    from ccd_amd.model.dino_vision import DINO_Finetune
    model = DINO_Finetune(_config(aux_ctc_weight=0.2, joint_ctc_weight=0.3, beam_width=4))
    assert model.ctc is False and model.aux_ctc_weight == 0.2 and model.joint_ctc_weight == 0.3 and model.decoder.beam_width == 4
    assert "ctc_decoder.fc.weight" not in model._transposed_names() and model.last_losses is None


def test_shipped_configurations_build_the_keys_they_built_before():
    from ccd_amd.utils.utils import Config
    from ccd_amd.model.dino_vision import DINO_Finetune
    for name, hybrid in (("CCD_vision_model_ARD.yaml", False), ("CCD_vision_model_ARD_CTC.yaml", False)):
        config = Config(os.path.join(ROOT, "Dino", "configs", name))
        assert config.decoder_aux_ctc_weight is None and config.decoder_joint_ctc_weight is None
        config.arch = "vit_tiny"
        model = DINO_Finetune(config)
        assert not any(k.startswith("ctc_decoder.") for k in model.state_dict()) and model.aux_ctc_weight == 0.0
        assert model.joint_ctc_weight is None


def test_refusals_name_the_missing_key(tmp_path):
    from ccd_amd.model.dino_vision import DINO_Finetune
    words = tmp_path / "words.txt"
    words.write_text("hello\nworld\n", encoding="utf-8")
    for keys, match in ((dict(joint_ctc_weight=0.3, beam_width=4), "needs decoder.aux_ctc_weight"),
                        (dict(aux_ctc_weight=0.2, joint_ctc_weight=0.3), "needs decoder.beam_width"),
                        (dict(aux_ctc_weight=0.2, joint_ctc_weight=0.3, beam_width=0), "needs decoder.beam_width"),
                        (dict(aux_ctc_weight=0.2, joint_ctc_weight=0.3, lexicon=str(words), lexicon_beam=4), "excludes decoder.lexicon"),
                        (dict(aux_ctc_weight=0.2, joint_ctc_weight=1.5, beam_width=4), r"joint_ctc_weight must lie in \[0, 1\]"),
                        (dict(aux_ctc_weight=0.2, joint_ctc_weight=True, beam_width=4), r"joint_ctc_weight must lie in \[0, 1\]"),
                        (dict(aux_ctc_weight=1.0), r"aux_ctc_weight must lie in \[0, 1\)"),
                        (dict(aux_ctc_weight=-0.1), r"aux_ctc_weight must lie in \[0, 1\)"),
                        (dict(aux_ctc_weight="0.2"), r"aux_ctc_weight must lie in \[0, 1\)"),
                        (dict(type="CTCDecoder", joint_ctc_weight=0.3, beam_width=4), "CTCDecoder")):
        with pytest.raises(ValueError, match=match):
            DINO_Finetune(_config(**keys))
    with pytest.raises(ValueError, match="beam_width must lie in 0..16"):
        DINO_Finetune(_config(aux_ctc_weight=0.2, joint_ctc_weight=0.3, beam_width=17))
    ctc = DINO_Finetune(_config(type="CTCDecoder", aux_ctc_weight=0.2))         # a CTC head takes the key and stays what it is
    assert ctc.ctc and ctc.aux_ctc_weight == 0.0 and not any(k.startswith("ctc_decoder.") for k in ctc.state_dict())
    model = DINO_Finetune(_config())
    with pytest.raises(ValueError, match="no auxiliary CTC head"):
        model.forward_ctc(torch.zeros(1, 3, 32, 128))


def test_decoder_refuses_frames_with_a_trie_and_frames_without_a_weight():
    from ccd_amd import finetune_engine as fe, ops
    from ccd_amd.decoder.nrtr_decoder import NRTRDecoder
    dec = NRTRDecoder(n_layers=1, max_seq_len=6, num_classes=93, start_idx=91, padding_idx=92)
    assert dec._joint_graphs == {} and dec._beam_graphs == {} and dec._trie_graphs == {}
    trie = ops.ctc_lexicon_trie(ops.ctc_lexicon(torch.tensor([[3, 4]])))
    out_enc, frames = torch.zeros(1, 256, 512), torch.zeros(1, 32, 92)
    with pytest.raises(ValueError, match="excludes a trie"):
        dec.forward_beam(None, out_enc, 2, trie=trie, ctc_frames=frames, ctc_weight=0.3)
    with pytest.raises(ValueError, match="excludes a trie"):
        fe.beam_decode(dec, out_enc, 2, trie=trie, ctc_frames=frames, ctc_weight=0.3)
    with pytest.raises(ValueError, match="come together"):
        dec.forward_beam(None, out_enc, 2, ctc_frames=frames)
    with pytest.raises(ValueError, match="come together"):
        dec.forward_beam(None, out_enc, 2, ctc_weight=0.3)


def test_command_lines_take_the_joint_weight():
    from ccd_amd import decoding_cli
    assert "joint_ctc_weight" in decoding_cli.DECODING_FLAGS
    for name in SCRIPTS:
        helps, configure = declared(name)
        assert "--joint_ctc_weight" in helps and not helps["--joint_ctc_weight"].startswith("CTC head"), name
        assert "aux_ctc_weight" in helps["--joint_ctc_weight"] and "--beam_width" in helps["--joint_ctc_weight"]
        assert configure(["--joint_ctc_weight", "0.3"]) == {"decoder_joint_ctc_weight": 0.3}
        assert configure(["--joint_ctc_weight", "0", "--beam_width", "4"]) == {"decoder_joint_ctc_weight": 0.0, "decoder_beam_width": 4}
        assert configure([]) == {}


def test_yaml_keys_reach_the_model(tmp_path):
    from ccd_amd.utils.utils import Config
    src = open(os.path.join(ROOT, "Dino", "configs", "CCD_vision_model_ARD.yaml")).read()
    assert "max_seq_len: 25" in src
    (tmp_path / "hybrid.yaml").write_text(src.replace("max_seq_len: 25", "max_seq_len: 25, aux_ctc_weight: 0.2, joint_ctc_weight: 0.3, beam_width: 8", 1))
    config = Config(str(tmp_path / "hybrid.yaml"))
    assert config.decoder_aux_ctc_weight == 0.2 and config.decoder_joint_ctc_weight == 0.3 and config.decoder_beam_width == 8


def test_ctc_targets_of_hand_made_rows():
    """Positions 1 onward, the classes in front of the first <EOS> as class + 1, everything else 0: an empty word, a word cut at
    max_seq_len (no <EOS> in its row), <UKN> (class 90 -> 91), and a row whose padding holds junk behind the <EOS>."""
    from ccd_amd.model.dino_vision import DINO_Finetune
    model = DINO_Finetune(_config(aux_ctc_weight=0.2))
    conv = model.label_convertor
    assert (conv.start_idx, conv.end_idx, conv.padding_idx, conv.unknown_idx) == (91, 91, 92, 90)
    rows = conv.str2tensor(["", "ab", "x" * 40, "aéb"])
    assert tuple(rows.shape) == (4, 25) and rows[0, :3].tolist() == [91, 91, 92] and 91 not in rows[2, 1:].tolist()
    got = model.ctc_targets(rows)
    assert got.dtype == torch.int64 and tuple(got.shape) == (4, 24) and got.is_contiguous()
    assert got[0].tolist() == [0] * 24
    assert got[1].tolist() == [11, 12] + [0] * 22
    assert got[2].tolist() == [34] * 24
    assert got[3].tolist() == [11, 91, 12] + [0] * 21
    junk = rows[1:2].clone()
    junk[0, 4:] = torch.tensor([5, 91, 7] + [92] * 18)                         # behind the first <EOS>: ignored
    assert model.ctc_targets(junk)[0].tolist() == [11, 12] + [0] * 22
    assert int(got.max()) < 92                                                 # within the auxiliary head's 92 classes


def test_a_checkpoint_without_the_head_loads_and_a_hybrid_one_round_trips(caplog):
    import logging
    from ccd_amd.model.dino_vision import DINO_Finetune
    from ccd_amd.parallel import DataParallel
    torch.manual_seed(1)
    plain = DINO_Finetune(_config())
    torch.manual_seed(2)
    hybrid = DINO_Finetune(_config(aux_ctc_weight=0.2))
    head = {k: v.clone() for k, v in hybrid.state_dict().items() if k.startswith("ctc_decoder.")}
    with caplog.at_level(logging.INFO):
        hybrid.load_state_dict(plain.state_dict())
    assert sum("no auxiliary CTC head" in r.getMessage() for r in caplog.records) == 1
    sd = hybrid.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in plain.state_dict().items()) and all(torch.equal(sd[k], v) for k, v in head.items())
    caplog.clear()
    torch.manual_seed(3)
    other = DataParallel(DINO_Finetune(_config(aux_ctc_weight=0.2)))            # the `module.` prefix of the training script
    with caplog.at_level(logging.INFO):
        other.load_state_dict({"module." + k: v for k, v in sd.items()})
    assert not caplog.records and all(torch.equal(other.state_dict()["module." + k], v) for k, v in sd.items())
    with caplog.at_level(logging.INFO):
        other.load_state_dict({"module." + k: v for k, v in plain.state_dict().items()})
    assert sum("no auxiliary CTC head" in r.getMessage() for r in caplog.records) == 1
    with pytest.raises(RuntimeError, match="ctc_decoder"):                     # the reverse stays an error: a head nobody owns
        plain.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="ctc_decoder.fc.bias"):             # and half a head is no head
        hybrid.load_state_dict({k: v for k, v in sd.items() if k != "ctc_decoder.fc.bias"})
