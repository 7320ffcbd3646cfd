"""Beam search over the NRTR decoder along a lexicon's prefix tree (kernels/nrtr_beam.h: nrtr_beam_step_kernel<true>,
ccd_nrtr_beam_step_trie) under the CPU SIMT executor (tests/hipsim), through the wrappers of ccd_amd.ops.  The same checks run on the
MI355X in tests/test_nrtr_trie_gpu.py; gates: tests/nrtr_trie_checks.py."""
import pytest
import torch

from backends import Backend
import nrtr_trie_checks as K

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_paths_parents_word_ids_and_nodes_equal_the_oracle_sim(sim):
    K.check_oracle(CPU)


def test_a_beam_as_wide_as_the_lexicon_returns_every_word_sim(sim):
    K.check_wide_beam(CPU)


def test_width_one_is_the_constrained_arg_max_chain_sim(sim):
    K.check_width_one(CPU)


def test_masked_allowed_classes_leave_the_sample_unused_sim(sim):
    K.check_masked_sample(CPU)


def test_mask_bits_32_64_127_and_the_class_without_a_bit_sim(sim):
    K.check_boundary_classes(CPU)


def test_argument_validation_sim(sim):
    K.check_arguments(CPU)


def test_beam_decode_walks_the_trie_sim(sim):
    """fe.beam_decode(trie=) through NRTRDecoder.forward_beam on a 1-layer decoder of 6 steps: a lexicon that holds exactly the plain
    beam's three hypotheses (the empty word among them, and class + 1 rows) and a beam as wide leaves nothing to prune, so the same
    sequences come back in the same order - and a slot's logits depend on its own tokens alone, so with the same score bits."""
    import nrtr_trie_np as S
    from ccd_amd.decoder.nrtr_decoder import NRTRDecoder
    torch.manual_seed(2)
    dec = NRTRDecoder(n_layers=1, max_seq_len=6, num_classes=93, start_idx=91, padding_idx=92).eval()
    with torch.no_grad():
        dec.classifier.bias[91] += 1.5                                         # (the hypotheses finish within the six steps)
    out_enc = torch.randn(2, 256, 512, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        paths, lengths, scores = dec.forward_beam(None, out_enc, 3)
    assert int(lengths.min()) >= 0 and int(lengths.max()) < 6 and torch.equal(paths[0], paths[1])
    words = [tuple(paths[0, r, :lengths[0, r]].tolist()) for r in (2, 0, 1)]   # (not in rank order: the ids say which is which)
    assert len(set(words)) == 3
    trie = K.handle_of(words)
    with torch.no_grad():
        got = dec.forward_beam(None, out_enc, 3, trie=trie)
    assert len(got) == 4 and torch.equal(got[0], paths) and torch.equal(got[1], lengths) and torch.equal(got[2], scores)
    assert got[3].dtype == torch.int32 and got[3].tolist() == [[1, 2, 0]] * 2
    assert len(dec._beam_graphs) == 0 and len(dec._trie_graphs) == 0           # (no graphs off the GPU)
    narrow = dec.forward_beam(None, out_enc, 1, trie=K.handle_of(words[:1]))    # the one word of the lexicon, whatever the arg-max says
    assert narrow[3].tolist() == [[0]] * 2 and torch.equal(narrow[0][:, 0], paths[:, 2]) and torch.equal(narrow[2][:, 0], scores[:, 2])
