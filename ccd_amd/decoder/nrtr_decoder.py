"""NRTR transformer decoder behind the reference's module surface (Dino/decoder/nrtr_decoder.py:12-203,
transformer_layers.py:78-164, transformer_module.py:35-147, base_decoder.py).

The nn.Module tree only CARRIES the parameters - same names, shapes, construction order and init RNG stream as the
reference (state dicts and seeds are interchangeable); the computation is ccd_amd.finetune_engine on the HIP kernels.
There is no PyTorch-eager fallback.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from .. import finetune_engine as fe
from ..modules.vision_transformer import ArenaModule, _holder


def sinusoid_table(n_position, d_hid):
    """transformer_module.py:132-145 (same float32 arithmetic: the table is a persistent buffer of the checkpoints)."""
    denominator = torch.Tensor([1.0 / np.power(10000, 2 * (j // 2) / d_hid) for j in range(d_hid)]).view(1, -1)
    table = torch.arange(n_position).unsqueeze(-1).float() * denominator
    table[:, 0::2] = torch.sin(table[:, 0::2])
    table[:, 1::2] = torch.cos(table[:, 1::2])
    return table.unsqueeze(0)


def _mha(d_model, n_head, d_k, d_v):
    # linear_q / linear_k / linear_v / fc, all bias-free (qkv_bias=False): transformer_module.py:64-70
    return _holder(linear_q=nn.Linear(n_head * d_k, n_head * d_k, bias=False),
                   linear_k=nn.Linear(n_head * d_k, n_head * d_k, bias=False),
                   linear_v=nn.Linear(n_head * d_v, n_head * d_v, bias=False),
                   fc=nn.Linear(n_head * d_v, d_model, bias=False))


class _DropoutSeeds:
    """Per-module stream of dropout seeds: host integers derived from torch's seeded generator at first use, so that
    torch.manual_seed() makes a run reproducible without any device-side RNG state."""

    _base = None
    _calls = 0

    def next_dropout_seed(self):
        if self._base is None:
            self._base = int(torch.randint(0, 2 ** 62, (1,)).item())
        self._calls += 1
        return self._base + self._calls * 0x2545F4914F6CDD1D


class Mlp(ArenaModule, _DropoutSeeds):
    """fc1 -> GELU -> Dropout -> fc2 -> Dropout (Dino/model/dino_vision.py:117-132)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        if act_layer is not nn.GELU or in_features % 64 or hidden_features % 64 or out_features % 8:
            raise NotImplementedError("HIP Mlp: GELU, feature counts that are multiples of 64")
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        self.drop_p = float(drop)

    def _transposed_names(self):
        return ["fc1.weight", "fc2.weight"]

    def forward(self, x):
        self.ensure_arena()
        self.drop_p = float(self.drop.p)
        return fe.MlpFn.apply(x.to(torch.bfloat16), self)


class NRTRDecoder(ArenaModule, _DropoutSeeds):
    def __init__(self, n_layers=6, d_embedding=512, n_head=8, d_k=64, d_v=64, d_model=512, d_inner=256, n_position=200,
                 dropout=0.1, num_classes=93, max_seq_len=40, start_idx=1, padding_idx=92, init_cfg=None, **kwargs):
        super().__init__()
        if kwargs or d_embedding != d_model or d_v != d_k:
            raise NotImplementedError("HIP NRTRDecoder covers the shipped configuration: pre-norm layers, "
                                      "d_embedding == d_model, d_v == d_k, qkv_bias=False")
        self.padding_idx, self.start_idx, self.max_seq_len = padding_idx, start_idx, max_seq_len
        # construction order == reference order (nrtr_decoder.py:60-75, transformer_layers.py:112-124)
        self.trg_word_emb = nn.Embedding(num_classes, d_embedding, padding_idx=padding_idx)
        self.position_enc = nn.Module()
        self.position_enc.register_buffer("position_table", sinusoid_table(n_position, d_embedding))
        self.dropout = nn.Dropout(p=dropout)
        self.layer_stack = nn.ModuleList([
            _holder(norm1=nn.LayerNorm(d_model), norm2=nn.LayerNorm(d_model), norm3=nn.LayerNorm(d_model),
                    self_attn=_mha(d_model, n_head, d_k, d_v), enc_attn=_mha(d_model, n_head, d_k, d_v),
                    mlp=_holder(w_1=nn.Linear(d_model, d_inner), w_2=nn.Linear(d_inner, d_model)))
            for _ in range(n_layers)])
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-6)
        self.classifier = nn.Linear(d_model, num_classes - 1)          # <PAD> is never predicted
        self.dec_spec = fe.DecoderSpec(embed_dim=d_model, n_layers=n_layers, d_model=d_model, n_head=n_head, d_k=d_k,
                                       d_inner=d_inner, num_classes=num_classes, max_seq_len=max_seq_len,
                                       start_idx=start_idx, padding_idx=padding_idx, dropout=dropout)
        self.packed = None
        self._graphs = {}
        self.beam_width = 0            # forward_beam's default width (DINO_Finetune sets it from decoder.beam_width); 0: none
        self._beam_graphs = {}
        self._trie_graphs = {}         # forward_beam(trie=): graphs of their own, keyed by the trie as well
        self._joint_graphs = {}        # forward_beam(ctc_frames=): graphs of their own, keyed by the frames' shape and the weight too

    def _transposed_names(self):
        names = []
        for i in range(self.dec_spec.L):
            b = f"layer_stack.{i}."
            names += [b + "self_attn.fc.weight", b + "enc_attn.linear_q.weight", b + "enc_attn.fc.weight",
                      b + "mlp.w_1.weight", b + "mlp.w_2.weight"]
        return names

    @property
    def pos_table(self):
        return self.position_enc.position_table[0]

    def _ready(self):
        self.ensure_arena()
        self.dec_spec.p = float(self.dropout.p)
        if self.packed is None or self.packed.cls.device != self.arena.device:
            self.packed = fe.PackedOperands(self.dec_spec, self.arena.device)

    # ---------------------------------------------------------------------------------- reference surface
    def forward_train(self, feat, out_enc, targets_dict, img_metas=None):
        """out_enc [N,256,D]; targets_dict['padded_targets'] int64 [N,T] -> (logits [N,T,C-1] fp32, attn [N,H,T,256])."""
        if img_metas is not None:
            raise NotImplementedError("valid_ratio masks (img_metas) are not used by DINO_Finetune")
        self._ready()
        targets = targets_dict["padded_targets"].to(out_enc.device).long().contiguous()
        return fe.DecoderFn.apply(out_enc.to(torch.bfloat16), self, targets)

    def forward_test(self, feat, out_enc, img_metas=None):
        self._ready()
        out_enc = out_enc.to(torch.bfloat16)
        if out_enc.is_cuda and os.environ.get("CCD_DECODE_GRAPH", "1") != "0":
            return self._graphed_decode(out_enc)
        return fe.greedy_decode(self, out_enc)

    def _replay(self, graphs, key, decode, out_enc, *more):
        """The 25 decoding steps launch ~1 800 small kernels (6 layers x ~12 kernels per step): launch-bound when issued one
        by one.  The whole loop `decode(input)` is captured ONCE per `key` into a HIP graph, on a single stream, and replayed; the
        graph reads the arena / packed operands in place, so optimizer steps between evaluations need no re-capture.
        `more`: further input tensors of `decode` (dense), each a graph input buffer of its own like out_enc.
        -> the graph's static outputs, which the caller clones."""
        entry = graphs.get(key)
        if entry is None:
            static_in = torch.empty_like(out_enc)
            static_in.copy_(out_enc)
            static_more = tuple(torch.empty_like(t) for t in more)
            for dst, src in zip(static_more, more):
                dst.copy_(src)
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream(device=out_enc.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):                  # warm-up outside the capture (lazy one-time kernel attributes)
                decode(static_in, *static_more)
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = decode(static_in, *static_more)
            if len(graphs) >= 4:                           # a few batch shapes at most (last partial batch, ...)
                graphs.pop(next(iter(graphs)))
            entry = graphs[key] = (graph, static_in, static_out) + static_more
        graph, static_in, static_out = entry[:3]
        static_in.copy_(out_enc)
        for dst, src in zip(entry[3:], more):
            dst.copy_(src)
        graph.replay()
        return static_out

    def _graphed_decode(self, out_enc):
        """One graph per (batch shape, arena)."""
        key = (tuple(out_enc.shape), out_enc.device, self.arena.flat.data_ptr())
        return self._replay(self._graphs, key, lambda x: fe.greedy_decode(self, x), out_enc).clone()

    def forward_beam(self, feat, out_enc, beam_width=None, trie=None, ctc_frames=None, ctc_weight=None):
        """Beam search of width `beam_width` (default: self.beam_width, which must then be > 0) -> (paths int32 [N, W, max_seq_len] by
        rank, -1-padded; lengths int32 [N, W], -1 for an unused slot; scores fp32 [N, W], the log-probability of the word with its
        <EOS>, -inf for an unused slot): fe.beam_decode.  On the GPU the loop is captured into a HIP graph per (batch shape, width) and
        replayed, as forward_test's (CCD_DECODE_GRAPH=0: eager).
        trie: an ops.ctc_lexicon_trie handle (AttnConvertor.lexicon_trie: rows class + 1) - the beam walks the lexicon's prefix tree
        and a fourth tensor comes back, word_ids int32 [N, W]: the lexicon row of every finished hypothesis, -1 for a slot that is
        unused or still a prefix.  The trie's device copy is made before the capture; the graphs of this path are kept apart from
        the plain beam's, one per (batch shape, width, trie).
        ctc_frames: fp32 [N, Tc <= 64, Cc <= 128] logits of an auxiliary CTC head (class c of the decoder is its class c + 1), with
        ctc_weight w in [0, 1] - joint CTC / attention decoding (fe.beam_decode, kernels/nrtr_joint.h): scores are S = (1 - w)
        attention + w CTC and a fourth tensor comes back, att_scores fp32 [N, W], the attention parts.  Excludes a trie.  The frames
        are an input buffer of a graph of their own kind, one per (batch shape, width, frames' shape, weight)."""
        from ..ops import NRTR_MAX_BEAM, CTCLexiconTrie
        if trie is not None and not isinstance(trie, CTCLexiconTrie):
            raise TypeError(f"forward_beam: trie must come from ops.ctc_lexicon_trie, got {type(trie).__name__}")
        if ctc_frames is not None and trie is not None:
            raise ValueError("forward_beam: ctc_frames (joint CTC / attention decoding) excludes a trie")
        if (ctc_frames is None) != (ctc_weight is None):
            raise ValueError("forward_beam: ctc_frames and ctc_weight come together")
        width = int(self.beam_width if beam_width is None else beam_width)
        if not 1 <= width <= NRTR_MAX_BEAM:
            raise ValueError(f"forward_beam: beam_width must lie in 1..{NRTR_MAX_BEAM}, got {width}")
        self._ready()
        out_enc = out_enc.to(torch.bfloat16)
        if trie is not None:
            trie.on(out_enc.device)                        # the upload happens here, never inside a capture
        graphed = out_enc.is_cuda and os.environ.get("CCD_DECODE_GRAPH", "1") != "0"
        if ctc_frames is not None:
            w = float(ctc_weight)
            if ctc_frames.dim() != 3 or ctc_frames.shape[0] != out_enc.shape[0] or ctc_frames.dtype != torch.float32:
                raise ValueError(f"forward_beam: ctc_frames must be float32 [{out_enc.shape[0]}, Tc, Cc], got {ctc_frames.dtype} "
                                 f"{list(ctc_frames.shape)}")
            if not 0.0 <= w <= 1.0:
                raise ValueError(f"forward_beam: ctc_weight must lie in [0, 1], got {ctc_weight!r}")
            if not graphed:
                return fe.beam_decode(self, out_enc, width, ctc_frames=ctc_frames, ctc_weight=w)
            frames = ctc_frames.contiguous()
            key = (tuple(out_enc.shape), out_enc.device, self.arena.flat.data_ptr(), width, tuple(frames.shape), w)
            out = self._replay(self._joint_graphs, key, lambda x, f: fe.beam_decode(self, x, width, ctc_frames=f, ctc_weight=w), out_enc,
                               frames)
            return tuple(t.clone() for t in out)
        if graphed:
            return self._graphed_beam(out_enc, width, trie)
        return fe.beam_decode(self, out_enc, width, trie)

    def _graphed_beam(self, out_enc, width, trie=None):
        """One graph per (batch shape, arena, width) and, with a trie, per trie: the graph holds the address of its device copy, which
        the handle keeps alive as long as the entry keeps the handle."""
        key = (tuple(out_enc.shape), out_enc.device, self.arena.flat.data_ptr(), width)
        if trie is None:
            out = self._replay(self._beam_graphs, key, lambda x: fe.beam_decode(self, x, width), out_enc)
        else:
            out = self._replay(self._trie_graphs, key + (trie,), lambda x: fe.beam_decode(self, x, width, trie), out_enc)
        return tuple(t.clone() for t in out)

    def forward_score(self, feat, out_enc, seq, row_ptr):
        """Teacher-forced scores of given words (fe.score_words): seq int64 [R, max_seq_len + 1] rows `<BOS> chars <EOS> <PAD>..`
        (AttnConvertor.words2rows), row_ptr the CSR table of which image owns which rows (ops.csr_rows handle or host integers) ->
        {'score' [R], 'length' [R], 'char_logp' [R, max_seq_len], 'char_pos' [R, max_seq_len, 4], 'row_ptr' [N + 1]} on the device.
        Eager launches, no HIP graph: the shapes change with the word lists."""
        self._ready()
        return fe.score_words(self, out_enc.to(torch.bfloat16), seq.to(out_enc.device, non_blocking=True), row_ptr)

    def forward_twopass(self, feat, out_enc, frames, paths, lengths, weight, normalized=False):
        """Two-pass decoding (fe.twopass_decode; kernels/nrtr_twopass.h): frames fp32 [N, Tc, Cc] of an auxiliary CTC head (class c + 1
        is the decoder's class c), paths int32 [N, W, Tp] / lengths int32 [N, W] the W words per image a CTC decoder proposes from
        them, in CTC classes, weight w in [0, 1] -> (paths int32 [N, W, max_seq_len] by rank, -1-padded; lengths int32 [N, W]; scores
        fp32 [N, W] = (1 - w) log p_att + w log p_ctc, both parts exact; att_scores, ctc_scores fp32 [N, W]; source int32 [N, W], the
        proposal slot of every rank).  Eager launches, no HIP graph, no host synchronisation."""
        from ..ops import NRTR_MAX_BEAM
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) <= 1.0:
            raise ValueError(f"forward_twopass: weight must lie in [0, 1], got {weight!r}")
        N = out_enc.shape[0]
        if frames.dim() != 3 or frames.shape[0] != N or frames.dtype != torch.float32:
            raise ValueError(f"forward_twopass: frames must be float32 [{N}, Tc, Cc], got {frames.dtype} {list(frames.shape)}")
        if paths.dim() != 3 or paths.shape[0] != N or not 1 <= paths.shape[1] <= NRTR_MAX_BEAM or tuple(lengths.shape) != tuple(paths.shape[:2]):
            raise ValueError(f"forward_twopass: proposals must be paths [{N}, 1..{NRTR_MAX_BEAM}, Tp] with lengths [{N}, W], got "
                             f"{list(paths.shape)} and {list(lengths.shape)}")
        self._ready()
        return fe.twopass_decode(self, out_enc.to(torch.bfloat16), frames, paths, lengths, float(weight), normalized=normalized)

    def forward_test_speed(self, feat, out_enc, img_metas=None):
        self._ready()
        return fe.greedy_decode(self, out_enc.to(torch.bfloat16), stop_on_eos_of_first=True)

    def forward(self, feat, out_enc, targets_dict=None, img_metas=None, train_mode=True, test_speed=False):
        self.train_mode = train_mode
        if train_mode:
            return self.forward_train(feat, out_enc, targets_dict, img_metas)
        if test_speed:
            return self.forward_test_speed(feat, out_enc, img_metas)
        return self.forward_test(feat, out_enc, img_metas)
