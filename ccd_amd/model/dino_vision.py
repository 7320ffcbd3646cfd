"""ABIDINOModel: dual-view backbone + segmentation head + character-region pooling + DINO head
(Dino/model/dino_vision.py:21-115), MI355X-native.

Differences from the reference that are invisible at the boundary:
  * the character clusters live on the device as uint8 id maps (ccd_amd.engine.Selection) - the host-side
    numpy/skimage labelling loop (dino_vision.py:59-71) is the HIP kernel ccl_label_kernel;
  * the number of selected character rows M never reaches the host: 'instances_view' is backed by a worst-case
    buffer and only materialises a [2M, K] tensor if somebody indexes the output dict for it.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn

from .. import engine, ops
from ..modules.vision_transformer import ArenaModule
from ..utils.DBSCAN import DBSCAN_cluster, label_cluster

# the reference's module-level clusterers (dino_vision.py:18-19); constructing them does not touch the GPU.  ABIDINOModel itself
# keeps its character regions on the device as id maps (ops.ccl_label) and does not go through these.
dbscan = DBSCAN_cluster(eps=1.5, min_samples=4)
label = label_cluster()


AUX_CTC_CLASSES = 92             # the auxiliary CTC head of the hybrid model: the blank, DICT90's 90 characters, <UKN>


def _absent(value, default):
    """A key the YAML leaves out reads as None: the default then; 0 and False are values."""
    return default if value is None else value


class ClusterMaps:
    """What the student hands to the teacher as `clusters=` (reference: a dense [2B,26,32,128] tensor)."""

    def __init__(self, selection: engine.Selection):
        self.selection = selection

    def dense(self):
        return self.selection.dense()

    # a little tensor-likeness for callers that only look at the shape / move it around
    @property
    def shape(self):
        return torch.Size((2 * self.selection.batch, 26, 32, 128))

    def to(self, *a, **k):
        return self


class ModelOutput(dict):
    """Output dict whose reference-shaped entries are produced lazily (they need a host sync on M)."""

    def __init__(self, eager, lazy):
        super().__init__(eager)
        self._lazy = lazy

    def __getitem__(self, key):
        if key not in self.keys() and key in self._lazy:
            super().__setitem__(key, self._lazy[key]())
        return super().__getitem__(key)

    def __contains__(self, key):
        return super().__contains__(key) or key in self._lazy

    def raw(self, key, default=None):
        return super().get(key, default)


class ABIDINOModel(ArenaModule):
    def __init__(self, backbone, Segmentation, head):
        super().__init__()
        backbone.fc, backbone.head = nn.Identity(), nn.Identity()
        self.backbone = backbone
        self.segmentation = Segmentation
        self.head = head

    # ------------------------------------------------------------------------------------------- arena
    def _transposed_names(self):
        return ["backbone." + n for n in self.backbone._transposed_names()] + \
               ["head." + n for n in self.head._transposed_names()]

    def attach_arena(self, arena, prefix):
        super().attach_arena(arena, prefix)
        self.backbone.attach_arena(arena, prefix + "backbone.")
        self.head.attach_arena(arena, prefix + "head.")

    def unused_parameter_names(self):
        """Parameters that never take part in the forward pass (reference: their .grad stays None, so AdamW and the
        DDP reducer ignore them - 19 tensors, the reason for find_unused_parameters=True at train.py:106)."""
        pre = self.arena_prefix
        names = [pre + "backbone.cls_token"]
        names += [pre + n for n, _ in self.named_parameters() if n.startswith("segmentation.conv_mla.")]
        return names

    # ---------------------------------------------------------------------------------------- sub-steps
    def _pooled_logits(self, tokens, sel):
        rows = engine.RegionPoolFn.apply(tokens, sel)
        # (lazy: the head may leave its last product to the loss - engine.LazyLogits, ccd_head_loss_fwd / _bwd)
        return self.head.forward_rows(rows, sel.total, lazy=True)

    def attention(self, feature, clusters):
        """Reference-shaped helper (dino_vision.py:38-49): feature [N,E,8,32], clusters [N,26,32,128] -> ([N,26,E], index)."""
        n, e = feature.shape[0], feature.shape[1]
        idmap = ops.planes_to_idmap(clusters)
        tok_plane, tok_coef, present = ops.region_stats(idmap)
        tokens = feature.permute(0, 2, 3, 1).reshape(n, 256, e).float()
        onehot = (tok_plane.long().unsqueeze(-1) == torch.arange(26, device=feature.device)).float()
        w = onehot * tok_coef.unsqueeze(-1)                                  # [N,256,26], tiny glue for API parity
        return torch.bmm(w.transpose(1, 2), tokens), present.bool()

    def backbone_tokens(self, x):
        """Final-norm tokens of both views [2B,256,E] (no taps): the teacher's backbone pass on its own, so that it can be
        enqueued before the student's clusters exist (pretrain._forward_backward with a CU partition)."""
        self.ensure_arena()
        tokens, = self.backbone.tokens_and_taps(torch.cat([x[:, 1], x[:, 2]]), need_taps=False)
        return tokens

    def forward(self, x, metrics, target_mask, epoch, clusters=None, index=None, tokens=None):
        self.ensure_arena()
        B = x.shape[0]
        if tokens is None:
            views = torch.cat([x[:, 1], x[:, 2]])
            tokens, *taps = self.backbone.tokens_and_taps(views, need_taps=clusters is None)
        else:
            assert clusters is not None, "precomputed tokens are the teacher's (no segmentation taps)"
        if clusters is None:
            seg_in = [self.backbone.to_2D(t) for t in taps]
            seg = self.segmentation(seg_in)                                    # [2B,2,32,128] fp32
            if epoch < 30:
                mask = target_mask.contiguous().float()
            else:
                mask = ops.seg_to_mask(seg.detach().contiguous(), B)
            ids_src = ops.ccl_label(mask)
            ids_img = ops.warp_idmap(ids_src, metrics.contiguous().float())
            sel = engine.Selection(torch.cat([ids_src, ids_img]), B)
            logits = self._pooled_logits(tokens, sel)
            return ModelOutput(
                {"mask": seg, "image": x, "zero": ClusterMaps(sel), "logits_buf": logits, "selection": sel},
                {"instances_view": lambda: engine.logits_tensor(logits)[: 2 * sel.M], "index": lambda: sel.new_index.bool()})
        sel = clusters.selection if isinstance(clusters, ClusterMaps) else \
            engine.Selection(ops.planes_to_idmap(clusters), B)
        logits = self._pooled_logits(tokens, sel)
        return ModelOutput({"logits_buf": logits, "selection": sel},
                           {"instances_view": lambda: engine.logits_tensor(logits)[: 2 * sel.M],
                            "feature": lambda: self.backbone.to_2D(tokens).float()})


# ------------------------------------------------------------------------------------------------ segmentation finetune
class DINO_Segment(ArenaModule):
    """Text segmenter of the segmentation finetune stage (no reference counterpart: the reference names the task - its data tree
    holds TextSeg - and ships no training code for it): the pretrained ViT backbone and the pretrained character-region head,
    trained on image / mask pairs under SegSupLoss.  The module names are the pretraining model's, so the `module.backbone.*` and
    `module.segmentation.*` entries of a pretraining checkpoint load as they are.
    config: `arch`, `patch_size`, `drop_path_rate` as DINO_Finetune reads them, and the `seg_loss:` block - class_weight (1, 1),
    ignore_index 255, dice_weight 0, edge_weight 0, edge_radius 0 (ccd_amd/loss/seg_loss.py).
    Training runs the head in train mode (batch statistics; one rank: the SyncBatchNorm exchange of a supervised run is not part of
    this model's scripts), `forward_test` / `forward_mask` normalise by the running statistics (seghead.seg_head_inference)."""

    last_logits = None                 # the logits of the last forward_train, fp32 [N, 2, 32, 128], detached

    def __init__(self, config):
        super().__init__()
        from ..modules import vision_transformer as vits
        config.arch = config.arch.replace("deit", "vit")
        if config.arch not in vits.__dict__:
            raise NotImplementedError(f"Unknow architecture: {config.arch} (HIP kernels cover vit_tiny / vit_small / vit_base)")
        self.backbone = vits.__dict__[config.arch](patch_size=config.patch_size, drop_path_rate=_absent(config.drop_path_rate, 0.0))
        taps = self.backbone.out_indices
        if len(taps) != 3 or not all(1 <= t <= len(self.backbone.blocks) for t in taps):
            raise ValueError(f"DINO_Segment: the segmentation head reads three taps inside the backbone, got out_indices {taps} for "
                             f"{len(self.backbone.blocks)} blocks")
        # nothing reads the stream behind the last tap (the stock architectures tap blocks 2, 4, 6 of 12): the passes stop there.  The
        # blocks behind it keep their parameters (a pretraining checkpoint loads and saves whole) and the blocks in front keep the
        # DropPath rates of the full depth.
        spec, last = self.backbone.spec, max(taps)
        if last < spec.depth:
            cut = engine.VitSpec(spec.E, last, spec.heads, spec.taps, spec.patch, spec.eps)
            cut.dpr = list(spec.dpr[:last])
            self.backbone.spec = cut
        self._build_task(config)

    def _build_task(self, config):
        """The head and the loss (DINO_SuperRes builds its own on the same backbone)."""
        from ..loss.seg_loss import SegSupLoss
        from ..modules.segmentor import SegHead
        self.segmentation = SegHead(in_channels=self.backbone.embed_dim, mla_channels=128, mlahead_channels=64, num_classes=2)
        g = lambda k, d: _absent(getattr(config, "seg_loss_" + k, None), d)
        self.loss = SegSupLoss(class_weight=g("class_weight", (1.0, 1.0)), ignore_index=g("ignore_index", 255),
                               dice_weight=g("dice_weight", 0.0), edge_weight=g("edge_weight", 0.0), edge_radius=g("edge_radius", 0))

    # ------------------------------------------------------------------------------------------- arena
    def _transposed_names(self):
        return ["backbone." + n for n in self.backbone._transposed_names()]

    def attach_arena(self, arena, prefix):
        super().attach_arena(arena, prefix)
        self.backbone.attach_arena(arena, prefix + "backbone.")

    def unused_parameter_names(self):
        """Parameters this forward pass never reads, so that the optimiser leaves them alone (no weight decay on tensors without a
        gradient): cls_token and the head's conv_mla branch as in pretraining, and what lies behind the last tap - the final norm and,
        for the stock architectures (taps behind blocks 2, 4, 6 of 12), the blocks after it."""
        pre = self.arena_prefix
        last = max(self.backbone.out_indices)
        names = [pre + "backbone.cls_token", pre + "backbone.norm.weight", pre + "backbone.norm.bias"]
        for n, _ in self.named_parameters():
            if n.startswith("segmentation.conv_mla.") or (n.startswith("backbone.blocks.") and int(n.split(".")[2]) >= last):
                names.append(pre + n)
        return names

    # ------------------------------------------------------------------------------------------- surface
    def forward(self, img, gt=None, return_loss=True):
        if return_loss:
            return self.forward_train(img, gt)
        return self.forward_test(img)

    def _taps(self, img):
        self.ensure_arena()
        _, *taps = self.backbone.tokens_and_taps(img, need_taps=True)
        n, e = img.shape[0], self.backbone.embed_dim
        return [t.reshape(n * 256, e) for t in taps], n

    def forward_train(self, img, gt):
        """img fp32 [N, 3, 32, 128], gt uint8 [N, 32, 128] (0 background, 1 text, ignore_index not scored) -> the loss (a device
        scalar); the gradient flows through the head into the three taps of the backbone.  `loss.last_parts` / `loss.last_confusion`
        keep the parts and the batch's confusion matrix, `last_logits` the logits."""
        from ..seghead import seg_head_forward
        taps, n = self._taps(img)
        logits = seg_head_forward(self.segmentation, taps, n)
        self.last_logits = logits.detach()
        return self.loss(logits, gt)

    @torch.no_grad()
    def forward_test(self, img):
        """img fp32 [N, 3, 32, 128] -> eval-mode logits fp32 [N, 2, 32, 128]: no DropPath, BatchNorm by running statistics, whatever
        mode the model is in; no statistic is updated."""
        from ..seghead import seg_head_inference
        was = self.backbone.training
        self.backbone.eval()
        try:
            taps, n = self._taps(img)
        finally:
            self.backbone.train(was)
        return seg_head_inference(self.segmentation, taps, n)

    @torch.no_grad()
    def forward_mask(self, img):
        """-> (mask uint8 [N, 32, 128]: 1 where logit1 > logit0, a tie is background as in torch.argmax; prob fp32 [N, 32, 128] =
        softmax(logits)[:, 1])."""
        logits = self.forward_test(img)
        # (two elementwise views of the logits; ops.seg_to_mask thresholds the rounded softmax, which is not the tie rule)
        return (logits[:, 1] > logits[:, 0]).to(torch.uint8), torch.sigmoid(logits[:, 1] - logits[:, 0])


# ------------------------------------------------------------------------------------------------ super-resolution finetune
class DINO_SuperRes(DINO_Segment):
    """Text image super-resolver of the super-resolution finetune stage (no reference counterpart: the reference names the task - its
    data tree holds Super_Resolution - and ships the metrics, no training code): DINO_Segment's backbone (cut at the last tap, the
    same unused parameters) under the pretrained MLA head, whose last convolution writes a residual image instead of two logits:

        base = bicubic_x2(lr)                       fp32 [N, 3, 32, 128] from lr [N, 3, 16, 64] in [0, 1] (ops.sr_upsample)
        sr   = base + segmentation((base - MEAN) / STD)

    The head keeps the attribute name `segmentation`, so the `module.backbone.*` and `module.segmentation.*` entries of a
    pretraining checkpoint load as they are - except `segmentation.cls.*`, which has three output channels here and starts at zero:
    sr = base bit for bit at initialisation.  Training uses the unclamped sr under SRLoss; `forward_sr` returns clamp(sr, 0, 1).
    config: `arch`, `patch_size`, `drop_path_rate`, and the `sr_loss:` block - gp_weight 1e-4, ssim_weight 0 (ccd_amd/loss/sr_loss.py)."""

    LR_SIZE, HR_SIZE = ops.SR_LR_SIZE, ops.SR_HR_SIZE
    last_sr = None                     # the unclamped sr of the last forward_train, fp32 [N, 3, 32, 128], detached

    def _build_task(self, config):
        from ..loss.sr_loss import SRLoss
        from ..modules.segmentor import SegHead
        self.segmentation = SegHead(in_channels=self.backbone.embed_dim, mla_channels=128, mlahead_channels=64, num_classes=3)
        nn.init.zeros_(self.segmentation.cls.weight)
        nn.init.zeros_(self.segmentation.cls.bias)
        g = lambda k, d: _absent(getattr(config, "sr_loss_" + k, None), d)
        self.loss = SRLoss(gp_weight=g("gp_weight", 1e-4), ssim_weight=g("ssim_weight", 0.0))

    def forward(self, lr, hr=None, return_loss=True):
        if return_loss:
            return self.forward_train(lr, hr)
        return self.forward_sr(lr)

    def upsample(self, lr):
        """lr fp32 [N, 3, 16, 64] -> (base, the normalised network input), both fp32 [N, 3, 32, 128]."""
        from ..dataset.datasetsupervised_kmeans import MEAN, STD
        if lr.dim() != 4 or tuple(lr.shape[1:]) != (3, *self.LR_SIZE):
            raise ValueError(f"DINO_SuperRes: lr must be [N, 3, {self.LR_SIZE[0]}, {self.LR_SIZE[1]}] (TextZoom's sizes), got {list(lr.shape)}")
        self.ensure_arena()               # (a model or batch that is not on the GPU is refused here: there is no CPU path)
        return ops.sr_upsample(lr.float(), MEAN, STD)

    def forward_train(self, lr, hr):
        """lr fp32 [N, 3, 16, 64], hr fp32 [N, 3, 32, 128], both in [0, 1] -> the loss (a device scalar) of the unclamped sr; the
        gradient flows through the head into the three taps of the backbone.  `loss.last_parts` / `loss.last_mse` keep the parts."""
        from ..seghead import sr_head_forward
        if hr is None or hr.dim() != 4 or tuple(hr.shape[1:]) != (3, *self.HR_SIZE) or hr.shape[0] != lr.shape[0]:
            raise ValueError(f"DINO_SuperRes: hr must be [N, 3, {self.HR_SIZE[0]}, {self.HR_SIZE[1]}] with lr's N, got "
                             f"{None if hr is None else list(hr.shape)}")
        base, xin = self.upsample(lr)
        taps, n = self._taps(xin)
        sr = sr_head_forward(self.segmentation, taps, n, base)
        self.last_sr = sr.detach()
        return self.loss(sr, hr.float())

    @torch.no_grad()
    def forward_sr(self, lr, clamp=True):
        """lr fp32 [N, 3, 16, 64] -> sr fp32 [N, 3, 32, 128] clamped to [0, 1]: eval mode whatever mode the model is in - no DropPath,
        BatchNorm by running statistics, no statistic updated."""
        from ..seghead import sr_head_inference
        base, xin = self.upsample(lr)
        was = self.backbone.training
        self.backbone.eval()
        try:
            taps, n = self._taps(xin)
        finally:
            self.backbone.train(was)
        sr = sr_head_inference(self.segmentation, taps, n, base)
        return sr.clamp_(0.0, 1.0) if clamp else sr

    forward_test = forward_sr

    def forward_mask(self, img):
        raise NotImplementedError("DINO_SuperRes writes images, not masks: forward_sr")


# ------------------------------------------------------------------------------------------------ finetune
class DINO_Finetune(ArenaModule):
    """Text recogniser of the finetune stage (Dino/model/dino_vision.py:134-290): ViT backbone -> Mlp "encoder" ->
    NRTR decoder -> TFLoss.  Same constructor (a config object), parameter names and init RNG order as the reference.
    `decoder.type: 'CTCDecoder'` builds the CTC head instead (no reference counterpart): backbone -> CTCDecoder (frame pooling + one
    linear layer) -> CTCLoss, with a CTCConvertor; there is no `encoder` Mlp then.  `decoder.beam_width` > 0 makes evaluation decode by
    CTC prefix beam search of that width (absent or 0: the greedy rule); `decoder.lexicon: <path>` makes it pick the most probable word
    of that word list instead.  Any other type builds the NRTR recogniser; there
    `decoder.beam_width` > 0 is the width of `forward_beam` (beam search over the attention decoder: n-best words with their
    log-probabilities), which TextAccuracy then scores the best word of, and `decoder.lexicon: <path>` together with
    `decoder.lexicon_beam: N` (1..16; either alone is refused) makes evaluation decode over that word list instead: `forward_lexicon`,
    a beam of width N along the lexicon's prefix tree.  `forward_test` and `forward_test_speed` return the greedy
    probabilities whatever the width: a beam has no per-step distribution to return.
    `decoder.aux_ctc_weight: a`, 0 < a < 1, on the NRTR recogniser makes it the hybrid CTC / attention model: an auxiliary
    `ctc_decoder = CTCDecoder(embed_dim, 92)` on the same backbone tokens, trained under (1 - a) TFLoss + a CTCLoss (the parts:
    `last_losses`), read through `forward_ctc`; absent or 0 is the model without it, key for key.  `decoder.joint_ctc_weight: w` in
    [0, 1] - it needs that head and `decoder.beam_width` in 1..16, and excludes a lexicon - makes `forward_beam` rescore every
    candidate with the CTC prefix probability of its characters (kernels/nrtr_joint.h).  `decoder.twopass_beam: N` (1..16, with
    `decoder.twopass_ctc_weight: w` in [0, 1], default 0.5) needs that head too and excludes the three other decoders: evaluation
    scores rank 0 of `forward_twopass` - the CTC beam proposes N words, the decoder rescores them in one pass (kernels/nrtr_twopass.h).
    `decoder.type: 'ParallelAttnDecoder'` builds the reference's parallel attention head (Dino/modules/attention.py `Attention` + `cls`):
    backbone -> ParallelAttnDecoder on the backbone tokens -> TFLoss, with an AttnConvertor and no `encoder` Mlp.  It decodes greedily in
    one pass: `forward_train` returns (loss, attn [N, T, 8, 32]), `forward_test` the probabilities, `forward_attn` both; every other
    decoder's key and method is refused with a ValueError that names the head."""

    aux_ctc_weight = 0.0               # decoder.aux_ctc_weight; > 0: the model owns ctc_decoder and ctc_loss
    joint_ctc_weight = None            # decoder.joint_ctc_weight; a number: forward_beam decodes jointly
    last_losses = None                 # hybrid: {'tf', 'ctc'}, the two parts of the last forward_train as device scalars
    last_att_scores = None             # joint decoding: the attention scores of the last forward_beam, fp32 [N, W]; two-pass too
    last_ctc_scores = None             # two-pass decoding: the CTC scores of the last forward_twopass, fp32 [N, W]
    last_sources = None                # ... and the proposal slot of every rank, int32 [N, W]

    def __init__(self, config):
        super().__init__()
        self.ctc = getattr(config, "decoder_type", None) == "CTCDecoder"
        self.par = getattr(config, "decoder_type", None) == "ParallelAttnDecoder"
        if self.par:
            self._init_par(config)
            return
        aux, joint = self._checked_hybrid_keys(config)
        twopass = self._checked_twopass_keys(config, aux, joint)
        if self.ctc:
            self._init_ctc(config)
            return
        from ..convertor.attn import AttnConvertor
        from ..decoder.nrtr_decoder import Mlp, NRTRDecoder
        from ..loss.ce_loss import TFLoss
        from ..modules import vision_transformer as vits
        self.label_convertor = AttnConvertor(dict_type='DICT90', max_seq_len=config.decoder_max_seq_len, with_unknown=True,
                                             beam_width=int(getattr(config, "decoder_beam_width", 0) or 0),     # absent or 0: greedy
                                             lexicon=getattr(config, "decoder_lexicon", None) or None,          # absent: no lexicon; with
                                             lexicon_beam=int(getattr(config, "decoder_lexicon_beam", 0) or 0),  # its beam (alone: refused)
                                             lm=getattr(config, "decoder_lm", None) or None,                    # (refused as well)
                                             twopass_beam=twopass[0], twopass_ctc_weight=twopass[1])            # absent: 0, None
        config.arch = config.arch.replace("deit", "vit")
        if config.arch not in vits.__dict__:
            raise NotImplementedError(f"Unknow architecture: {config.arch} (HIP kernels cover vit_tiny / vit_small / vit_base)")
        self.backbone = vits.__dict__[config.arch](patch_size=config.patch_size, drop_path_rate=config.drop_path_rate)
        embed_dim = self.backbone.embed_dim
        self.encoder = Mlp(in_features=embed_dim, hidden_features=512, out_features=512, act_layer=nn.GELU, drop=0.1)
        config.decoder_num_classes = self.label_convertor.num_classes()
        config.decoder_start_idx = self.label_convertor.start_idx
        config.decoder_padding_idx = self.label_convertor.padding_idx
        self.decoder = NRTRDecoder(
            n_layers=config.decoder_n_layers, d_embedding=config.decoder_d_embedding, n_head=config.decoder_n_head,
            d_k=config.decoder_d_k, d_v=config.decoder_d_v, d_model=config.decoder_d_model, d_inner=config.decoder_d_inner,
            n_position=200, dropout=0.1, num_classes=config.decoder_num_classes, max_seq_len=config.decoder_max_seq_len,
            start_idx=config.decoder_start_idx, padding_idx=config.decoder_padding_idx)
        self.decoder.beam_width = self.label_convertor.beam_width
        self.loss = TFLoss(ignore_index=self.label_convertor.padding_idx)
        if joint is not None and self.label_convertor.lexicon is not None:
            raise ValueError("decoder.joint_ctc_weight excludes decoder.lexicon / decoder.lexicon_beam: joint decoding along a lexicon's "
                             "prefix tree is not implemented")
        if joint is not None and self.label_convertor.beam_width < 1:
            raise ValueError("decoder.joint_ctc_weight needs decoder.beam_width in 1..16: the CTC prefix scores rescore a beam")
        if aux > 0:                                        # (built last: the init RNG stream of everything above is the plain model's)
            from ..decoder.ctc_decoder import CTCDecoder
            from ..loss.ctc_loss import CTCLoss
            self.ctc_decoder = CTCDecoder(in_features=embed_dim, num_classes=AUX_CTC_CLASSES)
            self.ctc_loss = CTCLoss(blank=0, zero_infinity=True)
        self.aux_ctc_weight, self.joint_ctc_weight = aux, joint

    @staticmethod
    def _checked_joint_weight(w):
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= float(w) <= 1.0:
            raise ValueError(f"decoder.joint_ctc_weight must lie in [0, 1], got {w!r}")
        return float(w)

    def _checked_hybrid_keys(self, config):
        """(decoder.aux_ctc_weight, absent: 0; decoder.joint_ctc_weight, absent: None), checked against each other and the head."""
        aux, joint = getattr(config, "decoder_aux_ctc_weight", None), getattr(config, "decoder_joint_ctc_weight", None)
        aux = 0.0 if aux is None else aux
        if isinstance(aux, bool) or not isinstance(aux, (int, float)) or not 0.0 <= float(aux) < 1.0:
            raise ValueError(f"decoder.aux_ctc_weight must lie in [0, 1) (0: no auxiliary CTC head), got {aux!r}")
        if joint is not None:
            joint = self._checked_joint_weight(joint)
        if self.ctc:                                       # a CTC head is the CTC model already: the auxiliary weight means nothing there
            if joint is not None:
                raise ValueError("decoder.joint_ctc_weight rescores the NRTR decoder's beam: decoder.type 'CTCDecoder' has none")
            return 0.0, None
        if joint is not None and not aux > 0:
            raise ValueError("decoder.joint_ctc_weight needs decoder.aux_ctc_weight > 0: the auxiliary CTC head gives the prefix scores")
        return float(aux), joint

    def _checked_twopass_keys(self, config, aux, joint):
        """(decoder.twopass_beam, absent: 0; decoder.twopass_ctc_weight, absent: None - the convertor's default), checked against the
        head and the other decoders' keys."""
        beam, weight = getattr(config, "decoder_twopass_beam", None), getattr(config, "decoder_twopass_ctc_weight", None)
        if not beam and weight is None:                    # (a weight without a beam: the convertor refuses it)
            return 0, None
        if self.ctc:
            raise ValueError("decoder.twopass_beam / decoder.twopass_ctc_weight rescore CTC proposals with the NRTR decoder: decoder.type "
                             "'CTCDecoder' has none")
        if beam:
            if not aux > 0:
                raise ValueError("decoder.twopass_beam needs decoder.aux_ctc_weight > 0: the auxiliary CTC head proposes the words")
            if int(getattr(config, "decoder_beam_width", 0) or 0) > 0:
                raise ValueError("decoder.twopass_beam excludes decoder.beam_width > 0: the proposals come from the CTC beam of width "
                                 "twopass_beam, and one decoder is scored")
            if getattr(config, "decoder_lexicon", None) or getattr(config, "decoder_lexicon_beam", None):
                raise ValueError("decoder.twopass_beam excludes decoder.lexicon / decoder.lexicon_beam: rescoring a lexicon's proposals "
                                 "goes through forward_twopass(proposals=)")
            if joint is not None:
                raise ValueError("decoder.twopass_beam excludes decoder.joint_ctc_weight: joint decoding rescores inside the attention "
                                 "beam, two-pass decoding behind the CTC beam")
        return beam, weight

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A checkpoint of the NRTR recogniser alone loads into the hybrid model: the auxiliary CTC head stays as it was initialised."""
        keys = [prefix + "ctc_decoder.fc.weight", prefix + "ctc_decoder.fc.bias"]
        if self.aux_ctc_weight > 0 and not any(k in state_dict for k in keys):
            logging.info("the checkpoint holds no auxiliary CTC head (ctc_decoder.fc.*): it stays at its initialisation")
            state_dict[keys[0]], state_dict[keys[1]] = self.ctc_decoder.fc.weight.detach(), self.ctc_decoder.fc.bias.detach()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    _PAR_REFUSED_KEYS = ("beam_width", "lexicon", "lexicon_beam", "lm", "aux_ctc_weight", "joint_ctc_weight", "twopass_beam")

    def _init_par(self, config):
        """decoder.type 'ParallelAttnDecoder': the head decodes greedily in one pass and has no other decoder's machinery."""
        from ..convertor.attn import AttnConvertor
        from ..decoder.parallel_attn_decoder import ParallelAttnDecoder
        from ..loss.ce_loss import TFLoss
        from ..modules import vision_transformer as vits
        for key in self._PAR_REFUSED_KEYS:
            if getattr(config, "decoder_" + key, None):
                raise ValueError(f"decoder.{key} is not for decoder.type 'ParallelAttnDecoder': the parallel attention head decodes greedily "
                                 "in one pass (no beam, lexicon, language model, auxiliary CTC head, joint or two-pass decoding)")
        self.label_convertor = AttnConvertor(dict_type='DICT90', max_seq_len=config.decoder_max_seq_len or 25, with_unknown=True)
        config.arch = config.arch.replace("deit", "vit")
        if config.arch not in vits.__dict__:
            raise NotImplementedError(f"Unknow architecture: {config.arch} (HIP kernels cover vit_tiny / vit_small / vit_base)")
        self.backbone = vits.__dict__[config.arch](patch_size=config.patch_size, drop_path_rate=config.drop_path_rate)
        config.decoder_num_classes = self.label_convertor.num_classes()
        self.decoder = ParallelAttnDecoder(in_features=self.backbone.embed_dim, num_classes=config.decoder_num_classes,
                                           max_seq_len=config.decoder_max_seq_len or 25)
        self.loss = TFLoss(ignore_index=self.label_convertor.padding_idx)

    def _par_refuses(self, method):
        if self.par:
            raise ValueError(f"{method} is not for decoder.type 'ParallelAttnDecoder': the parallel attention head decodes greedily in one "
                             "pass (forward_test, forward_attn)")

    @torch.no_grad()
    def forward_attn(self, img):
        """The parallel attention head: img [N,3,32,128] -> (probabilities fp32 [N, T, C], attention maps fp32 [N, T, 8, 32])."""
        if not self.par:
            raise ValueError("forward_attn is the parallel attention head's (decoder.type: 'ParallelAttnDecoder')")
        logits, attn = self.decoder.forward_train(self.extract_feat(img))
        return logits.softmax(dim=-1), attn

    def _init_ctc(self, config):
        from ..convertor.ctc import CTCConvertor
        from ..decoder.ctc_decoder import CTCDecoder
        from ..loss.ctc_loss import CTCLoss
        from ..modules import vision_transformer as vits
        self.label_convertor = CTCConvertor(dict_type='DICT90', max_seq_len=config.decoder_max_seq_len or 25, with_unknown=True,
                                            beam_width=int(getattr(config, "decoder_beam_width", 0) or 0),     # absent or 0: greedy
                                            lexicon=getattr(config, "decoder_lexicon", None) or None,          # absent: no lexicon
                                            lexicon_beam=int(getattr(config, "decoder_lexicon_beam", 0) or 0), # absent or 0: every word
                                            lm=getattr(config, "decoder_lm", None) or None,                    # absent: no language model
                                            lm_order=_absent(getattr(config, "decoder_lm_order", None), 2),
                                            lm_weight=_absent(getattr(config, "decoder_lm_weight", None), 1.0),
                                            lm_bonus=_absent(getattr(config, "decoder_lm_bonus", None), 0.0),
                                            lm_eos=_absent(getattr(config, "decoder_lm_eos", None), True))
        config.arch = config.arch.replace("deit", "vit")
        if config.arch not in vits.__dict__:
            raise NotImplementedError(f"Unknow architecture: {config.arch} (HIP kernels cover vit_tiny / vit_small / vit_base)")
        self.backbone = vits.__dict__[config.arch](patch_size=config.patch_size, drop_path_rate=config.drop_path_rate)
        config.decoder_num_classes = self.label_convertor.num_classes()
        self.decoder = CTCDecoder(in_features=self.backbone.embed_dim, num_classes=config.decoder_num_classes)
        self.loss = CTCLoss(blank=self.label_convertor.blank_idx, zero_infinity=True)

    # ------------------------------------------------------------------------------------------- arena
    def _transposed_names(self):
        names = ["backbone." + n for n in self.backbone._transposed_names()]
        if not (self.ctc or self.par):
            names += ["encoder." + n for n in self.encoder._transposed_names()]
        names += ["decoder." + n for n in self.decoder._transposed_names()]
        if self.aux_ctc_weight > 0:
            names += ["ctc_decoder." + n for n in self.ctc_decoder._transposed_names()]
        return names

    def attach_arena(self, arena, prefix):
        super().attach_arena(arena, prefix)
        self.backbone.attach_arena(arena, prefix + "backbone.")
        if not (self.ctc or self.par):
            self.encoder.attach_arena(arena, prefix + "encoder.")
        self.decoder.attach_arena(arena, prefix + "decoder.")
        if self.aux_ctc_weight > 0:
            self.ctc_decoder.attach_arena(arena, prefix + "ctc_decoder.")

    def unused_parameter_names(self):
        """cls_token and the three norm_seg LayerNorms never take part in this forward pass (their .grad stays None in
        the reference, so torch's AdamW skips them)."""
        pre = self.arena_prefix
        return [pre + "backbone.cls_token"] + [pre + f"backbone.norm_seg.{j}.{k}" for j in range(3) for k in ("weight", "bias")]

    # ------------------------------------------------------------------------------ reference surface
    def forward(self, img, text, return_loss=True, test_speed=False):
        if return_loss:
            return self.forward_train(img, text)
        if test_speed:
            return self.forward_test_speed(img)
        return self.forward_test(img)

    def extract_feat(self, img):
        """Final-norm tokens [N,256,E] (bf16, the kernels' native layout)."""
        self.ensure_arena()
        tokens, = self.backbone.tokens_and_taps(img, need_taps=False)
        return tokens

    def forward_train(self, img, img_metas):
        """img [N,3,32,128], img_metas = padded target indices int64 [N,T] -> (loss, attn [N,H,T,256])."""
        feat = self.extract_feat(img)
        targets_dict = {'padded_targets': img_metas}
        if self.ctc:                                       # (no attention maps: the second value is None)
            return self.loss(self.decoder.forward_train(feat), targets_dict), None
        if self.par:                                       # (attn [N, T, 8, 32])
            logits, attn = self.decoder.forward_train(feat)
            return self.loss(logits, targets_dict), attn
        out_enc = self.encoder(feat)
        out_dec, attn = self.decoder(feat, out_enc, targets_dict, train_mode=True)
        if not self.aux_ctc_weight > 0:
            return self.loss(out_dec, targets_dict), attn
        a = self.aux_ctc_weight                            # the hybrid objective: (1 - a) CE + a CTC over the same tokens
        tf = self.loss(out_dec, targets_dict)
        ctc = self.ctc_loss(self.ctc_decoder.forward_train(feat), {'padded_targets': self.ctc_targets(img_metas.to(feat.device))})
        self.last_losses = {"tf": tf.detach(), "ctc": ctc.detach()}
        return (1.0 - a) * tf + a * ctc, attn

    def ctc_targets(self, padded_targets):
        """The NRTR target rows int64 [N, T] = <BOS> chars <EOS> <PAD>.. -> the CTC targets int64 [N, T - 1], zero-padded: positions 1
        onward, the classes in front of the first <EOS> as class + 1 (the blank is class 0), everything else 0.  On the rows' device."""
        conv = self.label_convertor
        body = padded_targets[:, 1:].long()
        word = ((body == conv.end_idx).cumsum(dim=1) == 0) & (body != conv.padding_idx)
        return torch.where(word, body + 1, torch.zeros_like(body)).contiguous()

    def forward_ctc(self, img):
        """img [N,3,32,128] -> the auxiliary CTC head's frame probabilities fp32 [N, 32, 92] (class 0 the blank, class c + 1 the NRTR
        class c): what a CTCConvertor built beside the model decodes with any of its decoders."""
        self._par_refuses("forward_ctc")
        if not self.aux_ctc_weight > 0:
            raise ValueError("forward_ctc: the model has no auxiliary CTC head (decoder.aux_ctc_weight)")
        return self.ctc_decoder.forward_test(self.extract_feat(img))

    def forward_test(self, img):
        feat = self.extract_feat(img)
        if self.ctc or self.par:
            return self.decoder.forward_test(feat)
        return self.decoder(feat, self.encoder(feat), None, train_mode=False)

    def forward_beam(self, img, beam_width=None, joint_ctc_weight=None):
        """img [N,3,32,128] -> (paths int32 [N, W, max_seq_len] by rank, -1-padded; lengths int32 [N, W]; scores fp32 [N, W]): the W
        best words of the NRTR decoder's beam search and their log-probabilities (NRTRDecoder.forward_beam; W defaults to
        `decoder.beam_width`).  AttnConvertor.paths2nbest turns them into index lists.
        joint_ctc_weight (default: `decoder.joint_ctc_weight`) = w in [0, 1] decodes jointly with the auxiliary CTC head: the beam runs
        over S = (1 - w) log p_att + w log p_ctc, the CTC part being the prefix probability of a live hypothesis and the word's
        probability of a finished one; `scores` is S and `last_att_scores` keeps the attention parts, fp32 [N, W]."""
        self._par_refuses("forward_beam")
        if self.ctc:
            raise NotImplementedError("forward_beam is the NRTR head's; the CTC head's beam is CTCConvertor.tensor2nbest on forward_test")
        w = self.joint_ctc_weight if joint_ctc_weight is None else self._checked_joint_weight(joint_ctc_weight)
        if w is not None and not self.aux_ctc_weight > 0:
            raise ValueError("forward_beam: joint_ctc_weight needs the auxiliary CTC head (decoder.aux_ctc_weight)")
        feat = self.extract_feat(img)
        if w is None:
            return self.decoder.forward_beam(feat, self.encoder(feat), beam_width)
        with torch.no_grad():
            frames = self.ctc_decoder.forward_train(feat)      # the head's logits [N, 32, 92], rows of a 128-wide buffer
        paths, lengths, scores, self.last_att_scores = self.decoder.forward_beam(feat, self.encoder(feat), beam_width, ctc_frames=frames,
                                                                                 ctc_weight=w)
        return paths, lengths, scores

    @torch.no_grad()
    def forward_twopass(self, img, beam=None, ctc_weight=None, proposals=None):
        """Two-pass decoding ("attention rescoring"): img [N,3,32,128] -> (paths int32 [N, W, max_seq_len] by rank, -1-padded; lengths
        int32 [N, W]; scores fp32 [N, W]), the shapes of forward_beam.  The auxiliary CTC head's prefix beam of width `beam` (default:
        `decoder.twopass_beam`) proposes W words per image; the decoder scores all of them in one teacher-forced pass; S = (1 - w) log
        p(word <EOS> | image) + w log p(word | frames), both exact (forward_score's and ops.ctc_score_paths' numbers, not the
        proposer's), w = `ctc_weight` (default: `decoder.twopass_ctc_weight`, 0.5 where the model has none - untuned); ranks go by (S
        descending, proposal slot ascending).  `last_att_scores`, `last_ctc_scores` (fp32 [N, W]) and `last_sources` (int32 [N, W]: the
        proposal slot of every rank) keep the parts.  A proposal that is unused, longer than max_seq_len - 1 characters, holds a class
        the decoder cannot write, or has no finite score is dropped; a rank left over is (-1.., -1, -inf).
        proposals=(paths int32 [N, W, Tp], lengths int32 [N, W]): any decoder's hypotheses on forward_ctc(img), in CTC classes -
        ops.ctc_beam_search_lm, the paths of ops.ctc_beam_search_trie, a CTCConvertor's n-best; their own scores are not used.
        Nothing is read back."""
        self._par_refuses("forward_twopass")
        if self.ctc:
            raise NotImplementedError("forward_twopass is the NRTR head's (its decoder rescores CTC proposals); the CTC head's beam is "
                                      "CTCConvertor.tensor2nbest on forward_test")
        if not self.aux_ctc_weight > 0:
            raise ValueError("forward_twopass: the model has no auxiliary CTC head to propose words (decoder.aux_ctc_weight)")
        from .. import ops
        conv = self.label_convertor
        w = ctc_weight if ctc_weight is not None else (conv.twopass_ctc_weight if conv.twopass_ctc_weight is not None
                                                        else conv.TWOPASS_DEFAULT_WEIGHT)
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= float(w) <= 1.0:
            raise ValueError(f"forward_twopass: ctc_weight must lie in [0, 1], got {w!r}")
        if proposals is None:
            width = conv.twopass_beam if beam is None else beam
            if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= ops.NRTR_MAX_BEAM:
                raise ValueError(f"forward_twopass: beam must lie in 1..{ops.NRTR_MAX_BEAM} (decoder.twopass_beam), got {width!r}")
        elif beam is not None:
            raise ValueError("forward_twopass: beam is the width of the default proposals; proposals= bring their own")
        feat = self.extract_feat(img)
        probs = self.ctc_decoder.forward_test(feat)            # the head's frame probabilities [N, 32, 92]
        paths, lengths = ops.ctc_beam_search(probs, width, normalized=True)[:2] if proposals is None else proposals
        paths, lengths, scores, self.last_att_scores, self.last_ctc_scores, self.last_sources = self.decoder.forward_twopass(
            feat, self.encoder(feat), probs, paths, lengths, float(w), normalized=True)
        return paths, lengths, scores

    def forward_lexicon(self, img, lexicon_beam=None):
        """img [N,3,32,128] -> (word_ids int32 [N, W], log_probs fp32 [N, W], paths int32 [N, W, max_seq_len], lengths int32 [N, W]), best
        first: the W most probable words OF THE LEXICON the beam over the NRTR decoder finds along the lexicon's prefix tree
        (NRTRDecoder.forward_beam with the convertor's trie; W defaults to `decoder.lexicon_beam`).  word_ids are positions in
        label_convertor.lexicon_words, log_probs the exact log p(word <EOS> | image) - a hypothesis has one path, so the beam's
        score is the word's probability, comparable across words.  An empty slot is (-1, -inf, all -1, -1).  Device tensors, nothing
        is read back; AttnConvertor.paths2lexicon is the host-side view."""
        self._par_refuses("forward_lexicon")
        if self.ctc:
            raise NotImplementedError("forward_lexicon is the NRTR head's; the CTC head's lexicon decoding is CTCConvertor.tensor2lexicon "
                                      "on forward_test")
        conv = self.label_convertor
        if conv.lexicon_trie is None:
            raise ValueError("forward_lexicon: the convertor has no lexicon (decoder.lexicon with decoder.lexicon_beam, or "
                             "label_convertor.set_lexicon)")
        width = conv.lexicon_beam if lexicon_beam is None else conv._checked_lexicon_beam(lexicon_beam)
        feat = self.extract_feat(img)
        paths, lengths, scores, word_ids = self.decoder.forward_beam(feat, self.encoder(feat), width, trie=conv.lexicon_trie)
        return word_ids, torch.where(word_ids >= 0, scores, float("-inf")), paths, lengths

    @torch.no_grad()
    def forward_chars(self, img, words=None, nbest=1):
        """img [N,3,32,128] -> CTCConvertor.tensor2align of the CTC head's frame probabilities: the best single alignment - character
        spans, per-character log-probabilities, the alignment's score - of `words` (a list of N transcriptions) or, words=None, of the
        `nbest` word(s) the convertor's configuration decodes (greedy, beam, LM-fused beam, lexicon).  A dict of device tensors;
        CTCConvertor.tensor2chars is the host-side view."""
        self._par_refuses("forward_chars")
        if not self.ctc:
            raise NotImplementedError("forward_chars is the CTC head's: the NRTR decoder has no frame axis to align a word against "
                                      "(use decoder.type: 'CTCDecoder')")
        return self.label_convertor.tensor2align(self.forward_test(img), words=words, nbest=nbest, normalized=True)

    _SCORE_IS_NRTR = ("forward_score / forward_words are the NRTR head's (a teacher-forced decoder pass over the given words); the CTC "
                      "head scores given words with CTCConvertor.tensor2lexicon(subset=) and aligns them with forward_chars")

    def _score_rows(self, img, words):
        from ..ops import csr_rows
        self._par_refuses("forward_score / forward_words")
        if self.ctc:
            raise NotImplementedError(self._SCORE_IS_NRTR)
        if len(words) != img.shape[0]:
            raise ValueError(f"expects one word list per image, got {len(words)} lists for {img.shape[0]} images")
        seq, row_ptr, _ = self.label_convertor.words2rows(words)
        rows = csr_rows(row_ptr)
        feat = self.extract_feat(img)
        return self.decoder.forward_score(feat, self.encoder(feat), seq, rows), rows

    @torch.no_grad()
    def forward_score(self, img, words):
        """img [N,3,32,128], words: a list of N word lists (strings, or lists of class indices: AttnConvertor.words2rows) - the words
        asked of every image, R in all -> a dict of device tensors, one row per word in list order: 'score' fp32 [R] = log p(word <EOS> |
        image), exact and comparable across words - the number forward_beam / forward_lexicon return for the same word; 'length' int32
        [R]; 'char_logp' fp32 [R, max_seq_len] (entry `length`: the <EOS>); 'char_pos' fp32 [R, max_seq_len, 4] = mean_x, mean_y, std_x,
        std_y of the decoder's attention over the 8 x 32 token grid for every character; 'row_ptr' int32 [N + 1].  A word too long for the
        decoder is an infeasible row (-inf, -1, zeros).  One teacher-forced decoder pass over all R rows, the encoder memory of an
        image shared by its words (NRTRDecoder.forward_score).  AttnConvertor.scores2chars is the host-side view."""
        return self._score_rows(img, words)[0]

    @torch.no_grad()
    def forward_words(self, img, words, nbest=1):
        """The closed-vocabulary protocol with a lexicon PER IMAGE: img [N,3,32,128], words a list of N word lists -> (index int32
        [N, nbest] into every image's own list, log_probs fp32 [N, nbest]), best first; (-1, -inf) where a list holds fewer feasible
        words.  forward_score, then AttnConvertor.scores2words on the device: nothing is read back."""
        result, rows = self._score_rows(img, words)
        return self.label_convertor.scores2words(result["score"], rows, nbest)

    def forward_test_speed(self, img):
        feat = self.extract_feat(img)
        if self.ctc or self.par:                           # (one pass either way: nothing to stop early)
            return self.decoder.forward_test(feat)
        return self.decoder(feat, self.encoder(feat), None, train_mode=False, test_speed=True)
