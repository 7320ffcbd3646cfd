"""What pins the two beam decoders to each other (kernels/beam_wave.h: the log-softmax and the selection both step kernels call), on
either backend: the CPU SIMT executor (tests/test_beam_shared_sim.py) and the MI355X (tests/test_beam_shared_gpu.py).  `device` is
where the tensors live.

By the two specifications (tests/ctc_beam_np.py, tests/nrtr_beam_np.py) a CTC prefix beam over ONE frame of logits and ONE step of the
NRTR beam with end_idx = 0 are the same computation: the empty prefix has pb = 0, so the stay candidate scores lp[0] and the extension
by class c scores lp[c], as slot 0 (score 0) gives lp[c] for every class; class 0 - the blank there, the end class here - leaves the
empty word, every other class the one-letter word; both keep the W best by (score descending, class ascending).  No gate: the results
are compared bit for bit."""
import itertools

import numpy as np
import torch

B = 5                                                            # one CTC workgroup (four waves) and a second with a single live wave
CLASSES = (2, 3, 64, 65, 128)                                    # the launcher's minimum, both sides of the 64-lane boundary, the maximum
WIDTHS = (1, 3, 16)                                              # greedy; W > C at C = 2; the maximum, with unused slots behind
LD_PAD = 5                                                       # the NRTR rows are C + 5 wide, NaN behind column C


def rows(C, seed):
    """Logits fp32 [B, C]; for C > 2 sample 1 carries a -inf logit and sample 2 two bit-identical logits in classes 0 and 1."""
    x = (np.random.default_rng(seed).normal(0.0, 2.0, (B, C))).astype(np.float32)
    if C > 2:
        x[1, C // 2] = -np.inf
        x[2, 1] = x[2, 0]
    return x


def check_one_frame_equals_one_step(device):
    from ccd_amd import ops
    for n, (C, W) in enumerate(itertools.product(CLASSES, WIDTHS)):
        x = torch.from_numpy(rows(C, 40 + n)).to(device)
        frame = ops.ctc_beam_search(x.view(B, 1, C), W, normalized=False)
        seq, score, state, parent = ops.nrtr_beam_state(B, W, 2, 0, C, device)
        buf = torch.full((B * W, C + LD_PAD), float("nan"), device=device)       # the rows of the slots that are not live stay NaN
        buf[::W, :C] = x
        step = ops.nrtr_beam_step(buf, C, 0, 0, C, seq, score, state, parent, final=True)
        for name, a, b in zip(("paths", "lengths", "hyp_scores"), frame, step):
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (C, W, name)
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (C, W, name, a, b)     # the scores as bit patterns
        lengths = frame[1].cpu().numpy()
        assert ((lengths >= 0).sum(axis=1) == np.minimum(W, np.isfinite(x.cpu().numpy()).sum(axis=1))).all(), (C, W)
