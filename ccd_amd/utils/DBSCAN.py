"""The reference's character clusterers (Dino/utils/DBSCAN.py), on the GPU: `DBSCAN_cluster`, `label_cluster`, `region_cluster`.

Each one is a batched HIP kernel (one workgroup per 32x128 mask, the mask held in LDS) followed by one expansion into the
reference's uint8 planes; nothing runs per image on the host.

    forward(mask)   numpy [32, 128]                      -> numpy uint8 [26, 32, 128]   (the reference contract; current GPU)
                    torch [32, 128] or [B, 32, 128]      -> torch uint8 [26, 32, 128] / [B, 26, 32, 128] on the mask's device

Input types: integer, bool, float32 and float64 masks are accepted.
  * DBSCAN_cluster takes the pixels with mask > 0.1 as its points.  The compare is made in fp32 (a float64 mask is rounded to
    fp32 first), so a pixel equal to float32(0.1) is background - as in the reference for a float32 mask.
  * label_cluster and region_cluster treat every nonzero pixel as foreground.  For the binary masks the pipeline produces that
    is what skimage's measure.label does; on a multi-valued mask skimage would also split touching pixels of different values
    into different components, which these clusterers do not.
Only 32x128 masks are supported (ValueError otherwise).  There is no host fallback: without a GPU the call raises RuntimeError.
The reference catches every exception and returns zero planes after printing 'real error'; the inputs that take that path
(a nonzero mask with no pixel > 0.1 in DBSCAN_cluster) give zero planes here too, silently.
All three reference classes also return zero planes whenever mask.sum() == 0.  For the non-negative masks of the pipeline that
means an empty mask, and the result is the same here.  A signed mask whose values cancel to a zero sum is clustered here like any
other mask; the reference would return zero planes for it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops

H, W, PLANES = 32, 128, 26


def _device_for_numpy():
    if _lib._stream_override is not None:           # the C ABI is bound to a host executor (kernel tests)
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise RuntimeError("ccd_amd.utils.DBSCAN runs on an AMD GPU only; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _prepare(mask, nonzero):
    """-> (fp32 [B,32,128] contiguous device tensor, was_numpy, was_2d).  `nonzero`: the clusterer only asks mask != 0, so
    the test is made in the mask's own dtype (a tiny float64 value stays foreground)."""
    was_numpy = not isinstance(mask, torch.Tensor)
    if was_numpy:
        arr = np.asarray(mask)
        if arr.ndim != 2 or arr.shape != (H, W):
            raise ValueError(f"ccd_amd.utils.DBSCAN supports [{H}, {W}] masks only, got {list(arr.shape)}")
        if nonzero and arr.dtype != np.float32:
            arr = arr != 0
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(_device_for_numpy())
    else:
        if mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != (H, W):
            raise ValueError(f"ccd_amd.utils.DBSCAN supports [{H}, {W}] or [B, {H}, {W}] masks only, got {list(mask.shape)}")
        if mask.device.type != "cuda" and _lib._stream_override is None:
            raise RuntimeError("ccd_amd.utils.DBSCAN runs on an AMD GPU only (move the mask with .cuda() first); "
                               "there is no CPU path")
        t = mask
        if nonzero and t.dtype != torch.float32:
            t = t != 0
        t = t.to(torch.float32).contiguous()
    was_2d = t.dim() == 2
    if was_2d:
        t = t.unsqueeze(0)
    return t, was_numpy, was_2d


def _planes(t, run):
    """run(t) on a non-empty batch; an empty batch gets its empty result without a launch."""
    return run(t) if t.shape[0] else torch.zeros((0, PLANES, H, W), dtype=torch.uint8, device=t.device)


def _finish(planes, was_numpy, was_2d):
    if was_2d:
        planes = planes[0]
    return planes.cpu().numpy() if was_numpy else planes


class DBSCAN_cluster(nn.Module):
    """sklearn DBSCAN(eps=1.5, min_samples=4) on the pixels with mask > 0.1; clusters of >= 30 pixels, the 26 with the smallest
    mean column, left to right (DBSCAN.py:10-59).  `eps` / `min_samples` are accepted and ignored, as in the reference.  Mean
    column ties go to the cluster found first (the reference's np.argsort leaves them unspecified)."""

    def __init__(self, eps=1.5, min_samples=4):
        super().__init__()

    def forward(self, mask):
        t, was_numpy, was_2d = _prepare(mask, nonzero=False)
        return _finish(_planes(t, lambda t: ops.idmap_to_planes_u8(ops.dbscan_label(t))), was_numpy, was_2d)


class label_cluster(nn.Module):
    """8-connected components of mask != 0 with >= 30 pixels, the first 26 in label order, sorted by mean column
    (DBSCAN.py:61-103).  The same kernel as ABIDINOModel's character regions; mean column ties go to the lower label."""

    def __init__(self):
        super().__init__()

    def forward(self, mask):
        t, was_numpy, was_2d = _prepare(mask, nonzero=True)
        return _finish(_planes(t, lambda t: ops.idmap_to_planes_u8(ops.ccl_label(t))), was_numpy, was_2d)


class region_cluster(nn.Module):
    """Bounding boxes of the 8-connected components of mask != 0, stably sorted by xmin + xmax, the first 26, each box of area
    >= 100 filled into the next plane (DBSCAN.py:106-141).  Planes may overlap."""

    def __init__(self):
        super().__init__()

    def forward(self, mask):
        t, was_numpy, was_2d = _prepare(mask, nonzero=True)
        return _finish(_planes(t, lambda t: ops.boxes_to_planes_u8(*ops.region_boxes(t))), was_numpy, was_2d)
