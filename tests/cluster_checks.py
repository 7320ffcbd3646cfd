"""Checks of the Dino.utils.DBSCAN clusterers through the C ABI, shared by test_cluster_sim.py (CPU SIMT executor) and
test_cluster_gpu.py (-m gpu, real MI355X)."""
import numpy as np
import torch

import cluster_np
from ccd_amd import ops
from ccd_amd.utils.DBSCAN import DBSCAN_cluster, label_cluster, region_cluster

CLASSES = {"dbscan": DBSCAN_cluster, "label": label_cluster, "region": region_cluster}


def batched_planes(dev, masks):
    """{clusterer: uint8 [B,26,32,128] numpy} of one batched call of each public class."""
    t = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32)).to(dev)
    out = {}
    for k, cls in CLASSES.items():
        p = cls()(t)
        assert p.dtype == torch.uint8 and tuple(p.shape) == (masks.shape[0], 26, 32, 128) and p.device == t.device
        out[k] = p.cpu().numpy()
    return out


def check_fixtures(dev, golden_dir):
    """Every fixture case bit-exact against the reference's recorded planes; mean-column tie cases against the restatement."""
    names, masks, want, ties = cluster_np.load_cases(golden_dir)
    got = batched_planes(dev, masks)
    for k, f in cluster_np.CLUSTERERS.items():
        for i, name in enumerate(names):
            ref = f(masks[i]) if ties[k][i] else want[k][i]
            np.testing.assert_array_equal(got[k][i], ref, err_msg=f"{k}/{name}")


def check_random(dev, masks):
    got = batched_planes(dev, masks)
    for k, f in cluster_np.CLUSTERERS.items():
        for i, m in enumerate(masks):
            np.testing.assert_array_equal(got[k][i], f(m), err_msg=f"{k}/mask {i}")


def check_ops_layers(dev, masks):
    """The op layer under the classes: id maps, boxes + count, and label_cluster == the pretraining path's planes."""
    t = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32)).to(dev)
    ids = ops.dbscan_label(t).cpu().numpy()
    boxes, count = ops.region_boxes(t)
    boxes, count = boxes.cpu().numpy(), count.cpu().numpy()
    for i, m in enumerate(masks):
        np.testing.assert_array_equal(ids[i], cluster_np.dbscan_idmap(m))
        want = cluster_np.region_boxes(m)
        assert count[i] == len(want)
        np.testing.assert_array_equal(boxes[i, :count[i]].reshape(-1, 4), np.array(want, dtype=np.int32).reshape(-1, 4))
        assert not boxes[i, count[i]:].any()
    pre = ops.idmap_to_planes(ops.ccl_label(t)).to(torch.uint8).cpu().numpy()
    np.testing.assert_array_equal(label_cluster()(t).cpu().numpy(), pre)
