"""tools/nmsbench.py -- times of the detection post-processing kernels, device events on one stream, medians, each
against the same step composed in this process: the IoU matrix at 1 000 x 1 000, NMS at 1 000 boxes (the configured pre_max) against
the mask kernel + the blocking copy of the mask to the host (the part of iou3d_nms.cpp's sequence that can be timed here without its
compiled scan; the scan as a Python loop is reported separately and is no baseline), the decode of a 180 x 180 x 6-task head against the
torch op sequence of center_head.py:344-421, and predict_padded end to end.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import link_amd as la  # noqa: E402
from link_amd import _lib as L  # noqa: E402
from link_amd.boxnms import nms_sorted  # noqa: E402

CFG = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 83,
                                                                                      "nms_iou_threshold": 0.2},
       "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075]}


def median_us(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return float(np.median(t))


def mask_copy(boxes, thr):
    """the device part of the reference's op sequence and its blocking copy: mask kernel, mask to the host.  The reference's compiled
    scan (tens of us at 1 000 boxes) comes on top; it is NOT timed here."""
    n = boxes.shape[0]
    nblk = (n + 63) // 64
    mask = torch.empty((n, nblk), dtype=torch.int64, device=boxes.device)
    L.check(L.lib().link_nms_mask(boxes.data_ptr(), n, None, L.NMS_ROTATE, thr, mask.data_ptr(), L.current_stream_handle()), "mask")
    return mask.cpu().numpy().view(np.uint64)


def host_scan_nms(boxes, thr):
    """mask_copy + the greedy scan as a PYTHON loop (about 1 us of interpreter time per box: an upper bound of no use as a baseline,
    kept to check the result)"""
    n = boxes.shape[0]
    nblk = (n + 63) // 64
    words = mask_copy(boxes, thr)
    remv = np.zeros(nblk, np.uint64)
    keep = []
    for i in range(n):
        nb, ib = divmod(i, 64)
        if not (int(remv[nb]) >> ib) & 1:
            keep.append(i)
            remv[nb:] |= words[i, nb:]
    return keep


def decode_torch(pd):
    pd = {k: v.permute(0, 2, 3, 1).contiguous() for k, v in pd.items()}
    hm, dim = torch.sigmoid(pd["hm"]), torch.exp(pd["dim"])
    rot = torch.atan2(pd["rot"][..., 0:1], pd["rot"][..., 1:2])
    B, H, W, K = hm.shape
    ys, xs = torch.meshgrid([torch.arange(0, H, device=hm.device), torch.arange(0, W, device=hm.device)], indexing="ij")
    xs = xs.reshape(1, -1, 1).to(hm) + pd["reg"].reshape(B, H * W, 2)[:, :, 0:1]
    ys = ys.reshape(1, -1, 1).to(hm) + pd["reg"].reshape(B, H * W, 2)[:, :, 1:2]
    xs = xs * CFG["out_size_factor"] * CFG["voxel_size"][0] + CFG["pc_range"][0]
    ys = ys * CFG["out_size_factor"] * CFG["voxel_size"][1] + CFG["pc_range"][1]
    boxes = torch.cat([xs, ys, pd["height"].reshape(B, H * W, 1), dim.reshape(B, H * W, 3), pd["vel"].reshape(B, H * W, 2),
                       rot.reshape(B, H * W, 1)], 2)
    scores, labels = hm.reshape(B, H * W, K).max(-1)
    r = torch.tensor(CFG["post_center_limit_range"], device=hm.device)
    mask = (scores > CFG["score_threshold"]) & (boxes[..., :3] >= r[:3]).all(-1) & (boxes[..., :3] <= r[3:]).all(-1)
    return boxes, labels, scores, mask


def main():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    n = 1000
    boxes = torch.zeros(n, 7)
    boxes[:, :2] = torch.rand(n, 2, generator=g) * 80 - 40
    boxes[:, 3:6] = torch.rand(n, 3, generator=g) * 4 + 0.5
    boxes[:, 6] = torch.rand(n, generator=g) * 6.28
    boxes = boxes.to(dev)
    out = {"iou_1000x1000_us": median_us(lambda: la.boxes_iou_bev(boxes, boxes)),
           "nms_1000_device_scan_us": median_us(lambda: nms_sorted(boxes, 0.2)),
           "nms_1000_mask_and_copy_to_host_us": median_us(lambda: mask_copy(boxes, 0.2)),
           "nms_1000_python_loop_scan_us": median_us(lambda: host_scan_nms(boxes, 0.2), reps=10, warm=2)}
    k, c = nms_sorted(boxes, 0.2)
    assert k[:int(c)].tolist() == host_scan_nms(boxes, 0.2)
    tasks = (1, 2, 2, 1, 2, 2)
    preds = []
    for k in tasks:
        preds.append({"hm": torch.randn(1, k, 180, 180, generator=g).to(dev) * 1.2 - 4.5, "reg": torch.rand(1, 2, 180, 180, generator=g).to(dev),
                      "height": torch.randn(1, 1, 180, 180, generator=g).to(dev), "dim": torch.randn(1, 3, 180, 180, generator=g).to(dev) * 0.4,
                      "rot": torch.randn(1, 2, 180, 180, generator=g).to(dev), "vel": torch.randn(1, 2, 180, 180, generator=g).to(dev)})
    dec = la.CenterHeadDecoder(CFG, tasks)
    out["decode_6_tasks_us"] = median_us(lambda: [dec.decode(pd) for pd in preds])
    out["decode_6_tasks_torch_us"] = median_us(lambda: [decode_torch(pd) for pd in preds])
    out["predict_padded_us"] = median_us(lambda: dec.predict_padded(preds), reps=10, warm=2)
    out["predict_us"] = median_us(lambda: dec.predict(preds), reps=10, warm=2)
    out["candidates_per_task"] = [int(dec.decode(pd)[3][0]) for pd in preds]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
