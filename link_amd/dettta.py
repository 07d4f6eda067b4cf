"""link_amd/dettta.py -- CenterHead test-time augmentation on the device (csrc/dettta.hip, section N of include/link_amd.h): what the
reference's double_flip / tt_rotation evaluation does on the host and in about forty torch ops per task.

tta_views is DoubleFlip (detection/det3d/datasets/pipelines/test_aug.py:12-32) after the rotation of preprocess.py:153-156: one
launch writes the four views of every cloud in the order the reference batches them.  CenterHeadTTADecoder is CenterHead.predict
with double_flip (models/bbox_heads/center_head.py:320-421, 461-503): the maps of the four views are read in place, flipped back,
averaged and decoded by one kernel, NMS is the existing one, and the kept boxes are rotated back by -tt_rotation on the device.
fuse_detections is the merge of the passes of several angles (detection/nms_better2.py:266-297) as one class-wise NMS.
CenterHeadDecoder (dethead.py) is not touched and keeps refusing the three flags; these names have no counterpart module in the
reference, so install_as_iou3d_nms / install_as_torchsparse register nothing for them.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from .dethead import CenterHeadDecoder, _get

_CFG_KEYS = ("nms", "circular_nms", "min_radius", "post_center_limit_range", "out_size_factor", "voxel_size", "pc_range", "score_threshold")
_offsets_cache = {}
_thr_cache = {}


def _cos_sin(angle: float):
    """cos / sin of the angle in float64, rounded to fp32: what rotation_points_single_angle's matrix holds for float32 points"""
    return float(np.float32(np.cos(np.float64(angle)))), float(np.float32(np.sin(np.float64(angle))))


class TTAViews(list):
    """The 4 B clouds as a list of [N_i, C] tensors (what Voxelizer.generate_padded takes), views of `packed` [4 N, C]; `offsets` is
    the int32 [4 B + 1] device array the kernel wrote."""
    packed: torch.Tensor
    offsets: torch.Tensor


@torch.no_grad()
def tta_views(points: Union[torch.Tensor, Sequence[torch.Tensor]], tt_rotation: float = 0.0, sizes: Sequence[int] = None) -> TTAViews:
    """B clouds -> the 4 B clouds of the double-flip evaluation, frame-major, view-minor: view 0 the cloud rotated by tt_rotation
    (x' = x c + y s, y' = -x s + y c; 0 = a copy), view 1 with y = -y, view 2 with x = -x, view 3 with both.  `points` is a list of
    [N_i, C] GPU tensors, or one packed [N, C] tensor with `sizes` = the N_i (default: one cloud)."""
    clouds = [points] if isinstance(points, torch.Tensor) else list(points)
    for c in clouds:
        if not isinstance(c, torch.Tensor) or not c.is_cuda:
            raise L.LinkAmdError("tta_views: link_amd runs on the GPU only (got a CPU tensor or an array); there is no CPU fallback")
        assert c.dim() == 2 and c.shape[1] == clouds[0].shape[1], "points are [n, ndim], the same ndim in every cloud"
    if sizes is None:
        sizes = [int(c.shape[0]) for c in clouds]
    else:
        sizes = [int(s) for s in sizes]
        assert isinstance(points, torch.Tensor) and sum(sizes) == points.shape[0], "sizes name the rows of one packed tensor"
    pts = (clouds[0] if len(clouds) == 1 else torch.cat(clouds)).contiguous().float()
    device, n, ndim, batch = pts.device, int(pts.shape[0]), int(pts.shape[1]), len(sizes)
    offs = L.point_offsets(_offsets_cache, device, sizes)
    out = torch.empty((4 * n, ndim), dtype=torch.float32, device=device)
    out_offs = torch.empty((4 * batch + 1,), dtype=torch.int32, device=device)
    cs, sn = _cos_sin(tt_rotation) if tt_rotation != 0 else (1.0, 0.0)
    with torch.cuda.device(device):
        L.check(L.lib().link_tta_views(pts.data_ptr(), offs.data_ptr(), batch, n, ndim, cs, sn, out.data_ptr(), out_offs.data_ptr(),
                                       L.current_stream_handle()), "link_tta_views")
    views = TTAViews()
    start = 0
    for nb in sizes:
        for v in range(4):
            views.append(out[4 * start + v * nb:4 * start + (v + 1) * nb])
        start += nb
    views.packed, views.offsets = out, out_offs
    return views


class CenterHeadTTADecoder(CenterHeadDecoder):
    """CenterHead.predict with test_cfg.double_flip (and tt_rotation) on maps of batch 4 B in tta_views' order.  Reads the test_cfg
    keys of CenterHeadDecoder plus double_flip (must be true) and tt_rotation (default 0).  predict / predict_padded are the base
    class's -- NMS runs in the rotated frame, where the range mask is defined -- followed by the rotation of the kept rows back."""

    def __init__(self, test_cfg, num_classes: Sequence[int]):
        if not _get(test_cfg, "double_flip", False):
            raise ValueError("CenterHeadTTADecoder: test_cfg.double_flip must be true (CenterHeadDecoder is the single-view decoder)")
        if _get(test_cfg, "per_class_nms", False):
            raise NotImplementedError("CenterHeadTTADecoder: test_cfg.per_class_nms is not built")     # center_head.py:425-426: `pass`
        super().__init__({k: _get(test_cfg, k) for k in _CFG_KEYS if _get(test_cfg, k) is not None}, num_classes)
        self.tt_rotation = float(_get(test_cfg, "tt_rotation", 0) or 0)
        rev = -self.tt_rotation                                                                         # center_head.py:492
        self._back = _cos_sin(rev) + (float(np.float32(rev)),)

    def decode(self, pd: Dict[str, torch.Tensor]):
        """One task's maps of batch 4 B -> (boxes [B, H W, 7 | 9], labels int32 [B, H W], scores [B, H W] with -inf at masked cells,
        counts int32 [B]) of the B frames, in the rotated frame"""
        hm = pd["hm"]
        if hm.shape[0] % 4 != 0:
            raise ValueError(f"CenterHeadTTADecoder: the batch holds four views per frame; {hm.shape[0]} is not a multiple of 4")
        if not hm.is_cuda:
            raise L.LinkAmdError("CenterHeadTTADecoder: link_amd runs on the GPU only; there is no CPU fallback")
        maps = {k: pd[k].contiguous().float() for k in ("hm", "reg", "height", "dim", "rot")}
        vel = pd["vel"].contiguous().float() if "vel" in pd else None
        B4, K, H, W = maps["hm"].shape
        B = B4 // 4
        boxes = torch.empty((B, H * W, 9 if vel is not None else 7), dtype=torch.float32, device=hm.device)
        labels = torch.empty((B, H * W), dtype=torch.int32, device=hm.device)
        scores = torch.empty((B, H * W), dtype=torch.float32, device=hm.device)
        counts = torch.zeros(B, dtype=torch.int32, device=hm.device)
        with torch.cuda.device(hm.device):
            L.check(L.lib().link_center_decode_flip4(maps["hm"].data_ptr(), maps["reg"].data_ptr(), maps["height"].data_ptr(),
                                                     maps["dim"].data_ptr(), maps["rot"].data_ptr(), vel.data_ptr() if vel is not None else None,
                                                     B, K, H, W, ctypes.byref(self.geom), boxes.data_ptr(), labels.data_ptr(),
                                                     scores.data_ptr(), counts.data_ptr(), L.current_stream_handle()),
                    "link_center_decode_flip4")
        return boxes, labels, scores, counts

    def rotate_back(self, boxes: torch.Tensor, idx: torch.Tensor = None) -> torch.Tensor:
        """center_head.py:489-503 on [m, 7 | 9] rows (idx int64 [m]: the rows boxes[idx], zeros where idx < 0)"""
        if self.tt_rotation == 0 and idx is None:
            return boxes
        boxes = boxes.contiguous()
        m = boxes.shape[0] if idx is None else idx.shape[0]
        out = torch.empty((m, boxes.shape[1]), dtype=torch.float32, device=boxes.device)
        cs, sn, rev = self._back
        with torch.cuda.device(boxes.device):
            L.check(L.lib().link_tta_rotate_back(boxes.data_ptr(), boxes.shape[0], boxes.shape[1], idx.data_ptr() if idx is not None else None,
                                                 m, cs, sn, rev, out.data_ptr(), L.current_stream_handle()), "link_tta_rotate_back")
        return out

    @torch.no_grad()
    def predict(self, preds: List[Dict[str, torch.Tensor]]) -> List[Dict[str, torch.Tensor]]:
        out = super().predict(preds)
        for ret in out:
            ret["box3d_lidar"] = self.rotate_back(ret["box3d_lidar"])
        return out

    @torch.no_grad()
    def predict_padded(self, preds: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
        """CenterHeadDecoder.predict_padded's keys and slots for the B = batch / 4 frames; no host round trip"""
        out = super().predict_padded(preds)
        if self.tt_rotation != 0:
            lab = out["label_preds"].reshape(-1)
            rows = torch.arange(lab.shape[0], dtype=torch.int64, device=lab.device)
            boxes = out["box3d_lidar"]
            out["box3d_lidar"] = self.rotate_back(boxes.reshape(-1, boxes.shape[-1]), torch.where(lab >= 0, rows, lab)).reshape(boxes.shape)
        return out


def _thr_table(class_thresholds, device) -> torch.Tensor:
    if isinstance(class_thresholds, torch.Tensor):
        if not class_thresholds.is_cuda:
            raise L.LinkAmdError("fuse_detections: a threshold tensor lives on the GPU (or pass a list of numbers)")
        return class_thresholds.contiguous().float()
    key = (device, tuple(float(t) for t in class_thresholds))
    t = _thr_cache.get(key)
    if t is None:
        if len(_thr_cache) >= 64:
            _thr_cache.clear()
        t = _thr_cache[key] = torch.tensor(key[1], dtype=torch.float32).to(device)
    return t


def _classwise_nms_sorted(boxes7: torch.Tensor, labels: torch.Tensor, thr: torch.Tensor, post_max: int, n_dev: torch.Tensor = None):
    """class-wise mask + greedy scan over pcdet boxes already in score order -> (keep int64 [cap], count int32 [1])"""
    cap = boxes7.shape[0]
    keep = torch.empty(cap, dtype=torch.int64, device=boxes7.device)
    count = torch.zeros(1, dtype=torch.int32, device=boxes7.device)
    if cap == 0:
        return keep, count
    lib = L.lib()
    ws = torch.empty(lib.link_nms_workspace_bytes(cap) // 8, dtype=torch.int64, device=boxes7.device)
    nd = n_dev.data_ptr() if n_dev is not None else None
    with torch.cuda.device(boxes7.device):
        stream = L.current_stream_handle()
        L.check(lib.link_nms_mask_classwise(boxes7.data_ptr(), labels.data_ptr(), cap, nd, thr.data_ptr(), thr.shape[0], ws.data_ptr(), stream),
                "link_nms_mask_classwise")
        L.check(lib.link_nms_reduce(ws.data_ptr(), cap, nd, int(post_max), keep.data_ptr(), count.data_ptr(), stream), "link_nms_reduce")
    return keep, count


def _sorted_inputs(boxes, scores, labels, what):
    for t in (boxes, scores, labels):
        if not t.is_cuda:
            raise L.LinkAmdError(f"{what}: link_amd runs on the GPU only (got a {t.device} tensor); there is no CPU fallback")
    assert boxes.dim() == 2 and boxes.shape[1] in (7, 9), f"{what}: box3d_lidar rows hold 7 or 9 columns"
    order = scores.sort(dim=0, descending=True, stable=True)[1]
    sb = boxes[order].float()
    # to_pcdet by slices (an index list would be a host-to-device copy): extents swapped, heading -> -heading - pi / 2
    nb = torch.cat([sb[:, 0:3], sb[:, 4:5], sb[:, 3:4], sb[:, 5:6], -sb[:, -1:] - math.pi / 2], 1)
    return order, sb, nb, labels[order].to(torch.int32).contiguous()


@torch.no_grad()
def fuse_detections_padded(boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, class_thresholds, max_dets: int = 500,
                           n_dev: torch.Tensor = None):
    """fuse_detections with fixed shapes and no host round trip (usable inside a captured graph): boxes [cap, 7 | 9], scores [cap],
    labels [cap] of all passes, of which the first n_dev (device int32 [1]; None: all) count -> (box3d_lidar [max_dets, C], scores
    [max_dets], label_preds int64 [max_dets] with -1 in unused slots, count int32 [1]), best first.  class_thresholds: a list (its
    device copy is kept per value) or a GPU tensor."""
    cap = boxes.shape[0]
    if n_dev is not None:
        assert n_dev.is_cuda and n_dev.dtype == torch.int32 and n_dev.numel() == 1
        scores = torch.where(torch.arange(cap, device=scores.device) < n_dev, scores, scores.new_full((), float("-inf")))
    order, sb, nb, lab = _sorted_inputs(boxes, scores, labels, "fuse_detections_padded")
    thr = _thr_table(class_thresholds, boxes.device)
    keep, count = _classwise_nms_sorted(nb, lab, thr, int(max_dets), n_dev)
    ob = torch.zeros((int(max_dets), boxes.shape[1]), dtype=torch.float32, device=boxes.device)
    os_ = torch.zeros((int(max_dets),), dtype=scores.dtype, device=boxes.device)
    ol = torch.full((int(max_dets),), -1, dtype=torch.int64, device=boxes.device)
    m = min(int(max_dets), cap)
    if m:
        k = keep[:m]
        ok = k >= 0
        kc = k.clamp(min=0)
        ob[:m] = sb[kc] * ok.unsqueeze(-1)
        os_[:m] = torch.where(ok, scores[order][kc], os_[:m])
        ol[:m] = torch.where(ok, lab[kc].long(), ol[:m])
    return ob, os_, ol, count


@torch.no_grad()
def fuse_detections(passes: Sequence[Dict[str, torch.Tensor]], class_thresholds, max_dets: int = 500):
    """The merge of one frame's detections from several test-time passes (nms_better2.py:266-297): the passes' box3d_lidar (7 or 9
    columns, det3d lidar format) / scores / label_preds are concatenated and sorted by score; rotated NMS (rotate_nms_pcdet, no
    pre-max cut) runs among the boxes of each class with class_thresholds[label]; the max_dets best survivors are returned as
    (box3d_lidar, scores, label_preds), best first.  One class-wise mask and one scan instead of a loop of NMS calls per class.

    The reference applies this after the nuScenes conversion to the global frame; BEV IoU does not depend on the frame (a rigid
    motion in the ground plane moves both footprints alike), so the lidar-frame boxes decide the same way.  The conversion itself is
    not built.  One host round trip: the number of boxes returned."""
    boxes = torch.cat([p["box3d_lidar"] for p in passes])
    scores = torch.cat([p["scores"] for p in passes])
    labels = torch.cat([p["label_preds"] for p in passes])
    order, sb, nb, lab = _sorted_inputs(boxes, scores, labels, "fuse_detections")
    if boxes.shape[0] == 0:
        return sb, scores[order], labels[order]
    keep, count = _classwise_nms_sorted(nb, lab, _thr_table(class_thresholds, boxes.device), int(max_dets))
    sel = keep[:int(count.item())]
    return sb[sel], scores[order][sel], labels[order][sel]
