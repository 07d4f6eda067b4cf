"""link_amd/boxnms.py -- rotated BEV IoU and NMS on the device (csrc/boxnms.hip, section I of include/link_amd.h) behind the surface of
the reference's det3d.ops.iou3d_nms (iou3d_nms_utils.py) and det3d.core.bbox.box_torch_ops.rotate_nms_pcdet.

The reference's nms_gpu copies the N x N/64 mask to the host and scans it there (iou3d_nms.cpp:100-135); here the scan is a kernel, so
the only host round trip of the variable-length forms is the one `.item()` their return shape forces, and `nms_padded` has none.
"""
from __future__ import annotations

import math
import sys
import types

import torch

from . import _lib as L

_PRED = {"rotate": L.NMS_ROTATE, "normal": L.NMS_NORMAL, "circle": L.NMS_CIRCLE}


def _boxes7(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise L.LinkAmdError(f"{what}: link_amd runs on the GPU only (got a {t.device} tensor); there is no CPU fallback")
    assert t.dim() == 2 and t.shape[1] == 7, f"{what}: boxes are [n, 7] = x, y, z, dx, dy, dz, heading"
    return t.contiguous().float()


def _pairs(fn_name: str, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    a, b = _boxes7(a, fn_name), _boxes7(b, fn_name)
    if out is None:
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (a.shape[0], b.shape[0])
    with torch.cuda.device(a.device):
        L.check(getattr(L.lib(), fn_name)(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(), L.current_stream_handle()), fn_name)
    return out


def boxes_iou_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """iou3d_nms_utils.py:13-27 -> [N, M] rotated BEV IoU"""
    return _pairs("link_boxes_iou_bev", boxes_a, boxes_b)


def boxes_overlap_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """[N, M] overlap areas of the rotated footprints"""
    return _pairs("link_boxes_overlap_bev", boxes_a, boxes_b)


def to_pcdet(boxes: torch.Tensor) -> torch.Tensor:
    """iou3d_nms_utils.py:29-33: swap the two footprint extents, heading -> -heading - pi / 2 (a copy)"""
    boxes = boxes[:, [0, 1, 2, 4, 3, 5, -1]]
    boxes[:, -1] = -boxes[:, -1] - math.pi / 2
    return boxes


def boxes_iou3d_gpu(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """iou3d_nms_utils.py:35-72"""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    boxes_a, boxes_b = to_pcdet(boxes_a), to_pcdet(boxes_b)
    a_max = (boxes_a[:, 2] + boxes_a[:, 5] / 2).view(-1, 1)
    a_min = (boxes_a[:, 2] - boxes_a[:, 5] / 2).view(-1, 1)
    b_max = (boxes_b[:, 2] + boxes_b[:, 5] / 2).view(1, -1)
    b_min = (boxes_b[:, 2] - boxes_b[:, 5] / 2).view(1, -1)
    overlaps_bev = boxes_overlap_bev(boxes_a, boxes_b)
    overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
    overlaps_3d = overlaps_bev * overlaps_h
    vol_a = (boxes_a[:, 3] * boxes_a[:, 4] * boxes_a[:, 5]).view(-1, 1)
    vol_b = (boxes_b[:, 3] * boxes_b[:, 4] * boxes_b[:, 5]).view(1, -1)
    return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-6)


def nms_sorted(boxes: torch.Tensor, thresh: float, pred: str = "rotate", post_max: int = 0, n_dev: torch.Tensor = None):
    """Mask + greedy scan over boxes already in score order, on the current stream: (keep int64[cap], kept first in ascending order
    then -1; count int32[1]).  n_dev: device int32 with the number of leading boxes that count (the capacity is boxes.shape[0])."""
    boxes = _boxes7(boxes, "nms_sorted")
    cap = boxes.shape[0]
    keep = torch.empty(cap, dtype=torch.int64, device=boxes.device)
    count = torch.zeros(1, dtype=torch.int32, device=boxes.device)
    if cap == 0:
        return keep, count
    lib = L.lib()
    nbytes = lib.link_nms_workspace_bytes(cap)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=boxes.device)
    if n_dev is not None:
        assert n_dev.is_cuda and n_dev.dtype == torch.int32 and n_dev.numel() == 1
    with torch.cuda.device(boxes.device):
        L.check(lib.link_nms_bev(boxes.data_ptr(), cap, n_dev.data_ptr() if n_dev is not None else None, _PRED[pred], float(thresh),
                                 int(post_max or 0), ws.data_ptr(), nbytes, keep.data_ptr(), count.data_ptr(), L.current_stream_handle()),
                "link_nms_bev")
    return keep, count


def _order(scores: torch.Tensor, pre_maxsize) -> torch.Tensor:
    order = scores.sort(0, descending=True)[1]
    return order if pre_maxsize is None else order[:pre_maxsize]


def _select(order: torch.Tensor, keep: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    return order[keep[:int(count.item())]].contiguous()        # the one round trip: the size of what is returned


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """iou3d_nms_utils.py:75-90 -> (indices of the kept boxes, best first; None)"""
    assert boxes.shape[1] == 7
    order = _order(scores, pre_maxsize)
    keep, count = nms_sorted(boxes[order], thresh, "rotate")
    return _select(order, keep, count), None


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """iou3d_nms_utils.py:93-107 (axis-aligned footprints)"""
    assert boxes.shape[1] == 7
    order = _order(scores, None)
    keep, count = nms_sorted(boxes[order], thresh, "normal")
    return _select(order, keep, count), None


def rotate_nms_pcdet(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """box_torch_ops.py:248-277"""
    boxes = to_pcdet(boxes)
    order = _order(scores, pre_maxsize)
    boxes = boxes[order].contiguous()
    if len(boxes) == 0:
        return order[:0].contiguous()
    keep, count = nms_sorted(boxes, thresh, "rotate", post_max=post_max_size or 0)
    return _select(order, keep, count)


def _circle_boxes(xy: torch.Tensor) -> torch.Tensor:
    b = torch.zeros((xy.shape[0], 7), dtype=torch.float32, device=xy.device)
    b[:, :2] = xy
    return b


def circle_nms(boxes, min_radius, post_max_size=83):
    """center_head.py:_circle_nms over circle_nms_jit.py: boxes [n, 3] = x, y, score; a box is dropped when its centre lies within
    squared distance min_radius of a kept better one.  -> indices of the kept boxes, best first, at most post_max_size."""
    order = _order(boxes[:, 2], None)
    keep, count = nms_sorted(_circle_boxes(boxes[order, :2]), min_radius, "circle", post_max=post_max_size or 0)
    return _select(order, keep, count)


def nms_padded(boxes, scores, thresh, pre_maxsize, post_max_size, pred="rotate"):
    """NMS with fixed shapes and no host round trip (usable inside a captured graph): (idx int64[post_max_size] = indices of the kept
    boxes, best first, then -1; count int32[1]).  pred "rotate" takes [n, 7] boxes as nms_gpu does, "normal" likewise, "circle"
    takes [n, >= 2] centres with thresh = the squared radius."""
    n = boxes.shape[0]
    pre = n if pre_maxsize is None else min(int(pre_maxsize), n)
    idx = torch.full((int(post_max_size),), -1, dtype=torch.int64, device=boxes.device)
    if pre == 0:
        return idx, torch.zeros(1, dtype=torch.int32, device=boxes.device)
    order = scores.topk(pre, sorted=True)[1] if pre < n else scores.sort(0, descending=True)[1]
    sel = boxes[order]
    keep, count = nms_sorted(_circle_boxes(sel[:, :2]) if pred == "circle" else sel, thresh, pred, post_max=int(post_max_size))
    m = min(int(post_max_size), pre)
    k = keep[:m]
    idx[:m] = torch.where(k >= 0, order[k.clamp(min=0)], k)
    return idx, count


class _Iou3dNmsCuda(types.ModuleType):
    """det3d.ops.iou3d_nms.iou3d_nms_cuda in the reference's argument orders (iou3d_nms_api.cpp); `keep` is a CPU LongTensor as in the
    reference, so nms_gpu / nms_normal_gpu copy once."""

    @staticmethod
    def boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap):
        _pairs("link_boxes_overlap_bev", boxes_a, boxes_b, ans_overlap)
        return 1

    @staticmethod
    def boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou):
        _pairs("link_boxes_iou_bev", boxes_a, boxes_b, ans_iou)
        return 1

    @staticmethod
    def _nms(boxes, keep, thresh, pred):
        k, count = nms_sorted(boxes, thresh, pred)
        n = boxes.shape[0]
        both = torch.cat([k, count.long()]).cpu()
        num = int(both[n])
        keep[:num] = both[:num]
        return num

    @staticmethod
    def nms_gpu(boxes, keep, nms_overlap_thresh):
        return _Iou3dNmsCuda._nms(boxes, keep, nms_overlap_thresh, "rotate")

    @staticmethod
    def nms_normal_gpu(boxes, keep, nms_overlap_thresh):
        return _Iou3dNmsCuda._nms(boxes, keep, nms_overlap_thresh, "normal")


iou3d_nms_cuda = _Iou3dNmsCuda("det3d.ops.iou3d_nms.iou3d_nms_cuda")


def install_as_iou3d_nms() -> None:
    """Register this module's surface under the names det3d imports: `from det3d.ops.iou3d_nms import iou3d_nms_cuda` and
    `from det3d.ops.iou3d_nms import iou3d_nms_utils` resolve here.  Parent packages that are already imported (a real det3d
    checkout) are kept; missing ones are created empty."""
    utils = types.ModuleType("det3d.ops.iou3d_nms.iou3d_nms_utils")
    for name in ("boxes_iou_bev", "to_pcdet", "boxes_iou3d_gpu", "nms_gpu", "nms_normal_gpu"):
        setattr(utils, name, globals()[name])
    utils.iou3d_nms_cuda = iou3d_nms_cuda
    parent = None
    for name in ("det3d", "det3d.ops", "det3d.ops.iou3d_nms"):
        mod = sys.modules.get(name)
        if mod is None:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
        if parent is not None:
            setattr(parent, name.rsplit(".", 1)[1], mod)
        parent = mod
    parent.iou3d_nms_cuda, parent.iou3d_nms_utils = iou3d_nms_cuda, utils
    sys.modules["det3d.ops.iou3d_nms.iou3d_nms_cuda"] = iou3d_nms_cuda
    sys.modules["det3d.ops.iou3d_nms.iou3d_nms_utils"] = utils
