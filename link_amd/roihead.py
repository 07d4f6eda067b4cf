"""link_amd/roihead.py -- the second stage of a two-stage CenterPoint on the device (csrc/roihead.hip, section O of include/link_amd.h):
what the reference's TwoStageDetector runs behind its first stage (detection/det3d/models/detectors/two_stage.py,
models/second_stage/bird_eye_view.py, models/roi_heads/roi_head.py, roi_head_template.py and target_assigner/proposal_target_layer.py).

    BEVFeatureExtractor(pc_start, voxel_size, out_stride)      bird_eye_view.py, same signature; `extract` is the padded form
    roi_box_points(boxes, num_point)                           TwoStageDetector.get_box_center for one frame
    ProposalTargetLayer(roi_sampler_cfg)                       proposal_target_layer.py on one call for the whole batch
    RoIHead(input_channels, model_cfg, ...)                    roi_head.py: same state_dict keys and initialisation
    TwoStageRefiner(extractor, roi_head, nms_post_maxsize, num_point)      two_stage.py:156-199 behind CenterHeadDecoder.predict_padded

The map is read in place (NCHW, channels_last or a slice), features are extracted only for the rows that are used, overlaps of all
frames and classes come from one launch, the sampler draws from a device array, and the loss divides on the device.  The MLP stays
nn.Conv1d / BatchNorm1d: library GEMMs.  CLS_LOSS='CrossEntropy' stays on torch.  A BEV map that requires grad (a first stage that
is not frozen) runs `_torch_extract`, the same formulas as a differentiable torch composition; both reference configs freeze it.
There is no CPU path: a CPU tensor raises LinkAmdError.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .dethead import _get

_IO = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}
# How `extract` handles a plain contiguous NCHW map: gather in place through its strides (True), or permute it once into a
# channels-last workspace and gather from that (False).  Decided by tools/roibench.py's layout figures.
NCHW_IN_PLACE = True


def _gpu(what, *tensors):
    for t in tensors:
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise L.LinkAmdError(f"{what}: link_amd runs on the GPU only (got a CPU tensor or an array); there is no CPU fallback")


def _trig(a):
    """cos / sin of a float32 tensor, correctly rounded (through float64), as the kernels form them"""
    d = a.double()
    return torch.cos(d).to(a.dtype), torch.sin(d).to(a.dtype)


# ------------------------------------------------------------------------------------------------------------------- O1: features
def roi_box_points(boxes: torch.Tensor, num_point: int, rot_col: int = -1) -> torch.Tensor:
    """TwoStageDetector.get_box_center for one frame (two_stage.py:51-78): boxes [R, L] with the heading in column rot_col (last in
    the first-stage order) -> [num_point R, 3]: the centres, then the front, back, left and right edge midpoints."""
    if num_point == 1 or boxes.shape[0] == 0:
        return boxes[:, :3]
    if num_point != 5:
        raise NotImplementedError(f"roi_box_points: num_point {num_point} (1 or 5)")
    c, s = _trig(boxes[:, rot_col])
    corners = []
    for nx, ny in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)):          # center_to_corner_box2d's order
        ux, uy = boxes[:, 3] * nx, boxes[:, 4] * ny
        corners.append(torch.stack([(ux * c + uy * s) + boxes[:, 0], (ux * -s + uy * c) + boxes[:, 1]], 1))
    height = boxes[:, 2:3]
    mids = [torch.cat([(corners[i] + corners[j]) / 2, height], 1) for i, j in ((0, 1), (2, 3), (0, 3), (1, 2))]
    return torch.cat([boxes[:, :3]] + mids, 0)


def _torch_interpolate(im: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """center_utils.py:92-121 on a [C, H, W] map read in place -> [N, C]; differentiable in the map"""
    H, W = im.shape[1:]
    x0 = torch.floor(x).long()
    y0 = torch.floor(y).long()
    x0, x1 = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
    y0, y1 = y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
    wa = (x1.type_as(x) - x) * (y1.type_as(y) - y)
    wb = (x1.type_as(x) - x) * (y - y0.type_as(y))
    wc = (x - x0.type_as(x)) * (y1.type_as(y) - y)
    wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
    return (im[:, y0, x0] * wa + im[:, y1, x0] * wb + im[:, y0, x1] * wc + im[:, y1, x1] * wd).t()


class BEVFeatureExtractor(nn.Module):
    """bird_eye_view.py: bilinear features of a BEV map at points of the proposals.  `forward` keeps the reference's signature;
    `extract` is the padded form on link_roi_bev_features and takes the NCHW map as the neck produced it."""

    def __init__(self, pc_start, voxel_size, out_stride):
        super().__init__()
        self.pc_start = [float(v) for v in pc_start][:2]
        self.voxel_size = [float(v) for v in voxel_size][:2]
        self.out_stride = float(out_stride)

    def absl_to_relative(self, absolute):
        a1 = (absolute[..., 0] - self.pc_start[0]) / self.voxel_size[0] / self.out_stride
        a2 = (absolute[..., 1] - self.pc_start[1]) / self.voxel_size[1] / self.out_stride
        return a1, a2

    def _torch_extract(self, bev, boxes, labels, sel, num_point, rot_col):
        B, R = boxes.shape[:2]
        out = []
        for b in range(B):
            src = boxes[b] if sel is None else boxes[b][sel[b].long().clamp(0, max(R - 1, 0))]
            pts = roi_box_points(src.float(), num_point, rot_col)
            xs, ys = self.absl_to_relative(pts)
            f = _torch_interpolate(bev[b].float(), xs, ys)
            n = src.shape[0]
            f = torch.cat([f[p * n:(p + 1) * n] for p in range(num_point)], 1) if num_point > 1 else f
            if labels is not None:
                lab = labels[b] if sel is None else labels[b][sel[b].long().clamp(0, max(R - 1, 0))]
                f = f * (lab != 0).unsqueeze(-1)
            out.append(f.to(bev.dtype))
        return torch.stack(out)

    def extract(self, bev: torch.Tensor, boxes: torch.Tensor, labels: Optional[torch.Tensor] = None, sel: Optional[torch.Tensor] = None,
                num_point: int = 5, rot_col: int = -1) -> torch.Tensor:
        """bev [B, C, H, W] (fp32 / fp16 / bf16; contiguous, channels_last or a slice: read in place), boxes [B, R, L >= 7] with the
        heading in column rot_col, labels int64 [B, R] (0 = an unused slot: a row of zeros), sel int32 [B, S] (rows to extract, repeats
        allowed; None: all R) -> [B, S, num_point C] in the map's dtype, the channels of point p at [p C, (p + 1) C)."""
        _gpu("BEVFeatureExtractor.extract", bev, boxes, labels, sel)
        if bev.dim() != 4 or boxes.dim() != 3 or boxes.shape[0] != bev.shape[0] or boxes.shape[2] < 7:
            raise ValueError(f"BEVFeatureExtractor.extract: bev [B, C, H, W] and boxes [B, R, >= 7] expected, got {tuple(bev.shape)} and "
                             f"{tuple(boxes.shape)}")
        if bev.dtype not in _IO:
            raise ValueError(f"BEVFeatureExtractor.extract: a float32 / float16 / bfloat16 map expected, got {bev.dtype}")
        B, C, H, W = bev.shape
        R, box_len = boxes.shape[1], boxes.shape[2]
        rot_col = rot_col % box_len
        if bev.requires_grad and torch.is_grad_enabled():
            return self._torch_extract(bev, boxes, labels, sel, num_point, rot_col)
        bev = bev.detach()
        if not NCHW_IN_PLACE and bev.is_contiguous() and C > 1 and H * W > 1:
            bev = bev.contiguous(memory_format=torch.channels_last)
        boxes = boxes.detach().float().contiguous()
        labels = None if labels is None else labels.to(torch.int64).contiguous()
        sel = None if sel is None else sel.to(torch.int32).contiguous()
        S = R if sel is None else sel.shape[1]
        out = torch.empty((B, S, num_point * C), dtype=bev.dtype, device=bev.device)
        strides = (ctypes.c_int64 * 4)(*[bev.stride(d) if bev.shape[d] > 1 else 0 for d in range(4)])
        with torch.cuda.device(bev.device):
            L.check(L.lib().link_roi_bev_features(bev.data_ptr(), _IO[bev.dtype], strides, B, C, H, W, boxes.data_ptr(), R, box_len, rot_col,
                                                  L.ptr(labels), L.ptr(sel), S, int(num_point), (ctypes.c_float * 2)(*self.pc_start),
                                                  (ctypes.c_float * 2)(*self.voxel_size), self.out_stride, out.data_ptr(),
                                                  L.current_stream_handle()), "link_roi_bev_features")
        return out

    def forward(self, example, batch_centers: Sequence[torch.Tensor], num_point: int) -> List[torch.Tensor]:
        """example['bev_feature'] = the map as the reference hands it over, [B, H, W, C]; batch_centers = per frame the
        [num_point n_b, 3] points of get_box_center -> per frame [n_b, num_point C]"""
        bev = example["bev_feature"]
        _gpu("BEVFeatureExtractor", bev, *batch_centers)
        B = len(bev)
        rows = [int(c.shape[0]) for c in batch_centers]
        cap = max(rows + [1])
        boxes = torch.zeros((B, cap, 7), dtype=torch.float32, device=bev.device)
        labels = torch.zeros((B, cap), dtype=torch.int64, device=bev.device)
        for b, c in enumerate(batch_centers):
            boxes[b, :rows[b], :2] = c[:, :2]
            labels[b, :rows[b]] = 1
        feats = self.extract(bev.permute(0, 3, 1, 2), boxes, labels, None, 1)        # a view: the channel stride is 1
        out = []
        for b in range(B):
            f = feats[b, :rows[b]]
            if num_point > 1:
                sec = rows[b] // num_point
                f = torch.cat([f[i * sec:(i + 1) * sec] for i in range(num_point)], 1)
            out.append(f)
        return out


# -------------------------------------------------------------------------------------------------------------------- O2: targets
class ProposalTargetLayer(nn.Module):
    """proposal_target_layer.py for the whole batch in two launches.  The random choices come from `noise` = torch.rand on the
    device (generator=: the torch.Generator to draw from), as section O defines: foreground without replacement by the smallest
    noise, every draw with replacement by floor(noise n).  forward(batch_dict) keeps the reference's keys ('gt_of_rois' is the
    assigned ground truth as given) and adds 'sel', 'max_overlaps', 'gt_assignment', 'gt_of_rois_canonical' and 'status' (int32
    [B]; LINK_ROI_STATUS_NO_CANDIDATE where the reference raises).  sampled_inds= replays recorded indices instead of drawing."""

    def __init__(self, roi_sampler_cfg, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        self.generator = generator
        kind = _get(roi_sampler_cfg, "CLS_SCORE_TYPE")
        if kind not in ("cls", "roi_iou"):
            raise NotImplementedError(f"ProposalTargetLayer: CLS_SCORE_TYPE {kind!r} ('cls' or 'roi_iou')")

    def forward(self, batch_dict, sampled_inds: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        cfg = self.roi_sampler_cfg
        rois, labels, scores, gt = batch_dict["rois"], batch_dict["roi_labels"], batch_dict["roi_scores"], batch_dict["gt_boxes_and_cls"]
        _gpu("ProposalTargetLayer", rois, labels, scores, gt, sampled_inds, noise)
        B, R, code = rois.shape
        M = int(_get(cfg, "ROI_PER_IMAGE"))
        if gt.dim() != 3 or gt.shape[0] != B or (gt.shape[1] > 0 and gt.shape[2] != code + 1):
            raise ValueError(f"ProposalTargetLayer: gt_boxes_and_cls [B, G, {code + 1}] expected, got {tuple(gt.shape)}")
        dev = rois.device
        rois_f, scores_f = rois.detach().float().contiguous(), scores.detach().float().contiguous()
        labels_l = labels.to(torch.int64).contiguous()
        gt_f = gt.detach().float().contiguous()
        G = gt_f.shape[1]
        if sampled_inds is not None:
            sampled_inds = sampled_inds.to(torch.int32).contiguous()
        elif noise is None:
            noise = torch.rand((B, R + M), dtype=torch.float32, device=dev, generator=self.generator)
        if noise is not None:
            noise = noise.float().contiguous()
            assert noise.shape == (B, R + M), "noise is [B, R + ROI_PER_IMAGE]"
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)                                 # noqa: E731
        out = {"max_overlaps": f32(B, R), "gt_assignment": torch.empty((B, R), dtype=torch.int32, device=dev),
               "sel": torch.empty((B, M), dtype=torch.int32, device=dev), "rois": f32(B, M, code),
               "roi_labels": torch.empty((B, M), dtype=torch.int64, device=dev), "roi_scores": f32(B, M), "gt_iou_of_rois": f32(B, M),
               "gt_of_rois": f32(B, M, code + 1), "gt_of_rois_canonical": f32(B, M, code + 1),
               "reg_valid_mask": torch.empty((B, M), dtype=torch.int64, device=dev), "rcnn_cls_labels": f32(B, M),
               "status": torch.empty(B, dtype=torch.int32, device=dev)}
        with torch.cuda.device(dev):
            L.check(L.lib().link_roi_assign(
                rois_f.data_ptr(), labels_l.data_ptr(), scores_f.data_ptr(), gt_f.data_ptr() if G else None, L.ptr(noise), L.ptr(sampled_inds),
                B, R, G, M, code, float(_get(cfg, "FG_RATIO")), int(bool(_get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False))),
                int(_get(cfg, "CLS_SCORE_TYPE") == "roi_iou"), float(_get(cfg, "CLS_FG_THRESH")), float(_get(cfg, "CLS_BG_THRESH")),
                float(_get(cfg, "CLS_BG_THRESH_LO")), float(_get(cfg, "HARD_BG_RATIO")), float(_get(cfg, "REG_FG_THRESH")),
                out["max_overlaps"].data_ptr(), out["gt_assignment"].data_ptr(), out["sel"].data_ptr(), out["rois"].data_ptr(),
                out["roi_labels"].data_ptr(), out["roi_scores"].data_ptr(), out["gt_iou_of_rois"].data_ptr(), out["gt_of_rois"].data_ptr(),
                out["gt_of_rois_canonical"].data_ptr(), out["reg_valid_mask"].data_ptr(), out["rcnn_cls_labels"].data_ptr(),
                out["status"].data_ptr(), L.current_stream_handle()), "link_roi_assign")
        feats = batch_dict.get("roi_features")
        if feats is not None:
            out["roi_features"] = torch.gather(feats, 1, out["sel"].long().unsqueeze(-1).expand(-1, -1, feats.shape[-1]))
        return out


# ----------------------------------------------------------------------------------------------------------------------- O3: loss
class _RoILossFn(torch.autograd.Function):
    """(rcnn_cls [N], rcnn_reg [N, code]) -> float32 [4] = total, cls, reg, fg_sum of section O.  Backward of out[0] alone."""

    @staticmethod
    def forward(ctx, cls, reg, labels, gt_of_rois, reg_valid, code_weights, cls_weight, reg_weight):
        cls, reg = cls.contiguous(), reg.contiguous()
        N, code = reg.shape
        dev = reg.device
        out = torch.empty(4, dtype=torch.float32, device=dev)
        unit_cls = torch.empty(N, dtype=torch.float32, device=dev)
        unit_reg = torch.empty((N, code), dtype=torch.float32, device=dev)
        cw = (ctypes.c_float * code)(*[float(v) for v in code_weights])
        with torch.cuda.device(dev):
            L.check(L.lib().link_roi_loss_forward(cls.data_ptr(), reg.data_ptr(), _IO[reg.dtype], N, code, labels.data_ptr(), gt_of_rois.data_ptr(),
                                                  reg_valid.data_ptr(), cw, float(cls_weight), float(reg_weight), out.data_ptr(),
                                                  unit_cls.data_ptr(), unit_reg.data_ptr(), L.current_stream_handle()), "link_roi_loss_forward")
        ctx.save_for_backward(unit_cls, unit_reg)
        ctx.io, ctx.cls_shape = reg.dtype, cls.shape
        total, lc, lr, fg = out[0], out[1], out[2], out[3]
        ctx.mark_non_differentiable(lc, lr, fg)
        return total, lc, lr, fg

    @staticmethod
    def backward(ctx, g_total, *_unused):
        unit_cls, unit_reg = ctx.saved_tensors
        N, code = unit_reg.shape
        dev = unit_reg.device
        up = g_total.detach().to(torch.float32).reshape(1).contiguous()
        g_cls = torch.empty(ctx.cls_shape, dtype=ctx.io, device=dev)
        g_reg = torch.empty((N, code), dtype=ctx.io, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().link_roi_loss_backward(unit_cls.data_ptr(), unit_reg.data_ptr(), up.data_ptr(), N, code, _IO[ctx.io], g_cls.data_ptr(),
                                                   g_reg.data_ptr(), L.current_stream_handle()), "link_roi_loss_backward")
        return g_cls, g_reg, None, None, None, None, None, None


def roi_loss(rcnn_cls: torch.Tensor, rcnn_reg: torch.Tensor, rcnn_cls_labels: torch.Tensor, gt_of_rois: torch.Tensor,
             reg_valid_mask: torch.Tensor, code_weights: Sequence[float], rcnn_cls_weight: float = 1.0, rcnn_reg_weight: float = 1.0):
    """RoIHeadTemplate.get_loss with BinaryCrossEntropy and L1 on link_roi_loss_forward / _backward: rcnn_cls [N] or [N, 1], rcnn_reg
    [N, code] (fp32 / fp16 / bf16), the targets of ProposalTargetLayer (any leading shape of N rows) -> (total, cls, reg, fg_sum),
    device scalars; `total` carries the gradient."""
    _gpu("roi_loss", rcnn_cls, rcnn_reg, rcnn_cls_labels, gt_of_rois, reg_valid_mask)
    N, code = rcnn_reg.shape
    if rcnn_cls.numel() != N or rcnn_cls.dtype != rcnn_reg.dtype or rcnn_reg.dtype not in _IO:
        raise ValueError(f"roi_loss: rcnn_cls [{N}] and rcnn_reg [{N}, code] of one 32- or 16-bit float type expected")
    if len(code_weights) != code:
        raise ValueError(f"roi_loss: {code} code weights expected, got {len(code_weights)}")
    return _RoILossFn.apply(rcnn_cls, rcnn_reg, rcnn_cls_labels.detach().float().reshape(-1).contiguous(),
                            gt_of_rois.detach().float().reshape(N, code + 1).contiguous(),
                            reg_valid_mask.to(torch.int64).reshape(-1).contiguous(), code_weights, rcnn_cls_weight, rcnn_reg_weight)


# --------------------------------------------------------------------------------------------------------------------- O4: refine
@torch.no_grad()
def roi_refine(rois: torch.Tensor, roi_labels: torch.Tensor, roi_scores: torch.Tensor, rcnn_cls: torch.Tensor, rcnn_reg: torch.Tensor):
    """generate_predicted_boxes + TwoStageDetector.post_process, padded and without a host read-back: rois [B, R, 7 | 9] (heading in
    column 6), roi_labels int64 [B, R] (0 = unused), roi_scores [B, R], rcnn_cls [B R] (or [B R, 1]), rcnn_reg [B R, code] ->
    {'box3d_lidar' [B, R, code] (heading last), 'scores' [B, R], 'label_preds' int64 [B, R] (-1 in unused slots), 'counts' int32 [B]},
    the slots in use packed to the front in slot order."""
    _gpu("roi_refine", rois, roi_labels, roi_scores, rcnn_cls, rcnn_reg)
    B, R, code = rois.shape
    dev = rois.device
    if rcnn_reg.dtype not in _IO or rcnn_cls.dtype != rcnn_reg.dtype or rcnn_cls.numel() != B * R or rcnn_reg.numel() != B * R * code:
        raise ValueError("roi_refine: rcnn_cls [B R] and rcnn_reg [B R, code] of one 32- or 16-bit float type expected")
    rois_f, scores_f, labels_l = rois.float().contiguous(), roi_scores.float().contiguous(), roi_labels.to(torch.int64).contiguous()
    cls, reg = rcnn_cls.contiguous(), rcnn_reg.contiguous()
    boxes = torch.empty((B, R, code), dtype=torch.float32, device=dev)
    scores = torch.empty((B, R), dtype=torch.float32, device=dev)
    labels = torch.empty((B, R), dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().link_roi_refine(rois_f.data_ptr(), labels_l.data_ptr(), scores_f.data_ptr(), cls.data_ptr(), reg.data_ptr(),
                                        _IO[reg.dtype], B, R, code, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(),
                                        L.current_stream_handle()), "link_roi_refine")
    return {"box3d_lidar": boxes, "scores": scores, "label_preds": labels, "counts": counts}


# ----------------------------------------------------------------------------------------------------------------------- the head
class RoIHead(nn.Module):
    """roi_head.py's RoIHead: the same layers under the same names (shared_fc_layer.*, cls_layers.*, reg_layers.*) with the same
    initialisation, so a reference checkpoint loads.  model_cfg holds SHARED_FC, CLS_FC, REG_FC, DP_RATIO, TARGET_CONFIG and
    LOSS_CONFIG (CLS_LOSS, REG_LOSS, LOSS_WEIGHTS: rcnn_cls_weight, rcnn_reg_weight, code_weights), as a dict or an object.

    In training `forward` assigns first; handed the map (batch_dict['bev_map'], NCHW, with `set_extractor` called) instead of
    precomputed batch_dict['roi_features'], it extracts features for the ROI_PER_IMAGE sampled rows only -- the same values the
    reference gets by extracting for every proposal and sampling afterwards."""

    def __init__(self, input_channels, model_cfg, num_class=1, code_size=7, add_box_param=False, test_cfg=None):
        super().__init__()
        self.model_cfg, self.num_class, self.test_cfg = model_cfg, num_class, test_cfg
        self.code_size, self.add_box_param = code_size, add_box_param
        self.proposal_target_layer = ProposalTargetLayer(_get(model_cfg, "TARGET_CONFIG"))
        self.forward_ret_dict = None
        self.extractor, self.num_point = None, 5
        dp = _get(model_cfg, "DP_RATIO", 0)
        shared_fc = list(_get(model_cfg, "SHARED_FC"))
        layers, pre = [], input_channels
        for k, width in enumerate(shared_fc):
            layers += [nn.Conv1d(pre, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre = width
            if k != len(shared_fc) - 1 and dp > 0:
                layers.append(nn.Dropout(dp))
        self.shared_fc_layer = nn.Sequential(*layers)
        self.cls_layers = self.make_fc_layers(pre, self.num_class, list(_get(model_cfg, "CLS_FC")))
        self.reg_layers = self.make_fc_layers(pre, code_size, list(_get(model_cfg, "REG_FC")))
        self.init_weights()

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        dp = _get(self.model_cfg, "DP_RATIO", 0)
        layers, pre = [], input_channels
        for k, width in enumerate(fc_list):
            layers += [nn.Conv1d(pre, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre = width
            if dp >= 0 and k == 0:
                layers.append(nn.Dropout(dp))
        layers.append(nn.Conv1d(pre, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    def set_extractor(self, extractor: BEVFeatureExtractor, num_point: int):
        """the extractor `forward` uses when it is handed batch_dict['bev_map'] (kept out of the state_dict: it has no parameters)"""
        object.__setattr__(self, "extractor", extractor)
        self.num_point = int(num_point)

    def assign_targets(self, batch_dict, sampled_inds=None, noise=None):
        with torch.no_grad():
            t = self.proposal_target_layer(batch_dict, sampled_inds=sampled_inds, noise=noise)
        t["gt_of_rois_src"] = t["gt_of_rois"]
        t["gt_of_rois"] = t.pop("gt_of_rois_canonical")
        return t

    def _features(self, batch_dict, rois, labels, sel):
        if self.extractor is None:
            raise ValueError("RoIHead: batch_dict has neither 'roi_features' nor an extractor for 'bev_map' (set_extractor)")
        return self.extractor.extract(batch_dict["bev_map"], rois, labels, sel, self.num_point, rot_col=6)

    def forward(self, batch_dict, training=True, sampled_inds=None, noise=None):
        batch_dict["batch_size"] = B = len(batch_dict["rois"])
        _gpu("RoIHead", batch_dict["rois"])
        if training:
            targets = self.assign_targets(batch_dict, sampled_inds, noise)
            if "roi_features" not in targets:
                targets["roi_features"] = self._features(batch_dict, batch_dict["rois"], batch_dict["roi_labels"], targets["sel"])
            for k in ("rois", "roi_labels", "roi_features", "roi_scores"):
                batch_dict[k] = targets[k]
        elif "roi_features" not in batch_dict:
            batch_dict["roi_features"] = self._features(batch_dict, batch_dict["rois"], batch_dict["roi_labels"], None)
        feats = batch_dict["roi_features"]
        if self.add_box_param:
            feats = torch.cat([feats, batch_dict["rois"].to(feats.dtype), batch_dict["roi_scores"].to(feats.dtype).unsqueeze(-1)], dim=-1)
            batch_dict["roi_features"] = feats
        pooled = feats.reshape(-1, feats.shape[-1], 1)                                     # (B N, C, 1)
        shared = self.shared_fc_layer(pooled)
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        if not training:
            batch_dict["rcnn_cls"], batch_dict["rcnn_reg"] = rcnn_cls, rcnn_reg
            cls_preds, box_preds = self.generate_predicted_boxes(B, batch_dict["rois"], rcnn_cls, rcnn_reg)
            batch_dict["batch_cls_preds"], batch_dict["batch_box_preds"] = cls_preds, box_preds
            batch_dict["cls_preds_normalized"] = False
        else:
            targets["rcnn_cls"], targets["rcnn_reg"] = rcnn_cls, rcnn_reg
            self.forward_ret_dict = targets
        return batch_dict

    def get_loss(self, tb_dict=None):
        """-> (rcnn_loss, tb_dict) with 'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss' as device scalars (no .item())"""
        tb_dict = {} if tb_dict is None else tb_dict
        ret = self.forward_ret_dict
        cfg = _get(self.model_cfg, "LOSS_CONFIG")
        w = _get(cfg, "LOSS_WEIGHTS")
        if _get(cfg, "REG_LOSS") != "L1":
            raise NotImplementedError(f"RoIHead: REG_LOSS {_get(cfg, 'REG_LOSS')!r} (the reference builds 'L1' only)")
        cw, wc, wr = list(_get(w, "code_weights")), float(_get(w, "rcnn_cls_weight")), float(_get(w, "rcnn_reg_weight"))
        kind = _get(cfg, "CLS_LOSS")
        if kind == "BinaryCrossEntropy":
            total, lc, lr, _ = roi_loss(ret["rcnn_cls"].reshape(-1), ret["rcnn_reg"], ret["rcnn_cls_labels"], ret["gt_of_rois"],
                                        ret["reg_valid_mask"], cw, wc, wr)
        elif kind == "CrossEntropy":
            # not built on the device: torch's cross entropy for the classification term, the kernels for the regression term
            labels = ret["rcnn_cls_labels"].reshape(-1).long()
            valid = (labels >= 0).float()
            ce = nn.functional.cross_entropy(ret["rcnn_cls"].float(), labels, reduction="none", ignore_index=-1)
            lc = (ce * valid).sum() / valid.sum().clamp(min=1.0) * wc
            zero = ret["rcnn_reg"].new_zeros(ret["rcnn_reg"].shape[0])
            lr = roi_loss(zero, ret["rcnn_reg"], torch.full_like(ret["rcnn_cls_labels"], -1.0), ret["gt_of_rois"], ret["reg_valid_mask"],
                          cw, 0.0, wr)[0]
            total = lc + lr
        else:
            raise NotImplementedError(f"RoIHead: CLS_LOSS {kind!r}")
        tb_dict.update({"rcnn_loss_cls": lc.detach(), "rcnn_loss_reg": lr.detach(), "rcnn_loss": total.detach()})
        return total, tb_dict

    @torch.no_grad()
    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """roi_head_template.py:153-183 -> (batch_cls_preds [B, N, num_class], batch_box_preds [B, N, code]) in slot order, the
        heading in column 6, through link_roi_refine with every slot in use"""
        B, R, code = rois.shape
        ones = torch.ones((B, R), dtype=torch.int64, device=rois.device)
        zeros = torch.zeros((B * R,), dtype=box_preds.dtype, device=rois.device)
        boxes = roi_refine(rois, ones, ones.float(), zeros, box_preds.detach())["box3d_lidar"]
        if code == 9:
            boxes = torch.cat([boxes[..., :6], boxes[..., 8:9], boxes[..., 6:8]], -1)
        return cls_preds.view(batch_size, -1, cls_preds.shape[-1]) if cls_preds.dim() > 1 else cls_preds.view(batch_size, -1, 1), boxes


class TwoStageRefiner(nn.Module):
    """The glue of two_stage.py:156-199 behind a first stage on the device.  forward takes CenterHeadDecoder.predict_padded's
    dictionary (box3d_lidar [B, R, 7 | 9] with the heading last, scores, label_preds with -1 in unused slots), the BEV map
    [B, C, H, W] as the neck produced it and, in training, gt_boxes_and_cls [B, G, 8 | 10] (the class last; for a 7-column head the
    velocity columns are dropped as two_stage.py:176-178 does).

    Training returns {'rcnn_loss', 'rcnn_loss_cls', 'rcnn_loss_reg'} (device scalars; 'rcnn_loss' carries the gradient);
    inference returns the padded predictions of roi_refine, or with per_frame=True the reference's list of dictionaries (one host
    read-back: the counts).

    One difference from the reference, a permutation of slots: reorder_first_stage_pred_and_feature packs every frame's proposals
    to the front of NMS_POST_MAXSIZE slots; with several tasks predict_padded leaves each task's proposals in its own block of
    slots, and they stay there.  Unused slots are zero rows with label 0 either way, so the same rows take part in sampling and the
    packed inference output is in slot order of that layout."""

    def __init__(self, extractor: BEVFeatureExtractor, roi_head: RoIHead, nms_post_maxsize: int, num_point: int = 5):
        super().__init__()
        self.extractor, self.roi_head = extractor, roi_head
        self.nms_post_maxsize, self.num_point = int(nms_post_maxsize), int(num_point)
        roi_head.set_extractor(extractor, num_point)

    def proposals(self, first_stage: Dict[str, torch.Tensor]):
        """-> (rois with the heading in column 6, roi_labels with 0 in unused slots, roi_scores)"""
        boxes, labels = first_stage["box3d_lidar"], first_stage["label_preds"]
        if boxes.shape[1] > self.nms_post_maxsize * max(1, first_stage["counts"].shape[1] if "counts" in first_stage and
                                                        first_stage["counts"].dim() > 1 else 1):
            raise ValueError(f"TwoStageRefiner: {boxes.shape[1]} slots per frame exceed NMS_POST_MAXSIZE = {self.nms_post_maxsize} per task")
        if boxes.shape[2] != self.roi_head.code_size:
            raise ValueError(f"TwoStageRefiner: boxes of {boxes.shape[2]} columns for a head of code size {self.roi_head.code_size}")
        if boxes.shape[2] == 9:
            boxes = torch.cat([boxes[..., :6], boxes[..., 8:9], boxes[..., 6:8]], -1)
        return boxes.contiguous(), torch.where(labels < 0, torch.zeros_like(labels), labels + 1), first_stage["scores"]

    def forward(self, first_stage: Dict[str, torch.Tensor], bev_map: torch.Tensor, gt_boxes_and_cls: Optional[torch.Tensor] = None,
                training: Optional[bool] = None, per_frame: bool = False, sampled_inds=None, noise=None):
        training = self.training if training is None else training
        _gpu("TwoStageRefiner", first_stage["box3d_lidar"], bev_map, gt_boxes_and_cls)
        rois, labels, scores = self.proposals(first_stage)
        batch_dict = {"rois": rois, "roi_labels": labels, "roi_scores": scores, "bev_map": bev_map}
        if training:
            if gt_boxes_and_cls is None:
                raise ValueError("TwoStageRefiner: training needs gt_boxes_and_cls")
            gt = gt_boxes_and_cls
            if self.roi_head.code_size == 7 and gt.shape[-1] > 8:
                gt = torch.cat([gt[..., :7], gt[..., -1:]], -1)
            batch_dict["gt_boxes_and_cls"] = gt
            self.roi_head(batch_dict, training=True, sampled_inds=sampled_inds, noise=noise)
            loss, tb = self.roi_head.get_loss()
            return {"rcnn_loss": loss, "rcnn_loss_cls": tb["rcnn_loss_cls"], "rcnn_loss_reg": tb["rcnn_loss_reg"]}
        with torch.no_grad():
            self.roi_head(batch_dict, training=False)
            out = roi_refine(rois, labels, scores, batch_dict["rcnn_cls"].reshape(-1), batch_dict["rcnn_reg"])
        if not per_frame:
            return out
        counts = out["counts"].tolist()
        return [{"box3d_lidar": out["box3d_lidar"][b, :n], "scores": out["scores"][b, :n], "label_preds": out["label_preds"][b, :n]}
                for b, n in enumerate(counts)]
