"""link_amd/centerloss.py -- CenterHead training on the device (csrc/centerloss.hip, section L of include/link_amd.h): target
assignment, focal loss and L1 regression loss, forward and backward, behind

    CenterTargetAssigner(tasks, out_size_factor, voxel_size, pc_range, ...)   what AssignLabel computes per sample on the host
                                                                              (detection/det3d/datasets/pipelines/preprocess.py:283-467)
    FastFocalLoss(), RegLoss()                                                det3d/models/losses/centernet_loss.py, same signatures
    CenterHeadLoss(num_classes, weight, code_weights)                         CenterHead.loss (det3d/models/bbox_heads/center_head.py:248-293)

GPU tensors in fp32 / fp16 / bf16 inside the limits of section L run the kernels: two launches for the targets of all tasks, three
for a task's loss and two for its gradient, no host read-back, capturable in a graph.  Everything else -- CPU tensors, float64 maps,
empty batches, a RegLoss of another width than 8 or 10 -- runs `_torch_*` below: the same formulas as a torch composition (no
`.item()`, no boolean indexing), which is also what the CPU tests check.  That composition is a second implementation for the inputs
the kernels are not built for, not a stand-in for a missing library: on a GPU tensor in the built range a missing library raises.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Sequence

import torch
from torch import nn

from . import _lib as L

_IO = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}
_CLAMP_LO, _CLAMP_HI = 1e-4, 1 - 1e-4
_NOVEL_COLS = (0, 1, 2, 3, 4, 5, 8, 9)                      # target columns of a head without `vel` (center_head.py:269)
_REG_NAMES = ("reg", "height", "dim", "vel", "rot")
_REG_CH = {"reg": 2, "height": 1, "dim": 3, "vel": 2, "rot": 2}


# ------------------------------------------------------------------------------------------------------------- torch composition
def _gaussian_radius(height, width, overlap):
    """center_utils.py:17-37 on float64 tensors (the third root as the reference writes it)"""
    b1 = height + width
    c1 = width * height * (1 - overlap) / (1 + overlap)
    r1 = (b1 + torch.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - overlap) * width * height
    r2 = (b2 + torch.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * overlap
    b3 = -2 * overlap * (height + width)
    c3 = (overlap - 1) * width * height
    r3 = (b3 + torch.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return torch.minimum(r1, torch.minimum(r2, r3))


def _torch_assign(boxes: torch.Tensor, classes: torch.Tensor, tasks: Sequence[int], osf: int, vs, lo, overlap: float, max_objs: int,
                  min_radius: int, W: int, H: int) -> Dict[str, List[torch.Tensor]]:
    """the targets of section L as a torch composition: fp32 where the contract says fp32, float64 where it says float64"""
    dev = boxes.device
    B, n = classes.shape
    boxes = boxes.float()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    osf_f = f32(float(osf))
    w = boxes[..., 3] / f32(vs[0]) / osf_f
    l = boxes[..., 4] / f32(vs[1]) / osf_f
    cx = (boxes[..., 0] - f32(lo[0])) / f32(vs[0]) / osf_f
    cy = (boxes[..., 1] - f32(lo[1])) / f32(vs[1]) / osf_f
    ok = (w > 0) & (l > 0) & (cx > -1) & (cx < W) & (cy > -1) & (cy < H)
    zero = torch.zeros_like(cx)
    x = torch.where(ok, cx, zero).to(torch.int64)                       # toward zero
    y = torch.where(ok, cy, zero).to(torch.int64)
    one = torch.ones_like(w, dtype=torch.float64)
    rad = _gaussian_radius(torch.where(ok, l.double(), one), torch.where(ok, w.double(), one), float(overlap))
    rad = torch.nan_to_num(rad, nan=0.0, posinf=2147483000.0, neginf=-2147483000.0).clamp(-2147483000.0, 2147483000.0)
    rad = rad.to(torch.int64).clamp_min(int(min_radius))
    p2 = f32(2 * math.pi)
    rot = boxes[..., 8] - torch.floor(boxes[..., 8] / p2 + f32(0.5)) * p2
    d = boxes.double()
    rows = torch.stack([cx - x.float(), cy - y.float(), boxes[..., 2], torch.log(d[..., 3]).float(), torch.log(d[..., 4]).float(),
                        torch.log(d[..., 5]).float(), boxes[..., 6], boxes[..., 7], torch.sin(rot.double()).float(),
                        torch.cos(rot.double()).float()], -1)
    rows = torch.where(ok[..., None], rows, torch.zeros_like(rows))
    out = {k: [] for k in ("hm", "anno_box", "ind", "mask", "cat")}
    first = 0
    ar = torch.arange(n, device=dev)
    ys, xs = torch.arange(H, device=dev)[:, None], torch.arange(W, device=dev)[None, :]
    for K in tasks:
        c = classes.to(torch.int64) - 1 - first
        mine = (c >= 0) & (c < K)
        first += K
        # slot of every object: class-major, input order inside a class; objects of other tasks behind everything
        order = torch.argsort(torch.where(mine, c, torch.full_like(c, K)) * n + ar[None, :], dim=1)      # keys are unique
        take = min(n, max_objs)
        src = order[:, :take]                                            # object of slot k
        sel = lambda v: torch.gather(v, 1, src)
        s_mine, s_ok = sel(mine), sel(mine & ok)
        pad = max_objs - take
        padded = lambda v: torch.cat([v, v.new_zeros((B, pad) + tuple(v.shape[2:]))], 1) if pad else v
        s_rows = torch.gather(rows, 1, src[..., None].expand(-1, -1, 10))
        out["anno_box"].append(padded(torch.where(s_ok[..., None], s_rows, torch.zeros_like(s_rows))))
        out["ind"].append(padded(torch.where(s_ok, sel(y) * W + sel(x), torch.zeros_like(src))))
        out["mask"].append(padded(s_ok.to(torch.uint8)))
        out["cat"].append(padded(torch.where(s_ok, sel(c), torch.zeros_like(src))))
        hm = torch.zeros((B, K, H, W), dtype=torch.float32, device=dev)
        sx, sy, sr, sc = sel(x), sel(y), sel(rad), torch.where(s_ok, sel(c), torch.full_like(src, -1))
        del s_mine
        for k0 in range(0, take, 32):                                    # chunks of slots: [B, 32, H, W] at a time
            kx, ky, kr, kc = (v[:, k0:k0 + 32, None, None] for v in (sx, sy, sr, sc))
            dx, dy = xs[None, None] - kx, ys[None, None] - ky
            inside = (dx >= -kr) & (dx <= kr) & (dy >= -kr) & (dy <= kr)
            sigma = (2 * kr.double() + 1) / 6
            g = torch.exp(-(dx * dx + dy * dy).double() / (2 * sigma * sigma)).float()
            for cls in range(K):
                v = torch.where(inside & (kc == cls), g, torch.zeros_like(g)).amax(1)
                hm[:, cls] = torch.maximum(hm[:, cls], v)
        out["hm"].append(hm)
    return out


def _activate(x: torch.Tensor, kind: int) -> torch.Tensor:
    if kind == L.CENTER_PROBAS:
        return x
    y = torch.clamp(torch.sigmoid(x), min=_CLAMP_LO, max=_CLAMP_HI)
    return torch.where(torch.isfinite(x), y, torch.full_like(y, float("nan")))          # section L: an overflow stays visible


def _gather_cells(feat: torch.Tensor, ind: torch.Tensor) -> torch.Tensor:
    """feat [B, C, H, W], ind [B, M] (in range) -> [B, M, C], read in place"""
    b, c = feat.shape[:2]
    return torch.gather(feat.reshape(b, c, -1), 2, ind[:, None, :].expand(-1, c, -1)).transpose(1, 2)


def _torch_loss(hm, regs, kind, hm_target, anno_box, ind, mask, cat, code_weights, weight):
    """one task's loss as section L defines it; hm or regs may be None.  Returns (loss, hm_loss, loc_loss, num_pos, box_loss)."""
    ref = hm if hm is not None else regs[0]
    wide = torch.float64 if ref.dtype == torch.float64 else torch.float32
    HW = ref.shape[2] * ref.shape[3]
    valid = (mask != 0) & (ind >= 0) & (ind < HW)
    if hm is not None:
        valid = valid & (cat >= 0) & (cat < hm.shape[1])
    num_pos = (mask != 0).sum().to(wide)
    safe_ind = torch.where(valid, ind, torch.zeros_like(ind))
    zero = torch.zeros((), dtype=wide, device=ref.device)
    hm_loss, loc_loss = zero, zero
    box_loss = torch.zeros(10, dtype=wide, device=ref.device)
    if hm is not None:
        y = _activate(hm.to(wide), kind)
        neg = (torch.log1p(-y) * y * y * (1 - hm_target.to(wide)) ** 4).sum()
        safe_cat = torch.where(valid, cat, torch.zeros_like(cat))
        yp = torch.gather(_gather_cells(y, safe_ind), 2, safe_cat[..., None])[..., 0]
        yp = torch.where(valid, yp, torch.ones_like(yp))                               # a slot that does not count is not read
        pos = (torch.log(yp) * (1 - yp) ** 2).sum()
        hm_loss = torch.where(num_pos > 0, -(pos + neg) / num_pos.clamp_min(1), -neg)
    if regs is not None:
        pred = _gather_cells(torch.cat([r.to(wide) for r in regs], 1), safe_ind)
        ncol = pred.shape[2]
        target = anno_box.to(wide) if anno_box.shape[2] == ncol else anno_box.to(wide)[..., list(_NOVEL_COLS)]
        diff = torch.where(valid[..., None], pred - target, torch.zeros_like(pred))
        elem = diff.abs().sum((0, 1)) / (num_pos + 1e-4)
        box_loss = torch.cat([elem, elem.new_zeros(10 - ncol)])
        loc_loss = (elem * torch.as_tensor(code_weights[:ncol], dtype=wide, device=ref.device)).sum()
    return hm_loss + weight * loc_loss, hm_loss, loc_loss, num_pos, box_loss


# ------------------------------------------------------------------------------------------------------------------- the kernels
class _Workspace:
    """Byte buffers per device, grown on demand (one stream at a time, as the C entry asks)."""

    def __init__(self):
        self._buf = {}

    def get(self, device, shape):
        need = L.lib().link_center_loss_workspace_bytes(*shape)
        if need == 0:
            raise L.LinkAmdError(f"link_center_loss: shape {shape} outside what the kernels address")
        buf = self._buf.get(device)
        if buf is None or buf.numel() < need:
            buf = self._buf[device] = torch.empty(need, dtype=torch.uint8, device=device)
        return buf


_WS = _Workspace()


def _reg_views(regs):
    """five data pointers (vel may be missing) and their batch strides: contiguous maps, or channel slices of one tensor"""
    ptrs, strides = [], (ctypes.c_int64 * 5)()
    for i, r in enumerate(regs):
        ptrs.append(L.ptr(r))
        strides[i] = 0 if r is None else (r.stride(0) if r.shape[0] > 1 else r.shape[1] * r.shape[2] * r.shape[3])   # a size-1 dimension's stride means nothing
    return ptrs, strides


def _sliceable(r):
    """a [B, C, H, W] view whose frames are dense C * H * W blocks some stride apart"""
    B, C, H, W = r.shape
    return ((W == 1 or r.stride(3) == 1) and (H == 1 or r.stride(2) == W) and (C == 1 or r.stride(1) == H * W) and
            (B == 1 or r.stride(0) >= C * H * W))


class _CenterLossFn(torch.autograd.Function):
    """(hm or None, reg, height, dim, vel or None, rot -- or five Nones) -> float32 [16] of section L.  Backward of out[0] alone."""

    @staticmethod
    def forward(ctx, hm, reg, height, dim, vel, rot, kind, hm_target, anno_box, ind, mask, cat, code_weights, weight):
        regs = [reg, height, dim, vel, rot]
        has_reg = reg is not None
        ref = hm if hm is not None else reg
        if hm is not None:
            hm = hm.contiguous()
        regs = [None if r is None else (r if _sliceable(r) else r.contiguous()) for r in regs]
        B, K = (hm.shape[0], hm.shape[1]) if hm is not None else (ref.shape[0], 1)
        H, W = ref.shape[2], ref.shape[3]
        M = ind.shape[1]
        dev = ref.device
        buf = _WS.get(dev, (B, K, H, W, M))
        out = torch.empty(16, dtype=torch.float32, device=dev)
        unit_hm = torch.empty((B, K, H, W), dtype=torch.float32, device=dev) if hm is not None else None
        unit_box = torch.empty((B, M, 10), dtype=torch.float32, device=dev) if has_reg else None
        cw = (ctypes.c_float * 10)(*([float(v) for v in code_weights] + [0.0] * (10 - len(code_weights))))
        ptrs, strides = _reg_views(regs)
        with torch.cuda.device(dev):
            L.check(L.lib().link_center_loss_forward(L.ptr(hm), *ptrs, strides if has_reg else None, _IO[ref.dtype], kind, L.ptr(hm_target),
                                                     L.ptr(anno_box), ind.data_ptr(), mask.data_ptr(), L.ptr(cat), B, K, H, W, M, cw,
                                                     float(weight), buf.data_ptr(), buf.numel(), out.data_ptr(), L.ptr(unit_hm),
                                                     L.ptr(unit_box), L.current_stream_handle()), "link_center_loss_forward")
        ctx.save_for_backward(*[t for t in (unit_hm, unit_box, ind, mask) if t is not None])
        ctx.has = (hm is not None, has_reg, vel is not None)
        ctx.shape = (B, K, H, W, M)
        ctx.io = ref.dtype
        loss, hm_loss, loc_loss, num_pos, box = out[0], out[1], out[2], out[3], out[4:14]
        ctx.mark_non_differentiable(hm_loss, loc_loss, num_pos, box)
        return loss, hm_loss, loc_loss, num_pos, box

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        has_hm, has_reg, has_vel = ctx.has
        saved = list(ctx.saved_tensors)
        unit_hm = saved.pop(0) if has_hm else None
        unit_box = saved.pop(0) if has_reg else None
        ind, mask = saved
        B, K, H, W, M = ctx.shape
        dev = ind.device
        up = g_loss.detach().to(torch.float32).reshape(1).contiguous()
        g_hm = torch.empty((B, K, H, W), dtype=ctx.io, device=dev) if has_hm else None
        grads = [None] * 5
        if has_reg:
            grads = [torch.empty((B, _REG_CH[n], H, W), dtype=ctx.io, device=dev) if (n != "vel" or has_vel) else None for n in _REG_NAMES]
        with torch.cuda.device(dev):
            L.check(L.lib().link_center_loss_backward(L.ptr(unit_hm), L.ptr(unit_box), ind.data_ptr(), mask.data_ptr(), up.data_ptr(), B, K, H, W,
                                                      M, _IO[ctx.io], L.ptr(g_hm), *[L.ptr(g) for g in grads], None,
                                                      L.current_stream_handle()), "link_center_loss_backward")
        return (g_hm, *grads, None, None, None, None, None, None, None, None)


def _fused_ok(ref: torch.Tensor, B, K, H, W, M) -> bool:
    """what the kernels are built for; every other input takes the torch composition (module docstring)"""
    return (ref.is_cuda and ref.dtype in _IO and 1 <= B <= L.CENTER_MAX_BATCH and 1 <= K <= L.CENTER_MAX_CLASSES and H >= 1 and W >= 1
            and 1 <= M <= L.CENTER_MAX_SLOTS and B * max(K, 3) * H * W < (1 << 31) - 1024)


def _check_map(t, what, channels=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a tensor expected")
    if t.dim() != 4 or not t.is_floating_point():
        raise ValueError(f"{what}: a floating [B, C, H, W] map expected, got {t.dtype} {tuple(t.shape)}")
    if channels is not None and t.shape[1] != channels:
        raise ValueError(f"{what}: {channels} channels expected, got {t.shape[1]}")


def _check_slots(ref, ind, mask, cat, what):
    B = ref.shape[0]
    for name, t, dt in (("ind", ind, torch.int64), ("mask", mask, None), ("cat", cat, torch.int64)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != B or t.shape != ind.shape:
            raise ValueError(f"{what}: {name} [B, max_objs] expected")
        if dt is not None and t.dtype != dt:
            raise ValueError(f"{what}: {name} must be {dt}, got {t.dtype}")
        if t.device != ref.device:
            raise ValueError(f"{what}: {name} on {t.device}, the maps on {ref.device}")
    if mask.is_floating_point() or mask.dtype == torch.bool:
        raise ValueError(f"{what}: mask must be an integer tensor of 0 / 1 (uint8 as the assigner writes it), got {mask.dtype}")


def _loss(hm, regs, kind, hm_target, anno_box, ind, mask, cat, code_weights, weight, what):
    """dispatch of one task: (loss, hm_loss, loc_loss, num_pos, box_loss[10])"""
    ref = hm if hm is not None else regs[0]
    B, K = ref.shape[0], (hm.shape[1] if hm is not None else 1)
    H, W, M = ref.shape[2], ref.shape[3], ind.shape[1]
    if _fused_ok(ref, B, K, H, W, M):
        mask8 = mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)
        r5 = [None] * 5 if regs is None else list(regs)
        return _CenterLossFn.apply(hm, *r5, kind, None if hm_target is None else hm_target.float().contiguous(),
                                   None if anno_box is None else anno_box.float().contiguous(), ind.contiguous(), mask8.contiguous(),
                                   None if cat is None else cat.contiguous(), code_weights, weight)
    present = None if regs is None else [r for r in regs if r is not None]
    return _torch_loss(hm, present, kind, hm_target, anno_box, ind, mask, cat, code_weights, weight)


# ------------------------------------------------------------------------------------------------------------------ the surface
class CenterTargetAssigner:
    """AssignLabel for a collated batch on the device.  tasks: classes per task (ints), or the reference's task dicts / objects with
    `num_class`.  __call__(gt_boxes [B, N, 9] = x, y, z, w, l, h, vx, vy, rot; gt_classes int [B, N], the global 1-based class, 0 =
    empty) -> {'hm', 'anno_box', 'ind', 'mask', 'cat'}, each a list over tasks of batched tensors (the reference's collated `example`).
    The map is round((hi - lo) / voxel_size) // out_size_factor cells; pc_range holds lo x, y, (z,) hi x, y(, z)."""

    def __init__(self, tasks, out_size_factor: int, voxel_size, pc_range, gaussian_overlap: float = 0.1, max_objs: int = 500,
                 min_radius: int = 2):
        def count(t):
            if isinstance(t, int):
                return t
            if isinstance(t, dict):
                return int(t["num_class"])
            return int(getattr(t, "num_class"))
        try:
            self.tasks = tuple(count(t) for t in tasks)
        except (TypeError, KeyError, AttributeError) as e:
            raise ValueError(f"CenterTargetAssigner: tasks must name their class counts ({e})")
        pc_range, voxel_size = [float(v) for v in pc_range], [float(v) for v in voxel_size]
        if len(pc_range) not in (4, 6) or len(voxel_size) < 2:
            raise ValueError("CenterTargetAssigner: pc_range of 4 or 6 values and voxel_size of 2 or 3 expected")
        half = len(pc_range) // 2
        if not 1 <= len(self.tasks) <= L.CENTER_MAX_TASKS or any(not 1 <= k <= L.CENTER_MAX_CLASSES for k in self.tasks):
            raise ValueError(f"CenterTargetAssigner: 1..{L.CENTER_MAX_TASKS} tasks of 1..{L.CENTER_MAX_CLASSES} classes, got {self.tasks}")
        if int(out_size_factor) < 1 or int(max_objs) < 1 or int(min_radius) < 0 or not 0 < float(gaussian_overlap) < 1 or \
                min(voxel_size[:2]) <= 0:
            raise ValueError("CenterTargetAssigner: out_size_factor, max_objs >= 1, min_radius >= 0, 0 < gaussian_overlap < 1 and "
                             "positive voxel sizes expected")
        self.out_size_factor, self.max_objs, self.min_radius = int(out_size_factor), int(max_objs), int(min_radius)
        self.gaussian_overlap = float(gaussian_overlap)
        self.voxel_size, self.lo = voxel_size[:2], pc_range[:2]
        import numpy as np
        lo32, hi32, vs32 = (np.asarray(v, np.float32) for v in (pc_range[:2], pc_range[half:half + 2], voxel_size[:2]))
        grid = np.round((hi32 - lo32) / vs32).astype(np.int64)           # preprocess.py:312-315
        self.W, self.H = (int(v) for v in grid // self.out_size_factor)
        if self.W < 1 or self.H < 1 or self.W > 32767 or self.H > 32767:
            raise ValueError(f"CenterTargetAssigner: a map of {self.W} x {self.H} cells")

    def _geom(self):
        g = L.LinkCenterAssignGeom()
        g.pc_range[0], g.pc_range[1] = self.lo
        g.voxel_size[0], g.voxel_size[1] = self.voxel_size
        g.gaussian_overlap, g.out_size_factor, g.w, g.h = self.gaussian_overlap, self.out_size_factor, self.W, self.H
        g.max_objs, g.min_radius, g.num_tasks = self.max_objs, self.min_radius, len(self.tasks)
        for i, k in enumerate(self.tasks):
            g.num_classes[i] = k
        return g

    def __call__(self, gt_boxes: torch.Tensor, gt_classes: torch.Tensor) -> Dict[str, List[torch.Tensor]]:
        if not isinstance(gt_boxes, torch.Tensor) or not isinstance(gt_classes, torch.Tensor):
            raise ValueError("CenterTargetAssigner: tensors expected")
        if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 9 or gt_classes.shape != gt_boxes.shape[:2]:
            raise ValueError(f"CenterTargetAssigner: gt_boxes [B, N, 9] and gt_classes [B, N] expected, got {tuple(gt_boxes.shape)} and "
                             f"{tuple(gt_classes.shape)}")
        if not gt_boxes.is_floating_point() or gt_classes.is_floating_point() or gt_classes.dtype == torch.bool:
            raise ValueError(f"CenterTargetAssigner: floating boxes and integer classes expected, got {gt_boxes.dtype} and {gt_classes.dtype}")
        if gt_boxes.device != gt_classes.device:
            raise ValueError(f"CenterTargetAssigner: gt_boxes on {gt_boxes.device}, gt_classes on {gt_classes.device}")
        B, n = gt_classes.shape
        M, W, H = self.max_objs, self.W, self.H
        fused = (gt_boxes.is_cuda and B >= 1 and n <= L.CENTER_MAX_OBJECTS and B * M * 10 < (1 << 31) and
                 all(B * k * H * W < (1 << 31) for k in self.tasks))
        if not fused:
            if B == 0 or n == 0:
                dev = gt_boxes.device
                return {"hm": [torch.zeros((B, k, H, W), device=dev) for k in self.tasks],
                        "anno_box": [torch.zeros((B, M, 10), device=dev) for _ in self.tasks],
                        "ind": [torch.zeros((B, M), dtype=torch.int64, device=dev) for _ in self.tasks],
                        "mask": [torch.zeros((B, M), dtype=torch.uint8, device=dev) for _ in self.tasks],
                        "cat": [torch.zeros((B, M), dtype=torch.int64, device=dev) for _ in self.tasks]}
            return _torch_assign(gt_boxes, gt_classes, self.tasks, self.out_size_factor, self.voxel_size, self.lo, self.gaussian_overlap,
                                 M, self.min_radius, W, H)
        dev = gt_boxes.device
        boxes = gt_boxes.detach().to(torch.float32).contiguous()
        classes = gt_classes.detach().to(torch.int32).contiguous()
        out = {"hm": [torch.empty((B, k, H, W), dtype=torch.float32, device=dev) for k in self.tasks],
               "anno_box": [torch.empty((B, M, 10), dtype=torch.float32, device=dev) for _ in self.tasks],
               "ind": [torch.empty((B, M), dtype=torch.int64, device=dev) for _ in self.tasks],
               "mask": [torch.empty((B, M), dtype=torch.uint8, device=dev) for _ in self.tasks],
               "cat": [torch.empty((B, M), dtype=torch.int64, device=dev) for _ in self.tasks]}
        tables = [(ctypes.c_void_p * L.CENTER_MAX_TASKS)(*[t.data_ptr() for t in out[k]]) for k in ("hm", "anno_box", "ind", "mask", "cat")]
        g = self._geom()
        with torch.cuda.device(dev):
            L.check(L.lib().link_center_assign(ctypes.byref(g), boxes.data_ptr(), classes.data_ptr(), B, n, *tables,
                                               L.current_stream_handle()), "link_center_assign")
        return out


class FastFocalLoss(nn.Module):
    """centernet_loss.py:26-54: forward(out [B, C, H, W] probabilities, target [B, C, H, W], ind, mask, cat [B, M]) -> the scalar loss"""

    def forward(self, out, target, ind, mask, cat):
        _check_map(out, "FastFocalLoss: out")
        _check_map(target, "FastFocalLoss: target")
        if target.shape != out.shape or target.device != out.device:
            raise ValueError(f"FastFocalLoss: out {tuple(out.shape)} on {out.device}, target {tuple(target.shape)} on {target.device}")
        _check_slots(out, ind, mask, cat, "FastFocalLoss")
        return _loss(out, None, L.CENTER_PROBAS, target, None, ind, mask, cat, (), 0.0, "FastFocalLoss")[0]


class RegLoss(nn.Module):
    """centernet_loss.py:6-24: forward(output [B, D, H, W], mask, ind [B, M], target [B, M, D]) -> the loss per column [D].  Widths 8
    and 10 (a CenterHead's box code without and with `vel`) read `output` in place through the kernels; other widths run the torch
    composition."""

    def forward(self, output, mask, ind, target):
        _check_map(output, "RegLoss: output")
        _check_slots(output, ind, mask, None, "RegLoss")
        D = output.shape[1]
        if not isinstance(target, torch.Tensor) or target.dim() != 3 or target.shape != (ind.shape[0], ind.shape[1], D) or \
                target.device != output.device:
            raise ValueError(f"RegLoss: target [B, max_objs, {D}] on {output.device} expected")
        if D in (8, 10) and _fused_ok(output, output.shape[0], 1, output.shape[2], output.shape[3], ind.shape[1]):
            # every column its own unit weight: D losses with D gradients in one call (the loss differentiated is their weighted sum)
            return _RegLossColumns.apply(output, mask, ind, target)
        m = (mask != 0) & (ind >= 0) & (ind < output.shape[2] * output.shape[3])
        wide = torch.float64 if output.dtype == torch.float64 else torch.float32
        pred = _gather_cells(output.to(wide), torch.where(m, ind, torch.zeros_like(ind)))
        diff = torch.where(m[..., None], pred - target.to(wide), torch.zeros_like(pred))
        return diff.abs().sum((0, 1)) / ((mask != 0).sum().to(wide) + 1e-4)


class _RegLossColumns(torch.autograd.Function):
    """RegLoss on the kernels: box_loss[0..D) of a forward with unit code weights; the gradient of column c is unit_box[..., c] times
    the upstream of that column, scattered by the backward entry after the columns are weighted."""

    @staticmethod
    def forward(ctx, output, mask, ind, target):
        output = output.contiguous()
        B, D, H, W = output.shape
        M = ind.shape[1]
        dev = output.device
        if D == 10:
            chans, anno = (0, 2, 3, 6, 8), target.float().contiguous()
        else:
            chans = (0, 2, 3, None, 6)
            anno = torch.zeros((B, M, 10), dtype=torch.float32, device=dev)
            anno[..., list(_NOVEL_COLS)] = target.float()
        regs = [None if c is None else output[:, c:c + _REG_CH[n]] for c, n in zip(chans, _REG_NAMES)]
        ptrs, strides = _reg_views(regs)
        mask8 = mask.to(torch.uint8).contiguous()
        ind = ind.contiguous()
        buf = _WS.get(dev, (B, 1, H, W, M))
        out = torch.empty(16, dtype=torch.float32, device=dev)
        unit_box = torch.empty((B, M, 10), dtype=torch.float32, device=dev)
        cw = (ctypes.c_float * 10)(*([1.0] * 10))
        with torch.cuda.device(dev):
            L.check(L.lib().link_center_loss_forward(None, *ptrs, strides, _IO[output.dtype], L.CENTER_PROBAS, None, anno.data_ptr(),
                                                     ind.data_ptr(), mask8.data_ptr(), None, B, 1, H, W, M, cw, 1.0, buf.data_ptr(),
                                                     buf.numel(), out.data_ptr(), None, unit_box.data_ptr(), L.current_stream_handle()),
                    "link_center_loss_forward")
        ctx.save_for_backward(unit_box, ind, mask8)
        ctx.shape, ctx.io = (B, D, H, W, M), output.dtype
        return out[4:4 + D].clone()

    @staticmethod
    def backward(ctx, g):
        unit_box, ind, mask8 = ctx.saved_tensors
        B, D, H, W, M = ctx.shape
        dev = ind.device
        weighted = unit_box.clone()
        weighted[..., :D] *= g.detach().float()
        one = torch.ones(1, dtype=torch.float32, device=dev)
        grad = torch.empty((B, D, H, W), dtype=ctx.io, device=dev)
        chans = (0, 2, 3, 6, 8) if D == 10 else (0, 2, 3, None, 6)
        regs = [None if c is None else grad[:, c:c + _REG_CH[n]] for c, n in zip(chans, _REG_NAMES)]
        ptrs, strides = _reg_views(regs)
        with torch.cuda.device(dev):
            L.check(L.lib().link_center_loss_backward(None, weighted.data_ptr(), ind.data_ptr(), mask8.data_ptr(), one.data_ptr(), B, 1, H, W, M,
                                                      _IO[ctx.io], None, *ptrs, strides, L.current_stream_handle()),
                    "link_center_loss_backward")
        return grad, None, None, None


class CenterHeadLoss(nn.Module):
    """CenterHead.loss (center_head.py:248-293) for a head's raw maps.  forward(example, preds_dicts): example = the assigner's
    dictionary, preds_dicts = per task {'hm', 'reg', 'height', 'dim', 'rot'[, 'vel']} (logits; left untouched -- the reference
    overwrites 'hm' with its sigmoid).  Returns the reference's rets_merged: {'loss', 'hm_loss', 'loc_loss', 'loc_loss_elem',
    'num_positive'}, lists over tasks of device tensors (no .cpu()); 'loss' carries the gradient, one autograd.Function per task."""

    def __init__(self, num_classes: Sequence[int], weight: float = 0.25, code_weights: Sequence[float] = (1.0,) * 10):
        super().__init__()
        self.num_classes = tuple(int(k) for k in num_classes)
        self.weight = float(weight)
        self.code_weights = tuple(float(v) for v in code_weights)
        if len(self.code_weights) not in (8, 10):
            raise ValueError(f"CenterHeadLoss: 8 or 10 code weights expected, got {len(self.code_weights)}")
        if not self.num_classes or any(k < 1 for k in self.num_classes):
            raise ValueError(f"CenterHeadLoss: class counts {self.num_classes}")

    def forward(self, example: Dict[str, List[torch.Tensor]], preds_dicts: List[Dict[str, torch.Tensor]]) -> Dict[str, List[torch.Tensor]]:
        if len(preds_dicts) != len(self.num_classes):
            raise ValueError(f"CenterHeadLoss: {len(self.num_classes)} tasks, {len(preds_dicts)} prediction dictionaries")
        for key in ("hm", "anno_box", "ind", "mask", "cat"):
            if key not in example or len(example[key]) != len(self.num_classes):
                raise ValueError(f"CenterHeadLoss: example[{key!r}] must list {len(self.num_classes)} tasks")
        rets = {k: [] for k in ("loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive")}
        for t, (K, preds) in enumerate(zip(self.num_classes, preds_dicts)):
            what = f"CenterHeadLoss task {t}"
            hm = preds["hm"]
            _check_map(hm, what + ": hm", K)
            has_vel = "vel" in preds
            ncol = 10 if has_vel else 8
            if len(self.code_weights) != ncol:
                raise ValueError(f"{what}: {ncol} columns{' (vel)' if has_vel else ''} but {len(self.code_weights)} code weights")
            regs = []
            for name in _REG_NAMES:
                r = preds.get(name)
                if r is None and name == "vel":
                    regs.append(None)
                    continue
                _check_map(r, f"{what}: {name}", _REG_CH[name])
                if r.shape[0] != hm.shape[0] or r.shape[2:] != hm.shape[2:] or r.dtype != hm.dtype or r.device != hm.device:
                    raise ValueError(f"{what}: {name} {r.dtype} {tuple(r.shape)} on {r.device} against hm {hm.dtype} {tuple(hm.shape)} on {hm.device}")
                regs.append(r)
            target, anno = example["hm"][t], example["anno_box"][t]
            ind, mask, cat = example["ind"][t], example["mask"][t], example["cat"][t]
            if not isinstance(target, torch.Tensor) or target.shape != hm.shape or target.device != hm.device:
                raise ValueError(f"{what}: example['hm'] must be {tuple(hm.shape)} on {hm.device}")
            _check_slots(hm, ind, mask, cat, what)
            if not isinstance(anno, torch.Tensor) or anno.shape != (ind.shape[0], ind.shape[1], 10) or anno.device != hm.device:
                raise ValueError(f"{what}: example['anno_box'] [B, max_objs, 10] on {hm.device} expected")
            loss, hm_loss, loc_loss, num_pos, box = _loss(hm, regs, L.CENTER_LOGITS, target, anno, ind, mask, cat, self.code_weights,
                                                          self.weight, what)
            rets["loss"].append(loss)
            rets["hm_loss"].append(hm_loss.detach())
            rets["loc_loss"].append(loc_loss)
            rets["loc_loss_elem"].append(box[:ncol].detach())
            rets["num_positive"].append(num_pos.detach())
        return rets
