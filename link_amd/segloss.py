"""link_amd/segloss.py -- the segmentation criterion of the reference's trainer on the device (csrc/segloss.hip, section K of
include/link_amd.h): cross-entropy + Lovasz-softmax, forward and backward, behind

    SegCriterion(ce_ignore=255, lovasz_ignore=0, classes='present')      what segmentation/core/trainers.py:64-73 computes with the
                                                                         pair core/builder.py:61-72 builds
    lovasz_softmax(probas, labels, classes, per_image, ignore)           core/lovasz_losses.py:156-171
    lovasz_softmax_flat(probas, labels, classes)                         core/lovasz_losses.py:174-202

GPU tensors with 2..32 classes in fp32 / fp16 / bf16 and at least one row run the kernels: 20 launches, no host read-back, capturable
in a graph.  Everything else -- CPU tensors, other class counts, GPU rows of another floating type (float64), an empty [0, C]
input -- runs `_torch_*` below: the same formula as a torch composition (one stable sort over all classes at
once, lovasz_grad in closed form, no `.item()` and no `nonzero()`), which is also what the CPU tests check.  That composition is a
second implementation of the formula for the inputs the kernels are not built for, not a stand-in for a missing library: on a GPU
tensor in the built range a missing library raises.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L

_IO = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}
_CLASSES = {"present": L.SEGLOSS_PRESENT, "all": L.SEGLOSS_ALL}


# ------------------------------------------------------------------------------------------------------------- torch composition
def _torch_lovasz_flat(probas: torch.Tensor, labels: torch.Tensor, classes: str = "present", ignore=None) -> torch.Tensor:
    """lovasz_softmax_flat over the rows with label != ignore, all classes at once.  Ignored rows stay in the table with an error
    of -1 (they sort behind every valid row and count for nothing), so no shape depends on the data."""
    p = probas.float() if probas.dtype in (torch.float16, torch.bfloat16) else probas
    n, c = p.shape
    if n == 0:
        return p.sum() * 0.0
    valid = torch.ones_like(labels, dtype=torch.bool) if ignore is None else labels != ignore
    fg = (labels[:, None] == torch.arange(c, device=p.device)[None, :]) & valid[:, None]
    err = torch.where(valid[:, None], (fg.to(p.dtype) - p).abs(), p.new_full((), -1.0))
    err_sorted, perm = torch.sort(err, dim=0, descending=True, stable=True)
    fg_s = torch.gather(fg, 0, perm).to(p.dtype)
    valid_s = valid[perm].to(p.dtype)
    n_c = fg_s.sum(0, keepdim=True)
    f_k = fg_s.cumsum(0)
    u_k = n_c + (valid_s * (1 - fg_s)).cumsum(0)
    u_prev = u_k - 1
    g_bg = torch.where(u_prev > 0, (n_c - f_k) / (u_prev * u_k).clamp_min(1), torch.ones_like(u_k))
    g = torch.where(fg_s > 0, 1 / u_k.clamp_min(1), g_bg) * valid_s
    loss_c = (err_sorted * g.detach()).sum(0)
    n_valid = valid.sum()
    taken = ((n_c[0] > 0) if classes == "present" else torch.ones_like(n_c[0], dtype=torch.bool)) & (n_valid > 0)
    return (loss_c * taken.to(p.dtype)).sum() / taken.sum().clamp_min(1).to(p.dtype)


def _torch_criterion(rows, labels, ce_ignore, lov_ignore, classes):
    x = rows.float()
    ce = F.cross_entropy(x, labels, ignore_index=ce_ignore)
    lov = _torch_lovasz_flat(F.softmax(x, dim=1), labels, classes, lov_ignore)
    return ce + lov, ce, lov


# ------------------------------------------------------------------------------------------------------------------- the kernels
class _Workspace:
    """Byte buffers per device, grown on demand (one stream at a time, as the C entry asks)."""

    def __init__(self):
        self._buf = {}

    def get(self, device, n: int, c: int):
        need = L.lib().link_segloss_workspace_bytes(n, c)
        if need == 0:
            raise L.LinkAmdError(f"link_segloss: shape [{n}, {c}] outside what the kernels address")
        buf = self._buf.get(device)
        if buf is None or buf.numel() < need:
            buf = self._buf[device] = torch.empty(need, dtype=torch.uint8, device=device)
        return buf


def _fused_ok(rows: torch.Tensor) -> bool:
    """what the kernels are built for; every other input takes the torch composition (module docstring)"""
    return rows.is_cuda and rows.dtype in _IO and L.SEGLOSS_MIN_CLASSES <= rows.shape[1] <= L.SEGLOSS_MAX_CLASSES and rows.shape[0] > 0


class _SegLossFn(torch.autograd.Function):
    """(rows [n, c], labels) -> float32 [3] = total, CE, Lovasz.  Backward of the total alone (kernel 4); CE and Lovasz are
    reported, not differentiated."""

    @staticmethod
    def forward(ctx, rows, labels, ws, kind, ce_ignore, lov_ignore, classes):
        rows = rows.contiguous()
        labels = labels.contiguous()
        n, c = rows.shape
        buf = ws.get(rows.device, n, c)
        out = torch.empty(3, dtype=torch.float32, device=rows.device)
        unit = torch.empty((c, n), dtype=torch.float32, device=rows.device)
        with torch.cuda.device(rows.device):
            L.check(L.lib().link_segloss_forward(rows.data_ptr(), _IO[rows.dtype], kind, labels.data_ptr(), n, c, int(ce_ignore),
                                                 0 if lov_ignore is None else int(lov_ignore), 0 if lov_ignore is None else 1,
                                                 _CLASSES[classes], buf.data_ptr(), buf.numel(), out.data_ptr(), unit.data_ptr(),
                                                 L.current_stream_handle()), "link_segloss_forward")
        ctx.save_for_backward(unit)
        ctx.io = rows.dtype
        total, ce, lov = out[0], out[1], out[2]
        ctx.mark_non_differentiable(ce, lov)
        return total, ce, lov

    @staticmethod
    def backward(ctx, g_total, _g_ce, _g_lov):
        (unit,) = ctx.saved_tensors
        c, n = unit.shape
        up = g_total.detach().to(torch.float32).reshape(1).contiguous()
        grad = torch.empty((n, c), dtype=ctx.io, device=unit.device)
        with torch.cuda.device(unit.device):
            L.check(L.lib().link_segloss_backward(unit.data_ptr(), up.data_ptr(), n, c, _IO[ctx.io], grad.data_ptr(),
                                                  L.current_stream_handle()), "link_segloss_backward")
        return grad, None, None, None, None, None, None


def _check_flat(rows, labels, what):
    if not isinstance(rows, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise ValueError(f"{what}: tensors expected")
    if rows.dim() != 2 or labels.dim() != 1 or labels.shape[0] != rows.shape[0]:
        raise ValueError(f"{what}: rows [N, C] and labels [N] expected, got {tuple(rows.shape)} and {tuple(labels.shape)}")
    if labels.dtype != torch.int64:
        raise ValueError(f"{what}: labels must be int64, got {labels.dtype}")
    if not rows.is_floating_point():
        raise ValueError(f"{what}: rows must be floating point, got {rows.dtype}")
    if labels.device != rows.device:
        raise ValueError(f"{what}: rows on {rows.device}, labels on {labels.device}")


def _check_classes(classes, c):
    if not isinstance(classes, str):
        raise NotImplementedError("classes given as a list is not built: 'present' or 'all'")
    if classes not in _CLASSES:
        raise ValueError(f"classes must be 'present' or 'all', got {classes!r}")
    if c == 1:
        raise NotImplementedError("C = 1 (the sigmoid form of lovasz_softmax) is not built")


class SegCriterion(nn.Module):
    """CrossEntropyLoss(ignore_index=ce_ignore)(logits, targets) + lovasz_softmax(softmax(logits), targets, ignore=lovasz_ignore),
    the softmax taken in fp32 (what autocast does to it in the reference).  forward(logits [N, C], targets int64 [N]) -> the scalar
    loss (fp32); .last_ce / .last_lovasz are the two terms of the last call, on the device.  lovasz_ignore=None ignores nothing."""

    def __init__(self, ce_ignore: int = 255, lovasz_ignore=0, classes: str = "present"):
        super().__init__()
        _check_classes(classes, 0)
        self.ce_ignore = int(ce_ignore)
        self.lovasz_ignore = None if lovasz_ignore is None else int(lovasz_ignore)
        self.classes = classes
        self._ws = _Workspace()
        self.last_ce = None
        self.last_lovasz = None

    def forward(self, logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        _check_flat(logits, targets, "SegCriterion")
        _check_classes(self.classes, logits.shape[1])
        if _fused_ok(logits):
            total, ce, lov = _SegLossFn.apply(logits, targets, self._ws, L.SEGLOSS_LOGITS, self.ce_ignore, self.lovasz_ignore,
                                              self.classes)
        else:
            total, ce, lov = _torch_criterion(logits, targets, self.ce_ignore, self.lovasz_ignore, self.classes)
        self.last_ce, self.last_lovasz = ce.detach(), lov.detach()
        return total

    def extra_repr(self):
        return f"ce_ignore={self.ce_ignore}, lovasz_ignore={self.lovasz_ignore}, classes={self.classes!r}"


_FLAT_WS = _Workspace()


def _lovasz_flat(probas, labels, classes, ignore):
    _check_flat(probas, labels, "lovasz_softmax")
    _check_classes(classes, probas.shape[1])
    if _fused_ok(probas):
        return _SegLossFn.apply(probas, labels, _FLAT_WS, L.SEGLOSS_PROBAS, 255, ignore, classes)[0]
    return _torch_lovasz_flat(probas, labels, classes, ignore)


def lovasz_softmax_flat(probas: torch.Tensor, labels: torch.Tensor, classes="present") -> torch.Tensor:
    """lovasz_losses.py:174-202: probas [P, C], labels int64 [P]."""
    return _lovasz_flat(probas, labels, classes, None)


def _flatten(probas: torch.Tensor, labels: torch.Tensor):
    """flatten_probas (lovasz_losses.py:205-225) without its nonzero(): the ignore label goes down to the kernels instead."""
    if probas.dim() == 3:
        raise NotImplementedError("C = 1 (3-D probas: the sigmoid form of lovasz_softmax) is not built")
    if probas.dim() == 5:
        b, c, l, h, w = probas.shape
        probas = probas.contiguous().view(b, c, l, h * w)
    if probas.dim() != 4:
        raise ValueError(f"lovasz_softmax: probas [B, C, H, W] or [B, C, L, H, W] expected, got {tuple(probas.shape)}")
    c = probas.shape[1]
    flat = probas.permute(0, 2, 3, 1).contiguous().view(-1, c)
    labels = labels.reshape(-1)
    if labels.shape[0] != flat.shape[0]:
        raise ValueError(f"lovasz_softmax: {labels.shape[0]} labels for {flat.shape[0]} predictions")
    return flat, labels


def lovasz_softmax(probas: torch.Tensor, labels: torch.Tensor, classes="present", per_image: bool = False, ignore=None) -> torch.Tensor:
    """lovasz_losses.py:156-171: probas [B, C, H, W] (or [B, C, L, H, W]), labels [B, H, W]; per_image is a Python loop over the
    images, as there."""
    if not isinstance(probas, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise ValueError("lovasz_softmax: tensors expected")
    if not isinstance(classes, str):
        raise NotImplementedError("classes given as a list is not built: 'present' or 'all'")
    if per_image:
        losses = [_lovasz_flat(*_flatten(p.unsqueeze(0), l.unsqueeze(0)), classes, ignore) for p, l in zip(probas, labels)]
        return torch.stack(losses).mean()
    return _lovasz_flat(*_flatten(probas, labels), classes, ignore)
