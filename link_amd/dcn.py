"""link_amd/dcn.py -- deformable convolution (DCN v1) and the CenterHead modules built on it (csrc/dcn.hip, section R of
include/link_amd.h).

The surface of the reference's detection/det3d/ops/dcn/deform_conv.py (`deform_conv`, `DeformConv`, `DeformConvPack`) and of the
`dcn_head=True` branch of detection/det3d/models/bbox_heads/center_head.py (`FeatureAdaption`, `SepHead`, `DCNSepHead`), with
the same constructor arguments and parameter names, so a reference checkpoint's state dict loads with strict=True.  Modulated
(v2) convolution and deformable ROI pooling are not built.

Where a call runs: CUDA tensors of one type out of float32 / float16 / bfloat16, groups == 1, kh kw <= 49, C and O <= 256 and at
most 2^31 elements per tensor run the HIP kernels (`deform_conv_native` says so for a given call).  Everything else -- CPU
tensors, float64, groups > 1, wider layers -- runs `deform_conv_torch`, the same formula in plain differentiable torch.  The
16-bit forward reads and writes 16-bit tensors with fp32 coordinates and sums inside; the 16-bit backward runs the fp32 kernels on
widened tensors and rounds the three gradients once.  Under torch.autocast the tensors are taken in the type they arrive in (the
reference has no custom_fwd); the three tensors of a call must share one type.

grad_weight and grad_offset are reproducible run to run; grad_input is summed with fp32 atomics and is not (its last bits depend
on the order in which the adds arrive) -- the one exception to this library's deterministic training, see DESIGN.md section 4s.
A non-finite offset, or one that no int holds, contributes exactly 0 and receives a zero gradient (the reference's backward is
undefined there).  The grad_weight workspace is kept per device and grows on demand: one stream at a time, and the largest shape
has to run once before a graph is captured.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair, _single

from . import _lib as L

_IO = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}
_MAX_ELEMS = 1 << 31


def _out_size(size, k, stride, pad, dil):
    return (size + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def _check(input, offset, weight, stride, padding, dilation, groups, deformable_groups):
    """shape errors that hold for every path; returns (Ho, Wo)"""
    if input.dim() != 4:
        raise ValueError(f"Expected 4D tensor as input, got {input.dim()}D tensor instead.")
    if offset.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"deform_conv: offset {tuple(offset.shape)} and weight {tuple(weight.shape)} must be 4D")
    B, C, H, W = input.shape
    O, Cw, kh, kw = weight.shape
    if min(stride) < 1 or min(dilation) < 1 or min(padding) < 0 or groups < 1 or deformable_groups < 1:
        raise ValueError(f"deform_conv: stride {stride}, padding {padding}, dilation {dilation}, groups {groups}, "
                         f"deformable_groups {deformable_groups}")
    if C % groups or O % groups or Cw != C // groups:
        raise ValueError(f"deform_conv: input {tuple(input.shape)}, weight {tuple(weight.shape)}, groups {groups}")
    if C % deformable_groups:
        raise ValueError(f"deform_conv: {C} channels do not divide into {deformable_groups} deformable groups")
    Ho, Wo = _out_size(H, kh, stride[0], padding[0], dilation[0]), _out_size(W, kw, stride[1], padding[1], dilation[1])
    if Ho < 1 or Wo < 1:
        raise ValueError(f"convolution input is too small (output would be {B}x{O}x{Ho}x{Wo})")
    if tuple(offset.shape) != (B, deformable_groups * 2 * kh * kw, Ho, Wo):
        raise ValueError(f"deform_conv: offset {tuple(offset.shape)}, expected {(B, deformable_groups * 2 * kh * kw, Ho, Wo)}")
    if not (input.dtype == offset.dtype == weight.dtype) or not (input.device == offset.device == weight.device):
        raise TypeError(f"deform_conv: input {input.dtype} on {input.device}, offset {offset.dtype} on {offset.device}, weight "
                        f"{weight.dtype} on {weight.device}: one type and one device expected")
    return Ho, Wo


def deform_conv_native(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64) -> bool:
    """Whether deform_conv(...) with these arguments runs the HIP kernels (and not the torch composition)."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = _check(input, offset, weight, stride, padding, dilation, groups, deformable_groups)
    B, C, H, W = input.shape
    O, _, kh, kw = weight.shape
    if not input.is_cuda or input.dtype not in _IO or groups != 1:
        return False
    if kh * kw > L.DCN_MAX_TAPS or C > L.DCN_MAX_CHANNELS or O > L.DCN_MAX_CHANNELS:
        return False
    return max(input.numel(), offset.numel(), B * O * Ho * Wo) <= _MAX_ELEMS


def deform_conv_torch(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """The formula in plain differentiable torch: gathered corners, torch.where for the range test (a non-finite offset gives 0, not
    NaN), one contraction.  Any device and float type, any groups."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = _check(input, offset, weight, stride, padding, dilation, groups, deformable_groups)
    B, C, H, W = input.shape
    O, Cw, kh, kw = weight.shape
    dg, K = deformable_groups, kh * kw
    cg = C // dg
    dt, dev = input.dtype, input.device
    off = offset.reshape(B, dg, K, 2, Ho, Wo)
    ti = torch.arange(K, device=dev) // kw
    tj = torch.arange(K, device=dev) % kw
    base_h = (torch.arange(Ho, device=dev) * stride[0] - padding[0]).view(1, 1, 1, Ho, 1) + (ti * dilation[0]).view(1, 1, K, 1, 1)
    base_w = (torch.arange(Wo, device=dev) * stride[1] - padding[1]).view(1, 1, 1, 1, Wo) + (tj * dilation[1]).view(1, 1, K, 1, 1)
    h = base_h.to(dt) + off[:, :, :, 0]                                              # [B, dg, K, Ho, Wo]
    w = base_w.to(dt) + off[:, :, :, 1]
    ok = (h > -1) & (w > -1) & (h < H) & (w < W)
    zero = torch.zeros((), dtype=dt, device=dev)
    h, w = torch.where(ok, h, zero), torch.where(ok, w, zero)
    h0, w0 = torch.floor(h), torch.floor(w)
    lh, lw = h - h0, w - w0
    xg = input.reshape(B, dg, cg, 1, H * W).expand(B, dg, cg, K, H * W)
    cols = None
    for dh_, dw_, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        hi, wi = (h0 + dh_).long(), (w0 + dw_).long()
        inb = ok & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        idx = (hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1)).reshape(B, dg, 1, K, Ho * Wo).expand(B, dg, cg, K, Ho * Wo)
        v = torch.gather(xg, 4, idx) * torch.where(inb, wt, zero).reshape(B, dg, 1, K, Ho * Wo)
        cols = v if cols is None else cols + v
    cols = cols.reshape(B, groups, (C // groups) * K, Ho * Wo)                       # channel-major, tap-minor: weight's own order
    wmat = weight.reshape(groups, O // groups, Cw * K)
    return torch.einsum("bgkp,gok->bgop", cols, wmat).reshape(B, O, Ho, Wo)


class _Workspace:
    """grad_weight partials per device, grown on demand (one stream at a time, as the C entry asks)."""

    def __init__(self):
        self._buf = {}

    def get(self, device, need):
        buf = self._buf.get(device)
        if buf is None or buf.numel() < need:
            buf = self._buf[device] = torch.empty(need, dtype=torch.uint8, device=device)
        return buf


_WS = _Workspace()


def _geom(input, weight, offset, stride, padding, dilation, dg, io, relu):
    g = L.LinkDeformConvGeom()
    g.batch, g.c, g.h, g.w = (int(v) for v in input.shape)
    g.o, g.kh, g.kw = int(weight.shape[0]), int(weight.shape[2]), int(weight.shape[3])
    g.stride_h, g.stride_w = stride
    g.pad_h, g.pad_w = padding
    g.dil_h, g.dil_w = dilation
    g.groups, g.deformable_groups, g.offset_channels = 1, int(dg), int(offset.shape[1])
    g.io_dtype, g.flags = io, (L.DCN_RELU if relu else 0)
    return g


class _DeformConvFn(torch.autograd.Function):
    """the native path: forward in the tensors' type, backward in fp32"""

    @staticmethod
    def forward(ctx, input, offset, weight, stride, padding, dilation, dg, relu):
        input, offset, weight = input.contiguous(), offset.contiguous(), weight.contiguous()
        B, C, H, W = input.shape
        O, _, kh, kw = weight.shape
        Ho, Wo = _out_size(H, kh, stride[0], padding[0], dilation[0]), _out_size(W, kw, stride[1], padding[1], dilation[1])
        out = torch.empty((B, O, Ho, Wo), dtype=input.dtype, device=input.device)
        g = _geom(input, weight, offset, stride, padding, dilation, dg, _IO[input.dtype], relu)
        with torch.cuda.device(input.device):
            L.check(L.lib().link_deform_conv_forward(ctypes.byref(g), input.data_ptr(), offset.data_ptr(), weight.data_ptr(),
                                                     out.data_ptr(), L.current_stream_handle()), "link_deform_conv_forward")
        ctx.save_for_backward(input, offset, weight, out if relu else None)
        ctx.cfg = (stride, padding, dilation, dg, relu)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        input, offset, weight, out = ctx.saved_tensors
        stride, padding, dilation, dg, relu = ctx.cfg
        need_in, need_off, need_w = ctx.needs_input_grad[:3]
        dt = input.dtype
        x, o, w = input.float(), offset.float(), weight.float()
        y = None if out is None else out.float()
        go = grad_out.contiguous().float()
        g = _geom(x, w, o, stride, padding, dilation, dg, L.IO_F32, relu)
        gi = gf = gw = None
        with torch.cuda.device(input.device):
            stream = L.current_stream_handle()
            if need_in or need_off:
                gi = torch.empty_like(x) if need_in else None          # zeroed by the call, on the stream
                gf = torch.empty_like(o) if need_off else None
                L.check(L.lib().link_deform_conv_backward_data(ctypes.byref(g), x.data_ptr(), o.data_ptr(), w.data_ptr(), _ptr(y),
                                                               go.data_ptr(), _ptr(gi), _ptr(gf), stream), "link_deform_conv_backward_data")
            if need_w:
                need = L.lib().link_deform_conv_workspace_bytes(ctypes.byref(g))
                ws = _WS.get(input.device, need)
                gw = torch.empty_like(w)
                L.check(L.lib().link_deform_conv_backward_weight(ctypes.byref(g), x.data_ptr(), o.data_ptr(), _ptr(y), go.data_ptr(),
                                                                 gw.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                        "link_deform_conv_backward_weight")
        cast = (lambda t: None if t is None else t.to(dt))
        return cast(gi), cast(gf), cast(gw), None, None, None, None, None


def _ptr(t):
    return None if t is None else t.data_ptr()


def _deform_conv(input, offset, weight, stride, padding, dilation, groups, deformable_groups, relu):
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if deform_conv_native(input, offset, weight, stride, padding, dilation, groups, deformable_groups):
        return _DeformConvFn.apply(input, offset, weight, stride, padding, dilation, deformable_groups, relu)
    out = deform_conv_torch(input, offset, weight, stride, padding, dilation, groups, deformable_groups)
    return torch.relu(out) if relu else out


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
    """DeformConvFunction.apply of the reference (deform_conv.py:14-112), positional arguments alike.  im2col_step is accepted and
    ignored: no column matrix is built, so nothing has to divide the batch."""
    return _deform_conv(input, offset, weight, stride, padding, dilation, groups, deformable_groups, False)


def deform_conv_relu(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """relu(deform_conv(...)) with the ReLU inside the kernels' epilogue and its mask applied to grad_out on load."""
    return _deform_conv(input, offset, weight, stride, padding, dilation, groups, deformable_groups, True)


class DeformConv(nn.Module):
    """deform_conv.py:192-255: weight [out, in / groups, kh, kw], no bias."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0, f"in_channels {in_channels} cannot be divisible by groups {groups}"
        assert out_channels % groups == 0, f"out_channels {out_channels} cannot be divisible by groups {groups}"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
        self.groups, self.deformable_groups = groups, deformable_groups
        self.transposed, self.output_padding = False, _single(0)                     # as nn.Conv2d has them
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        self.weight.data.uniform_(-stdv, stdv)

    def forward(self, x, offset, relu: bool = False):
        # an input smaller than the kernel is padded at the bottom and right, and the output cut back (deform_conv.py:239-255)
        pad_h, pad_w = max(self.kernel_size[0] - x.size(2), 0), max(self.kernel_size[1] - x.size(3), 0)
        if pad_h or pad_w:
            x = F.pad(x, (0, pad_w, 0, pad_h), "constant", 0).contiguous()
            offset = F.pad(offset, (0, pad_w, 0, pad_h), "constant", 0).contiguous()
        out = _deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups, relu)
        if pad_h or pad_w:
            out = out[:, :, :out.size(2) - pad_h, :out.size(3) - pad_w].contiguous()
        return out


class DeformConvPack(DeformConv):
    """deform_conv.py:258-296: a DeformConv that predicts its own offsets with a zero-initialised convolution."""
    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deformable_groups * 2 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=self.stride, padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def forward(self, x):
        return deform_conv(x, self.conv_offset(x), self.weight, self.stride, self.padding, self.dilation, self.groups,
                           self.deformable_groups)


class FeatureAdaption(nn.Module):
    """center_head.py:27-65: a 1 x 1 offset convolution (torch's), a 3 x 3 DeformConv and a ReLU, which runs inside the kernel."""

    def __init__(self, in_channels, out_channels, kernel_size=3, deformable_groups=4):
        super().__init__()
        self.conv_offset = nn.Conv2d(in_channels, deformable_groups * kernel_size * kernel_size * 2, 1, bias=True)
        self.conv_adaption = DeformConv(in_channels, out_channels, kernel_size=kernel_size, padding=(kernel_size - 1) // 2,
                                        deformable_groups=deformable_groups)
        self.relu = nn.ReLU(inplace=True)                                            # kept for the module list; fused below
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()

    def forward(self, x):
        return self.conv_adaption(x, self.conv_offset(x), relu=True)


class SepHead(nn.Module):
    """center_head.py:67-112: one small convolution stack per regression head; heads = {name: (channels, num_conv)}."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, bn=False, init_bias=-2.19, **kwargs):
        super().__init__(**kwargs)
        self.heads = heads
        for head, (classes, num_conv) in heads.items():
            layers = []
            for _ in range(num_conv - 1):
                layers.append(nn.Conv2d(in_channels, head_conv, kernel_size=final_kernel, stride=1, padding=final_kernel // 2, bias=True))
                if bn:
                    layers.append(nn.BatchNorm2d(head_conv))
                layers.append(nn.ReLU())
            layers.append(nn.Conv2d(head_conv, classes, kernel_size=final_kernel, stride=1, padding=final_kernel // 2, bias=True))
            fc = nn.Sequential(*layers)
            if "hm" in head:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):                                     # det3d.torchie.cnn.kaiming_init's defaults
                        nn.init.kaiming_normal_(m.weight, a=0, mode="fan_out", nonlinearity="relu")
                        nn.init.constant_(m.bias, 0)
            setattr(self, head, fc)

    def forward(self, x):
        return {head: getattr(self, head)(x) for head in self.heads}


class DCNSepHead(nn.Module):
    """center_head.py:114-166, what CenterHead(dcn_head=True) builds per task: separate deformable feature adaptions for the heat
    map and for the regression heads.  Returns {'hm', <heads>...}: the maps CenterHeadLoss, CenterHeadDecoder and
    CenterHeadTTADecoder take.  The BatchNorm2d(64) of the heat-map stack is the reference's (head_conv = 64 assumed there)."""

    def __init__(self, in_channels, num_cls, heads, head_conv=64, final_kernel=1, bn=False, init_bias=-2.19, **kwargs):
        super().__init__(**kwargs)
        self.feature_adapt_cls = FeatureAdaption(in_channels, in_channels, kernel_size=3, deformable_groups=4)
        self.feature_adapt_reg = FeatureAdaption(in_channels, in_channels, kernel_size=3, deformable_groups=4)
        self.cls_head = nn.Sequential(nn.Conv2d(in_channels, head_conv, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(64),
                                      nn.ReLU(inplace=True), nn.Conv2d(head_conv, num_cls, kernel_size=3, stride=1, padding=1, bias=True))
        self.cls_head[-1].bias.data.fill_(init_bias)
        self.task_head = SepHead(in_channels, heads, head_conv=head_conv, bn=bn, final_kernel=final_kernel)

    def forward(self, x):
        center_feat = self.feature_adapt_cls(x)
        reg_feat = self.feature_adapt_reg(x)
        ret = self.task_head(reg_feat)
        ret["hm"] = self.cls_head(center_feat)
        return ret
