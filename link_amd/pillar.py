"""link_amd/pillar.py -- the PointPillars reader and its BEV scatter (csrc/pillar.hip, section S of include/link_amd.h).

The surface of the reference's detection/det3d/models/readers/pillar_encoder.py (`PFNLayer`, `PillarFeatureNet`,
`PointPillarsScatter`) with the same constructor arguments and parameter names (`pfn_layers.{i}.linear.weight`,
`pfn_layers.{i}.norm.*`), so a reference checkpoint's state dict loads with strict=True, plus `PillarReader`, the two modules
fused: padded voxels in, the [B, C, ny, nx] pseudo-image out, with no [P, C] array in between.

Where a call runs.  `model.eval()` on CUDA float32 voxels inside the native range (`pillar_native`: 1 or 2 layers, every width a
multiple of 16 up to 128, 3 <= D <= 8, T <= 64) runs ONE kernel: decoration, mask, both layers with BatchNorm as a per-channel
affine after the dot product, ReLU and the max.  `model.train()` runs the decoration kernel and then torch's own Linear /
BatchNorm1d / ReLU / max on the decorated rows, so batch statistics run over all P T rows, padded ones included, the running
statistics update and autograd gives the weight gradients, all as in the reference.  Anything else (CPU tensors, float64, wider
layers, more than two layers) runs the torch composition of the reference's steps.  `virtual=True` is not built and raises.

Differences from the reference, all deliberate:
  * the reader returns [P, C] always; the reference squeezes, so P = 1 gives [C] there.
  * `count=` (keyword, every forward): a device int32 tensor of one element, the number of live rows; rows at or past it are inert
    (zero rows from the reader, nothing written by the scatter).  `voxel_offsets[B:]` of `Voxelizer.generate_padded` is one, so
    the chain points -> voxels -> canvas needs no host round trip and can be captured in a graph.  In train mode the inert
    pillars enter the batch statistics as all-padded pillars do; pass exactly the live rows (`Voxelizer.generate`) where the
    statistics must be the reference's.
  * a pillar with num_voxels == 0 gives the value of an all-padded pillar; the reference divides 0 by 0 there (NaN).
  * the fused eval-mode kernel is inference only: it runs under no_grad and its result carries no graph, whatever requires grad.  A
    reader kept in eval() for frozen BatchNorm while its weights train gets no weight gradients that way: call
    `reader.forward_torch(...)` there (differentiable, running statistics used as they are), or train().
  * the mean is the sum over the rows t < num (clamped to T) divided by num: padded input rows are taken to be zero, as every
    voxel generator here and in the reference writes them.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib as L

_IO = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}


def _build_norm(norm_cfg, units):
    if norm_cfg is None:
        norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
    cfg = dict(norm_cfg)
    kind = cfg.pop("type")
    if kind not in ("BN1d", "BN"):
        raise NotImplementedError(f"PFNLayer: norm type {kind!r} (the reference's configs use BN1d)")
    cfg.pop("requires_grad", None)
    cfg.setdefault("eps", 1e-5)
    return nn.BatchNorm1d(units, **cfg)


def _geom(T=1, D=3, with_distance=False, widths=(), batch=1, ny=1, nx=1, io=L.IO_F32, vx=0.0, vy=0.0, x_offset=0.0, y_offset=0.0):
    g = L.LinkPillarGeom()
    g.struct_bytes = ctypes.sizeof(L.LinkPillarGeom)
    g.t, g.d, g.with_distance, g.layers = int(T), int(D), int(bool(with_distance)), len(widths)
    for i, w in enumerate(widths[:2]):
        g.width[i] = int(w)
    g.batch, g.ny, g.nx, g.io_dtype = int(batch), int(ny), int(nx), io
    g.vx, g.vy, g.x_offset, g.y_offset = float(vx), float(vy), float(x_offset), float(y_offset)
    return g


def pillar_config_native(num_input_features: int, max_points: int, num_filters: Sequence[int], virtual: bool = False) -> bool:
    """Whether a reader of this shape is inside the fused kernel's range (the library's own table: link_pillar_native)."""
    widths = tuple(int(w) for w in num_filters)
    if virtual or not 1 <= len(widths) <= 2:
        return False
    return bool(L.lib().link_pillar_native(ctypes.byref(_geom(max_points, num_input_features, False, widths))))


def pillar_native(reader: "PillarFeatureNet", features: torch.Tensor) -> bool:
    """Whether reader(features, ...) -- and PillarReader on it -- runs the fused HIP kernel (and not the torch composition)."""
    if reader.training or features.dim() != 3 or not features.is_cuda or features.dtype != torch.float32:
        return False
    if features.shape[2] != reader.num_input or any(type(l.norm) is not nn.BatchNorm1d or not l.norm.track_running_stats or
                                                    not l.norm.affine for l in reader.pfn_layers):
        return False
    if any(t.device != features.device for t in list(reader.parameters()) + list(reader.buffers())):
        return False                  # the composition then raises torch's own device-mismatch error
    return pillar_config_native(features.shape[2], features.shape[1], reader.num_filters, reader.virtual)


def _int32(t):
    """t as contiguous int32.  For any other type this is a NEW tensor: the caller binds it to a name that lives until the launch
    is issued -- a temporary would hand its block back to the allocator, and the next conversion would be written over it."""
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()


def _out_dtype(out_dtype):
    dt = torch.float32 if out_dtype is None else out_dtype
    if dt not in _IO:
        raise TypeError(f"out_dtype {out_dtype}: torch.float32, torch.float16 or torch.bfloat16")
    return dt


def _count(count, device):
    if count is None:
        return None
    if not isinstance(count, torch.Tensor):
        raise TypeError("count: a device int32 tensor of one element (voxel_offsets[B:]), or None")
    assert count.numel() == 1 and count.device == device, "count: one element on the tensors' device"
    return _int32(count.reshape(1))


def _live_mask(count, P, device):
    return torch.arange(P, device=device) < count.reshape(1).clamp(0, P)


# ---------------------------------------------------------------------------------------------------------------------------------
class _ScatterFn(torch.autograd.Function):
    """link_pillar_scatter and its adjoint link_pillar_gather"""

    @staticmethod
    def forward(ctx, rows, coors, count, batch, ny, nx):
        rows = rows.contiguous()
        P, C = rows.shape
        canvas = torch.empty((batch, C, ny, nx), dtype=rows.dtype, device=rows.device)     # zero-filled by the call, on the stream
        g = _geom(batch=batch, ny=ny, nx=nx, io=_IO[rows.dtype])
        with torch.cuda.device(rows.device):
            L.check(L.lib().link_pillar_scatter(ctypes.byref(g), rows.data_ptr(), coors.data_ptr(), P, C, L.ptr(count), canvas.data_ptr(),
                                                L.current_stream_handle()), "link_pillar_scatter")
        ctx.save_for_backward(coors, count)
        ctx.cfg = (P, C, batch, ny, nx)
        return canvas

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        coors, count = ctx.saved_tensors
        P, C, batch, ny, nx = ctx.cfg
        grad = grad.contiguous()
        out = torch.empty((P, C), dtype=grad.dtype, device=grad.device)
        g = _geom(batch=batch, ny=ny, nx=nx, io=_IO[grad.dtype])
        with torch.cuda.device(grad.device):
            L.check(L.lib().link_pillar_gather(ctypes.byref(g), grad.data_ptr(), coors.data_ptr(), P, C, L.ptr(count), out.data_ptr(),
                                               L.current_stream_handle()), "link_pillar_gather")
        return out, None, None, None, None, None


def scatter_torch(rows, coors, batch, ny, nx, count=None):
    """PointPillarsScatter's indexed assignment in plain torch, any device and type.  Inert rows and rows whose cell lies outside
    the canvas go to a spare cell that is cut off."""
    P, C = rows.shape
    c = coors.long()
    ok = (c[:, 0] >= 0) & (c[:, 0] < batch) & (c[:, 2] >= 0) & (c[:, 2] < ny) & (c[:, 3] >= 0) & (c[:, 3] < nx)
    if count is not None:
        ok = ok & _live_mask(count, P, rows.device)
    cell = torch.where(ok, (c[:, 0] * ny + c[:, 2]) * nx + c[:, 3], torch.full_like(c[:, 0], batch * ny * nx))
    flat = rows.new_zeros((batch * ny * nx + 1, C))
    flat = flat.index_put((cell,), rows)
    return flat[:-1].view(batch, ny, nx, C).permute(0, 3, 1, 2).contiguous()


def pillar_scatter(rows, coors, batch_size, ny, nx, count=None):
    """rows [P, C] -> canvas [B, C, ny, nx]: zero everywhere but at (b, :, y, x) of every live pillar.  Differentiable in rows."""
    assert rows.dim() == 2 and coors.dim() == 2 and coors.shape[1] == 4 and coors.shape[0] == rows.shape[0]
    if rows.is_cuda and rows.dtype in _IO:
        return _ScatterFn.apply(rows, _int32(coors), _count(count, rows.device), int(batch_size), int(ny), int(nx))
    return scatter_torch(rows, coors, int(batch_size), int(ny), int(nx), count)


# ---------------------------------------------------------------------------------------------------------------------------------
def decorate_torch(features, num_voxels, coors, vx, vy, x_offset, y_offset, with_distance, count=None):
    """the reference's decoration and mask (pillar_encoder.py:129-156) in plain torch; num == 0 divides by 1"""
    P, T, _ = features.shape
    dt = features.dtype
    num = num_voxels.clamp(0, T)
    if count is not None:
        num = torch.where(_live_mask(count, P, features.device), num, torch.zeros_like(num))
    mask = (torch.arange(T, device=features.device).view(1, T) < num.view(P, 1)).to(dt).unsqueeze(-1)
    xyz = features[:, :, :3]
    mean = (xyz * mask).sum(dim=1, keepdim=True) / num.clamp(min=1).to(dt).view(P, 1, 1)
    cx = coors[:, 3].to(dt).view(P, 1) * vx + x_offset
    cy = coors[:, 2].to(dt).view(P, 1) * vy + y_offset
    parts = [features, xyz - mean, (features[:, :, 0] - cx).unsqueeze(-1), (features[:, :, 1] - cy).unsqueeze(-1)]
    if with_distance:
        parts.append(torch.norm(xyz, 2, 2, keepdim=True))
    return torch.cat(parts, dim=-1) * mask


def pillar_decorate(features, num_voxels, coors, vx, vy, x_offset, y_offset, with_distance=False, count=None):
    """[P, T, D] -> masked [P, T, D + 5 (+ 1)]; the device kernel for CUDA float32 with 3 <= D <= 8 and T <= 64, torch otherwise.
    The inputs are data: no gradient flows to them."""
    P, T, D = features.shape
    if not (features.is_cuda and features.dtype == torch.float32 and 3 <= D <= L.PILLAR_MAX_D and 1 <= T <= L.PILLAR_MAX_T):
        return decorate_torch(features, num_voxels, coors, vx, vy, x_offset, y_offset, with_distance, count)
    with torch.no_grad():
        x = features.detach().contiguous()
        out = torch.empty((P, T, D + 5 + int(bool(with_distance))), dtype=torch.float32, device=x.device)
        g = _geom(T, D, with_distance, vx=vx, vy=vy, x_offset=x_offset, y_offset=y_offset)
        num32, coors32, count32 = _int32(num_voxels), _int32(coors), _count(count, x.device)      # alive until the launch is issued
        with torch.cuda.device(x.device):
            L.check(L.lib().link_pillar_decorate(ctypes.byref(g), x.data_ptr(), num32.data_ptr(), coors32.data_ptr(), P, L.ptr(count32),
                                                 out.data_ptr(), L.current_stream_handle()), "link_pillar_decorate")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
class PFNLayer(nn.Module):
    """pillar_encoder.py:15-55: Linear(bias=False), BatchNorm1d over the channel, ReLU, max over all T rows; a layer that is not the
    last has out_channels // 2 units and returns [x, x_max repeated]."""

    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__()
        self.name = "PFNLayer"
        self.last_vfe = last_layer
        if not self.last_vfe:
            out_channels = out_channels // 2
        self.units = out_channels
        self.norm_cfg = norm_cfg
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = _build_norm(norm_cfg, self.units)

    def forward(self, inputs):
        x = self.linear(inputs)
        # torch's own BatchNorm kernels, not the vendor library's: the reference switches the library off around this call
        # (pillar_encoder.py:43-45).  Measured on the recorded train case, whose channels have means far from 0 (raw coordinates
        # times a weight): the canvas lies 1.0e-5 from float64 this way and 2.1e-5 through the library
        with torch.backends.cudnn.flags(enabled=False):
            x = self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1)
        x = F.relu(x)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.expand(-1, inputs.shape[1], -1)], dim=2)


def _layer_arg(layer: PFNLayer, keep: list):
    """link_pillar_layer_t of a layer: the module's own tensors (fp32 on the device: no copy is made then)"""
    ts = [t.detach().float().contiguous() for t in (layer.linear.weight, layer.norm.weight, layer.norm.bias, layer.norm.running_mean,
                                                    layer.norm.running_var)]
    keep.extend(ts)
    a = L.LinkPillarLayer()
    a.weight, a.gamma, a.beta, a.running_mean, a.running_var = (t.data_ptr() for t in ts)
    a.eps = float(layer.norm.eps)
    return a


class PillarFeatureNet(nn.Module):
    """pillar_encoder.py:58-162.  forward(features [P, T, D], num_voxels [P], coors [P, 4] = b, z, y, x, count=None) -> [P, C]
    (always two-dimensional: the reference squeezes, so P = 1 gives [C] there)."""

    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None, virtual=False):
        super().__init__()
        if virtual:
            raise NotImplementedError("PillarFeatureNet: virtual=True (virtual points) is not built")
        self.name = "PillarFeatureNet"
        assert len(num_filters) > 0
        self.num_input = num_input_features
        self.num_filters = tuple(int(f) for f in num_filters)
        self._with_distance = bool(with_distance)
        widths = [num_input_features + 5 + int(self._with_distance)] + list(self.num_filters)
        self.pfn_layers = nn.ModuleList(PFNLayer(widths[i], widths[i + 1], norm_cfg=norm_cfg, last_layer=i == len(widths) - 2)
                                        for i in range(len(widths) - 1))
        self.virtual = False
        self.vx, self.vy = voxel_size[0], voxel_size[1]
        self.x_offset = self.vx / 2 + pc_range[0]
        self.y_offset = self.vy / 2 + pc_range[1]

    out_channels = property(lambda self: self.num_filters[-1])

    def _check(self, features, num_voxels, coors):
        assert features.dim() == 3 and features.shape[2] == self.num_input, (tuple(features.shape), self.num_input)
        P = features.shape[0]
        assert num_voxels.shape == (P,) and coors.shape == (P, 4), (tuple(num_voxels.shape), tuple(coors.shape))

    def _layers(self, decorated):
        x = decorated
        for pfn in self.pfn_layers:
            x = pfn(x)
        return x.reshape(decorated.shape[0], self.out_channels)

    def forward_torch(self, features, num_voxels, coors, count=None):
        """the composition of the reference's steps in plain torch (any device and type)"""
        dec = decorate_torch(features, num_voxels, coors, self.vx, self.vy, self.x_offset, self.y_offset, self._with_distance, count)
        out = self._layers(dec)
        return out if count is None else out * _live_mask(count, out.shape[0], out.device).to(out.dtype).unsqueeze(1)

    def _fused(self, features, num_voxels, coors, count, canvas_shape, out_dtype):
        P, T, D = features.shape
        x = features.detach().contiguous()
        dev = x.device
        num32, coors32, count = _int32(num_voxels), _int32(coors), _count(count, dev)            # alive until the launch is issued
        keep = []
        layers = [_layer_arg(l, keep) for l in self.pfn_layers]
        C = self.out_channels
        if canvas_shape is None:
            g = _geom(T, D, self._with_distance, self.num_filters, io=_IO[out_dtype], vx=self.vx, vy=self.vy, x_offset=self.x_offset,
                      y_offset=self.y_offset)
            rows = (torch.zeros if count is not None else torch.empty)((P, C), dtype=out_dtype, device=dev)
            canvas = None
        else:
            batch, ny, nx = canvas_shape
            g = _geom(T, D, self._with_distance, self.num_filters, batch, ny, nx, _IO[out_dtype], self.vx, self.vy, self.x_offset,
                      self.y_offset)
            rows, canvas = None, torch.empty((batch, C, ny, nx), dtype=out_dtype, device=dev)   # zero-filled by the call
        with torch.cuda.device(dev):
            L.check(L.lib().link_pillar_reader(ctypes.byref(g), x.data_ptr(), num32.data_ptr(), coors32.data_ptr(), P, L.ptr(count),
                                               ctypes.byref(layers[0]), ctypes.byref(layers[1]) if len(layers) == 2 else None,
                                               L.ptr(rows), L.ptr(canvas), L.current_stream_handle()), "link_pillar_reader")
        return rows if canvas is None else canvas

    def forward(self, features, num_voxels, coors, count=None, out_dtype=None):
        self._check(features, num_voxels, coors)
        if pillar_native(self, features):
            with torch.no_grad():
                return self._fused(features, num_voxels, coors, count, None, _out_dtype(out_dtype))
        if self.training:
            dec = pillar_decorate(features, num_voxels, coors, self.vx, self.vy, self.x_offset, self.y_offset, self._with_distance, count)
            out = self._layers(dec)
            out = out if count is None else out * _live_mask(count, out.shape[0], out.device).to(out.dtype).unsqueeze(1)
        else:
            out = self.forward_torch(features, num_voxels, coors, count)
        return out if out_dtype is None else out.to(_out_dtype(out_dtype))


class PointPillarsScatter(nn.Module):
    """pillar_encoder.py:165-218.  forward(voxel_features [P, C], coords [P, 4] = b, z, y, x, batch_size, input_shape = (nx, ny, ...),
    count=None) -> [B, C, ny, nx]."""

    def __init__(self, num_input_features=64, norm_cfg=None, name="PointPillarsScatter", **kwargs):
        super().__init__()
        self.name = "PointPillarsScatter"
        self.nchannels = num_input_features

    def forward(self, voxel_features, coords, batch_size, input_shape, count=None):
        self.nx, self.ny = int(input_shape[0]), int(input_shape[1])
        assert voxel_features.dim() == 2 and voxel_features.shape[1] == self.nchannels, (tuple(voxel_features.shape), self.nchannels)
        return pillar_scatter(voxel_features, coords, batch_size, self.ny, self.nx, count)


class PillarReader(nn.Module):
    """reader + scatter as one call: forward(features, num_voxels, coors, batch_size, input_shape, count=None, out_dtype=None) ->
    [B, C, ny, nx].  In eval mode inside the native range this is one kernel that writes the canvas directly (after the zero fill);
    otherwise scatter(reader(...)).  With `voxels, _, coors, num, voff = Voxelizer.generate_padded(points, return_voxels=True)`:
    `PillarReader(...)(voxels, num, coors, B, grid_size, count=voff[B:])` -- fixed shapes, no host round trip, graph-capturable."""

    def __init__(self, reader: PillarFeatureNet, scatter: Optional[PointPillarsScatter] = None):
        super().__init__()
        self.reader = reader
        self.scatter = scatter if scatter is not None else PointPillarsScatter(reader.out_channels)
        assert self.scatter.nchannels == reader.out_channels, (self.scatter.nchannels, reader.out_channels)

    def forward(self, features, num_voxels, coors, batch_size, input_shape, count=None, out_dtype=None):
        if pillar_native(self.reader, features):
            self.reader._check(features, num_voxels, coors)
            nx, ny = int(input_shape[0]), int(input_shape[1])
            with torch.no_grad():
                return self.reader._fused(features, num_voxels, coors, count, (int(batch_size), ny, nx), _out_dtype(out_dtype))
        return self.scatter(self.reader(features, num_voxels, coors, count=count, out_dtype=out_dtype), coors, batch_size, input_shape,
                            count=count)


def pillar_bev(reader, features, num_voxels, coors, batch_size, input_shape, count=None, out_dtype=None):
    """PillarReader(reader)(...) as a function"""
    return PillarReader(reader)(features, num_voxels, coors, batch_size, input_shape, count=count, out_dtype=out_dtype)
