"""link_amd/voxelize.py -- point clouds to voxels on the device (csrc/voxelize.hip, section J of include/link_amd.h) behind the surfaces
of the reference's det3d.core.input.voxel_generator.VoxelGenerator, det3d.ops.point_cloud.point_cloud_ops.points_to_voxel and
det3d.models.readers.dynamic_voxel_encoder.DynamicVoxelEncoder.

The reference voxelises every frame on the host (a numba loop), ships [M, max_points, ndim] padded voxels to the device and reduces
them there with VoxelFeatureExtractorV3.  Here the points go to the device once and the per-voxel mean comes out of the same pass
that would write the voxels, so `Voxelizer.generate(points)` returns (features, coors, num_points) ready for SpMiddleResNetFHDELKv3;
the padded voxels exist only when asked for.  `generate` reads one number back (the voxel total: the size of what it returns);
`generate_padded` has fixed shapes, keeps the counts on the device and can be captured in a graph.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Union

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .index import MAX_CELLS, GridTooLarge

Points = Union[torch.Tensor, Sequence[torch.Tensor]]


def grid_size_of(voxel_size, point_cloud_range) -> np.ndarray:
    """round((hi - lo) / vs) in float32, half to even (voxel_generator.py:7-12) -> int64[3] = x, y, z"""
    rng = np.asarray(point_cloud_range, dtype=np.float32)
    vs = np.asarray(voxel_size, dtype=np.float32)
    return np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)


def _geom(voxel_size, point_cloud_range, grid, max_points: int, max_voxels: int, ndim: int, mode: int) -> L.LinkVoxelizeGeom:
    g = L.LinkVoxelizeGeom()
    for d in range(3):
        g.lo[d], g.hi[d], g.vs[d] = float(point_cloud_range[d]), float(point_cloud_range[3 + d]), float(voxel_size[d])
        g.grid[d] = int(grid[d])
    g.max_points, g.max_voxels, g.ndim, g.mode = int(max_points), int(max_voxels), int(ndim), int(mode)
    return g


class _Engine:
    """The geometry of one voxeliser, its workspaces (one per device and batch size, grown to the largest cloud seen; zeroed when
    allocated, left clean by every call) and the launch."""

    def __init__(self, voxel_size, point_cloud_range, mode: int):
        self.voxel_size = np.asarray(voxel_size, dtype=np.float32)
        self.range = np.asarray(point_cloud_range, dtype=np.float32)
        assert self.voxel_size.shape == (3,) and self.range.shape == (6,)
        self.grid = grid_size_of(self.voxel_size, self.range)
        self.mode = mode
        self._ws = {}
        self._offsets = {}

    def _workspace(self, g: L.LinkVoxelizeGeom, device, batch: int, ncap: int):
        cells = 1
        for d in range(3):
            cells *= int(self.grid[d]) + (1 if self.mode == L.VOXELIZE_DYNAMIC else 0)
        if cells > MAX_CELLS or cells * batch > (1 << 31) - 32 * batch:
            raise GridTooLarge(f"voxel grid of {cells} cells x {batch} samples (> {MAX_CELLS} per sample or 2^31 in all)")
        nbytes = L.lib().link_voxelize_workspace_bytes(ctypes.byref(g), ncap, batch)
        if nbytes == 0:
            raise L.LinkAmdError(f"link_voxelize: invalid geometry (voxel size {self.voxel_size}, grid {self.grid}, ndim {g.ndim}, "
                                 f"batch {batch})")
        key = (device, batch)                                            # the largest capacity seen stays
        ws = self._ws.get(key)
        if ws is None or ws.numel() * 4 < nbytes:
            ws = self._ws[key] = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)
        return ws, nbytes

    def run(self, points: Points, max_points: int, max_voxels: int, voxel_capacity, want_voxels: bool):
        """-> (voxels | None, mean [cap, ndim], coors int32 [cap, 4] = b, z, y, x, num_points int32 [cap], voxel_offsets int32 [B + 1])"""
        clouds: List[torch.Tensor] = [points] if isinstance(points, torch.Tensor) else list(points)
        assert len(clouds) >= 1, "at least one cloud"
        for c in clouds:
            if not isinstance(c, torch.Tensor) or not c.is_cuda:
                raise L.LinkAmdError("voxelize: link_amd runs on the GPU only (got a CPU tensor or an array); there is no CPU fallback")
            assert c.dim() == 2 and c.shape[1] == clouds[0].shape[1], "points are [n, ndim], the same ndim in every cloud"
        device, ndim, batch = clouds[0].device, int(clouds[0].shape[1]), len(clouds)
        if not 3 <= ndim <= 16:
            raise L.LinkAmdError(f"voxelize: ndim {ndim} outside 3..16")
        sizes = [int(c.shape[0]) for c in clouds]
        pts = (clouds[0] if batch == 1 else torch.cat(clouds)).contiguous().float()
        n = pts.shape[0]
        ncap = max(4096, 1 << max(n - 1, 0).bit_length())                # workspaces by powers of two: few sizes per voxeliser
        g = _geom(self.voxel_size, self.range, self.grid, max_points, max_voxels, ndim, self.mode)
        # The workspace is sized for ncap but the call is given n: the library lays the workspace out for the capacity it is given,
        # and that is sound only because the bitmap (the one part that must stay zero between calls) lies at offset 0 with a size
        # that follows grid and batch alone, and every other array is reset by each call (include/link_amd.h, section J).  A layout
        # that moved the bitmap with the capacity would break "left clean": then pass ncap here.
        ws, nbytes = self._workspace(g, device, batch, ncap)
        if voxel_capacity is None:
            voxel_capacity = min(n, batch * max_voxels) if self.mode == L.VOXELIZE_HARD else n
        cap = int(voxel_capacity)
        offs = L.point_offsets(self._offsets, device, sizes)
        mean = torch.empty((cap, ndim), dtype=torch.float32, device=device)
        coors = torch.empty((cap, 4), dtype=torch.int32, device=device)
        num = torch.empty((cap,), dtype=torch.int32, device=device)
        voff = torch.empty((batch + 1,), dtype=torch.int32, device=device)
        voxels = torch.empty((cap, max_points, ndim), dtype=torch.float32, device=device) if want_voxels else None
        with torch.cuda.device(device):
            L.check(L.lib().link_voxelize(ctypes.byref(g), pts.data_ptr(), offs.data_ptr(), batch, n, ws.data_ptr(), nbytes,
                                          voxels.data_ptr() if voxels is not None else None, mean.data_ptr(), coors.data_ptr(),
                                          num.data_ptr(), cap, voff.data_ptr(), L.current_stream_handle()), "link_voxelize")
        return voxels, mean, coors, num, voff


class Voxelizer:
    """VoxelGenerator (det3d/core/input/voxel_generator.py) on the device, with VoxelFeatureExtractorV3 (voxel_encoder.py:17-24) in
    the same pass.  `points` is one [n, ndim] GPU tensor or a list of them (a batch: every cloud is voxelised on its own, with its own
    max_voxels, and the rows are concatenated in order).  coors are int32 [M, 4] = b, z, y, x.  One Voxelizer serves one stream at
    a time (its workspaces are its own, not the process's)."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000):
        self._e = _Engine(voxel_size, point_cloud_range, L.VOXELIZE_HARD)
        self._max_num_points = int(max_num_points)
        self._max_voxels = int(max_voxels)

    voxel_size = property(lambda self: self._e.voxel_size)
    point_cloud_range = property(lambda self: self._e.range)
    grid_size = property(lambda self: self._e.grid)
    max_num_points_per_voxel = property(lambda self: self._max_num_points)

    def _mv(self, max_voxels):
        return self._max_voxels if max_voxels == -1 else int(max_voxels)

    @torch.no_grad()
    def generate_padded(self, points: Points, max_voxels=-1, return_voxels=False, capacity=None):
        """Fixed shapes, no host round trip: (features [cap, ndim], coors [cap, 4], num_points [cap], voxel_offsets int32 [B + 1] on
        the device), preceded by voxels [cap, max_points, ndim] with return_voxels.  cap = `capacity`, by default min(points,
        B max_voxels); rows past voxel_offsets[B] are zero."""
        voxels, mean, coors, num, voff = self._e.run(points, self._max_num_points, self._mv(max_voxels), capacity, return_voxels)
        return (voxels, mean, coors, num, voff) if return_voxels else (mean, coors, num, voff)

    @torch.no_grad()
    def generate(self, points: Points, max_voxels=-1, return_voxels=False):
        """Variable length: (features [M, ndim], coors [M, 4], num_points [M]), preceded by voxels [M, max_points, ndim] with
        return_voxels.  One host round trip: M."""
        voxels, mean, coors, num, voff = self._e.run(points, self._max_num_points, self._mv(max_voxels), None, return_voxels)
        m = int(voff[-1].item())
        out = (mean[:m], coors[:m], num[:m])
        return (voxels[:m],) + out if return_voxels else out


def points_to_voxel(points, voxel_size, coors_range, max_points=35, reverse_index=True, max_voxels=20000):
    """point_cloud_ops.py:112-184 on a GPU tensor -> (voxels [M, max_points, ndim], coors int32 [M, 3], num_points_per_voxel int32 [M]);
    coors are z, y, x, or x, y, z with reverse_index=False."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise L.LinkAmdError("points_to_voxel: link_amd runs on the GPU only; there is no CPU fallback")
    e = _Engine(voxel_size, coors_range, L.VOXELIZE_HARD)
    voxels, _, coors, num, voff = e.run(points, int(max_points), int(max_voxels), None, True)
    m = int(voff[-1].item())
    zyx = coors[:m, 1:]
    return voxels[:m], (zyx if reverse_index else zyx.flip(1)).contiguous(), num[:m]


class DynamicVoxelEncoder(nn.Module):
    """det3d/models/readers/dynamic_voxel_encoder.py:70-102 with virtual=False: forward(list of [n, ndim] GPU tensors) ->
    (voxels [M, ndim] = the mean of every voxel's points, coors int64 [M, 4] = b, z, y, x in ascending order per sample, shape_np)."""

    def __init__(self, pc_range, voxel_size, virtual=False):
        super().__init__()
        if virtual:
            raise NotImplementedError("DynamicVoxelEncoder: virtual=True (voxelization_virtual) is not built")
        self.pc_range = torch.tensor(pc_range, dtype=torch.float32)
        self.voxel_size = torch.tensor(voxel_size, dtype=torch.float32)
        self.shape = torch.round((self.pc_range[3:] - self.pc_range[:3]) / self.voxel_size)
        self.shape_np = self.shape.numpy().astype(np.int32)
        self.virtual = False
        self._e = _Engine(self.voxel_size.numpy(), self.pc_range.numpy(), L.VOXELIZE_DYNAMIC)

    @torch.no_grad()
    def forward(self, points: Sequence[torch.Tensor]):
        _, mean, coors, _, voff = self._e.run(list(points), 1, 1, None, False)
        m = int(voff[-1].item())
        return mean[:m], coors[:m].long(), self.shape_np
