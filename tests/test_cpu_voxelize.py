"""CPU-only checks of the voxelisation entries (csrc/voxelize.hip, section J of include/link_amd.h): the float32 restatements of
tests/voxel_oracle.py against every fixture recorded from the reference (tests/golden/make_golden_voxelize.py), exports and prototypes,
the struct layout, argument validation before anything touches a device, and the host grid computation."""
import ctypes
import os

import numpy as np
import pytest

from helpers import ROOT, golden_files, load_golden

import voxel_oracle as VO

HARD, DYN = VO.HARD, VO.DYN


def test_fixtures_are_complete():
    assert golden_files("voxelize_hard_*.npz") == sorted(f"voxelize_hard_{n}.npz" for n in HARD)
    assert golden_files("voxelize_dyn_*.npz") == sorted(f"voxelize_dyn_{n}.npz" for n in DYN)
    for name in golden_files("voxelize_*.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20), name
    g = load_golden("voxelize_hard_capped.npz")
    assert g["coors0"].shape[0] == g["meta"]["max_voxels"] == 3000            # more occupied cells than max_voxels
    assert VO.hard(g["points0"], g["voxel_size"], g["range"], 10, 1 << 30)[1].shape[0] > 3000
    assert load_golden("voxelize_hard_onevoxel.npz")["num0"].tolist() == [10]   # 100 points, the cap keeps ten
    assert (load_golden("voxelize_hard_clustered.npz")["num0"] == 10).sum() > 50
    full = load_golden("voxelize_hard_full.npz")
    assert full["shape"].tolist() == [1440, 1440, 40]
    corners = {(z, y, x) for z in (0, 39) for y in (0, 1439) for x in (0, 1439)}
    assert corners <= {tuple(r) for r in full["coors0"].tolist()}
    assert load_golden("voxelize_dyn_edges.npz")["coors"][:, 1:].max(0).tolist() == [40, 160, 160]     # the inclusive upper bound


@pytest.mark.parametrize("name", HARD)
def test_hard_restatement_equals_reference(name):
    g = load_golden(f"voxelize_hard_{name}.npz")
    m = g["meta"]
    for k in range(m["clouds"]):
        voxels, coors, num = VO.hard(g[f"points{k}"], g["voxel_size"], g["range"], m["max_points"], m["max_voxels"], m["reverse_index"])
        assert coors.dtype == g[f"coors{k}"].dtype == np.int32
        assert np.array_equal(coors, g[f"coors{k}"]) and np.array_equal(num, g[f"num{k}"])
        assert voxels.tobytes() == g[f"voxels{k}"].tobytes()
        # VoxelFeatureExtractorV3 in float32 (a sequential sum of the rows) lies within the bound the GPU test uses
        mean64, bound = VO.hard_mean64(g[f"voxels{k}"], g[f"num{k}"])
        acc = np.zeros(mean64.shape, np.float32)
        for j in range(m["max_points"]):
            acc = acc + g[f"voxels{k}"][:, j]
        mean32 = acc / np.maximum(num, 1).astype(np.float32)[:, None]
        assert np.all(np.abs(mean32.astype(np.float64) - mean64) <= bound)


@pytest.mark.parametrize("name", DYN)
def test_dynamic_restatement_equals_reference(name):
    g = load_golden(f"voxelize_dyn_{name}.npz")
    coors, means, bounds = [], [], []
    for k in range(g["meta"]["clouds"]):
        c, _, mean64, bound = VO.dynamic(g[f"points{k}"], g["range"], g["voxel_size"])
        coors.append(np.concatenate([np.full((c.shape[0], 1), k, np.int64), c], 1))
        means.append(mean64); bounds.append(bound)
    assert g["coors"].dtype == np.int64 and np.array_equal(np.concatenate(coors), g["coors"])
    assert np.all(np.abs(g["voxels"].astype(np.float64) - np.concatenate(means)) <= np.concatenate(bounds))
    assert np.array_equal(VO.grid_of(g["voxel_size"], g["range"]), g["shape"])


def test_host_grid_equals_the_fixtures_shape():
    from link_amd.voxelize import grid_size_of
    import link_amd as la
    for name in golden_files("voxelize_*.npz"):
        g = load_golden(name)
        assert np.array_equal(grid_size_of(g["voxel_size"], g["range"]), g["shape"]), name
    v = la.Voxelizer([0.075, 0.075, 0.2], [-54, -54, -5.0, 54, 54, 3.0], 10, 120000)
    assert v.grid_size.tolist() == [1440, 1440, 40] and v.grid_size.dtype == np.int64
    assert v.voxel_size.dtype == np.float32 and v.point_cloud_range.dtype == np.float32 and v.max_num_points_per_voxel == 10
    # half to even, in float32: 2.5 -> 2, 3.5 -> 4
    assert grid_size_of([1.0, 1.0, 1.0], [0, 0, 0, 2.5, 3.5, 1.0]).tolist() == [2, 4, 1]


def _geom(**kw):
    from link_amd import _lib as L
    g = L.LinkVoxelizeGeom()
    for d in range(3):
        g.lo[d], g.hi[d], g.vs[d], g.grid[d] = -6.0, 6.0, 0.075, 160
    g.max_points, g.max_voxels, g.ndim, g.mode = 10, 20000, 5, L.VOXELIZE_HARD
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for d in range(3):
                getattr(g, k)[d] = v[d]
        else:
            setattr(g, k, v)
    return g


def test_section_j_symbols_struct_and_version():
    from link_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in ("link_voxelize", "link_voxelize_workspace_bytes"):
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13                  # additive entries
    assert ctypes.sizeof(L.LinkVoxelizeGeom) == 16 * 4
    assert L.lib().link_abi_struct_size(L.STRUCT_VOXELIZE_GEOM) == ctypes.sizeof(L.LinkVoxelizeGeom)


def test_section_j_validates_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(64)                                            # a non-null, aligned pointer nothing dereferences

    def call(g, ncap=1000, batch=1, ws=one, nbytes=None, vcap=1000):
        if nbytes is None:
            nbytes = lib.link_voxelize_workspace_bytes(ctypes.byref(g), ncap, batch)
        return lib.link_voxelize(ctypes.byref(g), one, one, batch, ncap, ws, nbytes, None, one, one, one, vcap, one, None)

    good = _geom()
    need = lib.link_voxelize_workspace_bytes(ctypes.byref(good), 1000, 1)
    assert need >= 160 * 160 * 40 // 8 * 2 + 40 * 1000
    assert lib.link_voxelize_workspace_bytes(ctypes.byref(good), 1000, 3) > need
    bad = [_geom(ndim=2), _geom(ndim=17), _geom(vs=[0.075, 0.0, 0.2]), _geom(vs=[-0.075, 0.075, 0.2]), _geom(vs=[float("nan")] * 3),
           _geom(grid=[160, 0, 40]), _geom(grid=[160, 160, -1]), _geom(mode=2), _geom(max_points=0), _geom(max_voxels=0),
           _geom(grid=[1440, 1440, 400]),                                 # 8.3e8 cells: too large for one sample
           _geom(grid=[1 << 24, 1, 1])]
    for g in bad:
        assert lib.link_voxelize_workspace_bytes(ctypes.byref(g), 1000, 1) == 0
        assert call(g, nbytes=1 << 40) == L.LINK_ERR_ARG
    full = _geom(grid=[1440, 1440, 40])
    assert lib.link_voxelize_workspace_bytes(ctypes.byref(full), 1000, 25) > 0
    assert lib.link_voxelize_workspace_bytes(ctypes.byref(full), 1000, 26) == 0          # 2^31 bits over all samples
    assert call(full, batch=26, nbytes=1 << 40) == L.LINK_ERR_ARG
    assert call(good, batch=0, nbytes=1 << 40) == L.LINK_ERR_ARG and call(good, batch=1025, nbytes=1 << 40) == L.LINK_ERR_ARG
    assert call(good, ncap=-1, nbytes=1 << 40) == L.LINK_ERR_ARG and call(good, vcap=-1) == L.LINK_ERR_ARG
    assert call(good, nbytes=need - 1) == L.LINK_ERR_WORKSPACE and call(good, nbytes=0) == L.LINK_ERR_WORKSPACE
    assert call(good, ws=None) == L.LINK_ERR_ARG
    assert lib.link_voxelize(None, one, one, 1, 1000, one, need, None, one, one, one, 1000, one, None) == L.LINK_ERR_ARG
    assert lib.link_voxelize(ctypes.byref(good), None, one, 1, 1000, one, need, None, one, one, one, 1000, one, None) == L.LINK_ERR_ARG
    assert lib.link_voxelize(ctypes.byref(good), one, None, 1, 1000, one, need, None, one, one, one, 1000, one, None) == L.LINK_ERR_ARG
    assert lib.link_voxelize(ctypes.byref(good), one, one, 1, 1000, one, need, None, None, one, one, 1000, one, None) == L.LINK_ERR_ARG
    dyn = _geom(mode=L.VOXELIZE_DYNAMIC)
    assert lib.link_voxelize_workspace_bytes(ctypes.byref(dyn), 1000, 1) >= 161 * 161 * 41 // 8 * 2
    assert lib.link_voxelize(ctypes.byref(dyn), one, one, 1, 1000, one, 1 << 40, one, one, one, one, 1000, one, None) == L.LINK_ERR_ARG


def test_python_surface_fails_loudly_off_the_gpu():
    import torch
    import link_amd as la
    from link_amd._lib import LinkAmdError
    from link_amd.index import GridTooLarge
    p = torch.zeros(8, 5)
    v = la.Voxelizer([0.075, 0.075, 0.2], [-6, -6, -5.0, 6, 6, 3.0], 10, 1000)
    for fn in (lambda: v.generate(p), lambda: v.generate_padded([p, p]), lambda: v.generate(p.numpy()),
               lambda: la.points_to_voxel(p, [0.075, 0.075, 0.2], [-6, -6, -5.0, 6, 6, 3.0]),
               lambda: la.DynamicVoxelEncoder([-6, -6, -5.0, 6, 6, 3.0], [0.075, 0.075, 0.2])([p])):
        with pytest.raises(LinkAmdError):
            fn()
    with pytest.raises(NotImplementedError):
        la.DynamicVoxelEncoder([-6, -6, -5.0, 6, 6, 3.0], [0.075, 0.075, 0.2], virtual=True)
    enc = la.DynamicVoxelEncoder([-54, -54, -5.0, 54, 54, 3.0], [0.075, 0.075, 0.2])
    assert enc.shape_np.tolist() == [1440, 1440, 40] and enc.shape_np.dtype == np.int32
    assert issubclass(GridTooLarge, LinkAmdError)
