"""Shared helpers for the test-suite (fixture loading, seeded generators, error metrics)."""
import contextlib
import glob
import json
import os

import functools

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    d = {k: z[k] for k in z.files if k != "meta"}
    d["meta"] = json.loads(str(z["meta"]))
    return d


def golden_files(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, pattern)))


def rel_err(a, b):
    """max |a-b| / max(|b|) -- the 'within 1e-4 rel on fp32 features' metric of BASELINE.json."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    denom = max(float(np.abs(b).max()), 1e-30)
    return float(np.abs(a - b).max() / denom)


@functools.lru_cache(maxsize=12)
def _s_uniform_perm(grid, seed):
    """The generator's permutation of the grid's cells (what costs the time: 16.7 M cells for grid 256); cached per (grid, seed) --
    many tests draw the same seeds."""
    import torch
    return torch.randperm(grid ** 3, generator=torch.Generator().manual_seed(seed))


def s_uniform(n, grid=256, seed=0, batch=0):
    """SURVEY.md section 8d S-uniform generator (unique voxels, uniform in grid^3)."""
    import torch
    lin = _s_uniform_perm(grid, seed)[:n]
    x, y, z = lin % grid, (lin // grid) % grid, lin // (grid * grid)
    return torch.stack([x, y, z, torch.full_like(x, batch)], 1).int()


def lidar_like(n_target=60000, seed=0, voxel=0.05, stride=1):
    """Cheap LiDAR-shaped frame: ground plane + a few boxes, ring pattern; unique int32 voxels."""
    rng = np.random.default_rng(seed)
    n_az, n_el = 2048, 64
    az = rng.uniform(0, 2 * np.pi, n_az)
    el = np.deg2rad(np.linspace(-24.8, 2.0, n_el))
    A, E = np.meshgrid(az, el)
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    h = 1.73
    t = np.where(d[:, 2] < -1e-3, -h / np.minimum(d[:, 2], -1e-3), 50.0)
    t = np.minimum(t, 50.0)
    # a few walls
    for _ in range(12):
        c = rng.uniform(-35, 35, 2); w = rng.uniform(2, 8)
        for ax in (0, 1):
            tt = (c[ax] - 0) / np.where(np.abs(d[:, ax]) > 1e-6, d[:, ax], 1e-6)
            p = d * tt[:, None]
            ok = (tt > 1) & (np.abs(p[:, 1 - ax] - c[1 - ax]) < w) & (p[:, 2] + h < 3.5) & (p[:, 2] + h > 0)
            t = np.where(ok & (tt < t), tt, t)
    pts = d * t[:, None] + np.array([0, 0, h]) + rng.normal(0, 0.01, (d.shape[0], 3))
    pc = np.round(pts / voxel).astype(np.int64)
    pc -= pc.min(0)
    pc = (pc // stride) * stride
    pc = np.unique(pc, axis=0)
    rng.shuffle(pc)
    pc = pc[:n_target]
    out = np.zeros((pc.shape[0], 4), np.int32)
    out[:, :3] = pc
    return out


def ref_ops_cases():
    """The seeded inputs of the check of the oracle against the reference's compiled CPU ops (tests/test_oracle_golden.py):
    op name -> (the reference op's arguments as numpy arrays / ints, a callable returning the oracle's answer).  Shared with
    tests/golden/make_golden_ref_ops.py, which records the digests of the reference ops' outputs on these inputs."""
    from oracle import link_oracle as O
    rng = np.random.default_rng(0)
    coords = rng.integers(-500, 500, (5000, 4)).astype(np.int32)
    coords[:, 3] = 0
    off = O.get_kernel_offsets(3)
    idx = rng.integers(-1, 300, 5000).astype(np.int32)
    idxp = np.abs(idx)
    counts = O.spcount(idxp, 300)
    feats = rng.standard_normal((5000, 24)).astype(np.float32)
    top = rng.standard_normal((300, 24)).astype(np.float32)
    ind = rng.integers(-1, 300, (700, 8)).astype(np.int32)
    w = rng.random((700, 8)).astype(np.float32)
    return {"hash_cpu": ((coords,), lambda: O.sphash(coords)),
            "kernel_hash_cpu": ((coords, off), lambda: O.sphash_offsets(coords, off)),
            "count_cpu": ((idx, 300), lambda: O.spcount(idx, 300)),
            "voxelize_forward_cpu": ((feats, idxp, counts), lambda: O.spvoxelize_fwd(feats, idxp, counts)),
            "voxelize_backward_cpu": ((top, idxp, counts, 5000), lambda: O.spvoxelize_bwd(top, idxp, counts, 5000)),
            "devoxelize_forward_cpu": ((top, ind, w), lambda: O.spdevoxelize_fwd(top, ind, w))}


def array_digest(a):
    """sha256 of an op output's values (integers as int64, floats as float32: value equality, as np.array_equal checks it)."""
    import hashlib
    a = np.asarray(a)
    a = a.astype(np.int64 if np.issubdtype(a.dtype, np.integer) else np.float32)
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}


class _Spy:
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("link_"):
            return fn

        def call(*a):
            self._calls.append(name)
            return fn(*a)
        return call


@contextlib.contextmanager
def spied():
    """the names of the library entry points called inside the block"""
    from link_amd import _lib as L
    real, calls = L.lib, []
    spy = _Spy(real(), calls)
    L.lib = lambda: spy
    try:
        yield calls
    finally:
        L.lib = real
