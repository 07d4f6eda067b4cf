"""tests/golden/make_golden_voxelize.py -- records the fixtures of tests/test_cpu_voxelize.py and tests/test_gpu_voxelize.py
(tests/golden/voxelize_*.npz).  The tests do not run it.

The expected outputs come from the reference's own code, run from where the reference checkout lies (argument 1 or $LINK_REFERENCE):
detection/det3d/ops/point_cloud/point_cloud_ops.py::points_to_voxel, loaded by path with a stand-in `numba` module whose `jit` returns
the function unchanged (the loop then runs as plain Python on numpy float32 scalars), and detection/det3d/models/readers/
dynamic_voxel_encoder.py::DynamicVoxelEncoder, loaded by path with det3d.core.utils.scatter taken from the reference file and a stand-in
for ..registry.  The stand-ins exist only in sys.modules; nothing of the reference is copied here.

Geometry: the config's voxel size (0.075, 0.075, 0.2); a 160 x 160 x 40 grid (range -6, -6, -5 .. 6, 6, 3) unless the case says
otherwise, max_points 10.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VS = [0.075, 0.075, 0.2]
SMALL = [-6.0, -6.0, -5.0, 6.0, 6.0, 3.0]
FULL = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
F32 = np.float32


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    det3d = os.path.join(ref_root, "detection", "det3d")
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.modules["numba"] = numba
    ops = _load("ref_point_cloud_ops", os.path.join(det3d, "ops", "point_cloud", "point_cloud_ops.py"))
    for pkg in ("det3d", "det3d.core", "det3d.core.utils", "det3d.models", "det3d.models.readers"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    _load("det3d.core.utils.scatter", os.path.join(det3d, "core", "utils", "scatter.py"))
    reg = types.ModuleType("det3d.models.registry")
    reg.READERS = types.SimpleNamespace(register_module=lambda cls: cls)
    sys.modules["det3d.models.registry"] = reg
    dyn = _load("det3d.models.readers.dynamic_voxel_encoder", os.path.join(det3d, "models", "readers", "dynamic_voxel_encoder.py"))
    return ops.points_to_voxel, dyn.DynamicVoxelEncoder


def cloud(rng, n, box, ndim=5, spill=0.05):
    """n points uniform in the range grown by `spill` of its extent on every side (so some fall outside), extra columns U[0, 1)"""
    lo, hi = np.array(box[:3]), np.array(box[3:])
    ext = hi - lo
    p = rng.uniform(lo - spill * ext, hi + spill * ext, (n, 3))
    return np.concatenate([p, rng.uniform(0, 1, (n, ndim - 3))], 1).astype(F32)


def clustered(rng, n, cells, box, ndim=5):
    """n points drawn around `cells` random centres, 3 cm spread: many points per voxel, neighbours filled too"""
    lo, hi = np.array(box[:3]), np.array(box[3:])
    c = rng.uniform(lo, hi, (cells, 3))
    p = c[rng.integers(0, cells, n)] + rng.normal(0, 0.03, (n, 3))
    return np.concatenate([p, rng.uniform(0, 1, (n, ndim - 3))], 1).astype(F32)


def edge_points(box, ndim):
    """points exactly on lo and on hi of each axis and one ulp inside / outside of both, the other axes mid-range"""
    lo, hi = np.array(box[:3], F32), np.array(box[3:], F32)
    mid = ((lo + hi) / 2).astype(F32)
    rows = []
    for d in range(3):
        for v in (lo[d], hi[d]):
            for w in (v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))):
                r = mid.copy()
                r[d] = w
                rows.append(r)
    for corner in range(8):                                           # and the corners of the range themselves
        rows.append(np.array([hi[d] if corner >> d & 1 else lo[d] for d in range(3)], F32))
    p = np.stack(rows)
    return np.concatenate([p, np.linspace(0, 1, p.shape[0] * (ndim - 3), dtype=F32).reshape(p.shape[0], ndim - 3)], 1)


def corner_cloud(rng, n, box, ndim=5):
    """n points on the full grid that include the centres of the eight corner voxels"""
    lo, hi, vs = np.array(box[:3]), np.array(box[3:]), np.array(VS)
    p = cloud(rng, n, box, ndim)
    for corner in range(8):
        p[corner * 37, :3] = [(hi[d] - vs[d] / 2) if corner >> d & 1 else (lo[d] + vs[d] / 2) for d in range(3)]
    return p


def save(name, meta, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(f"{name}: {size} bytes", {k: tuple(v.shape) for k, v in arrays.items() if k != 'meta'})


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["LINK_REFERENCE"]
    points_to_voxel, DynamicVoxelEncoder = load_reference(ref_root)
    import torch
    rng = np.random.default_rng(2024)
    one = np.concatenate([rng.uniform([0.01, 0.01, 0.01], [0.07, 0.07, 0.19], (100, 3)), rng.uniform(0, 1, (100, 2))], 1).astype(F32)

    hard_cases = {f"n{n}": dict(clouds=[cloud(rng, n, SMALL)]) for n in (0, 1, 63, 64, 65, 4097)}
    far = cloud(rng, 200, SMALL)
    far[:, 0] += 40.0
    hard_cases["allout"] = dict(clouds=[far])
    hard_cases["onevoxel"] = dict(clouds=[one])
    hard_cases["clustered"] = dict(clouds=[clustered(rng, 6000, 150, SMALL)])
    hard_cases["capped"] = dict(clouds=[clustered(rng, 20000, 1500, SMALL)], max_voxels=3000)
    hard_cases["edges"] = dict(clouds=[edge_points(SMALL, 4)])
    hard_cases["ndim4"] = dict(clouds=[cloud(rng, 1000, SMALL, 4)])
    hard_cases["ndim6"] = dict(clouds=[cloud(rng, 1000, SMALL, 6)])
    hard_cases["noreverse"] = dict(clouds=[cloud(rng, 1000, SMALL)], reverse=False)
    hard_cases["batch3"] = dict(clouds=[cloud(rng, 500, SMALL), cloud(rng, 0, SMALL), clustered(rng, 1300, 40, SMALL)], max_voxels=400)
    hard_cases["full"] = dict(clouds=[corner_cloud(rng, 4096, FULL)], box=FULL)
    for name, case in hard_cases.items():
        box, mp, mv, rev = case.get("box", SMALL), 10, case.get("max_voxels", 20000), case.get("reverse", True)
        vs, rg = np.array(VS, F32), np.array(box, F32)
        arrays = {}
        for k, p in enumerate(case["clouds"]):
            v, c, n = points_to_voxel(p, vs, rg, mp, rev, mv)
            arrays.update({f"points{k}": p, f"voxels{k}": v, f"coors{k}": c, f"num{k}": n})
        shape = np.round((rg[3:] - rg[:3]) / vs).astype(np.int64)
        occupied = [int(a.shape[0]) for k, a in arrays.items() if k.startswith("coors")]
        save(f"voxelize_hard_{name}.npz", {"mode": "hard", "clouds": len(case["clouds"]), "max_points": mp, "max_voxels": mv,
                                           "reverse_index": rev, "voxels": occupied,
                                           "source": "point_cloud_ops.py::points_to_voxel, numba.jit replaced by the identity"},
             voxel_size=vs, range=rg, shape=shape, **arrays)

    dyn_cases = {f"n{n}": dict(clouds=[cloud(rng, n, SMALL)]) for n in (0, 1, 63, 64, 65, 4097)}
    dyn_cases["allout"] = dict(clouds=[far])
    dyn_cases["onevoxel"] = dict(clouds=[one])
    dyn_cases["clustered"] = dict(clouds=[clustered(rng, 6000, 150, SMALL)])
    dyn_cases["edges"] = dict(clouds=[edge_points(SMALL, 4)])
    dyn_cases["ndim4"] = dict(clouds=[cloud(rng, 1000, SMALL, 4)])
    dyn_cases["ndim6"] = dict(clouds=[cloud(rng, 1000, SMALL, 6)])
    dyn_cases["batch3"] = dict(clouds=[cloud(rng, 500, SMALL), cloud(rng, 0, SMALL), clustered(rng, 1300, 40, SMALL)])
    dyn_cases["full"] = dict(clouds=[corner_cloud(rng, 4096, FULL)], box=FULL)
    for name, case in dyn_cases.items():
        box = case.get("box", SMALL)
        enc = DynamicVoxelEncoder(box, VS)
        voxels, coors, shape = enc([torch.from_numpy(p) for p in case["clouds"]])
        assert coors.dtype == torch.int64
        arrays = {f"points{k}": p for k, p in enumerate(case["clouds"])}
        save(f"voxelize_dyn_{name}.npz", {"mode": "dynamic", "clouds": len(case["clouds"]), "voxels": [int(voxels.shape[0])],
                                          "source": "dynamic_voxel_encoder.py::DynamicVoxelEncoder.forward on CPU tensors"},
             voxel_size=np.array(VS, F32), range=np.array(box, F32), shape=np.asarray(shape).astype(np.int64), voxels=voxels.numpy(),
             coors=coors.numpy(), **arrays)


if __name__ == "__main__":
    main()
