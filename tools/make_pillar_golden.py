"""tools/make_pillar_golden.py -- record what the reference's own PillarFeatureNet and PointPillarsScatter compute, as
tests/golden/pillar_*.npz.  CPU only; needs a checkout of the reference; never called by a test.

    python tools/make_pillar_golden.py --reference /path/to/reference [--out tests/golden]

The reference's det3d package does not import on a machine without its compiled ops, so nothing of it is imported as a package:
pillar_encoder.py, models/utils/misc.py and models/utils/norm.py are loaded by file path into package shells (det3d, det3d.models,
det3d.models.readers, det3d.models.utils, det3d.models.registry with two do-nothing registries), with stubs for
det3d.utils.dist.dist_common and numba, which those files import and these classes never call.

Every case's inputs come from the builders of tests/pillar_oracle.py; weights, BatchNorm gamma, beta and running statistics are
randomised (the defaults would make a padded row leave a layer as exactly 0 and hide that it takes part in the max).  A file holds
arrays and settings only: the inputs, the state dict, the reader's rows and the canvas in float32 and in float64 (the same classes
run with .double()), and for the train-mode case the weight gradients of sum(canvas * g) and the updated running statistics.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pillar_oracle as PO  # noqa: E402

MAX_BYTES = 1 << 20

# name: (num_filters, D, T, with_distance, family, P, B, ny, nx, pattern, train)
CASES = {
    "l1": ((64,), 4, 20, False, "near", 9, 1, 7, 5, "mixed", False),
    "l2": ((64, 64), 5, 20, False, "far", 24, 2, 7, 5, "mixed", False),
    "l2_dist": ((64, 64), 5, 20, True, "near", 24, 2, 7, 5, "mixed", False),
    "l1_dist_t5": ((32,), 4, 5, True, "far", 12, 3, 7, 5, "mixed", False),
    "l2_t5": ((32, 128), 4, 5, False, "near", 16, 2, 7, 5, "mixed", False),
    "l2_p1": ((64, 64), 5, 20, False, "far", 1, 1, 7, 5, "ones", False),
    "l2_train": ((64, 64), 5, 20, False, "far", 24, 2, 7, 5, "mixed", True),
}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_classes(ref_root):
    det = os.path.join(ref_root, "detection", "det3d")

    def shell(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m

    for name in ("det3d", "det3d.models", "det3d.models.readers", "det3d.utils", "det3d.utils.dist"):
        shell(name)
    dist_common = types.ModuleType("det3d.utils.dist.dist_common")
    dist_common.get_world_size = lambda: 1
    sys.modules["det3d.utils.dist.dist_common"] = dist_common
    sys.modules["det3d.utils.dist"].dist_common = dist_common
    sys.modules.setdefault("numba", types.ModuleType("numba"))

    class _Registry:
        def register_module(self, cls):
            return cls

    registry = types.ModuleType("det3d.models.registry")
    registry.BACKBONES, registry.READERS = _Registry(), _Registry()
    sys.modules["det3d.models.registry"] = registry
    utils = shell("det3d.models.utils")
    misc = _load("det3d.models.utils.misc", os.path.join(det, "models", "utils", "misc.py"))
    norm = _load("det3d.models.utils.norm", os.path.join(det, "models", "utils", "norm.py"))
    utils.get_paddings_indicator = misc.get_paddings_indicator
    utils.build_norm_layer = norm.build_norm_layer
    enc = _load("det3d.models.readers.pillar_encoder", os.path.join(det, "models", "readers", "pillar_encoder.py"))
    return enc.PillarFeatureNet, enc.PointPillarsScatter


def record(name, spec, PillarFeatureNet, PointPillarsScatter, out_dir):
    filters, D, T, dist, family, P, B, ny, nx, pattern, train = spec
    seed = sorted(CASES).index(name)
    cfg = PO.make_cfg(filters, D, T, dist, family)
    feats, num, coors = PO.make_case(P, cfg, B, ny, nx, pattern, seed)
    sd = PO.make_state(cfg, D, seed)
    arrays = {"features": feats.numpy(), "num": num.numpy(), "coors": coors.numpy(), "B": np.int64(B), "ny": np.int64(ny), "nx": np.int64(nx),
              "train": np.bool_(train), "cfg_num_filters": np.asarray(filters, dtype=np.int64), "cfg_with_distance": np.bool_(dist),
              "cfg_voxel_size": np.asarray(cfg["voxel_size"], dtype=np.float64), "cfg_pc_range": np.asarray(cfg["pc_range"], dtype=np.float64)}
    arrays.update({"sd." + k: v.numpy() for k, v in sd.items()})
    g = torch.randn(B, filters[-1], ny, nx, generator=torch.Generator().manual_seed(77 + seed))
    if train:
        arrays["g"] = g.numpy()
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        net = PillarFeatureNet(num_input_features=D, num_filters=filters, with_distance=dist, voxel_size=cfg["voxel_size"],
                               pc_range=cfg["pc_range"])
        net.load_state_dict(sd, strict=True)
        net = net.to(dt)
        scat = PointPillarsScatter(num_input_features=filters[-1])
        net.train(train)
        # the reference multiplies its input by the mask in place: hand it a copy
        rows = net(feats.to(dt).clone(), num.clone(), coors.clone())
        arrays["rows_squeezed_shape"] = np.asarray(rows.shape, dtype=np.int64)
        rows = rows.reshape(P, filters[-1])
        canvas = scat(rows, coors, B, (nx, ny, 1))
        arrays["rows" + tag], arrays["canvas" + tag] = rows.detach().numpy(), canvas.detach().numpy()
        if train:
            (canvas * g.to(dt)).sum().backward()
            for k, v in net.named_parameters():
                arrays[f"grad{tag}." + k] = v.grad.numpy()
            for k, v in net.state_dict().items():
                if "running" in k or "num_batches" in k:
                    arrays[f"new{tag}." + k] = v.numpy()
    path = os.path.join(out_dir, f"pillar_{name}.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (path, size)
    print(f"{path}: {size} bytes, rows {tuple(arrays['rows32'].shape)}, canvas {tuple(arrays['canvas32'].shape)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds detection/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    classes = reference_classes(a.reference)
    os.makedirs(a.out, exist_ok=True)
    for name in sorted(CASES):
        record(name, CASES[name], *classes, a.out)


if __name__ == "__main__":
    main()
