"""Record tests/golden/segio_*.npz from the reference's own code.

    python tests/golden/make_golden_segio.py /path/to/LinK

The expected values come from the reference's segmentation/torchsparse-u/torchsparse/utils/quantize.py (sparse_quantize; it needs only
numpy) and segmentation/core/callbacks.py (MeanIoU), both loaded BY PATH; callbacks.py imports torchpack, so stand-in modules named
`torchpack`, `torchpack.distributed` (allreduce returns its argument: one process) and `torchpack.callbacks.callback` (an empty
Callback) are registered first.  The steps of segmentation/evaluate.py:125-133 around them -- per test-time-augmentation pass the
rows of that pass, indexed by the pass's inverse map, the passes stacked, summed, arg-maxed -- are composed here from torch ops on the
CPU, and so are the two lines of core/datasets/semantic_kitti.py:219-220 in front of sparse_quantize.  The inputs are the seeded cases
of tests/segio_oracle.py.  Nothing of the reference is copied into the repository."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import segio_oracle as SO  # noqa: E402


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference(root):
    seg = os.path.join(root, "segmentation")
    quant = by_path("ref_quantize", os.path.join(seg, "torchsparse-u", "torchsparse", "utils", "quantize.py"))
    tp, dist, cbs, cb = (types.ModuleType(n) for n in ("torchpack", "torchpack.distributed", "torchpack.callbacks", "torchpack.callbacks.callback"))
    dist.allreduce = lambda x, reduction="sum": x
    cb.Callback = type("Callback", (), {})
    tp.distributed, tp.callbacks, cbs.callback = dist, cbs, cb
    sys.modules.update({"torchpack": tp, "torchpack.distributed": dist, "torchpack.callbacks": cbs, "torchpack.callbacks.callback": cb})
    calls = by_path("ref_callbacks", os.path.join(seg, "core", "callbacks.py"))
    return quant, calls


def save(name, meta, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    assert os.path.getsize(path) < (1 << 20), name
    print(name, os.path.getsize(path))


def record_quantize(quant):
    # integer coordinates, the minimum not at zero: sparse_quantize itself
    pc = SO.make_cloud(6000, 11, offset=(-37, 12, -5))
    assert SO.duplicate_share(pc) >= 0.3 and pc.min() < 0
    coords, inds, inv = quant.sparse_quantize(pc.copy(), return_index=True, return_inverse=True)
    assert inds.dtype == np.int64 and inv.dtype == np.int64 and coords.dtype == np.int32
    save("segio_quantize_int.npz", {"seed": 11}, points=pc, coords=coords, indices=inds, inverse=inv)
    # a float block through semantic_kitti.py:219-225
    vs = 0.05
    block = SO.make_block(5000, 12, vs)
    pc_ = np.round(block[:, :3] / vs).astype(np.int32)
    pc_ -= pc_.min(0, keepdims=1)
    coords, inds, inv = quant.sparse_quantize(pc_, return_index=True, return_inverse=True)
    save("segio_quantize_block.npz", {"seed": 12, "voxel_size": vs}, block=block, pc=pc_, coords=coords, indices=inds, inverse=inv)
    # floating coordinates and a voxel size: the float64 divide and floor inside sparse_quantize
    pf = np.random.default_rng(13).normal(0.0, 3.0, (4000, 3))
    coords, inds, inv = quant.sparse_quantize(pf.copy(), 0.25, return_index=True, return_inverse=True)
    save("segio_quantize_float.npz", {"seed": 13, "voxel_size": 0.25}, points=pf, coords=coords, indices=inds, inverse=inv)


def vote_by_torch(rows, row_batch, inv_local, inv_batch):
    """evaluate.py:125-133 on CPU tensors: rows [n_rows, c] of all passes, row_batch the pass of every row, inv_local [V * P] the
    inverse map of every pass (indices inside the pass), inv_batch its pass"""
    outs = []
    for idx in range(int(inv_batch.max()) + 1):
        cur_scene_pts = (row_batch == idx).numpy()
        cur_inv = inv_local[inv_batch == idx].numpy()
        outs.append(rows[cur_scene_pts][cur_inv])
    return torch.stack(outs, dim=0).sum(dim=0).argmax(1)


def record_eval(calls):
    c, ignore, p, votes = 19, 0, 3000, 3
    steps = []
    arrays = {}
    with tempfile.TemporaryDirectory() as run_dir:
        miou = calls.MeanIoU(c, ignore, run_dir=run_dir)
        miou._before_epoch()
        for step in range(2):
            rng = np.random.default_rng(20 + step)
            sizes = [1500 + 37 * v + step for v in range(votes)]
            rows = torch.from_numpy(rng.standard_normal((sum(sizes), c)).astype(np.float32))
            row_batch = torch.cat([torch.full((m,), v, dtype=torch.int32) for v, m in enumerate(sizes)])
            inv_local = torch.cat([torch.from_numpy(rng.integers(0, m, p)) for m in sizes])
            inv_batch = torch.arange(votes, dtype=torch.int32).repeat_interleave(p)
            labels = torch.from_numpy(rng.integers(0, c - 2, p))             # class 17 is never seen, 18 neither
            labels[torch.from_numpy(rng.random(p) < 0.1)] = 0
            pred = vote_by_torch(rows, row_batch, inv_local, inv_batch)
            miou._after_step({"outputs": pred, "targets": labels})
            arrays.update({f"rows{step}": rows.numpy(), f"row_batch{step}": row_batch.numpy(), f"inv_local{step}": inv_local.numpy(),
                           f"labels{step}": labels.numpy(), f"pred{step}": pred.numpy()})
            steps.append(sizes)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            miou._after_epoch()
        printed = out.getvalue().strip().splitlines()
    assert len(printed) == 3 and printed[0].startswith("mIoU: ")
    arrays.update(total_seen=miou.total_seen, total_correct=miou.total_correct, total_positive=miou.total_positive)
    save("segio_eval.npz", {"num_classes": c, "ignore_label": ignore, "votes": votes, "points": p, "sizes": steps, "printed": printed}, **arrays)
    # exact ties: integer-valued rows; torch's CPU argmax must have taken the lowest index, or the fixture records nothing usable
    rows, inverse, labels = SO.make_eval_case(777, 5, 2, 31, integer_ties=True)
    inverse = np.clip(inverse, 0, rows.shape[0] - 1)
    t = torch.from_numpy(rows)
    summed = torch.stack([t[torch.from_numpy(inverse[v]).long()] for v in range(2)], 0).sum(0)
    pred = summed.argmax(1)
    ties = (summed == summed.max(1, keepdim=True).values).sum(1) > 1
    lowest = torch.where(summed == summed.max(1, keepdim=True).values, torch.arange(5)[None, :], torch.tensor(5)).min(1).values
    assert int(ties.sum()) > 100 and torch.equal(pred, lowest), "torch's CPU argmax did not take the lowest index on exact ties"
    save("segio_ties.npz", {"seed": 31, "ties": int(ties.sum())}, rows=rows, inverse=inverse, labels=labels, pred=pred.numpy())


if __name__ == "__main__":
    quant, calls = load_reference(sys.argv[1])
    record_quantize(quant)
    record_eval(calls)
