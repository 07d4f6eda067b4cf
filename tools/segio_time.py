"""tools/segio_time.py -- the segmentation front end and validation on the device against the numpy host path, on S-kitti frames.

    python tools/segio_time.py [--frames 2] [--reps 20] [--out FILE.json]

Times (device: 7 windows of `reps` calls each after 10 warm-up calls, [min, median, max] per call; host: a wall clock, per call):
  quantise     SegVoxelizer.generate_padded (no read-back) and SegVoxelizer.__call__ (one read-back, the four SparseTensors)
               against two host paths: tests/segio_oracle.py (np.round, the minimum, np.unique(axis=0): a row sort) and a 1-D
               hashed np.unique (the shape of the reference's own path, several times cheaper than the row sort)
  vote + eval  SegEvaluator.update on [voxels, 19] fp32 logits with the frame's inverse map, one pass and three,
               against the oracle's float64 vote and its counting loop
and counts the read-backs (Tensor.item / tolist / cpu / numpy) of one voxeliser call, one update and one compute.  No GPU: fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segio_oracle as SO  # noqa: E402

import link_amd as la  # noqa: E402
from link_amd import synth  # noqa: E402


def device_ms(fn, reps, windows=7):
    """per call: [min, median, max] over `windows` timed windows of `reps` calls each, after 10 warm-up calls"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / reps)
    per.sort()
    return [per[0], per[len(per) // 2], per[-1]]


def hashed_unique(block, vs):
    """the cheaper host path, the shape of what the reference runs per frame: round, minimum, a mixed-radix hash of the three
    coordinates into one uint64, a 1-D np.unique with return_index and return_inverse"""
    q = np.round(block[:, :3] / np.float32(vs)).astype(np.int64)
    q -= q.min(0)
    radix = q.max(0) + 1
    key = ((q[:, 0] * radix[1] + q[:, 1]) * radix[2] + q[:, 2]).astype(np.uint64)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    return q[first], first, inverse


def host_ms(fn, reps=3):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


class ReadBacks:
    """counts the calls that bring a device tensor's values to the host"""

    def __enter__(self):
        self.n = 0
        self._saved = {k: getattr(torch.Tensor, k) for k in ("item", "tolist", "cpu", "numpy")}
        for k, f in self._saved.items():
            def wrap(t, *a, _f=f, **kw):
                self.n += 1 if t.is_cuda else 0
                return _f(t, *a, **kw)
            setattr(torch.Tensor, k, wrap)
        return self

    def __exit__(self, *exc):
        for k, f in self._saved.items():
            setattr(torch.Tensor, k, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segio_time: no GPU visible; a CPU run gives no time")
    vs, c = 0.05, 19
    out = {"device": torch.cuda.get_device_name(0), "voxel_size": vs, "classes": c, "reps": args.reps, "frames": []}
    for seed in range(args.frames):
        _, _, pts = synth.s_kitti(seed=seed, return_points=True)
        rng = np.random.default_rng(seed)
        block = np.concatenate([pts[:, :3], rng.uniform(0, 1, (pts.shape[0], 1))], 1).astype(np.float32)
        labels = rng.integers(0, c, block.shape[0]).astype(np.int64)
        labels[rng.random(block.shape[0]) < 0.05] = 255
        want = SO.quantize([block], voxel_size=vs)
        bd, yd = torch.from_numpy(block).cuda(), torch.from_numpy(labels).cuda()
        vox = la.SegVoxelizer(vs)
        got = vox.generate_padded([bd])
        assert all(np.array_equal(t.cpu().numpy(), want[k]) for k, t in zip(("coords", "indices", "inverse"), got)), "quantiser disagrees with the oracle"
        hq, hfirst, hinv = hashed_unique(block, vs)
        assert np.array_equal(hq, want["coords"][:want["total"], :3]) and np.array_equal(hfirst, want["indices"][:want["total"]]) and \
            np.array_equal(hinv, want["inverse"]), "the hashed host path disagrees with the oracle"
        m = want["total"]
        rows = rng.standard_normal((m, c)).astype(np.float32)
        rd = torch.from_numpy(rows).cuda()
        inv1 = got[2][None].contiguous()
        inv3 = torch.stack([got[2], got[2].roll(1), got[2].roll(2)]).contiguous()
        ev = la.SegEvaluator(c, 0)
        pred = ev.update(rd, yd, inv1)
        cls, gap = SO.vote(rows, inv1.cpu().numpy())
        sure = gap >= 1e-4
        assert np.array_equal(pred.cpu().numpy()[sure], cls[sure]), "vote disagrees with the oracle"
        with ReadBacks() as rb_vox:
            vox([bd], [yd])
        with ReadBacks() as rb_upd:
            ev.update(rd, yd, inv1)
        with ReadBacks() as rb_cmp:
            ev.compute()
        frame = {"seed": seed, "points": int(block.shape[0]), "voxels": int(m), "key_bits": int(got[5][2]),
                 "quantize_padded_ms": device_ms(lambda: vox.generate_padded([bd]), args.reps),
                 "quantize_call_ms": device_ms(lambda: vox([bd], [yd]), args.reps),
                 "quantize_host_oracle_ms": host_ms(lambda: SO.quantize([block], voxel_size=vs)),
                 "quantize_host_hashed_ms": host_ms(lambda: hashed_unique(block, vs)),
                 "vote_eval_v1_ms": device_ms(lambda: ev.update(rd, yd, inv1), args.reps),
                 "vote_eval_v3_ms": device_ms(lambda: ev.update(rd, yd, inv3), args.reps),
                 "vote_eval_host_v1_ms": host_ms(lambda: SO.count(SO.vote(rows, inv1.cpu().numpy())[0], labels, c, 0), 1),
                 "launches": {"link_seg_quantize": 33, "link_seg_vote_eval": 1},
                 "read_backs": {"voxelizer_call": rb_vox.n, "update": rb_upd.n, "compute": rb_cmp.n}}
        out["frames"].append(frame)
        print(json.dumps(frame))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
