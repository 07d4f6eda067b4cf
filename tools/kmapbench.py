"""tools/kmapbench.py -- kernel-map build time of the general builder (csrc/kmap.hip) against the torch / hash-chain
composition it replaces, on the full-size S-kitti frame and its stride-2 stage.   python tools/kmapbench.py [--reps 30]

Per frame and geometry (k3 s2; (3,1,3) s1) the WHOLE map build -- output coordinates + table, bounds pass included, fresh
caches every repetition -- timed with device events after a warm-up, alternating the two builders in one process; median
and quartiles in us, and the launches each build enqueues (torch profiler, kernels + memsets + copies).  The two builders'
maps are compared bit for bit before anything is timed.  One JSON line per (frame, geometry).

What the two figures are: event to event on one stream, so host time counts wherever the host is the slower side.  The
builder waits for the host once per build (the bounds round trip; on strided geometries also the site count) and the k3 s2
composition waits in torch.unique / the boolean mask; the STRIDE-1 composition never waits, so its events sit back to back
and its figure is device time alone while the builder's is host-bound: that comparison leans against the builder.  The
layer object and the feature rows are made once, outside the timed region; a repetition makes only the SparseTensor (fresh
cmaps / kmaps: nothing cached carries over)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import link_amd as la  # noqa: E402
import link_amd.elk as E  # noqa: E402
from link_amd import synth  # noqa: E402


def composition(coords, ks, st, ts):
    """The map as the functional surface could compose it before the builder: Python spdownsample + the hash chain."""
    out_c = E._spdownsample_torch(coords, st, ks, ts) if any(s > 1 for s in st) else coords
    offs = la.get_kernel_offsets(ks, stride=ts, device=coords.device)
    return out_c, la.sphashquery(la.sphash(out_c, offs), la.sphash(coords)).t().contiguous().int()


def builder(conv, feats, coords, ts):
    x = la.SparseTensor(feats, coords, ts)               # fresh cmaps / kmaps
    table, _, _, _, out_c, _ = conv._route(x, need_back=False)
    return out_c, table


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(1e3 * a.elapsed_time(b) for a, b in ev)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(); torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    c1 = torch.from_numpy(synth.s_kitti()[0]).cuda()
    c2 = E.spdownsample(c1, 2, 2, 1)
    for frame, coords, ts in (("s_kitti", c1, (1, 1, 1)), ("s_kitti_stride2", c2, (2, 2, 2))):
        for ks, st in (((3, 3, 3), (2, 2, 2)), ((3, 1, 3), (1, 1, 1))):
            conv, feats = la.Conv3d(1, 1, ks, st), torch.zeros((coords.shape[0], 1), device=coords.device)
            fa, fb = (lambda: builder(conv, feats, coords, ts)), (lambda: composition(coords, ks, st, ts))
            a, b = fa(), fb()
            same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
            for _ in range(args.warmup):
                fa(); fb()
            ta, tb = [], []
            for _ in range(3):                          # alternate the two in blocks: drift hits both alike
                ta += timed(fa, args.reps // 3 + 1); tb += timed(fb, args.reps // 3 + 1)
            ta.sort(); tb.sort()
            q = lambda t: {"median_us": round(t[len(t) // 2], 1), "q1_us": round(t[len(t) // 4], 1), "q3_us": round(t[3 * len(t) // 4], 1)}
            rec = {"frame": frame, "voxels": int(coords.shape[0]), "kernel": ks, "stride": st, "sites": int(a[0].shape[0]),
                   "maps_equal": same, "builder": q(ta), "composition": q(tb), "reps": len(ta)}
            try:
                rec["builder"]["launches"], rec["composition"]["launches"] = launches(fa), launches(fb)
            except Exception as e:                       # the profiler is a convenience here, the times are the result
                rec["launches_error"] = repr(e)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
