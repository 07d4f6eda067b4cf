"""tools/detaugbench.py -- time of the detection training front end on the device at the nuScenes shape: B = 4 frames of
about 250 000 points x 5 features, about 40 ground-truth boxes each, the config's ten sample groups, a synthetic database.

Timed: DetTrainAugmenter.padded (device events around a window of calls, 7 windows, median and the spread min .. max) against the
same steps on this machine's host: tests/aug_oracle.py's float32 numpy restatement of the reference's Preprocess (the sampler's
scan, the paste, the four global transforms, the shuffle, the range filter), frame by frame.  The reference proper runs the
collision test and the point-in-box loops under numba, which is not installed here; the numpy restatement is vectorised but is NOT the
reference, so the host figure stands for "the same work in numpy on this host" and nothing else.  Also printed: launches and host round
trips per call, counted from what the code does (padded: points-in-boxes count only with min_points_in_gt > 0, scan, points, boxes;
no read-back).  Needs a GPU; prints one JSON line."""
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
import aug_oracle as AO  # noqa: E402
import link_amd as la  # noqa: E402

CLASS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
SAMPLE_GROUPS = [dict(car=2), dict(truck=3), dict(construction_vehicle=7), dict(bus=4), dict(trailer=6), dict(barrier=2), dict(motorcycle=6),
                 dict(bicycle=6), dict(pedestrian=2), dict(traffic_cone=2)]
SIZES = [(4.6, 1.9, 1.7), (6.9, 2.5, 2.8), (6.4, 2.8, 3.2), (11.0, 2.9, 3.5), (12.3, 2.9, 3.9), (0.5, 2.5, 1.0), (2.1, 0.8, 1.5), (1.7, 0.6, 1.3),
         (0.7, 0.7, 1.8), (0.4, 0.4, 1.1)]
PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
ROT, SCALE, STD = [-0.78539816, 0.78539816], [0.9, 1.1], 0.5


def boxes_of(rng, classes):
    b = np.zeros((len(classes), 9), np.float32)
    b[:, 0:2], b[:, 2] = rng.uniform(-50, 50, (len(classes), 2)), rng.uniform(-1.5, 0.0, len(classes))
    b[:, 3:6] = np.array(SIZES, np.float32)[classes - 1] * rng.uniform(0.85, 1.15, (len(classes), 3))
    b[:, 6:8], b[:, 8] = rng.normal(0, 2.0, (len(classes), 2)), rng.uniform(-np.pi, np.pi, len(classes))
    return b


def database(rng, per_class, ndim):
    classes = np.repeat(np.arange(1, 11), per_class).astype(np.int32)
    boxes = boxes_of(rng, classes)
    counts = rng.integers(20, 400, len(classes))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = rng.uniform(-0.5, 0.5, (offs[-1], ndim)).astype(np.float32)
    pts[:, :3] *= np.repeat(boxes[:, 3:6], counts, 0)
    return dict(points=pts, offsets=offs, boxes=boxes, classes=classes)


def scene(rng, n_points, n_gt, ndim):
    classes = rng.integers(1, 11, n_gt).astype(np.int32)
    pts = rng.uniform([-54, -54, -5, 0, 0][:ndim], [54, 54, 3, 1, 1][:ndim], (n_points, ndim)).astype(np.float32)
    return pts, boxes_of(rng, classes), classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=250000)
    ap.add_argument("--gt", type=int, default=40)
    ap.add_argument("--per-class", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=500, help="calls per timed window")
    ap.add_argument("--min-points", type=int, default=-1, help="min_points_in_gt (the nuScenes config leaves it at -1)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detaugbench: needs a GPU (a time taken elsewhere says nothing)")
    rng = np.random.default_rng(0)
    ndim, cap = 5, a.points + 7 * 10 * 400
    db_np = database(rng, a.per_class, ndim)
    frames = [scene(rng, a.points, a.gt, ndim) for _ in range(a.batch)]
    db = la.GTDatabase(db_np["points"], db_np["offsets"], db_np["boxes"], db_np["classes"])
    aug = la.DetTrainAugmenter(CLASS_NAMES, SAMPLE_GROUPS, 1.0, ROT, SCALE, STD, a.min_points, PC_RANGE, 500, cap, database=db)
    sampler = la.DatabaseSampler(db.by_class, np.random.RandomState(0))
    cand, lens = sampler.candidates(a.batch, aug.group_classes, aug.group_max, aug.max_candidates)
    draws = np.concatenate([rng.random((a.batch, 4)), rng.standard_normal((a.batch, 3))], 1).astype(np.float32)
    perm = np.stack([rng.permutation(cap) for _ in range(a.batch)]).astype(np.int32)
    dev = "cuda"
    args = dict(points=torch.from_numpy(np.concatenate([f[0] for f in frames])).to(dev),
                point_offsets=torch.tensor(np.arange(a.batch + 1) * a.points, dtype=torch.int32).to(dev),
                gt_boxes=torch.from_numpy(np.stack([f[1] for f in frames])).to(dev), gt_classes=torch.from_numpy(np.stack([f[2] for f in frames])).to(dev),
                draws=torch.from_numpy(draws).to(dev), perm=torch.from_numpy(perm).to(dev), candidates=torch.from_numpy(cand).to(dev),
                candidate_lengths=torch.from_numpy(lens).to(dev))
    for _ in range(5):
        out = aug.padded(**args)
    torch.cuda.synchronize()
    windows = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            out = aug.padded(**args)
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / a.calls)
    # the same steps in numpy on this host, float32, frame by frame; checked against the device before it is timed
    cfg = dict(min_points=a.min_points, group_classes=aug.group_classes, group_max=aug.group_max, rate=1.0, rot=ROT, scale=SCALE, std=[STD] * 3,
               flip_probability=0.5, bv_range=[float(np.float32(PC_RANGE[i])) for i in (0, 1, 3, 4)])
    npts = out["num_points"].cpu().numpy()

    def host():
        res = []
        for b, (pts, boxes, classes) in enumerate(frames):
            cands = [cand[b, q, :lens[b, q]] for q in range(len(aug.group_classes))]
            probe_total = int(npts[b])
            order = np.argsort(perm[b, :probe_total], kind="stable")
            res.append(AO.preprocess(pts, boxes, classes, cfg, draws[b], order, cands, db_np, np.float32))
        return res
    ref = host()
    acc = out["num_accepted"].cpu().numpy()
    same = all(np.array_equal(out["accepted"][b, :acc[b]].cpu().numpy(), ref[b]["accepted"]) and int(out["num_boxes"][b]) == len(ref[b]["gt_classes"])
               for b in range(a.batch))
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"tool": "detaugbench", "batch": a.batch, "points_per_frame": a.points, "gt_per_frame": a.gt, "database_objects": int(db.size),
                      "database_points": int(db_np["offsets"][-1]), "point_capacity": cap, "min_points_in_gt": a.min_points,
                      "accepted_per_frame": [int(v) for v in acc], "device_ms_per_call_median": float(np.median(windows)),
                      "device_ms_per_call_min": float(min(windows)), "device_ms_per_call_max": float(max(windows)), "windows": a.windows,
                      "calls_per_window": a.calls, "launches_per_call": 3 + (1 if a.min_points > 0 else 0) + (1 if a.min_points > 0 else 0),
                      "host_round_trips_per_call": 0, "host_numpy_ms_per_batch_median": float(np.median(host_ms)),
                      "host_numpy_ms_per_batch_min": float(min(host_ms)), "host_is": "float32 numpy restatement, no numba: not the reference",
                      "same_accepted_and_kept_as_host": bool(same)}))


if __name__ == "__main__":
    main()
