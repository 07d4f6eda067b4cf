"""tools/trackbench.py -- per-frame time of the tracker's step on the device at the nuScenes validation shape:
S = 150 sequences advancing together, about 300 detections per frame in 320 padded slots, the ten detection classes, max_age 3,
40 frames; and S = 1.

Timed: CenterTracker.step with device tensors for time_lag and reset (no upload, no read-back), device events around a window of one
pass over the 40 frames, 7 windows, median and the spread min .. max -- eagerly (one Python call and one launch per frame) and as one
captured graph of the 40 steps (the launches without the Python between them).  Against: the same frames through the numpy
composition of the same steps (link_amd.tracker's CPU path, which tests/test_cpu_track.py pins on the reference's recorded lists)
on this machine's host, one sequence after another as the reference runs them; it is timed on --host-sequences of the sequences and
scaled to S, since the sequences are independent and equally large.  It is NOT the reference's PubTracker (whose dict lists it
replaces by arrays), so the host figure stands for "the same steps in numpy on this host".  Also printed: launches and host round
trips per frame, counted from what the code does, and whether the device's ids equal the host's on the timed sequences.
Needs a GPU; prints one JSON line per S."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import link_amd as la  # noqa: E402


def scenes(rng, S, F, n_obj, slots):
    """-> boxes [F, S, slots, 9], scores, labels (-1 unused), time_lag [F, S]: objects move with noise, 15 % drop out per frame"""
    lab = rng.integers(0, 10, (S, n_obj))
    pos = rng.uniform(-50, 50, (S, n_obj, 2))
    vel = rng.normal(0, 3.0, (S, n_obj, 2))
    boxes, scores = np.zeros((F, S, slots, 9), np.float32), np.zeros((F, S, slots), np.float32)
    labels, lags = np.full((F, S, slots), -1, np.int32), rng.uniform(0.45, 0.55, (F, S))
    for f in range(F):
        pos += vel * lags[f][:, None, None] + rng.normal(0, 0.15, pos.shape)
        for s in range(S):
            keep = rng.permutation(np.nonzero(rng.random(n_obj) > 0.15)[0])[:slots]
            n = len(keep)
            boxes[f, s, :n, :2], boxes[f, s, :n, 3:6] = pos[s, keep], rng.uniform(0.5, 4, (n, 3))
            boxes[f, s, :n, 6:8] = vel[s, keep] + rng.normal(0, 0.6, (n, 2))
            scores[f, s, :n], labels[f, s, :n] = rng.uniform(0.1, 1, n), lab[s, keep]
    return boxes, scores, labels, lags


def bench(S, a, rng):
    dev = torch.device("cuda")
    boxes, scores, labels, lags = scenes(rng, S, a.frames, a.objects, a.slots)
    db, ds, dl, dlag = (torch.from_numpy(v).to(dev) for v in (boxes, scores, labels, lags))
    first = torch.ones(S, dtype=torch.uint8, device=dev)
    later = torch.zeros(S, dtype=torch.uint8, device=dev)
    t = la.CenterTracker.nuscenes(max_age=3, capacity=a.capacity, num_sequences=S)

    def one_pass(keep=None):
        for f in range(a.frames):
            out = t.step(db[f], ds[f], dl[f], dlag[f], reset=first if f == 0 else later)
            if keep is not None:
                keep.append(out["det_tracking_id"].clone())
    ids = []
    one_pass(ids)                                                      # warm-up, and the ids to compare
    torch.cuda.synchronize()

    def timed(fn):
        win = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            win.append(e0.elapsed_time(e1) / a.frames)
        return win
    eager = timed(one_pass)
    wall0 = time.perf_counter()
    one_pass()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - wall0) * 1e3 / a.frames
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_pass()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_pass()
    graph.replay()
    torch.cuda.synchronize()
    graphed = timed(graph.replay)

    # the host: the numpy composition, one sequence after another
    hs = min(S, a.host_sequences)
    host_ms, same = [], True
    for rep in range(a.host_repeats):
        t0 = time.perf_counter()
        got = []
        for s in range(hs):
            h = la.CenterTracker.nuscenes(max_age=3, capacity=a.capacity)
            for f in range(a.frames):
                out = h.step(torch.from_numpy(boxes[f, s:s + 1]), torch.from_numpy(scores[f, s:s + 1]), torch.from_numpy(labels[f, s:s + 1]),
                             float(lags[f, s]))
                if rep == 0:
                    got.append((f, s, out["det_tracking_id"][0].numpy()))
        host_ms.append((time.perf_counter() - t0) * 1e3 / (hs * a.frames))
        for f, s, v in got:
            same &= bool(np.array_equal(ids[f][s].cpu().numpy(), v))
    n_used = float((labels >= 0).sum(-1).mean())
    med = float(np.median(host_ms))
    return {"tool": "trackbench", "sequences": S, "frames": a.frames, "slots": a.slots, "detections_per_frame_mean": n_used, "max_age": 3,
            "capacity": a.capacity, "windows": a.windows,
            "device_eager_ms_per_frame_median": float(np.median(eager)), "device_eager_ms_per_frame_min": float(min(eager)),
            "device_eager_ms_per_frame_max": float(max(eager)), "device_eager_wall_ms_per_frame": wall,
            "device_graph_ms_per_frame_median": float(np.median(graphed)), "device_graph_ms_per_frame_min": float(min(graphed)),
            "device_graph_ms_per_frame_max": float(max(graphed)),
            "device_launches_per_frame": 1, "device_host_round_trips_per_frame": 0,
            "host_numpy_ms_per_sequence_frame_median": med, "host_numpy_ms_per_sequence_frame_min": float(min(host_ms)),
            "host_sequences_timed": hs, "host_numpy_ms_per_frame_all_sequences": med * S,
            "host_round_trips_per_frame": 1, "host_is": "numpy composition of the same steps, one sequence after another: not the reference's PubTracker",
            "same_ids_as_host": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[150, 1])
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--objects", type=int, default=350, help="objects per scene; 15 %% drop out of every frame")
    ap.add_argument("--slots", type=int, default=320)
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-sequences", type=int, default=8)
    ap.add_argument("--host-repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trackbench needs a GPU")
    for S in a.sequences:
        print(json.dumps(bench(S, a, np.random.default_rng(7))), flush=True)


if __name__ == "__main__":
    main()
