"""tests/golden/make_golden_track.py -- records the fixtures of tests/test_cpu_track.py and tests/test_gpu_track.py
(tests/golden/track_*.npz).  The tests do not run it.

Where the reference checkout (argument 1 or $LINK_REFERENCE) can be loaded, the expected track lists come from its own trackers on
the CPU: detection/tools/nusc_tracking/pub_tracker.py::PubTracker and detection/tools/waymo_tracking/tracker.py::PubTracker, loaded
by path (nusc_tracking on sys.path for track_utils, the constructor's print swallowed) and driven with the dict lists they expect,
built from the fixture arrays.  A frame with no detection of a tracked class is handed over as an empty list (the reference raises
an IndexError on an untracked-only frame: the project's deliberate difference).  Otherwise -- and for the capacity fixture, since
the reference has no capacity -- the meta says "restatement" and tests/track_oracle.py is the pin.  Nothing of the reference is
copied here; fixtures hold arrays and settings only.

Every fixture's meta records the smallest relative gap between the best and the second-best valid distance of a matched row and
the smallest distance between any same-class pair's distance and max_dist (not for the crafted fixture, whose ties are the point):
the arithmetic is meant to be bit-exact and the tests assert equality, the gaps tell a knife edge from a defect when one fails.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import track_oracle as TO  # noqa: E402

NUSC_DET = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
NUSC_TRK = ("bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck")
NUSC_MAP = [NUSC_TRK.index(n) if n in NUSC_TRK else -1 for n in NUSC_DET]
NUSC_DIST = [3, 5.5, 4, 13, 1, 3, 4]                       # the reference's table in NUSC_TRK's order (checked against it below)
WAYMO_DET = ("VEHICLE", "PEDESTRIAN", "CYCLIST", "SIGN")
WAYMO_MAP = [0, 1, 2, -1]
WAYMO_DIST = [0.8, 0.4, 0.6]


def load_reference(root):
    try:
        nusc = os.path.join(root, "detection", "tools", "nusc_tracking")
        sys.path.insert(0, nusc)
        mods = []
        for name, path in (("ref_nusc_tracker", os.path.join(nusc, "pub_tracker.py")),
                           ("ref_waymo_tracker", os.path.join(root, "detection", "tools", "waymo_tracking", "tracker.py"))):
            spec = importlib.util.spec_from_file_location(name, path)
            m = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(m)
            mods.append(m)
        assert [mods[0].NUSCENE_CLS_VELOCITY_ERROR[n] for n in NUSC_TRK] == NUSC_DIST and tuple(mods[0].NUSCENES_TRACKING_NAMES) == NUSC_TRK
        return mods
    except Exception as e:                                                            # noqa: BLE001
        print("reference not loaded:", repr(e))
        return None


def global_inputs(boxes, pose):
    """translation and velocity of every slot as the reference gets them: float64, in the global frame when there is a pose"""
    b = boxes.astype(np.float64)
    x, y, z, vx, vy = b[:, 0], b[:, 1], b[:, 2], b[:, -3], b[:, -2]
    if pose is None:
        return np.stack([x, y, z], 1), np.stack([vx, vy], 1)
    P = pose
    g = [((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3] for r in range(3)]
    return np.stack(g, 1), np.stack([P[0] * vx + P[1] * vy, P[4] * vx + P[5] * vy], 1)


def run_reference(mods, fx, cfg):
    names = WAYMO_DET if cfg["form"] == "waymo" else NUSC_DET
    with contextlib.redirect_stdout(io.StringIO()):
        if cfg["form"] == "waymo":
            trk = mods[1].PubTracker(max_age=cfg["max_age"], max_dist=dict(zip(WAYMO_DET[:3], WAYMO_DIST)), score_thresh=cfg["score_thresh"])
        else:
            trk = mods[0].PubTracker(hungarian=False, max_age=cfg["max_age"])
    F, N = fx["labels"].shape
    L = int(fx["list_len"])
    rec = {"det_tracking_id": np.full((F, N), -1, np.int32), "det_active": np.zeros((F, N), np.int32),
           "n_tracks": np.zeros(F, np.int32), "id_count": np.zeros(F, np.int32), "status": np.zeros(F, np.int32),
           "ct": np.zeros((F, L, 2), np.float64), "tracking": np.zeros((F, L, 2), np.float64),
           **{k: np.zeros((F, L), np.int32) for k in TO.FIELDS[2:]}}
    for f in range(F):
        trans, vel = global_inputs(fx["boxes"][f], fx["pose"][f] if "pose" in fx else None)
        dets = [{"detection_name": names[int(fx["labels"][f, i])], "translation": list(trans[i]), "velocity": list(vel[i]),
                 "score": fx["scores"][f, i], "slot": i} for i in range(N) if fx["labels"][f, i] >= 0]
        if not any(cfg["label_map"][int(fx["labels"][f, i])] >= 0 for i in range(N) if fx["labels"][f, i] >= 0):
            dets = []
        with contextlib.redirect_stdout(io.StringIO()):
            out = trk.step_centertrack(dets, fx["time_lag"][f])
        n = len(out)
        rec["n_tracks"][f], rec["id_count"][f] = n, trk.id_count
        for p, t in enumerate(out):
            rec["ct"][f, p], rec["tracking"][f, p] = t["ct"], t["tracking"]
            rec["label"][f, p], rec["tracking_id"][f, p], rec["age"][f, p], rec["active"][f, p] = t["label_preds"], t["tracking_id"], t["age"], t["active"]
            rec["src"][f, p] = t["slot"] if t["active"] > 0 else -1
            if t["active"] > 0:
                rec["det_tracking_id"][f, t["slot"]], rec["det_active"][f, t["slot"]] = t["tracking_id"], t["active"]
    return rec


def pad_frames(frames, nmax, rng=None, gappy=False):
    """frames: list of (boxes [n, 9], scores [n], labels [n]) -> padded arrays, unused slots -1 (at random places when gappy)"""
    F = len(frames)
    boxes, scores = np.zeros((F, nmax, 9), np.float32), np.zeros((F, nmax), np.float32)
    labels = np.full((F, nmax), -1, np.int32)
    for f, (b, s, l) in enumerate(frames):
        n = len(l)
        idx = np.sort(rng.choice(nmax, n, replace=False)) if gappy else np.arange(n)
        boxes[f, idx], scores[f, idx], labels[f, idx] = b, s, l
    return boxes, scores, labels


def random_scene(rng, schedule, labels, lag_lo, lag_hi, speed, noise, drop=0.15, score=lambda rng, n: rng.uniform(0.1, 1.0, n)):
    """objects move with noise; frame f shows the first schedule[f] objects, the large frames minus a 15 % dropout"""
    schedule = [np.arange(n) if np.isscalar(n) else np.asarray(n) for n in schedule]      # a count shows the first objects
    n_obj = max(max((int(k.max()) + 1 if k.size else 0) for k in schedule), 1)
    lab = rng.choice(np.asarray(labels), n_obj) if not np.isscalar(labels) else rng.integers(0, labels, n_obj)
    pos = rng.uniform(-50, 50, (n_obj, 3)) * [1, 1, 0.02]
    vel = rng.normal(0, speed, (n_obj, 2))
    frames, lags = [], []
    for keep in schedule:
        lag = rng.uniform(lag_lo, lag_hi)
        pos[:, :2] += vel * lag + rng.normal(0, noise, (n_obj, 2))
        if keep.size > 100:
            keep = keep[rng.random(keep.size) > drop]
        keep = rng.permutation(keep)                          # detections come in score order, not object order
        b = np.zeros((len(keep), 9), np.float32)
        b[:, :3], b[:, 3:6] = pos[keep], rng.uniform(0.5, 4, (len(keep), 3))
        b[:, 6:8] = vel[keep] + rng.normal(0, 0.2 * speed, (len(keep), 2))
        b[:, 8] = rng.uniform(-3.14, 3.14, len(keep))
        frames.append((b, score(rng, len(keep)).astype(np.float32), lab[keep].astype(np.int32)))
        lags.append(lag)
    return frames, np.asarray(lags, np.float64)


def crafted():
    """the crafted frames of the nuScenes form, max_age 3, time lag 0.5; every case in a region of its own"""
    CAR, TRUCK, BARRIER, PED, CONE = 0, 1, 5, 8, 9
    up = float(np.nextafter(np.float32(1), np.float32(2)))

    def det(x, y, lab, vx=0.0, vy=0.0):
        return ([x, y, 0.5, 2, 4, 1.5, vx, vy, 0.1], 0.5, lab)
    f0 = [det(0, 0, CAR), det(0, 0, CAR),                     # two tracks at the identical position
          det(100, 0, CAR), det(102, 0, CAR),                 # a detection will sit exactly between these
          det(200, 0, PED),                                   # distance == max_dist (1 for a pedestrian)
          det(300, 0, PED),                                   # distance one ulp above
          det(400, 0, CAR), det(400, 0.5, TRUCK)]             # a nearer track of another class
    f1 = [det(0.5, 0, CAR), det(101, 0, CAR), det(201, 0, PED), det(300, up, PED), det(400, 0.4, CAR)]
    f2 = [det(0.5, 0, BARRIER), det(101, 0, CONE)]            # untracked classes only: clears the list, keeps id_count
    f3 = [det(500, 0, CAR, 1.0), det(600, 0, CAR), det(700, 0, CAR)]
    f4 = [det(700, 0, CAR)]                                   # X (500) and Y (600) are carried over
    f5 = [det(700, 0, CAR)]
    f6 = [det(700, 0, CAR), det(501.5, 0, CAR, 1.0)]          # X revived after two frames (active 1), Y aged out at max_age
    f7 = []                                                   # an empty frame in mid-sequence
    f8 = [det(700, 0, CAR), det(0, 0, PED)]                   # the ids go on from id_count
    f9 = [det(700.5, 0, CAR), det(0, 0.5, PED), det(3, 3, BARRIER)]
    frames = []
    for f in (f0, f1, f2, f3, f4, f5, f6, f7, f8, f9):
        frames.append((np.array([d[0] for d in f], np.float32).reshape(-1, 9), np.array([d[1] for d in f], np.float32),
                       np.array([d[2] for d in f], np.int32)))
    return frames, np.full(len(frames), 0.5, np.float64)


def poses(rng, F):
    """ego poses of a drive: yaw and translation drift, a little roll and pitch; row-major 3 x 4, float64"""
    out = np.zeros((F, 12))
    for f in range(F):
        yaw, pitch, roll = 0.7 + 0.05 * f + rng.normal(0, 0.01), rng.normal(0, 0.01), rng.normal(0, 0.01)
        cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        out[f] = np.concatenate([R, np.array([[600.0 + 4 * f], [1500.0 + 3 * f], [1.8]]) + rng.normal(0, 0.01, (3, 1))], 1).reshape(-1)
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LINK_REFERENCE", "")
    mods = load_reference(root) if root else None
    nusc = {"form": "nuscenes", "label_map": NUSC_MAP, "max_dist": NUSC_DIST, "score_thresh": None}
    waymo = {"form": "waymo", "label_map": WAYMO_MAP, "max_dist": WAYMO_DIST, "score_thresh": 0.1}
    cases = []
    rng = np.random.default_rng(20261020)
    fr, lag = random_scene(rng, [300, 300, 65, 64, 63, 1, 0, 1, 300, 300], 10, 0.45, 0.55, 3.0, 0.15)
    cases.append(("a0", {**nusc, "max_age": 0}, fr, lag, {}))
    fr, lag = random_scene(rng, [300, 300, 300, 64, 65, 63, 300, 1, 300, 300, 0, 300], 10, 0.45, 0.55, 3.0, 0.15)
    cases.append(("a1", {**nusc, "max_age": 3}, fr, lag, {}))
    fr, lag = random_scene(rng, [120] * 9, 10, 0.45, 0.55, 3.0, 0.15, drop=0.3)
    cases.append(("a2", {**nusc, "max_age": 3}, fr, lag, {"gappy": True, "pose": True, "nmax": 160}))
    fr, lag = random_scene(rng, [65, 64, 63, 65, 300, 300, 64, 1, 65, 63], 4, 0.09, 0.11, 2.0, 0.05,
                           score=lambda rng, n: rng.uniform(0.0, 0.2, n))
    cases.append(("b0", {**waymo, "max_age": 2}, fr, lag, {}))
    fr, lag = crafted()
    cases.append(("c0", {**nusc, "max_age": 3}, fr, lag, {"crafted": True}))
    # (d) tracked classes only: 64 tracks, then 65, then other objects, so that carried-over tracks push the list over a capacity of 96
    pick = [np.arange(64), np.arange(65), np.arange(40, 110), np.arange(64), np.arange(30, 110), np.arange(65), np.arange(64), np.arange(96)]
    fr, lag = random_scene(rng, pick, [k for k, v in enumerate(NUSC_MAP) if v >= 0], 0.45, 0.55, 3.0, 0.15)
    cases.append(("d0", {**nusc, "max_age": 3, "capacity": 96}, fr, lag, {"nmax": 96}))

    for name, cfg, frames, lag, opt in cases:
        nmax = opt.get("nmax", max(max(len(f[2]) for f in frames), 1))
        boxes, scores, labels = pad_frames(frames, nmax, rng, opt.get("gappy", False))
        fx = {"boxes": boxes, "scores": scores, "labels": labels, "time_lag": lag}
        if opt.get("pose"):
            fx["pose"] = poses(rng, len(frames))
        probe = TO.OracleTracker(cfg["label_map"], cfg["max_dist"], cfg["max_age"], cfg["score_thresh"])
        fx["list_len"] = 1
        longest = 0
        for f in range(len(frames)):
            probe.step(boxes[f], scores[f], labels[f], lag[f], pose=fx["pose"][f] if "pose" in fx else None)
            longest = max(longest, len(probe.tracks))
        fx["list_len"] = np.int32(max(longest, 1))
        orc, stats = TO.run_sequence(TO.OracleTracker(cfg["label_map"], cfg["max_dist"], cfg["max_age"], cfg["score_thresh"],
                                                      capacity=cfg.get("capacity")), fx, want_stats=True)
        source = "restatement"
        exp = orc
        if mods is not None and "capacity" not in cfg:
            exp = run_reference(mods, fx, cfg)
            source = "reference"
        meta = {"source": source, **{k: v for k, v in cfg.items()}, "frames": len(frames),
                "n_per_frame": [int((labels[f] >= 0).sum()) for f in range(len(frames))],
                "n_tracks_per_frame": [int(v) for v in exp["n_tracks"]]}
        if not opt.get("crafted"):
            meta["min_rel_gap_best_second"] = float(stats["rel_gap"])
            meta["min_gap_to_max_dist"] = float(stats["max_gap"])
        same = all(np.array_equal(exp[k], orc[k]) for k in exp)
        print(name, source, "oracle equal:", same, json.dumps({k: meta[k] for k in meta if k not in ("label_map", "max_dist")}))
        np.savez_compressed(os.path.join(HERE, f"track_{name}.npz"), meta=json.dumps(meta), **fx, **{"exp_" + k: v for k, v in exp.items()})


if __name__ == "__main__":
    main()
