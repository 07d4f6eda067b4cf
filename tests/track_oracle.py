"""tests/track_oracle.py -- numpy restatement of the tracker's steps (include/link_amd.h, section Q) in exactly the stated arithmetic.
The project's own code: a list of dicts per sequence and an N x M distance matrix, the way the steps are written down, with a second
path that runs one greedy scan per tracking class (what the kernel does) to show that the decomposition changes nothing.
"""
import numpy as np

FIELDS = ("ct", "tracking", "label", "tracking_id", "age", "active", "src")


class OracleTracker:
    def __init__(self, label_map, max_dist, max_age=0, score_thresh=None, capacity=None, per_class=False):
        self.label_map = [int(v) for v in label_map]
        self.max_dist = np.asarray(max_dist, np.float32)
        self.max_age, self.capacity, self.per_class = int(max_age), capacity, per_class
        self.score_thresh = None if score_thresh is None or np.isnan(score_thresh) else np.float32(score_thresh)
        self.reset()

    def reset(self):
        self.id_count, self.tracks, self.status = 0, [], 0

    def _greedy(self, dist):
        """dist float32 [n, m] with inf at invalid pairs -> list of (row, column): the first minimum of every row in turn"""
        dist = dist.copy()
        out = []
        for i in range(dist.shape[0]):
            if dist.shape[1] == 0:
                break
            j = int(dist[i].argmin())
            if dist[i, j] < np.float32(1e16):
                dist[:, j] = np.inf
                out.append((i, j))
        return out

    def step(self, boxes, scores, labels, time_lag, count=None, pose=None, reset=False, want_stats=False):
        """-> det_tracking_id int32 [N], det_active int32 [N] (and the gap statistics of the frame)"""
        if reset:
            self.reset()
        boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
        N = boxes.shape[0]
        det_id, det_active = np.full(N, -1, np.int32), np.zeros(N, np.int32)
        stats = {"rel_gap": np.inf, "max_gap": np.inf}
        self.status = 0
        dets = []
        for i in range(N if count is None else min(int(count), N)):
            lab = int(labels[i])
            if lab < 0 or lab >= len(self.label_map) or self.label_map[lab] < 0:
                continue
            x, y, z = (np.float64(boxes[i, k]) for k in range(3))
            vx, vy = np.float64(boxes[i, -3]), np.float64(boxes[i, -2])
            if pose is not None:
                P = np.asarray(pose, np.float64).reshape(-1)
                ct = np.array([((P[0] * x + P[1] * y) + P[2] * z) + P[3], ((P[4] * x + P[5] * y) + P[6] * z) + P[7]])
                vx, vy = P[0] * vx + P[1] * vy, P[4] * vx + P[5] * vy
            else:
                ct = np.array([x, y])
            tracking = np.array([vx, vy]) * -1 * np.float64(time_lag)
            dets.append({"ct": ct, "tracking": tracking, "label": self.label_map[lab], "src": i, "score": scores[i]})
        if not dets:
            self.tracks = []
            return (det_id, det_active, stats) if want_stats else (det_id, det_active)
        n, m = len(dets), len(self.tracks)
        pos = np.array([d["ct"] + d["tracking"].astype(np.float32) for d in dets], np.float32)
        dlab = np.array([d["label"] for d in dets], np.int32)
        tpos = np.array([t["ct"] for t in self.tracks], np.float32).reshape(m, 2)
        tlab = np.array([t["label"] for t in self.tracks], np.int32)
        ex, ey = tpos[None, :, 0] - pos[:, None, 0], tpos[None, :, 1] - pos[:, None, 1]
        dist = np.sqrt(ex * ex + ey * ey)                                    # float32, every operation rounded on its own
        assert dist.dtype == np.float32
        invalid = (dist > self.max_dist[dlab][:, None]) | (dlab[:, None] != tlab[None, :])
        dist = np.where(invalid, np.float32(np.inf), dist)
        if self.per_class:
            matches = []
            for c in range(len(self.max_dist)):
                rows, cols = np.nonzero(dlab == c)[0], np.nonzero(tlab == c)[0]
                matches += [(int(rows[i]), int(cols[j])) for i, j in self._greedy(dist[np.ix_(rows, cols)])]
            matches.sort()
        else:
            matches = self._greedy(dist)
        if want_stats and m:
            free = np.ones(m, bool)
            md = dict(matches)
            for i in range(n):
                if i in md:
                    row = np.where(free, dist[i], np.inf).astype(np.float64)
                    best = row[md[i]]
                    rest = np.delete(row, md[i])
                    if rest.size and np.isfinite(rest.min()):
                        stats["rel_gap"] = min(stats["rel_gap"], (rest.min() - best) / max(rest.min(), 1e-30))
                    free[md[i]] = False
            same = dlab[:, None] == tlab[None, :]
            raw = np.sqrt(ex * ex + ey * ey).astype(np.float64)
            if same.any():
                stats["max_gap"] = float(np.abs(raw - self.max_dist[dlab][:, None].astype(np.float64))[same].min())
        matched_rows, matched_cols = {i for i, _ in matches}, {j for _, j in matches}
        new = []
        for i, j in matches:
            new.append({**dets[i], "tracking_id": self.tracks[j]["tracking_id"], "age": 1, "active": self.tracks[j]["active"] + 1})
        for i in range(n):
            if i in matched_rows:
                continue
            if self.score_thresh is None or dets[i]["score"] > self.score_thresh:
                self.id_count += 1
                new.append({**dets[i], "tracking_id": self.id_count, "age": 1, "active": 1})
        for t in new:
            det_id[t["src"]], det_active[t["src"]] = t["tracking_id"], t["active"]
        for j, t in enumerate(self.tracks):
            if j not in matched_cols and t["age"] < self.max_age:
                new.append({**t, "age": t["age"] + 1, "active": 0, "ct": t["ct"] - t["tracking"], "src": -1})
        if self.capacity is not None and len(new) > self.capacity:
            new, self.status = new[:self.capacity], 1
        self.tracks = new
        return (det_id, det_active, stats) if want_stats else (det_id, det_active)

    def arrays(self):
        """the ordered track list as arrays (ct, tracking float64 [n, 2]; the rest int32 [n])"""
        n = len(self.tracks)
        out = {"ct": np.array([t["ct"] for t in self.tracks], np.float64).reshape(n, 2),
               "tracking": np.array([t["tracking"] for t in self.tracks], np.float64).reshape(n, 2)}
        for k in FIELDS[2:]:
            out[k] = np.array([t[k] for t in self.tracks], np.int32)
        return out


def run_sequence(tracker, fx, want_stats=False):
    """Drive a tracker over a fixture (arrays of tests/golden/track_*.npz) -> per-frame records padded like the fixture's"""
    F, N = fx["labels"].shape
    L = int(fx["list_len"])
    rec = {"det_tracking_id": np.full((F, N), -1, np.int32), "det_active": np.zeros((F, N), np.int32),
           "n_tracks": np.zeros(F, np.int32), "id_count": np.zeros(F, np.int32), "status": np.zeros(F, np.int32),
           "ct": np.zeros((F, L, 2), np.float64), "tracking": np.zeros((F, L, 2), np.float64),
           **{k: np.zeros((F, L), np.int32) for k in FIELDS[2:]}}
    stats = {"rel_gap": np.inf, "max_gap": np.inf}
    for f in range(F):
        pose = fx["pose"][f] if "pose" in fx else None
        r = tracker.step(fx["boxes"][f], fx["scores"][f], fx["labels"][f], fx["time_lag"][f], pose=pose, want_stats=want_stats)
        if want_stats:
            stats = {k: min(stats[k], r[2][k]) for k in stats}
        a = tracker.arrays()
        n = a["label"].shape[0]
        rec["det_tracking_id"][f], rec["det_active"][f] = r[0], r[1]
        rec["n_tracks"][f], rec["id_count"][f], rec["status"][f] = n, tracker.id_count, tracker.status
        for k in FIELDS:
            rec[k][f, :n] = a[k]
    return (rec, stats) if want_stats else rec


# ---- shared by tests/test_cpu_track.py and tests/test_gpu_track.py -----------------------------------------------------------------
def load_fixtures(golden_dir):
    """-> {name: (meta, arrays)} of tests/golden/track_*.npz"""
    import glob
    import json
    import os
    out = {}
    for path in sorted(glob.glob(os.path.join(golden_dir, "track_*.npz"))):
        z = np.load(path)
        out[os.path.basename(path)[6:-4]] = (json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"})
    return out


def make_tracker(meta, num_sequences=1, **kw):
    import link_amd
    return link_amd.CenterTracker(meta["label_map"], meta["max_dist"], max_age=meta["max_age"], score_thresh=meta["score_thresh"],
                                  capacity=kw.pop("capacity", meta.get("capacity", 1024)), num_sequences=num_sequences, **kw)


def assert_frame(out, s, exp, f, what):
    """every output and every state field of sequence s after a step equals frame f of the expected record, exactly"""
    host = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in out.items()}
    n = int(exp["n_tracks"][f])
    for k in ("n_tracks", "id_count", "status"):
        assert int(host[k][s]) == int(exp[k][f]), (what, f, k, int(host[k][s]), int(exp[k][f]))
    for k in ("det_tracking_id", "det_active"):
        got = host[k][s] if host[k].ndim == 2 else host[k]
        assert np.array_equal(got[:exp[k].shape[1]], exp[k][f]) and (got[exp[k].shape[1]:] == (-1 if k == "det_tracking_id" else 0)).all(), (what, f, k)
    for k in FIELDS:
        got, want = host[k][s, :n], exp[k][f, :n]
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, f, k, np.nonzero(got != want))     # float64 ct: bit for bit
