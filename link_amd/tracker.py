"""link_amd/tracker.py -- the CenterPoint tracker on the device (csrc/track.hip, section Q of include/link_amd.h): greedy centre
matching of a frame's detections against the track list, for a batch of independent sequences in one launch.

What detection/tools/nusc_tracking/pub_tracker.py (PubTracker.step_centertrack, with track_utils.py::greedy_assignment) and
detection/tools/waymo_tracking/tracker.py do on the host with a list of dicts per frame.  CenterTracker.step takes the padded output
of CenterHeadDecoder.predict_padded / fuse_detections_padded (one sequence per batch row) or one frame's predict dict, keeps the
track lists on the device and never reads anything back, so a step can be captured in a graph.  The semantics, quirks included, are
listed step by step in include/link_amd.h; the differences on purpose: a frame whose detections are all of untracked classes clears
the track list like an empty frame (the reference raises an IndexError there), and hungarian=True is not built (the reference's path
calls a linear_assignment it never imports).

CPU tensors and num_sequences == 0 run a numpy composition of the same steps (one sequence after another, as the reference does).

boxes_to_global moves padded boxes into the global frame.  It is pinned on its float64 definition only: the reference does this
step with the nuScenes devkit's Box / Quaternion classes (detection/det3d/datasets/nuscenes/nusc_common.py::_lidar_nusc_box_to_global),
which this project does not depend on.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

# pub_tracker.py:8-16: the tracked classes, and :22-30: the largest centre distance of a match per class (metres per 0.5 s)
NUSCENES_TRACKING_NAMES = ("bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck")
NUSCENE_CLS_VELOCITY_ERROR = {"car": 4, "truck": 4, "bus": 5.5, "trailer": 3, "pedestrian": 1, "motorcycle": 13, "bicycle": 3}
# the ten detection classes in the head's task order (detection/configs/nusc/voxelnet/*.py: tasks)
NUSCENES_DETECTION_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                            "traffic_cone")
WAYMO_TRACKING_NAMES = ("VEHICLE", "PEDESTRIAN", "CYCLIST")     # waymo_tracking/tracker.py:21-25

LIST_FIELDS = ("ct", "tracking", "label", "tracking_id", "age", "active", "src")


def _pose_rows(pose, S: int) -> np.ndarray:
    """[S, 12] float64 of a [S, 12], [S, 3, 4], [S, 4, 4] (or, for one sequence, [12], [3, 4], [4, 4]) transform"""
    p = np.asarray(pose, np.float64)
    if p.ndim <= 2 and p.size in (12, 16) and S == 1:
        p = p.reshape(1, -1, 4)
    if p.ndim == 2:
        p = p.reshape(p.shape[0], -1, 4)
    if p.ndim != 3 or p.shape[0] != S or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"pose: one 3 x 4 (or 4 x 4) transform per sequence expected, got {np.asarray(pose).shape}")
    return np.ascontiguousarray(p[:, :3, :].reshape(S, 12))


def _empty_tracks() -> Dict[str, np.ndarray]:
    return {"ct": np.zeros((0, 2), np.float64), "tracking": np.zeros((0, 2), np.float64),
            **{k: np.zeros(0, np.int32) for k in LIST_FIELDS[2:]}}


def _host_step(cfg, old, id_count, boxes, scores, labels, count, lag, pose):
    """One sequence, one frame, in numpy: the steps of include/link_amd.h section Q.  -> (tracks, id_count, det_id, det_active,
    overflow)"""
    N = boxes.shape[0]
    det_id, det_active = np.full(N, -1, np.int32), np.zeros(N, np.int32)
    lab = np.asarray(labels).astype(np.int64)
    used = (np.arange(N) < (N if count is None else int(count))) & (lab >= 0) & (lab < len(cfg["label_map"]))
    tl = np.where(used, cfg["label_map"][np.clip(lab, 0, len(cfg["label_map"]) - 1)], -1)
    slots = np.nonzero(tl >= 0)[0].astype(np.int32)
    if slots.size == 0:
        return _empty_tracks(), id_count, det_id, det_active, False
    b = boxes[slots].astype(np.float32)
    x, y, z = (b[:, k].astype(np.float64) for k in range(3))
    vx, vy = b[:, -3].astype(np.float64), b[:, -2].astype(np.float64)
    if pose is not None:
        P = pose
        ct = np.stack([((P[0] * x + P[1] * y) + P[2] * z) + P[3], ((P[4] * x + P[5] * y) + P[6] * z) + P[7]], 1)
        vx, vy = P[0] * vx + P[1] * vy, P[4] * vx + P[5] * vy
    else:
        ct = np.stack([x, y], 1)
    tracking = np.stack([vx, vy], 1) * -1 * np.float64(lag)
    dets = (ct + tracking.astype(np.float32)).astype(np.float32)
    dlab = tl[slots].astype(np.int32)
    M = old["label"].shape[0]
    dmatch, tmatch = np.full(slots.size, -1, np.int64), np.full(M, -1, np.int64)
    if M:
        tr32 = old["ct"].astype(np.float32)
        d = tr32[None, :, :] - dets[:, None, :]
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        invalid = (dist > cfg["max_dist"][dlab][:, None]) | (dlab[:, None] != old["label"][None, :]) | ~(dist < np.float32(1e16))
        dist = np.where(invalid, np.float32(np.inf), dist)
        for i in range(slots.size):
            j = int(dist[i].argmin())
            if dist[i, j] < np.inf:
                dist[:, j] = np.inf
                dmatch[i], tmatch[j] = j, i
    th = cfg["score_thresh"]
    ism = dmatch >= 0
    isn = ~ism if th is None else (~ism & (scores[slots].astype(np.float32) > np.float32(th)))
    carried = (tmatch < 0) & (old["age"] < cfg["max_age"])
    mi, ni, ci = np.nonzero(ism)[0], np.nonzero(isn)[0], np.nonzero(carried)[0]
    new_ids = id_count + 1 + np.arange(ni.size, dtype=np.int32)
    new = {"ct": np.concatenate([ct[mi], ct[ni], old["ct"][ci] - old["tracking"][ci]]),
           "tracking": np.concatenate([tracking[mi], tracking[ni], old["tracking"][ci]]),
           "label": np.concatenate([dlab[mi], dlab[ni], old["label"][ci]]),
           "tracking_id": np.concatenate([old["tracking_id"][dmatch[mi]], new_ids, old["tracking_id"][ci]]),
           "age": np.concatenate([np.ones(mi.size + ni.size, np.int32), old["age"][ci] + 1]),
           "active": np.concatenate([old["active"][dmatch[mi]] + 1, np.ones(ni.size, np.int32), np.zeros(ci.size, np.int32)]),
           "src": np.concatenate([slots[mi], slots[ni], np.full(ci.size, -1, np.int32)])}
    new = {k: (v.astype(np.float64) if k in ("ct", "tracking") else v.astype(np.int32)) for k, v in new.items()}
    n_det = mi.size + ni.size
    det_id[new["src"][:n_det]] = new["tracking_id"][:n_det]
    det_active[new["src"][:n_det]] = new["active"][:n_det]
    overflow = new["label"].shape[0] > cfg["capacity"]
    if overflow:
        new = {k: v[:cfg["capacity"]] for k, v in new.items()}
    return new, id_count + ni.size, det_id, det_active, overflow


class CenterTracker:
    """label_map: tracking label of every detection label (-1: not tracked); max_dist: largest centre distance of a match, per
    tracking label; max_age: frames a track survives without a detection; score_thresh: None for the nuScenes form, a number for
    the Waymo form (an unmatched detection starts a track only with score > score_thresh); capacity: tracks kept per sequence
    (<= 1024, and at least the padded detection count); num_sequences: the batch of independent sequences one step advances."""

    def __init__(self, label_map: Sequence[int], max_dist: Sequence[float], max_age: int = 0, score_thresh: Optional[float] = None,
                 capacity: int = 1024, num_sequences: int = 1, hungarian: bool = False):
        if hungarian:
            raise NotImplementedError("CenterTracker: hungarian=True is not built (the reference's path calls a linear_assignment it "
                                      "never imports)")
        label_map, max_dist = [int(v) for v in label_map], [float(v) for v in max_dist]
        if not 1 <= len(label_map) <= L.TRACK_MAX_LABELS or not 1 <= len(max_dist) <= L.TRACK_MAX_LABELS:
            raise ValueError(f"CenterTracker: 1..{L.TRACK_MAX_LABELS} detection and tracking labels")
        if any(v < -1 or v >= len(max_dist) for v in label_map):
            raise ValueError("CenterTracker: label_map entries are -1 or an index into max_dist")
        if any(not (0 <= v < 1e16) for v in max_dist):
            raise ValueError("CenterTracker: max_dist entries lie in [0, 1e16)")
        if not 1 <= int(capacity) <= L.TRACK_MAX_CAPACITY:
            raise ValueError(f"CenterTracker: capacity 1..{L.TRACK_MAX_CAPACITY}")
        if int(max_age) < 0 or int(num_sequences) < 0:
            raise ValueError("CenterTracker: max_age and num_sequences are not negative")
        if score_thresh is not None and math.isnan(float(score_thresh)):
            score_thresh = None
        self.label_map, self.max_dist, self.max_age, self.capacity = label_map, max_dist, int(max_age), int(capacity)
        self.score_thresh = None if score_thresh is None else float(score_thresh)
        self.num_sequences = int(num_sequences)
        c = L.LinkTrackCfg()
        c.n_det_labels, c.n_track_labels, c.max_age, c.capacity = len(label_map), len(max_dist), self.max_age, self.capacity
        c.score_thresh = float("nan") if self.score_thresh is None else self.score_thresh
        for i, v in enumerate(label_map):
            c.label_map[i] = v
        for i, v in enumerate(max_dist):
            c.max_dist[i] = v
        self.cfg = c
        self._host_cfg = {"label_map": np.asarray(label_map, np.int32), "max_dist": np.asarray(max_dist, np.float32),
                          "max_age": self.max_age, "score_thresh": self.score_thresh, "capacity": self.capacity}
        self._state = None                       # uint8 [S, state bytes] on the device, made by the first device step
        self.reset()

    # ---- presets -----------------------------------------------------------------------------------------------------------
    @classmethod
    def nuscenes(cls, max_age: int = 3, **kw) -> "CenterTracker":
        """The reference's nuScenes tracker (pub_tracker.py) over the ten detection classes in the head's task order."""
        label_map = [NUSCENES_TRACKING_NAMES.index(n) if n in NUSCENES_TRACKING_NAMES else -1 for n in NUSCENES_DETECTION_NAMES]
        return cls(label_map, [NUSCENE_CLS_VELOCITY_ERROR[n] for n in NUSCENES_TRACKING_NAMES], max_age=max_age, **kw)

    @classmethod
    def waymo(cls, max_dist: Sequence[float], score_thresh: float = 0.1, max_age: int = 0, **kw) -> "CenterTracker":
        """The reference's Waymo tracker (waymo_tracking/tracker.py): detection label k is WAYMO_TRACKING_NAMES[k]; max_dist per name,
        as a sequence in that order or a dict by name."""
        if isinstance(max_dist, dict):
            max_dist = [max_dist[n] for n in WAYMO_TRACKING_NAMES]
        return cls(list(range(len(max_dist))), max_dist, max_age=max_age, score_thresh=score_thresh, **kw)

    # ---- state -------------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Forget every track and restart the ids of all sequences (PubTracker.reset)."""
        self._host = [(_empty_tracks(), 0) for _ in range(self.num_sequences)]
        self._host_status = np.zeros(self.num_sequences, np.int32)
        if self._state is not None:
            self._state.zero_()

    def _device_state(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            nbytes = int(L.lib().link_track_state_bytes(self.capacity))
            self._state = torch.zeros((self.num_sequences, nbytes), dtype=torch.uint8, device=device)
        return self._state

    def _views(self, state: torch.Tensor) -> Dict[str, torch.Tensor]:
        S, K, o = state.shape[0], self.capacity, L.TRACK_HDR_BYTES
        hdr = state[:, :o].view(torch.int32)
        out = {"n_tracks": hdr[:, 0], "id_count": hdr[:, 1], "status": hdr[:, 2]}
        for name in LIST_FIELDS[:2]:
            out[name] = state[:, o:o + 16 * K].view(torch.float64).view(S, K, 2)
            o += 16 * K
        for name in LIST_FIELDS[2:]:
            out[name] = state[:, o:o + 4 * K].view(torch.int32)
            o += 4 * K
        return out

    def tracks(self, s: int = 0) -> Dict[str, np.ndarray]:
        """A host copy of sequence s's ordered track list (ct, tracking float64 [n, 2]; label, tracking_id, age, active, src int32
        [n]) with id_count and status."""
        if self._state is None:
            t, idc = self._host[s]
            return {**{k: v.copy() for k, v in t.items()}, "id_count": int(idc), "status": int(self._host_status[s])}
        v = {k: t[s].cpu().numpy() for k, t in self._views(self._state).items()}
        n = int(v["n_tracks"])
        return {**{k: v[k][:n].copy() for k in LIST_FIELDS}, "id_count": int(v["id_count"]), "status": int(v["status"])}

    # ---- one frame ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, boxes, scores=None, labels=None, time_lag=None, counts=None, reset=None, pose=None) -> Dict[str, torch.Tensor]:
        """boxes float32 [S, N, C] (or [N, C] for one sequence), or a dict with box3d_lidar / scores / label_preds as predict,
        predict_padded and fuse_detections_padded return them; scores [S, N]; labels int32 / int64 [S, N], -1 an unused slot;
        time_lag, reset, pose: Python values (uploaded) or device tensors (float64 [S], uint8 [S], float64 [S, 12]).
        -> det_tracking_id, det_active int32 [S, N] (or [N]), and the track lists of all sequences as views of the state: n_tracks,
        id_count, status int32 [S]; ct, tracking float64 [S, capacity, 2]; label, tracking_id, age, active, src int32 [S, capacity].
        The views are overwritten by the next step."""
        if isinstance(boxes, dict):
            d = boxes
            boxes, scores, labels = d["box3d_lidar"], d["scores"], d["label_preds"]
            c = d.get("counts", d.get("count"))
            if counts is None and c is not None and c.numel() == self.num_sequences:     # predict_padded's per-task counts: the -1 labels do it
                counts = c.reshape(-1)
        if time_lag is None:
            raise ValueError("CenterTracker.step: time_lag is required")
        single = boxes.dim() == 2
        if single:
            boxes, scores, labels = boxes[None], scores[None], labels[None]
        S, N, C = boxes.shape
        if S != self.num_sequences:
            raise ValueError(f"CenterTracker.step: {S} rows for {self.num_sequences} sequences")
        if N > self.capacity:
            raise ValueError(f"CenterTracker.step: {N} detection slots exceed the capacity {self.capacity}")
        if N and C < 6:
            raise ValueError("CenterTracker.step: boxes need a centre, a velocity and a heading (at least 6 columns)")
        if scores.shape != (S, N) or labels.shape != (S, N):
            raise ValueError("CenterTracker.step: scores and labels are [S, N]")
        if boxes.is_cuda and S > 0:
            out = self._step_device(boxes, scores, labels, time_lag, counts, reset, pose)
        else:
            out = self._step_host(boxes, scores, labels, time_lag, counts, reset, pose)
        if single:
            out["det_tracking_id"], out["det_active"] = out["det_tracking_id"][0], out["det_active"][0]
        return out

    def _step_device(self, boxes, scores, labels, time_lag, counts, reset, pose):
        dev = boxes.device
        S, N, C = boxes.shape
        state = self._device_state(dev)
        boxes, scores = boxes.contiguous().float(), scores.contiguous().float()
        if labels.dtype not in (torch.int32, torch.int64):
            labels = labels.long()
        labels = labels.contiguous()

        def up(v, dtype, shape, prep=None):
            if v is None:
                return None
            if not torch.is_tensor(v):
                v = torch.as_tensor(np.asarray(prep(v) if prep else v), dtype=dtype)
                if v.dim() == 0:
                    v = v.expand(S)
            v = v.to(device=dev, dtype=dtype).reshape(shape).contiguous()
            return v
        lag = up(time_lag, torch.float64, (S,))
        rst = up(reset, torch.uint8, (S,))
        cnt = up(counts, torch.int32, (S,))
        pos = up(pose, torch.float64, (S, 12), lambda p: _pose_rows(p, S))
        det_id = torch.empty((S, N), dtype=torch.int32, device=dev)
        det_active = torch.empty((S, N), dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        with torch.cuda.device(dev):
            L.check(L.lib().link_track_step(ctypes.byref(self.cfg), S, N, C, ptr(boxes), ptr(scores), ptr(labels),
                                            1 if labels.dtype == torch.int64 else 0, ptr(cnt), ptr(lag), ptr(rst), ptr(pos),
                                            state.data_ptr(), ptr(det_id), ptr(det_active), L.current_stream_handle()),
                    "link_track_step")
        return {"det_tracking_id": det_id, "det_active": det_active, **self._views(state)}

    def _step_host(self, boxes, scores, labels, time_lag, counts, reset, pose):
        S, N, C = boxes.shape
        K = self.capacity
        to_np = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        b, sc, lab = to_np(boxes).astype(np.float32), to_np(scores).astype(np.float32), to_np(labels)
        lag = np.broadcast_to(to_np(time_lag).astype(np.float64), (S,))
        rst = np.zeros(S, bool) if reset is None else np.broadcast_to(to_np(reset).astype(bool), (S,))
        cnt = None if counts is None else to_np(counts).reshape(S)
        pos = None if pose is None else (to_np(pose).astype(np.float64).reshape(S, 12) if torch.is_tensor(pose) else _pose_rows(pose, S))
        out = {"det_tracking_id": np.full((S, N), -1, np.int32), "det_active": np.zeros((S, N), np.int32),
               "n_tracks": np.zeros(S, np.int32), "id_count": np.zeros(S, np.int32), "status": np.zeros(S, np.int32),
               "ct": np.zeros((S, K, 2), np.float64), "tracking": np.zeros((S, K, 2), np.float64),
               **{k: np.zeros((S, K), np.int32) for k in LIST_FIELDS[2:]}}
        for s in range(S):
            old, idc = (_empty_tracks(), 0) if rst[s] else self._host[s]
            new, idc, did, dact, over = _host_step(self._host_cfg, old, idc, b[s], sc[s], lab[s], None if cnt is None else cnt[s], lag[s],
                                                   None if pos is None else pos[s])
            self._host[s] = (new, idc)
            self._host_status[s] = L.TRACK_STATUS_OVERFLOW if over else 0
            n = new["label"].shape[0]
            out["det_tracking_id"][s], out["det_active"][s] = did, dact
            out["n_tracks"][s], out["id_count"][s], out["status"][s] = n, idc, self._host_status[s]
            for k in LIST_FIELDS:
                out[k][s, :n] = new[k]
        return {k: torch.from_numpy(v) for k, v in out.items()}


def boxes_to_global(boxes: torch.Tensor, pose) -> torch.Tensor:
    """boxes [..., N, C] in the lidar frame (centre in columns 0..2, velocity in columns C - 3 and C - 2 when C >= 9, heading last)
    -> float64 boxes in the global frame of pose (float64 [..., 12] or [..., 3, 4] / [..., 4, 4], row-major lidar-to-global, one
    per leading index): centre = ((r0 x + r1 y) + r2 z) + t per row, velocity = R (vx, vy, 0) (x and y kept), heading + the pose's
    yaw atan2(r10, r00); the other columns are copied.  A torch composition in float64 on the boxes' device; every product and sum
    is rounded on its own, which is the arithmetic link_track_step uses for the centre and the velocity."""
    b = boxes.double()
    p = pose.to(device=b.device, dtype=torch.float64) if torch.is_tensor(pose) else torch.as_tensor(np.asarray(pose, np.float64), device=b.device)
    p = p.reshape(*b.shape[:-2], -1, 4)[..., :3, :].unsqueeze(-3)          # [..., 1, 3, 4]: one transform per leading index
    r = lambda i, j: p[..., i, j]
    x, y, z = b[..., 0], b[..., 1], b[..., 2]
    out = b.clone()
    for i in range(3):
        out[..., i] = ((r(i, 0) * x + r(i, 1) * y) + r(i, 2) * z) + r(i, 3)
    C = b.shape[-1]
    if C >= 9:
        vx, vy = b[..., C - 3], b[..., C - 2]
        out[..., C - 3] = r(0, 0) * vx + r(0, 1) * vy
        out[..., C - 2] = r(1, 0) * vx + r(1, 1) * vy
    out[..., C - 1] = b[..., C - 1] + torch.atan2(r(1, 0), r(0, 0))
    return out
