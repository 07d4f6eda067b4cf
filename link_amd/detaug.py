"""link_amd/detaug.py -- the detection training front end on the device (csrc/detaug.hip, section P of include/link_amd.h): the
geometry behind the names of the reference's det3d.core.bbox.box_np_ops and det3d.core.sampler.preprocess, and DetTrainAugmenter,
which is datasets/pipelines/preprocess.py::Preprocess (train mode) plus the box filter of Voxelization for a whole batch.

points_in_rbbox / points_count_rbbox are box_np_ops.py:641-647 and :15-20 (eight corners, six surfaces, a numba loop over every
point, box and surface) as one launch that tests in the box frame; the batched forms take the packed points of several frames with
their offsets and one set of boxes per frame, which is what the minimum-points filter of the training pipeline
(datasets/pipelines/preprocess.py::Preprocess) needs for a whole batch.  center_to_corner_box2d and box_collision_test are
box_np_ops.py:265-285 and sampler/preprocess.py:854-937: the acceptance test of the ground-truth sampler.  Everything runs on the
current stream, allocates only its result and reads nothing back.

DetTrainAugmenter takes the frames' points and annotations as they are loaded and returns what Voxelizer.generate_padded and
CenterTargetAssigner take: four launches (counts, sampler scan, points, boxes), no host geometry, and in the padded form no host
round trip.  Random numbers are arguments -- a [B, 7] tensor of draws, a permutation per frame, and the candidate lists that
DatabaseSampler.draw() produces on the host (which objects to offer is control plane; whether they fit is decided on the device).
Group sampling, random_crop, road planes and a per-object rotation range (noise_per_object_v3_) are refused.
"""
from __future__ import annotations

import ctypes
import sys
import types
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L


def _gpu_f32(t, what: str, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.LinkAmdError(f"{what}: link_amd runs on the GPU only ({name} is a CPU tensor or an array); there is no CPU fallback")
    return t.contiguous().float()


def _points_boxes(points, rbbox, point_offsets, z_axis, origin, what):
    if int(z_axis) != 2 or tuple(float(o) for o in origin) != (0.5, 0.5, 0.5):
        raise ValueError(f"{what}: only z_axis = 2 with origin (0.5, 0.5, 0.5), the lidar boxes of the training pipeline, is built")
    pts, boxes = _gpu_f32(points, what, "points"), _gpu_f32(rbbox, what, "rbbox")
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError(f"{what}: points are [P, >= 3], got {tuple(pts.shape)}")
    if boxes.shape[-1] < 7:
        raise ValueError(f"{what}: boxes hold at least 7 columns (centre, extents, .., heading last), got {tuple(boxes.shape)}")
    if point_offsets is None:
        if boxes.dim() != 2:
            raise ValueError(f"{what}: boxes are [N, L] without point_offsets, got {tuple(boxes.shape)}")
        return pts, boxes, None, 1
    if not isinstance(point_offsets, torch.Tensor) or not point_offsets.is_cuda:
        raise L.LinkAmdError(f"{what}: point_offsets lives on the GPU (int32 [B + 1]); there is no CPU fallback")
    if point_offsets.dtype != torch.int32 or point_offsets.dim() != 1:
        raise ValueError(f"{what}: point_offsets is int32 [B + 1]")
    batch = int(point_offsets.shape[0]) - 1
    if boxes.dim() != 3 or boxes.shape[0] != batch or batch < 1:
        raise ValueError(f"{what}: with point_offsets [B + 1] the boxes are [B, N, L]; got {tuple(boxes.shape)} for B = {batch}")
    return pts, boxes, point_offsets.contiguous(), batch


def _launch(pts, boxes, offs, batch, mask, counts):
    if counts is not None and pts.shape[0] == 0:
        counts.zero_()
    if pts.shape[0] == 0 or boxes.shape[-2] == 0:                # nothing to test: an empty tensor has no address to hand over
        return
    with torch.cuda.device(pts.device):
        L.check(L.lib().link_points_in_rbbox(pts.data_ptr(), pts.shape[1], offs.data_ptr() if offs is not None else None, batch,
                                             pts.shape[0], boxes.data_ptr(), boxes.shape[-2], boxes.shape[-1],
                                             mask.data_ptr() if mask is not None else None,
                                             counts.data_ptr() if counts is not None else None, L.current_stream_handle()),
                "link_points_in_rbbox")


@torch.no_grad()
def points_in_rbbox(points: torch.Tensor, rbbox: torch.Tensor, z_axis: int = 2, origin=(0.5, 0.5, 0.5),
                    point_offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """box_np_ops.py:641-647 -> bool [P, N]: point p strictly inside box n (a point on a face is outside, as geometry.py:273
    decides; a box with a zero extent holds nothing).  points [P, >= 3], rbbox [N, >= 7] with the heading in the last column.
    Batched: point_offsets int32 [B + 1] on the device and rbbox [B, N, L]; row p is tested against the boxes of p's frame."""
    pts, boxes, offs, batch = _points_boxes(points, rbbox, point_offsets, z_axis, origin, "points_in_rbbox")
    n = boxes.shape[-2]
    mask = (torch.zeros if offs is not None else torch.empty)((pts.shape[0], n), dtype=torch.uint8, device=pts.device)
    _launch(pts, boxes, offs, batch, mask, None)
    return mask.view(torch.bool)


@torch.no_grad()
def points_count_rbbox(points: torch.Tensor, rbbox: torch.Tensor, z_axis: int = 2, origin=(0.5, 0.5, 0.5),
                       point_offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """box_np_ops.py:15-20 -> int32 [N]: the points strictly inside every box; batched (see points_in_rbbox) -> int32 [B, N].
    No mask is formed: one wave reduction and one integer atomic per (wave, box)."""
    pts, boxes, offs, batch = _points_boxes(points, rbbox, point_offsets, z_axis, origin, "points_count_rbbox")
    counts = torch.empty(boxes.shape[:-1], dtype=torch.int32, device=pts.device)
    _launch(pts, boxes, offs, batch, None, counts)
    return counts


@torch.no_grad()
def center_to_corner_box2d(centers: torch.Tensor, dims: torch.Tensor, angles: Optional[torch.Tensor] = None, origin: float = 0.5) -> torch.Tensor:
    """box_np_ops.py:265-285 -> [N, 4, 2]: the corners (-,-), (-,+), (+,+), (+,-) of every BEV box, turned clockwise by a positive
    angle: the order box_collision_test's `clockwise` names."""
    c, d = _gpu_f32(centers, "center_to_corner_box2d", "centers"), _gpu_f32(dims, "center_to_corner_box2d", "dims")
    a = _gpu_f32(angles, "center_to_corner_box2d", "angles").reshape(-1) if angles is not None else None
    n = c.shape[0]
    if c.dim() != 2 or c.shape[1] != 2 or tuple(d.shape) != (n, 2) or (a is not None and a.shape[0] != n):
        raise ValueError("center_to_corner_box2d: centers [N, 2], dims [N, 2], angles [N]")
    out = torch.empty((n, 4, 2), dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        L.check(L.lib().link_box2d_corners(c.data_ptr(), d.data_ptr(), a.data_ptr() if a is not None else None, n, float(origin),
                                           out.data_ptr(), L.current_stream_handle()), "link_box2d_corners")
    return out


@torch.no_grad()
def box_collision_test(boxes: torch.Tensor, qboxes: torch.Tensor, clockwise: bool = True) -> torch.Tensor:
    """sampler/preprocess.py:854-937 -> bool [N, K]: corners [N, 4, 2] against corners [K, 4, 2] (center_to_corner_box2d's order).
    Bounds that only touch, and boxes that share an edge without crossing, do not collide; a box wholly inside another does."""
    a, b = _gpu_f32(boxes, "box_collision_test", "boxes"), _gpu_f32(qboxes, "box_collision_test", "qboxes")
    if a.dim() != 3 or tuple(a.shape[1:]) != (4, 2) or b.dim() != 3 or tuple(b.shape[1:]) != (4, 2):
        raise ValueError(f"box_collision_test: corners are [N, 4, 2] and [K, 4, 2], got {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        L.check(L.lib().link_box_collision(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], 1 if clockwise else 0, out.data_ptr(),
                                           L.current_stream_handle()), "link_box_collision")
    return out.view(torch.bool)


class GTDatabase:
    """The ground-truth database on the device, built once from host arrays: `points` float32 [sum P, F], the objects' points
    packed in order and centred on their boxes (what the reference reads with one np.fromfile per pasted object); `offsets` int64
    [D + 1]; `boxes` float32 [D, 7 | 9] (box3d_lidar); `classes` int32 [D], the 1-based index of every object's name in the
    detector's class list.  by_class[c] lists the objects of class c in database order: the lists DatabaseSampler shuffles.

    Everything stays resident: 4 F bytes per point.  Its size at nuScenes scale has not been measured here."""

    def __init__(self, points, offsets, boxes, classes, device="cuda"):
        points = np.ascontiguousarray(points, dtype=np.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        boxes = np.ascontiguousarray(boxes, dtype=np.float32)
        classes = np.ascontiguousarray(classes, dtype=np.int32)
        d = boxes.shape[0]
        if points.ndim != 2 or points.shape[1] < 3 or boxes.ndim != 2 or boxes.shape[1] not in (7, 9):
            raise ValueError(f"GTDatabase: points are [sum P, F >= 3] and boxes [D, 7 | 9], got {points.shape} and {boxes.shape}")
        if offsets.shape != (d + 1,) or classes.shape != (d,):
            raise ValueError(f"GTDatabase: offsets are [D + 1] and classes [D] for D = {d}, got {offsets.shape} and {classes.shape}")
        if d >= 2 ** 31 or offsets[0] != 0 or offsets[-1] != points.shape[0] or (np.diff(offsets) < 0).any():
            raise ValueError("GTDatabase: offsets must rise from 0 to the number of points")
        if d and classes.min() < 1:
            raise ValueError("GTDatabase: classes are 1-based indices into the class list")
        self.size, self.point_dim, self.box_len = d, int(points.shape[1]), int(boxes.shape[1])
        self.by_class: Dict[int, np.ndarray] = {int(c): np.flatnonzero(classes == c).astype(np.int32) for c in np.unique(classes)}
        self.num_points = np.diff(offsets)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.LinkAmdError("GTDatabase: link_amd runs on the GPU only; there is no CPU fallback")
        self.points, self.offsets = torch.from_numpy(points).to(dev), torch.from_numpy(offsets).to(dev)
        self.boxes, self.classes = torch.from_numpy(boxes).to(dev), torch.from_numpy(classes).to(dev)


class DatabaseSampler:
    """The host half of the ground-truth sampler: which database objects to offer.  One shuffled index stream per class with
    BatchSampler's wrap rule (core/sampler/preprocess.py:19-53): draw(c, num) hands out the next num entries, or, when they reach
    or pass the end, what is left (possibly fewer, possibly none) followed by a reshuffle.  `lists` maps a class to its database
    indices (GTDatabase.by_class); `rng` is a np.random.RandomState (the reference uses the global one: seeded alike and asked in
    the same order, the streams are equal).

    The reference asks for exactly the number the frame lacks, which here is known on the device only; candidates() asks for
    every group's target number instead and the kernel takes the head it needs, so the stream moves faster than the reference's."""

    def __init__(self, lists: Dict[int, Sequence[int]], rng: Optional[np.random.RandomState] = None):
        self._rng = rng if rng is not None else np.random.RandomState()
        self._lists, self._indices, self._idx = {}, {}, {}
        for c, ids in lists.items():
            self._lists[c] = np.asarray(ids, dtype=np.int32)
            self._indices[c] = np.arange(len(ids))
            self._rng.shuffle(self._indices[c])
            self._idx[c] = 0

    def draw(self, c: int, num: int) -> np.ndarray:
        """int32 database indices, BatchSampler.sample(num) for class c"""
        ind, i, n = self._indices[c], self._idx[c], len(self._indices[c])
        if i + num >= n:
            ret = ind[i:].copy()
            self._rng.shuffle(ind)
            self._idx[c] = 0
        else:
            ret = ind[i:i + num]
            self._idx[c] = i + num
        return self._lists[c][ret]

    def candidates(self, batch: int, group_classes: Sequence[int], group_max: Sequence[int], max_candidates: int):
        """(int32 [batch, n_groups, max_candidates], int32 [batch, n_groups]) host arrays for DetTrainAugmenter: per frame and group
        one draw of the group's target number (a class the database lacks gets an empty list)"""
        cand = np.full((batch, len(group_classes), max_candidates), -1, np.int32)
        lens = np.zeros((batch, len(group_classes)), np.int32)
        for b in range(batch):
            for q, (c, m) in enumerate(zip(group_classes, group_max)):
                if c in self._lists and len(self._lists[c]):
                    got = self.draw(c, min(int(m), max_candidates))
                    cand[b, q, :len(got)], lens[b, q] = got, len(got)
        return cand, lens


class DetTrainAugmenter:
    """Preprocess in train mode (datasets/pipelines/preprocess.py:51-167) and the box filter of Voxelization (:193-197) for a batch,
    on the device.  class_names: the detector's classes (a ground-truth class k >= 1 is class_names[k - 1]); sample_groups: the
    db_sampler's list of {name: target number} dicts, one name each; rate: db_sampler.rate; global_rot_noise / global_scale_noise:
    [low, high]; global_translate_std: a number or three; min_points_in_gt; pc_range: the voxeliser's range (x, y of it filter the
    boxes); max_objs: rows of the box output (CenterTargetAssigner's max_objs); point_capacity: rows of the point output per frame.
    Limits: max_objs_in + 64-at-most candidates per group over all groups <= 1024 per frame (ValueError above).

    padded(...) -> dict with fixed shapes and no host round trip: points [B, cap, F] (rows past a frame's total are NaN, in
    shuffled places: Voxelizer's range test drops them), gt_boxes [B, max_objs, L], gt_classes int32 [B, max_objs] (0 = empty),
    num_points / num_boxes / status int32 [B], accepted int32 [B, A] (-1 = unused) with num_accepted.  __call__ -> the same
    trimmed: lists of [n_b, F] points, [m_b, L] boxes and [m_b] classes; one read-back of the totals."""

    def __init__(self, class_names: Sequence[str], sample_groups: Sequence[Dict[str, int]], rate: float, global_rot_noise,
                 global_scale_noise, global_translate_std, min_points_in_gt: int, pc_range, max_objs: int, point_capacity: int,
                 flip_probability: float = 0.5, database: Optional[GTDatabase] = None, max_candidates: Optional[int] = None,
                 global_random_rotation_range_per_object=(0, 0), random_crop: bool = False, road_planes=None):
        rr = global_random_rotation_range_per_object
        rr = [-rr, rr] if not isinstance(rr, (list, tuple, np.ndarray)) else list(rr)
        if abs(rr[0] - rr[1]) >= 1e-3:
            raise NotImplementedError("DetTrainAugmenter: global_random_rotation_range_per_object (noise_per_object_v3_) is not built; "
                                      "the ELKv3 configs set it to [0, 0]")
        if random_crop:
            raise NotImplementedError("DetTrainAugmenter: random_crop (frustum cropping of the pasted objects) is not built")
        if road_planes is not None:
            raise NotImplementedError("DetTrainAugmenter: road planes are not built")
        self.class_names = list(class_names)
        self.group_classes, self.group_max = [], []
        for g in sample_groups or []:
            if len(g) != 1:
                raise NotImplementedError("DetTrainAugmenter: group sampling (a sample group of several names) is not built")
            (name, num), = g.items()
            if name not in self.class_names:
                raise ValueError(f"DetTrainAugmenter: sample group {name!r} is not one of class_names")
            self.group_classes.append(self.class_names.index(name) + 1)
            self.group_max.append(int(num))
        if len(self.group_classes) > L.DETAUG_MAX_GROUPS:
            raise ValueError(f"DetTrainAugmenter: at most {L.DETAUG_MAX_GROUPS} sample groups")
        if self.group_classes and database is None:
            raise ValueError("DetTrainAugmenter: sample_groups need a GTDatabase")
        self.database = database if self.group_classes else None
        self.max_candidates = int(max_candidates if max_candidates is not None else max(self.group_max, default=0)) if self.group_classes else 0
        if self.max_candidates > L.DETAUG_MAX_CANDIDATES:
            raise ValueError(f"DetTrainAugmenter: at most {L.DETAUG_MAX_CANDIDATES} candidates per group and frame")
        self.max_accept = len(self.group_classes) * self.max_candidates
        rot = global_rot_noise if isinstance(global_rot_noise, (list, tuple, np.ndarray)) else [-global_rot_noise, global_rot_noise]
        std = global_translate_std
        std = [std] * 3 if not isinstance(std, (list, tuple, np.ndarray)) else list(std)
        if len(rot) != 2 or len(global_scale_noise) != 2 or len(std) != 3 or len(pc_range) != 6:
            raise ValueError("DetTrainAugmenter: global_rot_noise and global_scale_noise are [low, high], global_translate_std a number "
                             "or three, pc_range six numbers")
        if not 0.0 <= float(flip_probability) <= 1.0 or float(rate) < 0 or int(max_objs) < 1 or int(point_capacity) < 1:
            raise ValueError("DetTrainAugmenter: flip_probability in [0, 1], rate >= 0, max_objs and point_capacity >= 1")
        self.rate, self.min_points, self.max_objs, self.point_capacity = float(rate), int(min_points_in_gt), int(max_objs), int(point_capacity)
        t = self._tcfg = L.LinkDetaugTransformCfg()
        t.rot_lo, t.rot_hi, t.scale_lo, t.scale_hi = float(rot[0]), float(rot[1]), float(global_scale_noise[0]), float(global_scale_noise[1])
        for d in range(3):
            t.translate_std[d] = float(std[d])
        t.flip_probability = float(flip_probability)
        t.range[0], t.range[1], t.range[2], t.range[3] = (float(np.float32(pc_range[i])) for i in (0, 1, 3, 4))      # VoxelGenerator keeps an fp32 range
        t.max_objs, t.point_capacity = self.max_objs, self.point_capacity
        self._ws = {}

    def _workspace(self, device, batch: int, max_gt: int, box_len: int):
        """accepted, paste_start, n_accept, merged boxes / classes / count: owned by this object, one set per (device, shape)"""
        key = (device, batch, max_gt, box_len)
        ws = self._ws.get(key)
        if ws is None:
            a, t = self.max_accept, max_gt + self.max_accept
            i32 = dict(dtype=torch.int32, device=device)
            ws = self._ws[key] = dict(accepted=torch.full((batch, max(a, 1)), -1, **i32), paste_start=torch.zeros((batch, a + 1), **i32),
                                      n_accept=torch.zeros(batch, **i32), merged_boxes=torch.zeros((batch, max(t, 1), box_len), device=device),
                                      merged_classes=torch.zeros((batch, max(t, 1)), **i32), n_merged=torch.zeros(batch, **i32))
        return ws

    @torch.no_grad()
    def padded(self, points: torch.Tensor, point_offsets: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
               draws: torch.Tensor, perm: torch.Tensor, candidates: Optional[torch.Tensor] = None,
               candidate_lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """points float32 [P, F] (all frames packed) with point_offsets int32 [B + 1]; gt_boxes float32 [B, G, 7 | 9]; gt_classes int32
        [B, G] (0 = empty or DontCare, k >= 1 = class_names[k - 1], negative = a name outside class_names); draws float32 [B, 7];
        perm int32 [B, point_capacity]; candidates int32 [B, n_groups, max_candidates] and candidate_lengths int32 [B, n_groups]
        (DatabaseSampler.candidates, moved to the device).  Everything on the GPU; nothing is read back."""
        what = "DetTrainAugmenter"
        for name, t in (("points", points), ("point_offsets", point_offsets), ("gt_boxes", gt_boxes), ("gt_classes", gt_classes),
                        ("draws", draws), ("perm", perm)) + ((("candidates", candidates), ("candidate_lengths", candidate_lengths))
                                                             if self.group_classes else ()):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise L.LinkAmdError(f"{what}: link_amd runs on the GPU only ({name} is a CPU tensor or an array); there is no CPU fallback")
        batch = int(point_offsets.shape[0]) - 1
        if points.dim() != 2 or points.shape[1] < 3 or points.dtype != torch.float32:
            raise ValueError(f"{what}: points are float32 [P, F >= 3]")
        if gt_boxes.dim() != 3 or gt_boxes.shape[0] != batch or gt_boxes.shape[2] not in (7, 9) or gt_boxes.dtype != torch.float32:
            raise ValueError(f"{what}: gt_boxes are float32 [B, G, 7 | 9] for B = {batch}, got {tuple(gt_boxes.shape)}")
        max_gt, box_len, ndim = int(gt_boxes.shape[1]), int(gt_boxes.shape[2]), int(points.shape[1])
        if max_gt + self.max_accept > L.DETAUG_MAX_BOXES:
            raise ValueError(f"{what}: {max_gt} ground-truth rows + {self.max_accept} candidates per frame exceed {L.DETAUG_MAX_BOXES}")
        for name, t, shape in (("point_offsets", point_offsets, (batch + 1,)), ("gt_classes", gt_classes, (batch, max_gt)),
                               ("perm", perm, (batch, self.point_capacity))):
            if t.dtype != torch.int32 or tuple(t.shape) != shape:
                raise ValueError(f"{what}: {name} is int32 {list(shape)}, got {t.dtype} {list(t.shape)}")
        if draws.dtype != torch.float32 or tuple(draws.shape) != (batch, 7):
            raise ValueError(f"{what}: draws are float32 [B, 7]")
        db = self.database
        if self.group_classes:
            shape = (batch, len(self.group_classes), self.max_candidates)
            if candidates.dtype != torch.int32 or tuple(candidates.shape) != shape or candidate_lengths.dtype != torch.int32 or \
                    tuple(candidate_lengths.shape) != shape[:2]:
                raise ValueError(f"{what}: candidates are int32 {list(shape)} with lengths int32 {list(shape[:2])}")
            if db.box_len != box_len or db.point_dim != ndim:
                raise ValueError(f"{what}: the database holds {db.point_dim}-feature points and {db.box_len}-column boxes, the frames {ndim} and {box_len}")
        points, gt_boxes, gt_classes, draws, perm = (t.contiguous() for t in (points, gt_boxes, gt_classes, draws, perm))
        point_offsets = point_offsets.contiguous()
        device = points.device
        ws = self._workspace(device, batch, max_gt, box_len)
        i32 = dict(dtype=torch.int32, device=device)
        out = dict(points=torch.empty((batch, self.point_capacity, ndim), device=device),
                   gt_boxes=torch.empty((batch, self.max_objs, box_len), device=device), gt_classes=torch.empty((batch, self.max_objs), **i32),
                   num_points=torch.empty(batch, **i32), num_boxes=torch.empty(batch, **i32), status=torch.empty(batch, **i32))
        s = L.LinkDetaugSampleCfg()
        s.rate, s.n_groups, s.max_candidates, s.max_gt, s.min_points, s.box_len = self.rate, len(self.group_classes), self.max_candidates, max_gt, self.min_points, box_len
        for q, (c, m) in enumerate(zip(self.group_classes, self.group_max)):
            s.group_class[q], s.group_max[q] = c, m
        ptr = lambda t: t.data_ptr() if t is not None else None                                       # noqa: E731
        lib = L.lib()
        with torch.cuda.device(device):
            stream = L.current_stream_handle()
            counts = None
            if self.min_points > 0 and max_gt > 0:
                counts = torch.empty((batch, max_gt), **i32)
                L.check(lib.link_points_in_rbbox(points.data_ptr(), ndim, point_offsets.data_ptr(), batch, points.shape[0], gt_boxes.data_ptr(),
                                                 max_gt, box_len, None, counts.data_ptr(), stream), "link_points_in_rbbox")
            L.check(lib.link_detaug_sample(ctypes.byref(s), batch, gt_boxes.data_ptr(), gt_classes.data_ptr(), ptr(counts), ptr(candidates),
                                           ptr(candidate_lengths), ptr(db.boxes if db else None), ptr(db.classes if db else None),
                                           ptr(db.offsets if db else None), db.size if db else 0, ws["accepted"].data_ptr(),
                                           ws["paste_start"].data_ptr(), ws["n_accept"].data_ptr(), ws["merged_boxes"].data_ptr(),
                                           ws["merged_classes"].data_ptr(), ws["n_merged"].data_ptr(), out["status"].data_ptr(), stream),
                    "link_detaug_sample")
            L.check(lib.link_detaug_transform(ctypes.byref(self._tcfg), batch, draws.data_ptr(), points.data_ptr(), point_offsets.data_ptr(),
                                              points.shape[0], ndim, ptr(db.points if db else None), ptr(db.offsets if db else None),
                                              ptr(db.boxes if db else None), box_len, ws["accepted"].data_ptr(), ws["paste_start"].data_ptr(),
                                              ws["n_accept"].data_ptr(), self.max_accept, perm.data_ptr(), out["points"].data_ptr(),
                                              ws["merged_boxes"].data_ptr(), ws["merged_classes"].data_ptr(), ws["n_merged"].data_ptr(),
                                              max_gt + self.max_accept, out["gt_boxes"].data_ptr(), out["gt_classes"].data_ptr(),
                                              out["num_boxes"].data_ptr(), out["num_points"].data_ptr(), out["status"].data_ptr(), stream),
                    "link_detaug_transform")
        out["accepted"], out["num_accepted"] = ws["accepted"][:, :self.max_accept], ws["n_accept"]
        return out

    @torch.no_grad()
    def __call__(self, points: Sequence[torch.Tensor], gt_boxes: Sequence[torch.Tensor], gt_classes: Sequence[torch.Tensor],
                 draws: torch.Tensor, perm: torch.Tensor, candidates=None, candidate_lengths=None):
        """Variable length: points a list of [n_b, F] GPU tensors, gt_boxes / gt_classes lists of [g_b, L] / [g_b]; candidates and
        their lengths may be DatabaseSampler.candidates' host arrays.  -> dict(points, gt_boxes, gt_classes: lists per frame;
        accepted: list of int32 tensors; status int32 [B] on the host).  One read-back: the totals."""
        for c in points:
            if not isinstance(c, torch.Tensor) or not c.is_cuda:
                raise L.LinkAmdError("DetTrainAugmenter: link_amd runs on the GPU only (got a CPU tensor or an array); there is no CPU fallback")
        device, batch = points[0].device, len(points)
        box_len = next((int(g.shape[1]) for g in gt_boxes if g.dim() == 2), 9)
        max_gt = max(max((int(g.shape[0]) for g in gt_boxes), default=0), 1)
        gb = torch.zeros((batch, max_gt, box_len), device=device)
        gc = torch.zeros((batch, max_gt), dtype=torch.int32, device=device)
        for b in range(batch):
            n = int(gt_boxes[b].shape[0])
            if n:
                gb[b, :n], gc[b, :n] = gt_boxes[b].to(device).float(), gt_classes[b].to(device).int()
        offs = torch.tensor(np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in points])]), dtype=torch.int32).to(device)
        if candidates is not None and not isinstance(candidates, torch.Tensor):
            candidates, candidate_lengths = torch.from_numpy(np.ascontiguousarray(candidates)).to(device), torch.from_numpy(np.ascontiguousarray(candidate_lengths)).to(device)
        out = self.padded(torch.cat(list(points)).float(), offs, gb, gc, draws, perm, candidates, candidate_lengths)
        totals = torch.stack([out["num_points"], out["num_boxes"], out["num_accepted"], out["status"]]).cpu().numpy()      # the one round trip
        res = dict(points=[], gt_boxes=[], gt_classes=[], accepted=[], status=totals[3])
        # the rows that are not NaN, in place order: a stable sort of the flag instead of a boolean index (which would read back)
        order = torch.sort(torch.isnan(out["points"][:, :, 0]).to(torch.uint8), dim=1, stable=True)[1]
        for b in range(batch):
            res["points"].append(out["points"][b][order[b, :int(totals[0, b])]])
            res["gt_boxes"].append(out["gt_boxes"][b, :int(totals[1, b])])
            res["gt_classes"].append(out["gt_classes"][b, :int(totals[1, b])])
            res["accepted"].append(out["accepted"][b, :int(totals[2, b])])
        return res


box_np_ops = types.ModuleType("det3d.core.bbox.box_np_ops")
box_np_ops.points_in_rbbox, box_np_ops.points_count_rbbox = points_in_rbbox, points_count_rbbox
box_np_ops.center_to_corner_box2d = center_to_corner_box2d
sampler_preprocess = types.ModuleType("det3d.core.sampler.preprocess")
sampler_preprocess.box_collision_test = box_collision_test


def install_as_box_np_ops() -> None:
    """Register the functions above under the names det3d imports them by: det3d.core.bbox.box_np_ops and
    det3d.core.sampler.preprocess (tensors on the GPU in place of arrays).  Modules that are already imported (a real det3d
    checkout) keep everything else they hold and get these names replaced; missing parents are created empty."""
    for full, ours in (("det3d.core.bbox.box_np_ops", box_np_ops), ("det3d.core.sampler.preprocess", sampler_preprocess)):
        parent = None
        parts = full.split(".")
        for i in range(1, len(parts)):
            name = ".".join(parts[:i])
            mod = sys.modules.get(name)
            if mod is None:
                mod = types.ModuleType(name)
                mod.__path__ = []
                sys.modules[name] = mod
            if parent is not None:
                setattr(parent, parts[i - 1], mod)
            parent = mod
        have = sys.modules.get(full)
        if have is None or have is ours:
            sys.modules[full] = ours
            setattr(parent, parts[-1], ours)
        else:
            for k, v in vars(ours).items():
                if callable(v):
                    setattr(have, k, v)
