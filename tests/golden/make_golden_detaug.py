"""Record tests/golden/detaug_*.npz from the reference's own training front end.  Run by hand; the tests do not run it.

    python tests/golden/make_golden_detaug.py /path/to/LinK

The expected values come from the reference's modules loaded BY PATH under bare parent packages: det3d/core/bbox/geometry.py and
box_np_ops.py (points_in_rbbox, points_count_rbbox, center_to_corner_box2d), det3d/core/sampler/preprocess.py (box_collision_test,
the global transforms, filter_gt_box_outside_range), det3d/core/sampler/sample_ops.py (DataBaseSamplerV2) and
det3d/datasets/pipelines/preprocess.py (Preprocess).  Stand-ins: a module named `numba` whose decorators return the function;
np.random's choice / uniform / normal / shuffle return the recorded draws while Preprocess runs; every BatchSampler's `sample`
returns the head of the recorded candidate list; np.fromfile reads the in-memory database.  One more stand-in is needed because the
loops run as plain Python: box_collision_test writes `ret[i, j] is True`, which numba decides by value and Python by identity (a
numpy bool is never `True`), so while it runs np.zeros(.., dtype=np.bool_) hands out an object array of Python bools -- with it
the function takes the branches the compiled one takes.  Nothing of the reference is copied into the repository.

Stable inputs only.  A point is unstable when its float64 distance to a face plane of any box is below 1e-4 m, or when the
reference's float32 decision differs from the float64 one; a box pair, or a range test, when its float64 decision changes under
centre shifts of +-1e-4 m or extent scalings of 1 +- 1e-5, or differs from the reference's float32 one.  Unstable points and boxes
are drawn again, an unstable frame as a whole; every fixture's meta holds the share drawn again, and this script refuses more
than 5 %.  e_<name> is the distance of the reference's float32 recording from the float64 oracle (tests/aug_oracle.py).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aug_oracle as AO  # noqa: E402

CLASS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
SAMPLE_GROUPS = [dict(car=2), dict(truck=3), dict(construction_vehicle=7), dict(bus=4), dict(trailer=6), dict(barrier=2), dict(motorcycle=6),
                 dict(bicycle=6), dict(pedestrian=2), dict(traffic_cone=2)]
SIZES = {"car": (4.6, 1.9, 1.7), "truck": (6.9, 2.5, 2.8), "construction_vehicle": (6.4, 2.8, 3.2), "bus": (11.0, 2.9, 3.5),
         "trailer": (12.3, 2.9, 3.9), "barrier": (0.5, 2.5, 1.0), "motorcycle": (2.1, 0.8, 1.5), "bicycle": (1.7, 0.6, 1.3),
         "pedestrian": (0.7, 0.7, 1.8), "traffic_cone": (0.4, 0.4, 1.1)}
PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
ROT, SCALE, STD = [-0.78539816, 0.78539816], [0.9, 1.1], 0.5
MARGIN, DIM_EPS = 1e-4, 1e-5


class Cfg(dict):
    __getattr__ = dict.__getitem__


class Logger:
    def info(self, *a, **k):
        pass


def load_reference(root):
    det = os.path.join(root, "detection")
    for name in ("det3d", "det3d.core", "det3d.core.bbox", "det3d.core.sampler", "det3d.core.input", "det3d.core.utils", "det3d.utils",
                 "det3d.datasets", "det3d.datasets.pipelines"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(det, *name.split("."))]
        sys.modules[name] = m
    nb = types.ModuleType("numba")
    passthrough = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))       # noqa: E731
    nb.jit = nb.njit = passthrough
    sys.modules["numba"] = nb

    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class Registry:
        def register_module(self, cls):
            return cls
    stub("det3d.utils.check", shape_mergeable=lambda x, shape: True)
    stub("det3d.builder", build_dbsampler=lambda cfg: cfg["instance"])
    stub("det3d.core.input.voxel_generator", VoxelGenerator=object)
    stub("det3d.core.utils.center_utils", draw_umich_gaussian=None, gaussian_radius=None)
    stub("det3d.datasets.registry", PIPELINES=Registry())

    def by_path(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(det, *parts))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        parent, leaf = name.rsplit(".", 1)
        setattr(sys.modules[parent], leaf, m)
        return m

    by_path("det3d.core.bbox.geometry", "det3d", "core", "bbox", "geometry.py")
    ops = by_path("det3d.core.bbox.box_np_ops", "det3d", "core", "bbox", "box_np_ops.py")
    prep = by_path("det3d.core.sampler.preprocess", "det3d", "core", "sampler", "preprocess.py")
    sops = by_path("det3d.core.sampler.sample_ops", "det3d", "core", "sampler", "sample_ops.py")
    pipe = by_path("det3d.datasets.pipelines.preprocess", "det3d", "datasets", "pipelines", "preprocess.py")
    return ops, prep, sops, pipe


class PythonBools:
    """np.zeros(.., dtype=np.bool_) -> an object array of Python bools while box_collision_test runs (see the module docstring)"""

    def __enter__(self):
        self.zeros = np.zeros

        def zeros(shape, dtype=float, **k):
            if dtype is np.bool_:
                out = np.empty(shape, dtype=object)
                out[...] = False
                return out
            return self.zeros(shape, dtype=dtype, **k)
        np.zeros = zeros

    def __exit__(self, *a):
        np.zeros = self.zeros


def ref_collision(prep, a, b):
    with PythonBools():
        out = prep.box_collision_test(a, b)
    return np.asarray(out, dtype=bool)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def draw_boxes(rng, n, length=9, spread=50.0):
    b = np.zeros((n, length), np.float32)
    b[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    b[:, 2] = rng.uniform(-2.0, 1.0, n)
    b[:, 3:6] = np.exp(rng.uniform(np.log(0.4), np.log(12.0), (n, 3)))
    if length == 9:
        b[:, 6:8] = rng.normal(0, 3.0, (n, 2))
    b[:, -1] = rng.uniform(-np.pi, np.pi, n)
    return b


def draw_points(rng, n, boxes, ndim):
    """half of the points in and around the boxes (box-frame coordinates within +-0.7 extents: many lie near a face), half anywhere"""
    p = np.zeros((n, ndim), np.float32)
    p[:, :3] = rng.uniform([-55, -55, -4], [55, 55, 3], (n, 3))
    if len(boxes):
        near = rng.random(n) < 0.5
        which = rng.integers(0, len(boxes), n)
        local = rng.uniform(-0.7, 0.7, (n, 3)) * boxes[which, 3:6]
        a = boxes[which, -1].astype(np.float64)
        x = local[:, 0] * np.cos(a) + local[:, 1] * np.sin(a)
        y = -local[:, 0] * np.sin(a) + local[:, 1] * np.cos(a)
        w = np.stack([x, y, local[:, 2]], 1) + boxes[which, :3]
        p[near, :3] = w[near]
    p[:, 3:] = rng.random((n, ndim - 3))
    return p


def stable_points(ops, rng, n, boxes, ndim):
    """points whose reference decision is safe against every box; -> (points, reference mask, share drawn again)"""
    pts = draw_points(rng, n, boxes, ndim)
    again = 0
    for _ in range(20):
        if len(boxes) == 0 or n == 0:
            return pts, np.zeros((n, len(boxes)), bool), 0.0
        ref = np.asarray(ops.points_in_rbbox(pts, boxes), bool)
        bad = (AO.face_distance(pts, boxes) < MARGIN).any(1) | (ref != AO.points_in_rbbox(pts, boxes, np.float64)).any(1)
        if not bad.any():
            return pts, ref, again / max(n, 1)
        again += int(bad.sum())
        pts[bad] = draw_points(rng, int(bad.sum()), boxes, ndim)
    raise RuntimeError("points do not settle")


def pair_variants(boxes):
    """the box set under centre shifts of +-MARGIN and extent scalings of 1 +- DIM_EPS"""
    out = []
    for dx, dy, s in ((MARGIN, 0, 1), (-MARGIN, 0, 1), (0, MARGIN, 1), (0, -MARGIN, 1), (0, 0, 1 + DIM_EPS), (0, 0, 1 - DIM_EPS)):
        v = np.array(boxes, np.float64)
        v[:, 0] += dx
        v[:, 1] += dy
        v[:, 3:5] *= s
        out.append(v)
    return out


def unstable_pairs(a, b):
    """bool [N, K]: the float64 collision of a row of a (shifted, scaled) with a row of b changes"""
    base = AO.box_collision_test(AO.bev_corners(a), AO.bev_corners(b))
    bad = np.zeros_like(base)
    for v in pair_variants(a):
        bad |= AO.box_collision_test(AO.bev_corners(v), AO.bev_corners(b)) != base
    return bad, base


def save(name, meta, **arrays):
    np.savez_compressed(os.path.join(HERE, name), meta=np.array(json.dumps(meta)), **arrays)
    print(name, {k: v for k, v in meta.items() if k.startswith(("again", "e_"))})


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def record_inbox(ops, tag, seed, n_points, n_boxes, ndim, length):
    rng = np.random.default_rng(seed)
    boxes = draw_boxes(rng, n_boxes, length)
    if n_boxes > 3:
        boxes[1, 3:6] = 0.0                                              # a zero-size box holds nothing
        boxes[2, -1], boxes[3, -1] = np.float32(np.pi / 2), np.float32(-np.pi)
    pts, mask, again = stable_points(ops, rng, n_points, boxes, ndim)
    counts = np.asarray(ops.points_count_rbbox(pts, boxes)) if n_boxes and n_points else np.zeros(n_boxes, np.int64)
    assert again <= 0.05 and np.array_equal(counts, mask.sum(0))
    save(f"detaug_inbox_{tag}.npz", dict(again_points=again, source="box_np_ops.points_in_rbbox / points_count_rbbox, numba replaced by the identity"),
         points=pts, boxes=boxes, mask=np.packbits(mask, axis=None), counts=counts.astype(np.int32))


def record_collision(ops, prep, tag, seed, n, k):
    rng = np.random.default_rng(seed)

    def bev(m):
        b = draw_boxes(rng, m, 7, spread=18.0)
        b[:, 3:5] = rng.uniform(0.8, 6.0, (m, 2))
        return b
    a, b = bev(n), bev(k)
    again = 0
    for _ in range(20):
        ca = ops.center_to_corner_box2d(a[:, 0:2], a[:, 3:5], a[:, -1])
        cb = ops.center_to_corner_box2d(b[:, 0:2], b[:, 3:5], b[:, -1])
        ref = ref_collision(prep, ca, cb)
        bad, base = unstable_pairs(a, b)
        rows = (bad | (ref != base)).any(1)
        if not rows.any():
            break
        again += int(rows.sum())
        a[rows] = bev(int(rows.sum()))
    else:
        raise RuntimeError("boxes do not settle")
    assert ca.dtype == np.float32 and again / n <= 0.05
    e = float(np.abs(ca.astype(np.float64) - AO.bev_corners(a)).max())
    save(f"detaug_collision_{tag}.npz", dict(again_boxes=again / n, e_corners=e, hits=int(ref.sum()),
                                             source="preprocess.box_collision_test over box_np_ops.center_to_corner_box2d"),
         boxes_a=a, boxes_b=b, corners_a=ca, corners_b=cb, collide=np.packbits(ref, axis=None))


def make_database(rng, per_class=6, ndim=5):
    boxes, classes, pts, offs = [], [], [], [0]
    for c, name in enumerate(CLASS_NAMES):
        for _ in range(per_class):
            size = np.array(SIZES[name]) * rng.uniform(0.85, 1.15, 3)
            box = np.zeros(9, np.float32)
            box[0:2], box[2] = rng.uniform(-45, 45, 2), rng.uniform(-1.5, 0.0)
            box[3:6], box[6:8], box[8] = size, rng.normal(0, 2.0, 2), rng.uniform(-np.pi, np.pi)
            n = int(rng.integers(5, 40))
            p = np.zeros((n, ndim), np.float32)
            p[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * size
            p[:, 3:] = rng.random((n, ndim - 3))
            boxes.append(box); classes.append(c + 1); pts.append(p); offs.append(offs[-1] + n)
    return dict(points=np.concatenate(pts), offsets=np.array(offs, np.int64), boxes=np.stack(boxes), classes=np.array(classes, np.int32))


def random_frame(rng, db, n_points, n_gt, ndim=5):
    names, boxes = [], []
    for _ in range(n_gt):
        name = CLASS_NAMES[int(rng.integers(0, 10))] if rng.random() > 0.15 else ("ignore" if rng.random() < 0.5 else "animal")
        size = np.array(SIZES.get(name, (1.0, 1.0, 1.0))) * rng.uniform(0.85, 1.15, 3)
        box = np.zeros(9, np.float32)
        box[0:2], box[2] = rng.uniform(-58, 58, 2), rng.uniform(-1.5, 0.0)
        box[3:6], box[6:8], box[8] = size, rng.normal(0, 2.0, 2), rng.uniform(-np.pi, np.pi)
        names.append(name); boxes.append(box)
    boxes = np.stack(boxes) if boxes else np.zeros((0, 9), np.float32)
    pts = draw_points(rng, n_points, boxes, ndim) if n_points else np.zeros((0, ndim), np.float32)
    cands = []
    for q, g in enumerate(SAMPLE_GROUPS):
        (name, num), = g.items()
        ids = np.flatnonzero(db["classes"] == CLASS_NAMES.index(name) + 1)
        cands.append(rng.permutation(ids)[:min(num, len(ids))].astype(np.int32))
    return names, boxes, pts, cands


def crafted_frame(db_rng, ndim=5):
    """A frame and a database of axis-aligned boxes, far apart except where a collision is wanted.  car: the frame has its two, the
    group takes none.  truck: T0 sits on a ground-truth box (rejected), T1 overlaps T0 only (accepted BECAUSE T0 was rejected), T2
    is free (accepted).  construction_vehicle: seven wanted, three offered; C0-C1 and C1-C2 overlap: C0 and C1 both fall to a LATER
    candidate, C2 stays.  bus: both candidates sit on ground truth: none accepted.  trailer: R0 overlaps the pasted truck T2
    (rejected by an earlier class's paste), R1 is free.  Every other group is offered one free object (the reference cannot be
    handed an empty list when it wants one)."""
    def box(x, y, dx, dy, name):
        b = np.zeros(9, np.float32)
        b[:] = [x, y, -1.0, dx, dy, 2.0, 0.5, -0.25, 0.0]
        return b, name
    gt = [box(-40, -40, 4.5, 2.0, "car"), box(-40, -30, 4.5, 2.0, "car"), box(0, 0, 6.0, 2.5, "pedestrian"), box(20, 20, 10.0, 3.0, "animal"),
          box(30, -30, 3.0, 3.0, "ignore"), box(-20, 30, 8.0, 3.0, "barrier")]
    db = [box(-40.5, -35, 4.0, 2.0, "car"),                                                             # 0: offered, never looked at
          box(1.0, 0.5, 6.0, 2.5, "truck"), box(6.5, 1.0, 6.0, 2.5, "truck"), box(-10, -20, 6.0, 2.5, "truck"),      # 1 T0, 2 T1, 3 T2
          box(40, 0, 6.0, 3.0, "construction_vehicle"), box(44, 1, 6.0, 3.0, "construction_vehicle"),
          box(48, 2, 6.0, 3.0, "construction_vehicle"),                                                 # 4 C0, 5 C1, 6 C2
          box(21, 21, 11.0, 3.0, "bus"), box(-21, 31, 11.0, 3.0, "bus"),                                   # 7, 8: on ground truth
          box(-12, -21, 12.0, 3.0, "trailer"), box(-30, 10, 12.0, 3.0, "trailer"),                          # 9 R0 on T2, 10 R1
          box(-50, 50, 0.5, 2.5, "barrier"), box(50, 50, 2.0, 0.8, "motorcycle"), box(50, -50, 1.7, 0.6, "bicycle"),
          box(10, -45, 0.7, 0.7, "pedestrian"), box(-5, 45, 0.4, 0.4, "traffic_cone")]                       # 11..15: free, one per remaining group
    pts, offs = [], [0]
    for b, _ in db:
        n = int(db_rng.integers(4, 12))
        p = np.zeros((n, ndim), np.float32)
        p[:, :3] = db_rng.uniform(-0.45, 0.45, (n, 3)) * b[3:6]
        p[:, 3:] = db_rng.random((n, ndim - 3))
        pts.append(p); offs.append(offs[-1] + n)
    database = dict(points=np.concatenate(pts), offsets=np.array(offs, np.int64), boxes=np.stack([b for b, _ in db]),
                    classes=np.array([CLASS_NAMES.index(n) + 1 for _, n in db], np.int32))
    cands = [np.array(c, np.int32) for c in ([0], [1, 2, 3], [4, 5, 6], [7, 8], [9, 10], [11], [12], [13], [14], [15])]
    names, boxes = [n for _, n in gt], np.stack([b for b, _ in gt])
    scene = draw_points(db_rng, 300, boxes, ndim)
    return names, boxes, scene, cands, database, dict(expect_accepted=[2, 3, 6, 10, 11, 12, 13, 14, 15])


def class_ids(names):
    return np.array([CLASS_NAMES.index(n) + 1 if n in CLASS_NAMES else (0 if n in ("DontCare", "ignore", "UNKNOWN") else -1) for n in names],
                    np.int32).reshape(-1)


def run_reference(mods, db, names, boxes, pts, cands, draws, order, min_points):
    """the frame through the reference's Preprocess and the box filter of Voxelization -> (points, gt_boxes, gt_classes, accepted)"""
    ops, prep, sops, pipe = mods
    infos = {n: [] for n in CLASS_NAMES}
    for d in range(len(db["classes"])):
        name = CLASS_NAMES[db["classes"][d] - 1]
        infos[name].append(dict(name=name, path=f"obj_{d}.bin", box3d_lidar=db["boxes"][d].copy(), difficulty=0, group_id=d,
                                num_points_in_gt=int(db["offsets"][d + 1] - db["offsets"][d]), db_index=d))
    by_index = {i["db_index"]: i for v in infos.values() for i in v}
    sampler = sops.DataBaseSamplerV2(infos, SAMPLE_GROUPS, None, 1.0, [0, 0], Logger())
    for q, g in enumerate(SAMPLE_GROUPS):
        (name, _), = g.items()
        sampler._sampler_dict[name].sample = (lambda lst: (lambda num: [by_index[int(i)] for i in lst[:int(num)]]))(cands[q])
    accepted = []
    inner = sampler.sample_class_v2

    def sample_class_v2(name, num, gt_boxes):
        got = inner(name, num, gt_boxes)
        accepted.extend(s["db_index"] for s in got)
        return got
    sampler.sample_class_v2 = sample_class_v2
    cfg = Cfg(mode="train", shuffle_points=True, min_points_in_gt=min_points, global_rot_noise=list(ROT), global_scale_noise=list(SCALE),
              global_translate_std=STD, class_names=CLASS_NAMES, db_sampler=Cfg(enable=True, instance=sampler))
    p = pipe.Preprocess(cfg=cfg)
    res = dict(type="NuScenesDataset", lidar=dict(combined=pts.copy(), annotations=dict(boxes=boxes.copy(), names=list(names))),
               metadata=dict(image_prefix="/db", num_point_features=pts.shape[1]))
    noise = AO.draws_to_noise(draws, ROT, SCALE, [STD] * 3)
    uniforms = iter([(ROT, noise[2]), (SCALE, noise[3])])
    flips, normals = iter([noise[0], noise[1]]), iter(noise[4])
    keep = (np.random.choice, np.random.uniform, np.random.normal, np.random.shuffle, np.fromfile)

    def uniform(lo, hi):
        rng_, v = next(uniforms)
        assert [lo, hi] == list(rng_)
        return float(v)

    def shuffle(arr):
        arr[:] = arr[np.asarray(order[:len(arr)])] if len(order) else arr

    def fromfile(path, dtype=np.float32):
        d = int(os.path.basename(str(path))[4:-4])
        return db["points"][db["offsets"][d]:db["offsets"][d + 1]].copy().reshape(-1)
    np.random.choice = lambda *a, **k: bool(next(flips))
    np.random.uniform, np.random.shuffle, np.fromfile = uniform, shuffle, fromfile
    np.random.normal = lambda loc, scale, size: np.array([float(next(normals))])
    try:
        with PythonBools():
            res, _ = p(res, None)
    finally:
        np.random.choice, np.random.uniform, np.random.normal, np.random.shuffle, np.fromfile = keep
    gt = res["lidar"]["annotations"]
    pc = np.array(PC_RANGE, np.float32)
    mask = prep.filter_gt_box_outside_range(gt["gt_boxes"], pc[[0, 1, 3, 4]]) if len(gt["gt_boxes"]) else np.zeros(0, bool)
    return res["lidar"]["points"], gt["gt_boxes"][mask], gt["gt_classes"][mask], np.array(accepted, np.int32)


def frame_is_stable(db, boxes, classes, cands, draws, got, want):
    """the frame's collision pairs and range tests do not change under the shifts, and the reference decides as float64 does"""
    offered = np.concatenate([c for c in cands if len(c)]) if any(len(c) for c in cands) else np.zeros(0, np.int32)
    allb = np.concatenate([boxes[classes != 0], db["boxes"][offered]], 0).astype(np.float64)
    if len(allb):
        bad = unstable_pairs(allb, allb)[0]
        bad[np.arange(len(allb)), np.arange(len(allb))] = False              # a box against itself is never asked
        if bad.any():
            return False
    if not (np.array_equal(got[3], want["accepted"]) and got[1].shape == want["gt_boxes"].shape and np.array_equal(got[2], want["gt_classes"])):
        return False
    noise = AO.draws_to_noise(draws, ROT, SCALE, [STD] * 3)
    merged = np.concatenate([boxes[classes >= 1], db["boxes"][want["accepted"]]], 0)
    if len(merged):
        _, moved = AO.global_transform(np.zeros((0, 5)), merged, noise)
        rng32 = [float(np.float32(PC_RANGE[i])) for i in (0, 1, 3, 4)]
        base = AO.filter_gt_box_outside_range(moved, rng32)
        for v in pair_variants(moved):
            v[:, -1] = moved[:, -1]
            if not np.array_equal(AO.filter_gt_box_outside_range(v, rng32), base):
                return False
    return True


def record_frames(mods, tag, seed, frames, min_points, crafted=False):
    """frames: (points, ground-truth boxes) per frame"""
    rng = np.random.default_rng(seed)
    out, again, tried = {}, 0, 0
    meta = dict(class_names=CLASS_NAMES, sample_groups=SAMPLE_GROUPS, rate=1.0, rot=ROT, scale=SCALE, std=STD, min_points=min_points,
                pc_range=PC_RANGE, flip_probability=0.5, frames=len(frames), source="pipelines/preprocess.py::Preprocess + filter_gt_box_outside_range")
    db = None if crafted else make_database(rng)
    e_points = e_boxes = 0.0
    for f, (n_points, n_gt) in enumerate(frames):
        for _ in range(20):
            tried += 1
            if crafted:
                names, boxes, pts, cands, db, extra = crafted_frame(rng)
                meta.update(extra)
            else:
                names, boxes, pts, cands = random_frame(rng, db, n_points, n_gt)
            classes = class_ids(names)
            live = boxes[classes != 0]
            if min_points > 0 and len(live) and len(pts):                 # the counts must be safe too
                bad = (AO.face_distance(pts, live) < MARGIN).any(1)
                pts = pts[~bad]
            draws = rng.random(7).astype(np.float32)
            draws[4:] = rng.standard_normal(3).astype(np.float32)
            if crafted:
                draws[0], draws[1] = 0.75, 0.25                          # one flip on, one off
            cfg = dict(min_points=min_points, group_classes=[CLASS_NAMES.index(list(g)[0]) + 1 for g in SAMPLE_GROUPS],
                       group_max=[list(g.values())[0] for g in SAMPLE_GROUPS], rate=1.0, rot=ROT, scale=SCALE, std=[STD] * 3,
                       flip_probability=0.5, bv_range=[float(np.float32(PC_RANGE[i])) for i in (0, 1, 3, 4)])
            probe = AO.preprocess(pts, boxes, classes, cfg, draws, None, cands, db)
            total = len(probe["points"])
            order = rng.permutation(total)
            want = AO.preprocess(pts, boxes, classes, cfg, draws, order, cands, db)
            got = run_reference(mods, db, names, boxes, pts, cands, draws, order, min_points)
            if frame_is_stable(db, boxes, classes, cands, draws, got, want):
                break
            again += 1
        else:
            raise RuntimeError("frame does not settle")
        assert got[0].dtype == np.float32 and got[1].dtype == np.float32 and got[0].shape == want["points"].shape
        e_points = max(e_points, float(np.abs(got[0].astype(np.float64) - want["points"]).max()) if total else 0.0)
        e_boxes = max(e_boxes, float(np.abs(got[1].astype(np.float64) - want["gt_boxes"]).max()) if len(got[1]) else 0.0)
        out.update({f"f{f}_points": pts, f"f{f}_gt_boxes": boxes, f"f{f}_gt_classes": classes, f"f{f}_draws": draws,
                    f"f{f}_order": order.astype(np.int32), f"f{f}_cand": np.concatenate(cands) if any(len(c) for c in cands) else np.zeros(0, np.int32),
                    f"f{f}_cand_len": np.array([len(c) for c in cands], np.int32), f"f{f}_out_points": got[0], f"f{f}_out_boxes": got[1],
                    f"f{f}_out_classes": got[2].astype(np.int32), f"f{f}_accepted": got[3], f"f{f}_counts": want["counts"].astype(np.int32)})
    meta.update(again_frames=again / tried, e_points=e_points, e_boxes=e_boxes)
    assert again / tried <= 0.05, again / tried
    if crafted:
        assert list(out["f0_accepted"]) == meta["expect_accepted"], out["f0_accepted"]
    save(f"detaug_frames_{tag}.npz", meta, db_points=db["points"], db_offsets=db["offsets"], db_boxes=db["boxes"], db_classes=db["classes"], **out)


def record_sampler(prep):
    """BatchSampler's stream (core/sampler/preprocess.py:19-53) under np.random.seed: what DatabaseSampler.draw must hand out"""
    asks = [3, 5, 4, 6, 17, 2, 20, 1, 16, 1, 9, 9, 9]
    np.random.seed(123)
    sampler = prep.BatchSampler(list(range(100, 117)), "car")
    got = [np.asarray(sampler.sample(n), np.int32) for n in asks]
    save("detaug_sampler.npz", dict(seed=123, items=list(range(100, 117)), source="core/sampler/preprocess.py::BatchSampler.sample"),
         asks=np.array(asks, np.int32), lens=np.array([len(g) for g in got], np.int32), drawn=np.concatenate(got))


def main():
    mods = load_reference(sys.argv[1])
    ops, prep = mods[0], mods[1]
    record_sampler(prep)
    record_inbox(ops, "a", 1, 4097, 65, 5, 9)
    record_inbox(ops, "b", 2, 65, 500, 4, 7)
    record_inbox(ops, "c", 3, 1, 1, 6, 7)
    record_collision(ops, prep, "a", 4, 65, 130)
    record_collision(ops, prep, "b", 5, 1, 64)
    record_frames(mods, "rand", 6, [(1500, 30), (0, 0), (700, 12)], -1)
    record_frames(mods, "minpts", 7, [(900, 25)], 3)
    record_frames(mods, "crafted", 8, [(300, 6)], -1, crafted=True)


if __name__ == "__main__":
    main()
