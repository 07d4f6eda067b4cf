"""numpy restatement of the detection training front end (link_amd/detaug.py), written from the reference's rules:
det3d/core/bbox/box_np_ops.py (points_in_rbbox, points_count_rbbox, center_to_corner_box2d), core/bbox/geometry.py
(_points_in_convex_polygon_3d_jit), core/sampler/preprocess.py (box_collision_test, random_flip_both, global_rotation, global_scaling_v2,
global_translate_, filter_gt_box_outside_range), core/sampler/sample_ops.py (sample_all, sample_class_v2) and
datasets/pipelines/preprocess.py (Preprocess).  Every function takes `dtype`: np.float64 is the oracle the device is gated on,
np.float32 follows the reference's own arithmetic statement by statement.  tests/test_cpu_detaug.py pins both on fixtures recorded
from the reference (tests/golden/make_golden_detaug.py)."""
import numpy as np

SURFACES = np.array([[0, 1, 2, 3], [7, 6, 5, 4], [0, 3, 7, 4], [1, 5, 6, 2], [0, 4, 5, 1], [3, 2, 6, 7]])


def corners_nd(dims, origin=0.5):
    ndim = dims.shape[1]
    norm = np.stack(np.unravel_index(np.arange(2 ** ndim), [2] * ndim), axis=1).astype(dims.dtype)
    norm = norm[[0, 1, 3, 2]] if ndim == 2 else norm[[0, 1, 3, 2, 4, 5, 7, 6]]
    norm = norm - np.array(origin, dtype=dims.dtype)
    return dims.reshape(-1, 1, ndim) * norm.reshape(1, 2 ** ndim, ndim)


def _rotate_z(c, angles):
    """rotation_3d_in_axis(axis=2) / rotation_2d: x' = x cos + y sin, y' = -x sin + y cos"""
    s, k = np.sin(angles)[:, None], np.cos(angles)[:, None]
    out = c.copy()
    out[..., 0] = c[..., 0] * k + c[..., 1] * s
    out[..., 1] = -c[..., 0] * s + c[..., 1] * k
    return out


def center_to_corner_box2d(centers, dims, angles=None, origin=0.5, dtype=np.float64):
    centers, dims = np.asarray(centers, dtype).reshape(-1, 2), np.asarray(dims, dtype).reshape(-1, 2)
    c = corners_nd(dims, origin)
    if angles is not None:
        c = _rotate_z(c, np.asarray(angles, dtype).reshape(-1))
    return c + centers.reshape(-1, 1, 2)


def box_surfaces(boxes, dtype=np.float64):
    """inward normals [N, 6, 3] and offsets [N, 6] of boxes [N, >= 7] (heading last), as surface_equ_3d_jitv2 forms them"""
    b = np.asarray(boxes, dtype)
    c = _rotate_z(corners_nd(b[:, 3:6], (0.5, 0.5, 0.5)), b[:, -1]) + b[:, None, :3]
    s = c[:, SURFACES]                                         # [N, 6, 4, 3]
    v0, v1 = s[:, :, 0] - s[:, :, 1], s[:, :, 1] - s[:, :, 2]
    n = np.stack([v0[..., 1] * v1[..., 2] - v0[..., 2] * v1[..., 1], v0[..., 2] * v1[..., 0] - v0[..., 0] * v1[..., 2],
                  v0[..., 0] * v1[..., 1] - v0[..., 1] * v1[..., 0]], -1)
    d = -s[:, :, 0, 0] * n[..., 0] - s[:, :, 0, 1] * n[..., 1] - s[:, :, 0, 2] * n[..., 2]
    return n, d


def points_in_rbbox(points, boxes, dtype=np.float64):
    """bool [P, N]: outside when any surface has a p + d >= 0 (geometry.py:267-275)"""
    p = np.asarray(points, dtype)[:, :3]
    boxes = np.asarray(boxes, dtype)
    if boxes.shape[0] == 0 or p.shape[0] == 0:
        return np.zeros((p.shape[0], boxes.shape[0]), bool)
    n, d = box_surfaces(boxes, dtype)
    out = np.ones((p.shape[0], boxes.shape[0]), bool)
    for k in range(6):
        sign = p[:, None, 0] * n[None, :, k, 0] + p[:, None, 1] * n[None, :, k, 1] + p[:, None, 2] * n[None, :, k, 2] + d[None, :, k]
        out &= ~(sign >= 0)
    return out


def points_count_rbbox(points, boxes, dtype=np.float64):
    return points_in_rbbox(points, boxes, dtype).sum(0).astype(np.int32)


def face_distance(points, boxes):
    """float64 [P, N]: the least distance of every point to the six face planes of every box (the stability margin of a fixture); a
    face of no area has no plane and does not count (its sign is an exact zero: outside, whatever the point)"""
    p = np.asarray(points, np.float64)[:, :3]
    n, d = box_surfaces(boxes, np.float64)
    norm = np.linalg.norm(n, axis=-1)
    out = np.full((p.shape[0], n.shape[0]), np.inf)
    for k in range(6):
        sign = p[:, None, 0] * n[None, :, k, 0] + p[:, None, 1] * n[None, :, k, 1] + p[:, None, 2] * n[None, :, k, 2] + d[None, :, k]
        out = np.minimum(out, np.where(norm[None, :, k] > 0, np.abs(sign) / np.maximum(norm[None, :, k], 1e-300), np.inf))
    return out


def _holds(outer, inner, clockwise):
    """[No, Ni]: every corner of inner strictly inside every edge of outer (preprocess.py:905-917)"""
    ok = np.ones((outer.shape[0], inner.shape[0]), bool)
    for k in range(4):
        vec = outer[:, k] - outer[:, (k + 1) % 4]
        if clockwise:
            vec = -vec
        for l in range(4):
            cross = vec[:, None, 1] * (outer[:, None, k, 0] - inner[None, :, l, 0])
            cross = cross - vec[:, None, 0] * (outer[:, None, k, 1] - inner[None, :, l, 1])
            ok &= ~(cross >= 0)
    return ok


def box_collision_test(boxes, qboxes, clockwise=True, dtype=np.float64):
    """bool [N, K] (preprocess.py:854-937)"""
    a, q = np.asarray(boxes, dtype).reshape(-1, 4, 2), np.asarray(qboxes, dtype).reshape(-1, 4, 2)
    if a.shape[0] == 0 or q.shape[0] == 0:
        return np.zeros((a.shape[0], q.shape[0]), bool)
    iw = np.minimum(a[:, :, 0].max(1)[:, None], q[:, :, 0].max(1)[None]) - np.maximum(a[:, :, 0].min(1)[:, None], q[:, :, 0].min(1)[None])
    ih = np.minimum(a[:, :, 1].max(1)[:, None], q[:, :, 1].max(1)[None]) - np.maximum(a[:, :, 1].min(1)[:, None], q[:, :, 1].min(1)[None])
    standup = (iw > 0) & (ih > 0)
    hit = np.zeros_like(standup)
    for s in range(4):
        A, B = a[:, s][:, None], a[:, (s + 1) % 4][:, None]
        for t in range(4):
            C, D = q[:, t][None], q[:, (t + 1) % 4][None]
            acd = (D[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0]) > (C[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
            bcd = (D[..., 1] - B[..., 1]) * (C[..., 0] - B[..., 0]) > (C[..., 1] - B[..., 1]) * (D[..., 0] - B[..., 0])
            abc = (C[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0])
            abd = (D[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
            hit |= (acd != bcd) & (abc != abd)
    return standup & (hit | _holds(a, q, clockwise) | _holds(q, a, clockwise).T)


def bev_corners(boxes, dtype=np.float64):
    b = np.asarray(boxes, dtype)
    return center_to_corner_box2d(b[:, 0:2], b[:, 3:5], b[:, -1], dtype=dtype)


def sample_scan(gt_boxes, gt_classes, counts, min_points, group_classes, group_max, rate, candidates, db_boxes, dtype=np.float64):
    """sample_all + sample_class_v2 without group sampling: gt_classes as DetTrainAugmenter takes them (0 = empty); candidates: one
    list of database indices per group -> (survivor rows of the ground truth, accepted database indices in order)"""
    gt_classes = np.asarray(gt_classes)
    surv = [g for g in range(len(gt_classes)) if gt_classes[g] != 0 and (min_points <= 0 or counts[g] >= min_points)]
    avoid = np.asarray(gt_boxes, dtype).reshape(-1, np.asarray(db_boxes).shape[1] if len(np.asarray(db_boxes).shape) == 2 else 9)[surv]
    accepted = []
    for c, mx, cand in zip(group_classes, group_max, candidates):
        num = int(np.round(rate * int(mx - np.sum(gt_classes[surv] == c))))
        num = max(0, min(num, len(cand)))
        if num <= 0:
            continue
        cand = [int(i) for i in cand[:num]]
        sp = np.asarray(db_boxes, dtype)[cand]
        total = bev_corners(np.concatenate([avoid, sp], 0), dtype)
        coll = box_collision_test(total, total, True, dtype)
        coll[np.arange(len(total)), np.arange(len(total))] = False
        ok = []
        for i in range(len(avoid), len(total)):
            if coll[i].any():
                coll[i] = False
                coll[:, i] = False
            else:
                ok.append(cand[i - len(avoid)])
        accepted += ok
        if ok:
            avoid = np.concatenate([avoid, np.asarray(db_boxes, dtype)[ok]], 0)
    return surv, accepted


def draws_to_noise(draws, rot, scale, std, flip_probability=0.5):
    """the seven draws of a frame -> (flip x, flip y, angle, scale, translation [3]) as doubles: a flip where u >= 1 - p (the rule of
    np.random.choice([False, True], p=[1 - p, p])), low + (high - low) u for np.random.uniform, std n for np.random.normal; z
    is drawn with std[0] (preprocess.py:955)"""
    d = [float(v) for v in draws]
    return (d[0] >= 1.0 - flip_probability, d[1] >= 1.0 - flip_probability, rot[0] + (rot[1] - rot[0]) * d[2],
            scale[0] + (scale[1] - scale[0]) * d[3], np.array([std[0] * d[4], std[1] * d[5], std[0] * d[6]]))


def global_transform(points, boxes, noise, dtype=np.float64):
    """random_flip_both, global_rotation, global_scaling_v2, global_translate_ on copies; boxes [n, 7 | 9], heading last"""
    fx, fy, angle, scale, trans = noise
    points, boxes = np.array(points, dtype), np.array(boxes, dtype)
    angle, scale = float(angle), float(scale)
    if fx:
        boxes[:, 1] = -boxes[:, 1]
        boxes[:, -1] = -boxes[:, -1] + np.pi
        points[:, 1] = -points[:, 1]
        if boxes.shape[1] > 7:
            boxes[:, 7] = -boxes[:, 7]
    if fy:
        boxes[:, 0] = -boxes[:, 0]
        points[:, 0] = -points[:, 0]
        boxes[:, -1] = -boxes[:, -1] + 2 * np.pi
        if boxes.shape[1] > 7:
            boxes[:, 6] = -boxes[:, 6]
    s, c = np.sin(angle), np.cos(angle)
    mat = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=dtype)
    points[:, :3] = points[:, :3] @ mat
    boxes[:, :3] = boxes[:, :3] @ mat
    if boxes.shape[1] > 7:
        vel = np.hstack([boxes[:, 6:8], np.zeros((boxes.shape[0], 1))])        # float64, as the reference's hstack makes it
        boxes[:, 6:8] = (vel @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=vel.dtype))[:, :2]
    boxes[:, -1] += angle
    points[:, :3] *= scale
    boxes[:, :-1] *= scale
    if not all(t == 0 for t in trans):
        points[:, :3] += np.asarray(trans, np.float64)[None]
        boxes[:, :3] += np.asarray(trans, np.float64)[None]
    return points, boxes


def filter_gt_box_outside_range(boxes, bv_range, dtype=np.float64):
    """a box stays when one BEV corner lies strictly inside xmin, ymin, xmax, ymax (preprocess.py:108-122)"""
    c = bev_corners(boxes, dtype).astype(np.float64)
    r = [float(v) for v in bv_range]
    inside = (c[..., 0] > r[0]) & (c[..., 0] < r[2]) & (c[..., 1] > r[1]) & (c[..., 1] < r[3])
    return inside.any(1)


def preprocess(points, gt_boxes, gt_classes, cfg, draws, order, candidates, db, dtype=np.float64):
    """One frame through Preprocess (train) and Voxelization's box filter.  cfg: dict(min_points, group_classes, group_max, rate, rot,
    scale, std, flip_probability, bv_range); candidates: a list of index lists per group; db: dict(points, offsets, boxes, classes);
    order: the permutation np.random.shuffle applies (out[i] = in[order[i]]).  -> dict(points, gt_boxes, gt_classes, accepted,
    survivors, kept)"""
    gt_classes = np.asarray(gt_classes)
    counts = points_count_rbbox(points, gt_boxes, dtype) if cfg["min_points"] > 0 and len(gt_boxes) else np.zeros(len(gt_boxes), np.int32)
    surv, accepted = sample_scan(gt_boxes, gt_classes, counts, cfg["min_points"], cfg["group_classes"], cfg["group_max"], cfg["rate"],
                                 candidates, db["boxes"], dtype)
    own = [g for g in surv if gt_classes[g] >= 1]
    boxes = np.concatenate([np.asarray(gt_boxes, dtype).reshape(-1, db["boxes"].shape[1])[own], np.asarray(db["boxes"], dtype)[accepted]], 0)
    classes = np.concatenate([gt_classes[own], np.asarray(db["classes"])[accepted]]).astype(np.int32)
    pasted = []
    for d in accepted:
        sp = np.array(db["points"][db["offsets"][d]:db["offsets"][d + 1]], dtype)
        sp[:, :3] += np.asarray(db["boxes"], dtype)[d, :3]
        pasted.append(sp)
    pts = np.concatenate(pasted + [np.asarray(points, dtype)], 0)
    noise = draws_to_noise(draws, cfg["rot"], cfg["scale"], cfg["std"], cfg["flip_probability"])
    pts, boxes = global_transform(pts, boxes, noise, dtype)
    pts = pts[np.asarray(order, np.int64)] if order is not None else pts
    kept = filter_gt_box_outside_range(boxes, cfg["bv_range"], dtype) if len(boxes) else np.zeros(0, bool)
    return dict(points=pts, gt_boxes=boxes[kept], gt_classes=classes[kept], accepted=np.asarray(accepted, np.int32),
                survivors=np.asarray(surv, np.int32), kept=kept, counts=counts)


# ---- the fixtures of tests/golden/make_golden_detaug.py -------------------------------------------------------------------------------
def frame_cfg(m):
    return dict(min_points=m["min_points"], group_classes=[m["class_names"].index(list(g)[0]) + 1 for g in m["sample_groups"]],
                group_max=[list(g.values())[0] for g in m["sample_groups"]], rate=m["rate"], rot=m["rot"], scale=m["scale"], std=[m["std"]] * 3,
                flip_probability=m["flip_probability"], bv_range=[float(np.float32(m["pc_range"][i])) for i in (0, 1, 3, 4)])


def frame_of(g, f):
    lens = g[f"f{f}_cand_len"]
    cands = np.split(g[f"f{f}_cand"], np.cumsum(lens)[:-1])
    db = dict(points=g["db_points"], offsets=g["db_offsets"], boxes=g["db_boxes"], classes=g["db_classes"])
    return {k: g[f"f{f}_{k}"] for k in ("points", "gt_boxes", "gt_classes", "draws", "order", "out_points", "out_boxes", "out_classes", "accepted",
                                        "counts")}, cands, db
