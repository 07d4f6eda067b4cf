"""GPU checks of the detection training front end (link_amd/detaug.py, csrc/detaug.hip, section P).

Predicates -- in-box masks, counts, collision matrices, accepted lists, kept boxes -- are compared EXACTLY: with the reference's
recordings on the fixtures (tests/golden/make_golden_detaug.py keeps stable inputs only: every point at least 1e-4 m from every face
plane, every box pair and range test unchanged under centre shifts of 1e-4 m and extent scalings of 1 +- 1e-5), and with the float64
restatement (tests/aug_oracle.py, pinned on those recordings by tests/test_cpu_detaug.py) on the sizes no fixture holds, whose scenes
are filtered by the same rule.  Float outputs -- transformed points and boxes, BEV corners -- are gated on the float64 oracle:
distance at most 4 e_ref + 1 fp32 ulp of the largest magnitude, e_ref the reference recording's own distance from float64 (the
fixture's meta).  Every comparison leaves its figures in detaug_parity.jsonl in the directory LINK_AMD_PARITY_DIR names before any
verdict (profiles/detaug_parity.jsonl is one run)."""
import functools

import numpy as np
import pytest
import torch

import aug_oracle as AO
from helpers import golden_files, load_golden
from ref64 import record_row
from aug_oracle import frame_cfg, frame_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 1e-4


def t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def gate(test, case, name, got, want64, e_ref):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    big = float(np.abs(want64).max(initial=0.0))
    bound = 4 * float(e_ref) + float(np.spacing(np.float32(big)))
    d = float(np.abs(got - want64).max(initial=0.0))
    print(test, case, name, "e_dev", d, "e_ref", float(e_ref), "bound", bound)
    record_row({"test": test, **case, "component": name, "e_dev": d, "e_ref": float(e_ref), "bound": bound}, name="detaug_parity.jsonl")
    assert d <= bound, (test, case, name, d, bound)


# ---- P1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_files("detaug_inbox_*.npz"))
def test_points_in_boxes_replays_the_reference(name):
    import link_amd as la
    g = load_golden(name)
    p, n = g["points"].shape[0], g["boxes"].shape[0]
    want = np.unpackbits(g["mask"])[:p * n].reshape(p, n).astype(bool)
    mask = la.points_in_rbbox(t(g["points"]), t(g["boxes"]))
    counts = la.points_count_rbbox(t(g["points"]), t(g["boxes"]))
    assert mask.dtype == torch.bool and counts.dtype == torch.int32
    assert np.array_equal(mask.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), g["counts"])


@functools.lru_cache(maxsize=None)
def pool():
    """500 boxes, 4097 points that are safe against every one of them (so against every subset), and the float64 mask, once"""
    rng = np.random.default_rng(100)
    boxes = np.zeros((500, 7), np.float32)
    boxes[:, 0:2], boxes[:, 2] = rng.uniform(-50, 50, (500, 2)), rng.uniform(-2, 1, 500)
    boxes[:, 3:6] = np.exp(rng.uniform(np.log(0.4), np.log(12.0), (500, 3)))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, 500)
    boxes[7, 3:6] = 0.0
    pts = np.zeros((0, 3), np.float32)
    while len(pts) < 4097:
        which = rng.integers(0, 500, 4000)
        local = rng.uniform(-0.7, 0.7, (4000, 3)) * boxes[which, 3:6]
        a = boxes[which, 6].astype(np.float64)
        cand = np.stack([local[:, 0] * np.cos(a) + local[:, 1] * np.sin(a), -local[:, 0] * np.sin(a) + local[:, 1] * np.cos(a), local[:, 2]], 1)
        cand = (cand + boxes[which, :3]).astype(np.float32)
        cand[::3] = rng.uniform([-55, -55, -4], [55, 55, 3], (len(cand[::3]), 3))
        pts = np.concatenate([pts, cand[(AO.face_distance(cand, boxes) >= MARGIN).all(1)]])
    pts = pts[:4097]
    return boxes, pts, AO.points_in_rbbox(pts, boxes)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 500])
@pytest.mark.parametrize("p", [0, 1, 63, 64, 65, 4097])
def test_points_in_boxes_sizes(p, n):
    import link_amd as la
    boxes, pts, mask = pool()
    f = 4 + (p + n) % 3                                                        # F in {4, 5, 6}
    length = 7 + 2 * ((p + n) % 2)                                             # heading in the last of 7 or 9 columns
    pf = np.concatenate([pts[:p], np.full((p, f - 3), 7.0, np.float32)], 1)
    bf = np.concatenate([boxes[:n, :6], np.full((n, length - 7), 3.0, np.float32), boxes[:n, 6:]], 1)
    got = la.points_in_rbbox(t(pf), t(bf))
    cnt = la.points_count_rbbox(t(pf), t(bf))
    assert tuple(got.shape) == (p, n) and tuple(cnt.shape) == (n,)
    assert np.array_equal(got.cpu().numpy(), mask[:p, :n]) and np.array_equal(cnt.cpu().numpy(), mask[:p, :n].sum(0))
    if p == 4097 and n == 500:
        assert mask.sum() > 1000 and not mask[:, 7].any()


@pytest.mark.parametrize("batch", [1, 3])
def test_points_in_boxes_batched_with_an_empty_frame(batch):
    import link_amd as la
    boxes, pts, mask = pool()
    n = 65
    offs = [0, 4097] if batch == 1 else [0, 63, 63, 1000]                     # the middle frame holds no point
    bb = np.stack([boxes[b * n:(b + 1) * n] for b in range(batch)])
    want = np.zeros((offs[-1], n), bool)
    for b in range(batch):
        want[offs[b]:offs[b + 1]] = mask[offs[b]:offs[b + 1], b * n:(b + 1) * n]
    pf = np.concatenate([pts[:offs[-1]], np.zeros((offs[-1], 2), np.float32)], 1)
    got = la.points_in_rbbox(t(pf), t(bb), point_offsets=t(offs, torch.int32))
    cnt = la.points_count_rbbox(t(pf), t(bb), point_offsets=t(offs, torch.int32))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(cnt.cpu().numpy(), np.stack([want[offs[b]:offs[b + 1]].sum(0) for b in range(batch)]))
    assert want.sum() > 50


@pytest.mark.parametrize("heading", [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 2 * np.pi])
def test_points_beside_every_face(heading):
    """points 2e-4 m inside and outside each of the six faces (by construction: in the box frame), and a zero-size box"""
    import link_amd as la
    box = np.array([10.0, -5.0, 1.0, 4.0, 2.0, 1.5, heading], np.float64)
    pts, want = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            for eps, inside in ((-2e-4, True), (2e-4, False)):
                local = np.array([0.3, -0.2, 0.1])
                local[axis] = side * (box[3 + axis] / 2 + eps)
                x = local[0] * np.cos(heading) + local[1] * np.sin(heading)
                y = -local[0] * np.sin(heading) + local[1] * np.cos(heading)
                pts.append([x + box[0], y + box[1], local[2] + box[2]])
                want.append(inside)
    pts = np.array(pts, np.float32)
    boxes = np.stack([box, [10.0, -5.0, 1.0, 0.0, 0.0, 0.0, heading]]).astype(np.float32)
    assert np.array_equal(AO.points_in_rbbox(pts, boxes)[:, 0], want)
    got = la.points_in_rbbox(t(pts), t(boxes)).cpu().numpy()
    assert np.array_equal(got[:, 0], want) and not got[:, 1].any()
    centre = la.points_in_rbbox(t(boxes[:1, :3].copy()), t(boxes)).cpu().numpy()
    assert centre[0, 0] and not centre[0, 1]                                   # a zero-size box does not even hold its own centre


# ---- P2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_files("detaug_collision_*.npz"))
def test_collision_replays_the_reference(name):
    import link_amd as la
    g = load_golden(name)
    a, b = g["boxes_a"], g["boxes_b"]
    want = np.unpackbits(g["collide"])[:len(a) * len(b)].reshape(len(a), len(b)).astype(bool)
    ca = la.center_to_corner_box2d(t(a[:, 0:2]), t(a[:, 3:5]), t(a[:, -1]))
    cb = la.center_to_corner_box2d(t(b[:, 0:2]), t(b[:, 3:5]), t(b[:, -1]))
    gate("corners", {"fixture": name}, "corners_a", ca.cpu().numpy(), AO.bev_corners(a), g["meta"]["e_corners"])
    assert np.array_equal(la.box_collision_test(ca, cb).cpu().numpy(), want)                              # corners made on the device
    assert np.array_equal(la.box_collision_test(t(g["corners_a"]), t(g["corners_b"])).cpu().numpy(), want)   # the reference's corners
    plain = la.center_to_corner_box2d(t(a[:, 0:2]), t(a[:, 3:5])).cpu().numpy()                           # no angle: the corner order
    assert np.array_equal(np.sign(plain[0] - a[0, 0:2]), [[-1, -1], [-1, 1], [1, 1], [1, -1]])


@functools.lru_cache(maxsize=None)
def box_pool():
    """500 x 500 BEV boxes whose float64 collisions do not change under the shifts and scalings; rows that would are moved far away"""
    rng = np.random.default_rng(101)

    def draw(n):
        b = np.zeros((n, 7), np.float32)
        b[:, 0:2], b[:, 3:5], b[:, 6] = rng.uniform(-30, 30, (n, 2)), rng.uniform(0.8, 7.0, (n, 2)), rng.uniform(-np.pi, np.pi, n)
        return b
    a, b = draw(500), draw(500)
    cb = AO.bev_corners(b)
    base = AO.box_collision_test(AO.bev_corners(a), cb)
    bad = np.zeros(500, bool)
    for dx, dy, s in ((MARGIN, 0, 1), (-MARGIN, 0, 1), (0, MARGIN, 1), (0, -MARGIN, 1), (0, 0, 1 + 1e-5), (0, 0, 1 - 1e-5)):
        v = a.astype(np.float64)
        v[:, 0] += dx
        v[:, 1] += dy
        v[:, 3:5] *= s
        bad |= (AO.box_collision_test(AO.bev_corners(v), cb) != base).any(1)
    assert bad.mean() <= 0.05
    a[bad, 0] = 1000.0 + 40.0 * np.arange(bad.sum())
    return a, b, AO.box_collision_test(AO.bev_corners(a), cb)


@pytest.mark.parametrize("k", [0, 1, 64, 65, 500])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 500])
def test_collision_sizes(n, k):
    import link_amd as la
    a, b, want = box_pool()
    ca = la.center_to_corner_box2d(t(a[:n, 0:2]), t(a[:n, 3:5]), t(a[:n, 6]))
    cb = la.center_to_corner_box2d(t(b[:k, 0:2]), t(b[:k, 3:5]), t(b[:k, 6]))
    got = la.box_collision_test(ca, cb)
    assert tuple(got.shape) == (n, k) and np.array_equal(got.cpu().numpy(), want[:n, :k])
    if n == 500 and k == 500:
        assert want.sum() > 500


def test_collision_built_cases():
    import link_amd as la
    both = lambda a, b: (bool(la.box_collision_test(t(a, torch.float32), t(b, torch.float32))[0, 0]),      # noqa: E731
                         bool(la.box_collision_test(t(b, torch.float32), t(a, torch.float32))[0, 0]))
    diamond = np.array([[[0, 1], [1, 2], [2, 1], [1, 0]]], np.float64)          # shares the edge (1, 2)-(2, 1) with its copy at + (1, 1)
    assert not AO.box_collision_test(diamond, diamond + 1).any() and both(diamond, diamond + 1) == (False, False)
    big, small = AO.center_to_corner_box2d([[0, 0]], [[10, 6]], [0.3]), AO.center_to_corner_box2d([[0.5, 0.2]], [[1, 1]], [1.0])
    assert both(big, small) == (True, True)                                    # one wholly inside the other, both ways
    a, b = AO.center_to_corner_box2d([[0, 0]], [[2, 2]], [0.0]), AO.center_to_corner_box2d([[2, 0.5]], [[2, 3]], [0.0])
    assert both(a, b) == (False, False)                                        # stand-up boxes that touch: iw == 0 is not > 0
    assert both(a, a + np.array([1.0, 1.0])) == (True, True)
    counter = big[:, ::-1].copy()                                              # the other orientation needs clockwise=False
    assert AO.box_collision_test(counter, small[:, ::-1], False).all()
    assert bool(la.box_collision_test(t(counter, torch.float32), t(small[:, ::-1].copy(), torch.float32), clockwise=False)[0, 0])


# ---- P3 + P4 --------------------------------------------------------------------------------------------------------------------------
def perm_for(order, cap, rng):
    """a permutation of 0..cap-1 that leaves the frame's valid slots in the fixture's shuffled order: slot order[i] gets the i-th of
    len(order) sorted places, the unused slots the others"""
    places = rng.permutation(cap)
    mine = np.sort(places[:len(order)])
    perm = np.empty(cap, np.int32)
    perm[np.asarray(order, np.int64)] = mine
    perm[np.setdiff1d(np.arange(cap), order)] = places[len(order):]
    return perm


@functools.lru_cache(maxsize=None)
def frames_case(name, cap=2600, max_objs=64):
    """the fixture's frames as one batch on the device + everything the comparisons need, once per fixture"""
    import link_amd as la
    g = load_golden(name)
    m = g["meta"]
    rng = np.random.default_rng(5)
    frames = [frame_of(g, f) for f in range(m["frames"])]
    db_np = frames[0][2]
    db = la.GTDatabase(db_np["points"], db_np["offsets"], db_np["boxes"], db_np["classes"])
    aug = la.DetTrainAugmenter(m["class_names"], m["sample_groups"], m["rate"], m["rot"], m["scale"], m["std"], m["min_points"], m["pc_range"],
                               max_objs, cap, m["flip_probability"], database=db)
    B, G = len(frames), max(max(len(fr["gt_classes"]) for fr, _, _ in frames), 1)
    gb, gc = np.zeros((B, G, 9), np.float32), np.zeros((B, G), np.int32)
    cand, lens = np.full((B, len(aug.group_classes), aug.max_candidates), -1, np.int32), np.zeros((B, len(aug.group_classes)), np.int32)
    perm = np.zeros((B, cap), np.int32)
    for b, (fr, cands, _) in enumerate(frames):
        n = len(fr["gt_classes"])
        gb[b, :n], gc[b, :n] = fr["gt_boxes"], fr["gt_classes"]
        for q, c in enumerate(cands):
            cand[b, q, :len(c)], lens[b, q] = c, len(c)
        perm[b] = perm_for(fr["order"], cap, rng)
    pts = np.concatenate([fr["points"] for fr, _, _ in frames])
    offs = np.concatenate([[0], np.cumsum([len(fr["points"]) for fr, _, _ in frames])])
    args = dict(points=t(pts), point_offsets=t(offs, torch.int32), gt_boxes=t(gb), gt_classes=t(gc),
                draws=t(np.stack([fr["draws"] for fr, _, _ in frames])), perm=t(perm), candidates=t(cand), candidate_lengths=t(lens))
    want = [AO.preprocess(fr["points"], fr["gt_boxes"], fr["gt_classes"], frame_cfg(m), fr["draws"], fr["order"], c, db_np) for fr, c, _ in frames]
    return g, aug, args, frames, want


def bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", golden_files("detaug_frames_*.npz"))
def test_augmenter_replays_the_reference(name):
    g, aug, args, frames, want = frames_case(name)
    m = g["meta"]
    out = aug.padded(**args)
    nb, npts, nacc = out["num_boxes"].cpu().numpy(), out["num_points"].cpu().numpy(), out["num_accepted"].cpu().numpy()
    assert not out["status"].any()
    for b, ((fr, _, _), w) in enumerate(zip(frames, want)):
        case = {"fixture": name, "frame": b}
        assert np.array_equal(out["accepted"][b, :nacc[b]].cpu().numpy(), fr["accepted"]) and (out["accepted"][b, nacc[b]:] == -1).all()
        assert nb[b] == len(fr["out_classes"]) and np.array_equal(out["gt_classes"][b, :nb[b]].cpu().numpy(), fr["out_classes"])
        assert not out["gt_classes"][b, nb[b]:].any() and not out["gt_boxes"][b, nb[b]:].any()
        assert npts[b] == len(fr["out_points"])
        rows = out["points"][b].cpu().numpy()
        valid = ~np.isnan(rows[:, 0])
        assert valid.sum() == npts[b] and np.isnan(rows[~valid]).all()
        if npts[b]:
            gate("augmenter", case, "points", rows[valid], w["points"], m["e_points"])
            assert np.array_equal(rows[valid][:, 3:], fr["out_points"][:, 3:])                               # features are copied
        if nb[b]:
            gate("augmenter", case, "gt_boxes", out["gt_boxes"][b, :nb[b]].cpu().numpy(), w["gt_boxes"], m["e_boxes"])
    if "crafted" in name:
        assert list(out["accepted"][0, :nacc[0]].cpu().numpy()) == m["expect_accepted"]
    # the trimmed form is the padded one without its padding; two calls are bit for bit equal
    res = aug(list(torch.split(args["points"], [len(fr["points"]) for fr, _, _ in frames])), [t(fr["gt_boxes"]) for fr, _, _ in frames],
              [t(fr["gt_classes"]) for fr, _, _ in frames], args["draws"], args["perm"], args["candidates"].cpu().numpy(),
              args["candidate_lengths"].cpu().numpy())
    again = aug.padded(**args)
    for b in range(len(frames)):
        rows = out["points"][b]
        assert torch.equal(res["points"][b], rows[~torch.isnan(rows[:, 0])]) and torch.equal(res["gt_boxes"][b], out["gt_boxes"][b, :nb[b]])
        assert torch.equal(res["gt_classes"][b], out["gt_classes"][b, :nb[b]]) and torch.equal(res["accepted"][b], out["accepted"][b, :nacc[b]])
    for k in ("points", "gt_boxes", "gt_classes", "num_points", "num_boxes", "accepted", "num_accepted", "status"):
        assert torch.equal(bits(again[k]) if again[k].is_floating_point() else again[k], bits(out[k]) if out[k].is_floating_point() else out[k]), k


def test_min_points_filter_uses_the_counts():
    g, aug, args, frames, want = frames_case("detaug_frames_minpts.npz")
    import link_amd as la
    counts = la.points_count_rbbox(args["points"], args["gt_boxes"], point_offsets=args["point_offsets"])
    n = len(frames[0][0]["counts"])
    assert np.array_equal(counts[0, :n].cpu().numpy(), frames[0][0]["counts"])


def test_capacity_and_limits():
    g, aug, args, frames, want = frames_case("detaug_frames_crafted.npz")
    import link_amd as la
    from link_amd import _lib as L
    m = g["meta"]
    small = la.DetTrainAugmenter(m["class_names"], m["sample_groups"], m["rate"], m["rot"], m["scale"], m["std"], m["min_points"], m["pc_range"],
                                 3, 100, m["flip_probability"], database=aug.database)
    a = dict(args, perm=t(np.random.default_rng(0).permutation(100).astype(np.int32)[None]))
    out = small.padded(**a)
    assert int(out["status"][0]) == L.DETAUG_STATUS_POINTS_CUT | L.DETAUG_STATUS_BOXES_CUT
    assert int(out["num_boxes"][0]) == 3 and int(out["num_points"][0]) == 100 and not torch.isnan(out["points"]).any()
    full = aug.padded(**args)
    assert torch.equal(out["gt_boxes"][0], full["gt_boxes"][0, :3])
    with pytest.raises(ValueError, match="exceed"):
        aug.padded(**dict(args, gt_boxes=torch.zeros((1, 1000, 9), device=DEV), gt_classes=torch.zeros((1, 1000), dtype=torch.int32, device=DEV)))
    bad = args["candidates"].clone()
    bad[0, 1, 2] = 10 ** 6                                                     # T2 replaced by an index outside the database
    out = aug.padded(**dict(args, candidates=bad))
    assert int(out["status"][0]) & L.DETAUG_STATUS_BAD_INDEX and 3 not in out["accepted"][0].tolist()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_padded_points_voxelise_like_the_trimmed_ones():
    """NaN rows and the permutation are harmless: the views of the padded buffer give the voxels the trimmed clouds give, bit for bit"""
    import link_amd as la
    g, aug, args, frames, want = frames_case("detaug_frames_rand.npz")
    out = aug.padded(**args)
    trimmed = [out["points"][b][~torch.isnan(out["points"][b][:, 0])] for b in range(len(frames))]
    vox = la.Voxelizer([0.6, 0.6, 0.4], g["meta"]["pc_range"], max_num_points=5, max_voxels=2000)
    ref = vox.generate(trimmed, return_voxels=True)
    mean, coors, num, voff = vox.generate_padded([out["points"][b] for b in range(len(frames))], capacity=int(ref[2].shape[0]) + 7)
    n = int(voff[-1])
    assert n == ref[2].shape[0] and n > 500
    assert torch.equal(bits(mean[:n]), bits(ref[1])) and torch.equal(coors[:n], ref[2]) and torch.equal(num[:n], ref[3])


def test_center_targets_of_the_compacted_boxes():
    """CenterTargetAssigner on the augmenter's output against the same assigner on the reference's recorded gt_dict.  Integer targets
    are equal; the float targets differ by what the boxes differ: at most 4 e_boxes + 1 ulp ~ 3e-5 m, that is 5e-5 cells of 0.6 m, which
    moves a Gaussian of sigma >= 5 / 6 cells, and the offsets in anno_box, by less than 1e-4."""
    import link_amd as la
    g, aug, args, frames, want = frames_case("detaug_frames_rand.npz")
    m = g["meta"]
    out = aug.padded(**args)
    rec_b, rec_c = torch.zeros_like(out["gt_boxes"]), torch.zeros_like(out["gt_classes"])
    for b, (fr, _, _) in enumerate(frames):
        k = len(fr["out_classes"])
        rec_b[b, :k], rec_c[b, :k] = t(fr["out_boxes"]), t(fr["out_classes"])
    assigner = la.CenterTargetAssigner([1, 2, 2, 1, 2, 2], 8, [0.075, 0.075], m["pc_range"], max_objs=aug.max_objs)
    mine, theirs = assigner(out["gt_boxes"], out["gt_classes"]), assigner(rec_b, rec_c)
    for key in ("ind", "mask", "cat"):
        for a, b in zip(mine[key], theirs[key]):
            assert torch.equal(a, b), key
    for key in ("hm", "anno_box"):
        for a, b in zip(mine[key], theirs[key]):
            assert float((a - b).abs().max()) <= 1e-4, key
    assert sum(int(x.sum()) for x in mine["mask"]) > 20


def test_padded_call_replays_under_a_graph():
    g, aug, args, frames, want = frames_case("detaug_frames_rand.npz")
    static = {k: v.clone() for k, v in args.items()}
    aug.padded(**static)                                                       # warm: workspaces exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = aug.padded(**static)
    rng = np.random.default_rng(9)
    B, cap = static["perm"].shape
    for _ in range(2):                                                         # new draws, candidates and permutation in the same tensors
        static["draws"].copy_(t(np.concatenate([rng.random((B, 4)), rng.standard_normal((B, 3))], 1).astype(np.float32)))
        static["perm"].copy_(t(np.stack([rng.permutation(cap) for _ in range(B)]).astype(np.int32)))
        static["candidates"].copy_(static["candidates"].roll(1, 0))        # every frame is offered its neighbour's lists
        static["candidate_lengths"].copy_(static["candidate_lengths"].roll(1, 0))
        graph.replay()
        replayed = {k: v.clone() for k, v in out.items()}
        eager = aug.padded(**static)
        for k in ("points", "gt_boxes", "gt_classes", "num_points", "num_boxes", "accepted", "num_accepted", "status"):
            a, b = replayed[k], eager[k]
            assert torch.equal(bits(a) if a.is_floating_point() else a, bits(b) if b.is_floating_point() else b), k
    assert int(eager["num_points"].sum()) > 0
