"""CPU-only checks of the detection training front end (link_amd/detaug.py, section P): the numpy restatement the GPU tests are gated
on (tests/aug_oracle.py) against the fixtures recorded from the reference, the ABI of section P, and the host logic --
DatabaseSampler against BatchSampler's recorded stream, the argument errors, the refused options, loud failure on CPU tensors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import aug_oracle as AO
from aug_oracle import frame_cfg, frame_of
from helpers import ROOT, golden_files, load_golden

ULP = float(np.finfo(np.float32).eps)


@pytest.mark.parametrize("name", golden_files("detaug_inbox_*.npz"))
def test_oracle_points_in_boxes_is_the_reference(name):
    g = load_golden(name)
    p, n = g["points"].shape[0], g["boxes"].shape[0]
    mask = np.unpackbits(g["mask"])[:p * n].reshape(p, n).astype(bool)
    assert g["meta"]["again_points"] <= 0.05
    for dtype in (np.float64, np.float32):
        assert np.array_equal(AO.points_in_rbbox(g["points"], g["boxes"], dtype), mask), dtype
        assert np.array_equal(AO.points_count_rbbox(g["points"], g["boxes"], dtype), g["counts"])
    assert (AO.face_distance(g["points"], g["boxes"]) >= 1e-4).all()          # the stability the fixture claims
    if p > 1000:
        assert mask.sum() > 500 and not mask[:, 1].any()                       # plenty inside; the zero-size box holds nothing


@pytest.mark.parametrize("name", golden_files("detaug_collision_*.npz"))
def test_oracle_collision_is_the_reference(name):
    g = load_golden(name)
    n, k = g["boxes_a"].shape[0], g["boxes_b"].shape[0]
    want = np.unpackbits(g["collide"])[:n * k].reshape(n, k).astype(bool)
    assert g["meta"]["again_boxes"] <= 0.05
    assert np.array_equal(AO.box_collision_test(g["corners_a"], g["corners_b"], True, np.float32), want)
    assert np.array_equal(AO.box_collision_test(AO.bev_corners(g["boxes_a"]), AO.bev_corners(g["boxes_b"])), want)
    c32 = AO.bev_corners(g["boxes_a"], np.float32)
    assert c32.dtype == np.float32 and np.abs(c32 - g["corners_a"]).max() <= 2 * ULP * np.abs(g["corners_a"]).max()
    assert np.abs(AO.bev_corners(g["boxes_a"]) - g["corners_a"]).max() <= g["meta"]["e_corners"] * (1 + 1e-9)
    if n > 1:
        assert 0 < want.sum() < want.size


@pytest.mark.parametrize("name", golden_files("detaug_frames_*.npz"))
def test_oracle_pipeline_is_the_reference(name):
    g = load_golden(name)
    m = g["meta"]
    assert m["again_frames"] <= 0.05
    for f in range(m["frames"]):
        fr, cands, db = frame_of(g, f)
        for dtype in (np.float64, np.float32):
            got = AO.preprocess(fr["points"], fr["gt_boxes"], fr["gt_classes"], frame_cfg(m), fr["draws"], fr["order"], cands, db, dtype)
            assert np.array_equal(got["accepted"], fr["accepted"]) and np.array_equal(got["gt_classes"], fr["out_classes"])
            assert np.array_equal(got["counts"], fr["counts"])
            tol_p, tol_b = (m["e_points"], m["e_boxes"]) if dtype is np.float64 else (4 * ULP * 80, 4 * ULP * 80)
            assert got["points"].shape == fr["out_points"].shape
            if got["points"].size:
                assert np.abs(got["points"] - fr["out_points"]).max() <= tol_p * (1 + 1e-9)
            if got["gt_boxes"].size:
                assert np.abs(got["gt_boxes"] - fr["out_boxes"]).max() <= tol_b * (1 + 1e-9)


def test_crafted_frame_exercises_every_rule_of_the_scan():
    g = load_golden("detaug_frames_crafted.npz")
    assert list(g["f0_accepted"]) == g["meta"]["expect_accepted"] == [2, 3, 6, 10, 11, 12, 13, 14, 15]
    fr, cands, db = frame_of(g, 0)
    corners = AO.bev_corners(db["boxes"])
    coll = AO.box_collision_test(corners, corners)
    gt = AO.bev_corners(fr["gt_boxes"][fr["gt_classes"] != 0])
    on_gt = AO.box_collision_test(corners, gt).any(1)
    assert on_gt[1] and coll[2, 1] and not on_gt[2]                 # T1 overlaps only T0, which the ground truth rejected: T1 stays
    assert coll[4, 5] and coll[5, 6] and not coll[4, 6] and not on_gt[4:7].any()          # C0, C1 fall to a later candidate, C2 stays
    assert on_gt[7] and on_gt[8]                                    # every bus candidate rejected
    assert coll[9, 3] and not on_gt[9]                              # the trailer falls to the pasted truck
    assert (fr["gt_classes"] == 1).sum() == 2 and len(cands[0]) == 1               # the car group is full and still offered one
    assert (g["f0_gt_classes"] < 0).any() and (g["f0_gt_classes"] == 0).any()


def test_min_points_fixture_drops_boxes():
    g = load_golden("detaug_frames_minpts.npz")
    live = g["f0_gt_classes"] != 0
    assert (g["f0_counts"][live] < 3).any() and (g["f0_counts"][live] >= 3).any()


def test_database_sampler_follows_batch_sampler():
    from link_amd.detaug import DatabaseSampler
    g = load_golden("detaug_sampler.npz")
    s = DatabaseSampler({1: g["meta"]["items"]}, np.random.RandomState(g["meta"]["seed"]))
    want = np.split(g["drawn"], np.cumsum(g["lens"])[:-1])
    assert (g["lens"] < g["asks"]).any()                                      # the wrap rule is in the recording
    for ask, w in zip(g["asks"], want):
        got = s.draw(1, int(ask))
        assert got.dtype == np.int32 and np.array_equal(got, w), (ask, got, w)
    cand, lens = DatabaseSampler({1: [5, 6, 7], 3: []}, np.random.RandomState(0)).candidates(2, [1, 2, 3], [2, 4, 1], 4)
    assert cand.shape == (2, 3, 4) and cand.dtype == np.int32 and lens.dtype == np.int32
    assert lens[:, 1:].sum() == 0 and (lens[:, 0] <= 2).all() and set(cand[cand >= 0]) <= {5, 6, 7}


def test_section_p_abi():
    from link_amd import _lib as L
    lib = L.lib()
    assert L.ABI_VERSION == 13 and lib.link_abi_version() == 13                 # additive entries
    assert lib.link_abi_struct_size(L.STRUCT_DETAUG_SAMPLE_CFG) == ctypes.sizeof(L.LinkDetaugSampleCfg) == 8 + 6 * 4 + 2 * 16 * 4
    assert lib.link_abi_struct_size(L.STRUCT_DETAUG_TRANSFORM_CFG) == ctypes.sizeof(L.LinkDetaugTransformCfg) == 12 * 8 + 8
    P = lib.link_points_in_rbbox
    assert P(None, 5, None, 1, 0, None, 0, 9, None, None, None) == L.LINK_ERR_ARG           # neither mask nor counts
    assert P(None, 2, None, 1, 0, None, 0, 9, 1, None, None) == L.LINK_ERR_ARG              # ndim
    assert P(None, 5, None, 1, 0, None, 0, 6, 1, None, None) == L.LINK_ERR_ARG              # box_len
    assert P(None, 5, None, 2, 0, None, 0, 9, 1, None, None) == L.LINK_ERR_ARG              # a batch needs offsets
    assert P(None, 5, None, 1, 0, None, 0, 9, 1, None, None) == L.LINK_OK                   # no boxes: nothing to do
    assert P(None, 5, None, 1, 10, None, 3, 9, 1, None, None) == L.LINK_ERR_ARG             # null buffers
    assert lib.link_box2d_corners(None, None, None, 0, 0.5, None, None) == L.LINK_OK
    assert lib.link_box2d_corners(None, None, None, 4, 0.5, None, None) == L.LINK_ERR_ARG
    assert lib.link_box2d_corners(None, None, None, 4, float("nan"), None, None) == L.LINK_ERR_ARG
    assert lib.link_box_collision(None, 0, None, 5, 1, None, None) == L.LINK_OK
    assert lib.link_box_collision(None, 3, None, 5, 1, None, None) == L.LINK_ERR_ARG
    assert lib.link_box_collision(None, 1 << 20, None, 1 << 20, 1, None, None) == L.LINK_ERR_ARG
    s = L.LinkDetaugSampleCfg()
    s.rate, s.n_groups, s.max_candidates, s.max_gt, s.box_len = 1.0, 2, 8, 40, 9
    s.group_class[0], s.group_class[1], s.group_max[0], s.group_max[1] = 1, 2, 2, 3
    call = lambda batch=2: lib.link_detaug_sample(ctypes.byref(s), batch, *([None] * 8), 0, *([None] * 8))      # noqa: E731
    assert call(0) == L.LINK_OK and call() == L.LINK_ERR_ARG                      # empty batch; null buffers
    assert lib.link_detaug_sample(None, 1, *([None] * 8), 0, *([None] * 8)) == L.LINK_ERR_ARG
    for field, bad in (("n_groups", 17), ("max_candidates", 65), ("max_gt", 1020), ("box_len", 8), ("rate", -1.0)):
        keep = getattr(s, field)
        setattr(s, field, bad)
        assert call(0) == L.LINK_ERR_ARG, field
        setattr(s, field, keep)
    s.group_class[1] = 0
    assert call(0) == L.LINK_ERR_ARG                                              # classes are 1-based
    t = L.LinkDetaugTransformCfg()
    t.flip_probability, t.max_objs, t.point_capacity = 0.5, 10, 100
    tcall = lambda batch=1, ndim=5, box_len=9: lib.link_detaug_transform(ctypes.byref(t), batch, None, None, None, 0, ndim, None, None, None,      # noqa: E731
                                                                           box_len, None, None, None, 0, None, None, None, None, None, 0,
                                                                           *([None] * 6))
    assert tcall(0) == L.LINK_OK and tcall() == L.LINK_ERR_ARG and tcall(0, ndim=2) == L.LINK_ERR_ARG and tcall(0, box_len=8) == L.LINK_ERR_ARG
    t.flip_probability = 1.5
    assert tcall(0) == L.LINK_ERR_ARG
    t.flip_probability, t.rot_lo = 0.5, float("inf")
    assert tcall(0) == L.LINK_ERR_ARG


def test_detaug_kernels_use_no_scratch():
    """read from the built code object (tools/kernel_regs.py): eight kernels, none spills, the scan's LDS is the avoid set + rows"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_table
    from link_amd import build as hip_build
    hip_build.build()
    rows = kernel_table(os.path.join(ROOT, "link_amd", "lib", "obj", "detaug.o"))
    assert len(rows) == 8, [r[0] for r in rows]
    for name, vgpr, agpr, sgpr, lds, scratch, wg in rows:
        assert int(scratch) == 0 and int(wg) == 256, (name, scratch, wg)
        if "k_detaug_sample" in name:
            assert 1024 * 8 * 4 <= int(lds) <= 40 * 1024, lds
        if "k_points_in_rbbox" in name:
            assert int(lds) == 256 * 8 * 4, lds


def test_public_surface_and_aliases():
    import sys
    import link_amd as la
    for name in ("points_in_rbbox", "points_count_rbbox", "box_collision_test", "center_to_corner_box2d", "GTDatabase", "DatabaseSampler",
                 "DetTrainAugmenter"):
        assert getattr(la, name) is getattr(la.detaug, name)
    assert la.detaug.box_np_ops.points_in_rbbox is la.points_in_rbbox and la.detaug.box_np_ops.points_count_rbbox is la.points_count_rbbox
    assert la.detaug.box_np_ops.center_to_corner_box2d is la.center_to_corner_box2d
    assert la.detaug.sampler_preprocess.box_collision_test is la.box_collision_test
    before = {k for k in sys.modules if k == "det3d" or k.startswith("det3d.")}
    try:
        la.install_as_box_np_ops()
        from det3d.core.bbox import box_np_ops
        from det3d.core.sampler import preprocess as prep
        assert box_np_ops.points_in_rbbox is la.points_in_rbbox and prep.box_collision_test is la.box_collision_test
    finally:
        for k in [k for k in sys.modules if (k == "det3d" or k.startswith("det3d.")) and k not in before]:
            del sys.modules[k]


def _augmenter(**over):
    from link_amd.detaug import DetTrainAugmenter
    kw = dict(class_names=["car", "truck"], sample_groups=[], rate=1.0, global_rot_noise=[-0.78539816, 0.78539816], global_scale_noise=[0.9, 1.1],
              global_translate_std=0.5, min_points_in_gt=-1, pc_range=[-54, -54, -5.0, 54, 54, 3.0], max_objs=50, point_capacity=1000)
    kw.update(over)
    return DetTrainAugmenter(**kw)


def test_refused_options_and_argument_errors():
    from link_amd._lib import LinkAmdError
    from link_amd.detaug import GTDatabase, box_collision_test, center_to_corner_box2d, points_count_rbbox, points_in_rbbox
    a = _augmenter(global_rot_noise=0.3, global_translate_std=[0.1, 0.2, 0.3])
    assert (a._tcfg.rot_lo, a._tcfg.rot_hi) == (-0.3, 0.3) and list(a._tcfg.translate_std) == [0.1, 0.2, 0.3]
    assert a._tcfg.range[2] == 54.0 and a.max_accept == 0
    with pytest.raises(NotImplementedError, match="group sampling"):
        _augmenter(sample_groups=[dict(car=2, truck=3)])
    with pytest.raises(NotImplementedError, match="global_random_rotation_range_per_object"):
        _augmenter(global_random_rotation_range_per_object=[-0.5, 0.5])
    _augmenter(global_random_rotation_range_per_object=[0, 0])
    with pytest.raises(NotImplementedError, match="random_crop"):
        _augmenter(random_crop=True)
    with pytest.raises(NotImplementedError, match="road planes"):
        _augmenter(road_planes=np.zeros(4))
    with pytest.raises(ValueError, match="GTDatabase"):
        _augmenter(sample_groups=[dict(car=2)])
    with pytest.raises(ValueError, match="class_names"):
        _augmenter(sample_groups=[dict(bus=2)])
    with pytest.raises(ValueError):
        _augmenter(flip_probability=1.5)
    with pytest.raises(ValueError):
        _augmenter(pc_range=[0, 1, 2, 3])
    with pytest.raises(ValueError):
        GTDatabase(np.zeros((4, 5)), np.array([0, 2, 3]), np.zeros((2, 9)), np.array([1, 1]))           # offsets do not reach the points
    with pytest.raises(ValueError):
        GTDatabase(np.zeros((4, 5)), np.array([0, 2, 4]), np.zeros((2, 9)), np.array([1, 0]))           # classes are 1-based
    with pytest.raises(LinkAmdError):
        GTDatabase(np.zeros((4, 5)), np.array([0, 2, 4]), np.zeros((2, 9)), np.array([1, 1]), device="cpu")
    pts, boxes = torch.zeros(4, 5), torch.zeros(2, 9)
    for fn in (points_in_rbbox, points_count_rbbox):
        with pytest.raises(LinkAmdError):
            fn(pts, boxes)
        with pytest.raises(LinkAmdError):
            fn(pts.numpy(), boxes.numpy())
    with pytest.raises(LinkAmdError):
        box_collision_test(torch.zeros(2, 4, 2), torch.zeros(3, 4, 2))
    with pytest.raises(LinkAmdError):
        center_to_corner_box2d(torch.zeros(2, 2), torch.ones(2, 2), torch.zeros(2))
    i32 = torch.int32
    with pytest.raises(LinkAmdError):
        a.padded(pts, torch.zeros(2, dtype=i32), torch.zeros(1, 2, 9), torch.zeros(1, 2, dtype=i32), torch.zeros(1, 7), torch.zeros(1, 1000, dtype=i32))
    with pytest.raises(LinkAmdError):
        a([pts], [boxes], [torch.zeros(2, dtype=i32)], torch.zeros(1, 7), torch.zeros(1, 1000, dtype=i32))
