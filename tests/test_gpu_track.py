"""GPU checks of the tracker (section Q, csrc/track.hip): the device against tests/track_oracle.py and the recorded fixtures, exactly,
in every output and every state field -- one sequence, a batch of three with a reset in mid-batch, poses, a captured graph, the
decoder's padded output as input, and the overflow status."""
import os

import numpy as np
import pytest
import torch

import track_oracle as TO
from helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FIX = TO.load_fixtures(os.path.join(ROOT, "tests", "golden"))
NAMES = ["a0", "a1", "a2", "b0", "c0", "d0"]


def expected(fx):
    return {k[4:]: v for k, v in fx.items() if k.startswith("exp_")}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("labels64", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_recorded_lists(name, labels64):
    """S = 1: every frame of every fixture (a2 with its poses, d0 with the overflow status), int32 and int64 labels"""
    meta, fx = FIX[name]
    exp = expected(fx)
    t = TO.make_tracker(meta)
    for f in range(meta["frames"]):
        lab = dev(fx["labels"][f:f + 1], torch.int64 if labels64 else torch.int32)
        out = t.step(dev(fx["boxes"][f:f + 1]), dev(fx["scores"][f:f + 1]), lab, float(fx["time_lag"][f]),
                     pose=fx["pose"][f] if "pose" in fx else None)
        TO.assert_frame(out, 0, exp, f, name)
    host = t.tracks(0)
    n = int(exp["n_tracks"][-1])
    assert np.array_equal(host["ct"], exp["ct"][-1, :n]) and host["id_count"] == int(exp["id_count"][-1])
    if name == "d0":
        assert exp["status"].any() and host["status"] == int(exp["status"][-1])


def test_batch_of_three_sequences_with_a_reset():
    """rows: a1 (12 frames); c0 (10 frames, then empty rows); c0's first five frames, then reset and a1 from its start"""
    (m1, a1), (mc, c0) = FIX["a1"], FIX["c0"]
    assert m1["max_age"] == mc["max_age"] and m1["label_map"] == mc["label_map"]
    e1, ec = expected(a1), expected(c0)
    N = a1["labels"].shape[1]
    t = TO.make_tracker(m1, num_sequences=3)

    def frame(fx, f):
        n = fx["labels"].shape[1]
        b, s, l = np.zeros((N, 9), np.float32), np.zeros(N, np.float32), np.full(N, -1, np.int32)
        if f is not None and f < fx["labels"].shape[0]:
            b[:n], s[:n], l[:n] = fx["boxes"][f], fx["scores"][f], fx["labels"][f]
            return b, s, l, fx["time_lag"][f]
        return b, s, l, 0.5
    empty = {"n_tracks": np.zeros(1, np.int32), "status": np.zeros(1, np.int32), "det_tracking_id": np.full((1, 0), -1, np.int32),
             "det_active": np.zeros((1, 0), np.int32), **{k: np.zeros((1, 1) + ((2,) if k in ("ct", "tracking") else ()), ec[k].dtype) for k in TO.FIELDS}}
    for f in range(12):
        rows = [frame(a1, f), frame(c0, f), frame(c0, f) if f < 5 else frame(a1, f - 5)]
        b, s, l, lag = (np.stack([r[k] for r in rows]) for k in range(4))
        out = t.step(dev(b), dev(s), dev(l), dev(lag.astype(np.float64)), reset=dev(np.array([0, 0, f == 5], np.uint8)))
        TO.assert_frame(out, 0, e1, f, "row 0")
        if f < 10:
            TO.assert_frame(out, 1, ec, f, "row 1")
        else:                                                          # an empty row: no tracks, id_count kept
            TO.assert_frame(out, 1, {**empty, "id_count": ec["id_count"][-1:]}, 0, "row 1 after its end")
        if f < 5:
            TO.assert_frame(out, 2, ec, f, "row 2")
        else:
            TO.assert_frame(out, 2, e1, f - 5, "row 2 after the reset")


def test_pure_translation_and_pure_yaw_leave_the_decisions():
    """a pose run equals the run without a pose on inputs moved beforehand: an integer translation (the float32 sums of the moved
    inputs are within 8e-6 of the float64 ones, the fixture's smallest gaps are 7e-3 to max_dist and 4.6 % between candidates) and
    a quarter turn (exact in both forms)"""
    meta, fx = FIX["a1"]
    assert meta["min_gap_to_max_dist"] > 1e-3 and meta["min_rel_gap_best_second"] > 1e-3
    shift = np.array([[1, 0, 0, 64.0], [0, 1, 0, -32.0], [0, 0, 1, 1.0]])
    turn = np.array([[0, -1.0, 0, 0], [1.0, 0, 0, 0], [0, 0, 1, 0]])
    for what, P in (("translation", shift), ("yaw", turn)):
        with_pose, moved = TO.make_tracker(meta), TO.make_tracker(meta)
        for f in range(meta["frames"]):
            b = fx["boxes"][f:f + 1]
            mb = b.copy()
            mb[..., :3] = (b[..., :3] @ P[:, :3].T.astype(np.float32) + P[:, 3].astype(np.float32)).astype(np.float32)
            mb[..., 6:8] = b[..., 6:8] @ P[:2, :2].T.astype(np.float32)
            args = (dev(fx["scores"][f:f + 1]), dev(fx["labels"][f:f + 1]), float(fx["time_lag"][f]))
            o1 = with_pose.step(dev(b), *args, pose=P)
            o2 = moved.step(dev(mb), *args)
            n = int(o1["n_tracks"][0])
            assert n == int(o2["n_tracks"][0]) and n == int(fx["exp_n_tracks"][f])
            for k in ("det_tracking_id", "det_active", "id_count"):
                assert torch.equal(o1[k], o2[k]), (what, f, k)
            for k in ("label", "tracking_id", "age", "active", "src"):
                assert torch.equal(o1[k][0, :n], o2[k][0, :n]), (what, f, k)
            assert np.array_equal(o1["det_tracking_id"][0].cpu().numpy(), fx["exp_det_tracking_id"][f]), (what, f)
            if what == "yaw":                                          # exact: x' = -y, y' = x
                assert torch.equal(o1["ct"][0, :n], o2["ct"][0, :n]) and torch.equal(o1["tracking"][0, :n], o2["tracking"][0, :n])


def test_step_in_a_captured_graph():
    """time_lag, reset and the detections are written into static tensors between replays; the replays equal the recorded lists
    (which the eager run equals), through a reset in mid-sequence"""
    meta, fx = FIX["a1"]
    exp = expected(fx)
    N = fx["labels"].shape[1]
    t = TO.make_tracker(meta)
    sb, ss = torch.zeros((1, N, 9), device=DEV), torch.zeros((1, N), device=DEV)
    sl = torch.full((1, N), -1, dtype=torch.int32, device=DEV)
    lag, rst = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t.step(sb, ss, sl, lag, reset=rst)                             # the state exists and the allocator is warm
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = t.step(sb, ss, sl, lag, reset=rst)
    t.reset()
    order = [0, 1, 2, 3] + list(range(meta["frames"]))                 # four frames, then a reset and the whole sequence
    for i, f in enumerate(order):
        sb.copy_(dev(fx["boxes"][f:f + 1])); ss.copy_(dev(fx["scores"][f:f + 1])); sl.copy_(dev(fx["labels"][f:f + 1]))
        lag.copy_(dev(fx["time_lag"][f:f + 1])); rst.fill_(1 if i == 4 else 0)
        graph.replay()
        torch.cuda.synchronize()
        TO.assert_frame(out, 0, exp, f, f"replay {i}")


CFG = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
       "nms": {"nms_pre_max_size": 200, "nms_post_max_size": 20, "nms_iou_threshold": 0.2},
       "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075]}


def test_decoder_output_flows_into_the_tracker():
    """CenterHeadDecoder.predict_padded on a small synthetic head output (two frames of two sequences) -> step, nothing copied to the
    host in between; the oracle runs on host copies of the same padded tensors"""
    import link_amd as la
    num_classes = [1, 2, 2, 1, 2, 2]
    B, H, W = 2, 16, 16
    gen = torch.Generator().manual_seed(3)

    def maps(K):
        return {"reg": torch.rand(B, 2, H, W, generator=gen), "height": torch.randn(B, 1, H, W, generator=gen), "dim": torch.randn(B, 3, H, W, generator=gen) * 0.3,
                "rot": torch.randn(B, 2, H, W, generator=gen), "hm": torch.randn(B, K, H, W, generator=gen) * 1.5 - 3.0,
                "vel": torch.randn(B, 2, H, W, generator=gen)}
    first = [maps(K) for K in num_classes]
    second = [{**pd, "reg": pd["reg"] + 0.5 * pd["vel"] / 0.6} for pd in first]        # the objects moved by vel * lag (cells of 0.6 m)
    dec = la.CenterHeadDecoder(CFG, num_classes)
    t = la.CenterTracker.nuscenes(max_age=3, capacity=256, num_sequences=B)
    oracles = [TO.OracleTracker(t.label_map, t.max_dist, 3) for _ in range(B)]
    matched = 0
    for preds in (first, second, first):
        pad = dec.predict_padded([{k: v.to(DEV) for k, v in pd.items()} for pd in preds])
        assert pad["label_preds"].dtype == torch.int64 and pad["box3d_lidar"].shape == (B, 6 * 20, 9)
        out = t.step(pad, time_lag=0.5)
        hb, hs, hl = pad["box3d_lidar"].cpu().numpy(), pad["scores"].cpu().numpy(), pad["label_preds"].cpu().numpy()
        for s in range(B):
            ids, act = oracles[s].step(hb[s], hs[s], hl[s], 0.5)
            a = oracles[s].arrays()
            n = a["label"].shape[0]
            assert n > 10 and int(out["n_tracks"][s]) == n and int(out["id_count"][s]) == oracles[s].id_count
            assert np.array_equal(out["det_tracking_id"][s].cpu().numpy(), ids) and np.array_equal(out["det_active"][s].cpu().numpy(), act)
            for k in TO.FIELDS:
                assert np.array_equal(out[k][s, :n].cpu().numpy(), a[k]), k
            matched += int((act >= 2).sum())
    assert matched > 0
