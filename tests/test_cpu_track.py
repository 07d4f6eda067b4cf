"""CPU checks of the tracker (section Q): the numpy restatement against the fixtures recorded from the reference's trackers, the
per-class decomposition, the ABI entries and their argument checks, and CenterTracker's CPU composition."""
import ctypes
import os

import numpy as np
import pytest
import torch

import track_oracle as TO
from helpers import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = TO.load_fixtures(GOLDEN)
NAMES = ["a0", "a1", "a2", "b0", "c0", "d0"]


def oracle_for(meta, **kw):
    return TO.OracleTracker(meta["label_map"], meta["max_dist"], meta["max_age"], meta["score_thresh"], capacity=meta.get("capacity"), **kw)


def test_fixture_set_is_complete():
    assert sorted(FIX) == NAMES
    seen = set()
    for name, (meta, fx) in FIX.items():
        assert 8 <= meta["frames"] <= 12 and meta["source"] == ("restatement" if name == "d0" else "reference"), name
        seen |= set(meta["n_per_frame"])
    assert {0, 1, 63, 64, 65} <= seen and any(240 <= n <= 300 for n in seen)
    d0 = FIX["d0"][0]
    assert {64, 65, 96} <= set(d0["n_tracks_per_frame"]) and FIX["d0"][1]["exp_status"].any() and not FIX["d0"][1]["exp_status"].all()
    assert FIX["a0"][0]["max_age"] == 0 and FIX["a1"][0]["max_age"] == 3 and "pose" in FIX["a2"][1]
    lag = FIX["a0"][1]["time_lag"]
    assert (lag.astype(np.float32).astype(np.float64) != lag).all() and lag.min() >= 0.45 and lag.max() <= 0.55
    sc = FIX["b0"][1]["scores"][FIX["b0"][1]["labels"] >= 0]
    assert (sc > 0.1).any() and (sc < 0.1).any()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_recorded_lists(name):
    """ids, active, age, list order, id_count and the float64 ct of every frame, exactly"""
    meta, fx = FIX[name]
    rec = TO.run_sequence(oracle_for(meta), fx)
    for k, v in rec.items():
        assert v.dtype == fx["exp_" + k].dtype and np.array_equal(v, fx["exp_" + k]), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_per_class_scans_equal_the_single_scan(name):
    meta, fx = FIX[name]
    rec = TO.run_sequence(oracle_for(meta, per_class=True), fx)
    for k, v in rec.items():
        assert np.array_equal(v, fx["exp_" + k]), (name, k)


def test_crafted_frames_decide_as_designed():
    meta, fx = FIX["c0"]
    ids, act, age, n = fx["exp_det_tracking_id"], fx["exp_active"], fx["exp_age"], fx["exp_n_tracks"]
    assert list(ids[0][:8]) == [1, 2, 3, 4, 5, 6, 7, 8]                 # a first frame with no track
    # identical position: the first wins; equidistant: the first wins; == max_dist matches; one ulp above does not; the class decides
    assert list(ids[1][:5]) == [1, 3, 5, 9, 7]
    assert n[2] == 0 and fx["exp_id_count"][2] == 9                     # untracked classes only
    assert list(fx["exp_tracking_id"][5][:3]) == [12, 10, 11] and list(age[5][:3]) == [1, 3, 3]
    assert list(ids[6][:2]) == [12, 10] and list(act[6][:2]) == [4, 1] and n[6] == 2      # revived with active 1; the other aged out
    assert n[7] == 0 and fx["exp_id_count"][7] == 12 and list(ids[8][:2]) == [13, 14]     # an empty frame keeps id_count


def test_abi_entries():
    from link_amd import _lib as L
    from link_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in ("link_track_state_bytes", "link_track_step"):
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    lib = L.lib()
    assert lib.link_abi_version() == L.ABI_VERSION == 13
    assert lib.link_abi_struct_size(L.STRUCT_TRACK_CFG) == ctypes.sizeof(L.LinkTrackCfg) == 6 * 4 + 2 * 32 * 4
    assert "track.hip" in SOURCES
    assert lib.link_track_state_bytes(1024) == 32 + 2 * 52 * 1024 and lib.link_track_state_bytes(1) == 32 + 104
    assert lib.link_track_state_bytes(0) == 0 and lib.link_track_state_bytes(1025) == 0


def test_argument_checks_return_before_any_launch():
    import link_amd
    from link_amd import _lib as L
    lib = L.lib()
    t = link_amd.CenterTracker.nuscenes(capacity=96)
    p = 0x1000                                     # never dereferenced: every case below is refused on the host

    def call(cfg=t.cfg, S=1, N=8, C=9, boxes=p, scores=p, labels=p, lag=p, state=p, ids=p, act=p):
        return lib.link_track_step(ctypes.byref(cfg) if cfg is not None else None, S, N, C, boxes, scores, labels, 1, None, lag, None, None, state,
                                   ids, act, None)
    assert call(cfg=None) == L.LINK_ERR_ARG
    for k in ("boxes", "scores", "labels", "lag", "state", "ids", "act"):
        assert call(**{k: None}) == L.LINK_ERR_ARG, k
    assert call(N=97) == L.LINK_ERR_ARG            # capacity below N
    assert call(C=5) == L.LINK_ERR_ARG and call(S=-1) == L.LINK_ERR_ARG and call(N=-1) == L.LINK_ERR_ARG
    assert call(S=0) == L.LINK_OK                  # nothing to do, nothing launched

    def cfg_with(**kw):
        c = L.LinkTrackCfg.from_buffer_copy(t.cfg)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c
    for bad in (dict(label_map=(0, 7)), dict(label_map=(3, -2)), dict(n_det_labels=0), dict(n_det_labels=33), dict(n_track_labels=0),
                dict(n_track_labels=33), dict(max_dist=(2, -1.0)), dict(max_dist=(2, float("nan"))), dict(max_dist=(2, 1e17)),
                dict(capacity=0), dict(capacity=1025), dict(max_age=-1)):
        assert call(cfg=cfg_with(**bad)) == L.LINK_ERR_ARG, bad
    with pytest.raises(ValueError):
        link_amd.CenterTracker([0, 2], [1.0, 1.0])
    with pytest.raises(ValueError):
        link_amd.CenterTracker([0], [1.0], capacity=2000)
    with pytest.raises(NotImplementedError):
        link_amd.CenterTracker([0], [1.0], hungarian=True)
    with pytest.raises(ValueError):
        t.step(torch.zeros(1, 97, 9), torch.zeros(1, 97), torch.zeros(1, 97, dtype=torch.int64), 0.5)


def test_presets_restate_the_reference_tables():
    import link_amd
    from link_amd import tracker as T
    t = link_amd.CenterTracker.nuscenes()
    meta = FIX["a1"][0]                            # recorded by a maker that checked both tables against the reference's
    assert t.label_map == meta["label_map"] and t.max_dist == [float(v) for v in meta["max_dist"]] and t.max_age == 3
    assert t.score_thresh is None and len(T.NUSCENES_DETECTION_NAMES) == 10 and len(T.NUSCENES_TRACKING_NAMES) == 7
    w = link_amd.CenterTracker.waymo({"VEHICLE": 0.8, "PEDESTRIAN": 0.4, "CYCLIST": 0.6})
    assert w.label_map == [0, 1, 2] and w.score_thresh == 0.1 and w.max_age == 0


@pytest.mark.parametrize("name", NAMES)
def test_cpu_composition_equals_the_oracle(name):
    meta, fx = FIX[name]
    t = TO.make_tracker(meta)
    for f in range(meta["frames"]):
        out = t.step(torch.from_numpy(fx["boxes"][f:f + 1]), torch.from_numpy(fx["scores"][f:f + 1]), torch.from_numpy(fx["labels"][f:f + 1]),
                     float(fx["time_lag"][f]), pose=fx["pose"][f] if "pose" in fx else None)
        TO.assert_frame(out, 0, {k[4:]: v for k, v in fx.items() if k.startswith("exp_")}, f, name)
    host = t.tracks(0)
    n = int(fx["exp_n_tracks"][-1])
    assert np.array_equal(host["ct"], fx["exp_ct"][-1, :n]) and host["id_count"] == int(fx["exp_id_count"][-1])


def test_cpu_batch_reset_counts_and_no_sequences():
    """three rows at once with a reset in mid-batch, `counts` instead of -1 labels, one frame's dict, and S = 0"""
    import link_amd
    meta, fx = FIX["a2"]
    exp = {k[4:]: v for k, v in fx.items() if k.startswith("exp_")}
    t = TO.make_tracker(meta, num_sequences=3)
    solo = TO.make_tracker(meta)
    for f in range(4):
        rows = [f, max(f - 1, 0), f]
        b, s, l = (torch.from_numpy(np.stack([fx[k][r] for r in rows])) for k in ("boxes", "scores", "labels"))
        if f == 0:
            l[1] = -1                                                  # row 1 starts one frame late: an empty row while the others run
        out = t.step(b, s, l.long(), torch.from_numpy(fx["time_lag"][rows]), reset=[False, False, f == 2], pose=fx["pose"][rows])
        TO.assert_frame(out, 0, exp, f, "row 0")
        if f >= 1:
            TO.assert_frame(out, 1, exp, f - 1, "row 1")
        if f == 2:                                                     # the reset row starts over at frame 2: a fresh tracker's first frame
            ref = solo.step(b[2:3], s[2:3], l[2:3], float(fx["time_lag"][f]), pose=fx["pose"][f])
            for k in ref:
                assert torch.equal(ref[k][0], out[k][2]), k
    # counts: the same frames packed to the front
    meta, fx = FIX["a0"]
    exp = {k[4:]: v for k, v in fx.items() if k.startswith("exp_")}
    t = TO.make_tracker(meta)
    for f in range(meta["frames"]):
        n = int((fx["labels"][f] >= 0).sum())
        lab = torch.from_numpy(fx["labels"][f:f + 1]).clone()
        lab[lab < 0] = 0                                               # stale labels behind the count
        out = t.step(torch.from_numpy(fx["boxes"][f:f + 1]), torch.from_numpy(fx["scores"][f:f + 1]), lab, float(fx["time_lag"][f]),
                     counts=torch.tensor([n], dtype=torch.int32))
        TO.assert_frame(out, 0, exp, f, "counts")
    t.reset()
    out = t.step({"box3d_lidar": torch.from_numpy(fx["boxes"][0]), "scores": torch.from_numpy(fx["scores"][0]),
                  "label_preds": torch.from_numpy(fx["labels"][0]).long()}, time_lag=float(fx["time_lag"][0]))
    assert out["det_tracking_id"].shape == (fx["labels"].shape[1],)
    TO.assert_frame(out, 0, exp, 0, "dict")
    none = link_amd.CenterTracker.nuscenes(num_sequences=0)
    out = none.step(torch.zeros(0, 5, 9), torch.zeros(0, 5), torch.zeros(0, 5, dtype=torch.int64), torch.zeros(0, dtype=torch.float64))
    assert out["det_tracking_id"].shape == (0, 5) and out["n_tracks"].shape == (0,)


def test_boxes_to_global_is_its_float64_definition():
    import link_amd
    rng = np.random.default_rng(5)
    fx = FIX["a2"][1]
    boxes = torch.from_numpy(fx["boxes"][:3])
    pose = fx["pose"][:3]
    out = link_amd.boxes_to_global(boxes, pose).numpy()
    assert out.dtype == np.float64
    b = fx["boxes"][:3].astype(np.float64)
    for s in range(3):
        P = pose[s]
        for r in range(3):
            want = ((P[4 * r] * b[s, :, 0] + P[4 * r + 1] * b[s, :, 1]) + P[4 * r + 2] * b[s, :, 2]) + P[4 * r + 3]
            assert np.array_equal(out[s, :, r], want)
        assert np.array_equal(out[s, :, 6], P[0] * b[s, :, 6] + P[1] * b[s, :, 7]) and np.array_equal(out[s, :, 7], P[4] * b[s, :, 6] + P[5] * b[s, :, 7])
        assert np.array_equal(out[s, :, 8], b[s, :, 8] + np.arctan2(P[4], P[0])) and np.array_equal(out[s, :, 3:6], b[s, :, 3:6])
    # a pure yaw about z: a heading along the lidar's x axis points along the turned axis, and the speed is kept
    yaw = 0.3
    P = np.array([[np.cos(yaw), -np.sin(yaw), 0, 5], [np.sin(yaw), np.cos(yaw), 0, -2], [0, 0, 1, 0.5]])
    one = link_amd.boxes_to_global(torch.tensor([[1.0, 0, 0, 2, 4, 1.5, 3.0, 0.0, 0.0]]), P).numpy()[0]
    assert np.allclose(one[[0, 1, 2]], [5 + np.cos(yaw), -2 + np.sin(yaw), 0.5]) and np.isclose(one[8], yaw)
    assert np.allclose(one[6:8], [3 * np.cos(yaw), 3 * np.sin(yaw)]) and rng is not None
