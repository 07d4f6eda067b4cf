"""GPU checks of the CenterHead test-time augmentation (csrc/dettta.hip, section N of include/link_amd.h; link_amd/dettta.py) against
the restatements of tests/tta_oracle.py and the fixtures of tests/golden/make_golden_dettta.py.

Tolerance of the decode and the rotations (tta_oracle.gate): the arbiter is the float64 evaluation of the reference's formula on
the same fp32 inputs; per component the device may be at most 4 x as far from it as the float32 restatement of the reference is
(floor: one fp32 ulp), errors relative to the value, or to the component's mean magnitude where the value is smaller.  Labels,
masks, counts, kept sets and their order are compared exactly.  Each case's two errors go to dettta_parity.jsonl in the directory
LINK_AMD_PARITY_DIR names (profiles/dettta_parity.jsonl is one run)."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden
from ref64 import record_row

import box_oracle as BO
import tta_oracle as TO
import voxel_oracle as VO

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 83,
                                                                                      "nms_iou_threshold": 0.2},
       "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075], "double_flip": True}
ANGLES = [0.0, 0.3925, -0.785]
FUSE_CASES = [(0, 1, 2), (1, 1, 2), (64, 3, 2), (65, 3, 3), (1000, 10, 3), (1000, 3, 2)]


def _record(test, case, names, e_dev, e_ref):
    for name, d, r in zip(names, np.atleast_1d(e_dev), np.atleast_1d(e_ref)):
        record_row({"test": test, **case, "component": name, "e_dev": float(d), "e_ref32": float(r),
                    "bound": float(max(4 * r, 2.0 ** -23))}, name="dettta_parity.jsonl")


# ---- views ----------------------------------------------------------------------------------------------------------------------
def _clouds(sizes, C, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.uniform(-54, 54, (n, 2)), rng.uniform(-5, 3, (n, 1)), rng.uniform(0, 1, (n, C - 3))], 1).astype(np.float32)
            for n in sizes]


@pytest.mark.parametrize("sizes", [(0,), (1,), (257,), (5003,), (257, 0, 5003), (0, 1, 257)])
@pytest.mark.parametrize("C", [4, 5])
def test_views(sizes, C):
    import link_amd as la
    clouds = _clouds(sizes, C, 3 + C + sum(sizes))
    dev = [torch.from_numpy(c).to(DEV) for c in clouds]
    for angle in ANGLES:
        v = la.tta_views(dev, angle)
        assert len(v) == 4 * len(sizes) and v.packed.shape == (4 * sum(sizes), C)
        want_off = np.concatenate([[0], np.cumsum(np.repeat(sizes, 4))])
        assert np.array_equal(v.offsets.cpu().numpy(), want_off)
        got = [t.cpu().numpy() for t in v]
        r32, r64 = TO.views(clouds, angle, np.float32), TO.views(clouds, angle, np.float64)
        for b, src in enumerate(clouds):
            g0, g1, g2, g3 = got[4 * b:4 * b + 4]
            assert g0.shape == src.shape
            assert g0[:, 2:].tobytes() == src[:, 2:].tobytes()                          # columns 2.. are copies
            if angle == 0:
                assert g0.tobytes() == src.tobytes()                                    # angle 0: bit for bit
            for g, flip in ((g1, (1,)), (g2, (0,)), (g3, (0, 1))):                      # flips: copies with exact sign changes
                want = g0.copy()
                for c in flip:
                    want[:, c] = -want[:, c]
                assert g.tobytes() == want.tobytes()
        if angle != 0 and sum(sizes):
            cat = lambda parts: np.concatenate([p[:, :2] for p in parts[0::4]])        # noqa: E731
            ok, e_dev, e_ref = TO.gate(cat(got), cat(r32), cat(r64))
            _record("views", {"sizes": list(sizes), "C": C, "angle": angle}, ["x", "y"], e_dev, e_ref)
            print(f"views {sizes} C{C} angle {angle}: e_dev {e_dev}, e_ref32 {e_ref}")
            assert ok, (e_dev, e_ref)


def test_views_from_a_packed_tensor_and_through_the_voxelizer():
    """the device views, voxelised by Voxelizer, equal the oracle voxeliser run on those same device views, exactly"""
    import link_amd as la
    sizes = (257, 5003, 1)
    clouds = _clouds(sizes, 5, 77)
    packed = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    v = la.tta_views(packed, 0.3925, sizes=sizes)
    w = la.tta_views([torch.from_numpy(c).to(DEV) for c in clouds], 0.3925)
    assert torch.equal(v.packed, w.packed) and torch.equal(v.offsets, w.offsets)
    vs, rng, max_points, max_voxels = [0.075, 0.075, 0.2], [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], 10, 20000
    vox = la.Voxelizer(vs, rng, max_points, max_voxels)
    voxels, feats, coors, num, voff = vox.generate_padded(v, return_voxels=True)
    voff = voff.cpu().numpy()
    assert len(voff) == 4 * len(sizes) + 1
    for i, view in enumerate(v):
        want_v, want_c, want_n = VO.hard(view.cpu().numpy(), vs, rng, max_points, max_voxels)
        sl = slice(int(voff[i]), int(voff[i + 1]))
        assert sl.stop - sl.start == want_c.shape[0]
        assert np.array_equal(coors[sl, 1:].cpu().numpy(), want_c) and (coors[sl, 0] == i).all()
        assert np.array_equal(num[sl].cpu().numpy(), want_n) and voxels[sl].cpu().numpy().tobytes() == want_v.tobytes()


# ---- decode ---------------------------------------------------------------------------------------------------------------------
def _unflip(t, v):
    """a [B, C, H, W] map of view v in the frame's own coordinates (center_head.py:333-335); its own inverse"""
    return t if v == 0 else torch.flip(t, dims={1: [2], 2: [3], 3: [2, 3]}[v])


def _offending(pd, cfg, B, K):
    """[B, H W] bool: the cells whose decisions or conditioning are too close (the redraw rule of the issue)"""
    boxes, _, scores, _, hm = TO.decode(pd, cfg, torch.float64)
    r = torch.tensor(cfg["post_center_limit_range"], dtype=torch.float64)
    close = (scores - cfg["score_threshold"]).abs() < 1e-4
    close |= ((boxes[..., :3] - r[:3]).abs() < 1e-4).any(-1) | ((boxes[..., :3] - r[3:]).abs() < 1e-4).any(-1)
    if K > 1:
        top2 = hm.topk(2, dim=-1)[0]
        close |= (top2[..., 0] - top2[..., 1]) < 1e-5
    rot = pd["rot"].double().reshape(B, 4, 2, *pd["rot"].shape[2:])
    sgn_s, sgn_c = (1, 1, -1, -1), (1, -1, 1, -1)
    s = sum(sgn_s[v] * _unflip(rot[:, v], v)[:, 0] for v in range(4)) / 4
    c = sum(sgn_c[v] * _unflip(rot[:, v], v)[:, 1] for v in range(4)) / 4
    close |= (torch.hypot(s, c) < 0.05).reshape(B, -1)
    close |= boxes[..., -1].abs() > math.pi - 1e-3
    return close


def _tta_maps(B, H, W, K, vel, seed, cfg):
    """Random head maps of batch 4 B (asymmetric by construction), redrawn -- the offending cells only, in all four views -- until no
    averaged score lies within 1e-4 of the threshold, no centre within 1e-4 of the range, no two averaged class scores within 1e-5,
    every averaged (sin, cos) has norm >= 0.05 and no heading lies within 1e-3 of +-pi"""
    gen = torch.Generator().manual_seed(seed)
    draw = {"reg": lambda: torch.rand(4 * B, 2, H, W, generator=gen), "height": lambda: torch.randn(4 * B, 1, H, W, generator=gen) * 8 - 1,
            "rot": lambda: torch.randn(4 * B, 2, H, W, generator=gen), "hm": lambda: torch.randn(4 * B, K, H, W, generator=gen) * 1.5 - 3.0}
    pd = {k: f() for k, f in draw.items()}
    pd["dim"] = torch.randn(4 * B, 3, H, W, generator=gen) * 0.5
    if vel:
        pd["vel"] = torch.randn(4 * B, 2, H, W, generator=gen)
    for _ in range(30):
        close = _offending(pd, cfg, B, K)
        if not close.any():
            return pd
        cell = close.view(B, 1, 1, H, W).expand(B, 4, 1, H, W).clone()
        for v in range(1, 4):                                # the cell's place in the maps of view v
            cell[:, v] = _unflip(cell[:, v], v)
        cell = cell.reshape(4 * B, 1, H, W)
        for k, f in draw.items():
            pd[k] = torch.where(cell, f(), pd[k])
    raise AssertionError("could not draw maps away from the decision boundaries")


_SMALL = [(H, W, K, vel, B) for (H, W) in ((8, 12), (7, 5), (33, 19)) for K in (1, 3) for vel in (False, True) for B in (1, 2)]


@pytest.mark.parametrize("H,W,K,vel,B", _SMALL + [(180, 180, 3, True, 1)])
def test_decode_flip4(H, W, K, vel, B):
    import link_amd as la
    pd = _tta_maps(B, H, W, K, vel, 11 + 2 * K + vel + 5 * H + B, CFG)
    assert not _offending(pd, CFG, B, K).any()
    rb, rl, rs, rmask, _ = TO.decode(pd, CFG, torch.float32)
    tb, _, ts, _, _ = TO.decode(pd, CFG, torch.float64)
    share = float(rmask.float().mean())
    assert 0 < share < 1, share
    dec = la.CenterHeadTTADecoder(CFG, [K])
    boxes, labels, scores, counts = dec.decode({k: v.to(DEV) for k, v in pd.items()})
    C = 9 if vel else 7
    assert boxes.shape == (B, H * W, C) and labels.dtype == torch.int32 and scores.shape == (B, H * W) and counts.shape == (B,)
    mask = (scores > float("-inf")).cpu()
    assert torch.equal(mask, rmask)
    assert torch.equal(labels.cpu().long(), rl)
    assert torch.equal(counts.cpu().long(), rmask.sum(1))
    names = ["x", "y", "z", "dx", "dy", "dz"] + (["vx", "vy"] if vel else []) + ["heading"]
    ok_b, e_dev, e_ref = TO.gate(boxes.cpu().numpy(), rb.numpy(), tb.numpy())
    ok_s, s_dev, s_ref = TO.gate(scores.cpu()[rmask].numpy()[:, None], rs[rmask].numpy()[:, None], ts[rmask].numpy()[:, None])
    case = {"H": H, "W": W, "K": K, "vel": vel, "B": B, "unmasked": share}
    _record("decode", case, names + ["score"], np.concatenate([e_dev, s_dev]), np.concatenate([e_ref, s_ref]))
    for n, d, r in zip(names + ["score"], np.concatenate([e_dev, s_dev]), np.concatenate([e_ref, s_ref])):
        print(f"decode {case} {n}: e_dev {d:.3e} e_ref32 {r:.3e} ratio {d / max(r, 1e-30):.2f}")
    assert ok_b, (e_dev, e_ref)
    assert ok_s, (s_dev, s_ref)


# ---- predict --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def head_case4():
    """harness.bevhead.BevHalf on a seeded random BEV tensor of batch 4 (one frame's four views), prepared as the head_case of
    tests/test_gpu_boxnms.py: maps spread to unit variance, the heat map's logits evenly spaced in the head's own order with the
    top 1 800 above the threshold -- a view's score must pass 0.4 for the mean of four to pass 0.1, which leaves several hundred
    candidates per task"""
    from harness.bevhead import BevHalf
    torch.manual_seed(21)
    net = BevHalf(256).to(DEV).eval()
    bev = torch.randn(4, 256, 180, 180, generator=torch.Generator().manual_seed(22)).to(DEV)
    with torch.no_grad():
        preds = net(bev)
        thr_logit = float(np.log(CFG["score_threshold"] / (1 - CFG["score_threshold"])))
        for pd in preds:
            for k in pd:
                pd[k] = (pd[k] - pd[k].mean((0, 2, 3), keepdim=True)) / pd[k].std((0, 2, 3), keepdim=True)
            flat = pd["hm"].reshape(-1)
            N = flat.numel()
            rank = torch.empty(N, device=DEV)
            rank[flat.argsort(stable=True)] = torch.arange(N, dtype=torch.float32, device=DEV)
            pd["hm"] = (thr_logit + (rank - (N - 1800) + 0.5) * 2e-3).reshape(pd["hm"].shape)
            pd["reg"] = pd["reg"].sigmoid()
            pd["dim"] = (pd["dim"] * 0.6).clamp(-1.5, 2.0)
            pd["height"] = pd["height"].tanh() * 3
    return preds


def _kept_by_oracle(dec, preds):
    """per task: (boxes, scores, labels of the unmasked cells as the device decoded them, the oracle's kept indices into them)"""
    out = []
    for pd in preds:
        boxes, labels, scores, counts = dec.decode(pd)
        assert boxes.shape[0] == 1
        mask = scores[0] > float("-inf")
        bp, sc, lab = boxes[0][mask].cpu().numpy(), scores[0][mask].cpu().numpy(), labels[0][mask].cpu().numpy()
        assert int(counts[0]) == len(sc) and 100 <= len(sc) and len(np.unique(sc)) == len(sc), len(sc)
        sel = TO.nms_pcdet(bp, sc, CFG["nms"]["nms_iou_threshold"], CFG["nms"]["nms_pre_max_size"], CFG["nms"]["nms_post_max_size"])
        out.append((bp, sc, lab, sel))
    return out


@pytest.mark.parametrize("rot", [0.0, 0.3925])
def test_predict_and_predict_padded(head_case4, rot):
    import link_amd as la
    preds = head_case4
    num_classes = [pd["hm"].shape[1] for pd in preds]
    dec = la.CenterHeadTTADecoder(dict(CFG, tt_rotation=rot), num_classes)
    plain = la.CenterHeadTTADecoder(CFG, num_classes)                    # the unrotated decoder: the same decoded boxes, the same NMS
    kept = _kept_by_oracle(plain, preds)
    out = dec.predict(preds)
    pad = dec.predict_padded(preds)
    post = CFG["nms"]["nms_post_max_size"]
    C = kept[0][0].shape[1]
    assert len(out) == 1 and pad["box3d_lidar"].shape == (1, len(preds) * post, C) and pad["counts"].shape == (1, len(preds))
    flag, want_b, want_s, want_l, dev_rows = 0, [], [], [], []
    for t, (bp, sc, lab, sel) in enumerate(kept):
        pc = int(pad["counts"][0, t])
        assert pc == len(sel) and 0 < pc, (t, pc, len(sel))
        sl = slice(t * post, t * post + pc)
        assert np.array_equal(pad["scores"][0, sl].cpu().numpy(), sc[sel])                  # the kept set and its order
        assert np.array_equal(pad["label_preds"][0, sl].cpu().numpy(), lab[sel] + flag)
        assert (pad["label_preds"][0, t * post + pc:(t + 1) * post] == -1).all()
        assert (pad["box3d_lidar"][0, t * post + pc:(t + 1) * post] == 0).all()
        want_b.append(bp[sel]); want_s.append(sc[sel]); want_l.append(lab[sel] + flag)
        dev_rows.append(pad["box3d_lidar"][0, sl].cpu().numpy())
        flag += num_classes[t]
    want_b, dev_rows = np.concatenate(want_b), np.concatenate(dev_rows)
    assert np.array_equal(out[0]["scores"].cpu().numpy(), np.concatenate(want_s))
    assert np.array_equal(out[0]["label_preds"].cpu().numpy(), np.concatenate(want_l))
    assert out[0]["label_preds"].dtype == torch.int64 and out[0]["metadata"] is None
    assert np.array_equal(out[0]["box3d_lidar"].cpu().numpy(), dev_rows)                    # predict == the padded form's used slots
    if rot == 0:
        assert np.array_equal(dev_rows, want_b)                                             # no rotation: the decoded rows themselves
    else:
        ok, e_dev, e_ref = TO.gate(dev_rows, TO.rotate_back(want_b, rot, np.float32), TO.rotate_back(want_b, rot, np.float64))
        names = ["x", "y", "z", "dx", "dy", "dz", "vx", "vy", "heading"]
        _record("rotate_back", {"rows": int(len(want_b)), "angle": rot}, names, e_dev, e_ref)
        print("rotate back: e_dev", e_dev, "e_ref32", e_ref)
        assert ok, (e_dev, e_ref)
        assert np.array_equal(dev_rows[:, 2:6], want_b[:, 2:6])                             # z and the extents are copies


def test_predict_padded_and_fusion_in_a_captured_graph(head_case4):
    import link_amd as la
    preds = head_case4
    dec = la.CenterHeadTTADecoder(dict(CFG, tt_rotation=0.3925), [pd["hm"].shape[1] for pd in preds])

    def step():
        p = dec.predict_padded(preds)
        valid = p["label_preds"][0] >= 0
        n_dev = valid.sum().to(torch.int32).reshape(1)
        order = torch.sort(valid.to(torch.int32), descending=True, stable=True)[1]          # the used slots first
        fused = la.fuse_detections_padded(p["box3d_lidar"][0][order], p["scores"][0][order], p["label_preds"][0][order], [0.1] * 10,
                                          max_dets=200, n_dev=n_dev)
        return p, fused
    eager, eager_f = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                       # warm the allocator and the kept tables on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, captured_f = step()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], captured[k]), k
    for a, b in zip(eager_f, captured_f):
        assert torch.equal(a, b)
    assert 0 < int(eager_f[3]) <= 200


# ---- class-wise NMS and fusion --------------------------------------------------------------------------------------------------
def _passes(g):
    m = g["meta"]
    edges = [0] + m["split"] + [len(g["scores"])]
    return [{"box3d_lidar": torch.from_numpy(g["boxes"][a:b]).to(DEV), "scores": torch.from_numpy(g["scores"][a:b]).to(DEV),
             "label_preds": torch.from_numpy(g["labels"][a:b]).to(DEV)} for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("n,ncls,npass", FUSE_CASES)
def test_fuse_detections(n, ncls, npass):
    import link_amd as la
    g = load_golden(f"dettta_fuse_{n}_c{ncls}_p{npass}.npz")
    m = g["meta"]
    passes = _passes(g)
    assert len(passes) == npass and len(np.unique(g["scores"])) == n
    keep = g["keep"]
    for max_dets in (500, max(1, len(keep) // 3)):                    # the second: fewer than the kept count
        want = keep[:max_dets]
        boxes, scores, labels = la.fuse_detections(passes, m["thresholds"], max_dets=max_dets)
        assert boxes.shape == (len(want), 9) and labels.dtype == torch.int64
        assert np.array_equal(scores.cpu().numpy(), g["scores"][want])
        assert np.array_equal(labels.cpu().numpy(), g["labels"][want]) and np.array_equal(boxes.cpu().numpy(), g["boxes"][want])
        # the padded form: the same boxes in front of a tail of junk that n_dev excludes
        cat = {k: torch.cat([p[k] for p in passes]) for k in passes[0]}
        junk = 13
        pb = torch.cat([cat["box3d_lidar"], cat["box3d_lidar"].new_full((junk, 9), 2.0)])
        ps = torch.cat([cat["scores"], cat["scores"].new_full((junk,), 9.0)])
        pl = torch.cat([cat["label_preds"], cat["label_preds"].new_zeros(junk)])
        n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
        ob, os_, ol, count = la.fuse_detections_padded(pb, ps, pl, m["thresholds"], max_dets=max_dets, n_dev=n_dev)
        c = int(count.item())
        assert c == len(want) and ob.shape == (max_dets, 9)
        assert np.array_equal(os_[:c].cpu().numpy(), g["scores"][want]) and np.array_equal(ol[:c].cpu().numpy(), g["labels"][want])
        assert np.array_equal(ob[:c].cpu().numpy(), g["boxes"][want]) and (ol[c:] == -1).all() and (ob[c:] == 0).all()


@pytest.mark.parametrize("n,ncls,npass", [(65, 3, 3), (1000, 10, 3)])
def test_classwise_mask_words_equal_the_reference_decisions(n, ncls, npass):
    from link_amd import _lib as L
    g = load_golden(f"dettta_fuse_{n}_c{ncls}_p{npass}.npz")
    thrs = np.asarray(g["meta"]["thresholds"], np.float32)
    order = np.argsort(-g["scores"], kind="stable")
    p = BO.to_pcdet(g["boxes"][order][:, [0, 1, 2, 3, 4, 5, -1]])
    lab = g["labels"][order]
    iou = np.zeros((n, n), np.float32)
    r = 0.5 * np.hypot(p[:, 3], p[:, 4]) + 0.05
    near = np.argwhere(np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) <= r[:, None] + r[None, :])
    iou[near[:, 0], near[:, 1]] = BO.iou_bev(p[near[:, 0]], p[near[:, 1]])
    sup = (lab[:, None] == lab[None, :]) & (iou > thrs[lab][:, None])
    nblk = (n + 63) // 64
    mask = torch.full((n, nblk), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    dp, dl, dt = torch.from_numpy(p).to(DEV), torch.from_numpy(lab.astype(np.int32)).to(DEV), torch.from_numpy(thrs).to(DEV)
    L.check(L.lib().link_nms_mask_classwise(dp.data_ptr(), dl.data_ptr(), n, None, dt.data_ptr(), ncls, mask.data_ptr(),
                                            L.current_stream_handle()), "mask")
    torch.cuda.synchronize()
    got = mask.cpu().numpy().view(np.uint64)
    ref = BO.pack_mask(sup)
    computed = np.arange(nblk)[None, :] >= (np.arange(n) // 64)[:, None]
    assert np.array_equal(got[computed], ref[computed])
    assert (got[~computed] == np.uint64(0x5A5A5A5A)).all()


def test_planted_cross_class_and_cross_threshold_pairs():
    """Two coincident boxes of different classes are both kept; one pair geometry (IoU 0.18) is kept under class 0's threshold 0.25
    and suppressed under class 1's 0.1.  These pairs lie far from no threshold by construction: their classes are what decides."""
    import link_amd as la
    a = [0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.1, -0.2, 0.0]
    shifted = lambda b, d: [b[0] + d] + b[1:]                         # noqa: E731
    far = [300.0, 50.0, 0.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]
    rows = [a, a,                                                     # coincident, classes 0 and 2
            shifted(a, 40.0), shifted(a, 42.78),                      # IoU 0.18, both class 0 (thr 0.25): both stay
            far, shifted(far, 2.78)]                                  # the same geometry, both class 1 (thr 0.1): the second leaves
    labels = [0, 2, 0, 0, 1, 1]
    scores = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]
    iou = BO.iou_bev(BO.to_pcdet(np.asarray(rows, np.float32)[[2, 4]][:, [0, 1, 2, 3, 4, 5, -1]]),
                     BO.to_pcdet(np.asarray(rows, np.float32)[[3, 5]][:, [0, 1, 2, 3, 4, 5, -1]]))
    assert (np.abs(iou - 0.18) < 5e-3).all(), iou
    one = {"box3d_lidar": torch.tensor(rows[:3], device=DEV), "scores": torch.tensor(scores[:3], device=DEV),
           "label_preds": torch.tensor(labels[:3], device=DEV)}
    two = {"box3d_lidar": torch.tensor(rows[3:], device=DEV), "scores": torch.tensor(scores[3:], device=DEV),
           "label_preds": torch.tensor(labels[3:], device=DEV)}
    thr = [0.25, 0.1, 0.25]
    boxes, sc, lab = la.fuse_detections([one, two], thr)
    want = TO.classwise_nms(np.asarray(rows, np.float32), np.asarray(scores, np.float32), np.asarray(labels), thr)
    assert list(want) == [0, 1, 2, 3, 4]
    assert np.array_equal(sc.cpu().numpy(), np.asarray(scores, np.float32)[want]) and lab.tolist() == [0, 2, 0, 0, 1]
    assert np.array_equal(boxes.cpu().numpy(), np.asarray(rows, np.float32)[want])
