"""GPU checks of the detection post-processing kernels (csrc/boxnms.hip) against the fixtures recorded from the reference's compiled CPU
routine (tests/golden/make_golden_boxnms.py) and the numpy checkers of tests/box_oracle.py."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, load_golden

import box_oracle as BO

pytestmark = pytest.mark.gpu

PAIR_SHAPES = [(1, 1), (17, 63), (64, 64), (65, 130), (256, 192)]
NMS_SIZES = [0, 1, 64, 65, 1000, 4097]
DEV = "cuda"


def _nms_fixture(n):
    g = load_golden(f"boxnms_nms_{n}.npz")
    return g, torch.from_numpy(g["boxes"]).to(DEV), torch.from_numpy(g["scores"]).to(DEV)


@pytest.mark.parametrize("na,nb", PAIR_SHAPES)
def test_overlap_and_iou_matrices(na, nb):
    """|kernel - compiled reference| <= 4 d + 2e-6 per entry, d = the fixture's distance between the reference's float32 output and
    the float64 restatement (the factor 4: device sin / cos / atan2 against the host libm); exact zeros stay exact zeros."""
    import link_amd as la
    g = load_golden(f"boxnms_pairs_{na}x{nb}.npz")
    a, b = torch.from_numpy(g["a"]).to(DEV), torch.from_numpy(g["b"]).to(DEV)
    tol = 4 * g["meta"]["d"] + 2e-6
    iou = la.boxes_iou_bev(a, b).cpu().numpy()
    ov = la.boxes_overlap_bev(a, b).cpu().numpy()
    e_iou = float(np.abs(iou.astype(np.float64) - g["iou"]).max())
    e_ov = float(np.abs(ov.astype(np.float64) - g["overlap"]).max())
    print(f"{na}x{nb}: max |iou - ref| = {e_iou:.3e}, max |overlap - ref| = {e_ov:.3e} m^2, bound {tol:.3e}")
    if os.environ.get("LINK_WRITE_PROFILES"):           # record the observed maxima (merged into the file; off by default)
        path = os.path.join(ROOT, "profiles", "boxnms_parity.json")
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[f"{na}x{nb}"] = {"iou_max_abs_err": e_iou, "overlap_max_abs_err": e_ov, "bound": tol, "d": g["meta"]["d"]}
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    assert e_iou <= tol, (e_iou, tol)
    assert e_ov <= tol, (e_ov, tol)
    assert np.array_equal(iou == 0, g["iou"] == 0) and np.array_equal(ov == 0, g["overlap"] == 0)
    # the det3d-shaped namespace writes into the caller's tensor
    out = torch.full((na, nb), -1.0, device=DEV)
    assert la.boxnms.iou3d_nms_cuda.boxes_iou_bev_gpu(a, b, out) == 1
    assert torch.equal(out.cpu(), torch.from_numpy(iou))


def test_degenerate_pairs():
    """The special cases the stability rule of the fixture generator mostly removes from the recorded sets, built here directly: an
    exact duplicate (IoU 1), two equal squares on one centre at 45 degrees (the octagon, IoU 2 (sqrt 2 - 1) / (4 - 2 sqrt 2) =
    0.70710...), the same squares 0.002 rad apart (all 8 corners inside by the margin next to 8 crossings: 16 points, the longest
    list two rectangles give), neighbours that share an edge (0), a zero-area box in a large one (0), a small box in a large one
    (ratio of the areas).  Against the analytic value where there is one and against the float64 restatement otherwise.
    Bound: 1e-5 of the larger footprint in m^2, 1e-5 for IoU -- coordinates are below 8 m, so a corner or crossing carries an error
    of a few float32 ulps of 8 (5e-7 m each), times an edge of at most 12 m, times up to 16 points: ~1e-4 m^2 at the very worst on
    a 144 m^2 box, i.e. 1e-6 of its footprint; the factor 10 is slack for the sums of the fan."""
    import link_amd as la
    h = 0.3
    sq = [1.0, -2.0, 0.0, 4.0, 4.0, 1.5, h]
    cases = {"duplicate": ([2.0, 1.0, 0.0, 3.9, 1.7, 1.5, 1.1], [2.0, 1.0, 0.0, 3.9, 1.7, 1.5, 1.1], 1.0),
             "octagon": (sq, sq[:6] + [h + np.pi / 4], 2 * (np.sqrt(2) - 1) / (4 - 2 * np.sqrt(2))),
             "sixteen_points": (sq, sq[:6] + [h + 0.002], None),
             "shared_edge": ([0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0], [4.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0], 0.0),
             "zero_area": ([0.5, 0.5, 0.0, 12.0, 12.0, 1.5, 0.7], [1.0, 0.0, 0.0, 0.0, 3.0, 1.5, 0.2], 0.0),
             "small_in_large": ([0.5, 0.5, 0.0, 12.0, 12.0, 1.5, 0.7], [1.5, 0.5, 0.0, 0.25, 0.2, 1.5, -2.0], 0.25 * 0.2 / 144.0)}
    a = np.asarray([c[0] for c in cases.values()], np.float32)
    b = np.asarray([c[1] for c in cases.values()], np.float32)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    iou = la.boxes_iou_bev(ta, tb).cpu().numpy().diagonal()
    ov = la.boxes_overlap_bev(ta, tb).cpu().numpy().diagonal()
    ov64, cnt = BO.box_overlap(a, b, np.float64, return_count=True)
    iou64 = BO.iou_bev(a, b, np.float64)
    big = np.maximum(a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]).astype(np.float64)
    for i, (name, (_, _, want)) in enumerate(cases.items()):
        print(f"{name}: points {cnt[i]}, iou {iou[i]:.8f} (float64 restatement {iou64[i]:.8f}, analytic {want}), overlap {ov[i]:.6f}")
        assert abs(iou[i] - iou64[i]) <= 1e-5 and abs(ov[i] - ov64[i]) <= 1e-5 * big[i], name
        if want is not None:
            assert abs(iou[i] - want) <= 1e-5, (name, iou[i], want)
    assert cnt[list(cases).index("sixteen_points")] == 16 and cnt[list(cases).index("octagon")] == 8
    assert iou[list(cases).index("shared_edge")] == 0 and iou[list(cases).index("zero_area")] == 0


def _random_mask(n, density, seed):
    rng = np.random.default_rng(seed)
    nblk = (n + 63) // 64
    if density == 0:
        return np.zeros((n, nblk), np.uint64)
    if density == 1:
        return np.full((n, nblk), np.uint64(0xFFFFFFFFFFFFFFFF))
    bits = rng.random((n, nblk, 64)) < density
    return (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000, 4097])
def test_nms_reduce_is_the_greedy_rule_bit_for_bit(n):
    """Random mask words, every word of every row filled (also the ones below the diagonal block, which the scan must not read)."""
    from link_amd import _lib as L
    lib = L.lib()
    for di, density in enumerate((0, 0.01, 0.5, 1)):
        words = _random_mask(n, density, 100 * n + di)
        m = torch.from_numpy(words.view(np.int64)).to(DEV)
        for post in (0, 1, 83):
            keep = torch.full((n,), 7, dtype=torch.int64, device=DEV)
            count = torch.full((1,), -3, dtype=torch.int32, device=DEV)
            L.check(lib.link_nms_reduce(m.data_ptr(), n, None, post, keep.data_ptr(), count.data_ptr(), L.current_stream_handle()), "reduce")
            ref = BO.greedy_from_words(words, n, post or None)
            c = int(count.item())
            assert c == len(ref), (n, density, post, c, len(ref))
            k = keep.cpu().numpy()
            assert np.array_equal(k[:c], ref), (n, density, post)
            assert (k[c:] == -1).all(), (n, density, post)


@pytest.mark.parametrize("n", [64, 65, 1000])
def test_nms_mask_words_equal_the_reference_decisions(n):
    from link_amd import _lib as L
    lib = L.lib()
    g, boxes, scores = _nms_fixture(n)
    m = g["meta"]
    order = np.argsort(-g["scores"], kind="stable")
    s = g["boxes"][order]
    sb = torch.from_numpy(s).to(DEV)
    nblk = (n + 63) // 64
    decisions = {L.NMS_ROTATE: (BO.pairs_matrix(BO.iou_bev, s, s) > np.float32(m["thr"]), m["thr"]),
                 L.NMS_NORMAL: (BO.pairs_matrix(BO.iou_normal, s, s) > np.float32(m["thr"]), m["thr"]),
                 L.NMS_CIRCLE: (BO.pairs_matrix(BO.centre_dist2, s, s) <= np.float32(m["radius"]), m["radius"])}
    for pred, (sup, thr) in decisions.items():
        mask = torch.full((n, nblk), 0x5A5A5A5A, dtype=torch.int64, device=DEV)          # the kernel writes every computed word
        L.check(lib.link_nms_mask(sb.data_ptr(), n, None, pred, thr, mask.data_ptr(), L.current_stream_handle()), "mask")
        got = mask.cpu().numpy().view(np.uint64)
        ref = BO.pack_mask(sup)
        computed = np.arange(nblk)[None, :] >= (np.arange(n) // 64)[:, None]
        assert np.array_equal(got[computed], ref[computed]), pred
        assert (got[~computed] == np.uint64(0x5A5A5A5A)).all(), pred                       # and nothing else


@pytest.mark.parametrize("n", NMS_SIZES)
def test_nms_end_to_end_keep_lists(n):
    import link_amd as la
    g, boxes, scores = _nms_fixture(n)
    m = g["meta"]
    thr, pre, post, radius = m["thr"], m["pre"], m["post"], m["radius"]
    keep, none = la.nms_gpu(boxes, scores, thr)
    assert none is None and np.array_equal(keep.cpu().numpy(), g["keep_rotate"])
    keep, _ = la.nms_gpu(boxes, scores, thr, pre_maxsize=pre)
    assert np.array_equal(keep.cpu().numpy(), g["keep_rotate_pre"])
    keep, _ = la.nms_normal_gpu(boxes, scores, thr)
    assert np.array_equal(keep.cpu().numpy(), g["keep_normal"])
    sel = la.rotate_nms_pcdet(boxes, scores, thr, pre, post)
    assert sel.dtype == torch.int64 and np.array_equal(sel.cpu().numpy(), g["keep_pcdet"])
    dets = torch.cat([boxes[:, :2], scores.view(-1, 1)], 1)
    assert np.array_equal(la.circle_nms(dets, radius, post).cpu().numpy(), g["keep_circle"])
    if n:
        # the det3d-shaped entry: boxes in score order, a CPU LongTensor for the kept positions
        order = scores.sort(0, descending=True)[1]
        keep_cpu = torch.zeros(n, dtype=torch.int64)
        num = la.boxnms.iou3d_nms_cuda.nms_gpu(boxes[order].contiguous(), keep_cpu, thr)
        assert np.array_equal(order.cpu().numpy()[keep_cpu[:num].numpy()], g["keep_rotate"])


@pytest.mark.parametrize("n", [1, 65, 1000, 4097])
def test_nms_padded_and_device_count(n):
    import link_amd as la
    from link_amd.boxnms import nms_sorted
    g, boxes, scores = _nms_fixture(n)
    m = g["meta"]
    thr, pre, post = m["thr"], m["pre"], m["post"]
    idx, count = la.nms_padded(la.to_pcdet(boxes), scores, thr, pre, post)
    idx2, count2 = la.nms_padded(la.to_pcdet(boxes), scores, thr, pre, post)
    assert torch.equal(idx, idx2) and torch.equal(count, count2)                          # bitwise identical across runs
    c = int(count.item())
    assert idx.shape == (post,) and c == len(g["keep_pcdet"])
    assert np.array_equal(idx.cpu().numpy()[:c], g["keep_pcdet"]) and (idx[c:] == -1).all()
    idx, count = la.nms_padded(boxes[:, :2].contiguous(), scores, m["radius"], None, post, pred="circle")
    assert np.array_equal(idx.cpu().numpy()[:int(count.item())], g["keep_circle"])
    # device-side count with capacity > n: the boxes of the fixture in front of a tail of junk
    order = scores.sort(0, descending=True)[1]
    sb = boxes[order].contiguous()
    cap = n + 77
    padded = torch.cat([sb, sb.new_full((77, 7), 3.0)])
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    k_host, c_host = nms_sorted(sb, thr)
    k_dev, c_dev = nms_sorted(padded, thr, n_dev=n_dev)
    assert torch.equal(c_host, c_dev) and k_dev.shape == (cap,)
    c = int(c_host.item())
    assert torch.equal(k_host[:c], k_dev[:c]) and (k_dev[c:] == -1).all()
    assert np.array_equal(order[k_host[:c]].cpu().numpy(), g["keep_rotate"])


CFG = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 83,
                                                                                      "nms_iou_threshold": 0.2},
       "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075]}


def _decode_torch(pd, cfg):
    """center_head.py:314-316, 344-421 and the masks of :461-467, composed from torch ops"""
    pd = {k: v.permute(0, 2, 3, 1).contiguous() for k, v in pd.items()}
    hm, dim = torch.sigmoid(pd["hm"]), torch.exp(pd["dim"])
    rots, rotc = pd["rot"][..., 0:1], pd["rot"][..., 1:2]
    rot = torch.atan2(rots, rotc)
    batch, H, W, K = hm.shape
    reg, hei = pd["reg"].reshape(batch, H * W, 2), pd["height"].reshape(batch, H * W, 1)
    rot, dim, hm = rot.reshape(batch, H * W, 1), dim.reshape(batch, H * W, 3), hm.reshape(batch, H * W, K)
    ys, xs = torch.meshgrid([torch.arange(0, H), torch.arange(0, W)], indexing="ij")
    ys = ys.view(1, H, W).repeat(batch, 1, 1).to(hm)
    xs = xs.view(1, H, W).repeat(batch, 1, 1).to(hm)
    xs = xs.view(batch, -1, 1) + reg[:, :, 0:1]
    ys = ys.view(batch, -1, 1) + reg[:, :, 1:2]
    xs = xs * cfg["out_size_factor"] * cfg["voxel_size"][0] + cfg["pc_range"][0]
    ys = ys * cfg["out_size_factor"] * cfg["voxel_size"][1] + cfg["pc_range"][1]
    parts = [xs, ys, hei, dim] + ([pd["vel"].reshape(batch, H * W, 2)] if "vel" in pd else []) + [rot]
    boxes = torch.cat(parts, dim=2)
    scores, labels = torch.max(hm, dim=-1)
    r = torch.tensor(cfg["post_center_limit_range"], dtype=hm.dtype, device=hm.device)
    mask = (scores > cfg["score_threshold"]) & (boxes[..., :3] >= r[:3]).all(-1) & (boxes[..., :3] <= r[3:]).all(-1)
    return boxes, labels, scores, mask, hm


def _maps(B, H, W, K, vel, seed, cfg):
    """Random head maps, redrawn where a decision would be close: no score within 1e-4 of the threshold, no centre within 1e-4 of
    the range, no two class scores of a cell within 1e-5."""
    gen = torch.Generator().manual_seed(seed)
    pd = {"reg": torch.rand(B, 2, H, W, generator=gen), "height": torch.randn(B, 1, H, W, generator=gen) * 4 - 1,
          "dim": torch.randn(B, 3, H, W, generator=gen) * 0.5, "rot": torch.randn(B, 2, H, W, generator=gen),
          "hm": torch.randn(B, K, H, W, generator=gen) * 1.5 - 2.0}
    if vel:
        pd["vel"] = torch.randn(B, 2, H, W, generator=gen)
    for _ in range(20):
        boxes, _, scores, _, hm = _decode_torch(pd, cfg)
        r = torch.tensor(cfg["post_center_limit_range"])
        close = (scores - cfg["score_threshold"]).abs() < 1e-4
        close |= ((boxes[..., :3] - r[:3]).abs() < 1e-4).any(-1) | ((boxes[..., :3] - r[3:]).abs() < 1e-4).any(-1)
        if K > 1:
            top2 = hm.topk(2, dim=-1)[0]
            close |= (top2[..., 0] - top2[..., 1]) < 1e-5
        if not close.any():
            return pd
        cell = close.view(B, 1, H, W)
        pd["hm"] = torch.where(cell, torch.randn(B, K, H, W, generator=gen) * 1.5 - 2.0, pd["hm"])
        pd["height"] = torch.where(cell, torch.randn(B, 1, H, W, generator=gen) * 4 - 1, pd["height"])
        pd["reg"] = torch.where(cell, torch.rand(B, 2, H, W, generator=gen), pd["reg"])
    raise AssertionError("could not draw maps away from the decision boundaries")


@pytest.mark.parametrize("H,W", [(8, 12), (180, 180)])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("vel", [False, True])
def test_center_decode(H, W, K, vel):
    import link_amd as la
    B = 2
    pd = _maps(B, H, W, K, vel, 7 + K + 2 * vel + H, CFG)
    rb, rl, rs, rmask, _ = _decode_torch({k: v.clone() for k, v in pd.items()}, CFG)
    dec = la.CenterHeadDecoder(CFG, [K])
    boxes, labels, scores, counts = dec.decode({k: v.to(DEV) for k, v in pd.items()})
    assert boxes.shape == (B, H * W, 9 if vel else 7) and labels.dtype == torch.int32
    mask = (scores > float("-inf")).cpu()
    assert torch.equal(mask, rmask)
    assert torch.equal(labels.cpu().long(), rl)
    assert torch.equal(counts.cpu().long(), rmask.sum(1))
    assert 0 < int(rmask.sum()) < rmask.numel()
    got = boxes.cpu()
    nz = rb != 0
    rel = ((got - rb).abs()[nz] / rb.abs()[nz]).max()                 # per component, relative to that component
    srel = ((scores.cpu() - rs).abs()[rmask] / rs[rmask]).max()
    print(f"H{H} W{W} K{K} vel{vel}: boxes max rel err {float(rel):.3e}, scores {float(srel):.3e}")
    assert ((got - rb).abs() <= 1e-5 * rb.abs()).all(), float(rel)
    assert srel <= 1e-5
    copied = [2] + ([6, 7] if vel else [])                            # z and vel are copies
    assert torch.equal(got[..., copied], rb[..., copied])


@pytest.fixture(scope="module")
def head_case():
    """harness.bevhead.BevHalf on a seeded random BEV tensor, head biases shifted so that each task has 200-2 000 candidates"""
    from harness.bevhead import BevHalf
    torch.manual_seed(11)
    net = BevHalf(256).to(DEV).eval()
    bev = torch.randn(2, 256, 180, 180, generator=torch.Generator().manual_seed(12)).to(DEV)
    with torch.no_grad():
        preds = net(bev)
        thr_logit = float(np.log(CFG["score_threshold"] / (1 - CFG["score_threshold"])))
        for pd in preds:
            # a random-init head's maps are almost constant: spread each map out (unit variance), so that scores are distinct and
            # boxes have all headings, sizes and offsets
            for k in pd:
                pd[k] = (pd[k] - pd[k].mean((0, 2, 3), keepdim=True)) / pd[k].std((0, 2, 3), keepdim=True)
            pd["dim"] = pd["dim"] * 0.6
            # The heat map: keep the head's ORDER of the logits and give them evenly spaced values with ~1 200 above the threshold per
            # task (a random-init head's logits sit on a few hundred float32 steps around its bias, so its scores tie; distinct scores
            # are what makes the order of the candidates unique).  This is the head's bias shift, made tie-free.
            flat = pd["hm"].reshape(-1)
            N = flat.numel()
            rank = torch.empty(N, device=DEV)
            rank[flat.argsort(stable=True)] = torch.arange(N, dtype=torch.float32, device=DEV)
            pd["hm"] = (thr_logit + (rank - (N - 1200) + 0.5) * 2e-3).reshape(pd["hm"].shape)
            pd["reg"] = pd["reg"].sigmoid()
            pd["dim"] = pd["dim"].clamp(-1.5, 2.0)
            pd["height"] = pd["height"].tanh() * 3
    return preds


def test_center_head_decoder_predict(head_case):
    import link_amd as la
    preds = head_case
    num_classes = [pd["hm"].shape[1] for pd in preds]
    dec = la.CenterHeadDecoder(CFG, num_classes)
    out = dec.predict(preds)
    pad = dec.predict_padded(preds)
    post = CFG["nms"]["nms_post_max_size"]
    assert len(out) == 2 and pad["box3d_lidar"].shape == (2, len(preds) * post, 9)
    flag = 0
    for t, pd in enumerate(preds):
        boxes, labels, scores, counts = dec.decode(pd)
        for b in range(2):
            c = int(counts[b])
            assert 200 <= c <= 2000, (t, b, c)
            mask = scores[b] > float("-inf")
            bp, sc, lab = boxes[b][mask].cpu().numpy(), scores[b][mask].cpu().numpy(), labels[b][mask].cpu().numpy()
            order = np.argsort(-sc, kind="stable")[:CFG["nms"]["nms_pre_max_size"]]
            assert len(np.unique(sc)) == len(sc)
            p = BO.to_pcdet(bp[order][:, [0, 1, 2, 3, 4, 5, -1]])
            sup = BO.pairs_matrix(BO.iou_bev, p, p) > np.float32(CFG["nms"]["nms_iou_threshold"])
            sel = order[BO.greedy_nms(sup, post)]
            # the padded form's slots of this task and frame
            pc = int(pad["counts"][b, t])
            sl = slice(t * post, t * post + pc)
            assert pc == len(sel), (t, b, pc, len(sel))
            assert np.array_equal(pad["box3d_lidar"][b, sl].cpu().numpy(), bp[sel])
            assert np.array_equal(pad["scores"][b, sl].cpu().numpy(), sc[sel])
            assert np.array_equal(pad["label_preds"][b, sl].cpu().numpy(), lab[sel] + flag)
            assert (pad["label_preds"][b, t * post + pc:(t + 1) * post] == -1).all()
        flag += num_classes[t]
    for b in range(2):                                               # predict == the concatenation of the padded form's used slots
        used = torch.cat([torch.arange(t * post, t * post + int(pad["counts"][b, t])) for t in range(len(preds))]).to(DEV)
        assert torch.equal(out[b]["box3d_lidar"], pad["box3d_lidar"][b, used])
        assert torch.equal(out[b]["scores"], pad["scores"][b, used])
        assert torch.equal(out[b]["label_preds"], pad["label_preds"][b, used])


def test_predict_padded_in_a_captured_graph(head_case):
    import link_amd as la
    preds = head_case
    dec = la.CenterHeadDecoder(CFG, [pd["hm"].shape[1] for pd in preds])
    eager = dec.predict_padded(preds)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.predict_padded(preds)                                    # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = dec.predict_padded(preds)
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], captured[k]), k
