"""GPU checks of the two-stage ROI head (csrc/roihead.hip, section O of include/link_amd.h; link_amd/roihead.py) against the
restatements of tests/roi_oracle.py and the fixtures of tests/golden/make_golden_roihead.py.

Integer and index outputs are compared exactly.  A float output's distance from the float64 oracle may be at most 4 e_ref + 1 fp32
ulp of the largest magnitude in the tensor (the factor 4 covers a different but fixed summation order and fused multiply-adds), plus
half an ulp of the output format for a 16-bit output (rounded once).  e_ref is the distance of the reference's float32 recording from
the float64 oracle where the case runs on a recorded fixture (its meta), and the distance of the float32 restatement from the
float64 oracle on the shapes no fixture holds -- tests/test_cpu_roihead.py pins that restatement on the recordings, so it stands for
the reference's float32 error there.  Each comparison leaves its figures in roihead_parity.jsonl in the directory
LINK_AMD_PARITY_DIR names before any verdict (profiles/roihead_parity.jsonl is one run)."""
import numpy as np
import pytest
import torch

from helpers import load_golden
from ref64 import record_row

import roi_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
GEOM = {"pc_start": [-3.5, -2.5], "voxel_size": [0.25, 0.25], "out_stride": 4}       # a 7 x 5 map of unit cells
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}         # relative, of the largest magnitude
ASSIGN = ["roihead_assign_allclass.npz", "roihead_assign_code9.npz", "roihead_assign_waymo.npz"]


def gate(test, case, name, got, want64, e_ref, out_dtype=torch.float32):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    big = float(np.abs(want64).max(initial=0.0))
    bound = 4 * float(e_ref) + float(np.spacing(np.float32(big))) + HALF_ULP[out_dtype] * big
    d = float(np.abs(got - want64).max(initial=0.0))
    print(test, case, name, "e_dev", d, "e_ref", float(e_ref), "bound", bound)
    record_row({"test": test, **case, "component": name, "e_dev": d, "e_ref": float(e_ref), "bound": bound}, name="roihead_parity.jsonl")
    assert d <= bound, (test, case, name, d, bound)


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0.0))


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x if dtype is None else x.to(dtype)


# ---- O1: features ----------------------------------------------------------------------------------------------------------------
def _boxes(B, R, seed, L=9):
    rng = np.random.default_rng(seed)
    b = np.zeros((B, R, L), np.float32)
    b[..., 0], b[..., 1] = rng.uniform(-5.5, 5.5, (B, R)), rng.uniform(-4.5, 4.5, (B, R))
    b[..., 2] = rng.uniform(-1, 1, (B, R))
    b[..., 3:6] = rng.uniform(0.3, 3.0, (B, R, 3))
    b[..., -1] = rng.uniform(-2 * np.pi, 2 * np.pi, (B, R))
    special = [(-4.75, 0.25, 0.0), (4.75, 0.25, 0.0), (0.25, -3.75, 0.0), (0.25, 3.75, 0.0),      # off the map on the four sides
               (2.5, 1.5, 0.0), (2.3, -0.3, np.pi), (0.6, 1.3, -np.pi)]                              # on the last column and row; heading +-pi
    # (the +-pi boxes sit off the cell boundaries: sin(fp32 pi) is -8.7e-8, not 0, and a midpoint that far from a boundary lands in
    # another cell in float64 than in float32 -- the formula's own discontinuity, not an error to measure)
    for k, (x, y, h) in enumerate(special):
        if k < R:
            b[0, k, 0], b[0, k, 1], b[0, k, -1] = x, y, h
            if k < 5:
                b[0, k, 3:5] = 0.5                                                                # the edge midpoints stay on that side
    return b


def _layouts(bev):
    """the same [B, C, H, W] values as a contiguous NCHW map, a channels_last map, a batch slice and a channel slice"""
    B, C, H, W = bev.shape
    wide = torch.zeros((B, C + 3, H, W), dtype=bev.dtype, device=bev.device)
    wide[:, 2:2 + C] = bev
    tall = torch.zeros((2 * B + 1, C, H, W), dtype=bev.dtype, device=bev.device)
    tall[1:2 * B + 1:2] = bev
    return {"nchw": bev.contiguous(), "channels_last": bev.contiguous(memory_format=torch.channels_last), "batch_slice": tall[1:2 * B + 1:2],
            "channel_slice": wide[:, 2:2 + C]}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [1, 3, 64, 130])
def test_features(C, dtype):
    import link_amd as la
    ext = la.BEVFeatureExtractor(**GEOM)
    dt = DTYPES[dtype]
    B, H, W = 2, 5, 7
    bev = torch.from_numpy(np.random.default_rng(C).standard_normal((B, C, H, W)).astype(np.float32)).to(DEV).to(dt)
    bev_np = bev.float().cpu().numpy()
    maps = _layouts(bev)
    for R in (0, 1, 63, 65):
        boxes = _boxes(B, R, 10 + R)
        labels = (np.arange(B * R).reshape(B, R) % 5 != 3).astype(np.int64)                        # every fifth row an unused slot
        for P in (1, 5):
            r32 = RO.bev_features(bev_np, boxes, labels, None, P, **GEOM)
            r64 = RO.bev_features(bev_np, boxes, labels, None, P, dtype=np.float64, **GEOM)
            for layout, m in maps.items():
                out = ext.extract(m, t(boxes), t(labels), None, P)
                assert out.shape == (B, R, P * C) and out.dtype == dt
                got = out.float().cpu().numpy()
                assert not got[labels == 0].any()                                                 # label 0: a row of zeros
                gate("features", {"C": C, "dtype": dtype, "R": R, "P": P, "layout": layout}, "features", got, r64, dist(r32, r64), dt)


def test_features_sel_with_repeats_and_other_heading_column():
    import link_amd as la
    ext = la.BEVFeatureExtractor(**GEOM)
    B, C, R = 2, 12, 30
    bev = np.random.default_rng(5).standard_normal((B, C, 5, 7)).astype(np.float32)
    boxes = _boxes(B, R, 77, L=9)
    rois = boxes[..., [0, 1, 2, 3, 4, 5, 8, 6, 7]]                                                 # the heading moved to column 6
    labels = (np.arange(B * R).reshape(B, R) % 4 != 1).astype(np.int64)
    sel = np.random.default_rng(6).integers(0, R, (B, 17)).astype(np.int32)
    sel[:, 3] = sel[:, 2]                                                                          # a repeat
    r32 = RO.bev_features(bev, rois, labels, sel, 5, rot_col=6, **GEOM)
    r64 = RO.bev_features(bev, rois, labels, sel, 5, rot_col=6, dtype=np.float64, **GEOM)
    out = ext.extract(t(bev), t(rois), t(labels), t(sel), 5, rot_col=6).cpu().numpy()
    assert out.shape == (B, 17, 5 * C) and np.array_equal(out[:, 2], out[:, 3])
    gate("features_sel", {"C": C, "R": R, "S": 17}, "features", out, r64, dist(r32, r64))
    full = ext.extract(t(bev), t(boxes), t(labels), None, 5).cpu().numpy()                        # heading last: the first-stage order
    assert np.array_equal(full[np.arange(B)[:, None], sel], out)
    # the reference's signature: an NHWC map and the points of get_box_center
    g = load_golden("roihead_features.npz")
    m = g["meta"]
    ext2 = la.BEVFeatureExtractor(m["pc_start"], m["voxel_size"], m["out_stride"])
    nhwc = t(g["bev"]).permute(0, 2, 3, 1).contiguous()
    for P in (1, 5):
        feats = ext2({"bev_feature": nhwc}, [t(p) for p in g[f"points{P}"]], P)
        r64 = RO.bev_features(g["bev"], g["boxes"], None, None, P, dtype=np.float64, pc_start=m["pc_start"], voxel_size=m["voxel_size"],
                              out_stride=m["out_stride"])
        gate("features_forward", {"P": P}, "features", torch.stack(feats).cpu().numpy(), r64, m[f"e_features{P}"])
        gate("features_recorded", {"P": P}, "features", torch.stack(feats).cpu().numpy(), g[f"features{P}"], m[f"e_features{P}"])


def test_features_of_a_map_that_requires_grad_run_the_torch_restatement():
    import link_amd as la
    ext = la.BEVFeatureExtractor(**GEOM)
    bev = torch.randn(1, 4, 5, 7, device=DEV, requires_grad=True)
    boxes = t(_boxes(1, 9, 3))
    out = ext.extract(bev, boxes, None, None, 5)
    out.sum().backward()
    assert bev.grad is not None and bev.grad.abs().sum() > 0
    fused = ext.extract(bev.detach(), boxes, None, None, 5)
    assert torch.allclose(out.detach(), fused, atol=1e-5, rtol=1e-5)


# ---- O2: assign --------------------------------------------------------------------------------------------------------------------
def _layer(cfg):
    import link_amd as la
    return la.ProposalTargetLayer(cfg)


def _batch(rois, labels, scores, gt):
    return {"rois": t(rois), "roi_labels": t(labels), "roi_scores": t(scores), "gt_boxes_and_cls": t(gt)}


FLOAT_KEYS = ("max_overlaps", "gt_iou_of_rois", "gt_of_rois", "rcnn_cls_labels")
EXACT_KEYS = ("rois", "roi_labels", "roi_scores", "reg_valid_mask")


@pytest.mark.parametrize("name", ASSIGN)
def test_assign_replays_the_reference_draw(name):
    g = load_golden(name)
    m = g["meta"]
    out = _layer(m["cfg"])(_batch(g["in_rois"], g["in_roi_labels"], g["in_roi_scores"], g["in_gt"]), sampled_inds=t(g["sampled_inds"]))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    o64 = RO.assign(g["in_rois"], g["in_roi_labels"], g["in_roi_scores"], g["in_gt"], m["cfg"], sel_in=g["sampled_inds"], dtype=np.float64)
    assert np.array_equal(got["sel"], g["sampled_inds"]) and not got["status"].any()
    for k in EXACT_KEYS:
        assert np.array_equal(got[k], g[k]), k
    assert np.array_equal(got["gt_of_rois"], g["gt_of_rois_src"])                                 # ProposalTargetLayer's key: as given
    assert np.array_equal(got["gt_assignment"], o64["gt_assignment"])                             # stable inputs: no near ties
    case = {"fixture": name}
    gate("assign_replay", case, "max_overlaps", got["max_overlaps"], o64["max_overlaps"], m["e_max_overlaps"])
    gate("assign_replay", case, "gt_iou_of_rois", got["gt_iou_of_rois"], o64["gt_iou_of_rois"], m["e_gt_iou_of_rois"])
    gate("assign_replay", case, "gt_of_rois", got["gt_of_rois_canonical"], o64["gt_of_rois"], m["e_gt_of_rois"])
    gate("assign_replay", case, "rcnn_cls_labels", got["rcnn_cls_labels"], o64["rcnn_cls_labels"], m["e_rcnn_cls_labels"])
    # and the recording itself, to the same bound
    gate("assign_recorded", case, "gt_of_rois", got["gt_of_rois_canonical"], g["gt_of_rois"], m["e_gt_of_rois"])
    gate("assign_recorded", case, "max_overlaps", got["max_overlaps"], g["max_overlaps"], m["e_max_overlaps"])


def _frame(rng, R, G, G_pad, code, classes=3):
    gt = np.zeros((G_pad, code + 1), np.float32)
    gt[:G, 0:2] = rng.uniform(-40, 40, (G, 2))
    gt[:G, 2] = rng.uniform(-1, 1, G)
    gt[:G, 3:6] = np.exp(rng.uniform(np.log(0.6), np.log(5.0), (G, 3)))
    gt[:G, 6] = rng.uniform(-np.pi, np.pi, G)
    gt[:G, 7:code] = rng.standard_normal((G, code - 7))
    gt[:G, -1] = rng.integers(1, classes + 1, G)
    rois = np.zeros((R, code), np.float32)
    labels = np.ones(R, np.int64)
    for i in range(R):
        if G == 0:
            rois[i, :7] = [rng.uniform(-40, 40), rng.uniform(-40, 40), 0, 2, 1, 1.5, rng.uniform(-3, 3)]
            continue
        j = rng.integers(0, G)
        s = (0.02, 0.1, 0.3, 0.8, 3.0)[i % 5]
        rois[i] = gt[j, :code]
        rois[i, :3] += rng.normal(0, s, 3).astype(np.float32)
        rois[i, 6] += np.float32(rng.normal(0, 0.3 * min(s, 1.0)) + (np.pi if i % 7 == 0 else 0.0))
        labels[i] = int(gt[j, -1]) if i % 11 else classes + 1                                      # a class the ground truth does not hold
    if R > 4:
        rois[R - 1], labels[R - 1] = 0, 0                                                          # an unused slot
    return rois, labels, gt


def _check_assign(test, case, got, rois, labels, scores, gt, cfg, noise):
    """every output against the oracle; the draw is a pure function of (max_overlaps, noise): exact on the kernel's own overlaps"""
    B, R, code = rois.shape
    o32 = RO.assign(rois, labels, scores, gt, cfg, noise=noise)
    o64 = RO.assign(rois, labels, scores, gt, cfg, sel_in=got["sel"], dtype=np.float64)
    gate(test, case, "max_overlaps", got["max_overlaps"], o64["max_overlaps"], dist(o32["max_overlaps"], o64["max_overlaps"]))
    for b in range(B):
        sel, status = RO.sample(got["max_overlaps"][b], noise[b], cfg)
        assert np.array_equal(got["sel"][b], sel) and got["status"][b] == status, (case, b)
        g = RO.cut_gt(gt[b], code + 1)
        iou64 = RO.max_overlaps(rois[b], labels[b], g, cfg["SAMPLE_ROI_BY_EACH_CLASS"], np.float64, return_matrix=True)[2]
        if cfg["SAMPLE_ROI_BY_EACH_CLASS"]:
            iou64 = np.where(labels[b][:, None] == g[:, -1].astype(np.int64)[None], iou64, 0.0)
        ga = got["gt_assignment"][b]
        assert (ga >= 0).all() and (ga < len(g)).all()
        assert (iou64[np.arange(R), ga] >= o64["max_overlaps"][b] - 1e-5).all()                    # the assigned box is a maximal one
        assert np.array_equal(got["gt_of_rois"][b], g[ga[got["sel"][b]]])
    sel = got["sel"].astype(np.int64)
    take = lambda a: np.take_along_axis(a, sel if a.ndim == 2 else sel[..., None], 1)             # noqa: E731
    assert np.array_equal(got["rois"], take(rois)) and np.array_equal(got["roi_labels"], take(labels))
    assert np.array_equal(got["roi_scores"], take(scores)) and np.array_equal(got["gt_iou_of_rois"], take(got["max_overlaps"]))
    iou = got["gt_iou_of_rois"]
    assert np.array_equal(got["reg_valid_mask"], (iou > np.float32(cfg["REG_FG_THRESH"])).astype(np.int64))
    assert np.array_equal(got["rcnn_cls_labels"], RO.cls_labels(iou, cfg))
    can32 = np.stack([RO.canonical(got["rois"][b], got["gt_of_rois"][b]) for b in range(B)])
    can64 = np.stack([RO.canonical(got["rois"][b], got["gt_of_rois"][b], np.float64) for b in range(B)])
    gate(test, case, "gt_of_rois", got["gt_of_rois_canonical"], can64, dist(can32, can64))


@pytest.mark.parametrize("R,G,M,by_class,code,kind", [(1, 1, 8, True, 7, "roi_iou"), (64, 40, 8, False, 7, "cls"), (65, 0, 8, True, 9, "cls"),
                                                       (65, 1, 128, False, 7, "roi_iou"), (500, 40, 128, True, 7, "roi_iou"),
                                                       (500, 40, 128, True, 9, "cls"), (64, 0, 128, False, 7, "roi_iou")])
def test_assign_draws_as_the_oracle(R, G, M, by_class, code, kind):
    cfg = dict(RO.CFG, ROI_PER_IMAGE=M, SAMPLE_ROI_BY_EACH_CLASS=by_class, CLS_SCORE_TYPE=kind)
    if kind == "cls":
        cfg.update(CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.45)
    rng = np.random.default_rng(R * 1000 + G * 10 + M)
    B = 2
    frames = [_frame(rng, R, G if b == 0 else max(G - 1, 0), G + 3, code) for b in range(B)]        # trailing zero rows
    rois, labels, gt = (np.stack([f[k] for f in frames]) for k in range(3))
    if G == 0:
        gt = gt[:, :0] if R == 64 else gt                                                          # G = 0 both ways: no rows, rows of zeros
    scores = rng.uniform(0.1, 1, (B, R)).astype(np.float32)
    noise = rng.random((B, R + M)).astype(np.float32)
    out = _layer(cfg)(_batch(rois, labels, scores, gt), noise=t(noise))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _check_assign("assign_draw", {"R": R, "G": G, "M": M, "by_class": by_class, "code": code, "kind": kind}, got, rois, labels, scores, gt, cfg, noise)


@pytest.mark.parametrize("sizes,want", [((30, 20, 20), (8, 0, 6, 2)), ((3, 20, 20), (3, 0, 10, 3)), ((30, 0, 0), (0, 16, 0, 0)),
                                        ((0, 20, 20), (0, 0, 12, 4)), ((0, 20, 0), (0, 0, 16, 0)), ((0, 0, 20), (0, 0, 0, 16)),
                                        ((30, 20, 0), (8, 0, 8, 0)), ((30, 0, 20), (8, 0, 0, 8)), ((30, 2, 20), (8, 0, 2, 6))])
def test_assign_sampler_branches(sizes, want):
    """overlaps by construction: a copy of the ground-truth box shifted along its length by d of it has IoU (1 - d) / (1 + d)"""
    cfg = dict(RO.CFG, ROI_PER_IMAGE=16, SAMPLE_ROI_BY_EACH_CLASS=False)
    nfg, nhard, neasy = sizes
    R = sum(sizes)
    gt = np.float32([[[1.0, 2.0, 0.0, 4.0, 2.0, 1.5, 0.0, 1.0]]])
    shift = np.random.default_rng(3).permutation(np.float32([0.05] * nfg + [0.5] * nhard + [0.9] * neasy))
    rois = np.repeat(gt[:, :, :7], R, 1)
    rois[0, :, 0] += shift * 4.0
    labels, scores = np.ones((1, R), np.int64), np.full((1, R), 0.5, np.float32)
    noise = np.random.default_rng(4).random((1, R + 16)).astype(np.float32)
    out = _layer(cfg)(_batch(rois, labels, scores, gt), noise=t(noise))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    fg, hard, easy = RO.sample_lists(got["max_overlaps"][0], cfg)
    assert (len(fg), len(hard), len(easy)) == sizes
    take, repl, nh, ne = want
    sel = got["sel"][0]
    assert np.isin(sel[:take + repl], fg).all() and np.isin(sel[take + repl:take + repl + nh], hard).all()
    assert np.isin(sel[take + repl + nh:], easy).all() and len(np.unique(sel[:take])) == take
    _check_assign("assign_branch", {"fg": nfg, "hard": nhard, "easy": neasy}, got, rois, labels, scores, gt, cfg, noise)


def test_assign_flags_no_candidate_and_bad_replay_index():
    cfg = dict(RO.CFG, ROI_PER_IMAGE=8, SAMPLE_ROI_BY_EACH_CLASS=False)
    rois = np.zeros((2, 5, 7), np.float32)
    rois[..., 3:6] = 1.0
    rois[0, :, 5] = np.nan                                                                         # overlaps that are not finite
    gt = np.float32([[[0, 0, 0, 1, 1, 1, 0, 1]]] * 2)
    labels, scores = np.ones((2, 5), np.int64), np.ones((2, 5), np.float32)
    out = _layer(cfg)(_batch(rois, labels, scores, gt), noise=torch.rand(2, 13, device=DEV))
    assert out["status"].tolist() == [1, 0] and not out["sel"][0].any()
    sel = np.zeros((2, 8), np.int32)
    sel[1, 2] = 5
    out = _layer(cfg)(_batch(rois, labels, scores, gt), sampled_inds=t(sel))
    assert out["status"].tolist() == [0, 2] and not out["sel"][1].any()
    gen = torch.Generator(device=DEV).manual_seed(3)
    import link_amd as la
    a = la.ProposalTargetLayer(cfg, generator=gen)(_batch(rois, labels, scores, gt))["sel"]
    gen.manual_seed(3)
    b = la.ProposalTargetLayer(cfg, generator=gen)(_batch(rois, labels, scores, gt))["sel"]
    assert torch.equal(a, b)


# ---- O3: loss ----------------------------------------------------------------------------------------------------------------------
def _loss_case(test, case, cls, reg, labels, gt, valid, w, dtype, e_ref=None):
    import link_amd as la
    dt = DTYPES[dtype]
    x, r = t(cls, dt).requires_grad_(True), t(reg, dt).requires_grad_(True)
    xin, rin = x.detach().float().cpu().numpy(), r.detach().float().cpu().numpy()                 # the values the kernel reads
    total, lc, lr, fg = la.roi_loss(x, r, t(labels), t(gt), t(valid), w["code_weights"], w["rcnn_cls_weight"], w["rcnn_reg_weight"])
    scale = torch.tensor(3.0, device=DEV)                                                          # a device scalar upstream
    (total * scale).backward()
    o32 = RO.loss(xin, rin, labels, gt, valid, w["code_weights"], w["rcnn_cls_weight"], w["rcnn_reg_weight"])
    o64 = RO.loss(xin, rin, labels, gt, valid, w["code_weights"], w["rcnn_cls_weight"], w["rcnn_reg_weight"], np.float64)
    e = e_ref or {k: dist(o32[k], o64[k]) for k in ("out", "grad_cls", "grad_reg")}
    got = torch.stack([total, lc, lr, fg]).detach().cpu().numpy()
    assert got[3] == valid.sum() and x.grad.dtype == dt and r.grad.dtype == dt
    gate(test, case, "out", got, o64["out"], e["out"])
    gate(test, case, "grad_cls", x.grad.float().cpu().numpy().reshape(-1), 3.0 * o64["grad_cls"], 3.0 * e["grad_cls"], dt)
    gate(test, case, "grad_reg", r.grad.float().cpu().numpy(), 3.0 * o64["grad_reg"], 3.0 * e["grad_reg"], dt)
    return got


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("N", [1, 8, 512])
def test_loss_on_the_recorded_cases(N, dtype):
    g = load_golden(f"roihead_loss_{N}.npz")
    m = g["meta"]
    e = {k: m["e_" + k] for k in ("out", "grad_cls", "grad_reg")} if dtype == "f32" else None      # a rounded input is another case
    got = _loss_case("loss_recorded", {"N": N, "dtype": dtype}, g["cls"], g["reg"], g["labels"], g["gt_of_rois"], g["reg_valid_mask"], m["weights"],
                     dtype, e)
    if dtype == "f32":
        gate("loss_recording", {"N": N}, "out", got, g["out"], m["e_out"])                         # logits +-200: pinned on the recording


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", ["no_foreground", "all_ignored", "moderate_cls", "moderate_soft", "wide_cls"])
def test_loss_edge_cases(case, dtype):
    rng = np.random.default_rng(len(case))
    N, code = (8 if case != "wide_cls" else 512), 7
    span = 30.0 if case == "wide_cls" else 8.0
    cls = rng.uniform(-span, span, N).astype(np.float32)
    reg = rng.standard_normal((N, code)).astype(np.float32)
    gt = rng.standard_normal((N, code + 1)).astype(np.float32)
    iou = rng.uniform(0, 1, N).astype(np.float32)
    labels = iou.copy() if case == "moderate_soft" else RO.cls_labels(iou, dict(RO.CFG, CLS_SCORE_TYPE="cls", CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.45))
    valid = (iou > 0.55).astype(np.int64)
    if case == "no_foreground":
        valid[:] = 0                                                                               # the denominator is 1
    if case == "all_ignored":
        labels[:] = -1
    elif case != "moderate_soft":
        labels[0] = -1                                                                             # the ignore band is masked
    w = {"rcnn_cls_weight": 0.7, "rcnn_reg_weight": 1.3, "code_weights": [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0]}
    got = _loss_case("loss_edge", {"case": case, "dtype": dtype}, cls, reg, labels, gt, valid, w, dtype)
    if case == "no_foreground":
        assert got[2] == 0 and got[3] == 0
    if case == "all_ignored":
        assert got[1] == 0


# ---- O4: refine --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("code", [7, 9])
def test_refine(code, dtype):
    import link_amd as la
    g = load_golden(f"roihead_refine_{code}.npz")
    m = g["meta"]
    dt = DTYPES[dtype]
    cls, reg = t(g["cls"], dt), t(g["reg"], dt)
    out = la.roi_refine(t(g["rois"]), t(g["roi_labels"]), t(g["roi_scores"]), cls, reg)
    cin, rin = cls.float().cpu().numpy(), reg.float().cpu().numpy()
    b32 = RO.refine(g["rois"], g["roi_labels"], g["roi_scores"], cin, rin)
    b64 = RO.refine(g["rois"], g["roi_labels"], g["roi_scores"], cin, rin, np.float64)
    e = (m["e_boxes"], m["e_scores"]) if dtype == "f32" else (dist(b32[0], b64[0]), dist(b32[1], b64[1]))
    assert out["counts"].tolist() == m["counts"] and np.array_equal(out["label_preds"].cpu().numpy(), b64[2])
    case = {"code": code, "dtype": dtype, "R": g["rois"].shape[1]}
    gate("refine", case, "boxes", out["box3d_lidar"].cpu().numpy(), b64[0], e[0])
    gate("refine", case, "scores", out["scores"].cpu().numpy(), b64[1], e[1])
    if dtype == "f32":
        for b, n in enumerate(m["counts"]):
            gate("refine_recorded", case, "boxes", out["box3d_lidar"][b, :n].cpu().numpy(), g[f"f{b}_box3d_lidar"], m["e_boxes"])
            assert np.array_equal(out["label_preds"][b, :n].cpu().numpy(), g[f"f{b}_label_preds"])
        head = la.RoIHead(4, MODEL_CFG, code_size=code)
        cp, bp = head.generate_predicted_boxes(g["rois"].shape[0], t(g["rois"]), cls, reg)
        gate("refine_recorded", case, "batch_box_preds", bp.cpu().numpy(), g["batch_box_preds"], m["e_boxes"])
        assert cp.shape == (g["rois"].shape[0], g["rois"].shape[1], 1)


@pytest.mark.parametrize("R", [1, 65])
@pytest.mark.parametrize("code", [7, 9])
def test_refine_on_every_shape(code, R):
    """both codes at both sizes (the fixtures hold 7 at 65 and 9 at 1), the last frame without a slot in use"""
    import link_amd as la
    rng = np.random.default_rng(code * 100 + R)
    B = 3
    rois = rng.uniform(-40, 40, (B, R, code)).astype(np.float32)
    rois[..., 3:6] = rng.uniform(0.5, 5, (B, R, 3))
    rois[..., 6] = rng.uniform(-2 * np.pi, 2 * np.pi, (B, R))
    labels = rng.integers(0, 4, (B, R)).astype(np.int64)
    labels[0, 0], labels[-1] = 2, 0
    scores = rng.uniform(0.05, 1, (B, R)).astype(np.float32)
    cls, reg = rng.uniform(-6, 6, B * R).astype(np.float32), (rng.standard_normal((B * R, code)) * 0.3).astype(np.float32)
    out = la.roi_refine(t(rois), t(labels), t(scores), t(cls), t(reg))
    b32, b64 = RO.refine(rois, labels, scores, cls, reg), RO.refine(rois, labels, scores, cls, reg, np.float64)
    assert np.array_equal(out["counts"].cpu().numpy(), b64[3]) and out["counts"][-1] == 0 and out["counts"][0] >= 1
    assert np.array_equal(out["label_preds"].cpu().numpy(), b64[2])
    case = {"code": code, "R": R}
    gate("refine_shapes", case, "boxes", out["box3d_lidar"].cpu().numpy(), b64[0], dist(b32[0], b64[0]))
    gate("refine_shapes", case, "scores", out["scores"].cpu().numpy(), b64[1], dist(b32[1], b64[1]))


# ---- all entries -------------------------------------------------------------------------------------------------------------------
MODEL_CFG = {"SHARED_FC": [16, 16], "CLS_FC": [16], "REG_FC": [16], "DP_RATIO": 0.0, "TARGET_CONFIG": dict(RO.CFG, ROI_PER_IMAGE=8),
             "LOSS_CONFIG": {"CLS_LOSS": "BinaryCrossEntropy", "REG_LOSS": "L1",
                             "LOSS_WEIGHTS": {"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "code_weights": [1.0] * 7}}}


def _all_entries(ins):
    """one call of every entry on fixed inputs -> the list of every output"""
    import link_amd as la
    ext = la.BEVFeatureExtractor(**GEOM)
    tg = la.ProposalTargetLayer(dict(RO.CFG, ROI_PER_IMAGE=8))(ins["batch"], noise=ins["noise"])
    feats = ext.extract(ins["bev"], ins["batch"]["rois"], ins["batch"]["roi_labels"], tg["sel"], 5, rot_col=6)
    x, r = ins["cls"].clone().requires_grad_(True), ins["reg"].clone().requires_grad_(True)
    total, lc, lr, fg = la.roi_loss(x, r, tg["rcnn_cls_labels"], tg["gt_of_rois_canonical"], tg["reg_valid_mask"], [1.0] * 7)
    gx, gr = torch.autograd.grad(total, [x, r])
    ref = la.roi_refine(ins["batch"]["rois"], ins["batch"]["roi_labels"], ins["batch"]["roi_scores"], ins["cls_all"], ins["reg_all"])
    return [tg[k] for k in sorted(tg)] + [feats, total, lc, lr, fg, gx, gr] + [ref[k] for k in sorted(ref)]


def test_two_calls_are_bit_equal_and_a_graph_replays_the_eager_result():
    rng = np.random.default_rng(9)
    B, R, M = 2, 65, 8
    frames = [_frame(rng, R, 6, 8, 7) for _ in range(B)]
    rois, labels, gt = (np.stack([f[k] for f in frames]) for k in range(3))
    rois[..., :2] *= 0.1                                                                           # onto the 7 x 5 map
    gt[..., :2] *= 0.1
    ins = {"batch": _batch(rois, labels, rng.uniform(0.1, 1, (B, R)).astype(np.float32), gt), "noise": torch.rand(B, R + M, device=DEV),
           "bev": torch.randn(B, 16, 5, 7, device=DEV), "cls": torch.randn(B * M, device=DEV), "reg": torch.randn(B * M, 7, device=DEV),
           "cls_all": torch.randn(B * R, device=DEV), "reg_all": torch.randn(B * R, 7, device=DEV)}
    a, b = _all_entries(ins), _all_entries(ins)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _all_entries(ins)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = _all_entries(ins)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, c))


def test_two_stage_refiner_end_to_end():
    import link_amd as la
    rng = np.random.default_rng(21)
    B, R, C, M = 2, 24, 8, 8
    frames = [_frame(rng, R, 5, 6, 7) for _ in range(B)]
    rois, labels, gt = (np.stack([f[k] for f in frames]) for k in range(3))
    rois[..., :2] *= 0.08
    gt[..., :2] *= 0.08
    gt10 = np.concatenate([gt[..., :7], rng.standard_normal((B, gt.shape[1], 2)).astype(np.float32), gt[..., 7:]], -1)    # with velocity
    scores = rng.uniform(0.1, 1, (B, R)).astype(np.float32)
    first = {"box3d_lidar": t(rois), "scores": t(scores), "label_preds": t(labels - 1), "counts": torch.full((B, 1), R, dtype=torch.int32, device=DEV)}
    bev = np.random.default_rng(22).standard_normal((B, C, 5, 7)).astype(np.float32)
    torch.manual_seed(0)
    ext = la.BEVFeatureExtractor(**GEOM)
    head = la.RoIHead(5 * C, MODEL_CFG).to(DEV)
    refiner = la.TwoStageRefiner(ext, head, nms_post_maxsize=R, num_point=5)
    noise = rng.random((B, R + M)).astype(np.float32)
    cfg = MODEL_CFG["TARGET_CONFIG"]
    # training: the loss dictionary, stage by stage against the oracle
    refiner.train()
    losses = refiner(first, t(bev), t(gt10), noise=t(noise))
    assert set(losses) == {"rcnn_loss", "rcnn_loss_cls", "rcnn_loss_reg"}
    ret = head.forward_ret_dict
    got = {k: v.detach().float().cpu().numpy() if v.is_floating_point() else v.cpu().numpy() for k, v in ret.items()}
    o32 = RO.assign(rois, labels, scores, gt, cfg, noise=noise)
    assert np.array_equal(got["sel"], o32["sel"]) and np.array_equal(got["gt_of_rois_src"], o32["gt_of_rois_src"])
    o64 = RO.assign(rois, labels, scores, gt, cfg, sel_in=got["sel"], dtype=np.float64)
    gate("refiner", {"stage": "assign"}, "gt_of_rois", got["gt_of_rois"], o64["gt_of_rois"], dist(o32["gt_of_rois"], o64["gt_of_rois"]))
    f32 = RO.bev_features(bev, rois, labels, got["sel"], 5, rot_col=6, **GEOM)
    f64 = RO.bev_features(bev, rois, labels, got["sel"], 5, rot_col=6, dtype=np.float64, **GEOM)
    gate("refiner", {"stage": "features"}, "roi_features", got["roi_features"], f64, dist(f32, f64))
    w = MODEL_CFG["LOSS_CONFIG"]["LOSS_WEIGHTS"]
    args = (got["rcnn_cls"], got["rcnn_reg"], got["rcnn_cls_labels"], got["gt_of_rois"], got["reg_valid_mask"], w["code_weights"], 1.0, 1.0)
    l32, l64 = RO.loss(*args), RO.loss(*args, np.float64)
    out = np.float64([float(losses["rcnn_loss"].detach()), float(losses["rcnn_loss_cls"]), float(losses["rcnn_loss_reg"]), l64["out"][3]])
    gate("refiner", {"stage": "loss"}, "out", out, l64["out"], dist(l32["out"], l64["out"]))
    losses["rcnn_loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    # inference: features for every proposal, the refined boxes packed
    refiner.eval()
    pred = refiner(first, t(bev))
    f32 = RO.bev_features(bev, rois, labels, None, 5, rot_col=6, **GEOM)
    f64 = RO.bev_features(bev, rois, labels, None, 5, rot_col=6, dtype=np.float64, **GEOM)
    with torch.no_grad():
        bd = {"rois": t(rois), "roi_labels": t(labels), "roi_scores": t(scores), "bev_map": t(bev)}
        head(bd, training=False)
    gate("refiner", {"stage": "features_all"}, "roi_features", bd["roi_features"].cpu().numpy(), f64, dist(f32, f64))
    cls, reg = bd["rcnn_cls"].cpu().numpy(), bd["rcnn_reg"].cpu().numpy()
    b32, b64 = RO.refine(rois, labels, scores, cls, reg), RO.refine(rois, labels, scores, cls, reg, np.float64)
    assert np.array_equal(pred["counts"].cpu().numpy(), b64[3]) and np.array_equal(pred["label_preds"].cpu().numpy(), b64[2])
    gate("refiner", {"stage": "refine"}, "boxes", pred["box3d_lidar"].cpu().numpy(), b64[0], dist(b32[0], b64[0]))
    gate("refiner", {"stage": "refine"}, "scores", pred["scores"].cpu().numpy(), b64[1], dist(b32[1], b64[1]))
    frames_out = refiner(first, t(bev), per_frame=True)
    assert [len(f["scores"]) for f in frames_out] == b64[3].tolist()
