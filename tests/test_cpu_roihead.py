"""CPU-only checks of the two-stage ROI head (csrc/roihead.hip, section O of include/link_amd.h; link_amd/roihead.py): the restatements of
tests/roi_oracle.py against the fixtures recorded from the reference's own modules (tests/golden/make_golden_roihead.py), the
sampler's counts, membership and uniformity on the oracle, exports and prototypes, argument validation before anything touches a
device, loud failure on CPU tensors, and the state_dict keys of RoIHead.

Float comparisons of the float32 restatement with the reference's float32 recording allow e_ref + 4 ulp of the largest magnitude,
e_ref being the recording's distance from the float64 oracle (the fixture's meta): two float32 evaluations of one formula in
different summation orders lie within that of each other."""
import ctypes
import os

import numpy as np
import pytest

from helpers import ROOT, golden_files, load_golden

import roi_oracle as RO

SECTION_O = ("link_roi_bev_features", "link_roi_assign", "link_roi_loss_forward", "link_roi_loss_backward", "link_roi_refine")
ASSIGN = ["roihead_assign_allclass.npz", "roihead_assign_code9.npz", "roihead_assign_waymo.npz"]
FILES = sorted(ASSIGN + ["roihead_features.npz", "roihead_keys.npz", "roihead_loss_1.npz", "roihead_loss_8.npz", "roihead_loss_512.npz", "roihead_refine_7.npz",
                         "roihead_refine_9.npz"])


def close(a, b, e_ref):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = e_ref + 4 * float(np.spacing(np.float32(np.abs(b).max(initial=0.0))))
    d = float(np.abs(a - b).max(initial=0.0))
    print("distance", d, "allowed", tol)
    return d <= tol


def test_fixtures_are_complete_and_stable():
    assert golden_files("roihead_*.npz") == FILES
    for name in FILES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20), name
    for name in ASSIGN + ["roihead_features.npz"]:
        m = load_golden(name)["meta"]
        assert m["replaced"] <= 0.02 * m["rois"], (name, m["replaced"])              # the 2 % cap of the stabilisation
        assert "compiled from the reference" in m["source"] or "restatement" in m["source"]
    w = load_golden("roihead_assign_waymo.npz")["meta"]
    assert w["rois"] == 500 and all(v > 0 for v in w["lists"][0])                     # fg, hard and easy background all present


def test_points_and_features_restatement_equals_the_reference():
    g = load_golden("roihead_features.npz")
    m = g["meta"]
    geom = {k: m[k] for k in ("pc_start", "voxel_size", "out_stride")}
    B = g["boxes"].shape[0]
    pts = np.stack([RO.box_points(g["boxes"][b], 5).reshape(-1, 2) for b in range(B)])
    assert close(pts, g["points5"][..., :2], m["e_points5"])
    assert np.array_equal(g["points5"][:, :g["boxes"].shape[1], :], g["boxes"][..., :3])
    for P in (1, 5):
        f = RO.bev_features(g["bev"], g["boxes"], None, None, P, **geom)
        assert f.shape == g[f"features{P}"].shape and close(f, g[f"features{P}"], m[f"e_features{P}"])
    # off the map the clamped corners do not give border replication: a point left of column 0 has x0 == x1 == 0 and weights that
    # do not sum to one
    im = np.ones((5, 7, 1), np.float32)
    v = RO.bilinear(im, np.float32([-1.5, 3.25, 6.0, 7.5]), np.float32([2.0, 2.5, 4.0, 2.0]))[:, 0]
    assert v[1] == 1.0 and v[2] == 0.0 and v[0] == 0.0 and v[3] == 0.0             # (x1 - x) (y1 - y) + ... with equal corners


@pytest.mark.parametrize("name", ASSIGN)
def test_assign_restatement_equals_the_reference(name):
    g = load_golden(name)
    m = g["meta"]
    o = RO.assign(g["in_rois"], g["in_roi_labels"], g["in_roi_scores"], g["in_gt"], m["cfg"], sel_in=g["sampled_inds"])
    for k in ("rois", "roi_labels", "roi_scores", "gt_of_rois_src", "reg_valid_mask"):
        assert np.array_equal(o[k], g[k]), k
    assert np.array_equal(o["sel"], g["sampled_inds"])
    for k in ("max_overlaps", "gt_iou_of_rois", "gt_of_rois", "rcnn_cls_labels"):
        assert close(o[k], g[k], m["e_" + k]), k
    # the float64 form assigns alike on these stable inputs
    o64 = RO.assign(g["in_rois"], g["in_roi_labels"], g["in_roi_scores"], g["in_gt"], m["cfg"], sel_in=g["sampled_inds"], dtype=np.float64)
    assert np.array_equal(o64["gt_assignment"], o["gt_assignment"]) and np.array_equal(o64["reg_valid_mask"], g["reg_valid_mask"])
    # and the reference's own draw has the oracle's counts and category membership
    for b, mo in enumerate(g["max_overlaps"]):
        fg, hard, easy = RO.sample_lists(mo, m["cfg"])
        assert [len(fg), len(hard), len(easy)] == m["lists"][b]
        take, repl, nh, ne = RO.sample_counts(len(fg), len(hard), len(easy), m["cfg"])
        s = g["sampled_inds"][b]
        assert take + repl + nh + ne == len(s)
        assert np.isin(s[:take + repl], fg).all() and np.isin(s[take + repl:take + repl + nh], hard).all()
        assert np.isin(s[take + repl + nh:], easy).all() and len(np.unique(s[:take])) == take


def _mo(nfg, nhard, neasy):
    return np.float32([0.9] * nfg + [0.3] * nhard + [0.01] * neasy)


@pytest.mark.parametrize("sizes,want", [((30, 20, 20), (8, 0, 6, 2)), ((3, 20, 20), (3, 0, 10, 3)), ((30, 0, 0), (0, 16, 0, 0)),
                                        ((0, 20, 20), (0, 0, 12, 4)), ((0, 20, 0), (0, 0, 16, 0)), ((0, 0, 20), (0, 0, 0, 16)),
                                        ((30, 20, 0), (8, 0, 8, 0)), ((30, 0, 20), (8, 0, 0, 8)), ((30, 2, 20), (8, 0, 2, 6))])
def test_sampler_counts_in_every_branch(sizes, want):
    cfg = dict(RO.CFG, ROI_PER_IMAGE=16)
    assert RO.sample_counts(*sizes, cfg) == want
    mo = np.random.default_rng(1).permutation(_mo(*sizes))
    rng = np.random.default_rng(2)
    sel, status = RO.sample(mo, rng.random(len(mo) + 16).astype(np.float32), cfg)
    fg, hard, easy = RO.sample_lists(mo, cfg)
    take, repl, nh, ne = want
    assert status == 0 and np.isin(sel[:take + repl], fg).all() and np.isin(sel[take + repl:take + repl + nh], hard).all()
    assert np.isin(sel[take + repl + nh:], easy).all() and len(np.unique(sel[:take])) == take


def test_sampler_rounds_half_to_even_and_flags_no_candidate():
    assert RO.sample_counts(30, 20, 20, dict(RO.CFG, ROI_PER_IMAGE=5))[0] == 2           # np.round(2.5) == 2
    assert RO.sample_counts(30, 20, 20, dict(RO.CFG, ROI_PER_IMAGE=7))[0] == 4           # np.round(3.5) == 4
    sel, status = RO.sample(np.full(9, np.nan, np.float32), np.zeros(9 + 16, np.float32), dict(RO.CFG, ROI_PER_IMAGE=16))
    assert status == 1 and (sel == 0).all()


def test_sampler_chooses_foreground_uniformly():
    cfg = dict(RO.CFG, ROI_PER_IMAGE=16)
    mo = _mo(24, 10, 10)
    rng = np.random.default_rng(7)
    draws, hits = 2000, np.zeros(len(mo))
    for _ in range(draws):
        sel, _ = RO.sample(mo, rng.random(len(mo) + 16).astype(np.float32), cfg)
        hits[sel[:8]] += 1
    p = 8 / 24
    sigma = np.sqrt(draws * p * (1 - p))
    assert (hits[24:] == 0).all() and (np.abs(hits[:24] - draws * p) < 5 * sigma).all(), hits[:24]


@pytest.mark.parametrize("name", ["roihead_loss_1.npz", "roihead_loss_8.npz", "roihead_loss_512.npz"])
def test_loss_restatement_equals_the_reference(name):
    g = load_golden(name)
    m = g["meta"]
    w = m["weights"]
    o = RO.loss(g["cls"], g["reg"], g["labels"], g["gt_of_rois"], g["reg_valid_mask"], w["code_weights"], w["rcnn_cls_weight"], w["rcnn_reg_weight"])
    # e_ref is large where logits beyond about 17 saturate float32's sigmoid to 1 (log(1 - p) then meets the -100 clamp): the fixture
    # of one row has no such logit and pins the formula to float32 rounding
    assert o["out"][3] == g["reg_valid_mask"].sum()
    for k in ("out", "grad_cls", "grad_reg"):
        assert close(o[k].reshape(g[k].shape), g[k], m["e_" + k]), k
    if m["extreme"]:
        assert g["cls"][0] == 200 and g["cls"][1] == -200 and m["e_out"] > 1            # the -100 clamp acts in the recording
    else:
        assert m["e_out"] < 1e-6 and m["e_grad_cls"] < 1e-6


@pytest.mark.parametrize("code", [7, 9])
def test_refine_restatement_equals_the_reference(code):
    g = load_golden(f"roihead_refine_{code}.npz")
    m = g["meta"]
    boxes, scores, labels, counts = RO.refine(g["rois"], g["roi_labels"], g["roi_scores"], g["cls"], g["reg"])
    assert counts.tolist() == m["counts"] and 0 in m["counts"]
    for b, n in enumerate(m["counts"]):
        assert np.array_equal(labels[b, :n], g[f"f{b}_label_preds"]) and (labels[b, n:] == -1).all()
        assert close(boxes[b, :n], g[f"f{b}_box3d_lidar"], m["e_boxes"]) and close(scores[b, :n], g[f"f{b}_scores"], m["e_scores"])
        assert not boxes[b, n:].any() and not scores[b, n:].any()


def test_section_o_symbols_exported_and_prototyped():
    from link_amd import _lib as L
    from link_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in SECTION_O:
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13      # additive entries
    assert L.lib().link_abi_struct_size(10) == -1                         # no new struct
    assert "roihead.hip" in SOURCES
    import link_amd as la
    for name in ("BEVFeatureExtractor", "roi_box_points", "ProposalTargetLayer", "RoIHead", "TwoStageRefiner", "roi_loss", "roi_refine"):
        assert callable(getattr(la, name)), name


def test_section_o_validates_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    OK, ARG = L.LINK_OK, L.LINK_ERR_ARG
    one = ctypes.c_void_p(64)                                            # a non-null pointer nothing dereferences
    st = (ctypes.c_int64 * 4)(35, 1, 7, 1)
    f2 = lambda a, b: (ctypes.c_float * 2)(a, b)                          # noqa: E731
    bev = lambda **k: lib.link_roi_bev_features(*[{**dict(bev=one, io=0, st=st, b=2, c=4, h=5, w=7, boxes=one, r=10, bl=7, rc=6, lab=None, sel=None,
                                                          s=10, p=5, pc=f2(0, 0), vs=f2(1, 1), os=1.0, out=one, stream=None), **k}[n]
                                                  for n in ("bev", "io", "st", "b", "c", "h", "w", "boxes", "r", "bl", "rc", "lab", "sel", "s", "p", "pc",
                                                            "vs", "os", "out", "stream")])                  # noqa: E731
    assert bev(b=0) == OK and bev(s=0, r=0) == OK
    for bad in (dict(bev=None), dict(out=None), dict(boxes=None), dict(st=None), dict(pc=None), dict(vs=None), dict(p=2), dict(p=0), dict(io=3),
                dict(c=0), dict(bl=6), dict(rc=7), dict(s=9), dict(r=1 << 31, s=1 << 31), dict(b=4, r=1 << 29, s=1 << 29), dict(vs=f2(0, 1)),
                dict(os=float("nan")), dict(sel=one, s=(1 << 31) // 5)):
        assert bev(**bad) == ARG, bad
    base = dict(rois=one, lab=one, sc=one, gt=one, noise=one, sel_in=None, b=2, r=65, g=4, m=8, code=7, fg=0.5, by=1, soft=1, cfg=0.75, cbg=0.25,
                lo=0.1, hard=0.8, reg=0.55, outs=[one] * 12, stream=None)

    def assign(**k):
        a = {**base, **k}
        return lib.link_roi_assign(a["rois"], a["lab"], a["sc"], a["gt"], a["noise"], a["sel_in"], a["b"], a["r"], a["g"], a["m"], a["code"], a["fg"],
                                   a["by"], a["soft"], a["cfg"], a["cbg"], a["lo"], a["hard"], a["reg"], *a["outs"], a["stream"])
    for bad in (dict(rois=None), dict(gt=None), dict(noise=None), dict(outs=[one] * 11 + [None]), dict(outs=[None] + [one] * 11), dict(code=8),
                dict(code=9, by=0), dict(m=0), dict(m=1 << 31), dict(r=0), dict(r=1 << 31), dict(g=1 << 31), dict(b=0), dict(fg=1.5),
                dict(hard=-0.1), dict(lo=0.6), dict(cbg=0.8), dict(cfg=float("nan")), dict(lo=0.8, reg=0.9)):
        assert assign(**bad) == ARG, bad
    cw = (ctypes.c_float * 9)(*([1.0] * 9))
    fwd = lambda **k: lib.link_roi_loss_forward(*[{**dict(cls=one, reg=one, io=0, n=8, code=7, lab=one, gt=one, rv=one, cw=cw, wc=1.0, wr=1.0, out=one,
                                                          uc=one, ur=one, stream=None), **k}[n]
                                                  for n in ("cls", "reg", "io", "n", "code", "lab", "gt", "rv", "cw", "wc", "wr", "out", "uc", "ur",
                                                            "stream")])                                       # noqa: E731
    for bad in (dict(cls=None), dict(ur=None), dict(cw=None), dict(code=8), dict(n=0), dict(n=1 << 31), dict(io=5), dict(wc=float("inf"))):
        assert fwd(**bad) == ARG, bad
    assert lib.link_roi_loss_backward(one, one, None, 8, 7, 0, one, one, None) == ARG
    assert lib.link_roi_loss_backward(one, one, one, 8, 6, 0, one, one, None) == ARG
    assert lib.link_roi_loss_backward(one, one, one, 1 << 31, 7, 0, one, one, None) == ARG
    assert lib.link_roi_refine(None, None, None, None, None, 0, 0, 5, 7, None, None, None, None, None) == OK
    assert lib.link_roi_refine(one, one, one, one, one, 0, 2, 5, 8, one, one, one, one, None) == ARG
    assert lib.link_roi_refine(one, one, one, one, None, 0, 2, 5, 7, one, one, one, one, None) == ARG
    assert lib.link_roi_refine(one, one, one, one, one, 0, 2, 5, 7, one, one, one, None, None) == ARG
    assert lib.link_roi_refine(one, one, one, one, one, 0, 2, 1 << 31, 7, one, one, one, one, None) == ARG


def test_roihead_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_table
    from link_amd import build as hip_build
    hip_build.build()
    rows = kernel_table(os.path.join(ROOT, "link_amd", "lib", "obj", "roihead.o"))
    names = [r[0] for r in rows]
    for k, count in (("k_roi_bev", 6), ("k_roi_overlap", 1), ("k_roi_sample", 1), ("k_roi_loss<", 3), ("k_roi_loss_bwd", 3), ("k_roi_refine", 3)):
        assert sum(k in nm for nm in names) == count, (k, names)
    for name, vgpr, agpr, sgpr, lds, scratch, wg in rows:
        print(name, vgpr, agpr, sgpr, lds, scratch, wg)
        assert int(scratch) == 0 and int(wg) == 256 and int(lds) <= 65536, (name, scratch, wg, lds)


MODEL_CFG = {"SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256], "DP_RATIO": 0.3, "TARGET_CONFIG": RO.CFG,
             "LOSS_CONFIG": {"CLS_LOSS": "BinaryCrossEntropy", "REG_LOSS": "L1",
                             "LOSS_WEIGHTS": {"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "code_weights": [1.0] * 7}}}


def test_roi_head_state_dict_is_the_reference_s():
    import torch
    import link_amd as la
    m = load_golden("roihead_keys.npz")["meta"]
    torch.manual_seed(0)
    head = la.RoIHead(m["input_channels"], m["model_cfg"], num_class=1, code_size=7)
    sd = head.state_dict()
    assert list(sd.keys()) == m["keys"] and [list(v.shape) for v in sd.values()] == m["shapes"]
    assert abs(float(head.reg_layers[-1].weight.detach().std()) - 0.001) < 2e-4 and abs(m["reg_last_std"] - 0.001) < 2e-4
    assert float(head.cls_layers[-1].bias.abs().max()) == 0
    w = head.shared_fc_layer[0].weight                                   # xavier_normal_: std = sqrt(2 / (fan_in + fan_out))
    assert abs(float(w.detach().std()) - np.sqrt(2.0 / (w.shape[0] + w.shape[1]))) < 5e-3
    with pytest.raises(NotImplementedError):
        la.ProposalTargetLayer(dict(RO.CFG, CLS_SCORE_TYPE="raw_roi_iou"))


def test_cpu_tensors_fail_loudly():
    import torch
    import link_amd as la
    from link_amd._lib import LinkAmdError
    ext = la.BEVFeatureExtractor([-3.5, -2.5], [0.25, 0.25], 4)
    with pytest.raises(LinkAmdError):
        ext.extract(torch.zeros(1, 4, 5, 7), torch.zeros(1, 3, 7))
    with pytest.raises(LinkAmdError):
        ext({"bev_feature": torch.zeros(1, 5, 7, 4)}, [torch.zeros(3, 3)], 1)
    layer = la.ProposalTargetLayer(RO.CFG)
    batch = {"rois": torch.zeros(1, 4, 7), "roi_labels": torch.zeros(1, 4, dtype=torch.int64), "roi_scores": torch.zeros(1, 4),
             "gt_boxes_and_cls": torch.zeros(1, 2, 8)}
    with pytest.raises(LinkAmdError):
        layer(batch)
    with pytest.raises(LinkAmdError):
        la.roi_loss(torch.zeros(4), torch.zeros(4, 7), torch.zeros(4), torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), [1.0] * 7)
    with pytest.raises(LinkAmdError):
        la.roi_refine(batch["rois"], batch["roi_labels"], batch["roi_scores"], torch.zeros(4), torch.zeros(4, 7))
    head = la.RoIHead(4, MODEL_CFG)
    with pytest.raises(LinkAmdError):
        head(dict(batch, roi_features=torch.zeros(1, 4, 4)), training=True)
    # the torch restatement of the points agrees with the oracle (it serves a map that requires grad)
    boxes = torch.tensor(load_golden("roihead_features.npz")["boxes"][0])
    pts = la.roi_box_points(boxes, 5).numpy()
    assert pts.shape == (5 * boxes.shape[0], 3)
    assert np.abs(pts[:, :2] - RO.box_points(boxes.numpy(), 5).reshape(-1, 2)).max() <= 1e-6
