"""GPU checks of deformable convolution (csrc/dcn.hip, section R of include/link_amd.h; link_amd/dcn.py) against the restatements of
tests/dcn_oracle.py.

The gate is the project's (tests/test_gpu_roihead.py): a float output's largest distance from the float64 oracle may be at most
4 e_ref + 1 fp32 ulp of the tensor's largest magnitude, plus half an ulp of the format for a 16-bit tensor (rounded once).  e_ref is
the distance of the float32 restatement from the float64 one on the same inputs: the reference's own kernels run on CUDA only and no
recording of them exists, so the same formula evaluated in float32 by torch stands in for the reference's float32 error.  It is
measured here, never taken from the code under test.  grad_input, which the kernel sums with atomics, is held to the same rule (the
factor 4 covers another summation order).  A 16-bit case is the 16-bit values: both restatements run on their exact widenings.

The random offset families keep every sample coordinate at least 1/16 from an integer, where the offset gradient is discontinuous
(float32 and float64 may floor differently there); the integer family is exact in both precisions and tests the floor branch.  With
the ReLU epilogue the upstream gradient is zero where the float64 pre-activation is within 1e-4 of 0, the mask's own discontinuity.
Every case asserts deform_conv_native(...), so the torch composition cannot stand in for the kernels.  Each comparison appends
(e_dev, e_ref, bound) to dcn_parity.jsonl under LINK_AMD_PARITY_DIR before the verdict (profiles/dcn_parity.jsonl is one run)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ref64 import record_row

import dcn_oracle as DO

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}         # relative, of the largest magnitude
FORMS = [(64, 64, 4), (8, 6, 4), (16, 80, 1), (12, 64, 3)]                                    # C, O, deformable groups
MAPS = [(1, 5, 7), (3, 5, 7), (1, 9, 11), (3, 9, 11), (1, 17, 19), (3, 17, 19)]               # B, H, W
GEOMS = {"head": (3, 3, 1, 1, 1), "s2d2": (3, 3, 2, 0, 2), "1x1": (1, 1, 1, 0, 1), "3x1": (3, 1, (2, 1), (1, 0), 1)}   # kh kw stride pad dil
FAMILIES = ["zeros", "uniform", "normal", "integer", "nonfinite"]
NAMES = ("out", "grad_input", "grad_offset", "grad_weight")


def gate(test, case, name, got, want64, e_ref, out_dtype=torch.float32):
    got, want64 = got.detach().double().cpu().numpy(), want64.detach().double().cpu().numpy()
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    assert np.isfinite(got).all(), (test, case, name)
    big = float(np.abs(want64).max(initial=0.0))
    bound = 4 * float(e_ref) + float(np.spacing(np.float32(big))) + HALF_ULP[out_dtype] * big
    d = float(np.abs(got - want64).max(initial=0.0))
    print(test, case, name, "e_dev", d, "e_ref", float(e_ref), "bound", bound)
    record_row({"test": test, **case, "component": name, "e_dev": d, "e_ref": float(e_ref), "bound": bound}, name="dcn_parity.jsonl")
    assert d <= bound, (test, case, name, d, bound)


def dist(a, b):
    return float((a.double() - b.double()).abs().max())


def _reference(x, off, w, go, geom, dg, relu, backward=True):
    """float64 and float32 restatements on the same values: (out, gx, goff, gw) each, and the upstream gradient actually used"""
    kh, kw, stride, pad, dil = geom
    kwargs = dict(stride=stride, pad=pad, dil=dil, dg=dg, relu=relu)
    if not backward:
        with torch.no_grad():
            return (DO.dcn(x.double(), off.double(), w.double(), **kwargs),), (DO.dcn(x.float(), off.float(), w.float(), **kwargs),), go
    if relu:
        pre = DO.dcn(x.double(), off.double(), w.double(), stride, pad, dil, dg)
        go = torch.where(pre.abs() < 1e-4, torch.zeros_like(go), go)
    r64 = DO.grads(DO.dcn, x.double(), off.double(), w.double(), go.double(), **kwargs)
    r32 = DO.grads(DO.dcn, x.float(), off.float(), w.float(), go.float(), **kwargs)
    return r64, r32, go


def _native(x, off, w, go, geom, dg, relu, backward=True):
    import link_amd as la
    kh, kw, stride, pad, dil = geom
    xr, fr, wr = (t.to(DEV).requires_grad_(backward) for t in (x, off, w))
    assert la.deform_conv_native(xr, fr, wr, stride, pad, dil, 1, dg)
    fn = la.deform_conv_relu if relu else la.deform_conv
    out = fn(xr, fr, wr, stride, pad, dil, 1, dg)
    assert out.dtype == x.dtype and out.is_contiguous()
    if not backward:
        return (out,)
    gx, gf, gw = torch.autograd.grad(out, (xr, fr, wr), go.to(DEV))
    return out.detach(), gx, gf, gw


def _run(test, form, bhw, gname, family, relu, dtype, seed=0, backward=True):
    C, O, dg = form
    B, H, W = bhw
    geom = GEOMS[gname]
    dt = DTYPES[dtype]
    x, off, w, go, bad = DO.make_case(B, C, O, dg, H, W, geom[0], geom[1], geom[2], geom[3], geom[4], family, seed)
    x, off, w, go = (t.to(dt) for t in (x, off, w, go))                                # the case is these values
    case = {"C": C, "O": O, "dg": dg, "B": B, "H": H, "W": W, "geom": gname, "family": family, "relu": int(relu), "dtype": dtype}
    r64, r32, go = _reference(x, off, w, go, geom, dg, relu, backward)
    got = _native(x, off, w, go, geom, dg, relu, backward)
    for name, g, a, b in zip(NAMES, got, r64, r32):
        assert g.dtype == dt
        gate(test, case, name, g, a, dist(a, b), dt)
    if family == "zeros":
        conv = F.conv2d(x.double(), w.double(), None, geom[2], geom[3], geom[4])
        conv = torch.relu(conv) if relu else conv
        gate(test, case, "out_vs_conv2d", got[0], conv, dist(r32[0], conv), dt)
    if family == "nonfinite":
        assert bad.any() and not got[2].cpu()[bad].any()                               # zero offset gradient at those entries
    return x, off, got


def _cover(k, n):
    return k % n


@pytest.mark.parametrize("bhw", MAPS, ids=lambda m: "b%dx%dx%d" % m)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "c%do%dg%d" % f)
def test_forms_and_maps(form, bhw):
    """every channel form on every map size and batch, the head's geometry, fp32; the offset family and the ReLU rotate with the case"""
    k = FORMS.index(form) * len(MAPS) + MAPS.index(bhw)
    _run("forms_maps", form, bhw, "head", FAMILIES[_cover(k + FORMS.index(form), len(FAMILIES))], relu=bool(k & 1), dtype="f32", seed=k)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("gname", list(GEOMS))
def test_geometries_and_families(gname, family):
    """every geometry with every offset family, B = 3 on the 9 x 11 map (a pixel tile straddles images), fp32, ReLU on and off"""
    k = list(GEOMS).index(gname) * len(FAMILIES) + FAMILIES.index(family)
    form = FORMS[1] if k & 1 else FORMS[3]
    for relu in (False, True):
        _run("geoms_families", form, (3, 9, 11), gname, family, relu=relu, dtype="f32", seed=100 + k)


def test_normal_offsets_cross_every_border_of_the_small_map():
    """sigma = 3 on the 5 x 7 map: most samples leave the map, and h <= -1, -1 < h < 0, H-1 < h < H and h >= H all occur (w alike)"""
    form, (B, H, W), geom = FORMS[0], MAPS[1], GEOMS["head"]
    x, off, got = _run("borders", form, (B, H, W), "head", "normal", relu=False, dtype="f32", seed=7)
    h, w = DO.coords(off.double(), H, W, 3, 3, 1, 1, 1, form[2])
    for v, n in ((h, H), (w, W)):
        assert (v <= -1).any() and ((v > -1) & (v < 0)).any() and ((v > n - 1) & (v < n)).any() and (v >= n).any()
    outside = ~((h > -1) & (w > -1) & (h < H) & (w < W))
    assert float(outside.double().mean()) > 0.5
    frac = (h - torch.floor(h)).min(), (w - torch.floor(w)).min(), (torch.ceil(h) - h).min(), (torch.ceil(w) - w).min()
    assert min(float(f) for f in frac) >= 1 / 16 - 1e-6


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("family", ["zeros", "normal", "integer", "nonfinite"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_sixteen_bit(dtype, family, relu):
    _run("sixteen_bit", FORMS[0], (3, 5, 7), "head", family, relu=relu, dtype=dtype, seed=200)
    _run("sixteen_bit", FORMS[3], (1, 9, 11), "s2d2", family, relu=relu, dtype=dtype, seed=201)


@pytest.mark.parametrize("O", [100, 130])
def test_wide_outputs(O):
    """O above 64 and above 128: the kernels' two wider output tilings (the forms above cover O <= 64 and O = 80)"""
    _run("wide", (20, O, 2), (3, 5, 7), "head", "normal", relu=True, dtype="f32", seed=500 + O)
    _run("wide", (20, O, 2), (1, 9, 11), "s2d2", "nonfinite", relu=False, dtype="f16", seed=501 + O)


def test_production_pitch_forward():
    """180 x 180, B = 1, C = O = 64, dg = 4: the nuScenes head's map, forward only"""
    _run("pitch180", FORMS[0], (1, 180, 180), "head", "normal", relu=True, dtype="f32", seed=300, backward=False)


def test_reproducible_and_needs_input_grad():
    import link_amd as la
    C, O, dg = FORMS[0]
    x, off, w, go, _ = DO.make_case(3, C, O, dg, 17, 19, 3, 3, 1, 1, 1, "normal", 400)
    runs = [_native(x, off, w, go, GEOMS["head"], dg, relu=True) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])                                         # output, bit for bit
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])  # grad_offset and grad_weight as well
    assert dist(runs[0][1], runs[1][1]) <= 1e-5 * float(runs[0][1].abs().max())        # grad_input: atomics, last bits only
    plain = _native(x, off, w, go, GEOMS["head"], dg, relu=False)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        ts = [t.to(DEV).requires_grad_(n) for t, n in zip((x, off, w), need)]
        la.deform_conv(*ts, 1, 1, 1, 1, dg).backward(go.to(DEV))
        assert [t.grad is not None for t in ts] == list(need)
        assert all(torch.equal(t.grad, ref) for t, ref in list(zip(ts, plain[1:]))[1:] if t.grad is not None)
        if need[0]:
            assert dist(ts[0].grad, plain[1]) <= 1e-5 * float(plain[1].abs().max())


def test_graph_capture_of_a_feature_adaption():
    import link_amd as la
    torch.manual_seed(0)
    fa = la.FeatureAdaption(16, 16, deformable_groups=4).to(DEV)
    with torch.no_grad():
        fa.conv_offset.weight.normal_(0, 0.3)
    params = list(fa.parameters())
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(3, 16, 9, 11, generator=g).to(DEV) for _ in range(3)]
    gos = [torch.randn(3, 16, 9, 11, generator=g).to(DEV) for _ in range(3)]

    def step(x, go):
        return (fa(x),) + torch.autograd.grad(fa(x), [x] + params, go)

    sx, sgo = xs[0].clone().requires_grad_(True), gos[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                                             # warm-up: the workspace and torch's own kernels
            step(sx, sgo)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sx, sgo)
    for x, go in zip(xs[1:], gos[1:]):
        with torch.no_grad():
            sx.copy_(x)
            sgo.copy_(go)
        graph.replay()
        want = step(x.clone().requires_grad_(True), go)
        # Not bit equality: the offsets come from torch's own convolution, whose algorithm (and summation order) may differ between a
        # captured and an eager call, and so may its backward; the gradient of x is partly the atomics' sum.  Sums of a few hundred
        # fp32 terms: 1e-5 of the largest magnitude.  (Bit equality of this library's kernels: test_reproducible_and_needs_input_grad.)
        for k, (a, b) in enumerate(zip(outs, want)):
            assert torch.isfinite(a).all() and dist(a, b) <= 1e-5 * float(b.abs().max()), k


def test_dcn_head_end_to_end():
    """DCNSepHead -> CenterHeadLoss -> backward reaches the deformable layers; the same maps decode"""
    import link_amd as la
    import centerloss_oracle as CO
    heads = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    torch.manual_seed(0)
    head = la.DCNSepHead(64, 2, heads).to(DEV)
    H, W = 9, 11
    boxes, classes = CO.make_case(2, (2,), H, W, 6, 5, n_cap=8)
    assigner = la.CenterTargetAssigner((2,), CO.OSF, CO.VS, CO.geometry(W, H), CO.OVERLAP, 8, CO.MIN_RADIUS)
    example = assigner(torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV))
    x = torch.randn(2, 64, H, W, device=DEV)
    assert la.deform_conv_native(x, head.feature_adapt_cls.conv_offset(x), head.feature_adapt_cls.conv_adaption.weight, 1, 1, 1, 1, 4)
    preds = head(x)
    assert set(preds) == set(heads) | {"hm"} and preds["hm"].shape == (2, 2, H, W)
    crit = la.CenterHeadLoss((2,), 0.25, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0])
    loss = crit(example, [preds])["loss"][0]
    loss.sum().backward()
    for fa in (head.feature_adapt_cls, head.feature_adapt_reg):
        for p in (fa.conv_adaption.weight, fa.conv_offset.weight, fa.conv_offset.bias):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    cfg = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
           "nms": {"nms_pre_max_size": 100, "nms_post_max_size": 20, "nms_iou_threshold": 0.2},
           "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075]}
    with torch.no_grad():
        rets = la.CenterHeadDecoder(cfg, [2]).predict([{k: v.detach() for k, v in head.eval()(x).items()}])
    assert len(rets) == 2 and all(torch.isfinite(r["box3d_lidar"]).all() and r["box3d_lidar"].shape[1] == 9 for r in rets)
