"""tests/conv64.py and tests/conv_frames.py checked without a GPU: the lattice reaches every branch route() distinguishes, the
constants route() restates still stand in the sources, the float64 reference agrees with the oracle, with torch's dense conv3d and
with autograd, and the crafted tables have the counts their names state."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import conv_frames as CF
from conv64 import Conv64, epilogue, grad_magnitudes, grads
from helpers import ROOT, rel_err, s_uniform


def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_lattice_reaches_every_branch():
    reached = set()
    for c in CF.LATTICE:
        reached.update(CF.branch(CF.case_route(c)))
    for _, r in CF.wgrad_routes():
        reached.update(CF.branch(r))
    want = CF.all_branches()
    assert want - reached == set(), sorted(want - reached, key=str)
    assert reached - want == set(), sorted(reached - want, key=str)          # and route() names no branch the enumeration lacks


def test_every_pair_list_width_reaches_the_gemm_the_centre_sum_and_the_weight_gradient():
    """Each of the 12 widths of dispatch_conv_pairs is launched through the f32 pair GEMM and the centre-sum kernel (a direct plan
    runs both) and through link_conv_pairs_wgrad (the square widths up to 64 with WGRAD_TABLE_SQUARE off)."""
    widths = {(c, c) for c in CF.PAIRS_SQUARE} | set(CF.PAIRS_RECT)
    assert len(widths) == 12
    fwd = set()
    for c in CF.LATTICE:
        r = CF.case_route(c)
        if r["kernel"] == "pairs" and r["direct"] and c.rows == "fp32":
            fwd.add((r["CI"], r["CO"]))
    assert fwd == widths, widths ^ fwd
    wg = {(r["CI"], r["CO"]) for _, r in CF.wgrad_routes() if r["kernel"] == "pairs_wgrad"}
    for tkey, ci, co in CF.WGRAD_PAIRS_SQUARE:
        nbr, n_in = CF.table(tkey)
        density, direct = CF.table_stats(nbr, n_in)
        r = CF.route_wgrad(nbr.shape[0], ci, co, nbr.shape[1], density=density, direct=direct, table_square=False)
        assert r == dict(kernel="pairs_wgrad", CI=ci, CO=co, direct=True)
        assert CF.route_wgrad(nbr.shape[0], ci, co, nbr.shape[1])["kernel"] == "table_wgrad"
        wg.add((ci, co))
    assert wg == widths, widths ^ wg


def test_lattice_ids_are_unique_and_cases_are_what_the_issue_lists():
    ids = [CF.case_id(c) for c in CF.LATTICE]
    assert len(ids) == len(set(ids))
    width = [c for c in CF.LATTICE if c.group == "width"]
    assert len(width) == 28 and {(c.cin, c.cout) for c in width} == set(CF.LINK_CONV)
    assert all(CF.table(c.tkey)[0].shape[0] == 1007 for c in width)
    assert all(CF.case_route(c).get("DEEP", True) for c in width)            # MFMA instances: the DEEP one; the others: resident
    nt = {(c.cin, c.cout, CF.table(c.tkey)[0].shape[0]) for c in CF.LATTICE if c.group == "nt"}
    assert {(16, 64, n) for n in (16400, 65600, 131200, 262400)} | {(128, 128, n) for n in (16400, 65600, 131200)} <= nt
    assert max(n for _, _, n in nt) == 262400
    gen = {(c.cin, c.cout) for c in CF.LATTICE if c.group == "generic" and CF.table(c.tkey)[0].shape[1] == 27}
    assert gen == {(1, 1), (3, 5), (12, 40), (17, 65), (20, 129), (8, 193), (4, 256), (144, 144), (48, 64)}
    assert any(c.group == "generic" and CF.table(c.tkey)[0].shape[1] == 125 and c.cin == 16 for c in CF.LATTICE)
    for kernel in ("resident", "mfma"):
        kv = {CF.table(c.tkey)[0].shape[1] for c in CF.LATTICE if c.group == "kvol" and CF.case_route(c)["kernel"] == kernel}
        assert kv == {1, 8, 18}, (kernel, kv)
    assert {CF.table(c.tkey)[0].shape[0] for c in CF.LATTICE if c.group == "edge"} == {1, 15, 16, 17, 63, 64, 65}
    # (e): every forced pair-list case has its table-form twin
    forced = [c for c in CF.LATTICE if c.group == "pairs" and c.form == "pairs"]
    assert forced and all(c._replace(form="table") in CF.LATTICE for c in forced)
    assert all(CF.case_route(c)["kernel"] == "pairs" for c in forced)
    wg = {r["kernel"] for _, r in CF.wgrad_routes()}
    assert wg == {"table_wgrad", "pairs_wgrad", "torch"}
    assert {(r["chunks"], r["extra"]) for _, r in CF.wgrad_routes() if r["kernel"] == "table_wgrad"} == \
        {(16, 0), (32, 0), (64, 0), (16, 48), (32, 96), (64, 192)}


@pytest.mark.parametrize("n,ci,co,want", [
    (16384, 64, 64, dict(kernel="mfma", CI=64, CO=64, NT=1, DEEP=True, capped=False)),
    (16385, 64, 64, dict(kernel="mfma", CI=64, CO=64, NT=1, DEEP=False, capped=False)),
    (65536, 64, 64, dict(kernel="mfma", CI=64, CO=64, NT=1, DEEP=False, capped=False)),
    (65537, 64, 64, dict(kernel="mfma", CI=64, CO=64, NT=2, DEEP=False, capped=False)),
    (131073, 64, 64, dict(kernel="mfma", CI=64, CO=64, NT=4, DEEP=False, capped=False)),
    (131073, 128, 128, dict(kernel="mfma", CI=128, CO=128, NT=2, DEEP=False, capped=True)),
    (131072, 128, 128, dict(kernel="mfma", CI=128, CO=128, NT=2, DEEP=False, capped=False)),
    (262145, 64, 16, dict(kernel="mfma", CI=64, CO=16, NT=4, DEEP=False, capped=True)),
    (98305, 16, 16, dict(kernel="resident", CI=16, CO=16, split=False, NW=8, capped=True)),
    (98304, 16, 16, dict(kernel="resident", CI=16, CO=16, split=False, NW=8, capped=False)),
    (65537, 32, 32, dict(kernel="resident", CI=32, CO=32, split=False, NW=16, capped=True)),
])
def test_route_at_the_voxel_edges(n, ci, co, want):
    assert CF.route(n, ci, co, 27) == want


def test_route_python_side():
    assert CF.route(1000, 16, 16, 27, form="auto", half="fp16")["kernel"] == "resident_amp"
    assert CF.route(1000, 16, 16, 27, form="auto", density=5.0, direct=True)["kernel"] == "resident"
    assert CF.route(1000, 64, 64, 27, form="auto", density=18.0, direct=True)["kernel"] == "mfma"
    assert CF.route(1000, 64, 64, 27, form="auto", density=17.0, direct=True) == \
        dict(kernel="pairs", CI=64, CO=64, gemm="f32", direct=True, c16=False)
    assert CF.route(1000, 64, 64, 27, True, "auto", density=3.0, direct=False)["gemm"] == "split"
    assert CF.route(1000, 16, 32, 27, True, "pairs", density=3.0, direct=True)["gemm"] == "f32"
    assert CF.route(1000, 64, 64, 125, form="auto", density=3.0, direct=True)["kernel"] == "generic"     # 64-bit offset masks
    assert CF.route(1000, 5, 64, 27, form="auto", density=3.0, direct=True)["CI"] == 16
    assert CF.route(1000, 64, 3, 27, form="auto", density=3.0, direct=True)["CO"] == 16
    assert CF.route(1000, 48, 48, 27, form="auto", density=3.0, direct=True)["kernel"] == "mfma"
    assert CF.route_wgrad(4096, 32, 32, 27, link_subm=True) == dict(kernel="table_wgrad", chunks=16, extra=48)
    assert CF.route_wgrad(4096, 32, 32, 8, link_subm=True)["extra"] == 0
    assert CF.route_wgrad(4095, 32, 32, 27, link_subm=True)["extra"] == 0
    assert CF.route_wgrad(1000, 128, 128, 27, density=18.0, direct=True)["kernel"] == "torch"


# ------------------------------------------------------------------------------------------------------------------------------
# the constants, pinned against the literal lines of the sources
# ------------------------------------------------------------------------------------------------------------------------------
def test_conv_hip_pins():
    src = _src("link_amd", "csrc", "conv.hip")
    for line in (
        f"static constexpr int g_conv_wgs = {CF.G_CONV_WGS};",
        "static constexpr int g_conv_nt = 0;",
        "static constexpr int g_conv_deep = 1;",
        "#define CONV_RESIDENT_MIN 1 ",
        "if (wgs > g_conv_wgs) wgs = g_conv_wgs;",
        "int64_t wgs = (tiles + 4 * NT - 1) / (4 * NT);",
        "if (NT == 1 && g_conv_deep && tiles <= 1024) {",
        "constexpr bool nt4_fits = ((size_t)2 * CO * (CI + 4) + (size_t)4 * 27 * 4 * 16) * sizeof(float) <= 160 * 1024 && CO <= 112;",
        "if (tiles > (int64_t)g_conv_wgs * 4 * 2 && nt4_fits) return launch_conv_mfma_nt<CI, CO, 4>(",
        "if (tiles > (int64_t)g_conv_wgs * 4) return launch_conv_mfma_nt<CI, CO, 2>(",
        "static constexpr int TI = CI / 16, TO = CO / 16, KV = 27;",
        "static constexpr int LDW = CI + 4; ",
        "static constexpr int W_FLOATS = KV * CO * LDW;",
        "static constexpr int NW = (W_FLOATS * 4 > 48 * 1024) ? 16 : 8;",
        "static constexpr int LDS_BYTES = W_FLOATS * 4 + NW * (KV + 1) * 16 * 4;",
        "const int per_cu = (160 * 1024) / K::LDS_BYTES;",
        "int64_t wgs = (tiles + K::NW - 1) / K::NW;",
        "if (wgs > 256 * per_cu) wgs = 256 * per_cu;",
        "const bool mfma_ok = (cin & 15) == 0 && (cout & 15) == 0 && cin <= 128 && cout <= 128 && kvol <= 27;",
        "if (mfma_ok && kvol <= 27 && n >= CONV_RESIDENT_MIN) {",
        "const bool split = ep.ln_w != nullptr;",
        "if (n == 0) return LINK_OK;",
    ):
        assert line in src, line
    # the width lists stand once, in dispatch.h; the launchers hold no literal width
    assert _width_pairs("dispatch_conv_table") == CF.LINK_CONV
    assert _width_pairs("dispatch_conv_resident") == CF.RESIDENT
    assert not re.search(r"cin == \d|LINK_CONV", src)
    impl = src[src.index("static int subm_conv_impl(const float *feats, const int32_t *nbr, const float *w, const int32_t *order,\n"
                         "                          int64_t n, int32_t cin, int32_t cout, int32_t kvol, float *out,\n"
                         "                          const conv_epilogue &ep, void *stream) {"):]
    impl = impl[:impl.index("\n}\n")]
    assert impl.count("dispatch_conv_resident(cin, cout,") == 1 and impl.count("dispatch_conv_table(cin, cout,") == 1
    assert impl.index("launch_conv_resident<") < impl.index("dispatch_conv_table(")       # the resident test comes first
    assert impl.index("if (resident) return rc;") < impl.index("dispatch_conv_table(")
    # the generic kernel: channels per lane = (cout + 63) / 64, 1 .. 4
    assert impl.index("if (table) return rc;") < impl.index("dispatch_cpl(cout, [&](auto cpl) {")
    assert "k_subm_conv_generic<decltype(cpl)::value>" in impl
    assert "inline bool dispatch_cpl(int c, F &&f) { return dispatch_int<1, 2, 3, 4>((c + 63) / 64, f); }" in \
        _src("link_amd", "csrc", "dispatch.h")
    amp = src[src.index('extern "C" int link_subm_conv_resident_amp('):]
    assert "dispatch_conv_resident(cin, cout," in amp[:amp.index("\n}\n")]


def _width_pairs(wrapper):
    """The (cin, cout) list of one of dispatch.h's width-pair wrappers, in its order."""
    src = _src("link_amd", "csrc", "dispatch.h")
    fn = src[src.index(f"inline bool {wrapper}(int cin, int cout, F &&f) {{"):]
    fn = fn[:fn.index("\n}\n")]
    return tuple((int(a), int(b)) for a, b in re.findall(r"wp\((\d+), (\d+)\)", fn))


def test_conv_pairs_hip_pins():
    src = _src("link_amd", "csrc", "conv_pairs.hip")
    fn = src[src.index('extern "C" int link_conv_pairs_supported(int32_t cin, int32_t cout) {'):]
    fn = fn[:fn.index("\n}\n")]
    assert "return dispatch_conv_pairs(cin, cout, [](auto, auto) {}) ? 1 : 0;" in fn
    assert _width_pairs("dispatch_conv_pairs") == tuple((c, c) for c in CF.PAIRS_SQUARE) + CF.PAIRS_RECT
    assert CF.PAIRS_SQUARE == (16, 32, 64, 128)
    # six launchers, one list: no literal width and no macro ladder is left in the file
    assert src.count("dispatch_conv_pairs(cin, cout, [&](auto ci, auto co) {") == 6
    assert not re.search(r"cin == \d|LINK_C[PCWSA]\b", src)


def test_elk_py_pins():
    src = _src("link_amd", "elk.py")
    for line in (
        f"PAIR_DENSITY_MAX = {CF.PAIR_DENSITY_MAX}\n",
        f"_RESIDENT_SHAPES = {CF.RESIDENT!r}\n",
        "    return (RESIDENT_FORM and form == \"auto\" and kvol <= 27 and (cin, cout) in _RESIDENT_SHAPES and (not half or AMP_MFMA))\n",
        "    if not L.lib().link_conv_pairs_supported(cin, cout) or nbr.shape[1] > 64:\n",
        "    return plan if plan.density <= PAIR_DENSITY_MAX else None\n",
        "    elif split and SPLIT_MFMA and io == L.IO_F32 and cin >= 32:\n",
        "    c16 = amp and plan.direct and f.dtype in AMP_CONTRIB16 ",
        "AMP_CONTRIB16 = (torch.float16,) ",
        "    square_small = WGRAD_TABLE_SQUARE and cin == cout and cin <= 64 and cin % 4 == 0\n",
        f"        chunks = 16 if n_out < {CF.WGRAD_CHUNK_EDGES[0]} else (32 if n_out < {CF.WGRAD_CHUNK_EDGES[1]} else 64)\n",
        f"        dense_centre = bool(getattr(nbr, \"_link_subm\", False)) and kvol % 2 == 1 and kvol > 1 and n_out >= {CF.WGRAD_CENTRE_MIN}\n",
        "        extra = 3 * chunks if dense_centre else 0\n",
        "RESIDENT_FORM = True ", "AMP_MFMA = True ", "SPLIT_MFMA = True ", "WGRAD_TABLE_SQUARE = True ",
    ):
        assert line in src, line


def test_derived_launch_figures():
    assert CF.res_cfg(16, 16) == (8, 48896) and CF.res_cfg(32, 32) == (16, 153088)
    assert CF.res_cfg(16, 32)[0] == 16 and CF.res_cfg(32, 16)[0] == 16
    assert all(lds <= CF.LDS_LIMIT for _, lds in (CF.res_cfg(*p) for p in CF.RESIDENT))
    assert CF.nt4_fits(16, 64) and CF.nt4_fits(64, 16) and CF.nt4_fits(112, 112) and not CF.nt4_fits(128, 128) and not CF.nt4_fits(64, 128)
    # the NT = 2 image of the widest layer fits the LDS
    assert (2 * 128 * 132 + 4 * 27 * 2 * 16) * 4 <= CF.LDS_LIMIT


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle_on_a_real_map():
    from oracle import link_oracle as O
    co = s_uniform(700, grid=12, seed=3)
    nbr = torch.from_numpy(O.conv_neighbor_table(co.numpy(), 3, 1).astype(np.int32))
    f, w = CF.rows_of(700, 12, 1).double(), CF.weights_of(27, 12, 20, 1).double()
    want = O.subm_conv_torch(f, co, w, 1)
    got = Conv64(f, w, nbr, chunk=256).rows(0, 700)
    assert rel_err(got.numpy(), want.numpy()) < 1e-13


def test_reference_agrees_with_dense_conv3d_on_a_full_grid():
    from oracle import link_oracle as O
    g = 5
    zz, yy, xx = torch.meshgrid(torch.arange(g), torch.arange(g), torch.arange(g), indexing="ij")
    co = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1), torch.zeros(g ** 3, dtype=torch.long)], 1).int()
    perm = torch.randperm(g ** 3, generator=torch.Generator().manual_seed(1))
    co = co[perm]
    nbr = torch.from_numpy(O.conv_neighbor_table(co.numpy(), 3, 1).astype(np.int32))
    cin, cout = 3, 4
    f, w = CF.rows_of(g ** 3, cin, 2).double(), CF.weights_of(27, cin, cout, 2).double()
    got = Conv64(f, w, nbr).rows(0, g ** 3)
    dense = torch.zeros(1, cin, g, g, g, dtype=torch.float64)                        # [batch, c, z, y, x]
    dense[0, :, co[:, 2].long(), co[:, 1].long(), co[:, 0].long()] = f.t()
    # offset k = (x, y, z) with x fastest (get_kernel_offsets, odd volume): weight[co, ci, kz, ky, kx]
    wd = w.reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
    want = torch.nn.functional.conv3d(dense, wd, padding=1)[0][:, co[:, 2].long(), co[:, 1].long(), co[:, 0].long()].t()
    assert rel_err(got.numpy(), want.numpy()) < 1e-13


@pytest.mark.parametrize("tkey", [("crafted", 130, 60, 27, 9), ("granule", False), ("down", "lidar", 400)])
def test_reference_gradients_equal_autograd(tkey):
    nbr, n_in = CF.table(tkey)
    kvol = nbr.shape[1]
    f = CF.rows_of(n_in, 6, 3).double().requires_grad_(True)
    w = CF.weights_of(kvol, 6, 5, 3).double().requires_grad_(True)
    g = CF.rows_of(nbr.shape[0], 5, 4).double()
    # Conv64 detaches its inputs: autograd runs over the formula itself, written out once more
    fp =torch.cat([f, torch.zeros(1, 6, dtype=torch.float64)])
    idx = torch.where(nbr < 0, torch.full_like(nbr, n_in), nbr).long()
    out = sum(fp[idx[:, k]] @ w[k] for k in range(kvol))
    assert rel_err(Conv64(f, w, nbr, chunk=64).rows(0, nbr.shape[0]).numpy(), out.detach().numpy()) < 1e-14
    out.backward(g)
    g_f, g_w = grads(f, w, nbr, g, chunk=64)
    assert rel_err(g_f.numpy(), f.grad.numpy()) < 1e-13 and rel_err(g_w.numpy(), w.grad.numpy()) < 1e-13
    a_f, a_w, pairs = grad_magnitudes(f.detach(), w.detach(), nbr, g)
    assert bool((a_f + 1e-300 >= g_f.abs()).all()) and bool((a_w + 1e-300 >= g_w.abs()).all())
    assert pairs.tolist() == [(nbr[:, k] >= 0).sum().item() for k in range(kvol)]


def test_reference_magnitudes_epilogue_and_contracts():
    nbr, n_in = CF.table(("crafted", 90, 40, 27, 9))
    f, w = CF.rows_of(n_in, 8, 5), CF.weights_of(27, 8, 16, 5)
    ref = Conv64(f, w, nbr, chunk=32)
    x = ref.rows(0, 90)
    A, B = ref.magnitude(0, 90), ref.magnitude1(0, 90)
    assert bool((A >= x.abs()).all()) and ref.max_magnitude() == float(A.max())
    k_present = (nbr >= 0).sum(1)
    assert bool(ref.absent_rows()[1]) and int(ref.absent_rows().sum()) == int((k_present == 0).sum())
    assert bool((x[ref.absent_rows()] == 0).all()) and bool((A[ref.absent_rows()] == 0).all()) and bool((B[ref.absent_rows()] == 0).all())
    assert B[2, 0] == pytest.approx(float(f.abs().double()[nbr[2].long()].sum() + w.abs().double()[:, :, 0].sum()), rel=1e-12)
    # the fp32 evaluation costs about fp32 rounding, and worst_ratio of the fp32 evaluation sits below the fp32 bound
    r32 = Conv64(f, w, nbr, dtype=torch.float32, chunk=32)
    o32 = ref.rel(r32)[0]
    assert 0 < o32 < 1e-6
    assert ref.worst_ratio(r32.rows(0, 90), CF.element_bound(27 * 8, ref.max_magnitude())) < 1.0
    # epilogue: LayerNorm against torch's, affine, addend, ReLU
    ep = CF.ep_params(16, "ln_add_relu", 90)
    y = Conv64(f, w, nbr, ep=ep, chunk=32).rows(0, 90)
    want = torch.relu(ep["addend"].double() + torch.nn.functional.layer_norm(x, (16,), ep["ln_w"].double(), ep["ln_b"].double(), 1e-6))
    assert torch.equal(y, want)
    ident = Conv64(f, w, nbr, ep=CF.ep_params(16, "identity", 90)).rows(0, 90)
    assert torch.equal(ident, x)
    aff = CF.ep_params(16, "affine_add_relu", 90)
    assert torch.equal(epilogue(x, **aff), torch.relu(aff["addend"].double() + (x * aff["ln_w"].double() + aff["ln_b"].double())))
    # contracts: one rounding at the store costs at most the unit roundoff; per-offset roundings cost more, never more than kvol + 1
    f16, w16 = f.half().float(), w.half().float()
    truth = Conv64(f16, w16, nbr)
    end = Conv64(f16, w16, nbr, contract=("end", torch.float16))
    off = Conv64(f16, w16, nbr, contract=("offset", torch.float16, None))
    e_end, e_off = truth.rel(end)[0], truth.rel(off)[0]
    assert 0 < e_end <= 2.0 ** -11 and e_end <= e_off <= 28 * 2.0 ** -11
    bound = CF.element_bound(27 * 8, truth.max_magnitude(), rt=torch.float16, offset_roundings=True)
    assert truth.worst_ratio(off.rows(0, 90), bound) < 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# the frames
# ------------------------------------------------------------------------------------------------------------------------------
def test_crafted_tables_have_the_stated_rows():
    nbr, n_in = CF.table(CF.W_TABLE)
    assert nbr.dtype == torch.int32 and tuple(nbr.shape) == (1007, 27) and n_in == 700
    assert bool((nbr[1] == -1).all()) and bool((nbr[2] >= 0).all()) and bool((nbr[1006] == 699).all())
    assert int(nbr.max()) == 699 and int(nbr.min()) == -1
    assert 0.27 < float((nbr >= 0).float().mean()) < 0.33
    assert CF.table_stats(nbr, n_in)[1] is False and CF.table_stats(nbr, n_in)[0] <= CF.PAIR_DENSITY_MAX
    one, _ = CF.table(("crafted", 1, 50, 27, 5))
    assert tuple(one.shape) == (1, 27) and int((one >= 0).sum()) > 0
    sub, n_in = CF.table(("submlike", 2000, 27, 6))
    assert n_in == 2000 and CF.table_stats(sub, n_in)[1] is True and bool((sub[1, :13] == -1).all()) and int(sub[1, 13]) == 1
    empty, _ = CF.table(("crafted", 0, 50, 27, 1))
    assert tuple(empty.shape) == (0, 27)


@pytest.mark.parametrize("direct", [True, False])
def test_granule_tables_sit_on_the_granule_edge(direct):
    nbr, n_in = CF.table(("granule", direct))
    counts = (nbr >= 0).sum(0).tolist()
    if direct:
        assert counts == [127, 128, 200, 129, 0] and CF.table_stats(nbr, n_in) == (sum(counts) / 200, True)
    else:
        assert counts == [127, 128, 129, 0] and n_in != nbr.shape[0] and CF.table_stats(nbr, n_in)[1] is False


def test_real_and_strided_tables():
    nbr, n = CF.table(("real", "lidar", 3000))
    assert nbr.shape[0] == n and CF.table_stats(nbr, n)[1] is True and CF.table_stats(nbr, n)[0] <= CF.PAIR_DENSITY_MAX
    K = nbr.shape[1]
    j, k = torch.nonzero(nbr >= 0, as_tuple=True)                                    # the symmetry the input gradient rests on
    assert bool((nbr[nbr[j, k].long(), K - 1 - k] == j.int()).all())
    down, n_in = CF.table(("down", "lidar", 3000))
    assert int((down >= 0).sum()) == n_in and down.shape[1] == 8 and down.shape[0] < n_in
    assert sorted(down[down >= 0].tolist()) == list(range(n_in))                     # every input row in exactly one (cell, tap)
    back = CF.table_back(down, n_in)
    assert bool(((back >= 0).sum(1) == 1).all())
    i, k = torch.nonzero(back >= 0, as_tuple=True)
    assert bool((down[back[i, k].long(), k] == i.int()).all())


def test_rows_weights_and_orders_are_seeded():
    assert torch.equal(CF.rows_of(10, 4, 1), CF.rows_of.__wrapped__(10, 4, 1))
    assert float(CF.weights_of(27, 64, 64, 1, True).abs().max()) == 40000.0 and float(CF.weights_of(27, 64, 64, 1).abs().max()) < 2.0 ** 15
    o = CF.order_of(1007)
    assert o.dtype == torch.int32 and sorted(o.tolist()) == list(range(1007)) and o.tolist() != list(range(1007))


# ------------------------------------------------------------------------------------------------------------------------------
# the committed run
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_committed_parity_run_covers_the_lattice_on_the_predicted_routes():
    """profiles/conv_parity.jsonl (one run of tests/test_gpu_conv_lattice.py on an MI355X): every lattice and weight-gradient case
    has its rows, every row's route is the one route() predicts from the frames here, every figure is finite and inside (c)."""
    with open(os.path.join(ROOT, "profiles", "conv_parity.jsonl")) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    fwd = {}
    for r in rows:
        if "predicted" in r:
            assert r["route"] == r["predicted"], r
            fwd.setdefault(r["case"], []).append(r)
        if r["route"]["kernel"] != "none":
            assert math.isfinite(r["rel64"]) and (r["worst_c"] is None or r["worst_c"] <= 1.0), r
    for c in CF.LATTICE:
        got = fwd.get(CF.case_id(c))
        assert got and all(r["route"] == CF.case_route(c) for r in got), CF.case_id(c)
        assert c.group == "empty" or any(r["worst_c"] is not None for r in got), CF.case_id(c)
    wg = {r["case"]: r["route"] for r in rows if r.get("run") == "grad" and r.get("tensor") == "kernel" and r["case"].startswith("wgrad:")}
    for (tkey, ci, co, subm), want in CF.wgrad_routes():
        assert wg.get(CF.wgrad_label(tkey, ci, co, subm)) == want, (tkey, ci, co, subm)
