"""The sparse convolution (csrc/conv.hip, csrc/conv_pairs.hip, the routing of link_amd/elk.py) behind a per-case float64 gate over
a stated lattice of kernel instances and table edges -- the branches of subm_conv_impl / launch_conv_mfma / launch_conv_resident /
_conv_pairs / _conv_weight_grad that the networks' widths and frame sizes never reach under a tight reference:

  width     all 24 width pairs of the table form at n = 1 007 (20 MFMA pairs on the DEEP instance with a ragged last tile, the 4
            resident pairs plain = exact f32 and fused = fp16 split: 28 instances);
  nt        NT = 1 plain / 2 / 4 and the capped grids just past each voxel edge at (16, 64) and (128, 128); the resident kernel's
            persistent stride at NW = 8 and NW = 16;
  generic   CPL 1 .. 4, cin > 128, multiples of 16 outside the table, kvol = 125, LayerNorm over masked lanes;
  kvol      kvol 1 / 8 / 18 on a resident and an MFMA instance;
  edge      n_out of 1 .. 65 over 50 input rows; every crafted table has an all-absent row, a full row and a row of n_in - 1;
  epilogue  LayerNorm / affine, addend, ReLU on the MFMA kernel;
  pairs     the pair-list form next to the table form on the same case: direct and non-direct plans, 127 / 128 / 129 pairs per
            offset, the split GEMM and its `big` flag;   half: 16-bit rows on the pair-list and the resident AMP kernels;
  empty     n = 0;   and the weight / input gradients below.
(16-bit rows forced onto the fp32 table kernel with form="table" are widened, multiplied by unrounded weights and rounded once: no
network takes that path and no 16-bit contract describes it, so it is not in the lattice.)  No kernel defect was found by this file.
tests/conv_frames.py holds the tables, the lattice and route(); tests/test_cpu_conv_frames.py checks them without a device.

Gates, per case (tests/conv64.py is the float64 reference; nothing in a bound comes from the kernels):
  (a) every element finite; rows whose table row is all absent are exactly 0, or exactly the epilogue of 0 (the library allocates
      the result, so these rows carry the "was it written" check: torch.empty hands back whatever the allocator held, and
      _poison leaves it a freed block of the result's size full of NaN just before the call);
  (b) gate_rows of tests/ref64.py: rel64 <= 4 o32 + 2 o_round + 2e-6 under the ceilings 1e-4 / 4e-3 / 3e-2, o32 and o_round from
      the reference's own fp32 and rounded evaluations;
  (c) per element, against the convolution before any epilogue (fused cases run once more with affine scale 1, shift 0, no ReLU):
      |out - ref| <= E, conv_frames.element_bound, derived as follows with u = 2^-24, T = kvol * cin products per element,
      A = sum |f| |w| over them:
        fp32 forms     E32 = (T + 2) u A + (T + 2) u max(A) 1e-3: the bound of an fp32 dot product of T terms in any order (the
                       products are single roundings or fused), and a floor of one thousandth of the tensor's largest;
        split form     x = xh + xl + ex with xh = fp16(x), xl = fp16(x - xh): |x - xh| <= 2^-11 |x|, |xl| <= 2^-11 |x|, and
                       |ex| <= 2^-22 |x| + 2^-25 (the second term where xl is an fp16 subnormal, spacing 2^-24); the same for w.
                       The kernels keep xh wh + xh wl + xl wh = (x - ex)(w - ew) - xl wl, so a product is off by at most
                       |x ew| + |w ex| + |xl wl| + |ex ew| <= 3 2^-22 |x w| + 2^-25 (|x| + |w|) (+ terms of 2^-44): summed,
                       3 2^-22 A + 2^-25 B with B = sum (|x| + |w|) (Conv64.magnitude1).  Each kept product is exact in fp32
                       (11 x 11 bits) and there are 3 T of them: E = (3 T + 2) u (A + max(A) 1e-3) + 3 2^-22 A + 2^-25 B.
                       A row or weight at or beyond 2^15 takes the exact instruction (`big`): E32 <= E holds all the more;
        16-bit forms   the truth is over the rounded rows and weights, whose products are exact in fp32, so the sum costs E32;
                       the store rounds once: + v (|ref| + E32) with v = 2^-11 / 2^-8, + 2^-25 for an fp16 subnormal result.
                       The pair-list fp16 form on a submanifold table rounds every offset's product row but the centre's first:
                       + v (A + E32) + 27 2^-25 before the store's term.
  (d) a second call is bit-equal; order=None and a seeded permutation are bit-equal on the MFMA and generic kernels.  The
      resident kernel alternates two accumulator sets over the offsets THE TILE has, so a row's association depends on which 15
      rows share its tile: there a permuted order is gated by (a) - (c) instead;
  (e) form="table" and form="pairs" on the same case both pass (a) - (c).
Gradients: g_w through the table kernel at c in {4 .. 64} x n_out in {40 .. 60 000} x _link_subm set / unset (chunks 16 / 32 / 64,
centre_extra 0 / 48 / 96 / 192), through the pair list (direct, non-direct, padded first layer, strided table) and the torch
fallback; g_f through _SubmConv on a real map and _GatherConv on a stride-2 map.  Per tensor: finite, rel <= 4 o32 + 2e-6 under the
1e-4 ceiling, and per element the dot-product bound with the tensor's own term count (pairs of the offset for g_w, kvol * cout for
g_f).  Every case leaves its figures in conv_parity.jsonl in the directory LINK_AMD_PARITY_DIR names before any verdict
(profiles/conv_parity.jsonl is one run)."""
import functools

import pytest
import torch

import conv_frames as CF
from conv64 import U32, Conv64, epilogue, grad_magnitudes, grads
from ref64 import gate_rows, record_row

pytestmark = pytest.mark.gpu
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PARITY = "conv_parity.jsonl"


def _record(row):
    record_row(row, PARITY)


# ------------------------------------------------------------------------------------------------------------------------------
# shared, unchanged once made: tables, rows, weights, references
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(tkey, mark=None):
    """The table on the device; `mark`: the builder's structural mark (_link_subm) where a case wants it set."""
    nbr = CF.table(tkey)[0].cuda().contiguous()
    if mark is not None:
        nbr._link_subm = mark
    return nbr


@functools.lru_cache(maxsize=None)
def _rows(n, c, seed, dtn="fp32"):
    return CF.rows_of(n, c, seed).to(DT[dtn]).cuda()


@functools.lru_cache(maxsize=None)
def _weights(kvol, cin, cout, seed, big=False):
    return CF.weights_of(kvol, cin, cout, seed, big).cuda()


def _ep_dev(cout, kind, n_out, dtn):
    """epilogue()'s arguments on the device; the addend in the row type (what the 16-bit entry points read)."""
    ep = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in CF.ep_params(cout, kind, n_out).items()}
    if ep["addend"] is not None and dtn != "fp32":
        ep["addend"] = ep["addend"].to(DT[dtn])
    return ep


def _contract(case, route):
    """Where the contract of the form `route` names rounds (tests/conv64.py)."""
    if case.rows == "fp32":
        return None
    dt = DT[case.rows]
    if route["kernel"] == "pairs" and route["c16"]:
        return ("offset", dt, CF.table(case.tkey)[0].shape[1] // 2)
    assert route["kernel"] in ("pairs", "resident_amp"), route
    return ("end", dt)


@functools.lru_cache(maxsize=None)
def _ref(case, epkind):
    """(truth, o32, o_round) of a case under an epilogue kind (None: the plain convolution): computed once, shared, unchanged.
    16-bit rows: the truth runs over the rows, weights and addend rounded to the row type."""
    nbr = _table(case.tkey)
    n_out, kvol = nbr.shape
    n_in = CF.table(case.tkey)[1]
    f = _rows(n_in, case.cin, 1, case.rows)
    w = _weights(kvol, case.cin, case.cout, 1, case.big)
    w = w if case.rows == "fp32" else w.to(DT[case.rows])
    ep = _ep_dev(case.cout, epkind, n_out, case.rows) if epkind else None
    truth = Conv64(f, w, nbr, ep=ep)
    o32, ok = truth.rel(Conv64(f, w, nbr, dtype=torch.float32, ep=ep))
    assert ok or n_out == 0
    contract = _contract(case, CF.case_route(case))
    o_round = truth.rel(Conv64(f, w, nbr, ep=ep, contract=contract))[0] if contract else 0.0
    return truth, o32, o_round


def _observed_route(case, nbr):
    """route() from what the call actually saw: the tensors' shapes and, where a pair plan was consulted, the plan the LIBRARY built."""
    plan = getattr(nbr, "_link_pairs", None) if case.form != "table" else None
    density, direct = (plan.density, plan.direct) if plan not in (None, False) else (None, None)
    if density is None and case.form == "auto":
        density, direct = CF.table_stats(*CF.table(case.tkey))               # no plan: resident / unsupported widths / n = 0
    return CF.route(nbr.shape[0], case.cin, case.cout, nbr.shape[1], epilogue=case.ep is not None, form=case.form,
                    half=False if case.rows == "fp32" else case.rows, density=density, direct=direct)


def _poison(n_out, cout, dt):
    """The library allocates its result with torch.empty: leave a freed block of exactly that size full of NaN for the caching
    allocator to hand out, so that a row the kernel never writes most likely reads as NaN and not as a stale right answer."""
    if n_out:
        torch.full((n_out, cout), float("nan"), dtype=dt, device="cuda")


def _call(case, epkind, order):
    import link_amd.elk as E
    nbr = _table(case.tkey)
    n_out, kvol = nbr.shape
    _poison(n_out, case.cout, DT[case.rows])
    f = _rows(CF.table(case.tkey)[1], case.cin, 1, case.rows)
    w = _weights(kvol, case.cin, case.cout, 1, case.big)
    if epkind is None:
        return E.subm_conv(f, w, nbr, order, form=case.form)
    ep = _ep_dev(case.cout, epkind, n_out, case.rows)
    return E.subm_conv_ln_add_relu(f, w, nbr, order, ep["ln_w"], ep["ln_b"], ep["eps"], ep["addend"], relu=ep["relu"],
                                   form=case.form, affine=ep["affine"])


def _gate(case, route, epkind, out, label):
    """(a), (b) and -- before the epilogue -- (c) on one result; the row is on file before any verdict."""
    truth, o32, o_round = _ref(case, epkind)
    dt = DT[case.rows]
    assert out.dtype == dt and tuple(out.shape) == (truth.n, truth.C), (out.dtype, tuple(out.shape))
    row = dict(case=CF.case_id(case), run=label, ep=epkind, route=route, predicted=CF.case_route(case), worst_c=None, zero_rows_exact=None)
    absent = truth.absent_rows()
    if bool(absent.any()):                                                   # (a): exactly the epilogue of zero, in fp32, stored once
        zero = torch.zeros(int(absent.sum()), truth.C, dtype=torch.float32, device="cuda")
        if epkind:
            ep = dict(_ep_dev(case.cout, epkind, truth.n, case.rows))
            if ep["addend"] is not None:
                ep["addend"] = ep["addend"][absent].float()
            zero = epilogue(zero, **ep)
        row["zero_rows_exact"] = bool(torch.equal(out[absent], zero.to(dt)))
    if epkind in (None, "identity"):                                         # (c)
        split = route.get("split", False) or route.get("gemm") == "split"
        contract = _contract(case, route)
        bound = CF.element_bound(truth.kvol * truth.cin, truth.max_magnitude(), split=split, rt=None if dt == torch.float32 else dt,
                                 offset_roundings=bool(contract and contract[0] == "offset"))
        row["worst_c"] = truth.worst_ratio(out, bound, need_b=split)
    gate_rows(row, truth, o32, out, dt, record=_record, o_round=o_round)     # (a) finite, (b)
    assert row["route"] == row["predicted"], row
    assert row["zero_rows_exact"] in (None, True), row
    assert row["worst_c"] is None or row["worst_c"] <= 1.0, row


# ------------------------------------------------------------------------------------------------------------------------------
# the forward lattice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CF.LATTICE if c.group != "empty"], ids=CF.case_id)
def test_forward_lattice(case):
    nbr = _table(case.tkey)
    n_out = nbr.shape[0]
    perm = CF.order_of(n_out).cuda()
    kinds = [None] if case.ep is None else ["identity", case.ep]
    for epkind in kinds:
        out = _call(case, epkind, None)
        route = _observed_route(case, nbr)
        _gate(case, route, epkind, out, "order=None")
        again = _call(case, epkind, None)
        assert torch.equal(out, again), (CF.case_id(case), epkind, "second call differs", int((out != again).any(1).sum()))
        if case.form != "table":
            continue                                                         # `order` is a table-kernel argument
        permuted = _call(case, epkind, perm)
        if route["kernel"] == "resident":                                    # (d): the association depends on the tile's rows
            _gate(case, route, epkind, permuted, "order=perm")
        else:
            assert torch.equal(out, permuted), (CF.case_id(case), epkind, "order=perm differs", int((out != permuted).any(1).sum()))


@pytest.mark.parametrize("case", [c for c in CF.LATTICE if c.group == "empty"], ids=CF.case_id)
def test_an_empty_table_returns_an_empty_result(case):
    """n = 0: an empty result of the right width and type, nothing launched (no plan is built for the table either)."""
    nbr = _table(case.tkey)
    assert _observed_route(case, nbr) == CF.case_route(case) == dict(kernel="none")
    for epkind in (None, "ln"):
        out = _call(case, epkind, None)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (0, case.cout) and out.dtype == torch.float32
    assert getattr(nbr, "_link_pairs", None) is None
    _record(dict(case=CF.case_id(case), run="n=0", route=dict(kernel="none"), predicted=dict(kernel="none")))


# ------------------------------------------------------------------------------------------------------------------------------
# gradients
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grad_ref(tkey, cin, cout):
    """(f, w, g_out, g64, o32, magnitudes) of a gradient case: float64 gradients from the definition, what the same formula costs
    in fp32 per tensor, and the per-element magnitudes with the term counts."""
    nbr = _table(tkey)
    n_in = CF.table(tkey)[1]
    f, w, g = _rows(n_in, cin, 2), _weights(nbr.shape[1], cin, cout, 2), _rows(nbr.shape[0], cout, 3)
    g64 = dict(zip(("feats", "kernel"), grads(f, w, nbr, g)))
    g32 = dict(zip(("feats", "kernel"), grads(f, w, nbr, g, dtype=torch.float32)))
    o32 = {k: float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64}
    a_f, a_w, pairs = grad_magnitudes(f, w, nbr, g)
    return f, w, g, g64, o32, dict(feats=a_f, kernel=a_w, pairs=pairs)


def _gate_grad(label, route, tensor, got, g64, o32, A, terms):
    """One gradient tensor: finite, rel <= 4 o32 + 2e-6 under 1e-4, and per element |got - g64| <= (terms + 2) u (A + max(A) 1e-3)
    (`terms`: a number, or a tensor broadcasting over A -- the pairs of each offset for g_w)."""
    finite = bool(torch.isfinite(got).all())
    d = (got.double() - g64).abs()
    rel = float(d.max() / g64.abs().max()) if finite else float("inf")
    terms = torch.as_tensor(terms, dtype=torch.float64, device=A.device)
    fac = (terms + 2.0) * U32
    bnd = fac * A + fac.max() * float(A.max()) * 1e-3
    worst = float(torch.where(d > 0, d / bnd, torch.zeros_like(d)).max()) if finite else float("inf")
    row = dict(case=label, run="grad", tensor=tensor, route=route, rel64=rel, o32=o32, worst_c=worst)
    _record(row)
    assert finite and got.dtype == torch.float32 and got.shape == g64.shape, row
    assert float(g64.abs().max()) > 0 and rel < 1e-4 and rel <= 4.0 * o32 + 2e-6, row
    assert worst <= 1.0, row
    return row


def _weight_grad_case(tkey, cin, cout, mark, want):
    import link_amd.elk as E
    nbr = _table(tkey, mark)
    f, w, g, g64, o32, A = _grad_ref(tkey, cin, cout)
    shape = (nbr.shape[1], cin, cout)
    a = E._conv_weight_grad(f, g, nbr, shape)
    plan = getattr(nbr, "_link_pairs", None)
    density, direct = (plan.density, plan.direct) if plan not in (None, False) else CF.table_stats(*CF.table(tkey))
    route = CF.route_wgrad(nbr.shape[0], cin, cout, nbr.shape[1], link_subm=bool(mark), density=density, direct=direct)
    label = CF.wgrad_label(tkey, cin, cout, bool(mark))
    _gate_grad(label, route, "kernel", a, g64["kernel"], o32["kernel"], A["kernel"], A["pairs"].double()[:, None, None])
    assert route == want, (route, want)
    b = E._conv_weight_grad(f, g, nbr, shape)
    assert torch.equal(a, b), (label, "second call differs")


@pytest.mark.parametrize("c", CF.WGRAD_C)
@pytest.mark.parametrize("n", CF.WGRAD_N)
def test_weight_gradient_table_kernel(n, c):
    """k_subm_conv_wgrad + k_subm_wgrad_reduce over their split thresholds; c = 4 .. 20 masks lanes, n = 40 leaves all chunks but
    one empty (their partial slots still have to come back as zeros)."""
    for subm in (False, True):
        want = CF.route_wgrad(n, c, c, 27, link_subm=subm)
        assert want["kernel"] == "table_wgrad"
        _weight_grad_case(CF.wgrad_table_key(n, subm), c, c, True if subm else None, want)


@pytest.mark.parametrize("tkey,cin,cout", CF.WGRAD_PAIRS + CF.WGRAD_TORCH, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_weight_gradient_pair_list_and_fallback(tkey, cin, cout):
    nbr, n_in = CF.table(tkey)
    density, direct = CF.table_stats(nbr, n_in)
    want = CF.route_wgrad(nbr.shape[0], cin, cout, nbr.shape[1], density=density, direct=direct)
    assert want["kernel"] == ("torch" if (tkey, cin, cout) in CF.WGRAD_TORCH else "pairs_wgrad")
    _weight_grad_case(tkey, cin, cout, None, want)


@pytest.mark.parametrize("tkey,cin,cout", CF.WGRAD_PAIRS_SQUARE, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_weight_gradient_pair_list_square_widths(tkey, cin, cout, monkeypatch):
    """link_conv_pairs_wgrad at the square widths up to 64, which _conv_weight_grad gives to the table kernel while
    WGRAD_TABLE_SQUARE is set: with the switch off they run the pair list, under the same gate as every other width."""
    import link_amd.elk as E
    monkeypatch.setattr(E, "WGRAD_TABLE_SQUARE", False)
    nbr = _table(tkey)
    f, w, g, g64, o32, A = _grad_ref(tkey, cin, cout)
    shape = (nbr.shape[1], cin, cout)
    a = E._conv_weight_grad(f, g, nbr, shape)
    plan = nbr._link_pairs
    route = CF.route_wgrad(nbr.shape[0], cin, cout, nbr.shape[1], density=plan.density, direct=plan.direct, table_square=False)
    _gate_grad(CF.wgrad_label(tkey, cin, cout, False) + ":pairs", route, "kernel", a, g64["kernel"], o32["kernel"], A["kernel"],
               A["pairs"].double()[:, None, None])
    assert route == dict(kernel="pairs_wgrad", CI=cin, CO=cout, direct=True), route
    assert torch.equal(a, E._conv_weight_grad(f, g, nbr, shape)), "second call differs"


@pytest.mark.parametrize("cin,cout", [(64, 64), (16, 16), (48, 48), (32, 64), (128, 32)])
def test_input_gradient_through_submconv(cin, cout):
    """_SubmConv on a real (symmetric) map: g_f = the forward kernels on g_out with the flipped, transposed weights; g_w with it."""
    import link_amd.elk as E
    tkey = ("real", "lidar", 3000)
    f, w, g, g64, o32, A = _grad_ref(tkey, cin, cout)
    nbr = _table(tkey)
    label = f"submconv:{cin}x{cout}"
    outs = []
    for _ in range(2):
        fl, wl = f.clone().requires_grad_(True), w.clone().requires_grad_(True)
        E._SubmConv.apply(fl, wl, nbr, None).backward(g)
        outs.append((fl.grad, wl.grad))
    route = CF.route(nbr.shape[0], cout, cin, 27, form="auto", density=nbr._link_pairs.density if getattr(nbr, "_link_pairs", None) else
                     CF.table_stats(*CF.table(tkey))[0], direct=True)
    _gate_grad(label, route, "feats", outs[0][0], g64["feats"], o32["feats"], A["feats"], 27 * cout)
    _gate_grad(label, route, "kernel", outs[0][1], g64["kernel"], o32["kernel"], A["kernel"], A["pairs"].double()[:, None, None])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (label, "second backward differs")


@pytest.mark.parametrize("cin,cout", [(32, 64), (16, 16), (48, 48)])
def test_input_gradient_through_gatherconv(cin, cout):
    """_GatherConv on a stride-2 map: g_f = the forward kernels on g_out over the opposite direction's table."""
    import link_amd.elk as E
    tkey = ("down", "lidar", 3000)
    f, w, g, g64, o32, A = _grad_ref(tkey, cin, cout)
    nbr = _table(tkey)
    back = CF.table_back(*CF.table(tkey)).cuda()
    fl, wl = f.clone().requires_grad_(True), w.clone().requires_grad_(True)
    E._GatherConv.apply(fl, wl, nbr, back).backward(g)
    label = f"gatherconv:{cin}x{cout}"
    route = CF.route(back.shape[0], cout, cin, 8, form="auto", density=1.0, direct=False)
    _gate_grad(label, route, "feats", fl.grad, g64["feats"], o32["feats"], A["feats"], 8 * cout)
    _gate_grad(label, route, "kernel", wl.grad, g64["kernel"], o32["kernel"], A["kernel"], A["pairs"].double()[:, None, None])
