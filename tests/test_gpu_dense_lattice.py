"""The dense-cell R_core forward (ElkCorePlan(layout="dense"), ElkCoreBatch) behind a per-case float64 gate over a stated lattice of
kernels and cell occupancies -- the branches of link_elk_core_dense_forward / launch_k2 that uniform frames at coordinates 0 .. 255,
coord_div = 1, groups 1 / 2 and nn.Linear's initial weights never reach:

  a. the kernel-selection lattice (tests/dense_frames.py, LATTICE): widths 16 .. 128, groups 1 .. 8, every k1_form / k2_form, each
     at coord_div 1 and 2 (the DD = true instance of every K2 kernel, the division in every K1 form); half rows on the timed shape;
  b. slot capacity s^3 = 512 > 352: the unfused pre_mix + insert and per-cell sum kernels, the fused gather kernels behind them at
     C = 64; half rows and the batch entry point refuse that grid, slot_cap = 352 brings the fused kernels back;
  c. occupancy edges: a cell of exactly k voxels, neighbours in cell order summing to 352 and 353, every cell full at k = 8 / 27,
     rim strips over cells of 40 .. 71 voxels, one voxel, two voxels, the eight corners, an empty upper grid and batch item, n = 0;
  d. large theta: ~2 000 rad on the fast sincos path, and the slow path (the launch-wide bound of dc_theta_leaves_fast_range past
     32768) both with theta exact in fp32 (tight gate) and with the weights times 20 (theta ~ 4e4);
  e. the batch entry point on the frames of c and d, bit for bit the per-frame plan.

Every case: parameters of a seeded ELKBlock (cos_x: alpha uniform in (0.5, 1.5)), a result buffer pre-filled with NaN, then
  * gate_rows of tests/ref64.py against Ref64(..., coord_div=...): finite; rel64 < 1e-4 (fp32) / 4e-3 (fp16) / 3e-2 (bf16);
    rel64 <= 4 o32 + 2 o_round + 2e-6 -- nothing in a bound comes from the kernels;
  * check() clean and the cell counters back at zero;
  * a second cold run and a warm run (build_index=False) bit-equal to the first.
The one-voxel frame under `sin` is analytically zero before the final LayerNorm (f sin cos - f cos sin): no relative error exists
there, and gate_zero_rows holds the kernels' residue against that of the reference's own fp32 evaluation instead.
absolute=False drops the fixed 1e-4 on the two `far` frames of d, where fp32 evaluation of the formula itself costs about 1e-4
(theta ~ 2 000) and 2e-3 (weights times 20).  The gate on the times-20 frame is therefore LOOSE, about 1e-2: it is there to catch a
broken slow path (a wrong quadrant, a skipped reduction: errors of order 1), not rounding; the exact frame gates the same path
tightly.  Each case's figures go to dense_parity.jsonl in the directory LINK_AMD_PARITY_DIR names (profiles/dense_parity.jsonl is
one run).  The frames, their counts and which launcher branch a case reaches are checked without a GPU by
tests/test_cpu_dense_frames.py.

Found by b: the own-cell K2 kernel (k_dc_gather_demod_own) under cos_x gave rows that depended on a voxel's rank in its cell's slot
list by 1 - 4 ulp (~200 of the 2 862 rows of `s8` between two cold runs: the unfused insert leaves the records in arrival order) --
the compiler fused a * b + c differently in the two voxel slots of a pair.  Fixed in csrc/dense_gather_own_impl.h."""
import copy
import functools

import pytest
import torch

import dense_frames as DF
from ref64 import Ref64, gate_rows, gate_zero_rows

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


# ------------------------------------------------------------------------------------------------------------------------------
# shared, unchanged once made: blocks, frames, references
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block(c, groups, op, pos="init"):
    return copy.deepcopy(DF.block(c, groups, op, pos)).cuda().eval()


def _bind(obj, blk):
    alpha = blk.alpha if blk.baseop == "cos_x" else None
    args = (blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, alpha, blk.norm.weight,
            blk.norm.bias)
    obj.bind(*args)
    return obj


def _geometry(fkey):
    """fkey: ("lat", s, r) -- the lattice frame -- or (name, seed) of a named frame.  (coords on the CPU, bounds, s)."""
    if fkey[0] == "lat":
        return DF.lattice_frame(fkey[1], fkey[2]) + (fkey[1],)
    return DF.frame(*fkey)


@functools.lru_cache(maxsize=None)
def _frame(fkey, c, dt):
    co = _geometry(fkey)[0]
    seed = fkey[1] if fkey[0] != "lat" else 1
    return DF.rows_of(co.shape[0], c, seed).to(dt).cuda(), co.cuda()


@functools.lru_cache(maxsize=None)
def _ref(fkey, c, groups, op, pos, r, div, dt):
    """(float64 reference, o32) of a frame under a parameter set: computed once, shared, left unchanged."""
    f, co = _frame(fkey, c, dt)
    params = DF.params_of(_block(c, groups, op, pos))
    kw = dict(baseop=op, groups=groups, coord_div=div)
    s = _geometry(fkey)[2]
    ref = Ref64(f, co, params, s, r, **kw)
    r32 = Ref64(f, co, params, s, r, dtype=torch.float32, **kw)
    o32, ok = ref.rel(r32)
    assert ok
    return ref, (o32 if (fkey[0], op) not in DF.ANALYTIC_ZERO else r32)


def _gate(label, fkey, c, groups, op, pos, ref, o32, out, dt, absolute=True):
    """gate_rows -- or, where the truth is analytically zero (dense_frames.ANALYTIC_ZERO: `o32` is then the fp32 evaluation
    itself), gate_zero_rows on the scale of the norm weights."""
    if (fkey[0], op) in DF.ANALYTIC_ZERO:
        scale = float(_block(c, groups, op, pos).norm.weight.detach().abs().max())
        return gate_zero_rows(label, ref, o32, out, scale, record=True)
    return gate_rows(label, ref, o32, out, dt, absolute=absolute, record=True)


def _plan(fkey, c, groups, op, pos, r, div=1.0, bounds=None, **kw):
    import link_amd as la
    co, own, s = _geometry(fkey)
    plan = la.ElkCorePlan(co.shape[0], c, op, c // groups, r, s, bounds or own, "cuda", coord_div=div, layout="dense", **kw)
    assert plan.dense
    return _bind(plan, _block(c, groups, op, pos))


def _route(plan, fkey, c, groups, op, pos, r, div, half=False, bounds=None):
    """What the plan is about to launch (tests/dense_frames.py, route) from ITS grid, slot capacity and tuning words."""
    t = plan.buf.tune
    blk = _block(c, groups, op, pos)
    bound = DF.theta_bound(bounds or _geometry(fkey)[1], plan.s, div, blk.pos_weight[0].weight, blk.alpha if op == "cos_x" else None)
    return DF.route(c, groups, op, r, int(plan.dcg.k), list(plan.grid.dim), coord_div=div, half=half, slow=bound >= DF.FAST_RANGE,
                    k1_form=int(t.k1_form), k2_form=int(t.k2_form), mode=int(t.mode))


def _steps(plan, f, co):
    """Cold, cold again and warm, each into NaN: bit-equal; status and cell counters clean after every step."""
    outs = []
    for build in (True, True, False):
        out = torch.full((f.shape[0], f.shape[1]), NAN, dtype=f.dtype, device="cuda")
        got = plan.run(f, co, build_index=build, out=out)
        plan.check()
        assert got.data_ptr() == out.data_ptr() and int(plan.cnt.abs().sum()) == 0, "cell counters not cleaned by the step"
        outs.append(out)
    differ = [(int((o != outs[0]).any(1).sum()), float((o.float() - outs[0].float()).abs().max())) for o in outs[1:]]
    return outs[0], differ


def _bit_equal(differ, what):
    """The verdict on _steps' second cold and warm runs: (rows that differ, max |difference|) must be (0, 0) for both."""
    assert differ[0] == (0, 0.0), (what, "second cold run differs: (rows, max|d|)", differ[0])
    assert differ[1] == (0, 0.0), (what, "warm run differs: (rows, max|d|)", differ[1])


def _case(fkey, c, groups, op, pos, r, div, dtn, forms, group, absolute=True, want_slow=False, **plan_kw):
    """One plan through `forms` ([(tuning, expected route subset or None)]): every form stepped and gated; {form number: rows}."""
    dt = DTYPES[dtn]
    f, co = _frame(fkey, c, dt)
    ref, o32 = _ref(fkey, c, groups, op, pos, r, div, dt)
    plan = _plan(fkey, c, groups, op, pos, r, div, **plan_kw)
    rows = {}
    for i, (tuning, want) in enumerate(forms):
        plan.set_tuning(**tuning)
        assert (int(plan.buf.tune.k1_form), int(plan.buf.tune.k2_form), int(plan.buf.tune.mode)) == DF.tuning_of(c, op, **tuning)
        got = _route(plan, fkey, c, groups, op, pos, r, div, half=dt != torch.float32)
        assert "refused" not in got and got["div"] == (div != 1.0) and got["slow"] == want_slow, (tuning, got)
        if want:
            assert {k: got.get(k) for k in want} == want, (tuning, got)
        rows[i], differ = _steps(plan, f, co)
        label = dict(rows_differing_cold2_warm=differ, group=group, frame="/".join(str(v) for v in fkey), C=c, groups=groups, op=op, pos=pos, r=r, div=div, rows=dtn,
                     tuning=tuning, k1=got["k1"], k2=got["k2"], slow=got["slow"])
        _gate(label, fkey, c, groups, op, pos, ref, o32, rows[i], dt, absolute)     # the figures are on file before any verdict
        _bit_equal(differ, tuning)
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# a. the kernel-selection lattice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,forms", DF.LATTICE, ids=[DF.case_id(c) for c, _ in DF.LATTICE])
def test_kernel_selection_lattice(case, forms):
    c, groups, op, s, r, div = case
    _case(("lat", s, r), c, groups, op, "init", r, div, "fp32", forms, "a")


@pytest.mark.parametrize("dtn", ["fp16", "bf16"])
@pytest.mark.parametrize("op", ["cos", "sin"])
@pytest.mark.parametrize("r", [2, 3])
def test_lattice_half_rows_coord_div_2(r, op, dtn):
    """The C = 64, groups 2 row at coord_div = 2 with half rows, default forms: the gate through the truth rounded to the row type."""
    _case(("lat", 7, r), 64, 2, op, "init", r, 2.0, dtn, [(dict(), dict(k1="mm", k2="quad", div=True))], "a")


# ------------------------------------------------------------------------------------------------------------------------------
# b. slot capacity above 352
# ------------------------------------------------------------------------------------------------------------------------------
UNFUSED = dict(fused=False, k1="premix_insert+modsum")
# C, groups, op -> the K2 kernel at r = 2 / r = 3 behind the unfused K1 (it does not depend on the slot capacity)
S8_CASES = {(64, 2, "cos"): ("quad", "quad"), (64, 1, "cos"): ("split", "split"), (64, 1, "cos_x"): ("single", "own"),
            (32, 1, "sin"): ("gather+demod",) * 2, (128, 1, "cos"): ("gather+demod",) * 2}


def _s8_want(c, groups, op, r):
    return dict(UNFUSED, k2=S8_CASES[(c, groups, op)][r - 2])


@pytest.mark.parametrize("c,groups,op", list(S8_CASES))
@pytest.mark.parametrize("r", [2, 3])
def test_capacity_512_runs_the_unfused_kernels(r, c, groups, op):
    forms = [(dict(), _s8_want(c, groups, op, r))]
    if c == 64:                          # the insert leaves the records in arrival order: every K2 form must take them in any order
        forms += [(dict(k2_form=4), dict(UNFUSED, k2="own")), (dict(k2_form=1), dict(UNFUSED, k2="single"))]
    _case(("s8", 1), c, groups, op, "init", r, 1.0, "fp32", forms, "b")


@pytest.mark.parametrize("c,groups,op,r", [(64, 2, "cos", 3), (32, 1, "sin", 2), (128, 1, "cos", 3)])
def test_capacity_512_coord_div_2(c, groups, op, r):
    _case(("s8", 1), c, groups, op, "init", r, 2.0, "fp32", [(dict(), _s8_want(c, groups, op, r))], "b")


@pytest.mark.parametrize("groups,op,r", [(2, "cos", 3), (2, "sin", 2), (1, "cos_x", 3)])
def test_a_cell_of_512(groups, op, r):
    _case(("s8_full", 1), 64, groups, op, "init", r, 1.0, "fp32", [(dict(), UNFUSED)], "b")


def test_capacity_512_refuses_half_rows_and_the_batch():
    """A refusal is loud: no quiet fall-back to another kernel or another row type."""
    import link_amd as la
    from link_amd._lib import LinkAmdError
    fkey = ("s8", 1)
    plan = _plan(fkey, 64, 2, "cos", "init", 3)
    assert "refused" in _route(plan, fkey, 64, 2, "cos", "init", 3, 1.0, half=True)
    for dt in (torch.float16, torch.bfloat16):
        f, co = _frame(fkey, 64, dt)
        with pytest.raises(LinkAmdError):
            plan.run(f, co)
    f, co = _frame(fkey, 64, torch.float32)                             # the plan still serves fp32 rows
    ref, o32 = _ref(fkey, 64, 2, "cos", "init", 3, 1.0, torch.float32)
    out, differ = _steps(plan, f, co)
    gate_rows(dict(group="b", frame="s8/1", note="after the refusals"), ref, o32, out, record=True)
    _bit_equal(differ, "after the refusals")
    with pytest.raises(LinkAmdError):
        la.ElkCoreBatch(2, f.shape[0], 64, "cos", 32, 3, 8, _geometry(fkey)[1], "cuda")


@pytest.mark.parametrize("op,r", [("cos", 3), ("sin", 2)])
def test_slot_cap_352_brings_the_fused_kernels_back(op, r):
    """The same s = 8 frame (counts below 352) with slot_cap = 352."""
    forms = [(dict(), dict(fused=True, k1="mm", k2="quad")), (dict(k1_form=0), dict(fused=True, k1="range", k2="quad"))]
    _case(("s8", 1), 64, 2, op, "init", r, 1.0, "fp32", forms, "b", slot_cap=DF.LCAP)
    _case(("s8", 1), 64, 2, op, "init", r, 1.0, "fp16", forms[:1], "b", slot_cap=DF.LCAP)


@pytest.mark.parametrize("op,r", [("cos", 3), ("sin", 2)])
def test_slot_cap_352_with_a_cell_of_exactly_352(op, r):
    """The fused kernels' capacity used to the last record (the wave's LDS list, LCAP): no status bit, no voxel dropped."""
    forms = [(dict(), dict(fused=True, k1="mm", k2="quad")), (dict(k1_form=0), dict(k1="range")), (dict(k1_form=1), dict(k1="tiles")),
             (dict(k1_form=16), dict(k1="range", writeback=True)), (dict(k2_form=0), dict(k2="quad")), (dict(k2_form=4), dict(k2="own"))]
    _case(("s8_352", 1), 64, 2, op, "init", r, 1.0, "fp32", forms, "b", slot_cap=DF.LCAP)


def test_slot_cap_3_is_refused():
    from link_amd._lib import LinkAmdError
    fkey = ("s8", 1)
    f, co = _frame(fkey, 64, torch.float32)
    with pytest.raises(LinkAmdError):
        _plan(fkey, 64, 2, "cos", "init", 3, slot_cap=3).run(f, co)


# ------------------------------------------------------------------------------------------------------------------------------
# c. occupancy edges
# ------------------------------------------------------------------------------------------------------------------------------
OCC_FORMS = ([(dict(k1_form=f), dict(k1=n, k2="quad")) for f, n in ((0, "range"), (1, "tiles"), (2, "mm"))] +
             [(dict(k2_form=f, k2_zsplit=z), dict(k2=n)) for z in (1, 3) for f, n in ((0, "quad"), (16, "quad"), (4, "own"), (8, "split"))])


@pytest.mark.parametrize("name", DF.OCCUPANCY)
@pytest.mark.parametrize("op", ["cos", "sin"])
@pytest.mark.parametrize("r", [2, 3])
def test_occupancy_edges(r, op, name):
    rows = _case((name, 1), 64, 2, op, "init", r, 1.0, "fp32", OCC_FORMS, "c")
    if name in ("solid3", "solid2", "deep_strips13", "deep_strips5"):   # rim strips == square rim tiles, bit for bit
        for z in (0, 1):
            a, b = rows[3 + 4 * z], rows[4 + 4 * z]
            assert OCC_FORMS[3 + 4 * z][0]["k2_form"] == 0 and OCC_FORMS[4 + 4 * z][0]["k2_form"] == 16
            assert torch.equal(a, b), (name, "strips != square rim tiles", int((a != b).any(1).sum()))


@pytest.mark.parametrize("name", ["full", "solid3", "solid2"])
@pytest.mark.parametrize("c,groups,op,r", [(32, 2, "sin", 3), (16, 1, "cos_x", 2)])
def test_full_and_solid_at_the_other_widths(c, groups, op, r, name):
    k1 = [(dict(k1_form=f), dict(fused=True, k2="gather+demod")) for f in ((0, 1, 2) if c == 32 else (0, 1))]
    _case((name, 1), c, groups, op, "init", r, 1.0, "fp32", [(dict(), None)] + k1, "c")


@pytest.mark.parametrize("r", [2, 3])
def test_solid_fp16(r):
    forms = [(dict(), dict(k1="mm", k2="quad")), (dict(k1_form=0), dict(k1="range")), (dict(k2_form=0), dict(k2="quad"))]
    _case(("solid3", 1), 64, 2, "cos", "init", r, 1.0, "fp16", forms, "c")


def test_an_empty_frame():
    """n = 0, pinned as the code serves it today: the entry point returns LINK_OK without a launch -- no row and no status word is
    touched -- and the next frame through the same plan is right."""
    fkey = ("full", 1)
    plan = _plan(fkey, 64, 2, "cos", "init", 3)
    f, co = _frame(fkey, 64, torch.float32)
    ref, o32 = _ref(fkey, 64, 2, "cos", "init", 3, 1.0, torch.float32)
    plan.out.fill_(NAN)
    none = plan.run(torch.empty((0, 64), device="cuda"), torch.empty((0, 4), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    plan.check()
    assert tuple(none.shape) == (0, 64) and bool(torch.isnan(plan.out).all()) and int(plan.cnt.abs().sum()) == 0
    out, differ = _steps(plan, f, co)
    gate_rows(dict(group="c", frame="full/1", note="after n = 0"), ref, o32, out, record=True)
    _bit_equal(differ, "after n = 0")
    plan.run(f[:0], co[:0], build_index=False)
    plan.check()


# ------------------------------------------------------------------------------------------------------------------------------
# d. large theta
# ------------------------------------------------------------------------------------------------------------------------------
FAR = [("far", "init", False, False), ("far", "x20", False, True), ("exact_far", "exact", True, True)]   # frame, pos_weight, absolute, slow


@pytest.mark.parametrize("name,pos,absolute,slow", FAR, ids=["far", "far_x20", "exact_far"])
@pytest.mark.parametrize("op", ["cos", "sin"])
def test_large_theta_every_form(op, name, pos, absolute, slow):
    dims = DF.grid_of(DF.frame(name)[1], 7)[1]          # exact_far's box starts off a cell boundary: 6 x 6 x 5 cells, no rim strips
    strips = dims[0] % 4 == 1 or dims[1] % 4 == 1
    assert strips == (name == "far")
    forms = [(t, dict(w, rim="square") if (w.get("rim") == "strips" and not strips) else w) for t, w in DF._row1(3)]
    _case((name, 1), 64, 2, op, pos, 3, 1.0, "fp32", forms, "d", absolute=absolute, want_slow=slow)


@pytest.mark.parametrize("name,pos,absolute,slow,div", [f + (1.0,) for f in FAR] + [FAR[2] + (2.0,)],
                         ids=["far", "far_x20", "exact_far", "exact_far_div2"])
@pytest.mark.parametrize("c,groups,op,r", [(64, 1, "cos_x", 2), (32, 1, "sin", 3)])
def test_large_theta_other_shapes(c, groups, op, r, name, pos, absolute, slow, div):
    forms = [(dict(), None), (dict(k1_form=0), dict(k1="range"))] + ([(dict(k1_form=1), dict(k1="tiles"))] if c == 32 else
                                                                      [(dict(k2_form=4), dict(k2="own"))])
    _case((name, 1), c, groups, op, pos, r, div, "fp32", forms, "d", absolute=absolute, want_slow=slow)


@pytest.mark.parametrize("op", ["cos", "sin"])
def test_exact_far_fp16(op):
    forms = [(dict(), dict(k1="mm", k2="quad")), (dict(k1_form=0), dict(k1="range"))]
    _case(("exact_far", 1), 64, 2, op, "exact", 3, 1.0, "fp16", forms, "d", want_slow=True)


# ------------------------------------------------------------------------------------------------------------------------------
# e. the batch entry point
# ------------------------------------------------------------------------------------------------------------------------------
def _batch_case(fkeys, bounds, op, r, pos="init", absolute=True, dtn="fp32", slot_cap=0):
    """One ElkCoreBatch call over the frames, twice: every frame bit-equal to the per-frame plan with k1_form 0, k2_form 0 on the
    same grid, every frame through the gate, check() clean."""
    import link_amd as la
    dt = DTYPES[dtn]
    blk = _block(64, 2, op, pos)
    frames = [_frame(k, 64, dt) for k in fkeys]
    s = _geometry(fkeys[0])[2]
    nmax = max(f.shape[0] for f, _ in frames)
    batch = _bind(la.ElkCoreBatch(len(frames), nmax, 64, op, 32, r, s, bounds, "cuda", slot_cap=slot_cap), blk)
    calls = []
    for _ in range(2):
        outs = [torch.full((f.shape[0], 64), NAN, dtype=dt, device="cuda") for f, _ in frames]
        got = batch.run([f for f, _ in frames], [co for _, co in frames], outs=outs)
        torch.cuda.synchronize()
        batch.check()
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
        calls.append(outs)
    plan = _bind(la.ElkCorePlan(nmax, 64, op, 32, r, s, bounds, "cuda", layout="dense", slot_cap=slot_cap, k1_form=0, k2_form=0), blk)
    for i, (fkey, (f, co)) in enumerate(zip(fkeys, frames)):
        want = torch.full((f.shape[0], 64), NAN, dtype=dt, device="cuda")
        plan.run(f, co, out=want)
        plan.check()
        differ = [int((outs[i] != want).any(1).sum()) for outs in calls]
        ref, o32 = _ref(fkey, 64, 2, op, pos, r, 1.0, dt)
        label = dict(group="e", frame="/".join(str(v) for v in fkey), C=64, groups=2, op=op, pos=pos, r=r, div=1.0, rows=dtn,
                     batch_of=len(fkeys), rows_differing_from_plan=differ)
        _gate(label, fkey, 64, 2, op, pos, ref, o32, calls[0][i], dt, absolute)
        assert differ == [0, 0], (fkey, "batch rows differ from the per-frame plan", differ)


@pytest.mark.parametrize("op", ["cos", "sin"])
@pytest.mark.parametrize("r", [2, 3])
def test_batch_ragged_call_on_the_common_grid(r, op):
    """full (cells of 343, the 352 / 353 sums), one voxel, two voxels, the corners and the slab in ONE call: 1 .. 1 431 voxels per
    frame, batch item 1 empty in four of the five."""
    _batch_case([(n, 1) for n in ("full", "one", "pair", "corners", "slab")], DF.COMMON_BOUNDS, op, r)


@pytest.mark.parametrize("name", ["solid3", "solid2", "deep_strips13", "deep_strips5"])
@pytest.mark.parametrize("op,r", [("cos", 3), ("sin", 2), ("sin", 3)])
def test_batch_calls_of_three(op, r, name):
    _batch_case([(name, sd) for sd in (1, 2, 3)], DF.frame(name)[1], op, r)


@pytest.mark.parametrize("name,pos,absolute", [f[:3] for f in FAR], ids=["far", "far_x20", "exact_far"])
@pytest.mark.parametrize("op", ["cos", "sin"])
def test_batch_large_theta(op, name, pos, absolute):
    """Two frames of a kind per call.  (exact_far and far cannot share a call: one grid over both boxes would have 4.7e10 cells, and
    a call has one set of parameters.)"""
    _batch_case([(name, 1), (name, 2)], DF.frame(name)[1], op, 3, pos=pos, absolute=absolute)


@pytest.mark.parametrize("op,r", [("cos", 3), ("sin", 2)])
def test_batch_slot_cap_352(op, r):
    """s = 8 with slot_cap = 352: a cell of exactly 352 voxels next to cells of 0 .. 89."""
    _batch_case([("s8_352", 1), ("s8", 1), ("s8_352", 2)], DF.frame("s8")[1], op, r, slot_cap=DF.LCAP)


def test_batch_fp16_on_the_common_grid():
    _batch_case([(n, 1) for n in ("full", "one", "slab")], DF.COMMON_BOUNDS, "cos", 3, dtn="fp16")


def test_batch_refuses_coord_div():
    import ctypes
    import link_amd as la
    from link_amd import _lib as L
    with pytest.raises(L.LinkAmdError):
        la.ElkCoreBatch(2, 64, 64, "cos", 32, 3, 7, DF.COMMON_BOUNDS, "cuda", coord_div=2.0)
    # ... and the C entry point refuses a descriptor that carries one, launching nothing
    fkeys = [("one", 1), ("pair", 1)]
    frames = [_frame(k, 64, torch.float32) for k in fkeys]
    batch = _bind(la.ElkCoreBatch(2, 2, 64, "cos", 32, 3, 7, DF.COMMON_BOUNDS, "cuda"), _block(64, 2, "cos"))
    k, _ = batch._fill([f for f, _ in frames], [co for _, co in frames], None)
    p0 = batch.plans[0]
    desc = L.LinkElkDesc(p0.desc.op, 64, 32, 3, 2.0, 1e-6)
    rc = batch._fn(batch._ctx, batch._bufs, batch._n, k, ctypes.byref(p0.dcg), ctypes.byref(desc), L.current_stream_handle())
    assert rc == L.LINK_ERR_ARG
    torch.cuda.synchronize()
    batch.check()
