"""The three forms of R_core on the general layout -- the tile form (link_elk_premix_modsum_tiles + link_elk_gather_demod_tiles,
csrc/elk_tiles_impl.h), the lean form (link_elk_core_lean_forward, csrc/elk_lean_impl.h) and the four-kernel form (csrc/elk.hip) --
behind a per-case float64 gate over a stated lattice of kernels, block sizes and coordinates: the branches that LiDAR-like and
uniform frames at non-negative coordinates in batch item 0 never reach, or reach only kernel against kernel.

  a. the kernel-selection lattice (tests/core_frames.py, LATTICE) on the lattice frame with cells on both sides of zero: every width,
     every groups value with a distinct NB (8 and 16 included: every 16-channel block evaluates its own theta through % cg), cos / sin
     / cos_x, r 2 / 3, both block orders, coord_div 1 / 2, empty neighbours inside the grid and outside it, the lean form's channel
     split and the form without the scratch matrix, half rows, the four-kernel form at widths 20 .. 256, c % 4 != 0, r = 1 and under
     the flag sets of tests/test_gpu_split_paths.py;
  b. tile-form ranges and runs: one block of 15 .. 4 096 voxels, runs ending exactly at 16 / 32 / 64 / 128 / 256 and one past, blocks
     through whole waves and workgroups, tiles of one-voxel blocks (several gather passes at every width), capacity above n;
  c. lean-form edges: cells of exactly 31 / 32 / 33 / 64 / 65 / 343 / 352 voxels, the channel-split edge n = 4 096 / 4 097, the
     item-workgroup cap past n = 16 384, the three counter packings, a big frame after a small one and back;
  d. the tile form's span edge n = 32 768 / 32 800;
  e. large theta (fast path at ~2 000 rad; the slow sincos with theta exact in fp32 -- tight -- and with the weights times 20) and
     feature rows beyond the fp16 split's range;
  f. batch items, the bounds' corners, voxels outside the bounds, n = 0.

Every case: parameters of a seeded ELKBlock (core_frames.block_of), a caller's result buffer pre-filled with NaN, run cold, cold
again and warm (build_index=False), each into fresh NaN.  The first run goes through gate_rows of tests/ref64.py (gate_zero_rows for
the one-voxel frame under `sin`) against Ref64 on the device -- finite; rel64 < 1e-4 (fp32) / 4e-3 (fp16) / 3e-2 (bf16); rel64 <=
4 o32 + 2 o_round + 2e-6; nothing in a bound comes from a kernel -- and its figures, with the restated route, go to
core_parity.jsonl in the directory LINK_AMD_PARITY_DIR names BEFORE any verdict (profiles/core_parity.jsonl is one run).  Then: the
status word clean, blocks() the CPU's block count, the plan's blk_start the CPU's numbering (general layout), the second cold and the
warm run bit-equal to the first, the self-cleaning counters back at zero.  absolute=False drops the fixed bound only where
tests/test_cpu_core_frames.py shows the reference's own fp32 evaluation exceeds it: `far` under cos / sin, both at the initial weights
(o32 = 1.1e-4 .. 1.6e-4 at theta ~ 2 000 rad) and with the weights times 20 (2.4e-3: a LOOSE gate, there to catch a broken slow
path, as in tests/test_gpu_dense_lattice.py; `exact_far` under "exact_big" gates the same path tightly).

Found: nothing -- on an MI355X every case passes, the worst rel64 / (4 o32 + 2 o_round + 2e-6) over fp32 rows being 0.23 (tile form),
0.23 (lean) and 0.21 (four-kernel), and every second cold and warm run is bit-equal.  Four defects seeded one at a time fail exactly
the cases built for them: k_elk_tiles without its walk over `through` waves (b: every big_block of 63 voxels and up, edges16,
through -- no case of a), k_lean_gather ignoring coord_div (every lean case at coord_div = 2), and sin / cos swapped in the slow
branch of k_lean_sums_pm alone (e: the lean_pm cases of far x 20 and exact_big) or of k_lean_insert_premix alone (e: the lean_cs=False
and C = 32 cases of the same frames).  Merely SKIPPING a slow branch at theta ~ 1.3e5 fails
nothing, and should not: the fast reduction is still good to ~1e-6 there."""
import copy
import functools

import pytest
import torch

import core_frames as CF
from ref64 import Ref64, gate_rows, gate_zero_rows, record_row

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


ROW_DEFAULTS = dict(pos="init", div=1.0, rows="fp32", order="cell", clean=True)


def _record(row):
    """A row of core_parity.jsonl: figures to four significant digits; a field at its default (ROW_DEFAULTS) is left out."""
    row = {k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items() if ROW_DEFAULTS.get(k, ()) != v}
    record_row(row, "core_parity.jsonl")


# ------------------------------------------------------------------------------------------------------------------------------
# shared, unchanged once made: blocks, frames, references
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block(c, groups, op, pos="init"):
    return copy.deepcopy(CF.block_of(c, groups, op, pos)).cuda().eval()


def _bind(plan, blk):
    alpha = blk.alpha if blk.baseop == "cos_x" else None
    return plan.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, alpha,
                     blk.norm.weight, blk.norm.bias)


@functools.lru_cache(maxsize=None)
def _frame(fkey, c, dt):
    return CF.rows_for(fkey, c).to(dt).cuda(), CF.geometry(fkey)[0].cuda()


@functools.lru_cache(maxsize=None)
def _ref(fkey, c, groups, op, pos, r, div, dt):
    """(float64 reference, o32) of a frame under a parameter set: computed once on the device, shared, left unchanged.  The
    reference does not depend on the plan's bounds or block order."""
    f, co = _frame(fkey, c, dt)
    params = CF.params_of(_block(c, groups, op, pos))
    kw = dict(baseop=op, groups=groups, coord_div=div)
    s = CF.geometry(fkey)[2]
    ref = Ref64(f, co, params, s, r, **kw)
    r32 = Ref64(f, co, params, s, r, dtype=torch.float32, **kw)
    o32, ok = ref.rel(r32)
    assert ok
    return ref, (o32 if (fkey[0], op) not in CF.ANALYTIC_ZERO else r32)


@functools.lru_cache(maxsize=None)
def _numbering(fkey, bounds, order):
    co, _, s = CF.geometry(fkey)
    return CF.numbering(co, bounds, s, order)[1]


def _plan(form, fkey, c, groups, op, pos, r, div=1.0, order="cell", bounds=None, n_cap=None, slot_cap=0, flags=0, **kw):
    import link_amd as la
    co, own, s = CF.geometry(fkey)
    args = (n_cap or co.shape[0], c, op, c // groups, r, s, bounds or own, "cuda")
    if form == "lean":
        plan = la.ElkCorePlan(*args, coord_div=div, layout="lean", slot_cap=slot_cap, **kw)
        assert plan.lean
    else:
        plan = la.ElkCorePlan(*args, coord_div=div, layout="general", tiles=form == "tiles", block_order=order)
        assert not plan.dense and not plan.lean and bool(plan.tiles) == (form == "tiles") and plan.block_order == order
        plan.desc.flags |= flags
    return _bind(plan, _block(c, groups, op, pos))


def _counters(plan):
    """Sum of |.| over the self-cleaning counters a finished step must leave at zero."""
    if plan.lean:
        return int(plan.cnt2[plan._cur ^ 1].abs().sum())
    left = int(plan.cell_counts.abs().sum())
    return left + (int(plan.cell_pair.abs().sum()) if plan.cell_pair is not None else 0)


def _steps(plan, f, co):
    """Cold, cold again and warm, each into a fresh NaN buffer.  Nothing is judged here: (rows of the first run, [(rows differing,
    max |difference|)] of the other two, the status words, the counters left)."""
    outs, status, left = [], [], []
    for build in (True, True, False):
        out = torch.full((f.shape[0], f.shape[1]), NAN, dtype=f.dtype, device="cuda")
        got = plan.run(f, co, build_index=build, out=out)
        assert got.data_ptr() == out.data_ptr()
        from link_amd import _lib as L
        status.append(int(plan.hdr[L.HDR_STATUS]))
        left.append(_counters(plan))
        outs.append(out)
    differ = [(int((o != outs[0]).any(1).sum()), float((o.float() - outs[0].float()).nan_to_num(1e30).abs().max()) if o.numel() else 0.0)
              for o in outs[1:]]
    return outs[0], differ, status, left


def _case(form, fkey, c, groups, op, r, group, div=1.0, dtn="fp32", pos="init", order="cell", bounds=None, absolute=True, want=None,
          slow=False, plan=None, note=None, record=True, **kw):
    """One case: stepped, its figures written, then every verdict.  Returns the rows of the first run."""
    dt = DTYPES[dtn]
    order = "cell" if form == "lean" else order               # the lean layout has no block order: cells are its blocks
    co, own, s = CF.geometry(fkey)
    bounds = bounds or own
    f, cod = _frame(fkey, c, dt)
    ref, o32 = _ref(fkey, c, groups, op, pos, r, div, dt)
    sizes = _numbering(fkey, bounds, order)
    rkw = {k: v for k, v in kw.items() if k in ("lean_cs", "lean_pm", "flags")}
    dim = CF.grid_of(bounds, s)[1]
    got = CF.route(form, c, groups, op, r, co.shape[0], dim[0] * dim[1] * dim[2] * dim[3], k=kw.get("slot_cap") or s ** 3, slow=slow,
                   half=dt != torch.float32, blocks=int(sizes.shape[0]), coord_div=div, **rkw)
    assert "refused" not in got, got
    if want:
        assert {k: got.get(k) for k in want} == want, (want, got)
    if plan is None:
        plan = _plan(form, fkey, c, groups, op, pos, r, div, order, bounds, **kw)
    if form == "lean":
        assert plan.cnt_shift == got["cnt_shift"]
    out, differ, status, left = _steps(plan, f, cod)
    label = dict(group=group, form=form, frame="/".join(str(v) for v in fkey), C=c, groups=groups, op=op, pos=pos, r=r, div=div, rows=dtn,
                 order=order, route=CF.route_brief(got))
    if any(v is not None for v in kw.values()):               # lean_cs / lean_pm / flags / slot_cap / n_cap of the case
        label["kw"] = {k: v for k, v in kw.items() if v is not None}
    label["clean"] = (differ, status, left) == ([(0, 0.0)] * 2, [0] * 3, [0] * 3)      # repeats bit-equal, status and counters zero
    if not label["clean"]:
        label.update(rows_differing_cold2_warm=differ, status=status, counters_left=left)
    if note:
        label["note"] = note
    if (fkey[0], op) in CF.ANALYTIC_ZERO:
        scale = float(_block(c, groups, op, pos).norm.weight.detach().abs().max())
        gate_zero_rows(label, ref, o32, out, scale, record=_record if record else None)
    else:
        gate_rows(label, ref, o32, out, dt, absolute=absolute, record=_record if record else None)
    # ---- the figures are on file: the verdicts
    assert status == [0, 0, 0], ("status word", status)
    plan.check()
    assert plan.blocks() == int(sizes.shape[0])
    if form != "lean":                                     # the CPU's numbering IS the plan's: the frame is what its name says
        want_start = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
        assert torch.equal(plan.blk_start[:sizes.shape[0] + 1].cpu().long(), want_start), "blk_start differs from the restated numbering"
    assert differ[0] == (0, 0.0), ("second cold run differs: (rows, max|d|)", differ[0])
    assert differ[1] == (0, 0.0), ("warm run differs: (rows, max|d|)", differ[1])
    assert left == [0, 0, 0], ("self-cleaning counters not back at zero", left)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# a. the kernel-selection lattice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CF.LATTICE, ids=[CF.case_id(c) for c in CF.LATTICE])
def test_kernel_selection_lattice(case):
    want = dict(case["want"], div=case["div"] != 1.0)
    _case(case["form"], CF.case_frame(case), case["c"], case["groups"], case["op"], case["r"], "a", div=case["div"], dtn=case["rows"],
          order=case["order"], want=want, **case["kw"])


# ------------------------------------------------------------------------------------------------------------------------------
# b. tile-form range and run edges (and the four-kernel form on the same frames: big_block4096 = cooperative blocks)
# ------------------------------------------------------------------------------------------------------------------------------
EDGE_FRAMES, EDGE_OPS = CF.EDGE_FRAMES, CF.EDGE_OPS


@pytest.mark.parametrize("c", CF.EDGE_WIDTHS)
@pytest.mark.parametrize("name", EDGE_FRAMES)
def test_tile_ranges_and_runs(name, c):
    fkey = (name, 1)
    for groups, op, r in EDGE_OPS:
        _case("tiles", fkey, c, groups, op, r, "b", want=dict(wp=CF.gather_cfg(c)[0], rmax=CF.gather_cfg(c)[1]))
        coop = name != "singles"                            # mean voxels per block above 4 everywhere but on the one-voxel blocks
        _case("four", fkey, c, groups, op, r, "b", want=dict(coop=coop, modsum="group", gather="split"))


@pytest.mark.parametrize("c", CF.EDGE_WIDTHS)
@pytest.mark.parametrize("name", ["through", "singles"])
def test_tile_ranges_and_runs_fp16(name, c):
    for groups, op, r in EDGE_OPS:
        _case("tiles", (name, 1), c, groups, op, r, "b", dtn="fp16")


@pytest.mark.parametrize("name", ["through", "edges16"])
def test_tile_form_capacity_above_n(name):
    """m_cap > n: the table's scratch rows sit behind the capacity's rows, the all-zero row at m_cap."""
    n = CF.frame(name)[0].shape[0]
    _case("tiles", (name, 1), 64, 2, "cos", 3, "b", n_cap=3 * n + 11, note="n_cap = 3 n + 11")


# ------------------------------------------------------------------------------------------------------------------------------
# c. lean-form edges
# ------------------------------------------------------------------------------------------------------------------------------
LEAN_FORMS = [dict(), dict(lean_cs=True), dict(lean_cs=False), dict(lean_pm=True)]


@pytest.mark.parametrize("name,slot_cap", [("chunks", 0), ("s8_352", 352)])
@pytest.mark.parametrize("c,groups,op,r", CF.CHUNK_SHAPES)
def test_lean_chunks(c, groups, op, r, name, slot_cap):
    """Cells of exactly 31 / 32 / 33 / 64 / 65 / 343 voxels at slot capacity 343 (kch = 11), one of 352 at slot capacity 352."""
    for kw in LEAN_FORMS:
        if ("lean_cs" in kw and c < 64) or ("lean_pm" in kw and c > 64):
            continue
        want = dict(kch=11, pm=bool(kw.get("lean_pm")))
        _case("lean", (name, 1), c, groups, op, r, "c", want=want, slot_cap=slot_cap, **kw)


@pytest.mark.parametrize("n,cs", [(4096, True), (4097, False)])
def test_lean_channel_split_edge(n, cs):
    for groups, op, r in CF.CS_EDGE_SHAPES:
        _case("lean", ("n%d" % n, 1), 64, groups, op, r, "c", want=dict(cs=cs, pm=False, vpw=16 if cs else 64))


@pytest.mark.parametrize("n,capped", [(16384, False), (16400, True)])
@pytest.mark.parametrize("c", [16, 32])
def test_lean_item_workgroup_cap(c, n, capped):
    (g0, op0, r0), (g1, op1, r1) = CF.CS_EDGE_SHAPES
    _case("lean", ("n%d" % n, 1), c, g0, op0, r0, "c", want=dict(capped=capped, item_wgs=4096))
    _case("lean", ("n%d" % n, 1), c, g1, op1, r1, "c", want=dict(capped=capped, item_wgs=4096), lean_pm=True)


@pytest.mark.parametrize("c,groups,op,r", CF.PACKING_SHAPES)
def test_lean_counter_packing(c, groups, op, r):
    """The lattice frame under three bounds -- below 32 768 cells, below 262 144 and above: a counter per 128 bytes, per 32 bytes,
    packed.  The same reference for all three."""
    fkey = ("lat", 3, r)
    own = CF.geometry(fkey)[1]
    for extra, shift in ((0, 5), (31, 3), (61, 0)):
        lo = tuple(v - 3 * (extra // 2) for v in own[0][:3]) + (0,)
        hi = tuple(v + 3 * (extra - extra // 2) for v in own[1][:3]) + (0,)
        _case("lean", fkey, c, groups, op, r, "c", bounds=(lo, hi), want=dict(cnt_shift=shift), note="%d more cells per axis" % extra)


@pytest.mark.parametrize("kw", LEAN_FORMS, ids=["default", "cs", "no_cs", "pm"])
def test_lean_big_after_small_after_big(kw):
    """`chunks` (1 110 voxels, cells of 343) and `one` alternate through ONE plan: the counters and item lists of the frame before
    are gone, whichever was the bigger."""
    bounds = CF.frame("one")[1]
    plan = _plan("lean", ("chunks", 1), 64, 2, "cos", "init", 3, bounds=bounds, **kw)
    for i, name in enumerate(("chunks", "one", "chunks", "one", "one", "chunks")):      # every visit gated, the first of each on file
        _case("lean", (name, 1), 64, 2, "cos", 3, "c", bounds=bounds, plan=plan, note="alternating", record=i < 2, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# d. the tile form's span edge
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,span", [(32768, 64), (32800, 128)])
@pytest.mark.parametrize("c,groups,op,r", CF.SPAN_SHAPES)
def test_tile_span_edge(c, groups, op, r, n, span):
    _case("tiles", ("n%d" % n, 1), c, groups, op, r, "d", want=dict(span=span, wgs=(n + span - 1) // span))


# ------------------------------------------------------------------------------------------------------------------------------
# e. large theta and big rows
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pos,drop,slow", CF.LARGE_THETA, ids=["%s-%s" % f[:2] for f in CF.LARGE_THETA])
@pytest.mark.parametrize("c,groups,op,r", CF.LARGE_SHAPES)
@pytest.mark.parametrize("form", CF.FORMS)
def test_large_theta_and_big_rows(form, c, groups, op, r, name, pos, drop, slow):
    absolute = op not in drop                               # dropped where fp32 evaluation of the formula itself exceeds 1e-4
    forms = CF.large_lean_forms(c) if form == "lean" else [(dict(), None)]       # each copy of the lean kernels' `big` vote
    for kw, want in forms:
        _case(form, (name, 1), c, groups, op, r, "e", pos=pos, absolute=absolute, slow=slow is not False, want=want, **kw)


@pytest.mark.parametrize("pos", ["exact", "exact_big"])
@pytest.mark.parametrize("form", ["tiles", "lean"])
def test_exact_far_fp16(form, pos):
    for c, groups, op, r in CF.LARGE_SHAPES:
        for kw, want in (CF.large_lean_forms(c) if form == "lean" else [(dict(), None)]):
            _case(form, ("exact_far", 1), c, groups, op, r, "e", dtn="fp16", pos=pos, slow=pos == "exact_big", want=want, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# f. coordinates and status
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CF.COORD_FRAMES)
@pytest.mark.parametrize("form", CF.FORMS)
def test_batch_items_corners_and_lone_voxels(form, name):
    """`slab`: a second batch item holding one voxel; `corners`: the exact lo and hi of the bounds, every neighbour of a corner block
    outside the grid; `one` under sin: analytically zero (gate_zero_rows)."""
    for c, groups, op, r, order, div in CF.coord_shapes(name):
        _case(form, (name, 1), c, groups, op, r, "f", order=order, div=div)


@pytest.mark.parametrize("form", CF.FORMS)
def test_voxels_outside_the_bounds(form):
    """Three voxels outside the plan's bounds (beyond x, below y, a batch item too many).  The kept rows are the rows of the frame
    WITHOUT those voxels, check() and blocks() raise, and the dropped voxels' rows are pinned as the code serves them today:
    UNTOUCHED -- still the NaN the caller's buffer held -- on all three forms.  The index drops such a voxel before any kernel sees
    it (k_cell_count / k_cell_count_first of csrc/index.hip: not counted, not in vox_sorted; the lean inserts: `keep` is false, the
    voxel enters no list), and every later kernel writes the rows of indexed voxels alone.  (The module path's promise of zeros is
    kept by ITS output buffer, which starts as zeros: _alloc_out of link_amd/elk.py.)  The next clean frame through the same plan is
    right."""
    from link_amd import _lib as L
    c, groups, op, r = 64, 2, "cos", 3
    co, bounds, s = CF.frame("outside")
    n = co.shape[0]
    gone = list(CF.OUTSIDE_IDS(n))
    keep = torch.ones(n, dtype=torch.bool)
    keep[gone] = False
    assert bool((CF.cell_keys(co, bounds, s) < 0).eq(~keep).all())
    f, cod = _frame(("outside", 1), c, torch.float32)
    params = CF.params_of(_block(c, groups, op))
    keep_d = keep.cuda()
    ref = Ref64(f[keep_d], cod[keep_d], params, s, r, baseop=op, groups=groups)
    o32, ok = ref.rel(Ref64(f[keep_d], cod[keep_d], params, s, r, baseop=op, groups=groups, dtype=torch.float32))
    assert ok
    plan = _plan(form, ("outside", 1), c, groups, op, "init", r)
    out = torch.full((n, c), NAN, device="cuda")
    plan.run(f, cod, out=out)
    gate_rows(dict(group="f", form=form, frame="outside/1", note="kept rows"), ref, o32, out[keep_d], record=_record)
    with pytest.raises(L.LinkAmdError):
        plan.check()
    with pytest.raises(L.LinkAmdError):
        plan.blocks()
    assert bool(torch.isnan(out[~keep_d]).all()), "rows of dropped voxels: expected untouched NaN"
    _case(form, ("lat", 7, 3), c, groups, op, r, "f", plan=plan, note="after a frame with voxels outside")


@pytest.mark.parametrize("form", CF.FORMS)
def test_an_empty_frame_then_a_full_one(form):
    c, groups, op, r = 64, 2, "cos", 3
    fkey = ("lat", 7, 3)
    plan = _plan(form, fkey, c, groups, op, "init", r)
    f, cod = _frame(fkey, c, torch.float32)
    for build in (True, False):
        none = plan.run(f[:0], cod[:0], build_index=build)
        torch.cuda.synchronize()
        assert tuple(none.shape) == (0, c)
        plan.check()
    _case(form, fkey, c, groups, op, r, "f", plan=plan, note="after n = 0")
    plan.run(f[:0], cod[:0])
    torch.cuda.synchronize()
    plan.check()
    assert _counters(plan) == 0
    _case(form, fkey, c, groups, op, r, "f", plan=plan, note="after n = 0 behind a full frame")
