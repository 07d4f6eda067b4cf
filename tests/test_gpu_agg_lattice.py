"""The float64 gate over the oldest layer of the library, the drop-in surface the segmentation networks enter and leave through:
csrc/ops.hip (voxelize, devoxelize, link_ti_weights), csrc/aggregate.hip (k_block_mean<1|2|4>, k_nbr_reduce, k_row_gather64,
k_seg_sum, k_nbr_reduce_t), the aggregation entries of csrc/elk.hip (k_means_to_table, k_row_gather4, k_block_gather_g with its
scatter epilogue) and the Python on top (aggregate.py, pointvoxel.py, functional.py, backend.py).

The gate is the project's (tests/test_gpu_dcn.py, tests/test_gpu_roihead.py): for every float tensor
    max|got - ref64| <= 4 e_ref + one fp32 ulp of max|ref64|   (+ half an ulp of the format for a 16-bit result),
ref64 the float64 restatement of tests/agg64.py, e_ref the distance of the float32 restatement (the same code) from it on the same
inputs -- measured here, never taken from a kernel.  The factor 4 covers another summation order (atomics, column sums, x (1/d)
against x / d).  Every case calls the public surface under a spy on the library's entry points and asserts the entry that
agg_frames.route_* predicts, so a torch composition cannot stand in for a kernel (link_aux_to_voxel_forward_grid, which has no
caller, is called through _lib with NaN-filled buffers); the kernel instance behind the entry (VEC, parts, LPR, dense-grid or
column-walking form -- for the grid the index was actually built on -- and K passes) is what route_* PREDICTS from the dispatch
code, not something read back from the device, and is recorded with the figures as such.  Further, in every case: results finite
(the allocator's free blocks are NaN-filled before each call); integer outputs equal to the CPU numbering (block coordinates,
idx_query, counts, the neighbour tables of index.neighbor_map -- transposed at even r -- and foreign_neighbor_map, the corner table of
voxel_to_point); the indexed kernels (block mean, both aux_to_voxel directions, devoxelize forward, voxelize backward) bit-equal on a second
run; k_block_mean bit-equal to the sequential fp32 restatement at every VEC (segments of at most 8192 ids); a constant field constant
to 2 ulps through aux_to_voxel on every route (scatter, table, grid and foreign; the foreign route's backward is devoxelize backward,
which adds with atomics: its forward is the part held to bit equality).  Each case appends one row to agg_parity.jsonl under LINK_AMD_PARITY_DIR -- the case,
its route and, per compared tensor, [e_dev, e_ref, bound] to three digits -- before a failing verdict or when the case's last
comparison is in (profiles/agg_parity.jsonl is one MI355X run).

Groups: a voxel_to_aux; b aux_to_voxel (scatter, table, grid, foreign) with f, the speculated grid, run inside b's cases on `dense`
and `sparse`, the two ctypes cases of the grid entry included (index built with _SPEC_GRID cleared / after a frame of the same extents / after a larger frame whose grid is accepted:
all gated, integers equal, features bit-equal where route says the same form ran on the same grid); c spvoxelize / spdevoxelize and
the backend functions under fp16 / bf16 / fp64; d calc_ti_weights; e initial_voxelize -> point_to_voxel -> voxel_to_point on cells
of up to 8193 points, native and forced hash path.

The committed run (profiles/agg_parity.jsonl, 467 cases, 1385 comparisons): worst e_dev / bound per group -- a 0.25 (members8, w 256,
offset rows: e_dev = e_ref, the kernel is the sequential sum), b scatter 0.48, b table 0.45, b grid 0.20, b foreign 0.24, c ops 0.34
(devoxelize backward, atomics), c backend 0.66 (the fp16 and the bf16 voxelize forward alike: half an ulp of the format, as the bound
allows), d 0.22, e 0.35 (the hash path's means of the 8192- and 8193-point cells with offset rows, summed by atomics).  The atomic
kernels' figures move from run to run (c ops 0.29 to 0.41 and e 0.27 to 0.35 over four runs).  No case needs a factor above 4.

That the gate bites: four defects seeded one at a time in scratch builds (values only, never committed), the whole file run on each
(before the grid and foreign tests gained their second, constant-field and speculated-grid runs: those add checks, and remove none).
  k_block_mean adding only the first 64-id chunk: a[members7], a[members8] (not a[dense], a[corner]: blocks of at most 8), e[native],
    and what consumes those means: b scatter[members7-*], b table[4], b table[5] (their members7 case) -- every case with a block of
    more than 64 members, no other;
  k_nbr_reduce stopping after the first K pass: b table[5] (K = 125) alone;
  k_means_to_table not multiplying by the count: every b scatter case and both b grid cases; the table and foreign routes pass;
  the three-part scatter writing part 2's values into part 1: every b scatter test, at its first three-part width (12) after all
    two-part widths passed (84 two-part comparisons inside their bounds); grid, table and foreign pass.

Found: (1) k_voxelize_bwd read counts[idx] with no upper guard while the forward (and the reference, voxelize_cuda.cu:22,38) skip
idx >= len(counts); no caller inside the library can produce such an idx (every idx comes from a look-up into the set counts was
taken over), but spvoxelize / backend.voxelize_backward_cuda are public drop-ins that accept one, so they now go through
link_voxelize_backward_n1, which gives those rows zeros (checked here with in-range data only).  (2) "the same bits every run" of
initial_voxelize's means holds for cells of at most 8192 points (k_sort_seg's SORT_MAX_SEG); pointvoxel.py and INTEGRATION.md now say
so.  (3) Of the widths the scatter route takes in three parts (w % 12 == 0 and w % 8 != 0) the largest is 492: 504 is a multiple of 8
and takes two.  No wrong value, and no route the surface claims but does not take, was found."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import agg64 as A
import agg_frames as AF
from helpers import spied
from ref64 import record_row

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
HALF_ULP = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
AUX_FWD = ("link_aux_to_voxel_forward", "link_aux_to_voxel_forward_scatter", "link_aux_to_voxel_forward_grid")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_SHORT = {"route": "", "form": "", "parts": "p", "lpr": "l", "grid": "g", "k_passes": "k", "bwd_k_passes": "bk", "bwd_transposed": "bt",
          "vec4_gather": "v4", "vec": "vec", "j0_passes": "j", "tail": "tail", "scaled": "scaled", "native": "native"}


def _route_str(route):
    """'scatter p3 l4 column g5x7x9x2 bk1 bt0': the predicted kernel instance in one short field (the entry is implied by the route)"""
    words = []
    for k, v in route.items():
        if k == "entry":
            continue
        if isinstance(v, (list, tuple)):
            v = "x".join(str(d) for d in v)
        elif isinstance(v, bool):
            v = int(v)
        words.append(_SHORT.get(k, k) + str(v))
    return " ".join(words)


_PEND = []                      # the open row: one per case, its comparisons under "cmp" as component -> [e_dev, e_ref, bound]


def _flush():
    while _PEND:
        record_row(_PEND.pop(), name="agg_parity.jsonl")


@pytest.fixture(autouse=True)
def _rows_out():
    yield
    _flush()


def gate(test, case, route, name, got, want64, e_ref, out_dtype=torch.float32):
    got, want64 = got.detach().double().cpu().numpy(), torch.as_tensor(want64).detach().double().numpy()
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    big = float(np.abs(want64).max(initial=0.0))
    bound = 4 * float(e_ref) + float(np.spacing(np.float32(big))) + HALF_ULP[out_dtype] * big
    finite = bool(np.isfinite(got).all())
    d = float(np.abs(got - want64).max(initial=0.0)) if finite else float("inf")
    print(test, case, route, name, "e_dev", d, "e_ref", float(e_ref), "bound", bound)
    head = {"test": test, **case, "route": _route_str(route)}
    if not _PEND or {k: v for k, v in _PEND[0].items() if k != "cmp"} != head:
        _flush()
        _PEND.append(dict(head, cmp={}))
    _PEND[0]["cmp"][name] = [float("%.3g" % v) for v in (d, float(e_ref), bound)]
    if not (finite and d <= bound):
        _flush()                                                                          # the figures are out before the verdict
    assert finite, (test, case, name)
    assert d <= bound, (test, case, route, name, d, bound)


def poison():
    """NaN into the allocator's free blocks: a result row that is never written cannot pass as finite"""
    for k in (10, 14, 18, 22):
        t = torch.full((1 << k,), float("nan"), device=DEV)
        del t


@contextlib.contextmanager
def spec_grid(mode, coords, s):
    """index._SPEC_GRID as the case wants it: 'clear'ed, after a frame of the 'same' extents, after a 'larger' frame whose grid the
    case's frame accepts (under twice its own cells); the module state is put back afterwards"""
    import link_amd.index as li
    saved = dict(li._SPEC_GRID)
    li._SPEC_GRID.clear()
    try:
        assert li.SPECULATE_GRID
        if mode == "same":
            li.BlockIndex(dev(coords[::-1].copy()), s)
        elif mode == "larger":
            far = coords[:1].copy()
            far[0, 0] = coords[:, 0].max() + 2 * s                                        # two more blocks along x
            li.BlockIndex(dev(np.concatenate([coords, far], 0)), s)
        else:
            assert mode == "clear"
        yield
    finally:
        li._SPEC_GRID.clear()
        li._SPEC_GRID.update(saved)


def check_index(small, idx, counts, small_c, inv, cnt):
    assert idx.dtype == torch.int64 and counts.dtype == torch.int32 and small.C.dtype == torch.int32
    assert np.array_equal(small.C.cpu().numpy(), small_c.numpy())
    assert np.array_equal(idx.cpu().numpy(), inv.numpy())
    assert np.array_equal(counts.cpu().numpy(), cnt.numpy())


def check_neighbor_maps(index, small_c, nbr, r):
    """the index's neighbour table, and at even r the transposed one the backward reads, against the CPU numbering"""
    got = index.neighbor_map(r)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), nbr.numpy()), r
    if r % 2 == 0:
        got_t = index.neighbor_map(r, transpose=True)
        assert np.array_equal(got_t.cpu().numpy(), A.neighbor_table(small_c, r, transpose=True).numpy()), r


# ----------------------------------------------------------------------------------------------------------- a. voxel_to_aux
def _voxel_to_aux(x, go, coords, s):
    import link_amd as la
    xd = dev(x).requires_grad_(True)
    large = la.SparseTensor(xd, dev(coords), 1)
    poison()
    with spied() as calls:
        small, idx, counts = la.voxel_to_aux(large, s)
        (gx,) = torch.autograd.grad(small.F, xd, dev(go))
    return small, idx, counts, gx, calls


@pytest.mark.parametrize("name,widths", AF.CASES_A, ids=[c[0] for c in AF.CASES_A])
def test_a_voxel_to_aux(name, widths):
    coords, s, _ = AF.frame(name)
    n = coords.shape[0]
    small_c, inv, cnt = A.block_index(coords, s)
    for k, w in enumerate(widths):
        for family in (AF.FAMILIES[k % 3], "offset") if AF.FAMILIES[k % 3] != "offset" else ("offset",):
            route = AF.route_block_mean(w)
            case = {"frame": name, "w": w, "family": family}
            x, go = AF.rows(family, n, w, w), AF.rows("normal", small_c.shape[0], w, w + 1)
            with spec_grid("clear", coords, s):
                small, idx, counts, gx, calls = _voxel_to_aux(x, go, coords, s)
                small2, _, _, gx2, _ = _voxel_to_aux(x, go, coords, s)
            assert "link_block_mean" in calls and "link_voxelize_backward" in calls and "link_voxelize_forward" not in calls
            check_index(small, idx, counts, small_c, inv, cnt)
            m64, m32 = A.block_mean(x, inv, cnt, F64), A.block_mean(x, inv, cnt, F32)
            gate("a", case, route, "small_f", small.F, m64, A.dist(m32, m64))
            g64, g32 = A.voxelize_bwd(go, inv, cnt, n, F64), A.voxelize_bwd(go, inv, cnt, n, F32)
            gate("a", case, route, "grad_x", gx, g64, A.dist(g32, g64))
            assert torch.equal(small.F, small2.F) and torch.equal(gx, gx2)                # the same bits on a second run
            assert int(cnt.max()) <= AF.SORT_MAX_SEG                                      # ids ascending inside every block:
            assert np.array_equal(small.F.detach().cpu().numpy(), A.block_mean_seq32(x, inv.numpy(), cnt.numpy())), (case, route)


# ----------------------------------------------------------------------------------------- b. aux_to_voxel, f. speculated grid
def _aux_reference(x, go, coords, s, r):
    res = {}
    for dt in (F64, F32):
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        out, small_f, index = A.aggregate(xt, coords, s, r, dt)
        g_small, g_x = torch.autograd.grad(out, [small_f, xt], torch.from_numpy(go).to(dt))
        res[dt] = {"out": out.detach(), "grad_small": g_small, "grad_x": g_x}
    return res, index


def _aux_native(x, go, coords, s, r, mode, const=None):
    """(out, grad_small, grad_x, route, index grid) of voxel_to_aux + aux_to_voxel on the public surface; const: the block features
    are replaced by that constant before aux_to_voxel, forward only"""
    import link_amd as la
    xd = dev(x).requires_grad_(True)
    large = la.SparseTensor(xd, dev(coords), 1)
    with spec_grid(mode, coords, s):
        small, idx, counts = la.voxel_to_aux(large, s)
        index = small._link_index
        dims = tuple(int(d) for d in index.grid.dim)
        route = AF.route_aux(x.shape[1], r, index.M, dims)
        if const is not None:
            small.F = torch.full_like(small.F, const)
        poison()
        with spied() as calls:
            out = (la.aux_to_voxel(small, large, idx, counts, r) if r != 3 else la.small_to_large_v2(small, large, idx, counts)).F
            g_small, g_x = torch.autograd.grad(out, [small.F, xd], dev(go)) if const is None else (None, None)
    assert [c for c in calls if c in AUX_FWD] == [route["entry"]], (calls, route)         # the entry route() predicts, once
    assert ("link_aux_to_voxel_backward" in calls) == (const is None) and "link_devoxelize_forward" not in calls
    return (small, idx, counts), {"out": out.detach(), "grad_small": g_small, "grad_x": g_x}, route, dims


def _aux_case(test, name, w, r, k):
    coords, s, _ = AF.frame(name)
    n = coords.shape[0]
    family = AF.FAMILIES[k % 3]
    x, go = AF.rows(family, n, w, w + r), AF.rows("normal", n, w, w + r + 1)
    ref, (small_c, inv, cnt, nbr) = _aux_reference(x, go, coords, s, r)
    runs = {}
    for mode in (("clear", "same", "larger") if name in ("dense", "sparse") else ("clear",)):
        case = {"frame": name, "w": w, "r": r, "family": family, "spec": mode}
        (small, idx, counts), got, route, dims = _aux_native(x, go, coords, s, r, mode)
        route = dict(route, grid=list(dims), **{"bwd_" + a: b for a, b in AF.route_aux_backward(r).items() if a != "entry"})
        check_index(small, idx, counts, small_c, inv, cnt)
        check_neighbor_maps(small._link_index, small_c, nbr, r)
        for comp in ("out", "grad_small", "grad_x"):
            gate(test, case, route, comp, got[comp], ref[F64][comp], A.dist(ref[F32][comp], ref[F64][comp]))
        runs[mode] = (got, route, dims)
    # bits: a second run on the same grid (the previous frame had the same extents), and any run the same form took on the same grid
    tight = AF.block_grid(AF.frame(name)[2])[1]
    assert runs["clear"][2] == tight
    if "same" in runs:
        assert runs["same"][2] == tight and runs["larger"][2] != tight                     # the speculated grids were accepted
        for comp in ("out", "grad_small", "grad_x"):
            assert torch.equal(runs["clear"][0][comp], runs["same"][0][comp]), (name, w, r, comp)
    else:
        _, again, _, _ = _aux_native(x, go, coords, s, r, "clear")
        for comp in ("out", "grad_small", "grad_x"):
            assert torch.equal(runs["clear"][0][comp], again[comp]), (name, w, r, comp)
    # a constant field of block features is a fixed point of the box mean (count-weighted sums of 2.5 are exact in fp32)
    _, cgot, _, _ = _aux_native(x, go, coords, s, r, "clear", const=AF.CONST)
    assert float((cgot["out"] - AF.CONST).abs().max()) <= 2 * float(np.spacing(np.float32(AF.CONST))), (name, w, r)
    return runs["clear"][1]


@pytest.mark.parametrize("r", AF.SCATTER_R)
@pytest.mark.parametrize("name", AF.SCATTER_FRAMES)
def test_b_scatter_route(name, r):
    seen = set()
    for k, w in enumerate(AF.WIDTHS_P2 + AF.WIDTHS_P3 + AF.WIDTHS_P2X):
        route = _aux_case("b_scatter", name, w, r, k + r)
        assert route["route"] == "scatter" and route["parts"] == (3 if w in AF.WIDTHS_P3 else 2)
        seen.add((route["parts"], route["lpr"], route["form"]))
    assert {p for p, _, _ in seen} == {2, 3} and {l for _, l, _ in seen} == {4, 8, 16, 32, 64}
    assert ("dense" in {f for _, _, f in seen}) == (r == 3 and name != "sparse")


@pytest.mark.parametrize("r", AF.TABLE_R)
def test_b_table_route(r):
    for k, w in enumerate(AF.WIDTHS_TABLE):
        route = _aux_case("b_table", AF.TABLE_FRAMES[r], w, r, k + r)
        assert route["route"] == "table" and route["k_passes"] == (2 if r == 5 else 1) and route["bwd_transposed"] == (r % 2 == 0)
    if r >= 4:                                                                             # any width goes to the table beyond r = 3
        assert _aux_case("b_table", "members7", 24, r, r)["route"] == "table"


@pytest.mark.parametrize("name,w,r", AF.GRID_CASES, ids=["%s-w%d-r%d" % c for c in AF.GRID_CASES])
def test_b_grid_route_through_ctypes(name, w, r):
    """link_aux_to_voxel_forward_grid: exported, bound in _lib.py, no caller -- the table of neighbour means, the denominators and
    the gathered rows, into NaN-filled buffers"""
    import link_amd as la
    from link_amd import _lib as L
    coords, s, _ = AF.frame(name)
    n = coords.shape[0]
    x = AF.rows("normal", n, w, w)
    small_c, inv, cnt = A.block_index(coords, s)
    nbr = A.neighbor_table(small_c, r)
    den = torch.where(nbr >= 0, cnt[nbr.clamp(min=0)], torch.zeros_like(nbr)).sum(1)
    two_ulps = 2 * float(np.spacing(np.float32(AF.CONST)))
    grids, first = {}, None
    for mode in ("clear", "same", "larger"):
        with spec_grid(mode, coords, s):
            small, idx, counts = la.voxel_to_aux(la.SparseTensor(dev(x), dev(coords), 1), s)
        index, m = small._link_index, small.C.shape[0]
        check_index(small, idx, counts, small_c, inv, cnt)
        grids[mode] = tuple(int(d) for d in index.grid.dim)
        route = dict(AF.route_aux(w, r, m, grids[mode], entry="grid"), grid=list(grids[mode]))

        def call(small_f):
            nan = float("nan")
            S = torch.full(((m + 1) * (w + 1),), nan, device=DEV)
            new_feat, denom, out = torch.full((m, w), nan, device=DEV), torch.full((m,), nan, device=DEV), torch.full((n, w), nan, device=DEV)
            L.check(L.lib().link_aux_to_voxel_forward_grid(small_f.data_ptr(), counts.data_ptr(), index.blk_coords.data_ptr(),
                                                           index.cell_blk.data_ptr(), ctypes.byref(index.grid), index.hdr.data_ptr(),
                                                           idx.data_ptr(), n, m, w, r, S.data_ptr(), new_feat.data_ptr(),
                                                           denom.data_ptr(), out.data_ptr(), L.current_stream_handle()),
                    "link_aux_to_voxel_forward_grid")
            return S, new_feat, denom, out
        small_f = small.F.contiguous()
        S, new_feat, denom, out = call(small_f)
        case = {"frame": name, "w": w, "r": r, "family": "normal", "spec": mode}
        sf = small_f.cpu()                                                                 # the case is these block means
        b64, b32 = A.box_mean(sf, cnt, nbr, F64), A.box_mean(sf, cnt, nbr, F32)
        gate("b_grid", case, route, "new_feat", new_feat, b64, A.dist(b32, b64))
        gate("b_grid", case, route, "out", out, b64[inv], A.dist(b32, b64))
        assert np.array_equal(denom.cpu().numpy(), den.float().numpy())                    # sums of small integers: exact
        cS = S.cpu()
        assert np.array_equal(cS[m * w:(m + 1) * w].numpy(), np.zeros(w, np.float32))      # the zero row, and the count column
        assert np.array_equal(cS[(m + 1) * w:].numpy(), np.concatenate([cnt.float().numpy(), [0.0]]).astype(np.float32))
        again = call(small_f)                                                              # the same bits on a second run
        assert torch.equal(new_feat, again[1]) and torch.equal(out, again[3]) and torch.equal(denom, again[2])
        if mode == "clear":
            first = (new_feat, out)
        elif mode == "same":                                                               # the same form on the same grid
            assert torch.equal(new_feat, first[0]) and torch.equal(out, first[1])
        _, c_new, _, c_out = call(torch.full_like(small_f, AF.CONST))                      # a constant field stays constant
        assert float((c_new - AF.CONST).abs().max()) <= two_ulps and float((c_out - AF.CONST).abs().max()) <= two_ulps, (name, mode)
    tight = AF.block_grid(AF.frame(name)[2])[1]
    assert grids["clear"] == tight == grids["same"] and grids["larger"] != tight           # the speculated grids were accepted


@pytest.mark.parametrize("r", [2, 3])
def test_b_foreign_inputs(r):
    """aux_to_voxel with a small_x that did not come from voxel_to_aux: the reference algorithm on the op kernels"""
    import link_amd as la
    from link_amd.index import foreign_neighbor_map
    coords, s, _ = AF.frame("corner")
    n, w = coords.shape[0], 8
    small_c, inv, cnt = A.block_index(coords, s)
    nbr = A.neighbor_table(small_c, r)
    sf, go = AF.rows("offset", small_c.shape[0], w, r), AF.rows("normal", n, w, r + 1)
    route = AF.route_aux(w, r, small_c.shape[0], native=False)
    res = {}
    for dt in (F64, F32):
        t = torch.from_numpy(sf).to(dt).requires_grad_(True)
        out = A.aux_to_voxel(t, cnt, nbr, inv, dt)
        res[dt] = (out.detach(), torch.autograd.grad(out, t, torch.from_numpy(go).to(dt))[0])
    fd = dev(sf).requires_grad_(True)
    foreign = la.SparseTensor(fd, small_c.int().to(DEV), s)
    large = la.SparseTensor(torch.zeros(n, w, device=DEV), dev(coords), 1)
    poison()
    with spied() as calls:
        assert la.aux_to_voxel(foreign, large, inv.to(DEV), cnt.int().to(DEV), r) is large
        (g,) = torch.autograd.grad(large.F, fd, dev(go))
    assert "link_devoxelize_forward" in calls and "link_devoxelize_backward" in calls and not [c for c in calls if c in AUX_FWD]
    assert np.array_equal(foreign_neighbor_map(foreign.C, r).cpu().numpy(), nbr.numpy())   # the table this route looks up
    large2 = la.SparseTensor(torch.zeros(n, w, device=DEV), dev(coords), 1)               # the forward is indexed: the same bits again
    la.aux_to_voxel(la.SparseTensor(dev(sf), foreign.C, s), large2, inv.to(DEV), cnt.int().to(DEV), r)
    assert torch.equal(large.F, large2.F)
    flat = la.SparseTensor(torch.full((small_c.shape[0], w), AF.CONST, device=DEV), foreign.C, s)
    with spied() as ccalls:
        la.aux_to_voxel(flat, large2, inv.to(DEV), cnt.int().to(DEV), r)
    assert "link_devoxelize_forward" in ccalls and float((large2.F - AF.CONST).abs().max()) <= 2 * float(np.spacing(np.float32(AF.CONST)))
    case = {"frame": "corner", "w": w, "r": r, "family": "offset"}
    gate("b_foreign", case, route, "out", large.F, res[F64][0], A.dist(res[F32][0], res[F64][0]))
    gate("b_foreign", case, route, "grad_small", g, res[F64][1], A.dist(res[F32][1], res[F64][1]))


# ------------------------------------------------------------------------------------------ c. spvoxelize / spdevoxelize, backend
def _op_case(c, K, seed):
    rng = np.random.default_rng(seed)
    n, n1, nq = 700, 150, 300
    idx = rng.integers(-1, n1, n).astype(np.int32)
    counts = np.bincount(idx[idx >= 0], minlength=n1).astype(np.int32)
    counts[:5] = 0                                                                        # counts with zeros: rows of those voxels are skipped
    ind = rng.integers(-1, n1, (nq, K)).astype(np.int32)
    ind[:4] = -1                                                                          # rows whose indices are all -1
    w = rng.random((nq, K)).astype(np.float32)
    return idx, counts, ind, w, n, n1, nq


@pytest.mark.parametrize("c", AF.C_WIDTHS)
def test_c_voxelize_devoxelize(c):
    import link_amd as la
    for r in (1, 2, 3, 4, 5):
        K = r ** 3
        assert K in AF.C_K
        idx, counts, ind, w, n, n1, nq = _op_case(c, K, 10 * c + r)
        family = AF.FAMILIES[r % 2]
        x, top = AF.rows(family, n, c, c + r), AF.rows("normal", n1, c, c + r + 1)
        feat, gq = AF.rows(family, n1, c, c + r + 2), AF.rows("normal", nq, c, c + r + 3)
        case = {"c": c, "K": K, "family": family}
        route = {"k_passes": -(-K // 64), "j0_passes": -(-c // 64)}
        runs = []
        for _ in range(2):
            xd, fd = dev(x).requires_grad_(True), dev(feat).requires_grad_(True)
            poison()
            with spied() as calls:
                v = la.spvoxelize(xd, dev(idx), dev(counts))
                (gx,) = torch.autograd.grad(v, xd, dev(top))
                p = la.spdevoxelize(fd, dev(ind), dev(w), r)
                (gf,) = torch.autograd.grad(p, fd, dev(gq))
            assert [k for k in calls] == ["link_voxelize_forward", "link_voxelize_backward_n1", "link_devoxelize_forward",
                                          "link_devoxelize_backward"], calls
            runs.append((v.detach(), gx, p.detach(), gf))
        v, gx, p, gf = runs[0]
        for name, got, fn in (("voxelize_fwd", v, lambda dt: A.voxelize_fwd(x, idx, counts, dt)),
                              ("voxelize_bwd", gx, lambda dt: A.voxelize_bwd(top, idx, counts, n, dt)),
                              ("devoxelize_fwd", p, lambda dt: A.devoxelize_fwd(feat, ind, w, dt)),
                              ("devoxelize_bwd", gf, lambda dt: A.devoxelize_bwd(gq, ind, w, n1, dt))):
            r64, r32 = fn(F64), fn(F32)
            gate("c_ops", case, route, name, got, r64, A.dist(r32, r64))
        assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])   # the indexed ones: the same bits
        assert not v[:5].any() and not p[:4].any()                                           # skipped voxels and empty rows: zeros
        assert not gx[dev(idx) < 0].any() and not gx[dev(counts)[dev(idx).clamp(min=0).long()] == 0].any()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float64], ids=["f16", "bf16", "f64"])
def test_c_backend_row_types(dt):
    """the four feature functions of link_amd.backend under the row types the reference dispatches: the 16-bit inputs are the values
    (both restatements run on their exact widenings), fp32 accumulation, the result rounded to the type once"""
    from link_amd import backend as B
    c, r = 65, 2
    idx, counts, ind, w, n, n1, nq = _op_case(c, r ** 3, 99)
    x, top, feat, gq = (torch.from_numpy(AF.rows("normal", k, c, 40 + i)).to(dt) for i, k in enumerate((n, n1, n1, nq)))
    wt = torch.from_numpy(w).to(dt)
    xf, topf, featf, gqf, wf = (t.float() for t in (x, top, feat, gq, wt))                 # the case is these values (fp32-exact)
    case = {"c": c, "K": r ** 3, "dtype": str(dt).split(".")[-1]}
    poison()
    with spied() as calls:
        got = {"voxelize_fwd": B.voxelize_forward_cuda(x.to(DEV), dev(idx), dev(counts)),
               "voxelize_bwd": B.voxelize_backward_cuda(top.to(DEV), dev(idx), dev(counts), n),
               "devoxelize_fwd": B.devoxelize_forward_cuda(feat.to(DEV), dev(ind), wt.to(DEV), r),
               "devoxelize_bwd": B.devoxelize_backward_cuda(gq.to(DEV), dev(ind), wt.to(DEV), n1, r)}
    assert calls == ["link_voxelize_forward", "link_voxelize_backward_n1", "link_devoxelize_forward", "link_devoxelize_backward"]
    with pytest.raises(ValueError):                                                        # int32 idx and counts, as the forward asks
        B.voxelize_backward_cuda(top.to(DEV), dev(idx).long(), dev(counts), n)
    with pytest.raises(ValueError):
        B.voxelize_backward_cuda(top.to(DEV), dev(idx), dev(counts).long(), n)
    fns = {"voxelize_fwd": lambda d: A.voxelize_fwd(xf, idx, counts, d), "voxelize_bwd": lambda d: A.voxelize_bwd(topf, idx, counts, n, d),
           "devoxelize_fwd": lambda d: A.devoxelize_fwd(featf, ind, wf, d), "devoxelize_bwd": lambda d: A.devoxelize_bwd(gqf, ind, wf, n1, d)}
    for name, g in got.items():
        assert g.dtype == dt
        r64, r32 = fns[name](F64), fns[name](F32)
        gate("c_backend", case, {}, name, g, r64, A.dist(r32, r64), dt)


def test_c_backend_integer_functions():
    from link_amd import backend as B
    rng = np.random.default_rng(8)
    coords = rng.integers(-400, 400, (3000, 4)).astype(np.int32)
    coords[:, 3] = rng.integers(0, 3, 3000)
    assert np.array_equal(B.hash_cuda(dev(coords)).cpu().numpy(), A.fnv_hash(coords))
    off = A.kernel_offsets(3).numpy().astype(np.int32)
    want = np.stack([A.fnv_hash(coords + np.array([o[0], o[1], o[2], 0], np.int32)) for o in off], 0)
    assert np.array_equal(B.kernel_hash_cuda(dev(coords), dev(off)).cpu().numpy(), want)
    uniq = np.unique(coords, axis=0)
    tgt, qry = uniq[::2], uniq
    pos = A.lookup(tgt, qry).numpy()
    ids = np.arange(tgt.shape[0], dtype=np.int64) * 3 + 1
    got = B.hash_query_cuda(dev(A.fnv_hash(qry)), dev(A.fnv_hash(tgt)), dev(ids)).cpu().numpy()
    assert np.array_equal(got, np.where(pos >= 0, ids[np.clip(pos, 0, None)] + 1, 0))
    idx = rng.integers(-1, 200, 5000).astype(np.int32)
    assert np.array_equal(B.count_cuda(dev(idx), 200).cpu().numpy(), np.bincount(idx[idx >= 0], minlength=200))


# ------------------------------------------------------------------------------------------------------- d. calc_ti_weights
@pytest.mark.parametrize("scale", [1, 2, 4])
def test_d_trilinear_weights(scale):
    import link_amd as la
    rng = np.random.default_rng(scale)
    P = 4000
    pts = np.concatenate([(rng.random((P, 3)) - 0.5) * 60.0, rng.integers(0, 2, (P, 1))], 1).astype(np.float32)
    u = pts[:, :3].astype(np.float64) / scale
    pts = pts[np.minimum(u - np.floor(u), np.ceil(u) - u).min(1) >= 2.0 ** -9]             # away from the faces, where fp32 and fp64 may floor differently
    assert pts.shape[0] > 3900 and A.face_margin(pts, scale) >= 2.0 ** -10
    grid = np.concatenate([rng.integers(-30, 30, (500, 3)) * scale, np.zeros((500, 1))], 1).astype(np.float32)   # exactly on integer coordinates
    for family, p in (("interior", pts), ("integer", grid)):
        idx = rng.integers(-1, 500, (8, p.shape[0]))
        idx[:, :5] = -1                                                                   # points with no corner present
        idx[rng.integers(0, 8, 50), rng.integers(5, p.shape[0], 50)] = -1
        poison()
        with spied() as calls:
            got = la.calc_ti_weights(dev(p), dev(idx), scale=scale)
        assert calls == ["link_ti_weights"] and got.shape == (8, p.shape[0]) and got.dtype == torch.float32
        w64, w32 = A.ti_weights(p, idx, scale, F64), A.ti_weights(p, idx, scale, F32)
        gate("d_ti", {"scale": scale, "family": family}, {"scaled": scale != 1}, "weights", got, w64, A.dist(w32, w64))
        assert not got[:, :5].any() and not got[dev(idx) == -1].any()
        if family == "integer":                                                           # all of the weight on the cell's own corner
            assert np.array_equal(got[0].cpu().numpy(), (idx[0] != -1).astype(np.float32))


# ---------------------------------------------------------------- e. initial_voxelize -> point_to_voxel -> voxel_to_point
def _points_chain(pts, feats, pfeat, vfeat, go_v, go_p, force_hash, monkeypatch):
    import link_amd as la
    from link_amd import pointvoxel as PV
    from link_amd.index import GridTooLarge
    with monkeypatch.context() as mp:
        if force_hash:
            def boom(*a, **k):
                raise GridTooLarge("forced")
            mp.setattr(PV, "BlockIndex", boom)
            mp.setattr(PV, "foreign_neighbor_map", boom)
        f = dev(feats).requires_grad_(True)
        z = la.PointTensor(f, dev(pts))
        poison()
        with spied() as calls:
            st = la.initial_voxelize(z, 1, 1)
            (g_f,) = torch.autograd.grad(st.F, f, dev(go_v))
            z.F = dev(pfeat)
            v = la.point_to_voxel(st, z)
            xf = dev(vfeat).requires_grad_(True)
            p = la.voxel_to_point(la.SparseTensor(xf, st.C, 1), z)
            (g_x,) = torch.autograd.grad(p.F, xf, dev(go_p))
    native = "link_block_mean" in calls
    assert native != force_hash and ("link_hash_query" in calls) == force_hash
    assert "link_ti_weights" in calls and "link_devoxelize_forward" in calls
    return {"vox_F": st.F.detach(), "grad_feats": g_f, "p2v_F": v.F.detach(), "v2p_F": p.F.detach(), "grad_vox": g_x,
            "weights": z.weights[(1, 1, 1)]}, (st.C, z.additional_features["idx_query"][1], z.additional_features["counts"][1],
                                              z.idx_query[(1, 1, 1)], z.C)


@pytest.mark.parametrize("path", ["native", "hash"])
def test_e_point_voxel_chain(path, monkeypatch):
    pts, cells = AF.points()
    P, c = pts.shape[0], 6
    feats, pfeat = AF.rows("offset", P, c, 1), AF.rows("normal", P, 3, 2)
    _, vc, inv, cnt, scaled = A.initial_voxelize(pts, feats, 1, 1)
    M = vc.shape[0]
    vfeat, go_v, go_p = AF.rows("normal", M, 5, 3), AF.rows("normal", M, c, 4), AF.rows("normal", P, 5, 5)
    assert A.face_margin(pts) >= 2.0 ** -10
    ref = {}
    for dt in (F64, F32):
        v2p, idx8, w8 = A.voxel_to_point(vfeat, vc, 1, scaled, dtype=dt)
        ref[dt] = {"vox_F": A.block_mean(feats, inv, cnt, dt), "grad_feats": A.voxelize_bwd(go_v, inv, cnt, P, dt),
                   "p2v_F": A.point_to_voxel(scaled, pfeat, vc, 1, dt)[0], "v2p_F": v2p, "grad_vox": A.devoxelize_bwd(go_p, idx8, w8, M, dt),
                   "weights": w8}
    runs = [_points_chain(pts, feats, pfeat, vfeat, go_v, go_p, path == "hash", monkeypatch) for _ in range(2)]
    got, (C, idx_query, counts, corner_idx, zC) = runs[0]
    assert np.array_equal(C.cpu().numpy(), vc.numpy()) and np.array_equal(idx_query.cpu().numpy(), inv.numpy())
    assert np.array_equal(counts.cpu().numpy(), cnt.numpy()) and np.array_equal(corner_idx.cpu().numpy(), idx8.numpy())
    assert np.array_equal(zC.cpu().numpy(), scaled.numpy())
    keep = cnt <= AF.SORT_MAX_SEG                                                          # all but the 8193-point cell
    assert int((~keep).sum()) == 1 and int(cnt[keep].max()) == AF.SORT_MAX_SEG
    case = {"frame": "points", "path": path, "c": c}
    for name in ref[F64]:
        gate("e_points", case, {"native": path == "native"}, name, got[name], ref[F64][name], A.dist(ref[F32][name], ref[F64][name]))
    if path == "native":
        # segments of at most 8192 ids are sorted by id: the same bits every run, and the bits of the sequential mean; the 8193-point
        # cell is left in atomic-rank order and is gated only
        seq = A.block_mean_seq32(feats, inv.numpy(), cnt.numpy())
        assert torch.equal(runs[0][0]["vox_F"][keep.to(DEV)], runs[1][0]["vox_F"][keep.to(DEV)])
        assert np.array_equal(got["vox_F"].cpu().numpy()[keep.numpy()], seq[keep.numpy()])
    for name in ("grad_feats", "v2p_F", "weights"):                                        # voxelize backward, devoxelize forward: indexed
        assert torch.equal(runs[0][0][name], runs[1][0][name]), name
