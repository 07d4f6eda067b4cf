"""The exact gate over the integer layer every float kernel stands on: csrc/index.hip (k_cell_count, k_cell_scan, k_place, k_sort_seg,
the first-voxel family k_cell_count_first / k_vox_scan<TICKET> / k_place_first, link_index_cells, k_neighbor_map, k_cell_table and
its clear) and csrc/kmap.hip (k_kmap_candidates, k_kmap_box_table, k_kmap_transpose), with link_amd/index.py on top, on frames built
for their edges (tests/index_frames.py, whose every claim tests/test_cpu_index_frames.py checks) against the plain numpy restatement
tests/index_ref.py (pinned there to the C oracle, the recorded fixtures and link_amd.get_kernel_offsets).

Every comparison is np.array_equal: there is no tolerance in this file.  Caller-owned output buffers start as -7 and are compared
WHOLE -- the reference in front, -7 behind it -- so an entry that is never written cannot pass and one written past its range
cannot either; scratch starts as random bytes.  Cases of the kernel maps run under helpers.spied() and assert the entries
index_frames.route_* predict, with link_amd's sphash / sphashquery replaced by functions that fail: the hash chain cannot stand in
for the builders.  Each case appends one row to index_parity.jsonl under LINK_AMD_PARITY_DIR before its verdict (the case's fields,
n, V, M, scan tiles, the entries called, the number of arrays compared); profiles/index_parity.jsonl is one MI355X run.

Groups: a the cell-order scan (link_index_build through ctypes and BlockIndex on the same frame); b voxel order and the
wave-aggregated counter, blocks of exact sizes through k_sort_seg; c voxels outside the grid, n = 0, reuse of counters and scratch;
d the first-voxel scan against the reference directly, the 1025-tile frame that alone takes k_vox_scan<true>, and a sequence of
frames on one set of tables with ElkCorePlan's arena beside it; e link_index_cells / unique_cells; f neighbour maps and the cell
table; g the kernel maps and Conv3d._route / spdownsample on top.

The V = 130 x 2048 + 5 cases of group a exist because a look-back may then have to walk more than one 64-tile window; whether it
does depends on how the workgroups are scheduled and cannot be forced.  Those cases assert results, not the path taken.

The committed run (profiles/index_parity.jsonl): 246 tests, 263 rows, 3491 arrays compared, none different; 5.2 s on one MI355X.

That the gate bites: four value-only defects seeded one at a time in scratch builds (never committed), the file run once on each.
  1 the scalar tail of k_cell_scan one cell short.  Seeded in the tail's AGGREGATE (the last cell of the grid left out of the sums,
    its counter still handed to the write loop): read literally -- the counter itself read as 0 -- the cell's cell_start is never
    written and k_place would scatter through scratch.  Fails 48 cases of a -- every grid whose V is no multiple of 8 (1, 7, 9,
    2047, 2049, 4097, 17 x 241, 64 x 2048 + 1, 130 x 2048 + 5) under every occupancy that occupies the last cell (full, last,
    alternate, edges, tail_tile), at s 1, 3, 7 and with duplicates, none with V a multiple of 8 -- and b[cell], the 8193-block[cell]
    and the reuse case (V = 4097); the first-voxel cases, e, f and g pass.
  2 `lane <= first` -> `lane < first` in the look-back of k_cell_scan.  Run on the cases whose cell scan has at most three tiles
    (with more, an under-counted prefix can leave positions of perm_tmp unwritten, and k_sort_seg would follow them out of bounds):
    fails all 34 selected cases of a with voxels in a tile before the last (V = 2049, 4096, 4097, 17 x 241: full, first, edges,
    alternate, head_tile; `last` and `tail_tile` pass, as they must: the tiles before are empty), b[cell], the 8193-block[cell], the
    reuse case, e and 60 of the 88 kernel-map cases (those whose site grid spans more than one tile).  It did not stall.
  3 truncating division in k_kmap_candidates: fails 50 kernel-map cases (every candidate-rule geometry: the frame has negative
    coordinates), all 12 chained cases and the INT32_MIN frame; the floor-rule and stride-1 cases pass.
  4 a plain store for atomicMin in k_kmap_transpose: fails test_g_transpose_with_duplicate_output_rows_and_foreign_entries alone
    (unique output rows have one j per entry: nothing competes).

Found: strided_out_coords let sites and taps that leave the int32 range wrap into wrong rows (frames within 8 of INT32_MAX /
INT32_MIN); it now refuses them with ValueError before any launch (pinned by test_g_coordinates_at_the_ends_of_int32; the box table,
the cubic map and the transposed table are exact there).  The header said link_index_cells reports dropped rows in the status word
(it writes 0: NVALID < n is the sign) and promised perm ascending inside every block (up to 8192 voxels): both sentences corrected.
No wrong value was found in the scans, the neighbour maps, the cell table or the kernel maps inside the int32 range."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import index_frames as IF
import index_ref as R
from helpers import spied
from ref64 import record_row

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = -7
HOST_ONLY = ("link_grid_from_bounds", "link_index_scratch_bytes", "link_last_error")        # host helpers: no launch behind them


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def host(t):
    return t.cpu().numpy().astype(np.int64)


def link_grid(grid, s):
    from link_amd import _lib as L
    g = L.LinkGrid()
    g.s = int(s)
    for a in range(4):
        g.lo[a], g.dim[a] = int(grid[0][a]), int(grid[1][a])
    return g


def voxel_bounds(grid, s):
    lo, dim = np.asarray(grid[0]), np.asarray(grid[1])
    hi = lo + dim - 1
    return (tuple(int(v) for v in lo[:3] * s) + (int(lo[3]),), tuple(int(v) for v in hi[:3] * s + s - 1) + (int(hi[3]),))


def launched(calls):
    return [c for c in calls if c not in HOST_ONLY]


def row_out(**fields):
    record_row(fields, name="index_parity.jsonl")


class Tables:
    """caller-owned tables of link_index_build / _build_first / _cells: outputs -7, scratch random bytes, counters zero"""

    def __init__(self, n_cap, grid, s, first=False):
        from link_amd import _lib as L
        i32 = dict(dtype=torch.int32, device=DEV)
        self.L, self.grid, self.s, self.n_cap = L, link_grid(grid, s), s, n_cap
        self.v = v = self.grid.cells
        self.cell_counts = torch.zeros(v, **i32)
        self.cell_pair = torch.zeros(v, dtype=torch.int64, device=DEV)
        self.nbytes = L.lib().link_index_scratch_bytes(n_cap, v)
        self.scratch = torch.randint(0, 255, (self.nbytes,), dtype=torch.uint8, device=DEV)
        self.cell_blk = torch.full((v,), 0 if first else FILL, **i32)      # the first-voxel build keeps the table itself: zero once
        self.hdr = torch.zeros(L.HDR_WORDS, **i32)
        self.refill()

    def refill(self):
        i32 = dict(dtype=torch.int32, device=DEV)
        n = max(self.n_cap, 1)
        self.vox_blk = torch.full((n,), FILL, **i32)
        self.idx_query = torch.full((n,), FILL, dtype=torch.int64, device=DEV)
        self.perm = torch.full((n,), FILL, **i32)
        self.vox_sorted = torch.full((n, 4), FILL, **i32)
        self.pos_blk = torch.full((n,), FILL, **i32)
        self.blk_start = torch.full((n + 1,), FILL, **i32)
        self.blk_coords = torch.full((n, 4), FILL, **i32)
        self.counts = torch.full((n,), FILL, **i32)

    def build(self, coords, first=False, grid=None, counters=None, scratch=None):
        L, n = self.L, coords.shape[0]
        g = self.grid if grid is None else grid
        sc = self.scratch if scratch is None else scratch
        tail = (self.cell_blk.data_ptr(), self.vox_blk.data_ptr(), self.idx_query.data_ptr(), self.perm.data_ptr(),
                self.vox_sorted.data_ptr(), self.pos_blk.data_ptr(), self.blk_start.data_ptr(), self.blk_coords.data_ptr(),
                self.counts.data_ptr(), self.hdr.data_ptr(), L.current_stream_handle())
        if first:
            L.check(L.lib().link_index_build_first(coords.data_ptr(), n, ctypes.byref(g), self.cell_pair.data_ptr(), sc.data_ptr(),
                                                   sc.numel(), *tail), "link_index_build_first")
        else:
            cc = self.cell_counts if counters is None else counters
            L.check(L.lib().link_index_build(coords.data_ptr(), n, ctypes.byref(g), cc.data_ptr(), sc.data_ptr(), sc.numel(), *tail),
                    "link_index_build")
        torch.cuda.synchronize()

    def cells(self, rows):
        L, n = self.L, rows.shape[0]
        L.check(L.lib().link_index_cells(rows.data_ptr(), n, ctypes.byref(self.grid), self.cell_counts.data_ptr(),
                                         self.scratch.data_ptr(), self.scratch.numel(), self.cell_blk.data_ptr(),
                                         self.blk_start.data_ptr(), self.blk_coords.data_ptr(), self.counts.data_ptr(),
                                         self.hdr.data_ptr(), L.current_stream_handle()), "link_index_cells")
        torch.cuda.synchronize()


def padded(ref, size, tail_shape=()):
    out = np.full((size,) + tail_shape, FILL, np.int64)
    out[: ref.shape[0]] = ref
    return out


def diff_tables(t, ref, n, with_voxels=True, skip=()):
    """names of the arrays of `t` that differ from the reference (whole buffers, -7 behind the reference) and how many were compared"""
    L = t.L
    h = t.hdr.tolist()
    m = ref["m"]
    cap = max(t.n_cap, 1)
    want = {"hdr": np.array([m, ref.get("status", 0), ref["nvalid"]]),
            "blk_coords": padded(ref["blk_coords"], cap, (4,)), "counts": padded(ref["counts"], cap),
            "blk_start": padded(ref["blk_start"], cap + 1), "cell_blk": ref["cell_blk"]}
    got = {"hdr": np.array([h[L.HDR_M], h[L.HDR_STATUS], h[L.HDR_NVALID]]), "blk_coords": host(t.blk_coords), "counts": host(t.counts),
           "blk_start": host(t.blk_start), "cell_blk": host(t.cell_blk)}
    if with_voxels:
        vb = padded(ref["vox_blk"], cap)
        want.update(vox_blk=vb, idx_query=vb, perm=padded(ref["perm"], cap), pos_blk=padded(ref["pos_blk"], cap),
                    vox_sorted=padded(ref["vox_sorted"], cap, (4,)))
        got.update(vox_blk=host(t.vox_blk), idx_query=host(t.idx_query), perm=host(t.perm), pos_blk=host(t.pos_blk),
                   vox_sorted=host(t.vox_sorted))
    names = [k for k in want if k not in skip]
    return [k for k in names if not np.array_equal(got[k], want[k])], len(names)


def diff_block_index(idx, ref, n):
    """the same for a BlockIndex (exactly sized views of its buffers)"""
    m = ref["m"]
    h = idx.hdr.tolist()
    got = {"hdr": np.array(h[:3]), "blk_coords": host(idx.blk_coords[:m]), "counts": host(idx.counts_buf[:m]),
           "blk_start": host(idx.blk_start[: m + 1]), "cell_blk": host(idx.cell_blk), "vox_blk": host(idx.vox_blk),
           "idx_query": host(idx.idx_query), "perm": host(idx.perm[: ref["nvalid"]]), "pos_blk": host(idx.pos_blk[: ref["nvalid"]]),
           "vox_sorted": host(idx.vox_sorted[: ref["nvalid"]])}
    want = dict(ref, hdr=np.array([m, ref["status"], ref["nvalid"]]), idx_query=ref["vox_blk"])
    return [k for k in got if not np.array_equal(got[k], want[k])], len(got)


# ------------------------------------------------------------------------------------------------------------- a: cell scan
@pytest.mark.parametrize("case", IF.SCAN_CASES, ids=IF.scan_id)
def test_a_cell_scan(case):
    from link_amd.index import BlockIndex
    coords, grid, cells, per = IF.scan_case(case)
    n, s = coords.shape[0], case["s"]
    ref = R.block_index(coords, s, "cell", grid)
    t = Tables(n, grid, s)
    c = dev(coords)
    t.build(c)
    bad, k = diff_tables(t, ref, n)
    dirty = int(t.cell_counts.abs().sum())
    idx = BlockIndex(c, s, bounds=voxel_bounds(grid, s))
    bad2, k2 = diff_block_index(idx, ref, n)
    row_out(test="a_cell_scan", dim=list(case["dim"]), occ=case["occ"], s=s, dup=case["dup"], n=n, V=t.v, M=ref["m"],
            tiles=IF.tiles_of(t.v), entries=["link_index_build"], compared=k + k2, differ=bad + bad2)
    assert ref["m"] == cells.size and ref["status"] == 0
    assert bad == [] and bad2 == [] and dirty == 0, (IF.scan_id(case), bad, bad2, dirty)
    assert idx.v == t.v and idx.M == ref["m"]


# ------------------------------------------------------------------------------------------------------------ b: voxel order
@pytest.fixture(scope="module")
def order_data():
    vox, grid, sizes = IF.order_frame()
    return vox, grid, sizes


@pytest.mark.parametrize("first", [False, True], ids=["cell", "first"])
def test_b_voxel_orders_and_exact_blocks(order_data, first):
    """Every order of the same voxels: each equal to the reference (ascending voxel id inside every block, the 8192-block included),
    the same blocks, counts and starts in every order, and per block the same set of voxels."""
    vox, grid, sizes = order_data
    n = vox.shape[0]
    sets = {}
    for order in IF.ORDERS:
        coords = IF.orders(vox, sizes, order)
        ref = R.block_index(coords, IF.ORDER_S, "first" if first else "cell", grid)
        t = Tables(n, grid, IF.ORDER_S, first)
        t.build(dev(coords), first=first)
        bad, k = diff_tables(t, ref, n)
        row_out(test="b_voxel_orders", order=order, numbering="first" if first else "cell", n=n, V=t.v, M=ref["m"],
                tiles=IF.tiles_of(n if first else t.v), entries=["link_index_build_first" if first else "link_index_build"],
                compared=k, differ=bad)
        assert bad == [], (order, bad)
        assert int(t.cell_counts.abs().sum()) == 0 and int(t.cell_pair.abs().sum()) == 0
        perm, bs = host(t.perm), host(t.blk_start)
        blocks = {}
        for b in range(ref["m"]):
            blocks[tuple(host(t.blk_coords)[b])] = {tuple(r) for r in coords[perm[bs[b]:bs[b + 1]]].tolist()}
        sets[order] = blocks
    assert all(sets[o] == sets["sorted"] for o in IF.ORDERS)
    assert sorted(len(v) for v in sets["sorted"].values()) == sorted(sizes.values())


@pytest.mark.parametrize("first", [False, True], ids=["cell", "first"])
def test_b_block_past_sort_limit(first):
    """A block of 8193 voxels: past SORT_MAX_SEG its segment of perm holds the block's ids in no promised order -- checked as a set;
    everything outside that segment, and every other array, exactly."""
    vox, grid, sizes = IF.order_frame(big=IF.SORT_MAX_SEG + 1)
    coords = IF.orders(vox, sizes, "random")
    n = coords.shape[0]
    ref = R.block_index(coords, IF.ORDER_S, "first" if first else "cell", grid)
    t = Tables(n, grid, IF.ORDER_S, first)
    t.build(dev(coords), first=first)
    bad, k = diff_tables(t, ref, n, skip=("perm", "vox_sorted"))
    b = int(np.argmax(ref["counts"]))
    lo, hi = int(ref["blk_start"][b]), int(ref["blk_start"][b + 1])
    perm, vs = host(t.perm), host(t.vox_sorted)
    row_out(test="b_block_past_sort_limit", numbering="first" if first else "cell", n=n, V=t.v, M=ref["m"], tiles=IF.tiles_of(n if first else t.v),
            entries=["link_index_build_first" if first else "link_index_build"], compared=k + 4, differ=bad)
    assert hi - lo == IF.SORT_MAX_SEG + 1 and bad == [], bad
    keep = np.r_[0:lo, hi:n]
    assert np.array_equal(perm[keep], ref["perm"][keep]) and np.array_equal(vs[keep], ref["vox_sorted"][keep])
    assert np.array_equal(np.sort(perm[lo:hi]), ref["perm"][lo:hi])
    assert np.array_equal(vs[lo:hi, 3], perm[lo:hi]) and np.array_equal(vs[lo:hi, :3], coords[perm[lo:hi], :3])


# --------------------------------------------------------------------------------------------------------------- c: outside
@pytest.mark.parametrize("first", [False, True], ids=["cell", "first"])
@pytest.mark.parametrize("which", [(i,) for i in range(8)] + [tuple(range(8))], ids=lambda w: "all" if len(w) == 8 else "%s_%s" % IF.FACES[w[0]])
def test_c_voxels_outside_the_grid(which, first):
    inside, grid, beyond, at = IF.outside_frame()
    coords, ids = IF.with_outside(inside, beyond, at, which)
    n = coords.shape[0]
    ref = R.block_index(coords, IF.OUT_S, "first" if first else "cell", grid)
    t = Tables(n, grid, IF.OUT_S, first)
    t.build(dev(coords), first=first)
    bad, k = diff_tables(t, ref, n)
    row_out(test="c_outside", faces=["%s_%s" % IF.FACES[i] for i in which], numbering="first" if first else "cell", n=n, V=t.v, M=ref["m"],
            tiles=IF.tiles_of(n if first else t.v), entries=["link_index_build_first" if first else "link_index_build"], compared=k, differ=bad)
    assert ref["status"] == 1 and ref["nvalid"] == n - len(which) and ref["blk_start"][-1] == ref["nvalid"]
    assert np.array_equal(np.flatnonzero(ref["vox_blk"] < 0), ids)
    assert bad == [], bad
    # everything else: the index of the frame without those voxels, voxel ids kept
    keep = np.setdiff1d(np.arange(n), ids)
    clean = R.block_index(coords[keep], IF.OUT_S, "first" if first else "cell", grid)
    assert np.array_equal(host(t.blk_coords)[: clean["m"]], clean["blk_coords"]) and np.array_equal(host(t.counts)[: clean["m"]], clean["counts"])
    assert np.array_equal(host(t.vox_blk)[keep], clean["vox_blk"]) and np.array_equal(host(t.perm)[: n - len(which)], keep[clean["perm"]])
    assert np.array_equal(host(t.cell_blk), clean["cell_blk"])


def test_c_empty_frame_and_reuse_of_counters_and_scratch():
    """n = 0 on a grid with V > 0, then two builds of different n and V on the same counters and scratch: counters zero after each"""
    a = IF.scan_case(dict(dim=(4097, 1, 1, 1), lo=IF.LO_NEG, occ="alternate", s=3, dup=False))
    b = IF.scan_case(dict(dim=(8, 8, 8, 4), lo=IF.LO_NEG, occ="full", s=3, dup=True))
    ta, tb = Tables(a[0].shape[0], a[1], 3), Tables(b[0].shape[0], b[1], 3)
    empty = dev(np.zeros((0, 4)))
    for first in (False, True):
        ta.refill()
        ta.cell_blk.fill_(0 if first else FILL)
        ta.build(empty, first=first)
        ref = R.block_index(np.zeros((0, 4)), 3, "cell", a[1])
        bad, k = diff_tables(ta, ref, 0, with_voxels=False)
        row_out(test="c_empty", numbering="first" if first else "cell", n=0, V=ta.v, M=0, tiles=IF.tiles_of(0 if first else ta.v),
                entries=["link_index_build_first" if first else "link_index_build"], compared=k, differ=bad)
        assert bad == [] and int(ta.cell_counts.abs().sum()) == 0, bad
        assert int((ta.perm != FILL).sum()) == 0 and int((ta.vox_blk != FILL).sum()) == 0
    counters = torch.zeros(max(ta.v, tb.v), dtype=torch.int32, device=DEV)                  # shared by both
    scratch = torch.randint(0, 255, (max(ta.nbytes, tb.nbytes),), dtype=torch.uint8, device=DEV)
    for t, (coords, grid, _, _) in ((ta, a), (tb, b), (ta, a)):
        t.refill()
        t.build(dev(coords), counters=counters, scratch=scratch)
        ref = R.block_index(coords, 3, "cell", grid)
        bad, k = diff_tables(t, ref, coords.shape[0])
        row_out(test="c_reuse", n=coords.shape[0], V=t.v, M=ref["m"], tiles=IF.tiles_of(t.v), entries=["link_index_build"], compared=k, differ=bad)
        assert bad == [] and int(counters.abs().sum()) == 0, bad


# ----------------------------------------------------------------------------------------------------------- d: first voxel
@pytest.mark.parametrize("n", IF.FIRST_N)
def test_d_first_voxel_scan(n):
    coords = IF.first_frame(n)
    lo, hi = IF.first_bounds()
    grid = R.grid_of(lo, hi, IF.FIRST_S)
    ref = R.block_index(coords, IF.FIRST_S, "first", grid)
    t = Tables(n, grid, IF.FIRST_S, True)
    t.build(dev(coords), first=True)
    bad, k = diff_tables(t, ref, n)
    row_out(test="d_first_voxel_scan", n=n, V=t.v, M=ref["m"], tiles=IF.tiles_of(n), entries=["link_index_build_first"], compared=k, differ=bad)
    assert bad == [] and int(t.cell_pair.abs().sum()) == 0, bad
    assert t.hdr.tolist()[t.L.HDR_STATUS_ACC] == 0


def test_d_first_voxel_scan_in_ticket_order():
    """2^21 + 1 voxels = 1025 tiles: the only size in the suite past VSCAN_RESIDENT, where k_vox_scan<true> takes its tile from a
    ticket"""
    coords, (lo, hi) = IF.first_big()
    n = coords.shape[0]
    grid = R.grid_of(lo, hi, IF.BIG_S)
    ref = R.block_index(coords, IF.BIG_S, "first", grid)
    t = Tables(n, grid, IF.BIG_S, True)
    t.build(dev(coords), first=True)
    bad, k = diff_tables(t, ref, n)
    row_out(test="d_first_voxel_ticket", n=n, V=t.v, M=ref["m"], tiles=IF.tiles_of(n), entries=["link_index_build_first"], compared=k, differ=bad)
    assert IF.tiles_of(n) == IF.VSCAN_RESIDENT + 1
    assert bad == [] and int(t.cell_pair.abs().sum()) == 0, bad


def test_d_sequence_on_one_set_of_tables():
    """Frames one after another on the same tables (nothing refilled between them: what a frame leaves is what the next one finds),
    ElkCorePlan's general-layout arena in first-voxel order beside it (frames with n > 0; blocks() refuses the frame with a
    dropped voxel, whose M is read from the plan's header)."""
    import link_amd as la
    from link_amd import _lib as L
    seq = IF.first_sequence()
    lo, hi = IF.first_bounds()
    grid = R.grid_of(lo, hi, IF.SEQ_S)
    n_cap = max(c.shape[0] for _, c in seq)
    t = Tables(n_cap, grid, IF.SEQ_S, True)
    C, groups, r = 16, 2, 2                                                # (the general layout of tests/test_gpu_index_first.py: C 16, sin, s 8, r 2)
    torch.manual_seed(5)
    blk = la.ELKBlock(C, C, groups=groups, baseop="sin", variant="encoder").cuda().eval()
    plan = la.ElkCorePlan(n_cap, C, "sin", C // groups, r, IF.SEQ_S, (lo, hi), DEV, layout="general", block_order="first")
    plan.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, None, blk.norm.weight,
              blk.norm.bias)
    for name, coords in seq:
        n = coords.shape[0]
        ref = R.block_index(coords, IF.SEQ_S, "first", grid)
        c = dev(coords)
        t.build(c, first=True)
        h = t.hdr.tolist()
        got_cells = np.flatnonzero(host(t.cell_blk) != 0)
        # the tables keep the previous frame's rows past this frame's: only the valid fronts are compared here
        m, nv = ref["m"], ref["nvalid"]
        pairs = [("hdr", np.array(h[:3]), np.array([m, ref["status"], nv])), ("cell_blk", host(t.cell_blk), ref["cell_blk"]),
                 ("blk_start", host(t.blk_start)[: m + 1], ref["blk_start"])]
        if n:
            pairs += [("blk_coords", host(t.blk_coords)[:m], ref["blk_coords"]), ("counts", host(t.counts)[:m], ref["counts"]),
                      ("vox_blk", host(t.vox_blk)[:n], ref["vox_blk"]), ("idx_query", host(t.idx_query)[:n], ref["vox_blk"]),
                      ("perm", host(t.perm)[:nv], ref["perm"]), ("pos_blk", host(t.pos_blk)[:nv], ref["pos_blk"]),
                      ("vox_sorted", host(t.vox_sorted)[:nv], ref["vox_sorted"])]
        bad = [k for k, a, b in pairs if not np.array_equal(a, b)]
        plan_m = None
        if n:
            plan.run(torch.zeros(n, C, device=DEV), c)
            torch.cuda.synchronize()
            if ref["status"]:
                with pytest.raises(L.LinkAmdError):
                    plan.blocks()
                plan_m = int(plan.hdr.tolist()[L.HDR_M])
            else:
                plan_m = plan.blocks()
        row_out(test="d_sequence", frame=name, n=n, V=t.v, M=m, tiles=IF.tiles_of(n), entries=["link_index_build_first"],
                compared=len(pairs), differ=bad, plan_M=plan_m)
        assert bad == [], (name, bad)
        assert np.array_equal(got_cells, np.flatnonzero(ref["cell_blk"]))                 # non-zero at exactly this frame's cells
        assert int(t.cell_pair.abs().sum()) == 0
        assert h[L.HDR_STATUS] == ref["status"] == int(name == "dropped") and h[L.HDR_STATUS_ACC] == 0      # published and reset
        assert plan_m is None or plan_m == m, (name, plan_m, m)


# ------------------------------------------------------------------------------------------------------------------ e: cells
def test_e_index_cells_and_unique_cells():
    """link_index_cells on candidate-like rows: sorted unique rows, their multiplicities, hdr[M], NVALID = rows inside, the cell
    table, counters zero afterwards.  Status as the code defines it: link_index_cells never sets it -- rows outside the grid are
    dropped silently (hdr[STATUS] = 0); NVALID < n is how a caller can tell."""
    from link_amd import _lib as L
    from link_amd.index import unique_cells
    rows, grid, n_in, n_out = IF.cells_frame()
    n = rows.shape[0]
    ref = dict(R.unique_cells(rows, grid), status=0)
    t = Tables(n, grid, 1)
    t.hdr.fill_(FILL)
    t.cells(dev(rows))
    bad, k = diff_tables(t, ref, n, with_voxels=False)
    lo, dim = grid
    with spied() as calls:
        sites, hdr = unique_cells(dev(rows), (tuple(int(v) for v in lo), tuple(int(v) for v in lo + dim - 1)))
    h = hdr.tolist()
    bad2 = [] if (h[L.HDR_M], h[L.HDR_STATUS], h[L.HDR_NVALID]) == (ref["m"], 0, ref["nvalid"]) else ["hdr"]
    if not np.array_equal(host(sites)[: ref["m"]], ref["blk_coords"]):
        bad2.append("sites")
    row_out(test="e_index_cells", n=n, V=t.v, M=ref["m"], tiles=IF.tiles_of(t.v), entries=launched(calls), compared=k + 2, differ=bad + bad2)
    assert ref["nvalid"] == n_in == n - n_out and ref["m"] == 400
    assert bad == [] and bad2 == [] and int(t.cell_counts.abs().sum()) == 0, (bad, bad2)
    assert launched(calls) == ["link_index_cells"]


# ---------------------------------------------------------------------------------------------------------- f: neighbour map
@pytest.mark.parametrize("name", ["solid", "thin_x", "thin_y", "thin_z", "batch"])
def test_f_neighbor_maps(name):
    """link_neighbor_map on BlockIndex rows (r = 1..5, transposed at even r; hdr and m as an upper bound) and through
    foreign_neighbor_map (step 1..3, transposed at even r, table_rows != rows)."""
    from link_amd import _lib as L
    from link_amd.index import BlockIndex, foreign_neighbor_map
    rows = IF.nbr_frames()[name]
    m = rows.shape[0]
    idx = BlockIndex(dev(rows), 1)
    assert idx.M == m and np.array_equal(host(idx.block_coords), rows)
    others = rows[::3]                                                   # table_rows != rows: every third row, shifted order
    others = others[np.random.default_rng(7).permutation(others.shape[0])]
    bad, k, entries = [], 0, set()
    for r in IF.NBR_R:
        for tr in ((False, True) if r % 2 == 0 else (False,)):
            want = R.neighbor_map(rows, r, 1, tr)
            if name == "solid":
                assert np.array_equal(want, IF.solid_neighbor(rows, (-3, -2, -4), (7, 6, 8), r, 1, tr))
            with spied() as calls:
                got = idx.neighbor_map(r, transpose=tr)
            entries.update(launched(calls))
            k += 1
            if not np.array_equal(host(got), want):
                bad.append(("index", r, tr))
            # m handed in as an upper bound, the row count read from hdr: rows past M are not written
            cap = torch.full((m + 5, r ** 3), FILL, dtype=torch.int32, device=DEV)
            L.check(L.lib().link_neighbor_map(idx.blk_coords.data_ptr(), idx.cell_blk.data_ptr(), ctypes.byref(idx.grid), idx.hdr.data_ptr(),
                                              m + 5, r, 1, int(tr), cap.data_ptr(), L.current_stream_handle()), "link_neighbor_map")
            k += 1
            if not np.array_equal(host(cap), padded(want, m + 5, (r ** 3,))):
                bad.append(("hdr_cap", r, tr))
            for step in IF.NBR_STEP:
                for tab in (None, others):
                    want = R.neighbor_map(rows, r, step, tr, tab)
                    if name == "solid" and tab is None:
                        assert np.array_equal(want, IF.solid_neighbor(rows, (-3, -2, -4), (7, 6, 8), r, step, tr))
                    with spied() as calls:
                        got = foreign_neighbor_map(dev(rows), r, transpose=tr, step=step, table_rows=None if tab is None else dev(tab))
                    entries.update(launched(calls))
                    k += 1
                    if not np.array_equal(host(got), want):
                        bad.append(("foreign", r, tr, step, tab is not None))
    row_out(test="f_neighbor_maps", frame=name, n=m, V=idx.v, M=m, tiles=IF.tiles_of(idx.v), entries=sorted(entries), compared=k,
            differ=[list(map(str, b)) for b in bad])
    assert bad == [], bad
    assert entries == {"link_neighbor_map", "link_coords_bbox", "link_cell_table_build", "link_cell_table_clear"}


def test_f_cell_table_smallest_index_wins_and_clear():
    from link_amd import _lib as L
    rows, grid = IF.table_frame()
    g = link_grid(grid, 1)
    tab = torch.zeros(g.cells, dtype=torch.int32, device=DEV)
    hdr = torch.zeros(L.HDR_WORDS, dtype=torch.int32, device=DEV)
    r = dev(rows)
    st = L.current_stream_handle()
    L.check(L.lib().link_cell_table_build(r.data_ptr(), rows.shape[0], ctypes.byref(g), tab.data_ptr(), hdr.data_ptr(), st), "build")
    want, outside = R.cell_table(rows, grid)
    got = host(tab)
    L.check(L.lib().link_cell_table_clear(r.data_ptr(), rows.shape[0], ctypes.byref(g), tab.data_ptr(), st), "clear")
    cleared = int(tab.abs().sum())
    far = rows.copy()
    far[3, 1] += 100                                                    # a row outside the grid: status bit 0, no write
    hdr2 = torch.zeros(L.HDR_WORDS, dtype=torch.int32, device=DEV)
    L.check(L.lib().link_cell_table_build(dev(far).data_ptr(), rows.shape[0], ctypes.byref(g), tab.data_ptr(), hdr2.data_ptr(), st), "build")
    want2, outside2 = R.cell_table(far, grid)
    ok2 = np.array_equal(host(tab), want2)
    row_out(test="f_cell_table", n=rows.shape[0], V=g.cells, M=int((want > 0).sum()), tiles=0,
            entries=["link_cell_table_build", "link_cell_table_clear"], compared=3, differ=[] if np.array_equal(got, want) and ok2 else ["table"])
    assert np.array_equal(got, want) and not outside and hdr.tolist()[L.HDR_STATUS] == 0
    assert cleared == 0
    assert ok2 and outside2 and hdr2.tolist()[L.HDR_STATUS] == 1


# ------------------------------------------------------------------------------------------------------------ g: kernel maps
@contextlib.contextmanager
def no_hash():
    """link_amd's sphash / sphashquery fail inside the block: the hash chain cannot stand in for the builders"""
    import link_amd.elk as E

    def refuse(*a, **k):
        raise AssertionError("the hash chain ran where a builder was expected")
    saved = E.sphash, E.sphashquery
    E.sphash = E.sphashquery = refuse
    try:
        yield
    finally:
        E.sphash, E.sphashquery = saved


@pytest.fixture(scope="module")
def kmap_frames():
    base = IF.kmap_frame()
    return {ts: IF.on_lattice(base, ts) if ts != (1, 1, 1) else base for ts in ((1, 1, 1), (2, 1, 1), (2, 2, 1))}, base


def _bounds(c):
    return tuple(int(v) for v in c.min(0)), tuple(int(v) for v in c.max(0))


@pytest.mark.parametrize("ks,st,ts", IF.KMAP_CASES, ids=lambda v: "".join(map(str, v)))
def test_g_kernel_maps(kmap_frames, ks, st, ts):
    import link_amd as la
    import link_amd.functional as F
    from link_amd.index import box_neighbor_map, strided_out_coords, transpose_table
    frames, base = kmap_frames
    coords = frames[ts]
    n = coords.shape[0]
    strided = any(v > 1 for v in st)
    kvol = ks[0] * ks[1] * ks[2]
    offs = R.kernel_offsets(ks, ts)
    assert np.array_equal(la.get_kernel_offsets(ks, stride=ts).numpy(), offs)
    want_c = R.out_sites(coords, ks, st, ts) if strided else coords.astype(np.int64)
    want_t = R.gather_table(want_c, offs, coords)
    want_b = R.transpose_table(want_t, n)
    bad, k, entries = [], 0, []
    c = dev(coords)
    with no_hash():
        # the entry points of index.py by themselves
        if strided:
            with spied() as calls:
                got_c, box = strided_out_coords(c, _bounds(coords), ks, st, ts)
            entries += launched(calls)
            assert launched(calls) == IF.route_sites(ks, st, ts), (launched(calls), IF.route_sites(ks, st, ts))
            k += 1
            if not np.array_equal(host(got_c), want_c):
                bad.append("strided_out_coords")
            # a tight box only where the floor rule promises one
            assert (box is not None) == (R.floor_rule(ks, st) and want_c.shape[0] > 0)
            if box is not None:
                assert box == _bounds(want_c)
            # off the tensor-stride lattice: every residue present, same rule (no site from an input that is no multiple of ts)
            off_c = R.out_sites(base, ks, st, ts)
            k += 1
            if not np.array_equal(host(F.spdownsample(dev(base), st, ks, ts)), off_c):
                bad.append("spdownsample")
        out_rows = dev(want_c)
        with spied() as calls:
            got_t = box_neighbor_map(out_rows, ks, ts, table_rows=c, bounds=_bounds(coords))
        assert launched(calls) == IF.route_table(ks, ts, False, strided)
        entries += launched(calls)
        with spied() as calls:
            got_b = transpose_table(got_t, n)
        assert launched(calls) == ["link_kmap_transpose"]
        k += 2
        if not np.array_equal(host(got_t), want_t):
            bad.append("box_neighbor_map")
        if not np.array_equal(host(got_b), want_b):
            bad.append("transpose_table")
        # the module on top
        x = la.SparseTensor(torch.zeros(n, 4, device=DEV), c, ts)
        conv = la.Conv3d(4, 4, ks, st).cuda()
        with spied() as calls:
            table, back, _, subm, out_c, s_out = conv._route(x, need_back=True)
        entries += launched(calls)
        assert launched(calls) == IF.route_conv(ks, st, ts, True), (launched(calls), IF.route_conv(ks, st, ts, True))
        assert s_out == tuple(ts[d] * st[d] for d in range(3))
        if table is None:
            assert kvol == 1 and not strided
        else:
            k += 2
            if not np.array_equal(host(out_c), want_c):
                bad.append("route.coords")
            if not np.array_equal(host(table), want_t):
                bad.append("route.table")
            if strided or kvol % 2 == 0:
                k += 1
                if back is None or not np.array_equal(host(back), want_b):
                    bad.append("route.back")
            else:
                assert back is None and subm
    row_out(test="g_kernel_maps", ks=list(ks), st=list(st), ts=list(ts), n=n, V=None, M=int(want_c.shape[0]), tiles=None,
            entries=sorted(set(entries)), compared=k, differ=bad, rule=("floor" if R.floor_rule(ks, st) else "candidates") if strided else "none")
    assert bad == [], (ks, st, ts, bad)


def test_g_transpose_with_duplicate_output_rows_and_foreign_entries():
    """Duplicated output rows handed to transpose_table: the smallest j wins; table entries >= n_in (and negative ones) are ignored;
    n_in rows past the table's reach stay -1."""
    from link_amd.index import box_neighbor_map, transpose_table
    coords = IF.kmap_frame()
    n = coords.shape[0]
    rng = np.random.default_rng(79)
    ks = (3, 2, 3)
    out = coords[rng.integers(0, n, 3 * n)]                               # every row about three times, in random order
    want_t = R.gather_table(out, R.kernel_offsets(ks), coords)
    with spied() as calls:
        got_t = box_neighbor_map(dev(out), ks, (1, 1, 1), table_rows=dev(coords))
        tables = {"dup": got_t}
        noisy = got_t.clone()
        noisy[::5, ::2] = n + 3                                           # entries >= n_in
        tables["foreign"] = noisy
    bad = [] if np.array_equal(host(got_t), want_t) else ["table"]
    k = 1
    for key, tab in tables.items():
        for n_in in (n, n - 50, n + 9):
            got = transpose_table(tab, n_in)
            k += 1
            if not np.array_equal(host(got), R.transpose_table(host(tab), n_in)):
                bad.append((key, n_in))
    row_out(test="g_transpose_duplicates", n=n, V=None, M=int(out.shape[0]), tiles=None, entries=sorted(set(launched(calls))), compared=k,
            differ=[str(b) for b in bad])
    assert bad == [], bad
    jj, kk = np.nonzero(want_t >= 0)
    pairs = want_t[jj, kk] * want_t.shape[1] + kk
    assert np.unique(pairs).size < pairs.size // 2                       # duplicates really compete for an entry: several j per (i, k)


@pytest.mark.parametrize("first", [((1, 1, 1), (2, 2, 2)), ((2, 2, 2), (3, 3, 3)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 1), (2, 2, 1))])
@pytest.mark.parametrize("shift", [(0, 0, 0), (3, 1, 5), (-7, 2, -1)])
def test_g_chained_layers(first, shift):
    """Two and three strided layers in a row (the chained case of tests/test_gpu_generalconv.py) against the reference applied
    again and again: the candidate rule of a later layer filters with the exact minimum of the earlier one's sites."""
    import link_amd as la
    coords = IF.kmap_frame().astype(np.int64)
    coords[:, :3] += np.asarray(shift) - coords[:, :3].min(0)
    x = la.SparseTensor(torch.zeros(coords.shape[0], 4, device=DEV), dev(coords), 1)
    x.cmaps.setdefault(x.stride, x.coords)
    c, s, bad, k, entries = coords, (1, 1, 1), [], 0, []
    with no_hash():
        for depth, (ks, st) in enumerate((first, ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (2, 2, 2)))):
            with torch.no_grad(), spied() as calls:
                y = la.Conv3d(4, 4, ks, st).cuda()(x)
            entries += launched(calls)
            want = R.out_sites(c, ks, st, s)
            table = x.kmaps[(s, ks, st, 1)].nbr_down
            k += 2
            if not np.array_equal(host(y.C), want):
                bad.append((depth, "coords"))
            if not np.array_equal(host(table), R.gather_table(want, R.kernel_offsets(ks, s), c)):
                bad.append((depth, "table"))
            x, c, s = y, want, tuple(s[d] * st[d] for d in range(3))
            assert y.s == s
    row_out(test="g_chained_layers", first=[list(v) for v in first], shift=list(shift), n=int(coords.shape[0]), V=None, M=int(c.shape[0]),
            tiles=None, entries=sorted(set(entries)), compared=k, differ=[str(b) for b in bad])
    assert bad == [], bad


@pytest.mark.parametrize("end", ["max", "min"])
def test_g_coordinates_at_the_ends_of_int32(end):
    """Every coordinate within 8 of INT32_MAX / INT32_MIN: taps leave the int32 range.  Each entry point gives the reference's rows
    (computed in int64) or refuses before any launch -- never other rows.  Pinned: strided_out_coords refuses with ValueError where
    index_frames.edge_refuses says so (a floored site below INT32_MIN; a candidate tap outside the range) and is exact elsewhere;
    the box table, the cubic map and the transposed table are exact everywhere (a look-up that leaves the range finds no row)."""
    from link_amd.index import box_neighbor_map, foreign_neighbor_map, strided_out_coords, transpose_table
    coords = IF.edge_frame(end)
    n = coords.shape[0]
    c = dev(coords)
    lo, hi = _bounds(coords)
    ts = (1, 1, 1)
    bad, k, refused, entries = [], 0, [], []
    with no_hash():
        for ks, st in IF.EDGE_CASES:
            out = coords.astype(np.int64)
            if any(v > 1 for v in st):
                want_c = R.out_sites(coords, ks, st, ts)
                if IF.edge_refuses(ks, st, ts, lo, hi):
                    with spied() as calls, pytest.raises(ValueError):
                        strided_out_coords(c, (lo, hi), ks, st, ts)
                    assert launched(calls) == [], calls                      # refused before any launch
                    refused.append([list(ks), list(st)])
                    out = want_c[((want_c >= IF.I32_MIN) & (want_c <= IF.I32_MAX)).all(1)]
                else:
                    assert ((want_c >= IF.I32_MIN) & (want_c <= IF.I32_MAX)).all()
                    with spied() as calls:
                        got_c, _ = strided_out_coords(c, (lo, hi), ks, st, ts)
                    entries += launched(calls)
                    k += 1
                    if not np.array_equal(host(got_c), want_c):
                        bad.append(("sites", ks, st))
                    out = want_c
            if out.shape[0] == 0:
                continue
            want_t = R.gather_table(out, R.kernel_offsets(ks, ts), coords)
            got_t = box_neighbor_map(dev(out), ks, ts, table_rows=c, bounds=(lo, hi))
            got_b = transpose_table(got_t, n)
            k += 2
            if not np.array_equal(host(got_t), want_t):
                bad.append(("table", ks, st))
            if not np.array_equal(host(got_b), R.transpose_table(want_t, n)):
                bad.append(("back", ks, st))
        for r in (2, 3):
            k += 1
            if not np.array_equal(host(foreign_neighbor_map(c, r, bounds=(lo, hi))), R.neighbor_map(coords, r)):
                bad.append(("cubic", r))
    row_out(test="g_int32_ends", end=end, n=n, V=None, M=None, tiles=None, entries=sorted(set(entries)), compared=k, refused=refused,
            differ=[str(b) for b in bad])
    assert bad == [], bad
    assert len(refused) >= 2 and k >= 12
