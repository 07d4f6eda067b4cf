"""CPU checks of the exact gate over the integer layer (tests/test_gpu_index_lattice.py): the constants tests/index_frames.py restates
are the text of csrc/index.hip / csrc/kmap.hip, its frames have the properties they were built for, its route_* cover the case lattice,
and the numpy restatement tests/index_ref.py is pinned to what the project already trusts: the C oracle (voxel_to_aux_index,
neighbor_index, conv_neighbor_table, downsample_coords, strided_conv_table) on the cubic cases, the coordinates and their order in the
g_agg_*, g_stridedconv_* and g_generalconv_* fixtures, and link_amd.get_kernel_offsets for every extent triple used.  Integers only:
every comparison is equality."""
import os
import re

import numpy as np
import pytest

import index_frames as IF
import index_ref as R
from helpers import ROOT, golden_files, load_golden
from oracle import link_oracle as O


def _src(name):
    with open(os.path.join(ROOT, "link_amd", "csrc", name)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- constants
def test_restated_constants_are_the_text_of_the_sources():
    idx, kmap = _src("index.hip"), _src("kmap.hip")
    items = int(re.search(r"#define LINK_SCAN_ITEMS (\d+)", idx).group(1))
    threads = int(re.search(r"constexpr int SCAN_THREADS = (\d+);", idx).group(1))
    assert re.search(r"constexpr int SCAN_TILE = SCAN_THREADS \* SCAN_ITEMS;", idx)
    assert re.search(r"constexpr int SCAN_ITEMS = LINK_SCAN_ITEMS;", idx)
    assert re.search(r"constexpr int VSCAN_ITEMS = SCAN_ITEMS;", idx) and re.search(r"constexpr int VSCAN_TILE = SCAN_THREADS \* VSCAN_ITEMS;", idx)
    assert threads * items == IF.SCAN_TILE and items == 8                # (8: the V = 7, 8, 9 cases stand on one thread's items)
    assert int(re.search(r"constexpr int VSCAN_RESIDENT = (\d+);", idx).group(1)) == IF.VSCAN_RESIDENT
    assert int(re.search(r"constexpr int SORT_MAX_SEG = (\d+);", idx).group(1)) == IF.SORT_MAX_SEG
    assert int(re.search(r"constexpr int KMAP_MAX_EXTENT = (\d+);", kmap).group(1)) == IF.KMAP_MAX_EXTENT
    # the look-back window: one tile per lane of a 64-wide wave, both scans
    assert idx.count("look -= 64;") == 2 and idx.count("int64_t t = look - lane;") == 2 and IF.LOOKBACK == 64
    assert "tiles <= VSCAN_RESIDENT" in idx


# --------------------------------------------------------------------------------------------------------------------- a
def test_scan_lattice_covers_what_the_issue_lists():
    ids = [IF.scan_id(c) for c in IF.SCAN_CASES]
    assert len(set(ids)) == len(ids)
    line = {c["dim"][0] for c in IF.SCAN_CASES if c["dim"][1:] == (1, 1, 1) and c["s"] == 1}
    assert line == set(IF.LINE_V) == {1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 131072, 131073, 266245}
    assert [int(np.prod(d)) for d in IF.FACTORED] == [2048, 2048, 4097]
    for v in IF.LINE_V + (2048, 4097):
        occs = {c["occ"] for c in IF.SCAN_CASES if int(np.prod(c["dim"])) == v and c["s"] == 1}
        # every occupancy that is a different set of cells at this V (one tile has no boundary; at V = 1 all of them coincide)
        want = {o: tuple(IF.occupancy(v, o)) for o in IF.OCCUPANCIES if IF.occupancy(v, o).size}
        assert len({want[o] for o in occs}) == len(set(want.values())), v
    assert {c["s"] for c in IF.SCAN_CASES} == {1, 3, 7} and any(c["dup"] for c in IF.SCAN_CASES)
    assert IF.tiles_of(130 * 2048 + 5) == 131 > 2 * IF.LOOKBACK and IF.tiles_of(64 * 2048) == 64 and IF.tiles_of(64 * 2048 + 1) == 65
    assert all(v < 0 for v in IF.LO_NEG)


def test_occupancies_are_what_they_say():
    v = 3 * 2048 + 5
    e = IF.occupancy(v, "edges")
    assert e.tolist() == [2047, 2048, 4095, 4096, 6143, 6144]
    assert IF.occupancy(v, "head_tile").tolist() == list(range(2048)) and IF.occupancy(v, "tail_tile").tolist() == list(range(6144, v))
    assert IF.occupancy(v, "alternate").tolist() == list(range(0, v, 2))
    assert IF.occupancy(v, "first").tolist() == [0] and IF.occupancy(v, "last").tolist() == [v - 1] and IF.occupancy(v, "full").size == v


@pytest.mark.parametrize("case", [c for c in IF.SCAN_CASES if int(np.prod(c["dim"])) <= 4097], ids=IF.scan_id)
def test_scan_frames_occupy_the_cells_they_claim(case):
    coords, grid, cells, per = IF.scan_case(case)
    assert coords.dtype == np.int32 and coords.shape[0] == per.sum()
    ref = R.block_index(coords, case["s"], "cell", grid)
    assert ref["status"] == 0 and ref["m"] == cells.size
    assert np.array_equal(np.flatnonzero(ref["cell_blk"]), cells) and np.array_equal(ref["counts"], per)
    assert np.array_equal(R.cells_of(ref["blk_coords"], grid), cells)          # np.unique's row order IS ascending cell order
    assert np.array_equal(R.rows_of_cells(cells, grid), ref["blk_coords"])
    if case["dup"]:
        assert np.unique(coords, axis=0).shape[0] < coords.shape[0] and per.max() == 3
    if case["s"] > 1 and case["occ"] == "full" and int(np.prod(case["dim"])) > 8:
        assert coords[:, :3].min() < 0 < coords[:, :3].max()                   # both sides of zero: floor division, not truncation
        assert not np.array_equal(R.block_rows(coords, case["s"])[:, :3], np.trunc(coords[:, :3] / case["s"]))


def test_largest_scan_frame():
    case = [c for c in IF.SCAN_CASES if c["dim"][0] == 130 * 2048 + 5 and c["occ"] == "edges"][0]
    coords, grid, cells, per = IF.scan_case(case)
    assert cells.size == 2 * 130 and coords.shape[0] == 260
    ref = R.block_index(coords, 1, "cell", grid)
    assert np.array_equal(np.flatnonzero(ref["cell_blk"]), cells)


# --------------------------------------------------------------------------------------------------------------------- b
def test_order_frame_and_its_orders():
    vox, grid, sizes = IF.order_frame()
    n = vox.shape[0]
    assert np.unique(vox, axis=0).shape[0] == n and int(np.prod(grid[1])) == 4097
    ref = R.block_index(vox, IF.ORDER_S, "cell", grid)
    assert ref["status"] == 0 and dict(zip(R.cells_of(ref["blk_coords"], grid).tolist(), ref["counts"].tolist())) == sizes
    cnt = sorted(sizes.values())
    for k in IF.EXACT_BLOCKS:
        assert cnt.count(k) >= 1, k
    assert cnt[-1] == IF.SORT_MAX_SEG and cnt[-2] <= 70
    ordinary = [k for c, k in sizes.items() if c % 10 or c > 90]
    assert len(ordinary) >= 90 and min(ordinary) >= 3 and max(ordinary) <= 70
    assert {0, 2047, 2048, 4095, 4096} <= set(sizes)
    cell_of = lambda c: R.cells_of(R.block_rows(c, IF.ORDER_S), grid)
    got = {o: IF.orders(vox, sizes, o) for o in IF.ORDERS}
    for o, c in got.items():
        assert c.shape == (n, 4) and np.array_equal(np.unique(c, axis=0), np.unique(vox, axis=0)), o
    s = cell_of(got["sorted"])
    assert np.all(np.diff(s) >= 0)
    waves = s[: n // 64 * 64].reshape(-1, 64)
    assert (waves.min(1) == waves.max(1)).sum() >= 128                     # whole waves share a cell (the 8192-block alone: 127)
    assert np.array_equal(cell_of(got["reversed"]), s[::-1])
    rr = cell_of(got["roundrobin"])[: 3 * 64].reshape(-1, 64)
    assert all(np.unique(w).size == 64 for w in rr)                        # every lane of those waves alone in its cell
    rnd = cell_of(got["random"])
    assert (np.diff(rnd) != 0).mean() > 0.3
    # unaligned heads and tails: segment starts of every residue modulo 4 (the 16-byte pieces of k_sort_seg)
    assert set((ref["blk_start"][:-1] % 4).tolist()) == {0, 1, 2, 3}
    big = IF.order_frame(big=IF.SORT_MAX_SEG + 1)
    assert max(big[2].values()) == IF.SORT_MAX_SEG + 1 and big[0].shape[0] == n + 1


# --------------------------------------------------------------------------------------------------------------------- c
def test_outside_frame_has_one_voxel_beyond_each_face():
    inside, grid, beyond, at = IF.outside_frame()
    assert R.block_index(inside, IF.OUT_S, "cell", grid)["status"] == 0 and len(IF.FACES) == 8 == beyond.shape[0]
    lo, dim = grid
    for (axis, side), vox in zip(IF.FACES, beyond):
        u = R.block_rows(vox[None], IF.OUT_S)[0] - lo
        out = [(u[a] < 0, u[a] >= dim[a]) for a in range(4)]
        assert out[axis] == ((side == "lo"), (side == "hi")) and not any(any(o) for a, o in enumerate(out) if a != axis)
        # the NEAREST voxel beyond the face: one step back on that axis is inside
        back = vox.astype(np.int64).copy()
        back[axis] += 1 if side == "lo" else -1
        assert R.cells_of(R.block_rows(back[None], IF.OUT_S), grid)[0] >= 0
    coords, ids = IF.with_outside(inside, beyond, at, tuple(range(8)))
    ref = R.block_index(coords, IF.OUT_S, "cell", grid)
    assert np.array_equal(np.flatnonzero(ref["vox_blk"] < 0), ids) and ids.tolist() == sorted(at) and ref["status"] == 1
    assert ref["nvalid"] == coords.shape[0] - 8 == ref["blk_start"][-1] == ref["perm"].size
    keep = np.setdiff1d(np.arange(coords.shape[0]), ids)
    clean = R.block_index(coords[keep], IF.OUT_S, "cell", grid)
    assert np.array_equal(ref["perm"], keep[clean["perm"]]) and np.array_equal(ref["blk_coords"], clean["blk_coords"])


# --------------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("n", IF.FIRST_N)
def test_first_frames(n):
    c = IF.first_frame(n)
    lo, hi = IF.first_bounds()
    assert c.shape == (n, 4) and np.unique(c, axis=0).shape[0] == n
    assert (c >= np.asarray(lo)).all() and (c <= np.asarray(hi)).all()
    grid = R.grid_of(lo, hi, IF.FIRST_S)
    first, cell = R.block_index(c, IF.FIRST_S, "first", grid), R.block_index(c, IF.FIRST_S, "cell", grid)
    assert first["status"] == 0 and first["m"] == cell["m"]
    # the two numberings: the same blocks, first-voxel order ranks them by their smallest voxel id
    order = np.lexsort(first["blk_coords"].T[::-1])
    assert np.array_equal(first["blk_coords"][order], cell["blk_coords"]) and np.array_equal(first["counts"][order], cell["counts"])
    smallest = first["perm"][first["blk_start"][:-1]]
    assert np.all(np.diff(smallest) > 0) and np.array_equal(first["blk_coords"][first["vox_blk"]], cell["blk_coords"][cell["vox_blk"]])
    if n > IF.FIRST_MARK[1] + 2:
        for mark in IF.FIRST_MARK:
            b = first["vox_blk"][mark]
            assert smallest[b] == mark and first["counts"][b] == 2, mark      # first voxel of its cell, and a later member
    assert IF.tiles_of(n) == (n + 2047) // 2048


def test_first_big_and_sequence():
    assert IF.tiles_of(IF.BIG_N) == IF.VSCAN_RESIDENT + 1 and IF.BIG_N == 2 ** 21 + 1 and (IF.BIG_BOX, IF.BIG_S) == (600, 5)
    seq = dict(IF.first_sequence())
    assert list(seq) == ["A", "subset", "disjoint", "superset", "few", "empty", "dropped", "A_again"]
    lo, hi = IF.first_bounds()
    grid = R.grid_of(lo, hi, IF.SEQ_S)
    cells = {k: set(np.flatnonzero(R.block_index(v, IF.SEQ_S, "first", grid)["cell_blk"]).tolist()) for k, v in seq.items()}
    assert cells["subset"] < cells["A"] and not (cells["disjoint"] & cells["A"]) and cells["superset"] > cells["A"]
    assert seq["few"].shape[0] < len(cells["superset"]) and seq["empty"].shape[0] == 0 and np.array_equal(seq["A"], seq["A_again"])
    d = R.block_index(seq["dropped"], IF.SEQ_S, "first", grid)
    assert d["status"] == 1 and d["nvalid"] == seq["dropped"].shape[0] - 1
    assert all(R.block_index(v, IF.SEQ_S, "first", grid)["status"] == 0 for k, v in seq.items() if k != "dropped")


# ------------------------------------------------------------------------------------------------------------------ e, f
def test_cells_frame():
    rows, grid, n_in, n_out = IF.cells_frame()
    ref = R.unique_cells(rows, grid)
    assert ref["m"] == 400 and ref["nvalid"] == n_in == 2000 and rows.shape[0] == n_in + n_out
    assert 1 - ref["m"] / ref["nvalid"] >= 0.8                              # 80 % duplicates
    cell = R.cells_of(rows, grid)
    assert (cell < 0).sum() == n_out == 8 + 37
    assert (rows == np.array([IF.CELLS_LO[0] - 1, 0, 0, 0])).all(1).sum() == 37
    assert np.array_equal(ref["blk_coords"], np.unique(rows[cell >= 0], axis=0)) and ref["counts"].sum() == n_in


def test_neighbor_and_table_frames():
    fr = IF.nbr_frames()
    assert fr["solid"].shape[0] == 7 * 6 * 8
    for r in IF.NBR_R:
        for step in IF.NBR_STEP:
            for tr in (False, True):
                assert np.array_equal(R.neighbor_map(fr["solid"], r, step, tr), IF.solid_neighbor(fr["solid"], (-3, -2, -4), (7, 6, 8), r, step, tr))
    for axis, name in enumerate(("thin_x", "thin_y", "thin_z")):
        assert np.unique(fr[name][:, axis]).size == 1 and fr[name].shape[0] == 144
    b = fr["batch"]
    assert set(b[:, 3].tolist()) == {0, 1} and b.shape[0] == 216
    assert np.unique(b[:, :3], axis=0).shape[0] == 216                     # item 1 holds exactly the cells item 0 does not
    nb = R.neighbor_map(b, 3)
    hit = nb[nb >= 0]
    assert (b[np.repeat(np.arange(216), 27)[nb.reshape(-1) >= 0], 3] == b[hit, 3]).all() and (nb < 0).sum() > 216 * 27 // 3
    rows, grid = IF.table_frame()
    u, cnt = np.unique(rows, axis=0, return_counts=True)
    assert sorted(cnt.tolist())[-3:] == list(IF.TABLE_REPEATS) and u.shape[0] == 500
    tab, outside = R.cell_table(rows, grid)
    assert not outside and (tab > 0).sum() == 500
    for i in np.flatnonzero(tab):
        first = np.flatnonzero((rows == R.rows_of_cells(np.array([i]), grid)[0]).all(1))[0]
        assert tab[i] == first + 1


# --------------------------------------------------------------------------------------------------------------------- g
def test_kmap_frame_and_lattice():
    c = IF.kmap_frame()
    assert 550 <= c.shape[0] <= 640 and np.unique(c, axis=0).shape[0] == c.shape[0]
    assert c[:, :3].min() >= -40 and c[:, :3].max() < 40 and set(c[:, 3].tolist()) == {0, 1}
    assert {tuple(r) for r in (c[:, :3] % 2).tolist()} == {(a, b, d) for a in (0, 1) for b in (0, 1) for d in (0, 1)}
    assert not np.array_equal(c, np.unique(c, axis=0))                     # shuffled
    xs = {(ks[0], st[0], ts[0]) for ks, st, ts in IF.KMAP_CASES if ks[1:] == (1, 1) and st[1:] == (1, 1)}
    assert {(k, s, t) for k in range(1, 8) for s in range(1, 5) for t in (1, 2)} <= xs
    assert any(k < s for k, s, _ in xs) and any(k == s for k, s, _ in xs) and any(k > s > 1 for k, s, _ in xs)
    geo = {(ks, st) for ks, st, _ in IF.KMAP_CASES}
    assert {((7, 7, 7), (1, 1, 1)), ((2, 3, 4), (1, 1, 1)), ((4, 3, 2), (2, 3, 1))} <= geo and set(IF.GEOMETRIES) <= geo
    rules = {R.floor_rule(ks, st) for ks, st, _ in IF.KMAP_CASES if any(v > 1 for v in st)}
    assert rules == {True, False}
    assert {(ks[0] * ks[1] * ks[2]) % 2 for ks, _, _ in IF.KMAP_CASES} == {0, 1} and max(ks[0] * ks[1] * ks[2] for ks, _, _ in IF.KMAP_CASES) == 343


def test_candidate_rows_off_lattice_and_below_minimum():
    """the share of candidate rows the two filters remove, per candidate-rule case: both filters bite somewhere"""
    c = IF.kmap_frame()
    off = below = 0
    for ks, st, ts in IF.KMAP_CASES:
        if not any(v > 1 for v in st) or R.floor_rule(ks, st):
            continue
        frame = IF.on_lattice(c, ts) if ts != (1, 1, 1) else c
        rows, on, above = R.candidate_rows(frame, ks, st, ts)
        sites = R.candidate_sites(frame, ks, st, ts)
        assert rows.shape[0] == frame.shape[0] * ks[0] * ks[1] * ks[2] and 0 < sites.shape[0] <= (on & above).sum()
        assert (~on).mean() > 0.3                                          # most taps miss the lattice
        off += int((~on).sum())
        below += int((on & ~above).sum())
        ss = np.asarray([st[d] * ts[d] for d in range(3)])
        assert (sites[:, :3] % ss == 0).all() and (sites[:, :3] >= frame[:, :3].min(0)).all()
    assert off > 0 and below > 0


def test_routes():
    assert IF.route_sites((3, 3, 3), (2, 2, 2), (1, 1, 1)) == ["link_kmap_candidate_count", "link_kmap_out_candidates", "link_index_cells"]
    assert IF.route_sites((2, 2, 2), (2, 2, 2), (1, 1, 1)) == ["link_index_cells"] == IF.route_sites((1, 1, 1), (1, 1, 1), (1, 1, 1))
    assert IF.route_table((3, 3, 3), (1, 1, 1), True, False)[1] == "link_neighbor_map"
    assert IF.route_table((3, 1, 3), (1, 1, 1), False, False) == ["link_cell_table_build", "link_kmap_box_table", "link_cell_table_clear"]
    assert IF.is_cubic((3, 3, 3), (1, 1, 1), (2, 2, 2)) and not IF.is_cubic((3, 3, 3), (1, 1, 1), (2, 2, 1)) and not IF.is_cubic((3, 3, 3), (2, 2, 2), (1, 1, 1))
    assert IF.is_cubic((2, 2, 2), (2, 2, 2), (1, 1, 1)) and not IF.is_cubic((2, 2, 2), (2, 2, 2), (2, 2, 1))
    assert IF.route_conv((1, 1, 1), (1, 1, 1), (1, 1, 1), True) == []
    assert IF.route_conv((2, 2, 2), (1, 1, 1), (1, 1, 1), True)[-1] == "link_kmap_transpose" != IF.route_conv((3, 3, 3), (1, 1, 1), (1, 1, 1), True)[-1]
    kinds = {tuple(IF.route_conv(ks, st, ts, True)) for ks, st, ts in IF.KMAP_CASES}
    assert len(kinds) >= 6
    # written from the dispatch code: the words it keys on are still there
    with open(os.path.join(ROOT, "link_amd", "elk.py")) as f:
        elk = f.read()
    assert "self.kernel_size == (2, 2, 2) and self.stride == (2, 2, 2) and len(set(x.s)) == 1" in elk
    assert "cubic = len(set(kernel_size)) == 1 and len(set(x.s)) == 1" in elk
    with open(os.path.join(ROOT, "link_amd", "index.py")) as f:
        assert "if all(int(stride[k]) in (1, int(kernel[k])) for k in range(3)):" in f.read()


# --------------------------------------------------------------------------------------- index_ref against oracle and fixtures
def _oracle_frames():
    rng = np.random.default_rng(5)
    a = rng.integers(-30, 30, (1500, 4)).astype(np.int32)
    a[:, 3] = rng.integers(0, 2, 1500)
    return {"both_signs": np.unique(a, axis=0)[rng.permutation(np.unique(a, axis=0).shape[0])], "kmap": IF.kmap_frame(),
            "first": IF.first_frame(2049)}


@pytest.mark.parametrize("name", ["both_signs", "kmap", "first"])
def test_index_ref_against_the_oracle(name):
    coords = _oracle_frames()[name]
    rows = R.block_rows(np.concatenate([coords, coords[::3]], 0), 3)
    for a, b in zip(R.unique_rows(rows), np.unique(rows, axis=0, return_index=True, return_inverse=True, return_counts=True)):
        assert np.array_equal(a, b.reshape(a.shape))                         # the keyed unique IS np.unique(axis=0)
    for s in (1, 3, 7):
        small_c, idx, cnt = O.voxel_to_aux_index(coords, s)
        ref = R.block_index(coords, s, "cell")
        assert np.array_equal(ref["blk_coords"], small_c) and np.array_equal(ref["vox_blk"], idx) and np.array_equal(ref["counts"], cnt)
        for r in (1, 2, 3, 4, 5):
            assert np.array_equal(R.kernel_offsets(r), O.get_kernel_offsets(r)), r
            if small_c.shape[0] * r ** 3 < 200000:
                assert np.array_equal(R.neighbor_map(small_c, r), O.neighbor_index(small_c, r)), (s, r)
    single = coords[coords[:, 3] == 0]                                      # (the oracle's table builders follow the reference's CPU hash)
    for ts in (1, 2):
        c = np.unique(single // np.array([ts, ts, ts, 1]) * np.array([ts, ts, ts, 1]), axis=0).astype(np.int32)
        for k in (2, 3):
            assert np.array_equal(R.gather_table(c, R.kernel_offsets(k, ts), c), O.conv_neighbor_table(c, k, ts)), (ts, k)
        down = O.downsample_coords(c, 2, ts)
        assert np.array_equal(R.out_sites(c, (2, 2, 2), (2, 2, 2), (ts,) * 3), down) and np.array_equal(R.floor_sites(c, (2, 2, 2), (ts,) * 3), down)
        assert np.array_equal(R.gather_table(down, R.kernel_offsets(2, ts), c), O.strided_conv_table(c, down, 2, ts))


@pytest.mark.parametrize("name", golden_files("g_agg_*.npz"))
def test_index_ref_against_the_aggregation_fixtures(name):
    g = load_golden(name)
    s, r = g["meta"]["s"], g["meta"]["r"]
    ref = R.block_index(g["coords"], s, "cell")
    assert np.array_equal(ref["blk_coords"], g["small_c"]) and np.array_equal(ref["vox_blk"], g["idx_query"]) and np.array_equal(ref["counts"], g["counts"])
    if not g["meta"].get("multi_batch"):                                    # (two batch items: the reference's CPU neighbour hash is defective)
        assert np.array_equal(R.neighbor_map(g["small_c"], r), g["nbr"])


@pytest.mark.parametrize("name", golden_files("g_stridedconv_*.npz") + golden_files("g_generalconv_*.npz"))
def test_index_ref_against_the_convolution_fixtures(name):
    g = load_golden(name)
    if "layers" not in g["meta"]:
        assert np.array_equal(R.out_sites(g["coords"], (2, 2, 2), (2, 2, 2), (1, 1, 1)), g["x2_C"]) and np.array_equal(g["x4_C"], g["coords"])
        return
    c, stack = g["coords"].astype(np.int64), []
    for i, lay in enumerate(g["meta"]["layers"]):
        ks, st, ts = tuple(lay["kernel_size"]), tuple(lay["stride"]), tuple(lay["in_stride"])
        if f"offs{i}" in g:
            offs = R.kernel_offsets(ks, ts if not lay["transposed"] else lay["out_stride"])
            assert np.array_equal(offs, g[f"offs{i}"]) or lay["transposed"], (name, i)
        if lay["transposed"]:
            c = stack.pop() if any(v > 1 for v in st) else c
        else:
            if any(v > 1 for v in st):
                stack.append(c)
                c = R.out_sites(c, ks, st, ts)
        assert np.array_equal(c, g[f"x{i}_C"]), (name, i)
        assert tuple(lay["out_stride"]) == (tuple(ts[d] // st[d] for d in range(3)) if lay["transposed"] else tuple(ts[d] * st[d] for d in range(3)))


def test_kernel_offsets_against_the_package_for_every_extent_triple_used():
    from link_amd import get_kernel_offsets
    seen = set()
    for ks, st, ts in IF.KMAP_CASES + [((r, r, r), (1, 1, 1), (t, t, t)) for r in IF.NBR_R for t in IF.NBR_STEP] + [((3, 2, 3), (1, 1, 1), (1, 1, 1))]:
        if (ks, ts) in seen:
            continue
        seen.add((ks, ts))
        assert np.array_equal(R.kernel_offsets(ks, ts), get_kernel_offsets(ks, stride=ts).numpy()), (ks, ts)
    assert len(seen) >= 50
    assert R.taps(1) == [0] and R.taps(2) == [0, 1] and R.taps(3) == [-1, 0, 1] and R.taps(4) == [-1, 0, 1, 2] and R.taps(7) == [-3, -2, -1, 0, 1, 2, 3]


def test_transpose_reference_smallest_j_wins():
    t = np.array([[0, 2], [0, -1], [5, 2], [1, 0]])
    back = R.transpose_table(t, 3)
    assert back.tolist() == [[0, 3], [3, -1], [-1, 0]]


@pytest.mark.parametrize("end", ["max", "min"])
def test_edge_frames_sit_at_the_ends_of_int32(end):
    c = IF.edge_frame(end)
    assert c.dtype == np.int32 and 280 <= c.shape[0] <= 300 and np.unique(c, axis=0).shape[0] == c.shape[0] and set(c[:, 3].tolist()) == {0, 1}
    ext = IF.I32_MAX if end == "max" else IF.I32_MIN
    assert (np.abs(c[:, :3].astype(np.int64) - ext) <= 8).all() and (c[:, :3] == ext).any(0).all()      # the extreme on every axis
    lo, hi = tuple(int(v) for v in c.min(0)), tuple(int(v) for v in c.max(0))
    verdicts = {}
    for ks, st in IF.EDGE_CASES:
        if not any(v > 1 for v in st):
            continue
        want = R.out_sites(c, ks, st, (1, 1, 1))
        fits = bool(((want >= IF.I32_MIN) & (want <= IF.I32_MAX)).all())
        verdicts[(ks, st)] = IF.edge_refuses(ks, st, (1, 1, 1), lo, hi)
        assert fits or verdicts[(ks, st)], (ks, st)                         # rows that cannot be written down are always refused
    assert True in verdicts.values() and (end == "min" or False in verdicts.values())
    assert {R.floor_rule(ks, st) for ks, st in verdicts} == {True, False}
