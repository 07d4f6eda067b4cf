"""Frames, the case lattice and the route restatement of the exact gate over the integer layer: csrc/index.hip (both numberings of
the block index, link_index_cells, the neighbour map, the cell table) and csrc/kmap.hip (candidate sites, box table, transposed
table), with link_amd/index.py on top (tests/test_gpu_index_lattice.py; every claim made here is checked on the CPU by
tests/test_cpu_index_frames.py).  numpy only: no link_amd, no GPU.

Constants restated from the sources (pinned to their text by the CPU test, so that a change there fails loudly instead of moving
the edges away from the frames):
  SCAN_TILE = 256 threads x LINK_SCAN_ITEMS 8 = 2048 cells (voxels) per workgroup of k_cell_scan (k_vox_scan);
  LOOKBACK = 64: tiles one look-back step of a scan reads (one per lane of wave 0);
  VSCAN_RESIDENT = 1024: k_vox_scan<false> up to that many tiles, k_vox_scan<true> (ticket order) above;
  SORT_MAX_SEG = 8192: k_sort_seg orders a block's ids up to that length, a longer segment stays in atomic-rank order;
  KMAP_MAX_EXTENT = 7: largest per-axis extent of the kernel-map builders.

What each frame exists for:
  a  scan_case(...)   one voxel (or 1-3 duplicates) in chosen cells of a grid of V cells, V on both sides of 1, 8 (one thread's
                      items: the uint4 body against the scalar tail), 1 and 2 tiles, the 64-tile look-back window, and 130 tiles + 5
                      (more than two windows).  Occupancy puts the non-zero counters where a scan can lose them: everywhere, only the
                      first / last cell, both sides of every tile boundary, every other cell, one full tile before / after empty
                      ones.  Factorised grids with a negative lo on every axis (batch too) exercise the decode of blk_coords.
  b  order_frame()    V = 4097 along x, s = 21: 3..70 voxels in each of 96 cells (cells 0, 2047, 2048, 4095, 4096 among them) and
                      blocks of exactly 1, 2, 3, 4, 5, 63, 64, 65 and 8192 voxels (the unaligned head / tail of k_sort_seg's 16-byte
                      pieces, SORT_MAX_SEG on the nose); orders(): sorted by cell (whole waves share a cell: one atomic per wave in
                      k_cell_count), reversed, random, round-robin (every lane of a wave alone in its cell).  order_frame(big=8193):
                      the same with a block of 8193.
  c  outside_frame()  a 6 x 5 x 4 x 3 grid (s = 3, lo negative) and one voxel beyond each of its eight faces.
  d  first_frame(n)   n unique voxels (s = 3) in which ids 2047 and 2048 -- the last of tile 0, the first of tile 1 -- are each the
                      first voxel of their cell, with later members; first_big(): 2^21 + 1 voxels = 1025 tiles, the one size past
                      VSCAN_RESIDENT; first_sequence(): frames run one after another on one set of tables.
  e  cells_frame()    candidate-like rows (b, x, y, z), about 80 % duplicates, with rows beyond every face and the bad_b row.
  f  nbr_frames()     solid box (closed form), one-cell-thick boxes, two batch items adjacent in memory; table_frame(): rows
                      repeated 2, 64 and 1000 times.
  g  kmap_frame()     about 600 unique voxels in [-40, 40)^3 x 2 with every residue modulo 2 on every axis, shuffled; KMAP_CASES:
                      the per-axis lattice on x (k 1..7 x stride 1..4 x tensor stride 1, 2) and the anisotropic geometries;
                      edge_frame(): 300 voxels within 8 of INT32_MAX / INT32_MIN, where taps leave the int32 range.

route_sites / route_table restate which entry points the host code calls (link_amd/index.py: strided_out_coords, unique_cells,
foreign_neighbor_map, box_neighbor_map, transpose_table; link_amd/elk.py: Conv3d._route, _strided_map, _general_map,
neighbor_table_of), written from that code, not from what a run did."""
import numpy as np

import index_ref as R

SCAN_TILE = 2048
LOOKBACK = 64
VSCAN_RESIDENT = 1024
SORT_MAX_SEG = 8192
KMAP_MAX_EXTENT = 7


def tiles_of(v):
    return (v + SCAN_TILE - 1) // SCAN_TILE


def _shuffled(coords, rng):
    return np.ascontiguousarray(coords[rng.permutation(coords.shape[0])].astype(np.int32))


def voxels_in_cells(cells, grid, s, rng, per_cell=1):
    """per_cell voxels (duplicates when per_cell > s^3 is not the point: drawn with replacement) inside each block of `cells`"""
    rows = R.rows_of_cells(np.asarray(cells, np.int64), grid)
    rows = np.repeat(rows, per_cell, 0) if np.isscalar(per_cell) else np.repeat(rows, np.asarray(per_cell), 0)
    c = rows.copy()
    c[:, :3] = rows[:, :3] * s + rng.integers(0, s, (rows.shape[0], 3))
    return c


# ----------------------------------------------------------------------------------------------------------------- a: scan
LINE_V = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 64 * 2048, 64 * 2048 + 1, 130 * 2048 + 5)
LO_NEG = (-5, -3, -2, -1)
FACTORED = ((16, 16, 8, 1), (8, 8, 8, 4), (17, 241, 1, 1))          # 2048, 2048, 4097 cells
OCCUPANCIES = ("full", "first", "last", "edges", "alternate", "head_tile", "tail_tile")


def occupancy(v, occ):
    """the occupied cells (ascending) of a grid of v cells"""
    if occ == "full":
        return np.arange(v)
    if occ == "first":
        return np.array([0])
    if occ == "last":
        return np.array([v - 1])
    if occ == "edges":                                              # both sides of every tile boundary
        b = np.arange(SCAN_TILE, v, SCAN_TILE)
        return np.sort(np.concatenate([b - 1, b]))
    if occ == "alternate":
        return np.arange(0, v, 2)
    if occ == "head_tile":                                          # one occupied tile followed by empty ones
        return np.arange(min(v, SCAN_TILE))
    if occ == "tail_tile":                                          # empty tiles followed by the last (partial) tile
        return np.arange((tiles_of(v) - 1) * SCAN_TILE, v)
    raise ValueError(occ)


def _scan_cases():
    cases, seen = [], set()

    def add(dim, lo, occ, s, dup):
        v = int(np.prod(dim))
        cells = occupancy(v, occ)
        key = (dim, s, dup, cells.size, int(cells[0]) if cells.size else -1, int(cells[-1]) if cells.size else -1,
               int(cells[: 4096].sum()))
        if cells.size == 0 or key in seen:                          # no tile boundary in one tile; 'first' = 'full' at V = 1 ...
            return
        seen.add(key)
        cases.append(dict(dim=dim, lo=lo, occ=occ, s=s, dup=dup))
    for v in LINE_V:
        for occ in OCCUPANCIES:
            add((v, 1, 1, 1), (-(v // 3), 2, -1, 1), occ, 1, False)
    for dim in FACTORED:
        for occ in OCCUPANCIES:
            add(dim, LO_NEG, occ, 1, False)
    for dim in ((9, 1, 1, 1), (2049, 1, 1, 1)) + FACTORED:          # block edges 3 and 7, coordinates on both sides of zero
        for s in (3, 7):
            for occ in ("full", "alternate", "edges"):
                add(dim, LO_NEG, occ, s, False)
    for dim in ((2049, 1, 1, 1), (8, 8, 8, 4)):                     # duplicate voxels: 1 to 3 copies of a voxel
        for occ in ("full", "alternate"):
            add(dim, LO_NEG, occ, 3, True)
    return cases


SCAN_CASES = _scan_cases()


def scan_id(c):
    return "x".join(str(d) for d in c["dim"]) + f"-{c['occ']}-s{c['s']}" + ("-dup" if c["dup"] else "")


def scan_case(c):
    """(coords int32 [n, 4] shuffled, grid (lo, dim) in block units, occupied cells ascending, voxels per occupied cell)"""
    rng = np.random.default_rng([int(d) for d in c["dim"]] + [OCCUPANCIES.index(c["occ"]), c["s"], int(c["dup"])])
    grid = (np.asarray(c["lo"], np.int64), np.asarray(c["dim"], np.int64))
    cells = occupancy(int(np.prod(c["dim"])), c["occ"])
    vox = voxels_in_cells(cells, grid, c["s"], rng)
    per = np.ones(cells.size, np.int64)
    if c["dup"]:
        per = rng.integers(1, 4, cells.size)
        vox = np.repeat(vox, per, 0)
    return _shuffled(vox, rng), grid, cells, per


# ---------------------------------------------------------------------------------------------------------------- b: order
ORDER_S = 21
ORDER_DIM, ORDER_LO = (4097, 1, 1, 1), (-2000, 0, 0, 0)
EXACT_BLOCKS = (1, 2, 3, 4, 5, 63, 64, 65, SORT_MAX_SEG)
ORDERS = ("sorted", "reversed", "random", "roundrobin")


def _block_voxels(cell, k, grid, s, rng):
    """k UNIQUE voxels of the block at `cell`: the first k of a random order of its s^3 positions"""
    assert k <= s ** 3
    row = R.rows_of_cells(np.array([cell]), grid)[0]
    pos = rng.permutation(s ** 3)[:k]
    c = np.stack([pos // (s * s), (pos // s) % s, pos % s], 1) + row[:3] * s
    return np.concatenate([c, np.full((k, 1), row[3])], 1)


def order_frame(big=SORT_MAX_SEG):
    """(coords int64 [n, 4] grouped by cell ascending, grid, {cell: count}).  The exact blocks sit at cells 10, 20, ...; the last
    one has `big` voxels."""
    rng = np.random.default_rng(41)
    grid = (np.asarray(ORDER_LO, np.int64), np.asarray(ORDER_DIM, np.int64))
    sizes = {}
    for i, k in enumerate(EXACT_BLOCKS[:-1] + (big,)):
        sizes[10 * (i + 1)] = k
    ordinary = [0, 2047, 2048, 4095, 4096] + [int(c) for c in rng.choice(np.arange(100, 4000), 120, replace=False)]
    for c in ordinary:
        if c not in sizes and len(sizes) < 96 + len(EXACT_BLOCKS):
            sizes[c] = int(rng.integers(3, 71))
    sizes = dict(sorted(sizes.items()))
    vox = np.concatenate([_block_voxels(c, k, grid, ORDER_S, rng) for c, k in sizes.items()], 0)
    return vox, grid, sizes


def orders(vox, sizes, order):
    """the frame's rows (grouped by cell) in one of ORDERS, as int32"""
    n = vox.shape[0]
    if order == "sorted":
        idx = np.arange(n)
    elif order == "reversed":
        idx = np.arange(n)[::-1]
    elif order == "random":
        idx = np.random.default_rng(43).permutation(n)
    elif order == "roundrobin":                                     # by (rank inside the cell, cell): neighbours differ in cell
        cnt = np.fromiter(sizes.values(), np.int64)
        rank = np.concatenate([np.arange(k) for k in cnt])
        cell = np.repeat(np.arange(cnt.size), cnt)
        idx = np.lexsort((cell, rank))
    else:
        raise ValueError(order)
    return np.ascontiguousarray(vox[idx].astype(np.int32))


# -------------------------------------------------------------------------------------------------------------- c: outside
OUT_S = 3
OUT_DIM, OUT_LO = (6, 5, 4, 3), (-2, -3, -1, -1)
FACES = tuple((axis, side) for axis in range(4) for side in ("lo", "hi"))


def outside_frame():
    """(coords int32 [n, 4] all inside, grid, eight voxels: one beyond each face, the ids they are inserted at)"""
    rng = np.random.default_rng(47)
    grid = (np.asarray(OUT_LO, np.int64), np.asarray(OUT_DIM, np.int64))
    v = int(np.prod(OUT_DIM))
    cells = np.sort(rng.choice(v, 150, replace=False))
    inside = _shuffled(voxels_in_cells(cells, grid, OUT_S, rng, per_cell=rng.integers(1, 5, cells.size)), rng)
    beyond = []
    for axis, side in FACES:
        row = R.rows_of_cells(np.array([int(rng.integers(v))]), grid)[0]
        row[axis] = OUT_LO[axis] - 1 if side == "lo" else OUT_LO[axis] + OUT_DIM[axis]
        vox = row.copy()
        vox[:3] = row[:3] * OUT_S + (0 if side == "hi" else OUT_S - 1)        # the nearest voxel beyond the face on that axis
        beyond.append(vox)
    at = (0, 1, 63, 64, 65, 200, inside.shape[0] // 2, inside.shape[0] - 1)
    return inside, grid, np.asarray(beyond, np.int32), at


def with_outside(inside, beyond, at, which):
    """the frame with beyond[which] inserted so that they get the ids at[which]; (coords, their ids)"""
    coords = inside
    pairs = sorted((at[i], i) for i in which)
    for pos, i in pairs:
        coords = np.insert(coords, pos, beyond[i], 0)
    ids = np.array([p for p, _ in pairs])
    return np.ascontiguousarray(coords.astype(np.int32)), ids


# ---------------------------------------------------------------------------------------------------------- d: first voxel
FIRST_S = 3
FIRST_N = (1, 7, 8, 9, 2047, 2048, 2049, 4097, 64 * 2048 + 1)
FIRST_BOX = 96                                                      # voxels in [-48, 48)^3 x 2 batch items: 1.7 M positions
FIRST_MARK = (2047, 2048)                                           # the last id of tile 0, the first id of tile 1
SEQ_S = 8                                                           # block edge of first_sequence(): one the general layout's plan runs


def first_bounds():
    return (-FIRST_BOX // 2, -FIRST_BOX // 2, -FIRST_BOX // 2, 0), (FIRST_BOX // 2 - 1, FIRST_BOX // 2 - 1, FIRST_BOX // 2 - 1, 1)


def first_frame(n, seed=0):
    """n unique voxels in random order; where n allows, ids 2047 and 2048 are the first voxels of two reserved blocks, which get
    later members too"""
    rng = np.random.default_rng(50 + seed)
    h = FIRST_BOX // 2
    lin = rng.choice(2 * FIRST_BOX ** 3, min(2 * FIRST_BOX ** 3, n + 4096), replace=False)
    c = np.stack([lin % FIRST_BOX - h, (lin // FIRST_BOX) % FIRST_BOX - h, (lin // FIRST_BOX ** 2) % FIRST_BOX - h,
                  lin // FIRST_BOX ** 3], 1).astype(np.int64)
    reserved = np.array([[0, 0, 0, 0], [-1, -1, -1, 1]])             # blocks (0,0,0,0) and (-1,-1,-1,1)
    blk = R.block_rows(c, FIRST_S)
    is_res = [(blk == r).all(1) for r in reserved]
    rest = c[~(is_res[0] | is_res[1])][:n]
    if n <= FIRST_MARK[1] + 2:
        return np.ascontiguousarray(rest.astype(np.int32))
    out = rest.copy()
    for r, mark, later in zip(reserved, FIRST_MARK, (n - 1, FIRST_MARK[1] + 1)):
        out[mark] = np.concatenate([r[:3] * FIRST_S, r[3:]])
        out[later] = np.concatenate([r[:3] * FIRST_S + 1, r[3:]])
    return np.ascontiguousarray(out.astype(np.int32))


BIG_N, BIG_BOX, BIG_S = 2 ** 21 + 1, 600, 5


def first_big():
    rng = np.random.default_rng(53)
    c = rng.integers(0, BIG_BOX, (BIG_N, 4))
    c[:, 3] = rng.integers(0, 2, BIG_N)
    return np.ascontiguousarray(c.astype(np.int32)), ((0, 0, 0, 0), (BIG_BOX - 1, BIG_BOX - 1, BIG_BOX - 1, 1))


def first_sequence():
    """[(name, coords int32)] run one after another on one set of tables over first_bounds(): A, a subset of A's cells, a disjoint
    frame, a superset, a frame with n < the previous M, n = 0, a frame with a dropped voxel, A again"""
    a = first_frame(3000, seed=1)
    blk = R.block_rows(a, SEQ_S)
    u, inv = np.unique(blk, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sub = a[inv % 3 == 0]                                           # every voxel of a third of A's cells
    other = first_frame(6000, seed=2)
    ob = R.block_rows(other, SEQ_S)
    keys = set(map(tuple, u.tolist()))
    disjoint = other[np.array([tuple(r) not in keys for r in ob.tolist()])][:2500]
    superset = np.concatenate([a, disjoint[:1500]], 0)[np.random.default_rng(54).permutation(4500)]
    few = a[:40]                                                    # n < M of the superset
    dropped = a[:500].copy()
    dropped[17, 0] = first_bounds()[1][0] + 10 * SEQ_S
    seq = [("A", a), ("subset", sub), ("disjoint", disjoint), ("superset", superset), ("few", few), ("empty", a[:0]),
           ("dropped", dropped), ("A_again", a)]
    return [(k, np.ascontiguousarray(v.astype(np.int32))) for k, v in seq]


# ---------------------------------------------------------------------------------------------------------------- e: cells
CELLS_DIM, CELLS_LO = (2, 9, 11, 13), (3, -4, -5, -6)               # rows are (b, x, y, z)


def cells_frame():
    """(rows int32 [n, 4] shuffled, grid, number inside, number outside): 400 distinct rows inside drawn 2000 times, one row beyond
    each face, and 37 copies of the row k_kmap_candidates emits for 'no site': (lo_b - 1, 0, 0, 0)"""
    rng = np.random.default_rng(59)
    grid = (np.asarray(CELLS_LO, np.int64), np.asarray(CELLS_DIM, np.int64))
    v = int(np.prod(CELLS_DIM))
    distinct = rng.choice(v, 400, replace=False)
    inside = R.rows_of_cells(distinct[np.concatenate([np.arange(400), rng.integers(0, 400, 1600)])], grid)
    outside = []
    for axis, side in FACES:
        row = R.rows_of_cells(np.array([int(rng.integers(v))]), grid)[0]
        row[axis] = CELLS_LO[axis] - 1 if side == "lo" else CELLS_LO[axis] + CELLS_DIM[axis]
        outside.append(row)
    outside += [np.array([CELLS_LO[0] - 1, 0, 0, 0])] * 37
    rows = np.concatenate([inside, np.asarray(outside)], 0)
    return _shuffled(rows, rng), grid, inside.shape[0], len(outside)


# -------------------------------------------------------------------------------------------------------- f: neighbour map
NBR_R, NBR_STEP = (1, 2, 3, 4, 5), (1, 2, 3)


def _box(lo, dim, batch):
    g = np.stack(np.meshgrid(*[np.arange(lo[d], lo[d] + dim[d]) for d in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.full((g.shape[0], 1), batch)], 1)


def nbr_frames():
    """{name: rows int32 [m, 4] in np.unique order (what a BlockIndex with s = 1 gives)}"""
    out = {"solid": _box((-3, -2, -4), (7, 6, 8), 0),
           "thin_x": _box((-1, -6, -6), (1, 12, 12), 0), "thin_y": _box((-6, 2, -6), (12, 1, 12), 0),
           "thin_z": _box((-6, -6, 0), (12, 12, 1), 0),
           # two batch items whose cells are adjacent in memory: batch is the fastest axis of the cell number, and item 1 holds
           # exactly the cells item 0 does not -- any look-up that crosses the batch finds a neighbour where there is none
           "batch": None}
    full = _box((0, 0, 0), (6, 6, 6), 0)
    pick = np.random.default_rng(61).random(full.shape[0]) < 0.5
    b0, b1 = full[pick], full[~pick].copy()
    b1[:, 3] = 1
    out["batch"] = np.concatenate([b0, b1], 0)
    return {k: np.unique(v, axis=0).astype(np.int32) for k, v in out.items()}


def solid_neighbor(rows, lo, dim, r, step, transpose):
    """closed form for the solid box in np.unique order: index = ((x - x0) * dy + (y - y0)) * dz + (z - z0)"""
    offs = R.kernel_offsets(r) * (-step if transpose else step)
    q = rows[:, None, :3].astype(np.int64) + offs[None] - np.asarray(lo)
    ok = ((q >= 0) & (q < np.asarray(dim))).all(2)
    return np.where(ok, (q[..., 0] * dim[1] + q[..., 1]) * dim[2] + q[..., 2], -1)


TABLE_REPEATS = (2, 64, 1000)


def table_frame():
    """(rows int32 [m, 4] in random order with three rows repeated 2, 64 and 1000 times among 500 distinct ones, grid)"""
    rng = np.random.default_rng(67)
    grid = (np.array([-4, -4, -4, 0]), np.array([9, 9, 9, 2]))
    cells = rng.choice(9 * 9 * 9 * 2, 500, replace=False)
    rep = np.ones(500, np.int64)
    rep[:3] = TABLE_REPEATS
    rows = np.repeat(R.rows_of_cells(cells, grid), rep, 0)
    return _shuffled(rows, rng), grid


# ------------------------------------------------------------------------------------------------------------ g: kernel maps
def kmap_frame():
    rng = np.random.default_rng(71)
    c = np.unique(np.concatenate([rng.integers(-40, 40, (640, 3)), rng.integers(0, 2, (640, 1))], 1), axis=0)
    return _shuffled(c, rng)


def on_lattice(coords, ts):
    """the frame moved onto the lattice of the per-axis tensor stride (what a layer at that stride sees), unique, shuffled"""
    c = coords.astype(np.int64)
    c[:, :3] = c[:, :3] // np.asarray(ts) * np.asarray(ts)
    return _shuffled(np.unique(c, axis=0), np.random.default_rng(73))


GEOMETRIES = [((3, 1, 3), (1, 1, 1)), ((1, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 1), (2, 2, 1)), ((3, 3, 1), (2, 2, 1)),
              ((2, 2, 2), (1, 1, 1)), ((5, 5, 3), (1, 1, 1)), ((3, 2, 3), (1, 1, 1)), ((3, 3, 3), (2, 1, 3)), ((4, 3, 2), (2, 2, 1)),
              ((7, 1, 1), (3, 1, 1)), ((2, 2, 2), (2, 2, 2)), ((1, 1, 1), (2, 2, 2))]          # tests/test_gpu_generalconv.py
EXTRA = [((7, 7, 7), (1, 1, 1)), ((2, 3, 4), (1, 1, 1)), ((4, 3, 2), (2, 3, 1))]


def _kmap_cases():
    cases = []
    for ts in ((1, 1, 1), (2, 1, 1)):
        for k in range(1, KMAP_MAX_EXTENT + 1):
            for s in range(1, 5):
                cases.append(((k, 1, 1), (s, 1, 1), ts))
    for ts in ((1, 1, 1), (2, 2, 1)):
        for ks, st in GEOMETRIES + EXTRA:
            cases.append((ks, st, ts))
    return cases


KMAP_CASES = _kmap_cases()


I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
EDGE_CASES = [((2, 1, 1), (2, 1, 1)), ((3, 1, 1), (3, 1, 1)), ((1, 1, 1), (2, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((4, 3, 2), (2, 2, 1)),
              ((1, 1, 1), (3, 1, 1)), ((3, 1, 3), (1, 1, 1)), ((2, 2, 2), (1, 1, 1)), ((5, 5, 3), (1, 1, 1))]


def edge_frame(end):
    """about 300 unique voxels, two batch items, every coordinate within 8 of INT32_MAX ('max') or of INT32_MIN ('min'), the extreme
    value itself present on every axis: taps of any kernel wider than 1 leave the int32 range there"""
    rng = np.random.default_rng(83)
    lin = rng.choice(2 * 9 ** 3, 300, replace=False)
    c = np.stack([lin % 9, (lin // 9) % 9, (lin // 81) % 9, lin // 729], 1).astype(np.int64)
    c[:3, :3] = np.array([[0, 4, 4], [4, 0, 4], [4, 4, 0]]) if end == "min" else np.array([[8, 4, 4], [4, 8, 4], [4, 4, 8]])
    c = np.unique(c, axis=0)
    c[:, :3] += I32_MIN if end == "min" else I32_MAX - 8
    return _shuffled(c, rng)


def edge_refuses(ks, st, ts, lo, hi):
    """does strided_out_coords refuse (ValueError before any launch) a frame with per-axis bounds lo .. hi?  The floor rule: when a
    floored coordinate is below INT32_MIN; the candidate rule: when a tap of an extreme input leaves the int32 range (link_amd/index.py)"""
    ss = [st[d] * ts[d] for d in range(3)]
    if R.floor_rule(ks, st):
        return any((lo[d] // ss[d]) * ss[d] < I32_MIN for d in range(3))
    return any(hi[d] + R.taps(ks[d])[-1] * ts[d] > I32_MAX or lo[d] + R.taps(ks[d])[0] * ts[d] <= I32_MIN for d in range(3))


# ------------------------------------------------------------------------------------------------------------------ routes
def route_sites(ks, st, ts):
    """entries strided_out_coords calls for the output sites of a strided layer (link_amd/index.py): the floor rule is torch
    arithmetic, the candidate rule link_kmap_candidate_count + link_kmap_out_candidates; link_index_cells follows either"""
    if R.floor_rule(ks, st):
        return ["link_index_cells"]
    return ["link_kmap_candidate_count", "link_kmap_out_candidates", "link_index_cells"]


def route_table(ks, ts, cubic, strided):
    """entries of the gather table.  cubic (one extent, one tensor stride) at stride 1, and kernel 2 / stride 2 on an isotropic
    tensor stride: foreign_neighbor_map -> link_neighbor_map; everything else box_neighbor_map -> link_kmap_box_table; both between
    link_cell_table_build and link_cell_table_clear.  (neighbor_table_of / _strided_map / _general_map of link_amd/elk.py)"""
    look = "link_neighbor_map" if cubic else "link_kmap_box_table"
    return ["link_cell_table_build", look, "link_cell_table_clear"]


def is_cubic(ks, st, ts):
    """does Conv3d take the cubic builders for this layer?"""
    iso = len(set(ts)) == 1
    if all(s == 1 for s in st):
        return len(set(ks)) == 1 and iso
    return tuple(ks) == (2, 2, 2) and tuple(st) == (2, 2, 2) and iso


def route_conv(ks, st, ts, need_back):
    """every library entry Conv3d._route makes on a fresh tensor whose bounds are not cached (link_coords_bbox first), in order"""
    if all(s == 1 for s in st):
        if ks == (1, 1, 1):
            return []
        calls = ["link_coords_bbox"] + route_table(ks, ts, is_cubic(ks, st, ts), False)
        if need_back and (ks[0] * ks[1] * ks[2]) % 2 == 0:
            calls.append("link_kmap_transpose")
        return calls
    calls = ["link_coords_bbox"]
    calls += ["link_index_cells"] if is_cubic(ks, st, ts) else route_sites(ks, st, ts)
    calls += route_table(ks, ts, is_cubic(ks, st, ts), True)
    if need_back:
        calls.append("link_kmap_transpose")
    return calls
