"""Frames, row families, the case lattice and the route restatement of the float64 gate over the aggregation and point <-> voxel
surface (tests/test_gpu_agg_lattice.py; checked on the CPU by tests/test_cpu_agg_frames.py).  numpy only: no link_amd, no GPU.

Every frame is as small as its purpose allows (a few hundred to a few thousand voxels; `points` has 17 k rows because a cell of 8193
points is the case).  Each is a (coords int32 [N, 4], block edge s) pair whose rows are shuffled, so that voxel ids are not grouped by
block:

  members(s)  unique voxels with blocks of EXACTLY 1, 63, 64, 65, 127, 128, 129, 343 (and 512 at s = 8) members -- one, two and more
              64-id chunks of perm, a last chunk of another length, 64 and 65 on the nose -- and ordinary blocks around them;
  points()    float points for initial_voxelize (block edge 1, duplicates): cells of 1, 64, 65, 8192 and 8193 points, the last one
              past k_sort_seg's SORT_MAX_SEG;
  dense()     a 5 x 7 x 9 block grid (multiples of neither TZ = 4 nor any G = 16, 8, 4, 2), two batch items, cells on both sides of
              zero, more than a third occupied, with holes: the dense-grid form of the block gather at r = 3;
  sparse()    a 9 x 11 x 13 grid under one third occupied: z-runs of consecutive blocks (the column walk keeps planes) and blocks
              with no neighbour at all;
  corner()    every cell of the shell of a 5^3 grid: neighbours of every face, edge and corner block fall outside the grid.

route_*() restate which kernel instance a call takes, written from the dispatch code (aggregate.py, csrc/aggregate.hip,
csrc/elk.hip: link_aux_to_voxel_forward_scatter / _grid, launch_block_gather, dispatch_lpr), not from what a run did."""
import numpy as np

SPECIAL = (1, 63, 64, 65, 127, 128, 129, 343, 512)
POINT_CELLS = (1, 64, 65, 8192, 8193)
SORT_MAX_SEG = 8192                     # csrc/index.hip: a longer segment stays in atomic-rank order
DENSE_RATIO = 3                         # csrc/elk.hip: dense-grid form iff cells <= DENSE_RATIO * M


def _voxels_of(blocks, s, rng):
    """coords of {block (x, y, z, b): member count}: the first `count` cells of a random order of the block's s^3 cells"""
    cell = np.stack(np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij"), -1).reshape(-1, 3)
    out = []
    for (bx, by, bz, bb), k in blocks.items():
        assert 1 <= k <= s ** 3
        c = cell[rng.permutation(s ** 3)[:k]] + np.array([bx, by, bz]) * s
        out.append(np.concatenate([c, np.full((k, 1), bb)], 1))
    coords = np.concatenate(out, 0).astype(np.int32)
    return coords[rng.permutation(coords.shape[0])]


def members(s):
    """(coords, s, {block: count}): the special blocks on a 3 x 3 lattice of step 2 inside a 7 x 7 x 3 block box from -1, ordinary
    blocks (2 .. 40 members) on half of the other cells"""
    assert s in (7, 8)
    rng = np.random.default_rng(70 + s)
    sizes = [k for k in SPECIAL if k <= s ** 3]
    spots = [(2 * i, 2 * j, 0, 0) for i in range(3) for j in range(3)]
    blocks = dict(zip(spots, sizes))
    for x in range(-1, 6):
        for y in range(-1, 6):
            for z in range(-1, 2):
                if (x, y, z, 0) not in spots and rng.random() < 0.5:
                    blocks[(x, y, z, 0)] = int(rng.integers(2, 41))
    return _voxels_of(blocks, s, rng), s, blocks


def points():
    """(points float32 [P, 4], {cell: count}): init_res = after_res = 1; every coordinate at least 0.05 of a cell from a face"""
    rng = np.random.default_rng(77)
    spots = [(0, 0, 0, 0), (3, 0, 0, 0), (0, 3, 0, 0), (-3, 0, 1, 0), (2, -2, -1, 0)]
    cells = dict(zip(spots, POINT_CELLS))
    for x in range(-4, 6):
        for y in range(-4, 6):
            for z in range(-2, 3):
                if (x, y, z, 0) not in cells and rng.random() < 0.25:
                    cells[(x, y, z, 0)] = int(rng.integers(1, 6))
    rows = []
    for (x, y, z, b), k in cells.items():
        p = np.array([x, y, z], np.float64) + rng.uniform(0.05, 0.95, (k, 3))
        rows.append(np.concatenate([p, np.full((k, 1), float(b))], 1))
    pts = np.concatenate(rows, 0).astype(np.float32)
    return pts[rng.permutation(pts.shape[0])], cells


def _box_frame(lo, dims, batches, occupied, s, seed, vox=(1, 8)):
    rng = np.random.default_rng(seed)
    blocks = {}
    for b in range(batches):
        for x in range(dims[0]):
            for y in range(dims[1]):
                for z in range(dims[2]):
                    if occupied(x, y, z, b, rng):
                        blocks[(lo[0] + x, lo[1] + y, lo[2] + z, b)] = int(rng.integers(vox[0], min(vox[1], s ** 3) + 1))
    return _voxels_of(blocks, s, rng), s, blocks


def dense():
    dims = (5, 7, 9)

    def occ(x, y, z, b, rng):
        ends = x in (0, dims[0] - 1) and y in (0, dims[1] - 1) and z in (0, dims[2] - 1)     # the grid is exactly the box
        return ends or rng.random() < 0.6
    return _box_frame((-2, -3, -4), dims, 2, occ, 2, 81)


def sparse():
    dims = (9, 11, 13)
    rng0 = np.random.default_rng(82)
    runs = {}
    for _ in range(10):                                               # z-runs of 3 .. 6 consecutive blocks in 10 columns
        x, y = int(rng0.integers(0, dims[0])), int(rng0.integers(0, dims[1]))
        z0, ln = int(rng0.integers(0, 7)), int(rng0.integers(3, 7))
        for z in range(z0, z0 + ln):
            runs[(x, y, z)] = True
    lone = {(0, 0, 0): True, (8, 10, 12): True, (4, 0, 12): True}     # isolated blocks, two of them at the grid's ends
    for _ in range(60):
        c = tuple(int(v) for v in rng0.integers(0, dims))
        if all(max(abs(c[0] - o[0]), abs(c[1] - o[1]), abs(c[2] - o[2])) > 2 for o in list(runs) + list(lone)):
            lone[c] = True
    keep = {**runs, **lone}
    return _box_frame((-3, 2, -6), dims, 1, lambda x, y, z, b, rng: (x, y, z) in keep, 3, 83, vox=(1, 10))


def corner():
    def occ(x, y, z, b, rng):
        return min(x, y, z) == 0 or max(x, y, z) == 4 or (x, y, z) == (2, 2, 2)
    return _box_frame((-2, -2, -2), (5, 5, 5), 1, occ, 2, 84)


FRAMES = {"members7": lambda: members(7), "members8": lambda: members(8), "dense": dense, "sparse": sparse, "corner": corner}
_CACHE = {}


def frame(name):
    if name not in _CACHE:
        _CACHE[name] = FRAMES[name]()
    return _CACHE[name]


def block_grid(blocks):
    """(lo, dims) of the tight block grid of {block: count}: x, y, z, batch"""
    k = np.array(list(blocks))
    return tuple(int(v) for v in k.min(0)), tuple(int(v) for v in k.max(0) - k.min(0) + 1)


# ------------------------------------------------------------------------------------------------------------- row families
FAMILIES = ("normal", "offset", "onehot", "const")
CONST = 2.5


def rows(family, n, w, seed=0):
    """float32 [n, w]: N(0,1); N(0,1) + 1000 (a common offset: the division-first mean loses bits); one-hot rows; a constant field"""
    rng = np.random.default_rng(1000 + seed)
    if family == "normal":
        return rng.standard_normal((n, w)).astype(np.float32)
    if family == "offset":
        return (rng.standard_normal((n, w)) + 1000.0).astype(np.float32)
    if family == "onehot":
        x = np.zeros((n, w), np.float32)
        x[np.arange(n), (np.arange(n) * 7 + 3) % w] = 1.0
        return x
    assert family == "const"
    return np.full((n, w), CONST, np.float32)


# -------------------------------------------------------------------------------------------------------------------- routes
def route_block_mean(c):
    """link_block_mean (csrc/aggregate.hip): VEC channels a lane, ceil(c / (64 VEC)) passes of the j0 loop, a partial last pass"""
    vec = 4 if (c % 4 == 0 and c >= 256) else (2 if (c % 2 == 0 and c >= 128) else 1)
    return {"entry": "link_block_mean", "vec": vec, "j0_passes": -(-c // (64 * vec)), "tail": c % (64 * vec) != 0}


def lpr_of(c):
    """dispatch_lpr: lanes a row of c channels, 4 channels a lane, a power of two, at least 4"""
    need, l = (c + 3) // 4, 4
    while l < need:
        l <<= 1
    return l


def route_aux(w, r, m, grid_dims=None, native=True, entry=None):
    """_AuxToVoxel.forward / aux_to_voxel (aggregate.py) for m blocks of width w at radius r.  grid_dims: the four dimensions of the
    grid the index was ACTUALLY built on (a speculated grid may be larger than the frame's own).  entry: 'grid' for
    link_aux_to_voxel_forward_grid called directly."""
    K = r ** 3
    if not native:
        return {"route": "foreign", "entry": "link_devoxelize_forward", "k_passes": -(-K // 64)}
    scatter = (w % 8 == 0 or w % 12 == 0) and r <= 3 and w <= 512 and m > 0 and (m + 1) * (w + 1) * 4 < 2 ** 32
    if not scatter:
        assert entry is None
        return {"route": "table", "entry": "link_aux_to_voxel_forward", "k_passes": -(-K // 64), "vec4_gather": w % 4 == 0}
    parts = 2 if (w % 8 == 0 and w // 2 <= 256) else 3
    assert parts == 2 or (w % 12 == 0 and w // 3 <= 256)
    lpr = lpr_of(w // parts)
    out = {"route": entry or "scatter", "entry": "link_aux_to_voxel_forward_" + (entry or "scatter"), "parts": parts, "lpr": lpr}
    if grid_dims is not None:
        cells = int(np.prod([int(d) for d in grid_dims]))
        G, TZ = 64 // lpr, 4
        tiles = grid_dims[0] * grid_dims[3] * (-(-grid_dims[1] // max(G, 1))) * (-(-grid_dims[2] // TZ)) if lpr <= 32 else 0
        dense = lpr <= 32 and r == 3 and (tiles + 3) // 4 < (1 << 22) and cells <= DENSE_RATIO * m
        out["form"] = "dense" if dense else "column"
    return out


def route_aux_backward(r):
    """link_aux_to_voxel_backward: k_seg_sum, then k_nbr_reduce_t over the transposed map (the map itself at odd r)"""
    return {"entry": "link_aux_to_voxel_backward", "k_passes": -(-(r ** 3) // 64), "transposed": r % 2 == 0}


# --------------------------------------------------------------------------------------------------------------- the lattice
# a. voxel_to_aux: (frame, widths)
WIDTHS_A = (1, 126, 128, 130, 256, 260)
CASES_A = [("members7", WIDTHS_A), ("members8", WIDTHS_A), ("dense", (1, 130, 260)), ("corner", (126, 128, 256))]
# b. aux_to_voxel, scatter route: every width at every r on every frame
WIDTHS_P2 = (8, 24, 48, 128, 256, 264, 512)
WIDTHS_P3 = (12, 36, 60, 132, 300, 492)          # w % 12 == 0 and w % 8 != 0 (504 = 12 * 42 is a multiple of 8 and takes two parts: WIDTHS_P2X)
WIDTHS_P2X = (504,)
SCATTER_R = (1, 2, 3)
SCATTER_FRAMES = ("dense", "sparse", "corner", "members7")
WIDTHS_TABLE = (1, 4, 129, 260, 520)
TABLE_R = (1, 2, 3, 4, 5)
TABLE_FRAMES = {1: "dense", 2: "corner", 3: "sparse", 4: "corner", 5: "dense"}
GRID_CASES = (("dense", 24, 3), ("sparse", 132, 2))          # through ctypes: two of the scatter cases
C_WIDTHS = (1, 63, 64, 65, 129)
C_K = (1, 8, 27, 64, 125)


def lattice():
    """every case of groups a and b as (group, frame, w, r, route dict) with the frame's own (tight) grid"""
    out = []
    for name, widths in CASES_A:
        for w in widths:
            out.append(("a", name, w, None, route_block_mean(w)))
    for name in SCATTER_FRAMES:
        _, _, blocks = frame(name)
        dims = block_grid(blocks)[1]
        for r in SCATTER_R:
            for w in WIDTHS_P2 + WIDTHS_P3 + WIDTHS_P2X:
                out.append(("b", name, w, r, route_aux(w, r, len(blocks), dims)))
    for r in TABLE_R:
        _, _, blocks = frame(TABLE_FRAMES[r])
        for w in WIDTHS_TABLE:
            out.append(("b", TABLE_FRAMES[r], w, r, route_aux(w, r, len(blocks), block_grid(blocks)[1])))
    for name, w, r in GRID_CASES:
        _, _, blocks = frame(name)
        out.append(("b", name, w, r, route_aux(w, r, len(blocks), block_grid(blocks)[1], entry="grid")))
    out.append(("b", "corner", 8, 3, route_aux(8, 3, 99, native=False)))
    return out
