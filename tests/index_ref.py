"""The integer layer of the library restated in plain numpy (int64 throughout): what csrc/index.hip (both numberings of the block
index, link_index_cells, the neighbour map, the cell table) and csrc/kmap.hip (candidate sites, box table, transposed table) have
to produce, written from the reference's Python (segmentation/core/models/utils.py:44-73, torchsparse nn/utils/kernel.py:11-32,
nn/functional/downsample.py:11-51, nn/functional/conv.py:103-113) and not from the kernels.  Imports nothing from link_amd; pinned
to the C oracle, the recorded fixtures and link_amd.get_kernel_offsets by tests/test_cpu_index_frames.py; the yardstick of
tests/test_gpu_index_lattice.py.  Every comparison against it is np.array_equal.

Voxels outside a given grid (block_index(..., grid=...)).  Read from k_cell_count / k_place / k_sort_seg as they stand: a voxel
whose block lies outside the grid is not counted, gets vox_blk = idx_query = -1 and sets bit 0 of the status word; everything else
is the complete index of the remaining voxels WITH THEIR VOXEL IDS KEPT -- M, counts, blk_start (blk_start[M] = NVALID = n -
dropped), blk_coords, cell_blk, and perm / pos_blk / vox_sorted in their first NVALID positions (positions past NVALID are not
written).  That is a usable index of the voxels inside, so it is what the variant returns: the index of coords[inside] with ids
mapped back through flatnonzero(inside)."""
import numpy as np

I64 = np.int64


def floordiv(a, b):
    return np.floor_divide(np.asarray(a, I64), np.asarray(b, I64))


# ------------------------------------------------------------------------------------------------------------------- grids
def grid_of(lo, hi, s):
    """(lo, dim) of the dense block grid over inclusive voxel bounds lo..hi (x, y, z, b), in block units: link_grid_from_bounds"""
    lo, hi = np.asarray(lo, I64), np.asarray(hi, I64)
    blo = np.concatenate([floordiv(lo[:3], s), lo[3:]])
    bhi = np.concatenate([floordiv(hi[:3], s), hi[3:]])
    return blo, bhi - blo + 1


def cells_of(rows, grid):
    """cell number of block rows (x, y, z, b) in grid (lo, dim): x outermost, batch fastest; -1 outside"""
    lo, dim = (np.asarray(v, I64) for v in grid)
    u = np.asarray(rows, I64).reshape(-1, 4) - lo
    inside = ((u >= 0) & (u < dim)).all(1)
    cell = ((u[:, 0] * dim[1] + u[:, 1]) * dim[2] + u[:, 2]) * dim[3] + u[:, 3]
    return np.where(inside, cell, -1)


def rows_of_cells(cells, grid):
    lo, dim = (np.asarray(v, I64) for v in grid)
    c = np.asarray(cells, I64)
    b = c % dim[3]; c = c // dim[3]
    z = c % dim[2]; c = c // dim[2]
    y = c % dim[1]; c = c // dim[1]
    return np.stack([c, y, z, b], 1) + lo


# ------------------------------------------------------------------------------------------------------------- block index
def unique_rows(rows):
    """np.unique(rows, axis=0, return_index=True, return_inverse=True, return_counts=True) through ONE linear key per row (first
    column outermost, so key order is the lexicographic row order): the 2 M-row frame in a second instead of six.  The CPU test
    holds it to np.unique(axis=0) itself."""
    lo = rows.min(0)
    ext = rows.max(0) - lo + 1
    assert float(ext[0]) * float(ext[1]) * float(ext[2]) * float(ext[3]) < 2.0 ** 62
    u = rows - lo
    key = ((u[:, 0] * ext[1] + u[:, 1]) * ext[2] + u[:, 2]) * ext[3] + u[:, 3]
    _, first, inv, cnt = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    return rows[first], first, inv.reshape(-1), cnt


def block_rows(coords, s):
    c = np.asarray(coords, I64).reshape(-1, 4)
    return np.concatenate([floordiv(c[:, :3], s), c[:, 3:]], 1)


def block_index(coords, s, order="cell", grid=None):
    """The block index of int coords [n, 4] (x, y, z, b) for block edge s.  order 'cell': blocks in the row order of
    np.unique(axis=0) over (x // s, y // s, z // s, b) (torch.unique(dim=0) of utils.py:47); 'first': blocks ranked by their
    smallest voxel id.  grid (lo, dim) in block units: voxels outside are dropped as the module docstring says.
    Returns a dict of int64 arrays: blk_coords [M, 4], counts [M], blk_start [M + 1], vox_blk [n] (-1 dropped), perm [NVALID]
    (voxel ids grouped by block, ascending inside a block), pos_blk [NVALID], vox_sorted [NVALID, 4] (x, y, z, id), and the
    ints m, nvalid, status; with a grid also cell_blk [V] (block + 1, 0 empty)."""
    c = np.asarray(coords, I64).reshape(-1, 4)
    n = c.shape[0]
    rows = block_rows(c, s)
    inside = np.ones(n, bool) if grid is None else cells_of(rows, grid) >= 0
    ids = np.flatnonzero(inside)
    if ids.size:
        u, first, inv, cnt = unique_rows(rows[ids])
    else:
        u, first, inv, cnt = np.zeros((0, 4), I64), np.zeros(0, I64), np.zeros(0, I64), np.zeros(0, I64)
    if order == "first":
        rank = np.argsort(first, kind="stable")            # `first` indexes ids, which ascends: the smallest voxel id of each block
        new = np.empty_like(rank)
        new[rank] = np.arange(rank.size)
        u, cnt, inv = u[rank], cnt[rank], new[inv]
    else:
        assert order == "cell"
    vox_blk = np.full(n, -1, I64)
    vox_blk[ids] = inv
    perm = ids[np.argsort(inv, kind="stable")]
    out = dict(blk_coords=u.astype(I64), counts=cnt.astype(I64), blk_start=np.concatenate([[0], np.cumsum(cnt)]).astype(I64),
               vox_blk=vox_blk, perm=perm.astype(I64), pos_blk=vox_blk[perm],
               vox_sorted=np.concatenate([c[perm, :3], perm[:, None]], 1).astype(I64),
               m=int(u.shape[0]), nvalid=int(ids.size), status=int(ids.size != n))
    if grid is not None:
        v = int(np.prod(np.asarray(grid[1], I64)))
        cell_blk = np.zeros(v, I64)
        cell_blk[cells_of(u, grid)] = np.arange(1, u.shape[0] + 1)
        out["cell_blk"] = cell_blk
    return out


def unique_cells(rows, grid):
    """link_index_cells: sorted unique rows of `rows` inside grid (lo, dim; block edge 1), their multiplicities, NVALID = rows
    inside, and the cell table.  Columns are compared in the order given (the callers pass (b, x, y, z))."""
    r = np.asarray(rows, I64).reshape(-1, 4)
    cell = cells_of(r, grid)
    keep = r[cell >= 0]
    if keep.shape[0]:
        u, cnt = np.unique(keep, axis=0, return_counts=True)
    else:
        u, cnt = np.zeros((0, 4), I64), np.zeros(0, I64)
    cell_blk = np.zeros(int(np.prod(np.asarray(grid[1], I64))), I64)
    cell_blk[cells_of(u, grid)] = np.arange(1, u.shape[0] + 1)
    return dict(blk_coords=u, counts=cnt.astype(I64), blk_start=np.concatenate([[0], np.cumsum(cnt)]).astype(I64), m=int(u.shape[0]),
                nvalid=int(keep.shape[0]), cell_blk=cell_blk)


def cell_table(rows, grid):
    """link_cell_table_build: (index + 1 of the FIRST row in each cell, 0 empty; whether a row lay outside)"""
    cell = cells_of(rows, grid)
    tab = np.zeros(int(np.prod(np.asarray(grid[1], I64))), I64)
    idx = np.flatnonzero(cell >= 0)
    big = np.full(tab.shape, np.iinfo(I64).max)
    np.minimum.at(big, cell[idx], idx + 1)
    tab[big != np.iinfo(I64).max] = big[big != np.iinfo(I64).max]
    return tab, bool((cell < 0).any())


# ----------------------------------------------------------------------------------------------------------- kernel offsets
def taps(k):
    """the taps of one axis of extent k: -(k + 1) // 2 + 1 ... (kernel.py:20, -k // 2 + 1 in Python's floor division)"""
    lo = -((k + 1) // 2) + 1
    return list(range(lo, lo + k))


def kernel_offsets(ks, step=(1, 1, 1)):
    """int64 [K, 3] in the reference's order (kernel.py:25-31): x fastest when the volume is odd, z fastest when it is even"""
    ks = (ks,) * 3 if np.isscalar(ks) else tuple(int(k) for k in ks)
    step = (step,) * 3 if np.isscalar(step) else tuple(int(v) for v in step)
    ax = [[t * step[d] for t in taps(ks[d])] for d in range(3)]
    if (ks[0] * ks[1] * ks[2]) % 2 == 1:
        offs = [(x, y, z) for z in ax[2] for y in ax[1] for x in ax[0]]
    else:
        offs = [(x, y, z) for x in ax[0] for y in ax[1] for z in ax[2]]
    return np.asarray(offs, I64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------- output sites
def _unique_bxyz(c):
    if c.shape[0] == 0:
        return np.zeros((0, 4), I64)
    u = np.unique(c[:, [3, 0, 1, 2]], axis=0)
    return np.ascontiguousarray(u[:, [1, 2, 3, 0]])


def floor_rule(ks, st):
    return all(int(st[d]) in (1, int(ks[d])) for d in range(3))


def floor_sites(coords, st, ts):
    """downsample.py:25-27: floored to multiples of stride * tensor stride; unique rows in (b, x, y, z) order"""
    c = np.asarray(coords, I64).reshape(-1, 4).copy()
    ss = np.asarray([int(st[d]) * int(ts[d]) for d in range(3)], I64)
    c[:, :3] = floordiv(c[:, :3], ss) * ss
    return _unique_bxyz(c)


def candidate_rows(coords, ks, st, ts):
    """downsample.py:29-43 by brute force over every (input, tap): (sites [n * K, 4], on the s * ts lattice on every axis,
    >= the inputs' per-axis minimum)"""
    c = np.asarray(coords, I64).reshape(-1, 4)
    offs = kernel_offsets(ks, ts)
    ss = np.asarray([int(st[d]) * int(ts[d]) for d in range(3)], I64)
    x = (c[:, None, :3] + offs[None]).reshape(-1, 3)
    b = np.repeat(c[:, 3:], offs.shape[0], 0)
    on = (x % ss == 0).all(1)
    above = (x >= c[:, :3].min(0)).all(1)
    return np.concatenate([x, b], 1), on, above


def candidate_sites(coords, ks, st, ts):
    rows, on, above = candidate_rows(coords, ks, st, ts)
    return _unique_bxyz(rows[on & above])


def out_sites(coords, ks, st, ts):
    """spdownsample (downsample.py:11-51): the floor rule where stride is 1 or the kernel extent on every axis, else candidates"""
    if np.asarray(coords).shape[0] == 0:
        return np.zeros((0, 4), I64)
    return floor_sites(coords, st, ts) if floor_rule(ks, st) else candidate_sites(coords, ks, st, ts)


# ------------------------------------------------------------------------------------------------------------------- tables
def _keys(rows, lo, ext):
    u = rows - lo
    return ((u[:, 3] * ext[0] + u[:, 0]) * ext[1] + u[:, 1]) * ext[2] + u[:, 2]


def gather_table(out_rows, offsets, table_rows):
    """table [n_out, K]: entry [j, k] = index of the FIRST row of table_rows equal to out_rows[j] + offsets[k] (same batch), -1
    when there is none (conv.py:105-113)"""
    o, t = np.asarray(out_rows, I64).reshape(-1, 4), np.asarray(table_rows, I64).reshape(-1, 4)
    offsets = np.asarray(offsets, I64).reshape(-1, 3)
    if o.shape[0] == 0 or t.shape[0] == 0:
        return np.full((o.shape[0], offsets.shape[0]), -1, I64)
    q = np.repeat(o, offsets.shape[0], 0)
    q[:, :3] += np.tile(offsets, (o.shape[0], 1))
    both = np.concatenate([q, t], 0)
    lo = both.min(0)
    ext = (both.max(0) - lo + 1)[:3]
    assert float(ext[0]) * float(ext[1]) * float(ext[2]) * float(both[:, 3].max() - lo[3] + 1) < 2.0 ** 62
    kt, first = np.unique(_keys(t, lo, ext), return_index=True)              # the first occurrence of every key
    kq = _keys(q, lo, ext)
    pos = np.minimum(np.searchsorted(kt, kq), kt.size - 1)
    hit = kt[pos] == kq
    return np.where(hit, first[pos], -1).reshape(o.shape[0], offsets.shape[0]).astype(I64)


def transpose_table(table, n_in):
    """back [n_in, K]: back[i, k] = the SMALLEST j with table[j, k] = i, -1 when there is none; entries outside [0, n_in) are
    ignored"""
    table = np.asarray(table, I64)
    m, kvol = table.shape
    big = np.iinfo(I64).max
    back = np.full((n_in, kvol), big, I64)
    jj, kk = np.nonzero((table >= 0) & (table < n_in))
    np.minimum.at(back, (table[jj, kk], kk), jj)
    back[back == big] = -1
    return back


def neighbor_map(rows, r, step=1, transpose=False, table_rows=None):
    """the cubic maps (link_neighbor_map): rows[i] +- offset_k * step looked up in table_rows (default: the rows themselves)"""
    offs = kernel_offsets(r) * (-int(step) if transpose else int(step))
    return gather_table(rows, offs, rows if table_rows is None else table_rows)
