"""Plain-torch restatements of the aggregation and point <-> voxel surface, parameterised by dtype: float64 is the truth of the
gate in tests/test_gpu_agg_lattice.py, float32 from the SAME code is what evaluating the formula in fp32 costs (e_ref).

  block mean        utils.py:52 -> voxelize_cuda.cu:21: divide by the count, then add (index_add)
  box mean          utils.py:61-84: sum of count-weighted means over the r^3 neighbours of get_kernel_offsets(r), over the sum of
                    their counts, absent neighbours skipped; rows handed to the block's voxels
  voxelize / devoxelize, forward and adjoint (voxelize_cuda.cu, devoxelize_cuda.cu)
  trilinear weights devoxelize.py:10-48
  initial_voxelize / point_to_voxel / voxel_to_point (utils.py:234-324) composed from these

Everything integer (cells, voxel numbering, look-ups) is evaluated as the surface defines it -- from the float32 point coordinates
with float32 arithmetic -- whatever `dtype` is: the integer results are part of the contract, not of the rounding.  Blocks are numbered
as Ref64 numbers them (tests/ref64.py: torch.unique over the block coordinates with the batch column, x, y, z, batch lexicographic).
block_mean_seq32 is the strictly sequential fp32 block mean (acc += x / count in ascending voxel id, numpy) the kernel is held to bit
for bit.  Test infrastructure only: does not import link_amd."""
import numpy as np
import torch


def kernel_offsets(r: int) -> torch.Tensor:
    """get_kernel_offsets(r) (nn/utils/kernel.py:11-32, stride = dilation = 1) int64[r^3, 3]: odd volume x fastest, even z fastest."""
    ax = list(range((-r) // 2 + 1, r // 2 + 1))
    if (r ** 3) % 2 == 1:
        offs = [[x, y, z] for z in ax for y in ax for x in ax]
    else:
        offs = [[x, y, z] for x in ax for y in ax for z in ax]
    return torch.tensor(offs, dtype=torch.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------- integer side
def block_index(coords, s: int):
    """(small_c int64[M,4], idx_query int64[N], counts int64[M]) of utils.py:45-51."""
    c = torch.as_tensor(coords).to(torch.int64)
    bc = torch.cat([torch.div(c[:, :3], int(s), rounding_mode="floor"), c[:, 3:4]], 1)
    small_c, inv, counts = torch.unique(bc, dim=0, return_inverse=True, return_counts=True)
    return small_c, inv, counts


def lookup(table_rows, query_rows) -> torch.Tensor:
    """int64[Q]: the index in table_rows[M,4] of every query row, -1 if absent (the first of equal table rows wins)."""
    t, q = torch.as_tensor(table_rows).to(torch.int64), torch.as_tensor(query_rows).to(torch.int64)
    if t.shape[0] == 0:
        return torch.full((q.shape[0],), -1, dtype=torch.int64)
    lo = torch.minimum(t.min(0).values, q.min(0).values) if q.shape[0] else t.min(0).values
    hi = torch.maximum(t.max(0).values, q.max(0).values) if q.shape[0] else t.max(0).values
    span = hi - lo + 1
    assert float(span.double().prod()) < 2.0 ** 62

    def key(rows):
        u = rows - lo
        return ((u[:, 0] * span[1] + u[:, 1]) * span[2] + u[:, 2]) * span[3] + u[:, 3]
    tk, order = torch.sort(key(t), stable=True)
    qk = key(q)
    pos = torch.searchsorted(tk, qk).clamp(max=tk.shape[0] - 1)
    return torch.where(tk[pos] == qk, order[pos], torch.full_like(pos, -1))


def neighbor_table(small_c, r: int, step: int = 1, transpose: bool = False, queries=None) -> torch.Tensor:
    """int64[Q, r^3]: row of small_c holding queries[i] + offset_k * step (queries default to small_c), -1 absent."""
    sc = torch.as_tensor(small_c).to(torch.int64)
    q0 = sc if queries is None else torch.as_tensor(queries).to(torch.int64)
    cols = []
    for o in kernel_offsets(r) * (-step if transpose else step):
        q = q0.clone()
        q[:, :3] += o
        cols.append(lookup(sc, q))
    return torch.stack(cols, 1)


def fnv_hash(coords) -> np.ndarray:
    """sphash (hash_cuda.cu:8-22): FNV-1a over the four int32 columns, folded to 60 bits.  int64[N]."""
    c = np.asarray(coords).astype(np.int64)
    h = np.full(c.shape[0], 14695981039346656037, np.uint64)
    for a in range(4):
        h ^= (c[:, a] & 0xFFFFFFFF).astype(np.uint64)
        h *= np.uint64(1099511628211)
    h = (h >> np.uint64(60)) ^ (h & np.uint64(0x0FFFFFFFFFFFFFFF))
    return h.astype(np.int64)


# --------------------------------------------------------------------------------------------------------------- block level
def block_mean(x, inv, counts, dtype=torch.float64) -> torch.Tensor:
    """[M, c]: sum over the block's voxels of x / count -- the division first (voxelize_cuda.cu:21)."""
    x = torch.as_tensor(x).to(dtype)
    cnt = torch.as_tensor(counts).to(dtype)
    return torch.zeros(cnt.shape[0], x.shape[1], dtype=dtype).index_add_(0, inv, x / cnt[inv][:, None])


def block_mean_seq32(x, inv, counts) -> np.ndarray:
    """fp32 [M, c], strictly sequential: for voxel ids ascending, acc[block] += x[id] / float(count[block]) -- the order and the
    operations of voxelize_cpu.cpp:7-25 and of k_block_mean (segments sorted by id)."""
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    inv = np.asarray(inv, np.int64)
    cntf = np.asarray(counts).astype(np.float32)
    m = cntf.shape[0]
    order = np.argsort(inv, kind="stable")                           # ascending id inside a block
    sinv = inv[order]
    start = np.searchsorted(sinv, np.arange(m))
    rank = np.arange(inv.shape[0]) - start[sinv]                     # position of the voxel among its block's members
    o2 = np.argsort(rank, kind="stable")
    cut = np.searchsorted(rank[o2], np.arange(int(rank.max(initial=-1)) + 2))
    acc = np.zeros((m, x.shape[1]), np.float32)
    for k in range(cut.shape[0] - 1):                                # the k-th member of every block: distinct blocks, one add each
        rows = order[o2[cut[k]:cut[k + 1]]]
        b = inv[rows]
        acc[b] += x[rows] / cntf[b][:, None]
    return acc


def box_mean(small_f, counts, nbr, dtype=torch.float64) -> torch.Tensor:
    """[M, c] of utils.py:75-80: f = [F, 1] * count; sum over the present neighbours in k order; features over the count column."""
    f = torch.as_tensor(small_f).to(dtype)
    cnt = torch.as_tensor(counts).to(dtype)
    f = f * cnt[:, None]
    num = torch.zeros_like(f)
    den = torch.zeros_like(cnt)
    for k in range(nbr.shape[1]):
        q = nbr[:, k]
        hit = q >= 0
        g = q.clamp(min=0)
        num = num + torch.where(hit[:, None], f[g], torch.zeros_like(num))
        den = den + torch.where(hit, cnt[g], torch.zeros_like(den))
    return num / den[:, None]


def aux_to_voxel(small_f, counts, nbr, inv, dtype=torch.float64) -> torch.Tensor:
    """[N, c]: the box mean of every voxel's block (utils.py:82)."""
    return box_mean(small_f, counts, nbr, dtype)[inv]


def aggregate(x, coords, s: int, r: int, dtype=torch.float64):
    """voxel_to_aux then aux_to_voxel on x [N, c] (a tensor that may require grad): (out [N, c], small_f, parts of the index)."""
    small_c, inv, counts = block_index(coords, s)
    nbr = neighbor_table(small_c, r)
    small_f = block_mean(x, inv, counts, dtype)
    return aux_to_voxel(small_f, counts, nbr, inv, dtype), small_f, (small_c, inv, counts, nbr)


# ----------------------------------------------------------------------------------------------------- voxelize / devoxelize
def _valid(idx, counts):
    idx = torch.as_tensor(idx).to(torch.int64)
    cn = torch.as_tensor(counts).to(torch.int64)
    ok = (idx >= 0) & (idx < cn.shape[0])
    ok = ok & (cn[idx.clamp(0, max(cn.shape[0] - 1, 0))] > 0) if cn.shape[0] else ok
    return idx, cn, ok


def voxelize_fwd(x, idx, counts, dtype=torch.float64) -> torch.Tensor:
    """voxelize_cuda.cu:12-25: out[idx[i]] += x[i] / counts[idx[i]]; idx < 0, idx >= len(counts) and count 0 are skipped."""
    x = torch.as_tensor(x).to(dtype)
    idx, cn, ok = _valid(idx, counts)
    out = torch.zeros(cn.shape[0], x.shape[1], dtype=dtype)
    return out.index_add_(0, idx[ok], x[ok] / cn[idx[ok]].to(dtype)[:, None])


def voxelize_bwd(top, idx, counts, n: int, dtype=torch.float64) -> torch.Tensor:
    """voxelize_cuda.cu:28-42, the adjoint: bottom[i] = top[idx[i]] / counts[idx[i]], zero rows where the forward skipped."""
    top = torch.as_tensor(top).to(dtype)
    idx, cn, ok = _valid(idx, counts)
    out = torch.zeros(int(n), top.shape[1], dtype=dtype)
    out[ok] = top[idx[ok]] / cn[idx[ok]].to(dtype)[:, None]
    return out


def devoxelize_fwd(feat, ind, w, dtype=torch.float64) -> torch.Tensor:
    """devoxelize_cuda.cu:11-34: out[i] = sum_k w[i, k] * feat[ind[i, k]] over ind >= 0, k ascending."""
    feat, w = torch.as_tensor(feat).to(dtype), torch.as_tensor(w).to(dtype)
    ind = torch.as_tensor(ind).to(torch.int64)
    out = torch.zeros(ind.shape[0], feat.shape[1], dtype=dtype)
    for k in range(ind.shape[1]):
        hit = ind[:, k] >= 0
        out = out + torch.where(hit[:, None], w[:, k:k + 1] * feat[ind[:, k].clamp(min=0)], torch.zeros_like(out))
    return out


def devoxelize_bwd(top, ind, w, n: int, dtype=torch.float64) -> torch.Tensor:
    """devoxelize_cuda.cu:37-59, the adjoint: bottom[ind[i, k]] += w[i, k] * top[i]."""
    top, w = torch.as_tensor(top).to(dtype), torch.as_tensor(w).to(dtype)
    ind = torch.as_tensor(ind).to(torch.int64)
    out = torch.zeros(int(n), top.shape[1], dtype=dtype)
    for k in range(ind.shape[1]):
        hit = ind[:, k] >= 0
        out.index_add_(0, ind[hit, k], w[hit, k:k + 1] * top[hit])
    return out


def ti_weights(points, idx_query, scale=1, dtype=torch.float64) -> torch.Tensor:
    """devoxelize.py:10-48: [8, P] trilinear weights, corner k = 4 dx + 2 dy + dz, zero for absent corners (idx_query [8, P] == -1),
    renormalised by their sum + 1e-8."""
    p = torch.as_tensor(points)[:, :3].to(dtype)
    lo = torch.floor(p / scale) * scale if scale != 1 else torch.floor(p)
    hi = lo + scale
    near, far = hi - p, p - lo
    rows = []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                rows.append((far[:, 0] if dx else near[:, 0]) * (far[:, 1] if dy else near[:, 1]) * (far[:, 2] if dz else near[:, 2]))
    w = torch.stack(rows, 0)
    if scale != 1:
        w = w / scale ** 3
    w = torch.where(torch.as_tensor(idx_query) == -1, torch.zeros_like(w), w)
    return w / (w.sum(0) + 1e-8)


def face_margin(points, scale=1) -> float:
    """Smallest distance of a coordinate from a face of its cell of edge `scale`, in cells (float64 on the float32 values)."""
    u = torch.as_tensor(points)[:, :3].double() / scale
    f = u - torch.floor(u)
    return float(torch.minimum(f, 1.0 - f).min())


# ------------------------------------------------------------------------------------------------------------ point <-> voxel
def voxel_keys(scaled, stride: int) -> torch.Tensor:
    """utils.py:262-265: int64 [P, 4] voxel coordinate (multiple of stride) + batch, from the float32 coordinates in float32."""
    pc = torch.as_tensor(scaled).float()
    return torch.cat([torch.floor(pc[:, :3] / stride).int() * stride, pc[:, -1].int().view(-1, 1)], 1).to(torch.int64)


def initial_voxelize(points, feats, init_res, after_res, dtype=torch.float64):
    """utils.py:234-254: (vox_F [M, c], vox_C int64 [M, 4], idx_query int64 [P], counts int64 [M], z_C float32 [P, 4]); voxels are
    numbered by ascending coordinate hash (torch.unique of the hashes)."""
    pts = torch.as_tensor(points).float()
    scaled = torch.cat([(pts[:, :3] * init_res) / after_res, pts[:, -1].view(-1, 1)], 1)
    cells = torch.floor(scaled).int()
    h = fnv_hash(cells.numpy())
    _, first, inv, counts = np.unique(h, return_index=True, return_inverse=True, return_counts=True)
    inv, counts = torch.from_numpy(inv.reshape(-1)).to(torch.int64), torch.from_numpy(counts).to(torch.int64)
    vox_c = cells[torch.from_numpy(first)].to(torch.int64)
    return block_mean(feats, inv, counts, dtype), vox_c, inv, counts, scaled


def point_to_voxel(scaled, feats, vox_c, stride=1, dtype=torch.float64):
    """utils.py:259-281, uncached branch: (vox_F, idx_query, counts)."""
    idx = lookup(vox_c, voxel_keys(scaled, stride))
    counts = torch.bincount(idx[idx >= 0], minlength=torch.as_tensor(vox_c).shape[0])
    return voxelize_fwd(feats, idx, counts, dtype), idx, counts


def voxel_to_point(vox_f, vox_c, stride, scaled, nearest=False, dtype=torch.float64):
    """utils.py:286-324, uncached branch: (point feats [P, c], idx_query int64 [P, 8], weights [P, 8])."""
    idx = neighbor_table(vox_c, 2, step=int(stride), queries=voxel_keys(scaled, stride))
    w = ti_weights(scaled, idx.t(), stride, dtype).t().contiguous()
    if nearest:
        w[:, 1:] = 0.0
        idx[:, 1:] = -1
    return devoxelize_fwd(vox_f, idx, w, dtype), idx, w


def dist(a, b) -> float:
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) if a.numel() else 0.0
