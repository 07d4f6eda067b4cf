"""tests/voxel_oracle.py -- vectorised float32 numpy restatements of the reference's two voxelisation rules (test infrastructure only).

hard():    det3d/ops/point_cloud/point_cloud_ops.py:8-55,112-184.  The sequential loop is equivalent to: rank the occupied cells by
           their minimum point index, keep rank < max_voxels, keep in each kept cell the max_points smallest indices, ascending.
dynamic(): det3d/models/readers/dynamic_voxel_encoder.py:8-17 (inclusive upper bound, truncation, unique(dim=0) order, mean of all).
Points with a coordinate that is not finite are dropped (link_amd's documented deviation; the fixtures hold none).
"""
import numpy as np

F32 = np.float32
# the fixture sets of tests/golden/make_golden_voxelize.py: voxelize_hard_<name>.npz, voxelize_dyn_<name>.npz
HARD = ["n0", "n1", "n63", "n64", "n65", "n4097", "allout", "onevoxel", "clustered", "capped", "edges", "ndim4", "ndim6", "noreverse",
        "batch3", "full"]
DYN = ["n0", "n1", "n63", "n64", "n65", "n4097", "allout", "onevoxel", "clustered", "edges", "ndim4", "ndim6", "batch3", "full"]


def grid_of(voxel_size, rng):
    vs, rng = np.asarray(voxel_size, F32), np.asarray(rng, F32)
    return np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)


def hard(points, voxel_size, rng, max_points, max_voxels, reverse_index=True):
    """-> voxels float32 [M, max_points, ndim], coors int32 [M, 3], num int32 [M]"""
    points = np.ascontiguousarray(points, F32)
    vs, rng = np.asarray(voxel_size, F32), np.asarray(rng, F32)
    grid = grid_of(vs, rng)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((points[:, :3] - rng[:3]) / vs)
        ok = np.all((c >= 0) & (c < grid.astype(np.float64)), 1)
    idx = np.nonzero(ok)[0]
    ci = c[idx].astype(np.int64)
    lin = (ci[:, 2] * grid[1] + ci[:, 1]) * grid[0] + ci[:, 0]
    _, first, inv, counts = np.unique(lin, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    by_first = np.argsort(first, kind="stable")                       # cells in order of their first point
    rank = np.empty_like(by_first)
    rank[by_first] = np.arange(by_first.shape[0])
    m = min(int(max_voxels), by_first.shape[0])
    cr = rank[inv]                                                    # every point's voxel
    order = np.argsort(cr, kind="stable")                             # points by voxel, input order inside
    start = np.concatenate([[0], np.cumsum(counts[by_first])])[:-1]
    pos = np.empty(idx.shape[0], np.int64)
    pos[order] = np.arange(idx.shape[0]) - np.repeat(start, counts[by_first])
    keep = (cr < m) & (pos < max_points)
    voxels = np.zeros((m, max_points, points.shape[1]), F32)
    voxels[cr[keep], pos[keep]] = points[idx[keep]]
    cell = ci[first[by_first[:m]]]
    coors = (cell[:, ::-1] if reverse_index else cell).astype(np.int32).reshape(m, 3)
    num = np.minimum(counts[by_first[:m]], max_points).astype(np.int32)
    return voxels, coors, num


def hard_mean64(voxels, num):
    """float64 mean of the recorded rows, and the bound n 2^-24 max_i |x_i| of summing them in float32 in any order plus the divide"""
    v = voxels.astype(np.float64)
    n = np.maximum(num.astype(np.float64), 1)[:, None]
    return v.sum(1) / n, n * 2.0 ** -24 * np.abs(v).max(1) if v.shape[1] else np.zeros((v.shape[0], v.shape[2]))


def dynamic(points, rng, voxel_size):
    """-> coors int64 [M, 3] = z, y, x ascending, counts [M], mean float64 [M, ndim], bound [M, ndim] (as hard_mean64's)"""
    points = np.ascontiguousarray(points, F32)
    vs, rng = np.asarray(voxel_size, F32), np.asarray(rng, F32)
    with np.errstate(invalid="ignore"):
        ok = np.all((points[:, :3] >= rng[:3]) & (points[:, :3] <= rng[3:]), 1)
    p = points[ok]
    coords = np.trunc((p[:, [2, 1, 0]] - rng[[2, 1, 0]]) / vs[[2, 1, 0]]).astype(np.int64)
    if p.shape[0] == 0:
        z = np.zeros((0, points.shape[1]))
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64), z, z
    uniq, inv, counts = np.unique(coords, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((uniq.shape[0], p.shape[1]))
    np.add.at(sums, inv, p.astype(np.float64))
    amax = np.zeros_like(sums)
    np.maximum.at(amax, inv, np.abs(p.astype(np.float64)))
    return uniq, counts, sums / counts[:, None], counts[:, None] * 2.0 ** -24 * amax
