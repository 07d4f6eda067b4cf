"""numpy / float64 restatement of section M of include/link_amd.h (csrc/segio.hip, link_amd/segio.py) and the seeded cases of its
tests.  Nothing here imports link_amd: this is the arbiter the kernels, the torch composition and the recorded fixtures are held to.

quantize   per sample: the integer coordinate (given, or np.round(p / float32(vs)) in fp32), minus the sample's minimum per axis;
           the distinct rows in ascending lexicographic (x, y, z) order by np.unique(axis=0) -- a row sort, not the reference's
           ravel hash --, the first point of every voxel, the voxel of every point; the samples concatenated.
vote       the rows of every pass summed in float64 in ascending pass order, arg max with the lowest class among equals (a NaN sum counts as -inf), and the
           gap between the two largest sums (what decides whether an fp32 sum may legitimately choose otherwise).
count      seen / positive / correct over the points with label != ignore.
metrics    core/callbacks.py:63-79 written as loops over the classes 1..c-1.
"""
import numpy as np

EXT = 1 << 20
FLAG_EXTENT, FLAG_NONFINITE, FLAG_KEYBITS = 1, 2, 4


def round_coords(points, voxel_size):
    """np.round(block[:, :3] / voxel_size) as semantic_kitti.py:219 computes it on a float32 block: an fp32 divide, half to even"""
    return np.round(np.asarray(points, np.float32)[:, :3] / np.float32(voxel_size))


def quantize(clouds, voxel_size=None, capacity=None):
    """clouds: a list of int arrays [n, 3] (voxel_size None) or float arrays [n, >= 3] (rounded with voxel_size).
    -> dict(coords int32 [cap, 4] = x, y, z, b, indices int32 [cap], inverse int32 [n], inverse_local int32 [n],
    voxel_offsets int32 [B + 1], total, flags)"""
    n = sum(c.shape[0] for c in clouds)
    cap = n if capacity is None else capacity
    per, flags, ext_max = [], 0, [0, 0, 0]
    for c in clouds:
        q, bad = None, 0
        if c.shape[0]:
            if voxel_size is None:
                q = np.asarray(c, np.int64)[:, :3]
            else:
                r = round_coords(c, voxel_size)
                if not np.isfinite(r).all():
                    bad |= FLAG_NONFINITE
                if (np.abs(r[np.isfinite(r)]) >= 2.0 ** 31).any():
                    bad |= FLAG_EXTENT
                if not bad:
                    q = r.astype(np.int64)
            if not bad:
                q = q - q.min(0, keepdims=True)
                if q.max() >= EXT:
                    bad |= FLAG_EXTENT
                else:
                    ext_max = [max(a, int(e)) for a, e in zip(ext_max, q.max(0))]
        flags |= bad
        per.append(None if (bad or not c.shape[0]) else q)
    if sum(int(e).bit_length() for e in ext_max) + (len(clouds) - 1).bit_length() > 64:
        flags |= FLAG_KEYBITS
        per = [None] * len(clouds)
    coords = np.zeros((cap, 4), np.int32)
    indices = np.zeros((cap,), np.int32)
    inverse = np.full((n,), -1, np.int32)
    inverse_local = np.full((n,), -1, np.int32)
    voff, total, p0 = [0], 0, 0
    for b, (c, q) in enumerate(zip(clouds, per)):
        m = c.shape[0]
        if q is not None:
            uniq, first, inv = np.unique(q, axis=0, return_index=True, return_inverse=True)
            inv = inv.reshape(-1)
            k = uniq.shape[0]
            keep = max(0, min(k, cap - total))
            coords[total:total + keep, :3] = uniq[:keep]
            coords[total:total + keep, 3] = b
            indices[total:total + keep] = first[:keep] + p0
            fits = inv + total < cap
            inverse[p0:p0 + m] = np.where(fits, inv + total, -1)
            inverse_local[p0:p0 + m] = np.where(fits, inv, -1)
            total += k
        voff.append(min(total, cap))
        p0 += m
    return {"coords": coords, "indices": indices, "inverse": inverse, "inverse_local": inverse_local,
            "voxel_offsets": np.asarray(voff, np.int32), "total": total, "flags": flags}


def vote(rows, inverse=None):
    """rows [n_rows, c] (any float type, widened exactly), inverse int [V, P] or None -> (class int64 [P], gap float64 [P]): the
    votes summed in float64, an entry outside [0, n_rows) contributing nothing"""
    rows = np.asarray(rows, np.float64)
    n_rows, c = rows.shape
    if inverse is None:
        acc = rows.copy()
    else:
        inverse = np.asarray(inverse)
        inverse = inverse[None] if inverse.ndim == 1 else inverse
        acc = np.zeros((inverse.shape[1], c), np.float64)
        for v in range(inverse.shape[0]):
            idx = inverse[v].astype(np.int64)
            ok = (idx >= 0) & (idx < n_rows)
            acc[ok] += rows[idx[ok]]
    if acc.shape[0] == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.float64)
    acc = np.where(np.isnan(acc), -np.inf, acc)                      # a NaN sum counts as -inf: it never wins
    cls = np.argmax(acc, axis=1)                                     # numpy documents it: the first of equal maxima
    top2 = np.sort(acc, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):                              # -inf - -inf: no gap to speak of (NaN compares false)
        return cls.astype(np.int64), top2[:, 1] - top2[:, 0]


def count(cls, labels, c, ignore_label):
    """-> int64 [3, c] = seen, positive, correct"""
    out = np.zeros((3, c), np.int64)
    for p, y in zip(np.asarray(cls).tolist(), np.asarray(labels).tolist()):
        if y == ignore_label:
            continue
        if 0 <= y < c:
            out[0, y] += 1
        if 0 <= p < c:
            out[1, p] += 1
        if 0 <= y < c and p == y:
            out[2, y] += 1
    return out


def metrics(counters):
    """callbacks.py:63-79 -> (miou, macc, oacc) in float64"""
    seen, positive, correct = (np.asarray(counters[k], np.float64) for k in range(3))
    ious, accs = [], []
    for i in range(1, seen.shape[0]):
        if seen[i] == 0:
            ious.append(1.0)
            accs.append(1.0)
        else:
            ious.append(correct[i] / (seen[i] + positive[i] - correct[i]))
            accs.append(correct[i] / seen[i])
    with np.errstate(divide="ignore", invalid="ignore"):
        oacc = np.sum(correct[1:]) / np.sum(seen[1:])
    return float(np.mean(ious)), float(np.mean(accs)), float(oacc)


# ----------------------------------------------------------------------------------------------------------------------- cases
def make_cloud(n, seed, offset=(0, 0, 0), spread=None):
    """int32 [n, 3]: at least 30 % of the points repeat an earlier coordinate (40 % are drawn from the first 60 %), coordinates on
    both sides of zero, the minimum displaced by `offset`"""
    rng = np.random.default_rng(seed)
    spread = spread if spread is not None else max(4, int(round(n ** (1 / 3))) * 3)
    base = rng.integers(-spread, spread + 1, (n, 3))
    fresh = n - (n * 2) // 5
    if n > 2:
        base[fresh:] = base[rng.integers(0, max(fresh, 1), n - fresh)]
    base = base[rng.permutation(n)]
    return (base + np.asarray(offset)).astype(np.int32)


def duplicate_share(cloud):
    return 1.0 - np.unique(cloud, axis=0).shape[0] / max(cloud.shape[0], 1)


def make_batch(sizes, seed):
    """clouds with distinct per-sample minima"""
    return [make_cloud(n, seed + 17 * b, offset=(-40 * b - 3, 25 * b + 1, 7 - 11 * b)) for b, n in enumerate(sizes)]


def make_block(n, seed, voxel_size=0.05):
    """float32 [n, 4] = x, y, z, intensity: a LiDAR-sized spread on both sides of zero, 40 % of the points jittered copies that land
    in an earlier point's voxel"""
    rng = np.random.default_rng(seed)
    q = make_cloud(n, seed, spread=max(6, int(round(n ** (1 / 3))) * 4)).astype(np.float64)
    xyz = (q + rng.uniform(-0.3, 0.3, q.shape)) * voxel_size             # well inside the voxel: no rounding boundary in play
    return np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)


def make_eval_case(p, c, votes, seed, integer_ties=False):
    """-> (rows float32 [n_rows, c], inverse int32 [votes, p] with entries on and outside both ends of [0, n_rows), labels int64 [p]
    with every class, the ignore label 0 and 255)"""
    rng = np.random.default_rng(seed)
    n_rows = max(1, (p * 2) // 3 + 5)
    if integer_ties:
        rows = rng.integers(-2, 3, (n_rows, c)).astype(np.float32)       # sums of small integers: exact in every format, many ties
    else:
        rows = rng.standard_normal((n_rows, c)).astype(np.float32)
    inverse = rng.integers(0, n_rows, (votes, p)).astype(np.int32)
    if p >= 8:
        inverse[0, 1], inverse[votes - 1, 3], inverse[0, 5] = -1, n_rows, n_rows + 7
        inverse[:, 6] = -1                                               # a point no pass reaches
    labels = rng.integers(0, c, (p,)).astype(np.int64)
    labels[rng.random(p) < 0.1] = 255
    labels[rng.random(p) < 0.1] = 0
    return rows, inverse, labels


def nan_case(c):
    """rows with a NaN in class 0, in a middle class, in the winning class, in every class; -inf everywhere -> (rows, expected class)"""
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((40, c)).astype(np.float32)
    rows[0:10, 0] = np.nan
    rows[10:20, c // 2] = np.nan
    for i in range(20, 30):
        rows[i, int(np.argmax(rows[i]))] = np.nan
    rows[30:35] = np.nan
    rows[35:40] = -np.inf
    return rows, vote(rows)[0]
