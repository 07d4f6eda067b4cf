"""CPU-only: the g_generalconv_* fixtures (the reference's spnn.Conv3d over per-axis kernel sizes and strides, plain and
transposed; tests/golden/make_golden_generalconv.py) re-derived by a brute-force numpy definition that shares no code with
the library or the oracle -- a dict from coordinate to row, offsets enumerated by the two ordering rules of
nn/utils/kernel.py:24-30, float64 accumulation -- and link_amd's get_kernel_offsets against the stored offsets."""
import numpy as np
import pytest

from helpers import golden_files, load_golden, rel_err

FILES = golden_files("g_generalconv_*.npz")


def _offsets(ks, step):
    ax = [[v * step[d] for v in range(-ks[d] // 2 + 1, ks[d] // 2 + 1)] for d in range(3)]
    if (ks[0] * ks[1] * ks[2]) % 2 == 1:
        return [(x, y, z) for z in ax[2] for y in ax[1] for x in ax[0]]       # odd volume: z outermost, x fastest
    return [(x, y, z) for x in ax[0] for y in ax[1] for z in ax[2]]           # even volume: x outermost, z fastest


def _out_coords(C, ks, st, ts):
    ss = [st[d] * ts[d] for d in range(3)]
    sites = set()
    if all(st[d] in (1, ks[d]) for d in range(3)):
        for x, y, z, b in C.tolist():
            sites.add((b, x // ss[0] * ss[0], y // ss[1] * ss[1], z // ss[2] * ss[2]))
    else:
        lo = C[:, :3].min(0).tolist()
        for x, y, z, b in C.tolist():
            for o in _offsets(ks, ts):
                p = (x + o[0], y + o[1], z + o[2])
                if all(p[d] % ss[d] == 0 and p[d] >= lo[d] for d in range(3)):       # no upper filter
                    sites.add((b,) + p)
    s = np.array(sorted(sites), dtype=np.int64).reshape(-1, 4)
    return s[:, [1, 2, 3, 0]]


def _table(out_c, in_c, offs):
    row = {tuple(c): i for i, c in reversed(list(enumerate(in_c.tolist())))}
    t = np.full((out_c.shape[0], len(offs)), -1, dtype=np.int64)
    for j, (x, y, z, b) in enumerate(out_c.tolist()):
        for k, o in enumerate(offs):
            t[j, k] = row.get((x + o[0], y + o[1], z + o[2], b), -1)
    return t


def _conv(F, W, table, n_out, transposed):
    out = np.zeros((n_out, W.shape[-1]), dtype=np.float64)
    W = W.reshape(table.shape[1], -1, W.shape[-1]).astype(np.float64)
    F = F.astype(np.float64)
    for k in range(table.shape[1]):
        j = np.nonzero(table[:, k] >= 0)[0]
        i = table[j, k]
        if transposed:
            np.add.at(out, i, F[j] @ W[k])           # the plain layer's pair (input i, output j) read the other way round
        else:
            out[j] += F[i] @ W[k]
    return out


def test_fixture_set_is_complete():
    assert {"g_generalconv_%s.npz" % t for t in "abcdef"} <= set(FILES) and any("_b2" in f for f in FILES)


@pytest.mark.parametrize("name", FILES)
def test_fixture_rederived_by_brute_force(name):
    g = load_golden(name)
    meta = g["meta"]
    C, F, s = g["coords"].astype(np.int64), g["feats"], (1, 1, 1)
    cmaps = {s: C}
    for i, lay in enumerate(meta["layers"]):
        ks, st = tuple(lay["kernel_size"]), tuple(lay["stride"])
        assert tuple(lay["in_stride"]) == s
        if lay["transposed"]:
            s_out = tuple(s[d] // st[d] for d in range(3))
            out_c = cmaps[s_out]
            offs = _offsets(ks, s_out)
            table = _table(C, out_c, offs)               # the matching plain layer's map: fine rows under the coarse sites
        else:
            s_out = tuple(s[d] * st[d] for d in range(3))
            out_c = _out_coords(C, ks, st, s) if any(v > 1 for v in st) else C
            offs = _offsets(ks, s)
            table = _table(out_c, C, offs)
        assert np.array_equal(np.array(offs), g[f"offs{i}"]), i
        assert tuple(lay["out_stride"]) == s_out
        assert np.array_equal(out_c, g[f"x{i}_C"]), (name, i)
        if meta["features_valid"]:
            F = _conv(F, g[f"k{i}"], table, out_c.shape[0], lay["transposed"])
            err = rel_err(F, g[f"x{i}_F"])
            print(name, i, "rel_err", err)
            assert err < 1e-5, (name, i, err)
        cmaps.setdefault(s_out, out_c)
        C, s = out_c, s_out


def test_k3_s2_fixture_shows_the_candidate_rule():
    g = load_golden("g_generalconv_b.npz")
    C, out = g["coords"], g["x0_C"]
    floored = {tuple(r) for r in (C[:, :3] // 2 * 2).tolist()}
    assert {tuple(r) for r in out[:, :3].tolist()} != floored and out[:, :3].max() > C[:, :3].max()


@pytest.mark.parametrize("name", FILES)
def test_get_kernel_offsets_for_box_sizes(name):
    import link_amd as la
    g = load_golden(name)
    for i, lay in enumerate(g["meta"]["layers"]):
        step = lay["out_stride"] if lay["transposed"] else lay["in_stride"]
        got = la.get_kernel_offsets(tuple(lay["kernel_size"]), stride=tuple(step))
        assert np.array_equal(got.numpy(), g[f"offs{i}"]), (name, i)
