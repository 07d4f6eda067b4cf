"""CPU checks of the float64 gate over the aggregation and point <-> voxel surface (tests/test_gpu_agg_lattice.py): the frames of
tests/agg_frames.py have the properties they were built for, the case lattice contains every route value the gate names, and the
float64 restatements of tests/agg64.py are pinned to what the reference produced (the g_agg_* and g_pointvoxel_* fixtures, and the C
oracle oracle/link_oracle.py).

Bound of a float comparison, stated from the data: the recorded values are fp32 results of a sum of `terms` products, each rounded, so
they lie within ULPS * terms * ulp32(largest magnitude of the terms) of the exact sum; ULPS = 4 covers the division, the product with
the count or weight, the add and the final rounding of one term.  Integer outputs are equal."""
import numpy as np
import pytest
import torch

import agg64 as A
import agg_frames as AF
from helpers import golden_files, load_golden
from oracle import link_oracle as O

ULPS = 4


def bound(big, terms):
    return ULPS * terms * float(np.spacing(np.float32(big)))


def close(got64, want32, big, terms, what):
    d = A.dist(got64, torch.from_numpy(np.asarray(want32)))
    assert d <= bound(big, terms), (what, d, bound(big, terms))


def counts_of(coords, s):
    _, _, cnt = A.block_index(coords, s)
    return cnt.numpy()


# ------------------------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("s", [7, 8])
def test_members_has_every_special_block(s):
    coords, s, blocks = AF.members(s)
    assert np.unique(coords, axis=0).shape[0] == coords.shape[0] < 20000                 # unique voxels
    small_c, inv, cnt = A.block_index(coords, s)
    got = {tuple(int(v) for v in c): int(k) for c, k in zip(small_c, cnt)}
    assert got == blocks
    want = [k for k in AF.SPECIAL if k <= s ** 3]
    assert (512 in want) == (s == 8) and 343 in want
    for k in want:
        assert (cnt == k).sum() >= 1, k
    assert cnt.max() == want[-1] and ((cnt > 1) & (cnt < 41)).sum() > 20                 # ordinary blocks around them
    # voxel ids are not grouped by block: a block's members are spread over the rows
    assert (np.diff(inv.numpy()) != 0).mean() > 0.5
    assert coords[:, :3].min() < 0 < coords[:, :3].max()


def test_points_cells():
    pts, cells = AF.points()
    assert pts.dtype == np.float32 and pts.shape[0] < 20000
    vf, vc, idx, cnt, scaled = A.initial_voxelize(pts, pts[:, :1], 1, 1)
    assert vc.shape[0] == len(cells) and sorted(cnt.tolist()) == sorted(cells.values())
    for k in AF.POINT_CELLS:
        assert (cnt == k).sum() >= 1, k
    assert cnt.max() == AF.SORT_MAX_SEG + 1 and (cnt == AF.SORT_MAX_SEG).sum() == 1
    assert A.face_margin(pts) >= 0.05 - 1e-6
    assert np.array_equal(scaled.numpy(), pts)


def _grid_props(name):
    coords, s, blocks = AF.frame(name)
    lo, dims = AF.block_grid(blocks)
    small_c, _, cnt = A.block_index(coords, s)
    assert small_c.shape[0] == len(blocks) and coords.shape[0] < 20000
    assert np.unique(coords, axis=0).shape[0] == coords.shape[0]
    return coords, s, blocks, lo, dims, int(np.prod(dims))


def test_dense_frame():
    coords, s, blocks, lo, dims, cells = _grid_props("dense")
    assert cells <= AF.DENSE_RATIO * len(blocks) and len(blocks) < cells                 # over a third occupied, with holes
    assert dims[3] == 2 and dims[2] % 4 != 0 and all(dims[1] % g != 0 for g in (16, 8, 4, 2))
    assert all(dims[a] % 2 == 1 for a in range(3))
    assert all(lo[a] < 0 < lo[a] + dims[a] - 1 for a in range(3))                         # cells on both sides of zero
    for b in (0, 1):                                                                      # holes in both items
        n_b = sum(1 for k in blocks if k[3] == b)
        assert cells // 2 // 3 < n_b < cells // 2


def test_sparse_frame():
    coords, s, blocks, lo, dims, cells = _grid_props("sparse")
    assert cells > AF.DENSE_RATIO * len(blocks)
    keys = set(blocks)
    runs = sum(1 for (x, y, z, b) in keys if (x, y, z + 1, b) in keys and (x, y, z + 2, b) in keys and (x, y, z - 1, b) not in keys)
    assert runs >= 5                                                                       # z-runs of three and more consecutive blocks
    nbr = A.neighbor_table(torch.tensor(sorted(keys)), 3)
    alone = ((nbr >= 0).sum(1) == 1).sum()
    assert alone >= 5                                                                      # blocks that are their only neighbour
    assert any(k[:3] == lo[:3] for k in keys)                                              # one of them in the grid's first cell


def test_corner_frame():
    coords, s, blocks, lo, dims, cells = _grid_props("corner")
    keys = set(blocks)
    hi = tuple(lo[a] + dims[a] - 1 for a in range(3))
    for x in (lo[0], hi[0]):
        for y in (lo[1], hi[1]):
            for z in (lo[2], hi[2]):
                assert (x, y, z, 0) in keys
    for a in range(3):                                                                     # every cell of every face
        for v in (lo[a], hi[a]):
            assert sum(1 for k in keys if k[a] == v) == 25
    for r in (2, 3):                                                                       # neighbours outside the grid, at both radii
        nbr = A.neighbor_table(torch.tensor(sorted(keys)), r)
        assert (nbr < 0).any(1).sum() >= 98 - (27 if r == 2 else 0)


def test_row_families():
    for fam in AF.FAMILIES:
        x = AF.rows(fam, 50, 12, 3)
        assert x.shape == (50, 12) and x.dtype == np.float32
    assert abs(float(AF.rows("offset", 500, 8).mean()) - 1000.0) < 1.0
    assert (AF.rows("onehot", 50, 12).sum(1) == 1).all() and len(set(AF.rows("onehot", 50, 12).argmax(1))) == 12
    assert (AF.rows("const", 5, 3) == AF.CONST).all()


# ------------------------------------------------------------------------------------------------------------------ lattice
def test_lattice_contains_every_route_value():
    lat = AF.lattice()
    a = [c[4] for c in lat if c[0] == "a"]
    assert {r["vec"] for r in a} == {1, 2, 4}
    for vec in (2, 4):                                                                     # a full width, and one with a tail and a second pass
        assert {(r["j0_passes"], r["tail"]) for r in a if r["vec"] == vec} == {(1, False), (2, True)}
    assert {(r["j0_passes"], r["tail"]) for r in a if r["vec"] == 1} >= {(1, True), (2, True)}
    b = [c for c in lat if c[0] == "b"]
    assert {c[4]["route"] for c in b} == {"scatter", "table", "grid", "foreign"}
    sc = [c for c in b if c[4]["route"] == "scatter"]
    assert {c[4]["parts"] for c in sc} == {2, 3}
    assert {c[4]["lpr"] for c in sc} == {4, 8, 16, 32, 64}
    assert {c[4]["lpr"] for c in sc if c[4]["parts"] == 3} == {4, 8, 16, 32, 64}
    assert {c[3] for c in sc} == {1, 2, 3}
    for name in ("dense", "corner", "members7"):                                           # both forms on the occupied grids
        assert {c[4]["form"] for c in sc if c[1] == name} == {"dense", "column"}
    assert {c[4]["form"] for c in sc if c[1] == "sparse"} == {"column"}
    for parts in (2, 3):
        assert {c[4]["form"] for c in sc if c[4]["parts"] == parts} == {"dense", "column"}
    # the dense form is taken at r = 3 below 64 lanes a row only
    assert all((c[4]["form"] == "dense") == (c[3] == 3 and c[4]["lpr"] <= 32 and c[1] != "sparse") for c in sc)
    tb = [c for c in b if c[4]["route"] == "table"]
    assert {c[3] for c in tb} == {1, 2, 3, 4, 5} and {c[4]["k_passes"] for c in tb} == {1, 2}
    assert {c[4]["k_passes"] for c in tb if c[3] == 4} == {1} and {c[4]["k_passes"] for c in tb if c[3] == 5} == {2}
    assert {c[4]["vec4_gather"] for c in tb} == {True, False}
    assert {c[2] for c in tb} >= {1, 4, 129, 260} and max(c[2] for c in tb) > 512
    assert {AF.route_aux_backward(r)["transposed"] for r in AF.TABLE_R} == {True, False}
    assert {c[4]["parts"] for c in b if c[4]["route"] == "grid"} == {2, 3}
    # what the issue's width list calls a three-part width "up to 504" takes two parts: 504 is a multiple of 8
    assert AF.route_aux(504, 3, 100)["parts"] == 2 and AF.route_aux(492, 3, 100)["parts"] == 3
    # widths the scatter route refuses go to the table
    for w in (4, 129, 260, 520, 516):
        assert AF.route_aux(w, 3, 100)["route"] == "table"
    assert AF.route_aux(24, 4, 100)["route"] == "table"


def test_route_lpr_and_vec_against_their_definitions():
    assert [AF.lpr_of(c) for c in (1, 4, 16, 17, 32, 64, 66, 128, 132, 164, 252, 256)] == [4, 4, 4, 8, 8, 16, 32, 32, 64, 64, 64, 64]
    assert [AF.route_block_mean(c)["vec"] for c in (1, 126, 127, 128, 130, 254, 256, 258, 260)] == [1, 1, 1, 2, 2, 2, 4, 2, 4]


# ------------------------------------------------------------------------- float64 restatements against the reference's results
@pytest.mark.parametrize("name", golden_files("g_agg_*.npz"))
def test_aggregation_restatement_vs_fixture(name):
    g = load_golden(name)
    s, r = g["meta"]["s"], g["meta"]["r"]
    x = torch.from_numpy(g["feats"])
    small_c, inv, cnt = A.block_index(g["coords"], s)
    assert np.array_equal(small_c.numpy(), g["small_c"]) and np.array_equal(inv.numpy(), g["idx_query"])
    assert np.array_equal(cnt.numpy(), g["counts"])
    nbr = A.neighbor_table(small_c, r)
    if "nbr" in g:
        assert np.array_equal(nbr.numpy(), g["nbr"])
    big = float(np.abs(g["feats"]).max())
    mean = A.block_mean(x, inv, cnt)
    close(mean, g["aux_f"], big, int(cnt.max()), "aux_f")
    # the box mean of the RECORDED block means: a sum of r^3 products mean * count over a sum of counts
    out = A.aux_to_voxel(torch.from_numpy(g["aux_f"]), cnt, nbr, inv)
    close(out, g["out"], float(np.abs(g["aux_f"]).max()), r ** 3, "out")
    if "out_refcpu" in g:
        close(out, g["out_refcpu"], float(np.abs(g["aux_f"]).max()), r ** 3, "out_refcpu")
    # and the oracle's, on the same inputs
    close(A.aggregate(x, g["coords"], s, r)[0], O.aggregate(g["feats"], g["coords"], s, r), big, int(cnt.max()) + r ** 3, "aggregate")


def test_sequential_block_mean_is_the_fixture_bit_for_bit():
    g = load_golden("g_agg_a_s3_r2_w16.npz")
    _, inv, cnt = A.block_index(g["coords"], 3)
    assert np.array_equal(A.block_mean_seq32(g["feats"], inv.numpy(), cnt.numpy()), g["aux_f"])
    # and the C oracle's voxelize on a frame with long segments (members: up to 512 ids a block)
    coords, s, _ = AF.frame("members8")
    x = AF.rows("offset", coords.shape[0], 5, 1)
    _, inv, cnt = A.block_index(coords, s)
    assert np.array_equal(A.block_mean_seq32(x, inv.numpy(), cnt.numpy()), O.spvoxelize_fwd(x, inv.numpy().astype(np.int32), cnt.numpy().astype(np.int32)))


@pytest.mark.parametrize("name", golden_files("g_pointvoxel_*.npz"))
def test_pointvoxel_restatement_vs_fixture(name):
    g = load_golden(name)
    m = g["meta"]
    vf, vc, idx, cnt, scaled = A.initial_voxelize(g["points"], g["feats"], m["init_res"], m["after_res"])
    assert np.array_equal(vc.numpy(), g["vox_C"]) and np.array_equal(idx.numpy(), g["idx_query"])
    assert np.array_equal(cnt.numpy(), g["counts"]) and np.array_equal(scaled.numpy(), g["z_C"])
    close(vf, g["vox_F"], float(np.abs(g["feats"]).max()), int(cnt.max()), "vox_F")
    pf, pidx, pcnt = A.point_to_voxel(scaled, g["p2v_feats_in"], vc, 1)
    assert np.array_equal(pidx.numpy(), g["idx_query"]) and np.array_equal(pcnt.numpy(), g["counts"])
    close(pf, g["p2v_F"], float(np.abs(g["p2v_feats_in"]).max()), int(cnt.max()), "p2v_F")
    if "v2p1_F" not in g:
        return
    for tag, c, stride in (("v2p1", vc, 1), ("v2p2", torch.from_numpy(g["v2p2_C"]), 2)):
        f, ix, w = A.voxel_to_point(g[tag + "_F_in"], c, stride, scaled)
        assert np.array_equal(ix.numpy(), g[tag + "_idx"])
        if tag + "_w" in g:
            # a weight: a product of three differences of O(scale) over scale^3, then a quotient -- a few ulps of 1
            close(w, g[tag + "_w"], 1.0, 2, tag + "_w")
        close(f, g[tag + "_F"], float(np.abs(g[tag + "_F_in"]).max()), 8, tag + "_F")
    f, ix, w = A.voxel_to_point(g["v2p1_F_in"], vc, 1, scaled, nearest=True)
    close(f, g["v2p1_nearest_F"], float(np.abs(g["v2p1_F_in"]).max()), 1, "nearest")


def test_op_restatements_vs_oracle():
    rng = np.random.default_rng(5)
    n, n1, c, K = 3000, 200, 7, 27
    coords = rng.integers(-300, 300, (n, 4)).astype(np.int32)
    assert np.array_equal(A.fnv_hash(coords), O.sphash(coords))
    idx = rng.integers(-1, n1, n).astype(np.int32)
    counts = O.spcount(idx, n1)
    counts[:3] = 0                                                                         # counts with zeros: those rows are skipped
    assert np.array_equal(np.bincount(idx[idx >= 0], minlength=n1)[3:], counts[3:])
    x = rng.standard_normal((n, c)).astype(np.float32)
    top = rng.standard_normal((n1, c)).astype(np.float32)
    close(A.voxelize_fwd(x, idx, counts), O.spvoxelize_fwd(x, idx, counts), float(np.abs(x).max()), int(counts.max()), "vox_fwd")
    close(A.voxelize_bwd(top, idx, counts, n), O.spvoxelize_bwd(top, idx, counts, n), float(np.abs(top).max()), 1, "vox_bwd")
    ind = rng.integers(-1, n1, (500, K)).astype(np.int32)
    ind[:4] = -1
    w = rng.random((500, K)).astype(np.float32)
    g = rng.standard_normal((500, c)).astype(np.float32)
    close(A.devoxelize_fwd(top, ind, w), O.spdevoxelize_fwd(top, ind, w), float(np.abs(top).max()), K, "devox_fwd")
    per_row = int(np.bincount(ind[ind >= 0], minlength=n1).max())
    close(A.devoxelize_bwd(g, ind, w, n1), O.spdevoxelize_bwd(g, ind, w, n1), float(np.abs(g).max()), per_row, "devox_bwd")
    # adjointness of the restatements themselves, in float64: <A x, y> = <x, A^T y>
    xa, ya = torch.from_numpy(x).double(), torch.from_numpy(top).double()
    assert abs(float((A.voxelize_fwd(xa, idx, counts) * ya).sum() - (xa * A.voxelize_bwd(ya, idx, counts, n)).sum())) < 1e-9
    ga = torch.from_numpy(g).double()
    assert abs(float((A.devoxelize_fwd(ya, ind, w) * ga).sum() - (ya * A.devoxelize_bwd(ga, ind, w, n1)).sum())) < 1e-9
    for scale in (1, 2, 4):
        pts = np.concatenate([(rng.random((2000, 3)) - 0.5) * 40.0, np.zeros((2000, 1))], 1).astype(np.float32)
        u = pts[:, :3] / scale
        pts = pts[np.minimum(u - np.floor(u), np.ceil(u) - u).min(1) > 2.0 ** -10]         # fp32 and fp64 floor alike
        iq = rng.integers(-1, 50, (8, pts.shape[0]))
        iq[:, :5] = -1
        close(A.ti_weights(pts, iq, scale), O.calc_ti_weights_np(pts, iq, scale), 1.0, 2 * scale, "ti_weights %d" % scale)
    assert [tuple(o) for o in A.kernel_offsets(2).tolist()] == [tuple(o) for o in O.get_kernel_offsets(2).tolist()]
    for r in (1, 3, 4, 5):
        assert np.array_equal(A.kernel_offsets(r).numpy(), O.get_kernel_offsets(r))


def test_gradient_of_the_restatement_is_the_oracles():
    coords = AF.frame("corner")[0]
    x = AF.rows("normal", coords.shape[0], 6, 2)
    go = AF.rows("normal", coords.shape[0], 6, 3)
    xt = torch.from_numpy(x).requires_grad_(True)
    ref = O.aggregate_torch(xt, torch.from_numpy(coords), 2, 2)
    ref.backward(torch.from_numpy(go))
    xd = torch.from_numpy(x).double().requires_grad_(True)
    A.aggregate(xd, coords, 2, 2)[0].backward(torch.from_numpy(go).double())
    close(xd.grad, xt.grad.numpy(), float(np.abs(go).max()), 8 * 8, "grad")
