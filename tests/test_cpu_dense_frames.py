"""tests/dense_frames.py without a GPU: every named frame is what tests/test_gpu_dense_lattice.py says it is (unique voxels inside
the bounds, the per-cell counts, the 352 / 353 sums in the kernels' cell order), the restated theta bound of every (frame,
parameters) pair sits on the side of 32768 its case needs, the float64 reference is finite and what fp32 evaluation costs (o32)
leaves the absolute 1e-4 bound attainable where a case applies it, Ref64 equals the oracle on the structured frames, and every case
of the kernel-selection lattice lands on the launcher branch it names."""
import pytest
import torch

import dense_frames as DF
from ref64 import Ref64


def _counts(name):
    co, bounds, s = DF.frame(name)
    return DF.cell_counts(co, bounds, s), DF.grid_of(bounds, s)[1]


@pytest.mark.parametrize("name", DF.NAMED)
def test_frames_are_unique_shuffled_and_inside_their_bounds(name):
    co, bounds, s = DF.frame(name)
    assert co.dtype == torch.int32 and co.shape[1] == 4 and 1 <= co.shape[0] <= 11_000
    assert torch.unique(co, dim=0).shape[0] == co.shape[0]
    lo, hi = torch.tensor(bounds[0]), torch.tensor(bounds[1])
    assert bool((co >= lo).all()) and bool((co <= hi).all())
    if name not in ("far", "exact_far"):
        assert int(co[:, :3].min()) < 0 and bounds[0][0] % s == 0       # cells below zero; the generator's cells are the kernel's
    if co.shape[0] > 8:                                                 # odd coordinates (halves under coord_div = 2); voxel ids shuffled
        assert bool((co[:, :3] % 2 == 1).any())
        lo_b, dim = DF.grid_of(bounds, s)
        key = ((co[:, 0].long() // s - lo_b[0]) * dim[1] + co[:, 1].long() // s - lo_b[1]) * dim[2] + co[:, 2].long() // s - lo_b[2]
        assert bool((key[1:] < key[:-1]).any())
    assert torch.equal(DF.frame(name)[0], DF.frame.__wrapped__(name)[0])   # seeded: the same frame every time


@pytest.mark.parametrize("name", DF.NAMED)
def test_grid_restatement_matches_the_library(name):
    from link_amd import _lib as L
    _, bounds, s = DF.frame(name)
    g = L.grid_from_bounds(bounds[0], bounds[1], s)
    lo, dim = DF.grid_of(bounds, s)
    assert list(g.lo) == lo and list(g.dim) == dim


def test_full():
    cnt, dim = _counts("full")
    assert dim == [3, 3, 3, 1]
    at = lambda x, y, z: int(cnt[(x * 3 + y) * 3 + z])                  # noqa: E731
    assert at(1, 1, 1) == 343 and at(0, 0, 0) == 342                    # a cell of exactly k = s^3, and one below
    c = cnt.tolist()
    pairs = [(c[i], c[i + 1]) for i in range(len(c) - 1)]               # consecutive in the kernels' cell order (z fastest)
    assert (343, 9) in pairs and (343, 10) in pairs
    assert 343 + 9 == DF.LCAP and 343 + 10 == DF.LCAP + 1
    rest = [v for i, v in enumerate(c) if v not in (343, 342, 9, 10)]
    assert len(rest) == 27 - 6 and set(rest) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("name,k,dims", [("solid3", 27, [5, 5, 5, 1]), ("solid2", 8, [5, 13, 3, 1])])
def test_solid(name, k, dims):
    cnt, dim = _counts(name)
    assert dim == dims and bool((cnt == k).all()) and k == DF.frame(name)[2] ** 3
    assert dim[0] % 4 == 1 and dim[1] % 4 == 1                          # rim strips on both axes at r = 3


@pytest.mark.parametrize("name,dims", [("deep_strips13", [13, 5, 3, 1]), ("deep_strips5", [5, 5, 5, 1])])
def test_deep_strips(name, dims):
    cnt, dim = _counts(name)
    assert dim == dims and int(cnt.min()) >= 40 and int(cnt.max()) <= 71
    # a strip's plane (10 columns with their halo) holds far more than the 64 entries of the quad kernel's voxel map
    assert 10 * int(cnt.min()) > 64


def test_one_pair_corners_slab():
    cnt, dim = _counts("one")
    assert dim == [5, 5, 5, 1] and int(cnt.sum()) == 1
    cnt, _ = _counts("pair")
    assert int(cnt.sum()) == 2 and int(cnt.max()) == 2
    cnt, _ = _counts("corners")
    g = cnt.view(5, 5, 5)
    assert int(cnt.sum()) == 27 and all(int(g[c]) == 3 for c in DF._corner_cells())
    co, bounds, _ = DF.frame("corners")
    assert bool((co == torch.tensor(bounds[0])).all(1).any()) and bool((co[:, :3] == torch.tensor(bounds[1][:3])).all(1).any())
    cnt, dim = _counts("slab")
    g = cnt.view(2, 5, 5, 5)
    assert dim == [5, 5, 5, 2] and int(g[:, :, :, 1:].sum()) == 0 and int(g[0, :, :, 0].min()) >= 1 and int(g[1].sum()) == 1
    for name in ("full", "one", "pair", "corners", "slab"):             # the batch cases' common grid holds them all
        co, _, s = DF.frame(name)
        assert s == 7 and int(DF.cell_counts(co, DF.COMMON_BOUNDS, 7).sum()) == co.shape[0]


def test_s8():
    cnt, dim = _counts("s8")
    assert dim == [4, 4, 4, 1] and sorted(cnt.tolist()) == sorted((37 * i) % 90 for i in range(64))
    assert int(cnt.min()) == 0 and int(cnt.max()) == 89 and int(cnt.max()) < DF.LCAP < 8 ** 3
    cnt, dim = _counts("s8_full")
    assert dim == [3, 3, 3, 1] and int(cnt.max()) == 512 and int((cnt == 512).sum()) == 1
    cnt, dim = _counts("s8_352")                                        # exactly the fused kernels' capacity, once
    assert dim == [3, 3, 3, 1] and int(cnt.max()) == DF.LCAP and int((cnt == DF.LCAP).sum()) == 1
    for name in ("s8_352", "s8"):                                       # the s = 8 batch case runs them on the grid of `s8`
        co = DF.frame(name)[0]
        assert int(DF.cell_counts(co, DF.frame("s8")[1], 8).max()) <= DF.LCAP


# ------------------------------------------------------------------------------------------------------------------------------
# theta: the side of 32768 every case needs (10 % clear of it: the kernels evaluate the bound in fp32)
# ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 2, "cos"), (64, 2, "sin"), (64, 1, "cos_x"), (32, 1, "sin")]


def _bound(name, pos, shape, div):
    c, groups, op = shape
    blk = DF.block(c, groups, op, pos)
    _, bounds, s = DF.frame(name)
    return DF.theta_bound(bounds, s, div, blk.pos_weight[0].weight, blk.alpha if op == "cos_x" else None)


@pytest.mark.parametrize("shape", SHAPES)
def test_theta_bounds_of_the_large_theta_frames(shape):
    assert 1000.0 < _bound("far", "init", shape, 1.0) < 0.9 * DF.FAST_RANGE            # thousands of radians on the fast path
    assert _bound("far", "x20", shape, 1.0) > 1.1 * DF.FAST_RANGE                      # the slow path
    for div in (1.0, 2.0):
        assert _bound("exact_far", "exact", shape, div) > 1.1 * DF.FAST_RANGE          # the slow path, theta itself below 40
    assert _bound("exact_far", "exact", shape, 1.0) < 1.4e5 * (1.5 if shape[2] == "cos_x" else 1.0)       # alpha < 1.5


def test_exact_far_theta_is_exact_in_fp32():
    co, _, _ = DF.frame("exact_far")
    for div in (1.0, 2.0):
        for c, groups, op in SHAPES:
            w = DF.block(c, groups, op, "exact").pos_weight[0].weight.detach()
            assert bool((w[:, 0] == -w[:, 1]).all()) and set(w.abs().unique().tolist()) <= {0.125, 0.25, 0.5}
            x32, x64 = co[:, :3].float() / div, co[:, :3].double() / div
            th64 = x64 @ w.double().t()
            for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):                            # any order of summation
                th = torch.zeros(co.shape[0], w.shape[0])
                for a in order:
                    th = th + x32[:, a:a + 1] * w[:, a]
                assert torch.equal(th.double(), th64)
            assert float(th64.abs().max()) < 40.0


@pytest.mark.parametrize("name", [n for n in DF.NAMED if n not in ("far", "exact_far")])
def test_occupancy_frames_stay_on_the_fast_path(name):
    for shape in SHAPES:
        assert _bound(name, "init", shape, 1.0) < 0.9 * DF.FAST_RANGE


# ------------------------------------------------------------------------------------------------------------------------------
# the reference on these frames
# ------------------------------------------------------------------------------------------------------------------------------
def _o32(name, pos, c, groups, op, r, div=1.0):
    co, _, s = DF.frame(name)
    f = DF.rows_of(name, c, 1)
    p = DF.params_of(DF.block(c, groups, op, pos))
    kw = dict(baseop=op, groups=groups, coord_div=div)
    ref = Ref64(f, co, p, s, r, **kw)
    o32, ok32 = ref.rel(Ref64(f, co, p, s, r, dtype=torch.float32, **kw))
    _, ok64 = ref.rel(ref)
    return o32, ok32 and ok64


@pytest.mark.parametrize("name", [n for n in DF.NAMED if n != "far"])
def test_reference_is_finite_and_the_absolute_bound_attainable(name):
    """Every frame gated with absolute=True: 4 o32 + 2e-6 < 1e-4."""
    pos = "exact" if name == "exact_far" else "init"
    for c, groups, op, r in ((64, 2, "cos", 3), (64, 1, "cos_x", 2)):
        o32, ok = _o32(name, pos, c, groups, op, r)
        assert ok and 4.0 * o32 + 2e-6 < 1e-4, (name, op, o32)


def test_the_analytically_zero_case_is_the_only_one():
    """sin on the one-voxel frame: the float64 rows are rounding residue (gate_zero_rows); every other occupancy frame has rows of
    the size of the norm weights under both operations."""
    for name in DF.OCCUPANCY:
        for op in ("cos", "sin"):
            co, _, s = DF.frame(name)
            ref = Ref64(DF.rows_of(name, 64, 1), co, DF.params_of(DF.block(64, 2, op)), s, 3, baseop=op, groups=2)
            m = ref.compare(ref)[1]
            assert (m < 1e-9) == ((name, op) in DF.ANALYTIC_ZERO) and (m < 1e-9 or m > 0.5), (name, op, m)


def test_reference_on_the_frames_gated_without_the_absolute_bound():
    """far: fp32 evaluation of theta ~ 2 000 rad costs about 1e-4; with the weights times 20 about 2e-3 -- why those two cases
    drop the fixed 1e-4 and keep 4 o32 + 2e-6 alone."""
    o_far, ok = _o32("far", "init", 64, 2, "cos", 3)
    assert ok and 1e-6 < o_far < 1e-3
    o_x20, ok = _o32("far", "x20", 64, 2, "cos", 3)
    assert ok and o_far < o_x20 < 2e-2


@pytest.mark.parametrize("name", ["full", "solid3", "solid2"])
@pytest.mark.parametrize("op,groups,r", [("cos", 2, 3), ("cos_x", 1, 2)])
def test_ref64_equals_the_oracle_on_structured_frames(name, op, groups, r):
    from oracle import link_oracle as O
    C = 16
    co, _, s = DF.frame(name)
    f = DF.rows_of(name, C, 1).double()
    p = {k: v.double() for k, v in DF.params_of(DF.block(C, groups, op)).items()}
    want = O.elk_core_torch(f, co, p, s, r, op, groups)
    d, m, ok = Ref64(f, co, p, s, r, op, groups, chunk=777).compare(want)
    assert ok and d / m <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# the launcher restatement on the lattice's own parametrisation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,forms", DF.LATTICE, ids=[DF.case_id(c) for c, _ in DF.LATTICE])
def test_lattice_cases_reach_the_branch_they_name(case, forms):
    c, groups, op, s, r, div = case
    co, bounds = DF.lattice_frame(s, r)
    cnt = DF.cell_counts(co, bounds, s)
    dims = DF.grid_of(bounds, s)[1]
    assert sorted(set(cnt.tolist())) == list(range(9)) and int(cnt.max()) < s ** 3 and int(co[:, :3].min()) < 0
    for tuning, want in forms:
        got = DF.route(c, groups, op, r, s ** 3, dims, coord_div=div, **tuning)
        assert "refused" not in got and got["div"] == (div != 1.0) and not got["slow"]
        assert {k: got.get(k) for k in want} == want, (case, tuning, got)


def test_lattice_covers_every_branch():
    seen = set()
    for (c, groups, op, s, r, div), forms in DF.LATTICE:
        dims = DF.grid_of(DF.lattice_frame(s, r)[1], s)[1]
        for tuning, _ in forms:
            g = DF.route(c, groups, op, r, s ** 3, dims, coord_div=div, **tuning)
            seen.add((g["k1"], g.get("nb"), g.get("writeback"), g["k2"], g.get("pair"), g.get("rim"), g.get("one_role"), g["div"]))
    for div in (False, True):
        for k2, pair in (("quad", True), ("own", True), ("own", False), ("split", True), ("split", False), ("single", True),
                         ("single", False), ("gather+demod", False)):
            assert any(t[3] == k2 and t[4] == pair and t[7] == div for t in seen), (k2, pair, div)
        for k1 in ("range", "tiles", "mm", "premix_insert+modsum"):
            assert any(t[0] == k1 and t[7] == div for t in seen), (k1, div)
        assert any(t[5] == "strips" and t[7] == div for t in seen) and any(t[2] is False and t[7] == div for t in seen)
        assert {t[1] for t in seen if t[0] in ("range", "mm") and t[7] == div} >= {1, 2, 4}
    assert len(DF.ROW1_FORMS) == 10


def test_route_capacity_and_refusals():
    big = DF.route(64, 2, "cos", 3, 8 ** 3, [4, 4, 4, 1])
    assert big == dict(big, fused=False, k1="premix_insert+modsum", k2="quad")           # C = 64: the fused gather kernels follow
    assert DF.route(32, 1, "sin", 2, 8 ** 3, [4, 4, 4, 1])["k2"] == "gather+demod"
    assert "refused" in DF.route(64, 2, "cos", 3, 8 ** 3, [4, 4, 4, 1], half=True)
    assert "refused" in DF.route(128, 1, "cos", 3, 64, [4, 4, 4, 1], half=True)
    assert DF.route(64, 2, "cos", 3, DF.LCAP, [4, 4, 4, 1])["fused"]                     # slot_cap = 352 at s = 8
    assert "refused" in DF.route(64, 2, "cos", 3, 3, [4, 4, 4, 1])                       # slot_cap = 3 < the inline records
