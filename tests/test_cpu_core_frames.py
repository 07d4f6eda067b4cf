"""tests/core_frames.py without a GPU: every named frame is what tests/test_gpu_core_lattice.py says it is (unique voxels inside
their bounds, seeded, the per-cell counts and the block sizes in sorted order, the exact voxel counts of the n... frames), the
restated grid equals the library's, the restated tile ranges and gather passes reach the branches the frames are named for, every
case of the lattice lands on the route() branch it names and every branch the lattice exists for is named by a case, theta sits on
the side of 32768 each slow / fast case needs, Ref64 equals the oracle on structured frames, and the reference alone leaves the
absolute bound attainable wherever a case applies it."""
import functools

import pytest
import torch

import core_frames as CF
from ref64 import Ref64, Rounded

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ABS_BOUND = {"fp32": 1e-4, "fp16": 4e-3, "bf16": 3e-2}                  # gate_rows of tests/ref64.py


# ------------------------------------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CF.NAMED)
def test_frames_are_unique_seeded_and_inside_their_bounds(name):
    co, bounds, s = CF.frame(name)
    big = name in CF.N_FRAMES
    assert co.dtype == torch.int32 and co.shape[1] == 4 and 1 <= co.shape[0] <= (33_000 if big else 11_000)
    assert torch.unique(co, dim=0).shape[0] == co.shape[0]
    inside = CF.cell_keys(co, bounds, s) >= 0
    assert int((~inside).sum()) == (3 if name == "outside" else 0)
    lo, hi = torch.tensor(bounds[0]), torch.tensor(bounds[1])
    assert bool(((co >= lo).all(1) & (co <= hi).all(1)).eq(inside).all())
    if name not in ("far", "exact_far"):
        assert int(co[:, :3].min()) < 0                                 # floor division below zero
    if co.shape[0] > 8:                                                 # odd coordinates (halves under coord_div = 2); ids shuffled
        assert bool((co[:, :3] % 2 == 1).any())
        if len(CF.block_sizes((name, 1))) > 1:
            key = CF.cell_keys(co, bounds, s)
            assert bool((key[1:] < key[:-1]).any())
    assert torch.equal(CF.frame(name)[0], CF.frame.__wrapped__(name)[0])


@pytest.mark.parametrize("fkey", [(n, 1) for n in CF.NAMED] + [("lat", 7, 3), ("lat_tight", 6, 2), ("lat", 3, 2)], ids=str)
def test_grid_restatement_matches_the_library(fkey):
    from link_amd import _lib as L
    _, bounds, s = CF.geometry(fkey)
    g = L.grid_from_bounds(bounds[0], bounds[1], s)
    lo, dim = CF.grid_of(bounds, s)
    assert list(g.lo) == lo and list(g.dim) == dim


@pytest.mark.parametrize("s,r", [(4, 3), (6, 2), (7, 3), (5, 2), (3, 3), (3, 2)])
def test_lattice_frame_and_its_two_bounds(s, r):
    co, wide, _ = CF.lat(s, r)
    _, tight, _ = CF.lat_tight(s, r)
    dw, dt = CF.grid_of(wide, s)[1], CF.grid_of(tight, s)[1]
    assert [a - b for a, b in zip(dw, dt)] == [4, 4, 4, 0]              # two empty cells on every side
    cnt = CF.cell_counts(co, tight, s)
    assert sorted(set(cnt.tolist())) == list(range(9)) and int(co[:, :3].min()) < 0
    # the same blocks in the same order under either bounds, and under either order the same multiset of sizes
    a, b = CF.numbering(co, wide, s)[1], CF.numbering(co, tight, s)[1]
    assert torch.equal(a, b) and sorted(CF.numbering(co, wide, s, "first")[1].tolist()) == sorted(a.tolist())
    assert not torch.equal(CF.numbering(co, wide, s, "first")[1], a)    # "first" IS another order on a shuffled frame


def test_numbering_orders():
    """cell order: batch fastest, then z, y, x (cell_of); first: by the smallest voxel id."""
    co = torch.tensor([[8, 0, 0, 0], [0, 0, 4, 1], [0, 0, 4, 0], [0, 0, 0, 0], [9, 0, 0, 0], [0, 4, 0, 0], [-1, 0, 0, 0]], dtype=torch.int32)
    bounds = ((-4, 0, 0, 0), (11, 7, 7, 1))
    blk, sizes = CF.numbering(co, bounds, 4, "cell")
    assert blk.tolist() == [5, 3, 2, 1, 5, 4, 0] and sizes.tolist() == [1, 1, 1, 1, 1, 2]
    blk, sizes = CF.numbering(co, bounds, 4, "first")
    assert blk.tolist() == [0, 1, 2, 3, 0, 4, 5] and sizes.tolist() == [2, 1, 1, 1, 1, 1]
    blk, _ = CF.numbering(co, ((0, 0, 0, 0), (11, 7, 7, 1)), 4, "cell")
    assert blk[-1] == -1 and blk[:-1].min() == 0                        # outside the grid: in no block


def test_block_sizes_as_named():
    assert CF.block_sizes(("edges16", 1)) == list(CF.EDGES16_SIZES)
    ends = CF.block_ends(("edges16", 1))
    assert set(ends) >= {16, 32, 64, 128, 256} | {17, 33, 65, 129, 257} and ends[-1] == 257
    for n in CF.BIG_BLOCK_N:
        assert CF.block_sizes(("big_block%d" % n, 1)) == [n]
    sizes = CF.block_sizes(("singles", 1))
    assert len(sizes) >= 4096 and set(sizes) == {1}
    co, bounds, s = CF.frame("singles")                                 # a SOLID box: every interior block has all 26 neighbours
    assert int(CF.cell_counts(co, bounds, s).min()) == 1
    sizes = CF.block_sizes(("through", 1))
    assert sizes[:33] == list(CF.THROUGH_SIZES) * 11 and sizes[33:] == [50, 50, 50]
    assert CF.block_sizes(("chunks", 1)) == [v for v in CF.CHUNK_SIZES if v]
    assert {31, 32, 33, 64, 65, 343} <= set(CF.CHUNK_SIZES) and 343 == 7 ** 3
    assert max(CF.block_sizes(("s8_352", 1))) == 352 == CF.LEAN_KMAX
    cnt = CF.cell_counts(*CF.frame("slab")[:2], 7).view(2, 5, 5, 5)
    assert int(cnt[1].sum()) == 1 and int(cnt[0].sum()) > 25            # the second batch item holds one voxel
    co, bounds, _ = CF.frame("corners")
    assert bool((co == torch.tensor(bounds[0])).all(1).any()) and bool((co[:, :3] == torch.tensor(bounds[1][:3])).all(1).any())
    assert CF.frame("one")[0].shape[0] == 1 and CF.block_sizes(("pair", 1)) == [2]


@pytest.mark.parametrize("n", list(CF.EXACT_N))
def test_exact_voxel_counts(n):
    co, bounds, s = CF.frame("n%d" % n)
    assert co.shape[0] == n
    cnt = CF.cell_counts(co, bounds, s).tolist()
    assert cnt[:-1] == [i % 9 for i in range(len(cnt) - 1)] and cnt[-1] == n - sum(cnt[:-1]) <= s ** 3


def test_outside_frame():
    co, bounds, s = CF.frame("outside")
    base = CF.lat(7, 3)[0]
    n = co.shape[0]
    gone = list(CF.OUTSIDE_IDS(n))
    assert n == base.shape[0] + 3 and torch.nonzero(CF.cell_keys(co, bounds, s) < 0).view(-1).tolist() == gone
    keep = torch.ones(n, dtype=torch.bool)
    keep[gone] = False
    assert torch.equal(co[keep], base)
    assert co[gone[0], 0] > bounds[1][0] and co[gone[1], 1] < bounds[0][1] and co[gone[2], 3] > bounds[1][3]


# ------------------------------------------------------------------------------------------------------------------------------
# the tile form's ranges and the gather kernel's passes on the frames named for them
# ------------------------------------------------------------------------------------------------------------------------------
def _ranges(fkey):
    sizes = CF.block_sizes(fkey)
    return CF.tile_ranges(sizes, CF.tiles_span(sum(sizes)))


def test_tile_ranges_reach_their_branches():
    for n in CF.BIG_BLOCK_N:
        st = _ranges(("big_block%d" % n, 1))
        assert st["wgs"] == (n + 63) // 64 and st["empty_wg"] == st["wgs"] - 1          # every other workgroup: a >= e
        tiles = (n + 15) // 16
        tpw = (tiles + 3) // 4                                           # whole tiles per wave
        assert st["waves"] == (tiles + tpw - 1) // tpw and st["through"] == max(st["waves"] - 2, 0)
        assert st["both"] == 0
    st = _ranges(("through", 1))
    assert st["through"] >= 20 and st["empty_wg"] >= 20 and st["head"] > st["through"] and st["tail"] > st["through"]
    st = _ranges(("edges16", 1))
    assert st["through"] > 0 and st["empty_wg"] > 0
    st = _ranges(("singles", 1))                                        # nothing straddles anything
    assert st["head"] == st["tail"] == st["empty_wg"] == 0 and st["waves"] == 4 * st["wgs"]
    # a wave whose two partial rows belong to DIFFERENT blocks: the lattice frames, `chunks` and the n... frames
    for fkey in (("lat", 7, 3), ("lat", 6, 2), ("chunks", 1), ("n4096", 1), ("n32768", 1), ("n32800", 1)):
        assert _ranges(fkey)["both"] > 0, fkey
    assert CF.tile_ranges([64, 64], 64) == dict(wgs=2, empty_wg=0, waves=8, through=4, head=6, tail=6, both=0)
    assert CF.tile_ranges([50, 50], 64)["both"] == 1


def test_tile_span_and_gather_configuration():
    assert [CF.tiles_span(n) for n in (1, 32768, 32769, 32800, 128 * 4096, 128 * 4096 + 1)] == [64, 64, 128, 128, 128, 256]
    assert [CF.gather_cfg(c) for c in CF.WIDTHS] == [(64, 16), (32, 16), (16, 8), (8, 4)]
    for c in CF.WIDTHS:                                                 # tiles of one-voxel blocks: every wave takes several passes
        most, fewest, passes = CF.gather_passes(CF.block_sizes(("singles", 1)), c)
        wp, rmax = CF.gather_cfg(c)
        assert most == fewest == wp > rmax and passes == wp // rmax >= 2
    for name in CF.BIG_BLOCKS:
        assert CF.gather_passes(CF.block_sizes((name, 1)), 64) == (1, 1, 1)
    t = CF.route("tiles", 64, 2, "cos", 3, 4097, 1000)
    assert t["gather_wgs"] % 8 == 0 and t["gather_wgs"] * 4 * t["wp"] >= 4097 and t["wgs"] == 65
    assert "refused" in CF.route("tiles", 48, 1, "cos", 3, 100, 100) and "refused" in CF.route("lean", 64, 1, "cos", 3, 100, 100, k=512)


# ------------------------------------------------------------------------------------------------------------------------------
# route(): the lattice, and the branches it exists for
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CF.LATTICE, ids=[CF.case_id(c) for c in CF.LATTICE])
def test_lattice_cases_reach_the_branch_they_name(case):
    got = CF.case_route(case)
    assert "refused" not in got and got["div"] == (case["div"] != 1.0) and not got["slow"]
    assert {k: got.get(k) for k in case["want"]} == case["want"], (got, case["want"])
    assert case["want"] or case["rows"] != "fp32"                       # a case names a branch, or is there for its row type
    if case["form"] != "four":
        assert case["c"] in CF.WIDTHS
    assert case["op"] != "cos_x" or case["groups"] == 1


def test_lattice_size_and_ids():
    ids = [CF.case_id(c) for c in CF.LATTICE]
    assert len(set(ids)) == len(ids) and 200 <= len(ids) <= 300


def test_nb_of_every_grouping():
    assert {(c, g): CF.nb_of(c, g) for c in CF.WIDTHS for g in CF.GROUPS[c]} == {
        (16, 1): (1, False), (16, 2): (1, True), (32, 1): (2, False), (32, 2): (1, False), (32, 4): (2, True),
        (64, 1): (4, False), (64, 2): (2, False), (64, 4): (1, False), (64, 8): (4, True),
        (128, 1): (8, False), (128, 2): (4, False), (128, 4): (2, False), (128, 8): (8, True), (128, 16): (8, True)}


def test_lattice_covers_every_branch():
    """Every branch the general layout's gate exists for is named -- in `want` -- by a case, per form."""
    named = [(c, CF.case_route(c)) for c in CF.LATTICE]

    def some(form, rows=None, order=None, bounds=None, div=None, r=None, op=None, **want):
        return any(c["form"] == form and all(c["want"].get(k) == v for k, v in want.items()) and all(g.get(k) == v for k, v in want.items())
                   and (rows is None or c["rows"] == rows) and (order is None or c["order"] == order)
                   and (bounds is None or c["bounds"] == bounds) and (div is None or c["div"] == div) and (r is None or c["r"] == r)
                   and (op is None or c["op"] == op) for c, g in named)

    for c in CF.WIDTHS:
        t = c // 16
        nbs = {(t, False), (t, True)} | ({(t // 2, False)} if t >= 2 else set()) | ({(t // 4, False)} if t >= 4 else set())
        assert {CF.nb_of(c, g) for g in CF.GROUPS[c]} == nbs
        for nb, own in nbs:
            for form in ("tiles", "lean"):                             # NB in {T, T/2, T/4, any other grouping}, at every width
                assert any(k["form"] == form and k["c"] == c and k["want"].get("nb") == nb and k["want"].get("own_theta") == own
                           for k, _ in named), (form, c, nb, own)
            if c <= 64:                                                 # lean_pm_nb
                assert any(k["form"] == "lean" and k["c"] == c and k["want"].get("pm") and k["want"].get("nb") == nb
                           and k["want"].get("own_theta") == own for k, _ in named), (c, nb, own)
        for form in ("tiles", "lean"):
            for rows in ("fp16", "bf16"):
                assert any(k["form"] == form and k["c"] == c and k["rows"] == rows for k, _ in named)
            assert any(k["form"] == form and k["c"] == c and k["rows"] != "fp32" and k["div"] == 2.0 for k, _ in named)
            for op in ("cos", "sin", "cos_x"):
                assert {k["r"] for k, _ in named if k["form"] == form and k["c"] == c and k["op"] == op} == {2, 3}
    assert any(k["groups"] == 8 and k["c"] in (64, 128) for k, _ in named) and any(k["groups"] == 16 and k["c"] == 128 for k, _ in named)
    for form in CF.FORMS:
        for bounds in ("wide", "tight"):
            assert any(k["form"] == form and k["bounds"] == bounds for k, _ in named)
        assert any(k["form"] == form and k["div"] == 2.0 for k, _ in named)
    for form in ("tiles", "four"):
        for order in ("cell", "first"):
            assert any(k["form"] == form and k["order"] == order for k, _ in named)
    # lean: the channel split by default (C = 64, n <= 4096), forced on at C = 128, forced off; the form without X below C = 64
    assert some("lean", cs=True) and any(k["c"] == 64 and k["kw"].get("lean_cs") is None and g.get("cs") for k, g in named)
    assert any(k["c"] == 128 and k["kw"].get("lean_cs") is True and g.get("cs") for k, g in named)
    assert any(k["c"] == 64 and k["kw"].get("lean_cs") is False and not g.get("cs") for k, g in named)
    assert any(k["c"] in (16, 32) and g.get("pm") for k, g in named) and any(k["kw"].get("lean_pm") is False for k, _ in named)
    # four-kernel form: idle lanes, every MFMA width off the product widths, the cpl fallback, lane = channel, r = 1, the flag sets
    for c, lpr, idle in ((20, 8, 3), (48, 16, 4), (96, 32, 8), (256, 64, 0)):
        assert any(k["c"] == c and k["want"].get("lpr") == lpr and k["want"].get("idle_lanes") == idle for k, _ in named)
    for c in (80, 96, 112):
        assert some("four", premix="mfma%d" % c)
    assert some("four", premix="cpl1") and some("four", premix="cpl4")
    assert any(k["c"] % 4 != 0 and k["want"].get("modsum") == "lane" for k, _ in named)
    assert some("four", r=1, modsum="lane") and some("four", r=1, modsum="group")
    assert some("four", pair=True) and some("four", pair=False, modsum="group")
    for c in (96, 64):
        got = {(g["modsum"], g["gather"], g["pair"], g.get("bg_dense")) for k, g in named if k["c"] == c and "flags" in k["kw"]}
        assert {("group", "fused-group"), ("lane", "fused-lane"), ("group", "split")} <= {t[:2] for t in got}
        assert {t[3] for t in got if t[1] == "split"} >= {True, False}
        if c == 64:
            assert {t[2] for t in got} == {True, False}
    # the cooperative-block switch and the cases of b - d: not on the lattice frame -- route() on their own frames
    sizes = CF.block_sizes(("big_block4096", 1))
    assert CF.route("four", 64, 2, "cos", 3, 4096, 1, blocks=len(sizes))["coop"]
    assert not CF.route("four", 64, 2, "cos", 3, 4096, 4096, blocks=4096)["coop"]       # `singles`
    assert not CF.route("four", 256, 2, "cos", 3, 4096, 1, blocks=1)["coop"]            # 64 lanes a row: no groups to cooperate
    lean = lambda n, c=64, **kw: CF.route("lean", c, 2, "cos", 3, n, 8192, k=64, **kw)   # noqa: E731
    assert lean(4096)["cs"] and not lean(4097)["cs"] and lean(4097, lean_cs=True)["cs"] and not lean(4096, lean_cs=False)["cs"]
    assert lean(4097, c=128, lean_cs=True)["cs"] and not lean(100, c=128)["cs"] and not lean(100, c=32, lean_cs=True)["cs"]
    assert not lean(100, lean_cs=True, lean_pm=True)["cs"] and not lean(100, c=128, lean_pm=True)["pm"]
    for c in (16, 32):
        assert not lean(16384, c=c)["capped"] and lean(16400, c=c)["capped"] and lean(16384, c=c)["item_wgs"] == 4096
        assert not lean(16384, c=c, lean_pm=True)["capped"] and lean(16400, c=c, lean_pm=True)["capped"]
    assert [CF.cnt_shift_of(v) for v in (729, 32768, 32769, 262144, 262145)] == [5, 5, 3, 3, 0]
    assert lean(100)["kch"] == 2 and CF.route("lean", 64, 2, "cos", 3, 100, 100, k=343)["kch"] == 11 == CF.route("lean", 64, 2, "cos", 3, 100, 100, k=352)["kch"]
    assert CF.route("tiles", 16, 2, "cos", 3, 32768, 1)["span"] == 64 and CF.route("tiles", 16, 2, "cos", 3, 32800, 1)["span"] == 128


def test_counter_packing_bounds():
    """The three bounds of the lean form's counter-packing case (tests/test_gpu_core_lattice.py builds them the same way)."""
    for r in (2, 3):
        own = CF.lat(3, r)[1]
        shifts = []
        for extra in (0, 31, 61):
            lo = tuple(v - 3 * (extra // 2) for v in own[0][:3]) + (0,)
            hi = tuple(v + 3 * (extra - extra // 2) for v in own[1][:3]) + (0,)
            dim = CF.grid_of((lo, hi), 3)[1]
            assert int((CF.cell_keys(CF.lat(3, r)[0], (lo, hi), 3) < 0).sum()) == 0
            shifts.append(CF.cnt_shift_of(dim[0] * dim[1] * dim[2] * dim[3]))
        assert shifts == [5, 3, 0]


# ------------------------------------------------------------------------------------------------------------------------------
# theta: the side of 32768 every case needs (the general-layout kernels vote per tile on the theta values themselves)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,groups,op,r", CF.LARGE_SHAPES)
def test_theta_of_the_large_theta_cases(c, groups, op, r):
    for name, pos, _, slow in CF.LARGE_THETA:
        lo, hi = CF.theta_range((name, 1), c, groups, op, pos)
        if slow is True:
            assert lo > 1.1 * CF.FAST_RANGE, (name, pos, lo)              # every voxel has a channel beyond: every tile votes `big`
        elif slow is False:
            assert hi < 0.9 * CF.FAST_RANGE, (name, pos, hi)
        else:
            assert hi > 1.1 * CF.FAST_RANGE, (name, pos, hi)           # some tiles vote `big`
    assert CF.theta_range(("far", 1), c, groups, op, "init")[1] > 500.0              # ... and the fast path is not trivial there


def test_every_copy_of_the_lean_vote_meets_a_slow_frame_under_cos_and_sin():
    """Group e: the channel-split, the default and the no-scratch-matrix kernel each run on a frame with slow tiles under cos and
    under sin, where sin and cos make up the row (under cos_x they carry ~1e-5 of it)."""
    slow = [(name, pos) for name, pos, _, s in CF.LARGE_THETA if s is not False]
    assert ("far", "x20") in slow and ("exact_far", "exact_big") in slow
    for op in ("cos", "sin"):
        seen = set()
        for c, groups, o, r in CF.LARGE_SHAPES:
            if o != op:
                continue
            for name, pos in slow:
                n = CF.frame(name)[0].shape[0]
                assert CF.theta_range((name, 1), c, groups, op, pos)[1] > 1.1 * CF.FAST_RANGE
                for kw, want in CF.large_lean_forms(c):
                    got = CF.route("lean", c, groups, op, r, n, 1000, k=343, **kw)
                    assert {k: got[k] for k in want} == want
                    seen.add((name, pos, got["cs"], got["pm"]))
        for name, pos in slow:
            assert {t[2:] for t in seen if t[:2] == (name, pos)} == {(True, False), (False, False), (False, True)}, (op, name, pos)


@pytest.mark.parametrize("c,groups,op,r", CF.LARGE_SHAPES)
def test_exact_big_theta_is_exact_in_fp32(c, groups, op, r):
    co = CF.frame("exact_far")[0]
    blk = CF.block_of(c, groups, op, "exact_big")
    w = blk.pos_weight[0].weight.detach()
    assert bool((w[:, 0] == w[:, 1]).all()) and set(w.abs().unique().tolist()) <= {0.125, 0.25, 0.5}
    al = blk.alpha.detach().view(-1) if op == "cos_x" else torch.ones(w.shape[0])
    assert set(al.tolist()) <= {0.5, 1.0}
    for div in (1.0, 2.0):
        x32, x64 = co[:, :3].float() / div, co[:, :3].double() / div
        th64 = (x64 @ w.double().t()) * al.double()
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            th = torch.zeros(co.shape[0], w.shape[0])
            for a in order:
                th = th + x32[:, a:a + 1] * w[:, a]
            assert torch.equal((th * al).double(), th64)
        if div == 1.0:
            assert float(th64.abs().max(1).values.min()) > 1.1 * 32768.0


@pytest.mark.parametrize("name", [n for n in CF.NAMED if n not in ("far", "exact_far")])
def test_the_other_frames_stay_on_the_fast_path(name):
    _, bounds, s = CF.frame(name)
    for c, groups, op in ((64, 2, "cos"), (64, 1, "cos_x"), (16, 2, "sin"), (128, 2, "cos"), (32, 1, "cos_x")):
        blk = CF.block(c, groups, op)
        assert CF.theta_bound(bounds, s, 1.0, blk.pos_weight[0].weight, blk.alpha if op == "cos_x" else None) < 0.9 * CF.FAST_RANGE


# ------------------------------------------------------------------------------------------------------------------------------
# the reference on these frames
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fkey", [("through", 1), ("slab", 1), ("lat", 5, 2)], ids=str)
@pytest.mark.parametrize("op,groups,r,div", [("cos", 2, 3, 1.0), ("cos_x", 1, 2, 2.0)])
def test_ref64_equals_the_oracle_on_structured_frames(fkey, op, groups, r, div):
    """Negative coordinates, a second batch item, blocks of 343 voxels; coord_div through the oracle's encoder variant."""
    from oracle import link_oracle as O
    C = 16
    co, _, s = CF.geometry(fkey)
    f = CF.rows_for(fkey, C).double()
    p = {k: v.double() for k, v in CF.params_of(CF.block(C, groups, op)).items()}
    want = O.elk_core_torch(f, co, p, s, r, op, groups, variant="encoder" if div != 1.0 else "unet", tensor_stride=int(div))
    d, m, ok = Ref64(f, co, p, s, r, op, groups, coord_div=div, chunk=777).compare(want)
    assert ok and d / m <= 1e-12


@functools.lru_cache(maxsize=None)
def _o32(fkey, c, groups, op, pos, r, div, rows):
    co, _, s = CF.geometry(fkey)
    dt = DTYPES[rows]
    f = CF.rows_for(fkey, c).to(dt)
    p = CF.params_of(CF.block_of(c, groups, op, pos))
    kw = dict(baseop=op, groups=groups, coord_div=div)
    ref = Ref64(f, co, p, s, r, **kw)
    o32, ok = ref.rel(Ref64(f, co, p, s, r, dtype=torch.float32, **kw))
    o_round = 0.0 if dt == torch.float32 else ref.rel(Rounded(ref, dt))[0]
    return o32, o_round, ok, ref.compare(ref)[1]


GATED = CF.gated_references()


@pytest.mark.parametrize("group", "abcdef")
def test_the_reference_leaves_the_absolute_bound_attainable(group):
    """For every case that applies the absolute bound: 4 o32 + 2 o_round + 2e-6, fp64 against fp32 Ref64 on the CPU, is below it.
    A case that drops it (absolute=False) is one where fp32 evaluation ALONE already exceeds it: `far` under cos / sin."""
    n = 0
    for g, fkey, c, groups, op, pos, r, div, rows, absolute in GATED:
        if g != group:
            continue
        n += 1
        o32, o_round, ok, m = _o32(fkey, c, groups, op, pos, r, div, rows)
        assert ok, (fkey, c, op)
        if (fkey[0], op) in CF.ANALYTIC_ZERO:
            assert m < 1e-9
            continue
        assert m > 0.5, (fkey, c, op, m)                                 # rows of the size of the norm weights
        own = 4.0 * o32 + 2.0 * o_round + 2e-6
        if absolute:
            assert own < ABS_BOUND[rows], (fkey, c, groups, op, pos, r, div, rows, o32, o_round)
        else:
            assert own >= ABS_BOUND[rows] and o32 >= ABS_BOUND[rows], (fkey, c, groups, op, pos, o32)
    assert n > 0


def test_which_large_theta_cases_drop_the_absolute_bound():
    """`far` under cos / sin: fp32 evaluation of the formula costs more than 1e-4 at theta ~ 2 000 rad, and ~2.4e-3 with the weights
    times 20 -- those cases keep rel64 <= 4 o32 + 2e-6 alone.  Under cos_x it costs ~2.5e-7 (the rows are dominated by v - fin theta)
    and the bound stays."""
    for c, groups, op, r in CF.LARGE_SHAPES:
        o_far = _o32(("far", 1), c, groups, op, "init", r, 1.0, "fp32")[0]
        o_x20 = _o32(("far", 1), c, groups, op, "x20", r, 1.0, "fp32")[0]
        if op == "cos_x":
            assert o_far < 1e-6 and o_x20 < 1e-6
        else:
            assert 1e-4 < o_far < 1e-3 and 1e-3 < o_x20 < 2e-2
    assert [f[2] for f in CF.LARGE_THETA] == [("cos", "sin"), ("cos", "sin"), (), (), ()]


# ------------------------------------------------------------------------------------------------------------------------------
# the restated constants against the literal lines of the sources; the committed figures
# ------------------------------------------------------------------------------------------------------------------------------
def _src(name):
    import os
    import link_amd
    with open(os.path.join(os.path.dirname(link_amd.__file__), "csrc", name)) as f:
        return f.read()


def test_restated_constants_are_the_sources():
    lean, disp, tiles, tdisp, elk, dsp = (_src(n) for n in ("elk_lean_impl.h", "elk_lean_dispatch.h", "elk_tiles_impl.h",
                                                          "elk_tiles_dispatch.h", "elk.hip", "dispatch.h"))
    assert "constexpr int LEAN_CH = %d;" % CF.LEAN_CH in lean and "constexpr int LEAN_KMAX = %d;" % CF.LEAN_KMAX in lean
    assert "constexpr int LEAN_SEGS = %d;" % CF.LEAN_SEGS in lean and "constexpr int LEAN_IW = %d;" % CF.LEAN_IW in lean
    assert "if (w > %d) w = %d;" % (CF.ITEM_WGS_CAP, CF.ITEM_WGS_CAP) in disp and "return d.c == 64 && n <= 4096;" in disp
    assert "const int vpw = pm ? 256 : (lean_use_cs(d, n) ? 16 : 64);" in disp
    assert "if (n <= 32768) return 64;" in tdisp and "(n + 128 * 4096 - 1) / (128 * 4096)" in tdisp
    assert "#define ELK_G_STEPS 4 " in tiles and "RMAX = WP / 2 < 16 ? WP / 2 : 16;" in tiles and "static constexpr int NW = 4;" in tiles
    assert "g_coop_threshold = %d;" % CF.COOP_THRESHOLD in elk and "constexpr int DENSE_RATIO = %d;" % CF.BG_DENSE_RATIO in elk
    assert "dispatch_int<%s>(c, f)" % ", ".join(str(w) for w in CF.MFMA_WIDTHS) in dsp
    from link_amd import _lib as L
    from link_amd.elk import ElkCorePlan
    import inspect
    assert (L.ELK_LANE_CHANNEL, L.ELK_NO_PAIR, L.ELK_FUSED_GATHER, L.ELK_NO_DENSE_GRID) == (CF.LANE_CHANNEL, CF.NO_PAIR, CF.FUSED_GATHER,
                                                                                            CF.NO_DENSE_GRID)
    assert (L.LEAN_KMAX, L.LEAN_SEGS, L.LEAN_CHUNK) == (CF.LEAN_KMAX, CF.LEAN_SEGS, CF.LEAN_CH)
    assert "self.cnt_shift = 5 if v <= 32768 else (3 if v <= 262144 else 0)" in inspect.getsource(ElkCorePlan._init_lean)


def test_committed_figures_cover_the_lattice_and_sit_inside_their_bounds():
    """profiles/core_parity.jsonl (one run on an MI355X): a row per lattice case with the route this file derives, every row inside
    the gate it was held to, no row differing between the cold, second cold and warm runs."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "core_parity.jsonl")
    with open(path) as f:
        rows = [json.loads(line) for line in f]
    a = [r for r in rows if r["group"] == "a"]
    assert len(a) == len(CF.LATTICE) and {r["group"] for r in rows} == set("abcdef") and {r["form"] for r in rows} == set(CF.FORMS)
    for r, case in zip(a, CF.LATTICE):
        assert (r["form"], r["C"], r["groups"], r["op"], r["r"], r.get("div", 1.0), r.get("rows", "fp32"), r.get("order", "cell")) == tuple(
            case[k] for k in ("form", "c", "groups", "op", "r", "div", "rows", "order"))
        assert r["route"] == json.loads(json.dumps(CF.route_brief(CF.case_route(case))))
        assert r.get("kw", {}) == {k: v for k, v in case["kw"].items() if v is not None}
    for r in rows:
        if r.get("zero"):
            assert r["e"] <= r["bound"]
            continue
        assert r["rel64"] <= 4.0 * r["o32"] + 2.0 * r["o_round"] + 2e-6
        if not (r["frame"].startswith("far") and r.get("op") in ("cos", "sin")):
            assert r["rel64"] < ABS_BOUND[r.get("rows", "fp32")]
        assert r.get("clean", True)                                       # repeats bit-equal, status and counters zero
