"""Frames and the case lattice of tests/test_gpu_dense_lattice.py: structured dense-cell frames (exact per-cell occupancy, large
theta), the parameters they run under, and a pure-Python restatement of which kernels the dense-cell launchers pick
(csrc/dense.hip: link_elk_core_dense_forward; csrc/dense_fused_impl.h: launch_k2, k2_takes_quads, dispatch_k1_nb).  No GPU code:
tests/test_cpu_dense_frames.py checks every claim made here (counts, bounds, theta bounds, routes) without a device.

A frame is (coords int32 [n, 4], bounds): unique voxels, voxel ids shuffled, bounds = ((lo x, y, z, 0), (hi x, y, z, batches - 1))
inclusive -- what ElkCorePlan takes.  "Cell" = a block of s^3 voxels; cell order = the kernels' (batch, x, y, z with z fastest:
dc_cell of csrc/dense_common.h)."""
import functools

import torch

LCAP = 352                                    # records a wave's LDS list holds: the fused kernels' slot capacity (csrc/dense_k1_impl.h)
DC_INL = 4                                    # inline records of a cell (csrc/dense_common.h)
FAST_RANGE = 32768.0                          # |theta| the fast sincos serves (dc_theta_leaves_fast_range)


# ------------------------------------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------------------------------------
def _shift3(shift):
    return tuple(int(v) for v in shift) if isinstance(shift, (tuple, list)) else (int(shift),) * 3


def cells_frame(dims, s, per, seed, shift, batches=1, pin=None):
    """Unique voxels placed by a per-cell count function: cell i = (batch, bx, by, bz) in cell order holds per(i, bx, by, bz, b)
    voxels (clipped to s^3) at random places of the cell -- `pin` {(bx, by, bz, b): [local linear positions]} fixes the first of them
    (linear = x + s y + s^2 z inside the cell).  The box of `dims` cells starts at voxel `shift` (a number, or one per axis; a
    multiple of s keeps the generator's cells the kernel's).  tests/test_gpu_k1_prologue.py's construction, generalised."""
    g = torch.Generator().manual_seed(seed)
    sh = _shift3(shift)
    rows, i = [], 0
    for b in range(batches):
        for bx in range(dims[0]):
            for by in range(dims[1]):
                for bz in range(dims[2]):
                    k = min(int(per(i, bx, by, bz, b)), s ** 3)
                    i += 1
                    lin = torch.randperm(s ** 3, generator=g)
                    first = torch.tensor((pin or {}).get((bx, by, bz, b), []), dtype=torch.int64)
                    if first.numel():
                        lin = torch.cat([first, lin[~torch.isin(lin, first)]])
                    lin = lin[:k]
                    rows.append(torch.stack([s * bx + lin % s + sh[0], s * by + (lin // s) % s + sh[1],
                                             s * bz + lin // (s * s) + sh[2], torch.full_like(lin, b)], 1))
    co = torch.cat(rows)
    co = co[torch.randperm(co.shape[0], generator=g)].int().contiguous()
    bounds = (sh + (0,), tuple(sh[a] + s * dims[a] - 1 for a in range(3)) + (batches - 1,))
    return co, bounds


def grid_of(bounds, s):
    """(lo, dim) of the block grid covering `bounds` (link_grid_from_bounds restated): lo in blocks, batch axis unscaled."""
    lo = [bounds[0][a] // s for a in range(3)] + [bounds[0][3]]
    hi = [bounds[1][a] // s for a in range(3)] + [bounds[1][3]]
    return lo, [h - l + 1 for l, h in zip(lo, hi)]


def cell_counts(coords, bounds, s):
    """Voxels per grid cell in cell order (int64 [batch, x, y, z] flattened: z fastest)."""
    lo, dim = grid_of(bounds, s)
    c = coords.long()
    u = [torch.div(c[:, a], s, rounding_mode="floor") - lo[a] for a in range(3)] + [c[:, 3] - lo[3]]
    assert all(bool(((u[a] >= 0) & (u[a] < dim[a])).all()) for a in range(4)), "voxels outside the bounds"
    key = ((u[3] * dim[0] + u[0]) * dim[1] + u[1]) * dim[2] + u[2]
    return torch.bincount(key, minlength=dim[0] * dim[1] * dim[2] * dim[3])


S7_SHIFT = -14                                # cells -2 ..: floor division below zero
# the grid the batch cases share (tests/test_gpu_dense_lattice.py, e): 5 x 5 x 5 cells of 7^3, two batch items
COMMON_BOUNDS = ((S7_SHIFT,) * 3 + (0,), (S7_SHIFT + 34,) * 3 + (1,))

# `full`: cells (x, y, z) -> count.  (1,1,1) holds k = 343 and (0,0,0) 342; (0,1,0) + (0,1,1) = 343 + 9 = LCAP, (2,0,1) + (2,0,2) =
# 343 + 10 = LCAP + 1: z-neighbours are consecutive in the kernels' cell order
_FULL = {(1, 1, 1): 343, (0, 0, 0): 342, (0, 1, 0): 343, (0, 1, 1): 9, (2, 0, 1): 343, (2, 0, 2): 10}
FAR_SHIFT = (1806, -1799, 903)                # multiples of 7
EXACT_SHIFT = (1 << 17, 1 << 17, -14)


def _corner_cells():
    return [(x, y, z) for x in (0, 4) for y in (0, 4) for z in (0, 4)] + [(2, 2, 2)]


@functools.lru_cache(maxsize=None)
def frame(name, seed=1):
    """The named frames: (coords, bounds, s).  Negative coordinates everywhere but `far` / `exact_far`."""
    if name == "full":                        # 3 x 3 x 3, s = 7
        return cells_frame((3, 3, 3), 7, lambda i, x, y, z, b: _FULL.get((x, y, z), i % 5), seed, S7_SHIFT) + (7,)
    if name == "solid3":                      # every cell full: k = 27
        return cells_frame((5, 5, 5), 3, lambda i, *c: 27, seed, -6) + (3,)
    if name == "solid2":                      # k = 8; rim strips on x and y (5 = 4 + 1, 13 = 12 + 1)
        return cells_frame((5, 13, 3), 2, lambda i, *c: 8, seed, -4) + (2,)
    if name in ("deep_strips13", "deep_strips5"):      # rim strips over cells of 40 .. 71 voxels
        dims = (13, 5, 3) if name == "deep_strips13" else (5, 5, 5)
        per = torch.randint(40, 72, (dims[0] * dims[1] * dims[2],), generator=torch.Generator().manual_seed(101 + seed)).tolist()
        return cells_frame(dims, 7, lambda i, *c: per[i], seed, S7_SHIFT) + (7,)
    if name == "one":                         # a single voxel
        return cells_frame((5, 5, 5), 7, lambda i, x, y, z, b: int((x, y, z) == (3, 1, 4)), seed, S7_SHIFT) + (7,)
    if name == "pair":                        # two voxels in one cell
        return cells_frame((5, 5, 5), 7, lambda i, x, y, z, b: 2 * int((x, y, z) == (0, 4, 2)), seed, S7_SHIFT) + (7,)
    if name == "corners":                     # three voxels in each corner cell and the centre cell; the exact lo and hi of the bounds
        cells = _corner_cells()
        pin = {(0, 0, 0, 0): [0], (4, 4, 4, 0): [7 ** 3 - 1]}
        return cells_frame((5, 5, 5), 7, lambda i, x, y, z, b: 3 * int((x, y, z) in cells), seed, S7_SHIFT, pin=pin) + (7,)
    if name == "slab":                        # only the z = 0 layer of cells; batch item 1 holds a single voxel
        def per(i, x, y, z, b):
            if z != 0:
                return 0
            return 1 + (5 * x + y) % 6 if b == 0 else int((x, y) == (2, 3))
        return cells_frame((5, 5, 5), 7, per, seed, S7_SHIFT, batches=2) + (7,)
    if name == "s8":                          # slot capacity 512 > LCAP; counts 0 .. 89
        return cells_frame((4, 4, 4), 8, lambda i, *c: (37 * i) % 90, seed, -16) + (8,)
    if name == "s8_full":                     # one cell of 512
        return cells_frame((3, 3, 3), 8, lambda i, x, y, z, b: 512 if (x, y, z) == (1, 2, 0) else i % 5, seed, -16) + (8,)
    if name == "s8_352":                      # one cell of exactly LCAP = 352 voxels: slot_cap = 352 holds it with no room to spare
        return cells_frame((3, 3, 3), 8, lambda i, x, y, z, b: LCAP if (x, y, z) == (1, 0, 2) else i % 5, seed, -16) + (8,)
    if name == "far":                         # |theta| ~ 2 000 rad under nn.Linear's initial weights (uniform in +-0.577)
        return cells_frame((5, 5, 5), 7, lambda i, *c: i % 9, seed, FAR_SHIFT) + (7,)
    if name == "exact_far":                   # with exact_pos_weight: theta exact in fp32, |theta| < 40, the launch-wide bound ~1.3e5
        return cells_frame((5, 5, 5), 7, lambda i, *c: i % 9, seed, EXACT_SHIFT) + (7,)
    raise KeyError(name)


# (frame, op) whose rows are analytically zero before the final LayerNorm: a voxel alone in its neighbourhood under `sin` gives
# f sin cos - f cos sin.  No relative error exists there; tests/ref64.py, gate_zero_rows
ANALYTIC_ZERO = {("one", "sin")}
OCCUPANCY = ["full", "solid3", "solid2", "deep_strips13", "deep_strips5", "one", "pair", "corners", "slab"]
NAMED = OCCUPANCY + ["s8", "s8_full", "s8_352", "far", "exact_far"]


def lattice_frame(s, r, seed=1):
    """The frame of the kernel-selection lattice: i % 9 voxels per cell, 5 x 5 x 5 cells (r = 3: rim strips on x and y) or 6 x 7 x 4
    (r = 2); cells on both sides of zero."""
    dims = (5, 5, 5) if r == 3 else (6, 7, 4)
    return cells_frame(dims, s, lambda i, *c: i % 9, seed, -2 * s)


@functools.lru_cache(maxsize=None)
def rows_of(name_or_n, c, seed, dtype=torch.float32):
    """Feature rows of a frame (CPU): `name_or_n` a frame name or a row count."""
    n = name_or_n if isinstance(name_or_n, int) else frame(name_or_n, seed)[0].shape[0]
    return torch.randn(n, c, generator=torch.Generator().manual_seed(1000 + seed)).to(dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# parameters
# ------------------------------------------------------------------------------------------------------------------------------
def exact_pos_weight(rows, seed=7):
    """[rows, 3] signed powers of two in [2^-3, 2^-1]; the x and y entries of a row are opposite and equal.  With coordinates
    (2^17 + a, 2^17 + b, c), |a|, |b|, |c| < 64 (halved or not), every product and partial sum of theta is a multiple of 2^-4 below
    2^17 -- exact in fp32 in any order of summation -- and |theta| = |wx (a - b) + wz c| < 40."""
    g = torch.Generator().manual_seed(seed)
    sign = lambda: torch.randint(0, 2, (rows,), generator=g) * 2.0 - 1.0          # noqa: E731
    mag = lambda: 2.0 ** -torch.randint(1, 4, (rows,), generator=g).float()       # noqa: E731
    wx, wz = sign() * mag(), sign() * mag()
    return torch.stack([wx, -wx, wz], 1)


@functools.lru_cache(maxsize=None)
def block(c, groups, baseop, pos="init", seed=3):
    """A seeded ELKBlock on the CPU.  cos_x: alpha uniform in (0.5, 1.5) (as tests/test_gpu_sizes.py).  pos: "init" (nn.Linear's
    initial pos_weight, uniform in +-0.577), "x20" (those times 20) or "exact" (exact_pos_weight)."""
    import link_amd as la
    torch.manual_seed(seed)
    blk = la.ELKBlock(c, c, groups=groups, baseop=baseop).eval()
    with torch.no_grad():
        if baseop == "cos_x":
            blk.alpha.uniform_(0.5, 1.5)
        w = blk.pos_weight[0].weight
        if pos == "x20":
            w.mul_(20.0)
        elif pos == "exact":
            w.copy_(exact_pos_weight(w.shape[0]))
        else:
            assert pos == "init"
    return blk


def params_of(blk):
    return {k: v.detach() for k, v in blk.state_dict().items()}


def theta_bound(bounds, s, coord_div, w_pos, alpha=None):
    """The launch-wide |theta| bound the fused kernels decide the sincos path by (dc_coord_absmax and dc_theta_leaves_fast_range of
    csrc/dense_common.h, restated in float64): max over the channels; the slow path runs when it is not below FAST_RANGE."""
    lo, dim = grid_of(bounds, s)
    a = torch.tensor([max(abs(lo[k] * s), abs((lo[k] + dim[k]) * s)) / float(coord_div) for k in range(3)], dtype=torch.float64)
    b = (w_pos.detach().double().cpu().abs() * a).sum(1)
    if alpha is not None:
        b = b * alpha.detach().double().cpu().abs().view(-1)
    return float(b.max()) * 1.01


# ------------------------------------------------------------------------------------------------------------------------------
# which kernels a dense-cell plan runs
# ------------------------------------------------------------------------------------------------------------------------------
def tuning_of(c, baseop, **kw):
    """link_dc_tuning_t as ElkCorePlan.set_tuning(**kw) leaves it for one frame in flight: (k1_form, k2_form, mode)."""
    k1 = 2 if (c in (32, 64) and baseop != "cos_x" and "k1_form" not in kw) else 0
    return kw.get("k1_form", k1), kw.get("k2_form", 16), kw.get("mode", 0)


def route(c, groups, baseop, r, k, dims, coord_div=1.0, half=False, slow=False, **tuning):
    """The kernels ONE cold step of ElkCorePlan(layout="dense") launches, restated from link_elk_core_dense_forward, dispatch_k1_nb,
    launch_k2 and k2_takes_quads: a dict, or {"refused": why}.  k = slot capacity, dims = the grid's cells per axis."""
    k1_form, k2_form, mode = tuning_of(c, baseop, **tuning)
    mode = mode or 7
    cg, parts, two_part = c // groups, (3 if baseop == "cos_x" else 2), baseop != "cos_x"
    if k < DC_INL:
        return {"refused": "slot capacity below the inline records"}
    fused = bool(mode & 1) and c <= 64 and k <= LCAP
    if half and not (fused and mode & 2):
        return {"refused": "half rows need the fused kernels"}
    out = dict(fused=fused, div=coord_div != 1.0, slow=bool(slow))
    t = c // 16
    nb = min(cg // 16, t) if cg % 16 == 0 else t       # distinct 16-channel theta blocks of a voxel (dispatch_k1_nb)
    if not (nb == t or (t >= 2 and nb == t // 2) or (t >= 4 and nb == t // 4)):
        nb = t
    # K2 first: the pre_mix launcher asks it whether the quad consumers follow
    split_fits = parts == 2                              # dc_k2_cfg::SPLIT_FITS, dc_k2q_cfg::FITS: two workgroups per CU -- not three-part rows
    pair = c == 2 * cg and two_part
    if (mode & 4) and c == 64:
        own = bool(k2_form & 4) or (not (k2_form & 1) and not split_fits and r == 3)
        quads = split_fits and not own and pair and baseop != "cos_x" and not (k2_form & 9) and not (k2_form & 2)
        if own:
            k2 = "own"
        elif quads:
            k2 = "quad"
        elif not (k2_form & 1) and split_fits:
            k2 = "split"
        else:
            k2 = "single"
        out.update(k2=k2, pair=pair)
        if k2 == "quad":
            strips = not (k2_form & 16) and r == 3 and (dims[0] % 4 == 1 or dims[1] % 4 == 1)
            out.update(rim="strips" if strips else "square")
        if k2 in ("split", "single"):
            out.update(one_role=bool(k2_form & 2))
    else:
        quads = False
        out.update(k2="gather+demod", pair=c == 2 * cg and two_part)
    if fused:
        form = k1_form & 15
        if form == 1:
            out.update(k1="tiles")
        elif form == 2 and c in (32, 64):
            out.update(k1="mm", nb=nb)
        else:
            out.update(k1="range", nb=nb)
            if c == 64 and nb == 2 and two_part:        # the instance without the record write-back exists for this shape alone
                out.update(writeback=bool(not quads or (k1_form & 16)))
    else:
        out.update(k1="premix_insert+modsum")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the kernel-selection lattice: (C, groups, op, s, r) x coord_div in {1, 2}; per case a list of (tuning, what the case is meant
# to reach).  `want` is a subset of route()'s answer; div / slow are added by the users.
# ------------------------------------------------------------------------------------------------------------------------------
def _row1(r):
    rim0 = "strips" if r == 3 else "square"              # r = 2 launches have no strips
    return [
        (dict(k1_form=0), dict(k1="range", nb=2, writeback=False, k2="quad", rim="square")),
        (dict(k1_form=1), dict(k1="tiles", k2="quad")),
        (dict(k1_form=2), dict(k1="mm", nb=2, k2="quad")),
        (dict(k1_form=16), dict(k1="range", nb=2, writeback=True, k2="quad")),
        (dict(k2_form=0), dict(k1="mm", k2="quad", rim=rim0)),
        (dict(k2_form=16), dict(k1="mm", k2="quad", rim="square")),
        (dict(k2_form=4), dict(k2="own", pair=True)),
        (dict(k2_form=8), dict(k2="split", pair=True, one_role=False)),
        (dict(k2_form=1), dict(k2="single", pair=True, one_role=False)),
        (dict(k2_form=2), dict(k2="split", pair=True, one_role=True)),
    ]


def _row2(groups):
    nb = {1: 4, 4: 1, 8: 4}[groups]                      # cg = 8 is no multiple of 16: every 16-channel block evaluates its own theta
    return [
        (dict(), dict(k1="mm", nb=nb, k2="split", pair=False)),
        (dict(k2_form=4), dict(k1="mm", nb=nb, k2="own", pair=False)),
        (dict(k2_form=1), dict(k1="mm", nb=nb, k2="single", pair=False)),
    ]


def _row3(r):
    return [
        (dict(), dict(k1="range", nb=4, k2="own" if r == 3 else "single", pair=False)),
        (dict(k2_form=1), dict(k1="range", nb=4, k2="single", pair=False)),
        (dict(k2_form=4), dict(k1="range", nb=4, k2="own", pair=False)),
    ]


def _k1_rows(forms, c):
    names = {0: "range", 1: "tiles", 2: "mm" if c in (32, 64) else "range"}
    return [(dict(k1_form=f), dict(fused=True, k1=names[f], k2="gather+demod")) for f in forms]


def _lattice():
    cases = []
    for div in (1.0, 2.0):
        for op in ("cos", "sin"):
            for r in (2, 3):
                cases.append(((64, 2, op, 7, r, div), _row1(r)))
                for groups in (1, 4, 8):
                    cases.append(((64, groups, op, 5, r, div), _row2(groups)))
        for r in (2, 3):
            cases.append(((64, 1, "cos_x", 3, r, div), _row3(r)))
        for groups, op in ((4, "sin"), (1, "sin"), (1, "cos_x")):
            cases.append(((32, groups, op, 6, 2, div), _k1_rows((0, 1, 2), 32)))
        for groups, op in ((1, "cos"), (2, "cos"), (1, "cos_x")):
            cases.append(((16, groups, op, 4, 3, div), _k1_rows((0, 1), 16)))
        for groups, op in ((4, "cos"), (1, "cos"), (1, "cos_x")):
            cases.append(((128, groups, op, 4, 3, div), [(dict(), dict(fused=False, k1="premix_insert+modsum", k2="gather+demod"))]))
    return cases


LATTICE = _lattice()
# the forms of row 1: what (d) runs the large-theta frames through
ROW1_FORMS = [t for t, _ in _row1(3)]


def case_id(case):
    c, groups, op, s, r, div = case
    return f"C{c}-g{groups}-{op}-s{s}-r{r}-div{div:g}"
