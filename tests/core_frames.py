"""Frames and the case lattice of tests/test_gpu_core_lattice.py: structured frames for the three forms of R_core on the general
layout -- the tile form (csrc/elk_tiles_impl.h), the lean form (csrc/elk_lean_impl.h) and the four-kernel form (csrc/elk.hip) --
with a pure-Python restatement of what their launchers pick and of the block numbering, so that the sorted positions of a frame are
known on the CPU.  It is to those forms what tests/dense_frames.py is to the dense-cell launchers, and reuses its generator,
parameters and theta bound.  No GPU code: tests/test_cpu_core_frames.py checks every claim made here without a device.

A frame is (coords int32 [n, 4], bounds, s): unique voxels, voxel ids shuffled, bounds inclusive as ElkCorePlan takes them.  "Block
order" = the numbering of the occupied blocks: "cell" (link_index_build: ascending cell index, cell_of of csrc/common.h: x slowest,
then y, z, the batch column FASTEST) or "first" (link_index_build_first: ascending smallest voxel id).  Sorted positions are
block-major; a block's positions hold its voxels."""
import functools

import torch

import dense_frames as DF
from dense_frames import (FAST_RANGE, block, cell_counts, cells_frame, exact_pos_weight, grid_of, params_of, rows_of,  # noqa: F401
                          theta_bound)

FORMS = ("tiles", "lean", "four")
WIDTHS = (16, 32, 64, 128)                    # the product widths: the tile and lean forms are built for these alone
LEAN_CH, LEAN_KMAX, LEAN_SEGS, LEAN_IW = 32, 352, 16, 4          # csrc/elk_lean_impl.h
ITEM_WGS_CAP = 4096                           # lean_item_wgs of csrc/elk_lean_dispatch.h
MFMA_WIDTHS = (16, 32, 48, 64, 80, 96, 112, 128)                 # dispatch_width of csrc/dispatch.h
COOP_THRESHOLD, BG_DENSE_RATIO = 4, 3         # g_coop_threshold, DENSE_RATIO of csrc/elk.hip
# link_elk_desc_t::flags (include/link_amd.h)
LANE_CHANNEL, NO_PAIR, FUSED_GATHER, NO_DENSE_GRID = 1, 2, 4, 8
# the flag sets of tests/test_gpu_split_paths.py
FLAG_SETS = {"split+group+pair": 0, "fused-group": FUSED_GATHER, "no-pair": NO_PAIR, "column-walking": NO_DENSE_GRID,
             "generic": LANE_CHANNEL | NO_PAIR | FUSED_GATHER}


# ------------------------------------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------------------------------------
def widen(bounds, s, cells=2):
    """`bounds` with `cells` empty blocks added on every side of x, y and z."""
    lo, hi = bounds
    return (tuple(v - cells * s for v in lo[:3]) + (lo[3],), tuple(v + cells * s for v in hi[:3]) + (hi[3],))


@functools.lru_cache(maxsize=None)
def lat(s, r, seed=1):
    """The dense lattice frame (i % 9 voxels per cell) with its bounds widened by two empty cells on every side: the rim blocks'
    neighbours are empty cells INSIDE the grid.  (coords, wide bounds, s); lat_tight() has the box's own bounds, where the same
    neighbours lie outside the grid (cell_of < 0)."""
    co, bounds = DF.lattice_frame(s, r, seed)
    return co, widen(bounds, s), s


def lat_tight(s, r, seed=1):
    co, bounds = DF.lattice_frame(s, r, seed)
    return co, bounds, s


BIG_BLOCK_N = (15, 16, 17, 63, 64, 65, 255, 256, 257, 1025, 4096)
# sizes of edges16's blocks in cell order: runs end at 16, 32, 64, 128 and 256 exactly, and one position past each
EDGES16_SIZES = (16, 1, 15, 1, 31, 1, 63, 1, 127, 1)
THROUGH_SIZES = (343, 342, 1)
CHUNK_SIZES = (31, 32, 33, 64, 65, 343, 0, 1, 96, 97, 343, 5)
# exact voxel counts: cells per axis (cell i holds i % 9 voxels, the LAST cell the remainder)
EXACT_N = {4096: (8, 8, 16), 4097: (8, 8, 16), 16384: (16, 16, 16), 16400: (16, 16, 16), 32768: (16, 16, 32), 32800: (16, 16, 32)}


def _exact_n(n, seed):
    dims, s = EXACT_N[n], 4
    cells = dims[0] * dims[1] * dims[2]
    rest = n - sum(i % 9 for i in range(cells - 1))
    assert 0 <= rest <= s ** 3, (n, rest)
    return cells_frame(dims, s, lambda i, *c: i % 9 if i < cells - 1 else rest, seed, -2 * s) + (s,)


@functools.lru_cache(maxsize=None)
def frame(name, seed=1):
    """The named frames: (coords, bounds, s).  Negative coordinates everywhere but `far` / `exact_far`."""
    if name in ("one", "pair", "corners", "slab", "far", "exact_far", "s8_352"):
        return DF.frame(name, seed)
    if name == "singles":                     # a solid box of 16^3 cells of s = 2, exactly one voxel each: every tile is 16 runs
        return cells_frame((16, 16, 16), 2, lambda i, *c: 1, seed, -16) + (2,)
    if name.startswith("big_block"):          # all N voxels in ONE block of 16^3
        return cells_frame((1, 1, 1), 16, lambda i, *c: int(name[9:]), seed, -16) + (16,)
    if name == "edges16":                     # one column of cells along z: cell order = z order
        return cells_frame((1, 1, len(EDGES16_SIZES)), 7, lambda i, *c: EDGES16_SIZES[i], seed, DF.S7_SHIFT) + (7,)
    if name == "through":                     # 11 x (343, 342, 1), then 50, 50, 50: blocks that cover whole waves and workgroups
        return cells_frame((3, 3, 4), 7, lambda i, *c: THROUGH_SIZES[i % 3] if i < 33 else 50, seed, DF.S7_SHIFT) + (7,)
    if name == "chunks":                      # the lean form's chunks of 32: cells of exactly 31 .. 65 and k = 343 voxels
        return cells_frame((2, 3, 2), 7, lambda i, *c: CHUNK_SIZES[i], seed, DF.S7_SHIFT) + (7,)
    if name[0] == "n" and name[1:].isdigit():
        return _exact_n(int(name[1:]), seed)
    if name == "bigrows":                     # lat(7, 3); rows_for() scales every 97th row by 1e5
        return lat(7, 3, seed)
    if name == "outside":                     # lat(7, 3) plus three voxels outside the bounds (ids 5, n // 2, n - 1 after the insert)
        co, bounds, s = lat(7, 3, seed)
        lo, hi = bounds
        extra = torch.tensor([[hi[0] + 1, 0, 0, 0], [0, lo[1] - 1, 0, 0], [0, 0, 0, 1]], dtype=torch.int32)
        n = co.shape[0]
        at = OUTSIDE_IDS(n + 3)
        out = torch.empty((n + 3, 4), dtype=torch.int32)
        keep = torch.ones(n + 3, dtype=torch.bool)
        keep[list(at)] = False
        out[keep], out[~keep] = co, extra
        return out.contiguous(), bounds, s
    raise KeyError(name)


def OUTSIDE_IDS(n):
    return (5, n // 2, n - 1)


BIG_BLOCKS = ["big_block%d" % n for n in BIG_BLOCK_N]
N_FRAMES = ["n%d" % n for n in EXACT_N]
NAMED = (["singles", "one", "pair", "corners", "slab", "edges16", "through", "chunks", "s8_352", "far", "exact_far", "bigrows",
          "outside"] + BIG_BLOCKS + N_FRAMES)
ANALYTIC_ZERO = DF.ANALYTIC_ZERO


def geometry(fkey):
    """fkey: ("lat", s, r) / ("lat_tight", s, r), or (name, seed)."""
    if fkey[0] == "lat":
        return lat(fkey[1], fkey[2])
    if fkey[0] == "lat_tight":
        return lat_tight(fkey[1], fkey[2])
    return frame(*fkey)


@functools.lru_cache(maxsize=None)
def rows_for(fkey, c):
    """fp32 feature rows of a frame (CPU, seeded).  `bigrows`: every 97th row times 1e5 -- beyond the fp16 split's range (w_big)."""
    n = geometry(fkey)[0].shape[0]
    f = rows_of(n, c, 1 if fkey[0].startswith("lat") else fkey[1])
    if fkey[0] == "bigrows":
        f = f.clone()
        f[::97] *= 1e5
    return f


# ------------------------------------------------------------------------------------------------------------------------------
# the block numbering (csrc/index.hip: link_index_build, link_index_build_first; csrc/common.h: cell_of, floordiv)
# ------------------------------------------------------------------------------------------------------------------------------
def cell_keys(coords, bounds, s):
    """cell_of of every voxel (int64; -1 outside the grid)."""
    lo, dim = grid_of(bounds, s)
    c = coords.long()
    u = [torch.div(c[:, a], s, rounding_mode="floor") - lo[a] for a in range(3)] + [c[:, 3] - lo[3]]
    inside = torch.ones(c.shape[0], dtype=torch.bool)
    for a in range(4):
        inside &= (u[a] >= 0) & (u[a] < dim[a])
    key = ((u[0] * dim[1] + u[1]) * dim[2] + u[2]) * dim[3] + u[3]
    return torch.where(inside, key, torch.full_like(key, -1))


def numbering(coords, bounds, s, order="cell"):
    """(block of every voxel [n] -- -1 for a voxel outside the grid --, block sizes [M] in numbering order)."""
    assert order in ("cell", "first")
    key = cell_keys(coords, bounds, s)
    ok = key >= 0
    uniq, inv = torch.unique(key[ok], sorted=True, return_inverse=True)
    if order == "first":                                   # blocks by their smallest voxel id
        ids = torch.nonzero(ok).view(-1)
        first = torch.full((uniq.shape[0],), coords.shape[0], dtype=torch.int64).scatter_reduce(0, inv, ids, "amin")
        rank = torch.empty_like(first)
        rank[torch.argsort(first)] = torch.arange(uniq.shape[0])
        inv = rank[inv]
    blk = torch.full((coords.shape[0],), -1, dtype=torch.int64)
    blk[ok] = inv
    return blk, torch.bincount(inv, minlength=uniq.shape[0])


def block_sizes(fkey, order="cell"):
    co, bounds, s = geometry(fkey)
    return numbering(co, bounds, s, order)[1].tolist()


def block_ends(fkey, order="cell"):
    """Sorted positions where blocks end (blk_start[1:])."""
    return torch.cumsum(torch.tensor(block_sizes(fkey, order)), 0).tolist()


# ------------------------------------------------------------------------------------------------------------------------------
# what the launchers pick
# ------------------------------------------------------------------------------------------------------------------------------
def nb_of(c, groups):
    """tiles_nb / lean_nb / lean_pm_nb: distinct 16-channel theta blocks of a voxel.  (NB, `own`: every block evaluates its own theta
    through % cg because cg is no multiple of 16 or the grouping is none of T, T/2, T/4.)"""
    t, cg = c // 16, c // groups
    nb = min(cg // 16, t) if cg % 16 == 0 else t
    if (t >= 2 and nb == t // 2) or (t >= 4 and nb == t // 4):
        return nb, False
    return t, nb != t or cg % 16 != 0


def tiles_span(n):
    """tiles_span of csrc/elk_tiles_dispatch.h."""
    if n <= 32768:
        return 64
    return 128 * max(1, (n + 128 * 4096 - 1) // (128 * 4096))


def gather_cfg(c):
    """elk_g_cfg of csrc/elk_tiles_impl.h: (WP sorted positions per wave, RMAX blocks per pass)."""
    g = 64 // (c // 4)
    wp = min(4 * g, 64)
    return wp, min(wp // 2, 16)


def lpr_of(c):
    """dispatch_lpr of csrc/dispatch.h."""
    need, l = (c + 3) // 4, 4
    while l < need:
        l <<= 1
    return l


def cnt_shift_of(cells):
    """ElkCorePlan._init_lean."""
    return 5 if cells <= 32768 else (3 if cells <= 262144 else 0)


def route(form, c, groups, op, r, n, cells, k=0, slow=False, half=False, blocks=None, lean_cs=None, lean_pm=None, flags=0,
          coord_div=1.0):
    """What ONE cold step of ElkCorePlan launches on the general layout (form "tiles" / "four") or the lean layout ("lean"),
    restated from the sources: a dict, or {"refused": why}.  n = voxels, cells = grid cells, k = slot capacity (lean), blocks =
    occupied blocks (four-kernel form: the cooperative switch)."""
    cg = c // groups
    out = dict(form=form, div=coord_div != 1.0, slow=bool(slow), r=r)
    if form == "tiles":                                    # csrc/elk_tiles_dispatch.h: tiles_span, tiles_wgs, tiles_nb, launch_gather
        if c not in WIDTHS or r not in (2, 3):
            return {"refused": "the tile form is built for C in 16 / 32 / 64 / 128 and r in 2 / 3"}
        span = tiles_span(n)
        wp, rmax = gather_cfg(c)
        nb, own = nb_of(c, groups)
        gw = ((n + wp * 4 - 1) // (wp * 4) + 7) & ~7
        out.update(span=span, wgs=(n + span - 1) // span, nb=nb, own_theta=own, wp=wp, rmax=rmax, gather_wgs=gw)
        return out
    if form == "lean":                                     # csrc/elk_lean_dispatch.h: run_lean, lean_use_cs, lean_use_pm, lean_item_wgs
        k = k or 0
        if c not in WIDTHS or r not in (2, 3) or not (1 <= k <= LEAN_KMAX) or cells >= 2 ** 27:
            return {"refused": "the lean form needs a product width, r in 2 / 3, 1 <= k <= 352"}
        pm = c <= 64 and lean_pm is True
        if c not in (64, 128) or lean_cs is False:
            cs = False
        elif lean_cs is True:
            cs = True
        else:
            cs = c == 64 and n <= 4096
        cs_runs = cs and not pm                            # lean_c_op: the form without X has its own insert launch
        vpw = 256 if pm else (16 if cs else 64)
        nwg = (n + vpw - 1) // vpw
        if pm:
            idx_cap = ((n + 63) // 64 + LEAN_SEGS - 1) // LEAN_SEGS * 64
        else:
            idx_cap = (nwg + LEAN_SEGS - 1) // LEAN_SEGS * vpw
        w = (LEAN_SEGS * idx_cap + LEAN_IW - 1) // LEAN_IW
        capped = w > ITEM_WGS_CAP
        w = max(4, min(w, ITEM_WGS_CAP))
        nb, own = nb_of(c, groups)
        out.update(cs=cs_runs, pm=pm, vpw=vpw, nwg=nwg, idx_cap=idx_cap, item_wgs=(w + 3) & ~3, capped=capped,
                   cnt_shift=cnt_shift_of(cells), kch=(k + LEAN_CH - 1) // LEAN_CH, nb=None if cs_runs else nb,
                   own_theta=False if cs_runs else own)
        return out
    assert form == "four"                                  # csrc/elk.hip: link_elk_core_forward and the entries it calls
    if half:
        return {"refused": "the four-kernel form is fp32"}
    if not (0 < c <= 256):
        return {"refused": "width"}
    lane = bool(flags & LANE_CHANNEL) or c % 4 != 0        # modsum_group_path / gather_group_path
    lpr = lpr_of(c)
    pair = (not flags & NO_PAIR) and c == 2 * cg and c == 4 * lpr and op != "cos_x"       # row_pairs
    split = (not flags & FUSED_GATHER) and c % 4 == 0 and r <= 3                          # link_elk_core_forward
    out.update(premix=("mfma%d" % c) if c in MFMA_WIDTHS else "cpl%d" % ((c + 63) // 64),  # premix_mfma / dispatch_cpl
               modsum="lane" if lane else "group", lpr=lpr, idle_lanes=lpr - (c + 3) // 4,
               pair=bool(pair) and (not lane or split),
               gather="split" if split else ("fused-lane" if (lane or r > 3) else "fused-group"))
    if not lane and blocks is not None:                    # k_modulate_sum_g
        out.update(coop=lpr < 64 and n > COOP_THRESHOLD * max(blocks, 1))
    if split:                                              # launch_block_gather: the dense-grid instance of the block gather
        inst = lpr <= 32 and r == 3 and not (flags & NO_DENSE_GRID) and cells <= BG_DENSE_RATIO * n      # host: the DENSE instance
        out.update(bg_dense_instance=inst)
        if blocks is not None:                             # device (dense_regime): the dense-grid form takes the frame when V <= 3 M
            out.update(bg_dense=inst and cells <= BG_DENSE_RATIO * blocks)
    return out


def route_brief(route):
    """route() as core_parity.jsonl keeps it: without what the row states anyway and without the entries that are False / None."""
    return {k: v for k, v in route.items() if k not in ("form", "div", "slow", "r") and v is not None and v is not False}


def tile_ranges(sizes, span):
    """k_elk_tiles' range logic restated (csrc/elk_tiles_impl.h) for blocks of `sizes` in sorted order: per workgroup the nominal
    span with both ends moved up to the next block boundary, cut into four waves of whole 16-voxel tiles.  Counts of: workgroups,
    `empty_wg` (a >= e: the span lies inside a block an earlier workgroup owns), waves with work, `through` (one block enters and
    leaves the wave), `head`, `tail` (a block straddles the wave's first / last position), `both` (head and tail by DIFFERENT
    blocks: both partial rows of the wave are used)."""
    ends = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0).tolist()
    n = ends[-1] if ends else 0
    pos_blk = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64)).tolist()

    def boundary(q):
        if q <= 0:
            return 0
        if q >= n:
            return n
        return q if pos_blk[q - 1] != pos_blk[q] else ends[pos_blk[q]]

    st = dict(wgs=(n + span - 1) // span, empty_wg=0, waves=0, through=0, head=0, tail=0, both=0)
    for w in range(st["wgs"]):
        a, e = boundary(w * span), boundary((w + 1) * span)
        if a >= e:
            st["empty_wg"] += 1
            continue
        tpw = (((e - a + 15) >> 4) + 3) // 4
        for wave in range(4):
            wa = a + wave * tpw * 16
            wb = min(wa + tpw * 16, e)
            if wa >= wb:
                continue
            head = wa > a and pos_blk[wa - 1] == pos_blk[wa]
            tail = wb < e and pos_blk[wb - 1] == pos_blk[wb]
            thr = head and tail and pos_blk[wa] == pos_blk[wb - 1]
            st["waves"] += 1
            st["head"] += head
            st["tail"] += tail
            st["through"] += thr
            st["both"] += head and tail and not thr
    return st


def gather_passes(sizes, c):
    """k_elk_gather_tiles: (the most run heads a wave of WP positions sees, the fewest, the most passes of RMAX blocks)."""
    wp, rmax = gather_cfg(c)
    pos_blk = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64))
    runs = [int(torch.unique(pos_blk[p:p + wp]).shape[0]) for p in range(0, pos_blk.shape[0], wp)]
    return max(runs), min(runs), (max(runs) + rmax - 1) // rmax


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the kernel-selection lattice on lat(s, r).  A case: dict(form, c, groups, op, s, r, div, rows, order, bounds, kw) + `want`,
# the subset of route() the case is there to reach.
# ------------------------------------------------------------------------------------------------------------------------------
GROUPS = {16: (1, 2), 32: (1, 2, 4), 64: (1, 2, 4, 8), 128: (1, 2, 4, 8, 16)}     # every value with a distinct (NB, own theta)
S_OF = {16: 4, 32: 6, 64: 7, 128: 5}                                                # block edge of a width's lattice frame


def _case(form, c, groups, op, r, div=1.0, rows="fp32", order="cell", bounds="wide", want=None, **kw):
    return dict(form=form, c=c, groups=groups, op=op, s=S_OF.get(c, 5), r=r, div=div, rows=rows, order=order, bounds=bounds,
                kw=kw, want=dict(want or {}))


def _lattice():
    cases = []
    for c in WIDTHS:
        for gi, groups in enumerate(GROUPS[c]):
            nb, own = nb_of(c, groups)
            for oi, op in enumerate(("cos", "sin", "cos_x")):
                if op == "cos_x" and groups != 1:          # the module refuses it (ELKBlock.forward)
                    continue
                r = 2 + (gi + oi) % 2                      # both r over every (groups, op) row, not the full product
                # ---- tile form: every NB; both block orders; coord_div 2 and the tight bounds on a sub-row
                order = "first" if (gi + oi) % 2 else "cell"
                cases.append(_case("tiles", c, groups, op, r, order=order, want=dict(nb=nb, own_theta=own)))
                if gi == 0 or own:
                    cases.append(_case("tiles", c, groups, op, 5 - r, div=2.0, order="cell" if order == "first" else "first",
                                       bounds="tight", want=dict(nb=nb, own_theta=own, div=True)))
                # ---- lean form: every NB under the default launch 1, the channel split and the form without X
                sub = gi == 0 or own or oi == 0
                if c == 64:                                # n <= 4096: the default IS the channel split; NB runs under lean_cs=False
                    cs_opts = [(False, True)] + ([(None, sub)] if sub else []) + ([(True, True)] if gi == 0 and oi == 0 else [])
                elif c == 128:
                    cs_opts = [(None, True)] + ([(True, sub)] if sub else []) + ([(False, True)] if gi == 0 and oi == 0 else [])
                else:
                    cs_opts = [(None, True)]
                for cs, _ in cs_opts:
                    split = cs is True or (cs is None and c == 64)
                    want = dict(pm=False, cs=split)
                    if not split:
                        want.update(nb=nb, own_theta=own)
                    cases.append(_case("lean", c, groups, op, r, want=want, lean_cs=cs))
                if c <= 64:
                    cases.append(_case("lean", c, groups, op, 5 - r, want=dict(pm=True, cs=False, nb=nb, own_theta=own), lean_pm=True))
                    if gi == 0:
                        cases.append(_case("lean", c, groups, op, r, want=dict(pm=False), lean_pm=False))
                if gi == 0 or own:
                    cases.append(_case("lean", c, groups, op, 5 - r, div=2.0, bounds="tight", want=dict(div=True)))
                # ---- four-kernel form at the product widths (fp32 training-shaped calls): PAIR or not, both block orders
                if gi <= 1:
                    cases.append(_case("four", c, groups, op, r, order=order,
                                       want=dict(premix="mfma%d" % c, modsum="group", pair=groups == 2 and op != "cos_x", gather="split")))
        # half rows: every width once per type, coord_div = 2 once
        for rows in ("fp16", "bf16"):
            for form in ("tiles", "lean"):
                cases.append(_case(form, c, 2, "cos", 3, rows=rows))
        cases.append(_case("tiles", c, 1, "cos_x", 2, div=2.0, rows="fp16", want=dict(div=True)))
        cases.append(_case("lean", c, 1, "sin", 2, div=2.0, rows="bf16", want=dict(div=True)))
    # ---- four-kernel form off the product widths
    idle = {20: (8, 3), 48: (16, 4), 96: (32, 8), 256: (64, 0), 80: (32, 12), 112: (32, 4)}
    for c, (lpr, lanes) in idle.items():
        premix = "mfma%d" % c if c in MFMA_WIDTHS else "cpl%d" % ((c + 63) // 64)
        for oi, (groups, op) in enumerate(((1, "cos"), (2, "sin"), (1, "cos_x"))):
            for r in (2, 3):
                if (oi + r) % 2 and c not in (20, 96):
                    continue
                cases.append(_case("four", c, groups, op, r, order="first" if oi == 1 else "cell", div=2.0 if oi == 2 else 1.0,
                                   bounds="tight" if r == 2 else "wide",
                                   want=dict(premix=premix, lpr=lpr, idle_lanes=lanes, modsum="group", gather="split",
                                             pair=groups == 2 and op != "cos_x" and c == 4 * lpr)))
    for groups, op, r in ((1, "cos", 3), (2, "sin", 2), (1, "cos_x", 3)):                 # c % 4 != 0: the lane = channel kernels
        cases.append(_case("four", 22, groups, op, r, want=dict(premix="cpl1", modsum="lane", gather="fused-lane")))
    cases.append(_case("four", 22, 1, "cos", 1, want=dict(modsum="lane", r=1)))          # r = 1 once (and on the group kernels)
    cases.append(_case("four", 64, 2, "cos", 1, want=dict(modsum="group", pair=True, gather="split", r=1)))
    for c in (96, 64):                                                                    # the flag sets of test_gpu_split_paths.py
        for name, flags in FLAG_SETS.items():
            lane = bool(flags & LANE_CHANNEL)
            want = dict(modsum="lane" if lane else "group",
                        gather="split" if not flags & FUSED_GATHER else ("fused-lane" if lane else "fused-group"),
                        pair=c == 64 and not flags & NO_PAIR)
            if not flags & FUSED_GATHER:
                want.update(bg_dense=not flags & NO_DENSE_GRID)
            for op, r in (("cos", 3), ("sin", 2)):
                if r == 2:
                    want = {k: v for k, v in want.items() if k != "bg_dense"}
                cases.append(_case("four", c, 2, op, r, bounds="tight", want=want, flags=flags))
    return cases


LATTICE = _lattice()


def case_id(case):
    kw = "".join("-%s%s" % (k.replace("lean_", ""), v) for k, v in sorted(case["kw"].items()) if v is not None)
    return "%s-C%d-g%d-%s-r%d-div%g-%s-%s-%s%s" % (case["form"], case["c"], case["groups"], case["op"], case["r"], case["div"],
                                                   case["rows"], case["order"], case["bounds"], kw)


def case_frame(case):
    return ("lat" if case["bounds"] == "wide" else "lat_tight", case["s"], case["r"])


def case_route(case, fkey=None, slot_cap=0, slow=False):
    """route() of a case on its frame (or on `fkey`)."""
    fkey = fkey or case_frame(case)
    co, bounds, s = geometry(fkey)
    dim = grid_of(bounds, s)[1]
    blocks = len(block_sizes(fkey, "cell"))
    return route(case["form"], case["c"], case["groups"], case["op"], case["r"], co.shape[0], dim[0] * dim[1] * dim[2] * dim[3],
                 k=slot_cap or s ** 3, slow=slow, half=case["rows"] != "fp32", blocks=blocks, coord_div=case["div"], **case["kw"])


# ------------------------------------------------------------------------------------------------------------------------------
# parameters and theta of the large-theta cases (e).  The general-layout kernels decide the sincos path per TILE, by the theta
# values themselves (`big`: some |theta| of the tile >= 32768; k_elk_tiles, k_elk_gather_tiles, the three lean kernels) -- not by a
# launch-wide bound as the dense-cell kernels do.  dense_frames' "exact" weights cancel the 2^17 offset of `exact_far` (|theta| <
# 40: the fast path here); "exact_big" keeps it: every |theta| >= 32768 and still exact in fp32.
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_of(c, groups, op, pos="init"):
    """dense_frames.block, plus pos = "exact_big": exact_pos_weight with the y column EQUAL to the x column -- on `exact_far`
    (x, y = 2^17 + a, 2^17 + b) theta = wx (2^18 + a + b) + wz z, a multiple of 2^-4 with |theta| in [2^15, 2^18): exact in fp32 in
    any order of summation, and on the slow path everywhere; cos_x: alpha a power of two in {0.5, 1} (theta alpha exact)."""
    if pos != "exact_big":
        return block(c, groups, op, pos)
    import copy
    blk = copy.deepcopy(block(c, groups, op, "exact"))
    with torch.no_grad():
        w = blk.pos_weight[0].weight
        w[:, 1] = w[:, 0]
        if op == "cos_x":
            g = torch.Generator().manual_seed(11)
            blk.alpha.copy_(2.0 ** -torch.randint(0, 2, blk.alpha.shape, generator=g).float())
    return blk


def theta_range(fkey, c, groups, op, pos, div=1.0):
    """(min over the voxels of the largest |theta| among a voxel's channels, max of |theta| over everything), in float64: a tile
    votes `big` as soon as ONE of its voxels has ONE channel at or beyond 32768."""
    from oracle.link_oracle import theta_torch
    blk = block_of(c, groups, op, pos)
    co = geometry(fkey)[0]
    th = theta_torch(co.double() / torch.tensor([div, div, div, 1.0], dtype=torch.float64), blk.pos_weight[0].weight.detach().double(),
                     op, groups, blk.alpha.detach().double() if op == "cos_x" else None).abs()
    return float(th.max(1).values.min()), float(th.max())


# (frame, pos_weight, the ops whose case DROPS the absolute bound, slow path: None = some tiles, True = every tile, False = none).
# The bound is dropped where the reference's own fp32 evaluation exceeds it (tests/test_cpu_core_frames.py computes it): `far` under
# cos / sin -- o32 = 1.1e-4 .. 1.6e-4 at theta ~ 2 000 rad, 2.4e-3 with the weights times 20.  Under cos_x the rows are dominated by
# v - fin theta, |theta| in the thousands: sin and cos carry 1e-4 of the row, o32 = 2.5e-7, and the bound stays.
LARGE_THETA = [("far", "init", ("cos", "sin"), False), ("far", "x20", ("cos", "sin"), None), ("exact_far", "exact", (), False),
               ("exact_far", "exact_big", (), True), ("bigrows", "init", (), False)]
LARGE_SHAPES = [(64, 2, "cos", 3), (64, 2, "sin", 2), (32, 1, "cos_x", 3)]


def large_lean_forms(c):
    """The lean kernels carry three copies of the `big` vote (k_lean_insert_premix, k_lean_insert_premix_cs, k_lean_sums_pm): the
    forms of launch 1 group e runs at width c, each with the route() subset it must reach.  The e frames hold fewer than 4 096
    voxels, so the bare C = 64 call IS the channel split and the default kernel needs lean_cs=False."""
    if c == 64:
        return [(dict(), dict(cs=True, pm=False)), (dict(lean_cs=False), dict(cs=False, pm=False)), (dict(lean_pm=True), dict(cs=False, pm=True))]
    return [(dict(), dict(cs=False, pm=False)), (dict(lean_pm=True), dict(cs=False, pm=True))]


# ------------------------------------------------------------------------------------------------------------------------------
# the parametrisations of groups b - f (tests/test_gpu_core_lattice.py takes them from here, tests/test_cpu_core_frames.py checks
# the reference on every one of them)
# ------------------------------------------------------------------------------------------------------------------------------
EDGE_FRAMES = BIG_BLOCKS + ["edges16", "through", "singles"]           # b
EDGE_WIDTHS = (16, 64, 128)
EDGE_OPS = [(2, "cos", 3), (1, "cos_x", 2)]                            # groups, op, r
CHUNK_SHAPES = [(64, 2, "cos", 3), (64, 1, "cos_x", 2), (16, 2, "sin", 3), (128, 2, "cos", 2)]      # c
CS_EDGE_SHAPES = [(2, "cos", 3), (1, "cos_x", 2)]
PACKING_SHAPES = [(32, 2, "cos", 3), (64, 1, "cos_x", 2)]
SPAN_SHAPES = [(16, 2, "cos", 3), (64, 1, "cos_x", 2)]                 # d
COORD_FRAMES = ["slab", "corners", "one", "pair"]                      # f
# c, groups, op, r, block order, coord_div.  `slab` runs its second case under cos: the lone voxel of its second batch item is
# analytically zero under sin, as `one` is -- which takes that case through gate_zero_rows


def coord_shapes(name):
    second = (64, 2, "cos" if name == "slab" else "sin", 2, "first", 1.0)
    return [(64, 2, "cos", 3, "cell", 1.0), second, (32, 1, "cos_x", 2, "cell", 1.0), (64, 2, "cos", 3, "first", 2.0)]


def gated_references():
    """Every distinct reference of groups a - f as (group, fkey, c, groups, op, pos, r, div, rows, absolute)."""
    out = []
    for case in LATTICE:
        out.append(("a", case_frame(case), case["c"], case["groups"], case["op"], "init", case["r"], case["div"], case["rows"], True))
    for name in EDGE_FRAMES:
        for c in EDGE_WIDTHS:
            for groups, op, r in EDGE_OPS:
                out.append(("b", (name, 1), c, groups, op, "init", r, 1.0, "fp32", True))
                if name in ("through", "singles"):
                    out.append(("b", (name, 1), c, groups, op, "init", r, 1.0, "fp16", True))
    for name in ("chunks", "s8_352"):
        for c, groups, op, r in CHUNK_SHAPES:
            out.append(("c", (name, 1), c, groups, op, "init", r, 1.0, "fp32", True))
    for n in (4096, 4097):
        for groups, op, r in CS_EDGE_SHAPES:
            out.append(("c", ("n%d" % n, 1), 64, groups, op, "init", r, 1.0, "fp32", True))
    for n in (16384, 16400):
        for c in (16, 32):
            for groups, op, r in CS_EDGE_SHAPES:
                out.append(("c", ("n%d" % n, 1), c, groups, op, "init", r, 1.0, "fp32", True))
    for c, groups, op, r in PACKING_SHAPES:
        out.append(("c", ("lat", 3, r), c, groups, op, "init", r, 1.0, "fp32", True))
    for name in ("chunks", "one"):
        out.append(("c", (name, 1), 64, 2, "cos", "init", 3, 1.0, "fp32", True))
    for n in (32768, 32800):
        for c, groups, op, r in SPAN_SHAPES:
            out.append(("d", ("n%d" % n, 1), c, groups, op, "init", r, 1.0, "fp32", True))
    for name, pos, drop, _ in LARGE_THETA:
        for c, groups, op, r in LARGE_SHAPES:
            out.append(("e", (name, 1), c, groups, op, pos, r, 1.0, "fp32", op not in drop))
    for pos in ("exact", "exact_big"):
        for c, groups, op, r in LARGE_SHAPES:
            out.append(("e", ("exact_far", 1), c, groups, op, pos, r, 1.0, "fp16", True))
    for name in COORD_FRAMES:
        for c, groups, op, r, _, div in coord_shapes(name):
            out.append(("f", (name, 1), c, groups, op, "init", r, div, "fp32", True))
    out.append(("f", ("lat", 7, 3), 64, 2, "cos", "init", 3, 1.0, "fp32", True))
    seen, uniq = set(), []
    for g in out:
        if g[1:] not in seen:
            seen.add(g[1:])
            uniq.append(g)
    return uniq
