"""Tables, rows and the case lattice of tests/test_gpu_conv_lattice.py, and a pure-Python restatement of which kernel instance a
sparse-convolution call reaches (csrc/conv.hip: subm_conv_impl, launch_conv_mfma, launch_conv_mfma_nt, launch_conv_resident;
csrc/dispatch.h: the width lists dispatch_conv_resident, dispatch_conv_table, dispatch_conv_pairs;
link_amd/elk.py: subm_conv, subm_conv_ln_add_relu, _conv_pairs, _conv_weight_grad).  No GPU code: tests/test_cpu_conv_frames.py
checks every claim made here (counts, routes, coverage, the constants against the sources) without a device.

A table is int32 [n_out, kvol], -1 = absent, entries < n_in.  Three kinds, named by a hashable key (table()):
  ("crafted", n_out, n_in, kvol, seed)   seeded random entries, each present with probability DENSITY; from 4 rows up row 1 is all
                                         absent, row 2 is full, and the last row names input row n_in - 1 at every offset.  The
                                         forward and weight-gradient kernels never ask for geometric consistency.
  ("submlike", n, kvol, seed)            the same with n_in = n_out and the centre column the identity: what a submanifold table
                                         looks like to the pair plan (direct) and to the weight gradient's centre split.
  ("granule", direct)                    pairs per offset of exactly 127, 128, 129 and 0: the pair plan's 128-row granule edge
                                         (direct: kvol 5 with the identity centre; else kvol 4, n_out != n_in).
  ("real", kind, n)                      the submanifold map of a lidar_like / s_uniform frame by the C oracle (symmetric: the
                                         input gradient of _SubmConv needs nbr[v, k] = u <=> nbr[u, K-1-k] = v).
  ("down", kind, n)                      the stride-2, kernel-2 gather table of such a frame (n_out = occupied 2^3 cells)."""
import collections
import functools

import numpy as np
import torch

from helpers import lidar_like, s_uniform

DENSITY = 0.3

# ------------------------------------------------------------------------------------------------------------------------------
# constants restated from the sources (pinned against their literal lines by tests/test_cpu_conv_frames.py)
# ------------------------------------------------------------------------------------------------------------------------------
G_CONV_WGS = 1024                              # conv.hip: g_conv_wgs
LDS_LIMIT = 160 * 1024
RESIDENT = ((16, 16), (32, 32), (16, 32), (32, 16))                    # dispatch.h: dispatch_conv_resident; elk.py: _RESIDENT_SHAPES
LINK_CONV = ((16, 16), (32, 32), (48, 48), (64, 64), (80, 80), (96, 96), (112, 112), (128, 128),
             (16, 32), (32, 16), (32, 64), (64, 32), (64, 128), (128, 64),
             (96, 128), (128, 96), (64, 96), (96, 64), (32, 96), (96, 32),
             (16, 64), (64, 16), (32, 128), (128, 32))                 # dispatch.h: dispatch_conv_table
MFMA = tuple(p for p in LINK_CONV if p not in RESIDENT)                 # (the resident test comes first: its four pairs never get there)
PAIRS_SQUARE = (16, 32, 64, 128)                                        # dispatch.h: dispatch_conv_pairs (link_conv_pairs_supported)
PAIRS_RECT = ((16, 32), (32, 16), (32, 64), (64, 32), (64, 128), (128, 64), (16, 64), (64, 16))
PAIR_DENSITY_MAX = 17.0                                                 # elk.py
WGRAD_CHUNK_EDGES = (16000, 60000)                                      # elk.py: chunks 16 / 32 / 64
WGRAD_CENTRE_MIN = 4096                                                 # elk.py: centre_extra = 3 * chunks from here on a _link_subm table


def nt4_fits(ci, co):
    return (2 * co * (ci + 4) + 4 * 27 * 4 * 16) * 4 <= LDS_LIMIT and co <= 112


def res_cfg(ci, co):
    """(NW, LDS_BYTES) of conv_res_cfg<CI, CO>."""
    w_floats = 27 * co * (ci + 4)
    nw = 16 if w_floats * 4 > 48 * 1024 else 8
    return nw, w_floats * 4 + nw * (27 + 1) * 16 * 4


def pairs_supported(ci, co):
    return (ci == co and ci in PAIRS_SQUARE) or (ci, co) in PAIRS_RECT


def _ceil16(c):
    return (c + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------------------------
# route: which kernel instance a call reaches
# ------------------------------------------------------------------------------------------------------------------------------
def _route_table(n_out, cin, cout, kvol, epilogue):
    """subm_conv_impl."""
    if n_out == 0:
        return dict(kernel="none")
    tiles = (n_out + 15) // 16
    mfma_ok = cin % 16 == 0 and cout % 16 == 0 and cin <= 128 and cout <= 128 and kvol <= 27
    if mfma_ok and (cin, cout) in RESIDENT:
        nw, lds = res_cfg(cin, cout)
        wgs = (tiles + nw - 1) // nw
        return dict(kernel="resident", CI=cin, CO=cout, split=bool(epilogue), NW=nw, capped=wgs > 256 * (LDS_LIMIT // lds))
    if mfma_ok and (cin, cout) in MFMA:
        if tiles > G_CONV_WGS * 4 * 2 and nt4_fits(cin, cout):
            nt = 4
        elif tiles > G_CONV_WGS * 4:
            nt = 2
        else:
            nt = 1
        wgs = (tiles + 4 * nt - 1) // (4 * nt)
        return dict(kernel="mfma", CI=cin, CO=cout, NT=nt, DEEP=nt == 1 and tiles <= 1024, capped=wgs > G_CONV_WGS)
    return dict(kernel="generic", CPL=(cout + 63) // 64)


def route(n_out, cin, cout, kvol, epilogue=False, form="table", half=False, density=None, direct=None):
    """The kernel a forward call reaches.  `epilogue`: through subm_conv_ln_add_relu; `half`: False, "fp16" or "bf16" rows;
    `density` (pairs per output row, identity pairs included) and `direct` (the pair plan found a submanifold table) matter only
    where a pair plan is consulted (form "auto" / "pairs")."""
    if form == "table":
        return _route_table(n_out, cin, cout, kvol, epilogue)
    assert form in ("auto", "pairs")
    if n_out == 0:
        return dict(kernel="none")
    if not epilogue and cout < 16 and pairs_supported(_ceil16(cin), 16):
        cout = 16                                                         # zero columns up to 16, sliced afterwards
    if cin < 16 and pairs_supported(16, cout):
        cin = 16                                                          # _pad_in_channels
    resident = form == "auto" and kvol <= 27 and (cin, cout) in RESIDENT
    if resident and half:
        return dict(kernel="resident_amp", CI=cin, CO=cout, rows=half)
    if not resident and pairs_supported(cin, cout) and kvol <= 64 and (form == "pairs" or density <= PAIR_DENSITY_MAX):
        gemm = "amp" if half else ("split" if epilogue and cin >= 32 else "f32")
        return dict(kernel="pairs", CI=cin, CO=cout, gemm=gemm, direct=bool(direct), c16=bool(half == "fp16" and direct))
    assert form == "auto", "form='pairs' on widths the pair-list kernels do not take"
    return _route_table(n_out, cin, cout, kvol, epilogue)


def route_wgrad(n_out, cin, cout, kvol, link_subm=False, density=None, direct=None, table_square=True):
    """_conv_weight_grad: the table kernel with its (chunks, centre_extra), the pair list, or the torch fallback.
    `table_square`: elk.py's WGRAD_TABLE_SQUARE."""
    square_small = table_square and cin == cout and cin <= 64 and cin % 4 == 0
    takes_pairs = lambda ci: n_out > 0 and pairs_supported(ci, cout) and kvol <= 64 and density <= PAIR_DENSITY_MAX   # noqa: E731
    if cin < 16 and not square_small and takes_pairs(16):
        cin = 16
    if not square_small and takes_pairs(cin):
        return dict(kernel="pairs_wgrad", CI=cin, CO=cout, direct=bool(direct))
    if square_small:
        chunks = 16 if n_out < WGRAD_CHUNK_EDGES[0] else (32 if n_out < WGRAD_CHUNK_EDGES[1] else 64)
        dense_centre = bool(link_subm) and kvol % 2 == 1 and kvol > 1 and n_out >= WGRAD_CENTRE_MIN
        return dict(kernel="table_wgrad", chunks=chunks, extra=3 * chunks if dense_centre else 0)
    return dict(kernel="torch")


def branch(r):
    """The hashable branch a route dict stands for (what LATTICE has to cover)."""
    k = r["kernel"]
    if k == "resident":
        return [("resident", r["CI"], r["CO"], r["split"]), ("resident_capped", r["capped"])]
    if k == "mfma":
        return [("mfma", r["CI"], r["CO"]), ("mfma_nt", r["NT"], r["DEEP"], r["capped"])]
    if k == "generic":
        return [("generic", r["CPL"])]
    if k == "resident_amp":
        return [("resident_amp", r["rows"])]
    if k == "pairs":
        return [("pairs", r["gemm"], r["direct"]), ("pairs_c16", r["c16"])]
    if k == "table_wgrad":
        return [("table_wgrad", r["chunks"], r["extra"])]
    if k == "pairs_wgrad":
        return [("pairs_wgrad", r["direct"])]
    return [(k,)]


def all_branches():
    """Every branch the launchers distinguish, enumerated from the constants alone."""
    b = {("resident", ci, co, s) for ci, co in RESIDENT for s in (False, True)}
    b |= {("resident_capped", c) for c in (False, True)}
    b |= {("mfma", ci, co) for ci, co in MFMA}
    b |= {("mfma_nt", 1, True, False), ("mfma_nt", 1, False, False), ("mfma_nt", 2, False, False), ("mfma_nt", 4, False, False),
          ("mfma_nt", 2, False, True), ("mfma_nt", 4, False, True)}
    b |= {("generic", c) for c in (1, 2, 3, 4)}
    b |= {("resident_amp", h) for h in ("fp16", "bf16")}
    b |= {("pairs", g, d) for g in ("f32", "split", "amp") for d in (False, True)}
    b |= {("pairs_c16", c) for c in (False, True)}
    b |= {("table_wgrad", ch, ex) for ch in (16, 32, 64) for ex in (0, 3 * ch)}
    b |= {("pairs_wgrad", d) for d in (False, True)}
    b |= {("torch",), ("none",)}
    return b


# ------------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------------
def _real_coords(kind, n):
    if kind == "uniform":
        return s_uniform(n, grid=24, seed=5)                                # ~ n / 13 824 occupancy: a few neighbours per voxel
    assert kind == "lidar", kind
    return torch.from_numpy(lidar_like(n, seed=3))


@functools.lru_cache(maxsize=None)
def table(tkey):
    """(int32 [n_out, kvol] on the CPU, n_in) of a table key; shared and never changed."""
    kind = tkey[0]
    if kind in ("crafted", "submlike"):
        if kind == "crafted":
            _, n_out, n_in, kvol, seed = tkey
        else:
            _, n_out, kvol, seed = tkey
            n_in = n_out
        g = torch.Generator().manual_seed(1000 + seed)
        if n_out == 0:
            return torch.empty((0, kvol), dtype=torch.int32), n_in
        present = torch.rand((n_out, kvol), generator=g) < DENSITY
        ids = torch.randint(0, n_in, (n_out, kvol), generator=g, dtype=torch.int32)
        nbr = torch.where(present, ids, torch.full_like(ids, -1))
        if n_out >= 4:
            nbr[1] = -1
            nbr[2] = ids[2]
            nbr[n_out - 1] = n_in - 1
        if kind == "submlike":
            nbr[:, kvol // 2] = torch.arange(n_out, dtype=torch.int32)
        return nbr.contiguous(), n_in
    if kind == "granule":
        direct = tkey[1]
        n_out, n_in, kvol = (200, 200, 5) if direct else (200, 150, 4)
        g = torch.Generator().manual_seed(77)
        nbr = torch.full((n_out, kvol), -1, dtype=torch.int32)
        cols = [0, 1, 3, 4] if direct else [0, 1, 2, 3]
        for col, cnt in zip(cols, (127, 128, 129, 0)):
            rows = torch.randperm(n_out, generator=g)[:cnt]
            nbr[rows, col] = torch.randint(0, n_in, (cnt,), generator=g, dtype=torch.int32)
        if direct:
            nbr[:, 2] = torch.arange(n_out, dtype=torch.int32)
        return nbr.contiguous(), n_in
    if kind == "real":
        from oracle import link_oracle as O
        co = _real_coords(tkey[1], tkey[2])
        return torch.from_numpy(O.conv_neighbor_table(co.numpy(), 3, 1).astype(np.int32)).contiguous(), co.shape[0]
    if kind == "down":
        co = _real_coords(tkey[1], tkey[2])[:, :3].long()
        cell, inv = torch.unique(torch.div(co, 2, rounding_mode="floor"), dim=0, return_inverse=True)
        tap = (co[:, 0] % 2) * 4 + (co[:, 1] % 2) * 2 + co[:, 2] % 2       # any fixed numbering of the 8 taps serves the kernels
        nbr = torch.full((cell.shape[0], 8), -1, dtype=torch.int32)
        nbr[inv, tap] = torch.arange(co.shape[0], dtype=torch.int32)
        return nbr.contiguous(), co.shape[0]
    raise KeyError(tkey)


def table_back(nbr, n_in):
    """The opposite direction's table of a gather table whose (input row, offset) pairs are unique: back[i, k] = j <=> nbr[j, k] = i."""
    back = torch.full((n_in, nbr.shape[1]), -1, dtype=torch.int32)
    j, k = torch.nonzero(nbr >= 0, as_tuple=True)
    back[nbr[j, k].long(), k] = j.int()
    return back.contiguous()


def table_stats(nbr, n_in):
    """(density, direct) as the pair plan sees the table: pairs per output row with the identity pairs counted, and whether the
    table is a submanifold one to it (odd kernel, every row's centre entry the row itself)."""
    n_out, kvol = nbr.shape
    if n_out == 0:
        return 0.0, False
    direct = kvol % 2 == 1 and bool((nbr[:, kvol // 2] == torch.arange(n_out, dtype=torch.int32)).all())
    return float((nbr >= 0).sum()) / n_out, direct


@functools.lru_cache(maxsize=None)
def rows_of(n, c, seed):
    """fp32 [n, c] N(0, 1) rows on the CPU."""
    return torch.randn(n, c, generator=torch.Generator().manual_seed(2000 + seed))


@functools.lru_cache(maxsize=None)
def weights_of(kvol, cin, cout, seed, big=False):
    """fp32 [kvol, cin, cout] N(0, 1 / cin) weights; `big`: one entry of 40 000 (>= 2^15: outside the fp16 split's range)."""
    w = torch.randn(kvol, cin, cout, generator=torch.Generator().manual_seed(3000 + seed)) / cin ** 0.5
    if big:
        w[kvol // 3, 1, 2] = 40000.0
    return w


@functools.lru_cache(maxsize=None)
def order_of(n, seed=0):
    """A seeded permutation of the output rows, int32 (what `order` may be: any permutation)."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(4000 + seed)).int()


@functools.lru_cache(maxsize=None)
def ep_params(cout, kind, n_out):
    """Keyword arguments of conv64.epilogue for an epilogue kind: "ln", "ln_add_relu", "affine_add_relu", "identity" (affine with
    scale 1, shift 0, no ReLU: the convolution itself through the fused entry point)."""
    g = torch.Generator().manual_seed(5000 + cout)
    lw, lb = 1 + 0.1 * torch.randn(cout, generator=g), 0.1 * torch.randn(cout, generator=g)
    add = torch.randn(n_out, cout, generator=g)
    if kind == "identity":
        return dict(ln_w=torch.ones(cout), ln_b=torch.zeros(cout), eps=0.0, addend=None, relu=False, affine=True)
    if kind == "ln":
        return dict(ln_w=lw, ln_b=lb, eps=1e-6, addend=None, relu=False, affine=False)
    if kind == "ln_add_relu":
        return dict(ln_w=lw, ln_b=lb, eps=1e-6, addend=add, relu=True, affine=False)
    assert kind == "affine_add_relu", kind
    return dict(ln_w=lw, ln_b=lb, eps=0.0, addend=add, relu=True, affine=True)


# ------------------------------------------------------------------------------------------------------------------------------
# the per-element bound (gate c)
# ------------------------------------------------------------------------------------------------------------------------------
def element_bound(terms, amax, split=False, rt=None, offset_roundings=False):
    """A, B, |ref| -> the bound on |out - ref| per element; the derivations are in tests/test_gpu_conv_lattice.py's docstring.
    terms: products per element (kvol * cin; pairs of the offset for g_w); amax: max A of the tensor (the floor)."""
    from conv64 import F16_SUB, U32, UNIT
    fac = ((3 * terms if split else terms) + 2) * U32

    def bound(A, B, ref):
        e = fac * A + fac * amax * 1e-3
        if split:
            e = e + 3 * 2.0 ** -22 * A + 2.0 ** -25 * B
        if rt is not None:
            u = UNIT[rt]
            sub = F16_SUB if rt == torch.float16 else 0.0
            if offset_roundings:                                           # every offset's product row rounded, then the sum
                e = e + u * (A + e) + sub * 27
            e = e + u * (ref + e) + sub                                    # the store
        return e
    return bound


# ------------------------------------------------------------------------------------------------------------------------------
# the lattice
# ------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "group tkey cin cout form ep rows big", defaults=("table", None, "fp32", False))


def case_id(c):
    t = "-".join(str(v) for v in c.tkey)
    return f"{c.group}:{t}:{c.cin}x{c.cout}:{c.form}" + (f":{c.ep}" if c.ep else "") + (f":{c.rows}" if c.rows != "fp32" else "") + \
        (":big" if c.big else "")


def case_route(c):
    """The route `c` is expected to take, from the table's own counts."""
    nbr, n_in = table(c.tkey)
    density, direct = table_stats(nbr, n_in)
    return route(nbr.shape[0], c.cin, c.cout, nbr.shape[1], epilogue=c.ep is not None, form=c.form,
                 half=False if c.rows == "fp32" else c.rows, density=density, direct=direct)


N_SMALL = 1007                                                             # 63 tiles, the last one of 15 rows: the DEEP instance
W_TABLE = ("crafted", N_SMALL, 700, 27, 1)
SUB_SMALL = ("submlike", N_SMALL, 27, 6)                                   # the same size with the identity centre: a direct pair plan
PAIRS_FORWARD_REST = ((32, 32), (32, 16), (64, 32), (64, 128), (32, 64))


def _lattice():
    L = []
    # every width instance of the table form: 20 MFMA pairs, 4 resident pairs plain (exact f32) and fused (fp16 split)
    L += [Case("width", W_TABLE, ci, co) for ci, co in LINK_CONV]
    L += [Case("width", W_TABLE, ci, co, ep="ln_add_relu") for ci, co in RESIDENT]
    # tiles per wave and the capped grids, n just past each edge: one narrow and one wide MFMA instance; the resident kernel's
    # persistent stride at both of its configurations (NW = 8: 768 workgroups x 8 tiles; NW = 16: 256 x 16)
    L += [Case("nt", ("crafted", n, n, 27, 2), 16, 64) for n in (16400, 65600, 131200, 262400)]
    L += [Case("nt", ("crafted", n, n, 27, 2), 128, 128) for n in (16400, 65600, 131200)]
    L += [Case("nt", ("crafted", 65600, 65600, 27, 2), 32, 32), Case("nt", ("crafted", 131200, 131200, 27, 2), 16, 16)]
    L += [Case("nt", ("crafted", 65600, 65600, 27, 2), 64, 64, ep="ln_add_relu")]
    # the generic kernel: CPL 1 .. 4, cin > 128, multiples of 16 outside the table, kvol = 125
    L += [Case("generic", W_TABLE, ci, co) for ci, co in ((1, 1), (3, 5), (12, 40), (17, 65), (20, 129), (8, 193), (4, 256),
                                                          (144, 144), (48, 64))]
    L += [Case("generic", ("crafted", N_SMALL, 700, 125, 3), 16, 16)]
    L += [Case("generic", W_TABLE, 17, 65, ep="ln"), Case("generic", W_TABLE, 20, 129, ep="ln_add_relu"),
          Case("generic", W_TABLE, 48, 64, ep="affine_add_relu"), Case("generic", W_TABLE, 4, 256, ep="ln")]
    # kvol below 27 on one resident and one MFMA instance (their LDS images are sized for 27)
    L += [Case("kvol", ("crafted", N_SMALL, 700, kv, 4), c, c) for kv in (1, 8, 18) for c in (16, 64)]
    L += [Case("kvol", ("crafted", N_SMALL, 700, 8, 4), 16, 16, ep="ln")]
    # tables that are not a submanifold map: n_out of 1 .. 65 over 50 input rows, on a resident, an MFMA and a generic instance
    L += [Case("edge", ("crafted", n, 50, 27, 5), ci, co) for n in (1, 15, 16, 17, 63, 64, 65) for ci, co in ((16, 16), (64, 64), (12, 40))]
    # epilogues on the MFMA kernel
    L += [Case("epilogue", W_TABLE, 64, 64, ep=e) for e in ("ln", "ln_add_relu", "affine_add_relu")]
    L += [Case("epilogue", W_TABLE, 32, 64, ep="ln_add_relu"), Case("epilogue", W_TABLE, 128, 128, ep="ln"),
          Case("epilogue", W_TABLE, 16, 16, ep="affine_add_relu")]
    # the pair-list form next to the table form on the same case (e): direct and non-direct plans, granule edges, the split GEMM
    # (fused entry point, cin >= 32) and its `big` flag, 16-bit rows
    real, sub, crafted = ("real", "lidar", 3000), ("submlike", 2000, 27, 6), ("crafted", 1500, 900, 27, 7)
    for form in ("pairs", "table"):
        L += [Case("pairs", real, ci, co, form) for ci, co in ((64, 64), (16, 64), (128, 64), (128, 128))]
        L += [Case("pairs", crafted, ci, co, form) for ci, co in ((64, 64), (32, 64), (64, 128), (16, 16))]
        L += [Case("pairs", ("granule", d), c, c, form) for d in (True, False) for c in (16, 64)]
        L += [Case("pairs", sub, 64, 64, form, ep="ln_add_relu"), Case("pairs", crafted, 32, 64, form, ep="affine_add_relu"),
              Case("pairs", real, 128, 128, form, ep="ln"), Case("pairs", ("granule", False), 64, 64, form, ep="ln"),
              Case("pairs", sub, 16, 32, form, ep="ln_add_relu")]
        L += [Case("pairs", sub, 64, 64, form, ep="affine_add_relu", big=True), Case("pairs", crafted, 64, 64, form, ep="ln", big=True)]
        # the widths of dispatch_conv_pairs that no case above sends through the f32 GEMM and the centre-sum kernel, on a
        # submanifold-like table of the small size: with them each of the 12 pairs reaches both entry points
        L += [Case("pairs", SUB_SMALL, ci, co, form) for ci, co in PAIRS_FORWARD_REST]
    L += [Case("pairs", real, 4, 64, "auto"), Case("pairs", real, 64, 3, "auto")]           # padded to 16 channels in / out
    L += [Case("half", sub, 64, 64, "pairs", rows="fp16"), Case("half", crafted, 64, 64, "pairs", rows="fp16"),
          Case("half", sub, 64, 64, "pairs", rows="bf16"), Case("half", real, 32, 64, "pairs", rows="fp16"),
          Case("half", sub, 64, 64, "pairs", ep="ln_add_relu", rows="fp16"), Case("half", crafted, 64, 128, "pairs", ep="ln", rows="bf16")]
    L += [Case("half", ("crafted", N_SMALL, 700, 27, 1), ci, co, "auto", rows=r)
          for (ci, co), r in zip(RESIDENT, ("fp16", "bf16", "fp16", "bf16"))]
    L += [Case("half", sub, 16, 16, "auto", ep="ln_add_relu", rows="fp16"), Case("half", sub, 32, 32, "auto", ep="affine_add_relu", rows="bf16"),
          Case("half", ("crafted", 65600, 65600, 8, 2), 16, 16, "auto", rows="fp16")]
    L += [Case("empty", ("crafted", 0, 50, 27, 1), c, c, f) for c, f in ((16, "table"), (64, "table"), (12, "table"), (64, "auto"))]
    return L


LATTICE = _lattice()

# the weight gradient: (c, n_out, _link_subm) through the table kernel; pair list and torch fallback cases
WGRAD_C = (4, 8, 12, 16, 20, 32, 48, 64)
WGRAD_N = (40, 4095, 4096, 15999, 16000, 60000)
# (table key, cin, cout): rectangular and wide pairs, direct (submanifold-like / real) and non-direct plans, first-layer padding
WGRAD_PAIRS = ((("submlike", 2000, 27, 6), 32, 64), (("real", "lidar", 3000), 128, 128), (("crafted", 1500, 900, 27, 7), 64, 128),
               (("crafted", 1500, 900, 27, 7), 128, 128), (("granule", True), 16, 32), (("granule", False), 64, 16),
               (("real", "lidar", 3000), 4, 64), (("down", "lidar", 3000), 32, 64),
               (SUB_SMALL, 32, 16), (SUB_SMALL, 64, 32), (SUB_SMALL, 128, 64))           # the rectangular widths the rows above leave out
# the square widths <= 64 reach link_conv_pairs_wgrad only with elk.py's WGRAD_TABLE_SQUARE off (the table kernel has them otherwise)
WGRAD_PAIRS_SQUARE = ((SUB_SMALL, 16, 16), (SUB_SMALL, 32, 32), (SUB_SMALL, 64, 64))
WGRAD_TORCH = ((W_TABLE, 6, 10),)


def wgrad_table_key(n, subm):
    return ("submlike", n, 27, 8) if subm else ("crafted", n, max(n // 2, 8), 27, 8)


def wgrad_label(tkey, cin, cout, subm):
    return f"wgrad:{'-'.join(str(v) for v in tkey)}:{cin}x{cout}" + (":subm" if subm else "")


def wgrad_routes():
    """Every weight-gradient case of the GPU test with the route it is expected to take."""
    out = []
    for c in WGRAD_C:
        for n in WGRAD_N:
            for subm in (False, True):
                out.append(((wgrad_table_key(n, subm), c, c, subm), route_wgrad(n, c, c, 27, link_subm=subm)))
    for tkey, ci, co in WGRAD_PAIRS + WGRAD_TORCH:
        nbr, n_in = table(tkey)
        density, direct = table_stats(nbr, n_in)
        out.append(((tkey, ci, co, False), route_wgrad(nbr.shape[0], ci, co, nbr.shape[1], density=density, direct=direct)))
    return out
