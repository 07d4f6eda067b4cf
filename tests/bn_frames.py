"""Cases, frames and a pure-Python restatement of the launch geometry of the training-mode BatchNorm kernels (csrc/bn.hip, C ABI
section F; tests/test_gpu_bn_lattice.py).  No GPU code and no link_amd import: tests/test_cpu_bn_frames.py checks every claim made
here (the constants against the literal lines of bn.hip, partial_workgroups against the library's host function, that every group
reaches the branch it names) without a device.

Geometry of k_col_moments on [n, c] rows: a thread owns 4 consecutive channels (cq = c / 4 threads per row), a workgroup of 256
threads covers rpp = 256 // cq rows per pass (rpp * cq <= 256 threads are active, the rest idle), `wgs` workgroups give
stride = wgs * rpp row slots; slot s reads rows s, s + stride, ... -- four at a time while four are left, then one at a time.
k_bn_finalize_* sums the wgs partials of a channel in 16 interleaved subtotals.  k_bn_apply is a grid-stride loop over n * cq
float4 pieces on at most APPLY_CAP workgroups.

A frame is x [n, c] by kind:
  plain    randn * (rand(c) * 3) + randn(c) * 5            the frame of tests/test_gpu_encoder.py: per-channel spread
  offset   100 + 0.01 * randn                              mean >> sigma: the mean's own fp32 rounding shifts xhat by up to 4e-4
           (16-bit rows: sigma of four spacings of the row type at 100, 0.25 / 2: rounded into the type the frame keeps a spread)
  wide     randn * sigma_c + sigma_c * randn(c), sigma_c log-spaced 1e-3 .. 1e3 over the channels
and `special` channels (channels 1 and 2: inside the first float4, next to ordinary channels that stay gated):
  const15  channel 1 is 1.5 everywhere          const01  channel 1 is float32(0.1) everywhere (var = 0)
  w0b0     channel 2: weight 0, bias 0 (y == 0, mask false everywhere, grad_x == 0)
  w0bpos   channel 2: weight 0, bias 0.75       wneg     channel 2: weight -1.25
  ginf     (non-finite) the upstream gradient of row n // 2, channel 2 is +inf"""
import collections
import functools

import torch

# ------------------------------------------------------------------------------------------------------------------------------
# constants restated from bn.hip (pinned against its literal lines by tests/test_cpu_bn_frames.py)
# ------------------------------------------------------------------------------------------------------------------------------
WG = 256                      # threads of a workgroup, every kernel
ROWS_PER_SLOT = 8             # link_bn_partial_workgroups: (n + rpp * 8 - 1) / (rpp * 8)
WGS_CAP = 512                 # ... if (wgs > 512) wgs = 512
APPLY_PIECES = 256 * 4        # bn_apply_grid: (n * (c / 4) + 256 * 4 - 1) / (256 * 4)
APPLY_CAP = 4096              # ... wgs > 4096 ? 4096
GATHER = 16                   # bn_gather_partials: w = wl; w < wgs; w += 16
C_MIN, C_MAX = 4, 1024        # bn_width_ok


def width_ok(c):
    return C_MIN <= c <= C_MAX and c % 4 == 0


def hip_ok(n, c, momentum=0.1):
    """link_amd.BatchNorm._hip_train_ok on fp32 GPU rows in training mode; everything else is torch.nn.functional.batch_norm."""
    return width_ok(c) and n > 1 and momentum is not None


def cq(c):
    return c // 4


def rpp(c):
    return WG // cq(c)


def active_threads(c):
    return rpp(c) * cq(c)


def partial_workgroups(n, c):
    if n <= 0 or not width_ok(c):
        return 0
    per = rpp(c) * ROWS_PER_SLOT
    return max(1, min(WGS_CAP, (n + per - 1) // per))


def wgs_uncapped(n, c):
    per = rpp(c) * ROWS_PER_SLOT
    return (n + per - 1) // per


def stride(n, c):
    return partial_workgroups(n, c) * rpp(c)


def slot_passes(n, c, slot):
    """(passes of the 4-row loop, passes of the tail loop) of row slot `slot` (0 <= slot < stride)."""
    st = stride(n, c)
    rows = (n - slot + st - 1) // st if slot < n else 0
    return rows // 4, rows % 4


def passes(n, c):
    """The set of (quad, tail) pairs over all slots."""
    st = stride(n, c)
    return {slot_passes(n, c, s) for s in {0, min(n, st) - 1, n % st, max(n % st - 1, 0), st - 1}}


def sum_depth(n, c):
    """The largest number of double additions one term of a column sum goes through: the slot's own rows, the workgroup's rpp
    slots, the wgs / 16 partials of a subtotal and the 16 subtotals."""
    st, wgs = stride(n, c), partial_workgroups(n, c)
    return (n + st - 1) // st + rpp(c) + (wgs + GATHER - 1) // GATHER + GATHER


def apply_grid(n, c):
    return max(1, min(APPLY_CAP, (n * cq(c) + APPLY_PIECES - 1) // APPLY_PIECES))


def apply_grid_uncapped(n, c):
    return (n * cq(c) + APPLY_PIECES - 1) // APPLY_PIECES


# ------------------------------------------------------------------------------------------------------------------------------
# the lattice
# ------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "group name n c kind rows relu eps momentum affine running scale coef special")
SPECIALS = ("const15", "const01", "w0b0", "w0bpos", "wneg", "ginf")
CH_CONST, CH_W = 1, 2                           # the special channels


def _case(group, name, n, c, kind="plain", rows="fp32", relu=True, eps=1e-3, momentum=0.1, affine=True, running=True, scale=True,
          coef=True, special=""):
    assert kind in ("plain", "offset", "wide") and rows in ("fp32", "fp16", "bf16") and special in SPECIALS + ("",)
    assert hip_ok(n, c), (n, c)
    return Case(group, f"{group}-{name}", n, c, kind, rows, relu, eps, momentum, affine, running, scale, coef, special)


WIDTHS = (4, 8, 12, 16, 20, 28, 48, 64, 100, 128, 256, 260, 344, 516, 1020, 1024)


def _rows_group(c):
    r = rpp(c)
    per = r * ROWS_PER_SLOT
    return [("n2", 2), ("rpp-1", r - 1), ("rpp", r), ("rpp+1", r + 1), ("8rpp", per), ("8rpp+1", per + 1),
            ("wgs15", 15 * per), ("wgs16", 16 * per), ("wgs17", 16 * per + 1), ("quads", 4 * r), ("tail1", 5 * r)]


def _lattice():
    out = []
    # widths: every cq class with and without idle threads, a few hundred rows each (an odd count: the last slot is ragged)
    for i, c in enumerate(WIDTHS):
        out.append(_case("widths", f"c{c}", 301 + 2 * i, c, relu=i % 2 == 0))
    # rows: slot edges at rpp = 16 and rpp = 256
    for c in (64, 4):
        for name, n in _rows_group(c):
            out.append(_case("rows", f"c{c}-{name}", n, c))
    # caps: the 512 workgroups of the partial sums just under, at and past; the 4096 workgroups of the apply pass
    for c, ns in ((64, (65408, 65536, 65537)), (1024, (4088, 4096, 4097))):
        for n in ns:
            out.append(_case("caps", f"c{c}-n{n}", n, c))
    out.append(_case("caps", "apply-c1024-n16500", 16500, 1024))
    # conditioning
    for kind in ("plain", "offset", "wide"):
        for relu in (True, False):
            out.append(_case("conditioning", f"{kind}-{'relu' if relu else 'lin'}", 1003, 48, kind=kind, relu=relu))
    out.append(_case("conditioning", "offset-n2", 2, 64, kind="offset"))
    for sp in SPECIALS[:5]:
        out.append(_case("conditioning", sp, 517, 20, special=sp))
        out.append(_case("conditioning", f"{sp}-offset-c4", 300, 4, kind="offset", special=sp))
    out.append(_case("conditioning", "eps1e-5", 517, 20, eps=1e-5))
    out.append(_case("conditioning", "eps1e-5-offset", 517, 20, kind="offset", eps=1e-5))
    out.append(_case("conditioning", "eps1e-5-const01", 517, 20, eps=1e-5, special="const01"))
    for mom in (0.01, 1.0):
        out.append(_case("conditioning", f"momentum{mom}", 517, 20, momentum=mom))
    # options
    out.append(_case("options", "no-affine", 517, 20, affine=False))
    out.append(_case("options", "no-affine-lin", 517, 20, affine=False, relu=False))
    out.append(_case("options", "no-running", 517, 20, running=False))
    out.append(_case("options", "no-scale", 517, 20, scale=False))
    out.append(_case("options", "no-coef", 517, 20, coef=False))
    out.append(_case("options", "no-coef-lin", 517, 20, coef=False, relu=False))
    out.append(_case("options", "lin", 517, 20, relu=False))
    # row types: one case per rpp class (256, 16, idle threads, 1), a cap case, the offset kind, both relu forms
    for rt in ("fp16", "bf16"):
        out.append(_case("rowtypes", f"{rt}-c4", 300, 4, rows=rt))
        out.append(_case("rowtypes", f"{rt}-c64", 2049, 64, rows=rt))
        out.append(_case("rowtypes", f"{rt}-c100", 317, 100, rows=rt, relu=False))
        out.append(_case("rowtypes", f"{rt}-c1020", 329, 1020, rows=rt))
        out.append(_case("rowtypes", f"{rt}-cap", 4097, 1024, rows=rt))
        out.append(_case("rowtypes", f"{rt}-offset", 1003, 48, kind="offset", rows=rt))
        out.append(_case("rowtypes", f"{rt}-w0b0", 517, 20, rows=rt, special="w0b0"))
    # non-finite: one inf in the upstream gradient
    out.append(_case("nonfinite", "fp32", 517, 20, relu=False, special="ginf"))
    out.append(_case("nonfinite", "fp16", 517, 20, relu=False, rows="fp16", special="ginf"))
    names = [k.name for k in out]
    assert len(set(names)) == len(names)
    return tuple(out)


LATTICE = _lattice()
FALLBACK = ((50, 6, 0.1), (50, 2, 0.1), (50, 1028, 0.1), (1, 64, 0.1), (50, 64, None))     # (n, c, momentum): torch's batch_norm
MODULE = tuple(k for k in LATTICE if k.name in (
    "widths-c100", "rows-c64-n2", "rows-c4-8rpp+1", "caps-c1024-n4097", "conditioning-offset-relu", "conditioning-w0b0",
    "options-no-affine", "options-no-running", "rowtypes-fp16-c64", "rowtypes-bf16-c100", "rowtypes-fp16-offset"))
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# Where verdict (a) drops the absolute ceiling (ref64.gate_rows: absolute=False, what the core lattice does for `far`): exactly the
# (tensor, case) pairs named here, those whose fp32 evaluation alone (o32 of the tensor's worst channel, tests/bn64.py) exceeds a
# QUARTER of the ceiling.  A quarter, not the whole: the gate is 4 o32 + 2 o_round + 2e-6, so from o32 = ceiling / 4 on the
# ceiling would ask of the kernels less than the four evaluations' worth of error the gate grants them -- it would replace the
# gate instead of capping it; below a quarter the gate is the tighter bound anyway and the ceiling stays.  The pairs are what
# one expects: the signed column sums and what is formed from them relative to a sum that happens to cancel in one of up to
# 1 024 channels, grad_x = a (g - mean g - xhat mean(g xhat)) at n = 2, y at sigma << mean (the offset frames, and the narrowest
# channels of a plain frame: rand(c) * 3 reaches 1e-3 against a mean of 5).  tests/test_cpu_bn_frames.py asserts the criterion
# in both directions on every (case, tensor) of the lattice.
NO_CEILING = {
    "sum_g": (
        "widths-c8", "widths-c256", "widths-c1020", "widths-c1024", "caps-c1024-n4088", "caps-c1024-n4096",
        "caps-c1024-n4097", "caps-apply-c1024-n16500", "conditioning-wide-relu", "rowtypes-fp16-c1020", "rowtypes-fp16-cap"),
    "coef_c": (
        "widths-c8", "widths-c256", "widths-c1020", "widths-c1024", "caps-c1024-n4088", "caps-c1024-n4096",
        "caps-c1024-n4097", "caps-apply-c1024-n16500", "conditioning-wide-relu", "rowtypes-fp16-c1020", "rowtypes-fp16-cap"),
    "sum_gx": (
        "widths-c28", "widths-c64", "widths-c128", "widths-c256", "widths-c260", "widths-c344", "widths-c516",
        "widths-c1020", "widths-c1024", "rows-c64-rpp", "rows-c64-8rpp+1", "rows-c64-wgs15", "rows-c64-wgs16",
        "rows-c64-quads", "caps-c64-n65537", "caps-c1024-n4088", "caps-c1024-n4096", "caps-c1024-n4097",
        "caps-apply-c1024-n16500", "conditioning-plain-relu", "conditioning-plain-lin", "conditioning-offset-relu",
        "conditioning-offset-lin", "conditioning-wide-relu", "conditioning-offset-n2", "conditioning-const15-offset-c4",
        "conditioning-const01-offset-c4", "conditioning-w0b0-offset-c4", "conditioning-w0bpos-offset-c4",
        "conditioning-wneg-offset-c4", "conditioning-eps1e-5-offset", "rowtypes-fp16-c64", "rowtypes-fp16-c100",
        "rowtypes-fp16-c1020", "rowtypes-fp16-cap", "rowtypes-fp16-offset", "rowtypes-bf16-c64", "rowtypes-bf16-c100",
        "rowtypes-bf16-c1020", "rowtypes-bf16-cap", "rowtypes-bf16-offset"),
    "coef_b": (
        "widths-c28", "widths-c64", "widths-c128", "widths-c256", "widths-c260", "widths-c344", "widths-c516",
        "widths-c1020", "widths-c1024", "rows-c64-rpp", "rows-c64-8rpp+1", "rows-c64-wgs15", "rows-c64-wgs16",
        "rows-c64-quads", "caps-c64-n65537", "caps-c1024-n4088", "caps-c1024-n4096", "caps-c1024-n4097",
        "caps-apply-c1024-n16500", "conditioning-plain-relu", "conditioning-plain-lin", "conditioning-offset-relu",
        "conditioning-offset-lin", "conditioning-wide-relu", "conditioning-offset-n2", "conditioning-const15-offset-c4",
        "conditioning-const01-offset-c4", "conditioning-w0b0-offset-c4", "conditioning-w0bpos-offset-c4",
        "conditioning-wneg-offset-c4", "conditioning-eps1e-5-offset", "rowtypes-fp16-c64", "rowtypes-fp16-c100",
        "rowtypes-fp16-c1020", "rowtypes-fp16-cap", "rowtypes-fp16-offset", "rowtypes-bf16-c64", "rowtypes-bf16-c100",
        "rowtypes-bf16-c1020", "rowtypes-bf16-cap", "rowtypes-bf16-offset"),
    "y": (
        "widths-c260", "widths-c516", "widths-c1020", "rows-c4-tail1", "caps-c1024-n4096", "caps-apply-c1024-n16500",
        "conditioning-offset-relu", "conditioning-offset-lin", "conditioning-offset-n2", "conditioning-const15-offset-c4",
        "conditioning-const01-offset-c4", "conditioning-w0b0-offset-c4", "conditioning-w0bpos-offset-c4",
        "conditioning-wneg-offset-c4", "conditioning-eps1e-5-offset"),
    "run_mean": (
        "widths-c1020", "widths-c1024", "caps-c1024-n4088", "caps-c1024-n4096", "rowtypes-bf16-c1020"),
    "grad_x": (
        "rows-c64-n2", "rows-c4-n2", "conditioning-offset-n2", "conditioning-eps1e-5-offset"),
}


WORST_CHANNEL_TENSORS = ("sum_gx", "coef_b")


def worst_channel_gate(case, tensor):
    """Verdict (a) takes o32 per channel, except (the tensor's worst channel instead) for the sum of fp32 products sum g xhat and
    the coefficient formed from it, and for grad_x at n = 2, where a column is two numbers that cancel: there a per-channel
    yardstick is one random draw against another (tests/test_cpu_bn_frames.py asserts the need for each)."""
    return tensor in WORST_CHANNEL_TENSORS or (tensor == "grad_x" and case.n == 2)


def has_ceiling(case_name, tensor):
    return case_name not in NO_CEILING.get(tensor, ())


def by_name(name):
    return next(k for k in LATTICE if k.name == name)


# ------------------------------------------------------------------------------------------------------------------------------
# frames (CPU, seeded, fp32; rows rounded into the case's row type)
# ------------------------------------------------------------------------------------------------------------------------------
OFFSET_SIGMA = {"fp32": 0.01, "fp16": 0.25, "bf16": 2.0}      # 16-bit rows: four spacings of the row type at 100 (2^-4, 2^-1)


def rows_of(n, c, kind, seed=11, rows="fp32"):
    g = torch.Generator().manual_seed(seed + 7919 * c + n)
    z = torch.randn(n, c, generator=g)
    if kind == "plain":
        return z * (torch.rand(c, generator=g) * 3) + torch.randn(c, generator=g) * 5
    if kind == "offset":
        return 100.0 + OFFSET_SIGMA[rows] * z
    sig = torch.logspace(-3, 3, c) if c > 1 else torch.ones(1)
    return z * sig + sig * torch.randn(c, generator=g)


@functools.lru_cache(maxsize=4)
def frame(case):
    """dict(x, g [n, c] in the row type; weight, bias [c] fp32 or None; run_mean, run_var [c] fp32 or None) of a case, on the CPU."""
    n, c = case.n, case.c
    x = rows_of(n, c, case.kind, rows=case.rows)
    gen = torch.Generator().manual_seed(1 + 31 * c + n)
    g = torch.randn(n, c, generator=gen)
    w = 0.5 + torch.rand(c, generator=gen)
    b = 0.5 * torch.randn(c, generator=gen)
    rm, rv = torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)
    sp = case.special
    if sp == "const15":
        x[:, CH_CONST] = 1.5
    elif sp == "const01":
        x[:, CH_CONST] = 0.1                                   # float32(0.1): not a dyadic number
    elif sp == "w0b0":
        w[CH_W], b[CH_W] = 0.0, 0.0
    elif sp == "w0bpos":
        w[CH_W], b[CH_W] = 0.0, 0.75
    elif sp == "wneg":
        w[CH_W] = -1.25
    elif sp == "ginf":
        g[n // 2, CH_W] = float("inf")
    dt = DT[case.rows]
    return dict(x=x.to(dt), g=g.to(dt), weight=w if case.affine else None, bias=b if case.affine else None,
                run_mean=rm if case.running else None, run_var=rv if case.running else None)
