"""A float64 reference of the training-mode BatchNorm (csrc/bn.hip) written from the definition, and the bounds the kernels are
held to (tests/test_gpu_bn_lattice.py; checked itself by tests/test_cpu_bn_frames.py against nn.BatchNorm1d in float64, autograd and
central differences).  Plain torch on the tensors' device; dtype=torch.float32 evaluates the same code in fp32 (`o32`).

  mean = sum x / n,  var = sum (x - mean)^2 / n (two passes),  invstd = 1 / sqrt(var + eps),  scale = weight invstd,  shift = bias
  y = (x - mean) scale + shift,  relu(y);   run_mean' = (1 - m) run_mean + m mean,  run_var' = (1 - m) run_var + m var n / (n - 1)
  g' = g where the ReLU let y through,  sum_g = sum g',  sum_gx = sum g' xhat,  xhat = (x - mean) invstd
  grad_x = a g' + bq (x - mean) + cq,  a = weight invstd,  bq = -a invstd sum_gx / n,  cq = -a sum_g / n
  (= a (g' - sum_g / n - xhat sum_gx / n));  grad_weight = sum_gx, grad_bias = sum_g.

16-bit rows: the reference runs on the widened rows and stays unrounded; what rounding it once into the row type costs is o_round
(tests/ref64.py: Rounded), and the per-element bound grows by the row type's unit (below).

The ReLU mask.  y is recomputed in fp32 by the kernels, so an element whose float64 y lies within the forward bound tau of 0 may
land on either side of `> 0`; its grad_x then differs by a whole a g.  Those elements -- |y64| <= tau, tau > 0 -- are AMBIGUOUS: on
them alone the reference takes the device's own y_dev > 0; everywhere else the mask is y64 > 0 and the device's must equal it
(resolve_mask: an assertion on y_dev, no tolerance).  The share of ambiguous elements is capped at AMBIGUOUS_CAP = 0.5 % of a case:
a condition on the frames, shown attainable by the reference's own fp32 evaluation on every case (tests/test_cpu_bn_frames.py).

Verdicts per case (verdict(); the figures go to bn_parity.jsonl through ref64.record_row BEFORE any assertion):
  (a) per channel, the gate of ref64.gate_rows on that channel's column: rel_c = max|dev - ref| / max|ref| over the column (a [c]
      vector's column is one number) <= 4 o32_c + 2 o_round_c + 2e-6, o32_c the larger of two fp32 evaluations of this file's code
      (rows as given, rows permuted) on the same column, and rel_c under the ceiling 1e-4 / 4e-3 / 3e-2 by row type (dropped for
      the pairs of bn_frames.NO_CEILING).  For sum_gx and coef_b, and for grad_x at n = 2, the yardstick is the tensor's worst
      channel instead (bn_frames.worst_channel_gate): a sum of fp32 products that happens to cancel is off by a random amount in
      every evaluation, and one draw of a correct evaluation exceeds 4 x the larger of two other draws in some channel
      (tests/test_cpu_bn_frames.py shows it for each of the three: 1.02 .. 1.45);
  (b) per element, |dev - ref| <= the bound of bounds(), built from the magnitudes of the kernel's own terms with every rounding
      counted (derivations at bounds()); nothing in it comes from the result or from the kernels' output.
Test infrastructure only: does not import link_amd."""
import torch

import bn_frames as BF
from grad64 import FACTOR, FLOOR                       # 4, 2e-6: the gate of tests/ref64.py::gate_rows
from ref64 import record_row

U = 2.0 ** -24                                         # unit roundoff of fp32
V = 2.0 ** -53                                         # ... of float64 (the kernels' accumulators)
UNIT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
F16_SUB = 2.0 ** -25                                   # absolute error of rounding into fp16's subnormal range
CEILING = {torch.float32: 1e-4, torch.float16: 4e-3, torch.bfloat16: 3e-2}      # ref64.gate_rows (b)
AMBIGUOUS_CAP = 0.005
SECOND = 1.0 + 2.0 ** -10                              # products of two first-order terms (each < 2^-10 of its own term)
PARITY = "bn_parity.jsonl"
ROW_TENSORS = ("y", "grad_x")
STAT_TENSORS = ("mean", "invstd", "scale", "run_mean", "run_var")
SUM_TENSORS = ("sum_g", "sum_gx", "coef_a", "coef_b", "coef_c")


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def forward(x, weight, bias, run_mean, run_var, eps, momentum, dtype=torch.float64):
    """{"mean", "var", "invstd", "scale", "shift", "y" (before any ReLU), "d" = x - mean, "run_mean", "run_var" (None without
    running statistics)} in `dtype`."""
    X = x.to(dtype)
    n, c = X.shape
    mean = X.sum(0) / n
    d = X - mean
    var = (d * d).sum(0) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    w = weight.to(dtype) if weight is not None else torch.ones(c, dtype=dtype, device=X.device)
    b = bias.to(dtype) if bias is not None else torch.zeros(c, dtype=dtype, device=X.device)
    scale = w * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=b, d=d, y=d * scale + b, w=w, run_mean=None, run_var=None)
    if run_mean is not None:
        out["run_mean"] = (1.0 - momentum) * run_mean.to(dtype) + momentum * mean
    if run_var is not None:
        unb = var * (n / (n - 1.0)) if n > 1 else var
        out["run_var"] = (1.0 - momentum) * run_var.to(dtype) + momentum * unb
    return out


def backward(fwd, g, mask=None):
    """{"sum_g", "sum_gx", "coef_a", "coef_b", "coef_c", "grad_x", "gm" (the masked gradient), "xhat"} in fwd's dtype; `mask`:
    None (no ReLU) or bool [n, c], where the ReLU let y through."""
    dtype = fwd["d"].dtype
    G = g.to(dtype)
    if mask is not None:
        G = torch.where(mask, G, torch.zeros_like(G))
    n = G.shape[0]
    xhat = fwd["d"] * fwd["invstd"]
    sum_g, sum_gx = G.sum(0), (G * xhat).sum(0)
    a = fwd["w"] * fwd["invstd"]
    bq, cq = -a * fwd["invstd"] * sum_gx / n, -a * sum_g / n
    return dict(sum_g=sum_g, sum_gx=sum_gx, coef_a=a, coef_b=bq, coef_c=cq, grad_x=a * G + bq * fwd["d"] + cq, gm=G, xhat=xhat)


def evaluate(fr, case, mask, dtype, perm=None):
    """The tensors verdict() compares, of one evaluation in `dtype` (rows under `perm`, un-permuted afterwards)."""
    x, g = fr["x"], fr["g"]
    if perm is not None:
        x, g, mask = x[perm], g[perm], (mask[perm] if mask is not None else None)
    f = forward(x, fr["weight"], fr["bias"], fr["run_mean"], fr["run_var"], case.eps, case.momentum, dtype)
    b = backward(f, g, mask)
    y = torch.relu(f["y"]) if case.relu else f["y"]
    out = dict(y=y, grad_x=b["grad_x"], mean=f["mean"], invstd=f["invstd"], scale=f["scale"], run_mean=f["run_mean"],
               run_var=f["run_var"], **{k: b[k] for k in SUM_TENSORS})
    if perm is not None:
        for k in ROW_TENSORS:
            un = torch.empty_like(out[k])
            un[perm] = out[k]
            out[k] = un
    return {k: v for k, v in out.items() if v is not None}, f, b


# ------------------------------------------------------------------------------------------------------------------------------
# bounds, from term magnitudes
# ------------------------------------------------------------------------------------------------------------------------------
def stat_errors(x, f, eps, depth):
    """Per channel, what the kernels' statistics may be off by (f: forward() in float64).  u = 2^-24, v = 2^-53.
      dsum = depth v          a column sum of exact terms accumulated in double, in any order of that depth (bn_frames.sum_depth)
      em   = u |mean| + dsum mean|x|                 mean[ch] = (float)(s / n): one rounding to fp32, the double sum under it
      dvar = (3 depth + 4) v mean(x^2)               var = sq / n - mu^2 in double: the sum sq (dsum mean(x^2)), mu^2 (2 dsum
                                                     mean|x| |mu| <= 2 dsum mean(x^2)) and 4 roundings of terms <= mean(x^2)
      ri   = 1.5 u + dvar / (2 (var + eps)) + 4 v    relative, invstd = (float)(1 / sqrt(var + (double)eps)): the rounding to fp32
                                                     (u), eps taken as an fp32 number where the reference has the double
                                                     (|d eps| <= u eps moves ln invstd by <= u / 2), dvar through the square root,
                                                     and sqrt / divide / add in double
      rs   = ri + u                                  relative, scale = weight * invstd rounded once"""
    X = x.double()
    absx, ex2 = X.abs().mean(0), (X * X).mean(0)
    dsum = depth * V
    em = U * f["mean"].abs() + dsum * absx
    dvar = (3 * depth + 4) * V * ex2
    ri = 1.5 * U + dvar / (2.0 * (f["var"] + eps)) + 4 * V
    return dict(dsum=dsum, em=em, dvar=dvar, ri=ri, rs=ri + U, absx=absx)


def forward_bounds(x, f, case, depth, run_mean, run_var):
    """Bounds of the forward tensors for fp32 rows (f: forward() in float64).  With d = x - mean, s = scale, e = stat_errors():
      y        the kernel forms fl(fl(x - m_f) * s_f + shift) with one fma: d_dev = (d - (m_f - mean)) (1 + d2), |d2| <= u;
               s_f = s (1 + es), |es| <= rs; the fma rounds once (u |y|):
                   tau = |d| |s| (u + rs) + em |s| + u |y|       = 2^-24 (k1 |d| |s| + |mean| |s| + |y|) + the sums' own error,
                   k1 = 1 + rs / u = 3.5 + dvar / (2 u (var + eps)): the subtraction, invstd's rounding and eps (1.5), the scale
                   product and the variance's double error; relu is 1-Lipschitz, so relu(y) keeps the bound
      mean     em;   invstd   ri |invstd|;   scale   rs |scale|
      run_mean u |ref| (the store) + u m (|run_mean| + |mean|) (momentum is an fp32 number in the kernel, a double in the
               reference: |dm| <= u m) + m dsum mean|x|
      run_var  u |ref| + u m (|run_var| + unb) + m dvar n / (n - 1)"""
    e = stat_errors(x, f, case.eps, depth)
    n = x.shape[0]
    d, s = f["d"].abs(), f["scale"].abs()
    out = dict(y=SECOND * (d * s * (U + e["rs"]) + e["em"] * s + U * f["y"].abs()), mean=e["em"], invstd=e["ri"] * f["invstd"],
               scale=e["rs"] * s)
    m = case.momentum
    if run_mean is not None:
        out["run_mean"] = U * f["run_mean"].abs() + U * m * (run_mean.double().abs() + f["mean"].abs()) + m * e["dsum"] * e["absx"]
    if run_var is not None:
        k = n / (n - 1.0) if n > 1 else 1.0
        out["run_var"] = U * f["run_var"].abs() + U * m * (run_var.double().abs() + f["var"] * k) + m * e["dvar"] * k
    return out, e


def backward_bounds(f, b, e):
    """Bounds of the backward tensors for fp32 rows (f, b: forward() / backward() in float64; e: stat_errors()).  With g' the masked
    gradient, A = a, BQ = bq, CQ = cq of the reference:
      sum_g    u |sum_g| (the store) + dsum sum|g'|                      the terms are exact in double
      sum_gx   each term is fl(g' * fl(fl(x - m_f) * is_f)): xhat_dev is off by |xhat| (2 u + ri) + em invstd (the subtraction
               and the product round, invstd is off by ri, the mean by em), the product with g' rounds once more:
                   esx = sum|g'| |xhat| (3 u + ri) + em invstd sum|g'| + dsum sum|g'| |xhat|;     bound = u |sum_gx| + esx
      coef_a   (float)(weight * invstd_f): |A| (u + ri)
      coef_c   (float)(-a sum_g / n) in double: |CQ| (u + ri + 3 v) + |A| dsum sum|g'| / n
      coef_b   (float)(-a invstd_f sum_gx / n): |BQ| (u + 2 ri + 4 v) + |A| invstd esx / n
      grad_x   o = fl(d_dev * bq_f + fl(g' * a_f + cq_f)), two fmas: the outer rounds u |o| <= u (|A||g'| + |BQ||d| + |CQ|), the
               inner u (|A||g'| + |CQ|); d_dev = (d - (m_f - mean)) (1 + d2) costs |BQ| (u |d| + em); the coefficients their own
               bounds ea, eb, ec:
                   2 u (|A||g'| + |BQ||d| + |CQ|) + |g'| ea + |d| eb + ec + |BQ| em
               = 2^-24 k2 (|a||g| + |bq||x - mean| + |cq|) + |bq| em + the sums' error, k2 <= 5 + 2 ri / u = 8 + dvar / (u (var + eps))"""
    n = f["d"].shape[0]
    G, xh, d = b["gm"].abs(), b["xhat"].abs(), f["d"].abs()
    A, BQ, CQ = b["coef_a"].abs(), b["coef_b"].abs(), b["coef_c"].abs()
    sg, sgx = G.sum(0), (G * xh).sum(0)
    ri, em, dsum, inv = e["ri"], e["em"], e["dsum"], f["invstd"]
    esx = SECOND * (sgx * (3 * U + ri) + em * inv * sg) + dsum * sgx
    ea = A * (U + ri)
    ec = CQ * (U + ri + 3 * V) + A * dsum * sg / n
    eb = BQ * (U + 2 * ri + 4 * V) + A * inv * esx / n
    gx = SECOND * (2 * U * (A * G + BQ * d + CQ) + G * ea + d * eb + ec + BQ * em)
    return dict(sum_g=U * b["sum_g"].abs() + dsum * sg, sum_gx=U * b["sum_gx"].abs() + esx, coef_a=ea, coef_b=eb, coef_c=ec,
                grad_x=gx)


def widen_bound(bound, ref, dt):
    """The per-element bound of a result stored in a 16-bit row type: the fp32 value is within `bound`, the store rounds once
    (unit |value|), into fp16's subnormal range at worst 2^-25."""
    if dt == torch.float32:
        return bound
    return bound + UNIT[dt] * (ref.abs() + bound) + (F16_SUB if dt == torch.float16 else 0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the mask
# ------------------------------------------------------------------------------------------------------------------------------
def resolve_mask(y64, tau, y_dev):
    """(mask, ambiguous share, mismatches): the reference's ReLU mask -- y64 > 0, and on the ambiguous elements the device's
    y_dev > 0 (y_dev: the fp32 instance's output, before or after its ReLU) -- and the number of unambiguous elements on which
    the device's mask differs (the caller asserts 0, and share <= AMBIGUOUS_CAP)."""
    amb = (y64.abs() <= tau) & (tau > 0)
    want, got = y64 > 0, y_dev > 0
    bad = int(((want != got) & ~amb).sum())
    return torch.where(amb, got, want), float(amb.double().mean()), bad


# ------------------------------------------------------------------------------------------------------------------------------
# the verdicts
# ------------------------------------------------------------------------------------------------------------------------------
def _cols(t):
    return t.double().reshape(-1, t.shape[-1])


def channel_rel(ref, other):
    """Per channel max|other - ref| / max|ref| ([c] float64; 0 where the reference's column is 0; inf where `other` is not finite)."""
    r, o = _cols(ref), _cols(other)
    e = torch.where(torch.isfinite(o), (o - r).abs(), torch.full_like(r, float("inf"))).amax(0)
    m = r.abs().amax(0)
    return torch.where(m > 0, e / m.clamp_min(1e-300), torch.zeros_like(m)), m


def yardstick(fr, case, mask, seed=0):
    """(ref, o32, f, b): the float64 tensors, per tensor the per-channel o32 (the larger of two fp32 evaluations of the same code:
    rows as given, rows under a seeded permutation) and the float64 forward / backward intermediates for the bounds."""
    ref, f, b = evaluate(fr, case, mask, torch.float64)
    ev_a = evaluate(fr, case, mask, torch.float32)[0]
    perm = torch.randperm(fr["x"].shape[0], generator=torch.Generator().manual_seed(1000 + seed)).to(fr["x"].device)
    ev_b = evaluate(fr, case, mask, torch.float32, perm)[0]
    o32 = {k: torch.maximum(channel_rel(ref[k], ev_a[k])[0], channel_rel(ref[k], ev_b[k])[0]) for k in ref}
    return ref, o32, f, b, ev_a


def _sig(x):
    return float(f"{x:.3g}")


def compact(row):
    """The row as bn_parity.jsonl keeps it: per tensor [rel, o32, a, b] (and o_round behind them where it is not 0) to three
    significant digits, the columns that are 0 in the reference under "zero" where there are any, of the exactness checks their
    number and the names of those that failed."""
    out, zero = {}, {}
    for k, v in row.items():
        if isinstance(v, dict) and "rel" in v:
            out[k] = [_sig(v[f]) for f in ("rel", "o32", "a", "b")] + ([_sig(v["o_round"])] if v["o_round"] else [])
            if v["zero_channels"]:
                zero[k] = v["zero_channels"]
        elif k == "exact":
            out["exact"], failed = len(v), [name for name, ok in v.items() if not ok]
            if failed:
                out["exact_failed"] = failed
        elif k == "ambiguous":
            out[k] = _sig(v)
        elif k != "group":                                           # (the case's name begins with it)
            out[k] = v
    if zero:
        out["zero"] = zero
    return out


def verdict(case, ref, o32, bounds, dev, dt=torch.float32, skip=None, extra=None, record=True, label=None, also=()):
    """Verdicts (a) and (b) of every tensor in `dev` (name -> tensor as the kernels left it) against ref / o32 / bounds (fp32-row
    bounds: widened here for the row tensors of a 16-bit case).  `skip`: a channel left out of both (the non-finite case's).
    `also`: failures found by the caller (the mask, the cap, the exactness checks), part of the row's `ok` and of the verdict.
    One row goes to bn_parity.jsonl first (compact()); then the assertions.  Returns the row."""
    row = dict(case=label or case.name, group=case.group, n=case.n, c=case.c, kind=case.kind, rows=case.rows, relu=case.relu)
    row.update(extra or {})
    bad = []
    keep = None
    for k, got in dev.items():
        r, o = ref[k], o32[k]
        rdt = dt if k in ROW_TENSORS else torch.float32
        rel, m = channel_rel(r, got)
        o_round = channel_rel(r, r.to(rdt))[0] if rdt != torch.float32 else torch.zeros_like(rel)
        err = torch.where(torch.isfinite(_cols(got)), (_cols(got) - _cols(r)).abs(), torch.full_like(_cols(r), float("inf")))
        bnd = _cols(widen_bound(bounds[k], r, rdt)).expand_as(err)
        ratio = torch.where(err > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err)).amax(0)
        if skip is not None:
            keep = torch.ones_like(rel, dtype=torch.bool)
            keep[skip] = False
            rel, ratio, o, o_round = rel[keep], ratio[keep], o[keep], o_round[keep]
        # per channel against that channel's own o32; against the tensor's worst channel only where bn_frames.worst_channel_gate
        # names the tensor or the case (figures of both are kept in the returned row: "ac", "aw")
        ac = float((rel / (FACTOR * o + 2.0 * o_round + FLOOR)).max())
        aw = float(rel.max()) / (FACTOR * float(o.max()) + 2.0 * float(o_round.max()) + FLOOR)
        absolute = BF.has_ceiling(case.name, k)
        fig = dict(rel=float(rel.max()), o32=float(o.max()), o_round=float(o_round.max()),
                   a=aw if BF.worst_channel_gate(case, k) else ac, ac=ac, aw=aw, b=float(ratio.max()), zero_channels=int((m == 0).sum()))
        row[k] = fig
        if not fig["a"] <= 1.0:
            bad.append(f"{k}: (a) rel / (4 o32 + 2 o_round + 2e-6) = {fig['a']:.3g} (worst channel of the kept ones: {int(rel.argmax())})")
        if absolute and not fig["rel"] < CEILING[rdt]:
            bad.append(f"{k}: (a) rel = {fig['rel']:.3g} over the ceiling {CEILING[rdt]}")
        if not fig["b"] <= 1.0:
            bad.append(f"{k}: (b) err / bound = {fig['b']:.3g} (worst channel of the kept ones: {int(ratio.argmax())})")
    bad += list(also)
    row["ok"] = not bad
    if record:
        record_row(compact(row), PARITY)
    assert not bad, "\n".join(bad) + "\n" + repr(row)
    return row


# ------------------------------------------------------------------------------------------------------------------------------
# one case, end to end
# ------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a * b + c) of fp32 tensors with one rounding: the product of two fp32 numbers is exact in double."""
    return (a.double() * b.double() + c.double()).float()


def emulate(fr, case):
    """The kernels' own expressions restated in torch (bn.hip: k_col_moments, k_bn_finalize_*, k_bn_apply): column sums in double
    over fp32 terms, statistics rounded to fp32 once, fp32 element arithmetic with single-rounded fmas, the mask recomputed from
    x.  Not the device: what tests/test_cpu_bn_frames.py feeds the verdicts to show that a correct evaluation of this precision
    passes them.  Returns the tensors verdict() compares (rows in the case's row type)."""
    x, g = fr["x"].float(), fr["g"].float()
    n, c = x.shape
    eps, mom = float(torch.tensor(case.eps, dtype=torch.float32)), float(torch.tensor(case.momentum, dtype=torch.float32))
    mu = x.double().sum(0) / n
    var = ((x.double() ** 2).sum(0) / n - mu * mu).clamp_min(0.0)
    mean, invstd = mu.float(), (1.0 / torch.sqrt(var + eps)).float()
    w = fr["weight"] if fr["weight"] is not None else torch.ones(c, device=x.device)
    shift = fr["bias"] if fr["bias"] is not None else torch.zeros(c, device=x.device)
    scale = w * invstd
    out = dict(mean=mean, invstd=invstd, scale=scale)
    if fr["run_mean"] is not None:
        out["run_mean"] = ((1.0 - mom) * fr["run_mean"].double() + mom * mu).float()
    if fr["run_var"] is not None:
        out["run_var"] = ((1.0 - mom) * fr["run_var"].double() + mom * (var * (n / (n - 1.0)) if n > 1 else var)).float()
    d = x - mean
    y = _fma(d, scale, shift)
    gm = torch.where(y > 0, g, torch.zeros_like(g)) if case.relu else g
    s, sx = gm.double().sum(0), (gm * (d * invstd)).double().sum(0)
    a = w.double() * invstd.double()
    ca, cb, cc = a.float(), (-a * invstd.double() * sx / n).float(), (-a * s / n).float()
    gx = _fma(d, cb, _fma(gm, ca, cc))
    dt = fr["x"].dtype
    out.update(y=(torch.relu(y) if case.relu else y).to(dt), y32=y, grad_x=gx.to(dt), sum_g=s.float(), sum_gx=sx.float(),
               coef_a=ca, coef_b=cb, coef_c=cc)
    return out


class Truth:
    """Everything verdict() needs of one case: the float64 forward, the mask resolved against the fp32 instance's y (`y_dev`),
    the float64 backward under that mask, o32 and the bounds.  `share` / `mask_mismatches`: resolve_mask's figures (the caller
    asserts on them after the row is written)."""

    def __init__(self, case, fr, y_dev, seed=0):
        depth = BF.sum_depth(case.n, case.c)
        f = forward(fr["x"], fr["weight"], fr["bias"], fr["run_mean"], fr["run_var"], case.eps, case.momentum)
        fb, e = forward_bounds(fr["x"], f, case, depth, fr["run_mean"], fr["run_var"])
        self.share, self.mask_mismatches, self.mask = 0.0, 0, None
        if case.relu:
            self.mask, self.share, self.mask_mismatches = resolve_mask(f["y"], fb["y"], y_dev)
        self.ref, self.o32, f, b, self.ev32 = yardstick(fr, case, self.mask, seed)
        self.bounds = dict(fb, **backward_bounds(f, b, e))

    def check(self, case, dev, dt, skip=None, label=None, record=True, extra=None):
        also = [f"exact: {k}" for k, ok in ((extra or {}).get("exact") or {}).items() if not ok]
        if self.mask_mismatches:
            also.append(f"mask: {self.mask_mismatches} unambiguous elements on the other side of y > 0")
        if not self.share <= AMBIGUOUS_CAP:
            also.append(f"mask: {self.share:.3g} of the elements ambiguous, over the cap {AMBIGUOUS_CAP}")
        return verdict(case, self.ref, self.o32, self.bounds, dev, dt, skip=skip, label=label, record=record, also=also,
                       extra=dict(extra or {}, ambiguous=self.share, mask_mismatches=self.mask_mismatches))
