"""The training-mode BatchNorm kernels (csrc/bn.hip, C ABI section F: forward statistics, apply, backward reduce plain and relu,
backward apply, and their _io twins for fp16 / bf16 rows) behind a float64 gate per channel and per element, over a stated lattice
of launch geometries and frames (tests/bn_frames.py; checked without a device by tests/test_cpu_bn_frames.py):

  widths        c = 4 .. 1024: every threads-per-row class, idle threads (c = 12, 20, 28, 48, 100, 260, 344, 516, 1020), rpp = 1;
  rows          at rpp = 16 and rpp = 256: n = 2, rpp - 1 / rpp / rpp + 1 (slots without a row), 8 rpp and one more (a second
                workgroup), 15 / 16 / 17 workgroups in the finalise's 16-way sum, the 4-row loop with an empty tail and with a
                tail of one row;
  caps          511 / 512 / 513 workgroups' worth of rows at c = 64 and c = 1024; the apply pass's 4 096-workgroup cap (16 500 x 1 024);
  conditioning  plain / offset (mean 100, sigma 0.01) / wide (sigma 1e-3 .. 1e3) frames, constant channels, weight 0 with bias 0
                and with bias > 0, a negative weight, eps 1e-3 / 1e-5, momentum 0.01 / 0.1 / 1;
  options       no affine, no running statistics, scale / shift null in forward_stats, coef null in backward_reduce, relu on / off;
  rowtypes      fp16 and bf16 rows over one case per rpp class, a cap case, the offset kind and the weight-0 channel;
  nonfinite     one inf in the upstream gradient: its channel is non-finite, its float4 neighbours and all others are gated.

The entries are driven through link_amd._lib directly; every output buffer, and the partial workspace with a guard of 16 more
workgroups' slots behind it, starts as NaN, so a slot that was never written, a read past wgs or a write past it shows.  Per case
(tests/bn64.py holds the reference, the mask rule and the derivations; nothing in a bound comes from the kernels):
  (a) per channel the gate of ref64.gate_rows, (b) per element the bounds built from term magnitudes, the device's ReLU mask
      equal to the float64 mask off the ambiguous elements (at most 0.5 % of a case);
  (c) a second pass on another stream is bit-equal (fp32 rows: through the _io twins with the fp32 row type); a 16-bit instance is
      bit-equal to the fp32 instance on the widened rows, rounded once (row_io.h); the weight-0, bias-0 channel has y == 0 and
      grad_x == 0 exactly.
Then the module path (link_amd.BatchNorm with and without the folded ReLU, the fused container's training path, torch.autocast,
two steps, num_batches_tracked), the fallback cases, and the inference fold Conv3d(1x1x1) -> BatchNorm -> ReLU per element.
Every case leaves its figures in bn_parity.jsonl in the directory LINK_AMD_PARITY_DIR names before any verdict
(profiles/bn_parity.jsonl is one run)."""
import copy

import pytest
import torch

import bn64
import bn_frames as BF
from ref64 import record_row

pytestmark = pytest.mark.gpu
GUARD = 16                                       # workgroups' worth of NaN slots behind the partial workspace


def _dev(case):
    return {k: (v.cuda() if v is not None else None) for k, v in BF.frame(case).items()}


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _p(t):
    return t.data_ptr() if t is not None else None


def run_entries(case, fr, io_entries, stream=None):
    """The five entries on one frame: forward statistics, apply, backward reduce (relu form when case.relu), backward apply.
    `io_entries`: through the _io twins with the rows' own type (else the plain fp32 entries: fp32 rows only).  `stream`: None
    (the current one) or a torch.cuda.Stream.  Returns the tensors bn64.verdict compares (+ "shift", "partial")."""
    from link_amd import _lib as L
    lib = L.lib()
    x, g = fr["x"], fr["g"]
    n, c = x.shape
    io = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}[x.dtype]
    assert io_entries or io == L.IO_F32
    wgs = int(lib.link_bn_partial_workgroups(n, c))
    assert wgs == BF.partial_workgroups(n, c)
    w, b = fr["weight"], fr["bias"]
    rm = fr["run_mean"].clone() if fr["run_mean"] is not None else None
    rv = fr["run_var"].clone() if fr["run_var"] is not None else None
    partial = _nan((wgs + GUARD) * 2 * c, dtype=torch.float64)
    vec, out = _nan(4, c), _nan(5, c)                               # mean | invstd | scale | shift;  sum_g | sum_gx | a | bq | cq
    y, gx = _nan(n, c, dtype=x.dtype), _nan(n, c, dtype=x.dtype)
    extra = {}
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    st = stream.cuda_stream if stream is not None else L.current_stream_handle()

    def stats(mean, invstd, rm_, rv_, scale, shift):
        tail = (n, c, float(case.eps), float(case.momentum), _p(partial), _p(mean), _p(invstd), _p(rm_), _p(rv_), _p(w), _p(b),
                _p(scale), _p(shift), st)
        if io_entries:
            L.check(lib.link_bn_forward_stats_io(_p(x), io, *tail), "link_bn_forward_stats_io")
        else:
            L.check(lib.link_bn_forward_stats(_p(x), *tail), "link_bn_forward_stats")

    def reduce(sum_g, sum_gx, coef):
        tail = (n, c, _p(partial), _p(sum_g), _p(sum_gx), _p(w), _p(coef), st)
        head = (_p(g), _p(x)) + ((io,) if io_entries else ())
        name = "link_bn_backward_reduce" + ("_relu" if case.relu else "") + ("_io" if io_entries else "")
        mid = (_p(vec[0]), _p(vec[1])) + ((_p(vec[2]), _p(vec[3])) if case.relu else ())
        L.check(getattr(lib, name)(*head, *mid, *tail), name)

    if not case.scale:                                              # statistics alone: no scale / shift asked for
        first = _nan(2, c)
        stats(first[0], first[1], rm, rv, None, None)
        stats(vec[0], vec[1], None, None, vec[2], vec[3])
        extra["first_stats"] = first
    else:
        stats(vec[0], vec[1], rm, rv, vec[2], vec[3])
    if io_entries:
        L.check(lib.link_bn_apply_forward_io(_p(x), io, _p(vec[0]), _p(vec[2]), _p(vec[3]), n, c, int(case.relu), _p(y), st),
                "link_bn_apply_forward_io")
    else:
        L.check(lib.link_bn_apply_forward(_p(x), _p(vec[0]), _p(vec[2]), _p(vec[3]), n, c, int(case.relu), _p(y), st),
                "link_bn_apply_forward")
    if not case.coef:                                               # the sums alone: no coefficients asked for
        first = _nan(2, c)
        reduce(first[0], first[1], None)
        extra["first_sums"] = first
    reduce(out[0], out[1], out[2:])
    sc, sh = (_p(vec[2]), _p(vec[3])) if case.relu else (None, None)
    if io_entries:
        L.check(lib.link_bn_apply_backward_io(_p(g), _p(x), io, _p(vec[0]), _p(out[2:]), sc, sh, n, c, _p(gx), st),
                "link_bn_apply_backward_io")
    else:
        L.check(lib.link_bn_apply_backward(_p(g), _p(x), _p(vec[0]), _p(out[2:]), sc, sh, n, c, _p(gx), st), "link_bn_apply_backward")
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    res = dict(mean=vec[0], invstd=vec[1], scale=vec[2], shift=vec[3], y=y, grad_x=gx, sum_g=out[0], sum_gx=out[1], coef_a=out[2],
               coef_b=out[3], coef_c=out[4], partial=partial, **extra)
    if rm is not None:
        res.update(run_mean=rm, run_var=rv)
    return res


def _same(a, b):
    """Bit-equal, NaN positions included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _workspace_clean(case, res):
    wgs, c = BF.partial_workgroups(case.n, case.c), case.c
    p = res["partial"]
    return bool(torch.isnan(p[wgs * 2 * c:]).all()) and (case.special == "ginf" or bool(torch.isfinite(p[:wgs * 2 * c]).all()))


@pytest.mark.parametrize("case", BF.LATTICE, ids=[k.name for k in BF.LATTICE])
def test_bn_entries_against_float64(case):
    fr = _dev(case)
    dt = BF.DT[case.rows]
    half = dt != torch.float32
    res = run_entries(case, fr, io_entries=half)
    wide = dict(fr, x=fr["x"].float(), g=fr["g"].float())
    res32 = run_entries(case, wide, io_entries=False) if half else res
    truth = bn64.Truth(case, fr, res32["y"])
    skip = BF.CH_W if case.special == "ginf" else None
    names = [k for k in truth.ref if k in res]
    exact = {}
    # (c) exactness, measured before any verdict
    again = run_entries(case, fr, io_entries=True, stream=torch.cuda.Stream())
    exact["second_pass_other_stream"] = all(_same(res[k], again[k]) for k in names + ["shift"])
    exact["workspace"] = _workspace_clean(case, res) and _workspace_clean(case, again)
    exact["shift_is_bias"] = _same(res["shift"], fr["bias"] if fr["bias"] is not None else torch.zeros_like(res["shift"]))
    if half:
        exact["rows_rounded_once"] = _same(res["y"], res32["y"].to(dt)) and _same(res["grad_x"], res32["grad_x"].to(dt))
        exact["vectors_equal_fp32_instance"] = all(_same(res[k], res32[k]) for k in names if k not in bn64.ROW_TENSORS)
    if case.special == "w0b0":
        exact["zero_channel"] = bool((res["y"][:, BF.CH_W] == 0).all()) and bool((res["grad_x"][:, BF.CH_W] == 0).all()) and \
            float(res["sum_g"][BF.CH_W]) == 0.0 == float(res["sum_gx"][BF.CH_W])
    if "first_stats" in res:
        exact["stats_without_scale"] = _same(res["first_stats"][0], res["mean"]) and _same(res["first_stats"][1], res["invstd"])
    if "first_sums" in res:
        exact["sums_without_coef"] = _same(res["first_sums"][0], res["sum_g"]) and _same(res["first_sums"][1], res["sum_gx"])
    if skip is not None:
        ch = skip
        exact["inf_channel_not_finite"] = not bool(torch.isfinite(res["grad_x"][:, ch].float()).any()) and not any(
            bool(torch.isfinite(res[k][ch])) for k in ("sum_g", "coef_c"))
    # the row (figures of (a), (b) and the exactness checks) is written before any verdict
    truth.check(case, {k: res[k] for k in names}, dt, skip=skip, extra=dict(exact=exact))
    assert all(exact.values()), exact


# ------------------------------------------------------------------------------------------------------------------------------
# the module path
# ------------------------------------------------------------------------------------------------------------------------------
def _module(case, fr):
    import link_amd as la
    bn = la.BatchNorm(case.c, eps=case.eps, momentum=case.momentum, affine=case.affine, track_running_stats=case.running).cuda().train()
    with torch.no_grad():
        if case.affine:
            bn.weight.copy_(fr["weight"]); bn.bias.copy_(fr["bias"])
        if case.running:
            bn.running_mean.copy_(fr["run_mean"]); bn.running_var.copy_(fr["run_var"])
    return bn


@pytest.mark.parametrize("case", BF.MODULE, ids=[k.name for k in BF.MODULE])
def test_bn_module_path_two_steps(case, monkeypatch):
    """link_amd.BatchNorm in training mode over two steps (the second starts from the first's running statistics): relu cases run
    through the fused container's training path (BatchNorm + ReLU in one pass).  torch.autocast: the 16-bit cases hand in rows that
    are already in the region's type, as the convolution in front of a BatchNorm leaves them; the fp32 cases run a twin module on
    the fp32 rows inside an fp16 region (first step) and a bf16 region (second step), which must take the native fp32 kernels and
    give, bit for bit, what the module gives outside any region.  Same verdicts."""
    import link_amd as la
    fr = _dev(case)
    dt = BF.DT[case.rows]
    half = dt != torch.float32
    coords = torch.zeros(case.n, 4, dtype=torch.int32, device="cuda")
    calls = []
    orig = torch.nn.functional.batch_norm
    monkeypatch.setattr(torch.nn.functional, "batch_norm", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    bn = _module(case, fr)
    bn32 = copy.deepcopy(bn)
    net = bn
    if case.relu and case.running:                                  # what fuse_for_inference leaves of [Conv3d, BatchNorm, ReLU]: its tail
        seq = la.fuse_for_inference(torch.nn.Sequential(torch.nn.Sequential(la.Conv3d(case.c, case.c, 1), bn, la.ReLU(True))))[0]
        assert type(seq) is la.modules._FusedSequential
        net = type(seq)(bn, seq[2]).cuda().train()
        net._link_groups = {}

    def step(m, x, g, region):
        xs = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=region or torch.float16, enabled=region is not None):
            st = la.SparseTensor(xs, coords, 1)
            y = m(st, relu=case.relu) if isinstance(m, la.BatchNorm) else m(st)      # (without running statistics nothing folds)
        y = y.F
        bn_ = m if isinstance(m, la.BatchNorm) else m[0]
        bn_.zero_grad()
        y.backward(g.to(y.dtype))
        out = dict(y=y.detach(), grad_x=xs.grad)
        if case.affine:
            out.update(sum_gx=bn_.weight.grad.clone(), sum_g=bn_.bias.grad.clone())
        if case.running:
            out.update(run_mean=bn_.running_mean.clone(), run_var=bn_.running_var.clone())
        return out

    for s in range(2):
        now = dict(fr)
        if case.running:
            now.update(run_mean=bn.running_mean.clone(), run_var=bn.running_var.clone())
        dev = step(net, fr["x"], fr["g"], dt if half else None)
        dev32 = step(bn32, fr["x"].float(), fr["g"].float(), None if half else (torch.float16, torch.bfloat16)[s])
        assert dev["y"].dtype == dt and dev["grad_x"].dtype == dt
        truth = bn64.Truth(case, now, dev32["y"], seed=s)
        truth.check(case, dev, dt, label=f"module/{case.name}/step{s}")
        if half:
            assert _same(dev["y"], dev32["y"].to(dt)) and _same(dev["grad_x"], dev32["grad_x"].to(dt))
            assert all(_same(dev[k], dev32[k]) for k in dev if k not in bn64.ROW_TENSORS)
        else:                                                       # fp32 rows entering an autocast region: the same fp32 kernels
            assert all(_same(dev[k], dev32[k]) for k in dev)
        if case.running:
            assert int(bn.num_batches_tracked) == int(bn32.num_batches_tracked) == s + 1
    assert not calls                                                # torch's batch_norm never ran


@pytest.mark.parametrize("n,c,momentum", BF.FALLBACK)
def test_bn_fallback_cases_take_torchs_batch_norm(n, c, momentum, monkeypatch):
    import link_amd as la
    assert not BF.hip_ok(n, c, momentum)
    calls, native = [], []
    orig, real = torch.nn.functional.batch_norm, la.modules._BatchNormTrain.apply
    monkeypatch.setattr(torch.nn.functional, "batch_norm", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    monkeypatch.setattr(la.modules._BatchNormTrain, "apply", staticmethod(lambda *a, **k: (native.append(1), real(*a, **k))[1]))
    bn = la.BatchNorm(c, momentum=momentum).cuda().train()
    x = BF.rows_of(n, c, "plain").cuda()
    st = la.SparseTensor(x, torch.zeros(n, 4, dtype=torch.int32, device="cuda"), 1)
    if n == 1:
        with pytest.raises(ValueError):                             # torch's own refusal of one value per channel
            bn(st)
    else:
        y = bn(st).F
        f = bn64.forward(x, bn.weight.detach(), bn.bias.detach(), None, None, bn.eps, 0.0)
        assert float(bn64.channel_rel(f["y"], y.detach())[0].max()) < 1e-3
    assert calls == [1] and not native


# ------------------------------------------------------------------------------------------------------------------------------
# the inference fold: Conv3d(c, c', 1) -> BatchNorm -> ReLU through fuse_for_inference
# ------------------------------------------------------------------------------------------------------------------------------
def _fold_net(c, co, seed=0):
    import link_amd as la
    torch.manual_seed(seed)
    conv, bn = la.Conv3d(c, co, 1, bias=True), la.BatchNorm(co, eps=1e-3)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        conv.kernel.copy_(torch.randn(c, co, generator=g) / c ** 0.5)
        conv.bias.copy_(torch.randn(co, generator=g))
        bn.weight.copy_(0.5 + torch.rand(co, generator=g)); bn.bias.copy_(0.3 * torch.randn(co, generator=g))
        bn.running_mean.copy_(torch.randn(co, generator=g)); bn.running_var.copy_(torch.logspace(-2, 1, co))
    plain = torch.nn.Sequential(conv, bn, la.ReLU(True)).cuda().eval()
    fused = la.fuse_for_inference(torch.nn.Sequential(copy.deepcopy(plain)))[0].cuda().eval()
    return plain, fused


def _fold_terms(net, x):
    """(ref, M, A) in float64: relu(((x @ W + cb) - mu) sc + beta), its term magnitude M = (|x| @ |W| + |cb| + |mu|) |sc| + |beta|
    and A = (|x| @ |W|) |sc|."""
    conv, bn = net[0], net[1]
    W, cb = conv.kernel.detach().double(), conv.bias.detach().double()
    mu, sc = bn.running_mean.double(), bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    beta = bn.bias.detach().double()
    X = x.double()
    ref = torch.relu((X @ W + cb - mu) * sc + beta)
    A = (X.abs() @ W.abs()) * sc.abs()
    return ref, A + (cb.abs() + mu.abs()) * sc.abs() + beta.abs(), A


@pytest.mark.parametrize("c,co", [(16, 16), (20, 36), (64, 128)])
def test_fold_1x1x1_conv_batchnorm_relu(c, co):
    """fp32 rows per element against float64: the row's dot product of c terms in any order ((c + 2) u A), scale's 4 u on it, the
    shift's 7 u (|mu||sc| + |beta| + |cb||sc|) (tests/test_cpu_bn_frames.py: fold_bounds) and addcmul's product and sum (2 u M):
    E = (c + 15) u M covers them all; against the unfused container 2 E (both sides are fp32 evaluations).  16-bit rows against the
    unfused container with its convolution's parameters in the row type: that path rounds the kernel, the bias, the product row,
    the biased row and the BatchNorm's output into the row type (5 v M), the fused path its result (v M): 6 v M + 2 E.  Under
    autocast the unfused convolution rounds rows, kernel and bias to fp16 and its three results to the region's type (6), the
    fused branch's matmul rounds rows, kernel and product to the region's type (3; the same roundings where the region is fp16):
    at most 7 v M + 2 E with v the coarser unit.  The 1x1x1 branch of forward_affine returns the input's row type, as its table
    branch does."""
    import link_amd as la
    n = 1003
    plain, fused = _fold_net(c, co)
    assert type(fused) is la.modules._FusedSequential
    x = torch.randn(n, c, generator=torch.Generator().manual_seed(9)).cuda()
    coords = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    coords[:, 0] = torch.arange(n, dtype=torch.int32)
    table_conv = la.Conv3d(c, co, 3).cuda().eval()                   # the table branch of forward_affine, for the dtype it returns
    sc, sh = la.elk.fold_batchnorm(plain[1], plain[0].bias)
    fig = dict(case=f"fold/c{c}-{co}")
    bad = []
    with torch.no_grad():
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            xs = x.to(dt)
            ref, M, A = _fold_terms(plain, xs)
            yf = fused(la.SparseTensor(xs, coords, 1)).F
            twin = plain if dt == torch.float32 else copy.deepcopy(plain)
            twin[0].to(dt)                                            # 16-bit rows: the convolution's parameters in the row type
            yp = twin(la.SparseTensor(xs, coords, 1)).F
            yt = table_conv.forward_affine(la.SparseTensor(xs, coords, 1), sc, sh, True).F
            E = (c + 15) * bn64.U * M
            name = str(dt).split(".")[1]
            if dt == torch.float32:
                fig["f32_vs_f64"] = float(((yf.double() - ref).abs() / E).max())
                fig["f32_vs_unfused"] = float(((yf.double() - yp.double()).abs() / (2 * E)).max())
                ok = fig["f32_vs_f64"] <= 1 and fig["f32_vs_unfused"] <= 1
            else:
                v = bn64.UNIT[dt]
                fig[name + "_vs_unfused"] = float(((yf.double() - yp.double()).abs() / (6 * v * M + 2 * E + 2 * bn64.F16_SUB)).max())
                ok = fig[name + "_vs_unfused"] <= 1
            fig[name + "_dtypes"] = [str(yf.dtype), str(yt.dtype), str(yp.dtype)]
            if not (ok and yf.dtype == yt.dtype == dt and bool(torch.isfinite(yf).all())):
                bad.append(name)
        for dt in (torch.float16, torch.bfloat16):
            ref, M, A = _fold_terms(plain, x)
            with torch.autocast("cuda", dtype=dt):
                yf = fused(la.SparseTensor(x, coords, 1)).F
                yp = plain(la.SparseTensor(x, coords, 1)).F
                yt = table_conv.forward_affine(la.SparseTensor(x, coords, 1), sc, sh, True).F
            name = "autocast_" + str(dt).split(".")[1]
            v = max(bn64.UNIT[dt], bn64.UNIT[torch.float16])        # the convolution rounds to fp16 under either region
            fig[name] = float(((yf.double() - yp.double()).abs() / (7 * v * M + 2 * (c + 15) * bn64.U * M + 2 * bn64.F16_SUB)).max())
            if not (fig[name] <= 1 and bool(torch.isfinite(yf).all()) and yf.dtype == yt.dtype):     # both branches: one dtype in a region too
                bad.append(name)
    record_row({k: (bn64._sig(v) if isinstance(v, float) else v) for k, v in fig.items() if not k.endswith("_dtypes")}, bn64.PARITY)
    assert not bad, (bad, fig)
