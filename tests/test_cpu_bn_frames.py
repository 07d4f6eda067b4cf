"""What tests/test_gpu_bn_lattice.py rests on, checked without a GPU: the restated launch geometry of csrc/bn.hip (bn_frames.py)
against the library's host function and the literal lines of the source, that every group of the lattice reaches the branch it
names, the float64 reference (bn64.py) against nn.BatchNorm1d in float64, autograd and central differences, that an evaluation of
the kernels' precision (bn64.emulate: double column sums, fp32 statistics and element arithmetic) passes verdicts (a) and (b) and
the 0.5 % cap on every case, that a wrong result fails them and still leaves its row -- and the inference fold of a BatchNorm
(link_amd.elk.fold_batchnorm) per channel against float64."""
import json
import os

import pytest
import torch

import bn64
import bn_frames as BF
from ref64 import gate_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE = {k.name: k for k in BF.LATTICE}


# ------------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------------
def test_partial_workgroups_is_the_librarys():
    from link_amd import _lib as L
    lib = L.lib()
    pairs = {(k.n, k.c) for k in BF.LATTICE} | {(n, c, ) for n, c, _ in BF.FALLBACK}
    for c in list(range(0, 1040, 4)) + [1, 2, 3, 5, 6, 7, 1026, 1028, 2048]:
        for n in (-1, 0, 1, 2, 7, 255, 256, 257, 1000, 2047, 2048, 2049, 4096, 4097, 65535, 65536, 65537, 10 ** 6, 1 << 33):
            pairs.add((n, c))
    for n, c in sorted(pairs):
        assert lib.link_bn_partial_workgroups(n, c) == BF.partial_workgroups(n, c), (n, c)


def test_constants_are_the_sources_literal_lines():
    src = open(os.path.join(ROOT, "link_amd", "csrc", "bn.hip")).read()
    for line in (
            "const int cq = c >> 2, rpp = 256 / cq;",                                              # WG, cq, rpp
            "const bool act = r < rpp;",                                                           # active threads
            "const int64_t stride = (int64_t)gridDim.x * rpp;",
            "for (; row + 3 * stride < n; row += 4 * stride) {",                                   # the 4-row loop
            "for (; row < n; row += stride) {",                                                    # the tail loop
            "const int rpp = 256 / (c / 4);",
            "int64_t wgs = (n + (int64_t)rpp * 8 - 1) / ((int64_t)rpp * 8);",                      # ROWS_PER_SLOT
            "if (wgs > 512) wgs = 512;",                                                           # WGS_CAP
            "for (int w = wl; w < wgs; w += 16)",                                                  # GATHER
            "const int64_t wgs = (n * (c / 4) + 256 * 4 - 1) / (256 * 4);",                        # APPLY_PIECES
            "return (unsigned)(wgs < 1 ? 1 : (wgs > 4096 ? 4096 : wgs));",                         # APPLY_CAP
            "static bool bn_width_ok(int32_t c) { return c >= 4 && c <= 1024 && (c & 3) == 0; }",  # the width guard
            "e < total; e += (int64_t)gridDim.x * 256)",                                           # the apply pass strides its grid
    ):
        assert line in src, line
    assert (BF.WG, BF.ROWS_PER_SLOT, BF.WGS_CAP, BF.GATHER, BF.APPLY_PIECES, BF.APPLY_CAP, BF.C_MIN, BF.C_MAX) == \
        (256, 8, 512, 16, 256 * 4, 4096, 4, 1024)
    mod = open(os.path.join(ROOT, "link_amd", "modules.py")).read()
    assert "x.dim() == 2 and x.shape[0] > 1" in mod and "x.shape[1] % 4 == 0 and 4 <= x.shape[1] <= 1024 and self.momentum is not None" in mod
    for n, c, mom in BF.FALLBACK:
        assert not BF.hip_ok(n, c, mom)
    assert [BF.hip_ok(50, c) for c in (2, 6, 1028, 4, 1024)] == [False, False, False, True, True] and not BF.hip_ok(1, 64)


def test_every_group_reaches_the_branch_it_names():
    by = lambda g: [k for k in BF.LATTICE if k.group == g]      # noqa: E731
    assert [k.c for k in by("widths")] == list(BF.WIDTHS) and all(200 <= k.n <= 400 for k in by("widths"))
    idle = {c for c in BF.WIDTHS if BF.active_threads(c) < 256}
    assert idle == {12, 20, 28, 48, 100, 260, 344, 516, 1020}
    assert {c for c in BF.WIDTHS if BF.rpp(c) == 1} == {516, 1020, 1024} and BF.active_threads(1024) == 256
    assert {BF.rpp(c) for c in BF.WIDTHS} >= {256, 128, 64, 16, 4, 2, 1}
    for c in (64, 4):
        r = BF.rpp(c)
        g = {k.name.split("-", 2)[2]: k for k in by("rows") if k.c == c}
        assert [g[s].n for s in ("n2", "rpp-1", "rpp", "rpp+1", "8rpp", "8rpp+1")] == [2, r - 1, r, r + 1, 8 * r, 8 * r + 1]
        assert [BF.partial_workgroups(g[s].n, c) for s in ("wgs15", "wgs16", "wgs17")] == [15, 16, 17]
        assert BF.partial_workgroups(g["8rpp"].n, c) == 1 and BF.partial_workgroups(g["8rpp+1"].n, c) == 2
        # n < rpp: slots without a row; n = 2 leaves all but two empty
        assert BF.slot_passes(g["rpp-1"].n, c, r - 1) == (0, 0) and BF.slot_passes(g["n2"].n, c, 2) == (0, 0)
        assert BF.slot_passes(g["rpp+1"].n, c, 0) == (0, 2) and BF.slot_passes(g["rpp+1"].n, c, 1) == (0, 1)
        # the 4-row loop with an empty tail, and with a tail of one row, in every slot
        assert {BF.slot_passes(g["quads"].n, c, s) for s in range(r)} == {(1, 0)}
        assert {BF.slot_passes(g["tail1"].n, c, s) for s in range(r)} == {(1, 1)}
        assert {BF.slot_passes(g["8rpp"].n, c, s) for s in range(r)} == {(2, 0)}
        assert BF.slot_passes(g["8rpp+1"].n, c, 0) == (1, 1) and BF.slot_passes(g["8rpp+1"].n, c, 1) == (1, 0)
    caps = {k.name: k for k in by("caps")}
    assert [BF.wgs_uncapped(caps[f"caps-c64-n{n}"].n, 64) for n in (65408, 65536, 65537)] == [511, 512, 513]
    assert [BF.wgs_uncapped(caps[f"caps-c1024-n{n}"].n, 1024) for n in (4088, 4096, 4097)] == [511, 512, 513]
    assert BF.partial_workgroups(65537, 64) == 512 == BF.partial_workgroups(4097, 1024)
    assert BF.slot_passes(65537, 64, 0) == (2, 1) and BF.slot_passes(4097, 1024, 0) == (2, 1)        # a ninth row past the cap
    big = caps["caps-apply-c1024-n16500"]
    assert BF.apply_grid_uncapped(big.n, big.c) > BF.APPLY_CAP == BF.apply_grid(big.n, big.c)
    assert all(BF.apply_grid_uncapped(k.n, k.c) <= BF.APPLY_CAP for k in BF.LATTICE if k is not big)
    assert max(k.n * k.c for k in BF.LATTICE) <= 17_000_000
    cond = by("conditioning")
    assert {k.kind for k in cond} == {"plain", "offset", "wide"} and {k.eps for k in cond} == {1e-3, 1e-5}
    assert {k.momentum for k in cond} == {0.01, 0.1, 1.0} and {k.special for k in cond} >= set(BF.SPECIALS[:5])
    opts = by("options")
    assert any(not k.affine for k in opts) and any(not k.running for k in opts) and any(not k.scale for k in opts)
    assert any(not k.coef and k.relu for k in opts) and any(not k.coef and not k.relu for k in opts) and any(not k.relu for k in opts)
    for rt in ("fp16", "bf16"):
        sub = [k for k in by("rowtypes") if k.rows == rt]
        assert {BF.rpp(k.c) for k in sub} >= {256, 16, 10, 1} and any(BF.active_threads(k.c) < 256 for k in sub)
        assert any(BF.wgs_uncapped(k.n, k.c) > BF.WGS_CAP for k in sub) and any(k.kind == "offset" for k in sub)
    assert {k.rows for k in by("nonfinite")} == {"fp32", "fp16"} and all(k.special == "ginf" for k in by("nonfinite"))
    assert all(k in BF.LATTICE for k in BF.MODULE) and len(BF.MODULE) == 11


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", ["widths-c20", "rows-c4-rpp+1", "conditioning-wide-lin", "options-no-affine"])
def test_reference_is_batchnorm1d_in_float64(name, relu):
    case = LATTICE[name]._replace(relu=relu)
    fr = BF.frame(case)
    bn = torch.nn.BatchNorm1d(case.c, eps=case.eps, momentum=case.momentum, affine=case.affine).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(fr["run_mean"]); bn.running_var.copy_(fr["run_var"])
        if case.affine:
            bn.weight.copy_(fr["weight"]); bn.bias.copy_(fr["bias"])
    x = fr["x"].double().requires_grad_(True)
    y = bn(x)
    y = torch.relu(y) if relu else y
    y.backward(fr["g"].double())
    f = bn64.forward(fr["x"], fr["weight"], fr["bias"], fr["run_mean"], fr["run_var"], case.eps, case.momentum)
    b = bn64.backward(f, fr["g"], (f["y"] > 0) if relu else None)
    close = lambda a, r: float((a - r).abs().max()) <= 1e-12 * max(float(r.abs().max()), 1e-300)      # noqa: E731
    assert close(torch.relu(f["y"]) if relu else f["y"], y.detach()) and close(b["grad_x"], x.grad)
    assert close(f["run_mean"], bn.running_mean) and close(f["run_var"], bn.running_var)
    if case.affine:
        assert close(b["sum_gx"], bn.weight.grad) and close(b["sum_g"], bn.bias.grad)


def test_reference_gradient_is_the_central_difference_of_its_forward():
    case = LATTICE["rows-c4-rpp+1"]._replace(n=9)
    fr = {k: (v[:9] if k in ("x", "g") else v) for k, v in BF.frame(LATTICE["rows-c4-rpp+1"]).items()}
    g = fr["g"].double()

    def loss(x):
        f = bn64.forward(x, fr["weight"], fr["bias"], None, None, case.eps, case.momentum)
        return float((torch.relu(f["y"]) * g).sum())

    x = fr["x"].double()
    f = bn64.forward(x, fr["weight"], fr["bias"], None, None, case.eps, case.momentum)
    assert float(f["y"].abs().min()) > 1e-3                       # no element near the kink
    gx = bn64.backward(f, g, f["y"] > 0)["grad_x"]
    h = 1e-6
    for i in range(9):
        for j in range(4):
            e = torch.zeros_like(x)
            e[i, j] = h
            num = (loss(x + e) - loss(x - e)) / (2 * h)
            assert abs(num - float(gx[i, j])) <= 1e-7 * float(gx.abs().max()), (i, j, num, float(gx[i, j]))


def test_channel_gate_is_gate_rows_on_one_column():
    """verdict (a) restates ref64.gate_rows per channel: the same factor, floor and ceilings, on a column that gate_rows itself judges."""
    class Col:
        def __init__(self, col):
            self.col, self.n = col, col.shape[0]

        def rows(self, lo, hi):
            return self.col[lo:hi]

        def rel(self, other):
            got = other.rows(0, self.n) if hasattr(other, "rows") else other
            return float((got.double() - self.col).abs().max() / self.col.abs().max()), bool(torch.isfinite(got).all())

    ref = torch.randn(50, 1, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for dt, ceiling in bn64.CEILING.items():
        for o32, scale, ok in ((1e-7, 1 + 2.3e-6, True), (1e-7, 1 + 2.5e-6, False), (1e-2, 1 + 0.9 * ceiling, True), (1e-2, 1 + 1.1 * ceiling, False)):
            out = (ref * scale).to(torch.float32)
            try:
                gate_rows("col", Col(ref), o32, out, dt=dt, o_round=0.0)
                passed = True
            except AssertionError:
                passed = False
            rel = float(bn64.channel_rel(ref, out)[0])
            mine = rel <= bn64.FACTOR * o32 + bn64.FLOOR and rel < ceiling
            assert passed == mine == ok, (dt, o32, scale)


# ------------------------------------------------------------------------------------------------------------------------------
# the verdicts on an evaluation of the kernels' precision, every case
# ------------------------------------------------------------------------------------------------------------------------------
def _emulated(case):
    fr = BF.frame(case)
    em = bn64.emulate(fr, case)
    truth = bn64.Truth(case, fr, em["y32"])
    return fr, em, truth, {k: v for k, v in em.items() if k in truth.ref}


def test_an_evaluation_of_the_kernels_precision_passes_every_case(monkeypatch):
    """Every case of the lattice: bn64.emulate (the kernels' own expressions in torch) is inside (a) and (b), its mask agrees with
    the float64 mask off the ambiguous elements, and those stay under the 0.5 % cap.  The ceiling is dropped for exactly the
    (tensor, case) pairs whose fp32 evaluation alone exceeds a quarter of it (bn_frames.NO_CEILING), and the worst-channel
    yardstick replaces the per-channel one only where a correct evaluation is shown to exceed the latter
    (bn_frames.worst_channel_gate: sum_gx, coef_b, grad_x at n = 2) -- every other tensor passes per channel."""
    monkeypatch.delenv("LINK_AMD_PARITY_DIR", raising=False)
    worst_share, need = 0.0, {}
    for case in BF.LATTICE:
        fr, em, truth, dev = _emulated(case)
        skip = BF.CH_W if case.special == "ginf" else None
        row = truth.check(case, dev, BF.DT[case.rows], skip=skip)
        worst_share = max(worst_share, truth.share)
        for k, o in truth.o32.items():
            ceiling = bn64.CEILING[BF.DT[case.rows] if k in bn64.ROW_TENSORS else torch.float32]
            o = o.clone()
            if skip is not None:
                o[skip] = 0.0
            assert (float(o.max()) > ceiling / 4) == (not BF.has_ceiling(case.name, k)), (case.name, k, float(o.max()) / ceiling)
            if BF.worst_channel_gate(case, k):
                key = k if k in BF.WORST_CHANNEL_TENSORS else "grad_x at n = 2"
                need[key] = max(need.get(key, 0.0), row[k]["ac"])
            else:
                assert row[k]["a"] == row[k]["ac"] <= 1.0
    assert set(need) == set(BF.WORST_CHANNEL_TENSORS) | {"grad_x at n = 2"} and all(v > 1.0 for v in need.values()), need
    assert 0.0 < worst_share <= bn64.AMBIGUOUS_CAP           # the offset frames do have ambiguous elements
    assert all(name in LATTICE for names in BF.NO_CEILING.values() for name in names)


@pytest.mark.parametrize("fault", ["channel-scaled", "slot-dropped", "mask-flipped"])
def test_a_wrong_result_fails_the_gate_and_leaves_its_row(fault, tmp_path, monkeypatch):
    monkeypatch.setenv("LINK_AMD_PARITY_DIR", str(tmp_path))
    case = LATTICE["widths-c20"]
    fr, em, truth, dev = _emulated(case)
    truth.check(case, dev, torch.float32)
    if fault == "channel-scaled":                            # one channel of y off by a thousandth, small next to its neighbours
        ch = int(truth.ref["y"].abs().amax(0).argmin())
        dev["y"] = dev["y"].clone()
        dev["y"][:, ch] *= 1.001
        words = ("y: (a)", "y: (b)")
    elif fault == "slot-dropped":                            # one of the rpp slots' share of one column sum never added
        r = BF.rpp(case.c)
        dev["mean"] = dev["mean"].clone()
        dev["mean"][3] -= (fr["x"][0::r, 3].double().sum() / case.n).float()
        words = ("mean: (a)", "mean: (b)")
    else:                                                    # an unambiguous element on the wrong side of the mask
        i = int(truth.ref["y"][:, 0].argmax())
        truth.mask_mismatches = bn64.resolve_mask(truth.ref["y"] + 0.0, truth.bounds["y"], -em["y32"])[2]
        assert truth.mask_mismatches > 0 and float(truth.ref["y"][i, 0]) > 0
        words = ()
    with pytest.raises(AssertionError) as err:
        truth.check(case, dev, torch.float32, label="faulty")
    assert all(w in str(err.value) for w in words)
    rows = [json.loads(line) for line in (tmp_path / bn64.PARITY).read_text().splitlines()]
    assert [r["case"] for r in rows] == [case.name, "faulty"] and rows[0]["ok"] and not rows[1]["ok"]
    assert rows[1]["mask_mismatches"] == truth.mask_mismatches


# ------------------------------------------------------------------------------------------------------------------------------
# the inference fold
# ------------------------------------------------------------------------------------------------------------------------------
FOLD_K_SCALE, FOLD_K_SHIFT = 4.0, 7.0


def fold_bounds(mu, beta, cb, sc):
    """Per channel, fold_batchnorm's fp32 evaluation against float64 (u = 2^-24):
      scale = weight * rsqrt(var + eps): the sum rounds (u, halved by the square root), eps is an fp32 number there (u / 2 at
              most), rsqrt is a square root and a division (2 u), the product with the weight rounds (u): 4 u |scale|;
      shift = (-mean * scale + bias) + conv_bias * scale: the two products carry scale's 4 u and round (u each), the two sums
              round (u each, of partial sums no larger than the terms' magnitudes together): 7 u (|mean||scale| + |bias| +
              |conv_bias||scale|)."""
    return FOLD_K_SCALE * bn64.U * sc.abs(), FOLD_K_SHIFT * bn64.U * (mu.abs() * sc.abs() + beta.abs() + cb.abs() * sc.abs())


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("conv_bias", [False, True])
@pytest.mark.parametrize("affine", [True, False])
def test_fold_batchnorm_per_channel_against_float64(affine, conv_bias, eps, half):
    from link_amd.elk import fold_batchnorm
    c = 97
    g = torch.Generator().manual_seed(3)
    bn = torch.nn.BatchNorm1d(c, eps=eps, affine=affine).eval()
    with torch.no_grad():
        bn.running_var.copy_(torch.logspace(-8, 4, c))
        bn.running_mean.copy_(torch.randn(c, generator=g) * torch.logspace(-2, 2, c).flip(0))
        if affine:
            bn.weight.copy_(torch.randn(c, generator=g)); bn.bias.copy_(torch.randn(c, generator=g))
    if half:
        bn = bn.half()
    cb = torch.randn(c, generator=g).to(bn.running_mean.dtype) * 3 if conv_bias else None
    sc, sh = fold_batchnorm(bn, cb)
    assert sc.dtype == sh.dtype == torch.float32 and sc.shape == sh.shape == (c,)
    one, zero = torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    w, beta = (bn.weight.detach().double(), bn.bias.detach().double()) if affine else (one, zero)
    cbd = cb.double() if conv_bias else zero
    mu = bn.running_mean.double()
    sc64 = w / torch.sqrt(bn.running_var.double() + eps)
    sh64 = beta + (cbd - mu) * sc64                              # bn(y + conv_bias) = y sc + sh, from the definition
    bsc, bsh = fold_bounds(mu, beta, cbd, sc64)
    assert bool(((sc.double() - sc64).abs() <= bsc).all()), float(((sc.double() - sc64).abs() / bsc).max())
    assert bool(((sh.double() - sh64).abs() <= bsh).all()), float(((sh.double() - sh64).abs() / bsh).max())
    # and the fold is what the module computes on rows
    y = torch.randn(33, c, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.batch_norm(y + cbd, mu, bn.running_var.double(), w if affine else None, beta if affine else None, False, 0.0, eps)
    assert float((y * sc64 + sh64 - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
