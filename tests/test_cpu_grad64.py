"""tests/grad64.py, the float64 arbiter of R_core's training gradients, checked on its own (no GPU):

  * its float64 autograd gradients agree with central finite differences of its float64 forward, element by element, for the
    three base operations (60 voxels, C = 8: blocks of several voxels with neighbours, two batch items, negative coordinates);
  * they do not depend on the order of the rows (1e-12);
  * gate() refuses one element off by 100 x o32, one NaN element, and a missing tensor -- and passes the float64 and the fp32
    evaluations themselves;
  * o32 on two frames of the GPU tests lies within a factor 3 of the figures measured when the gate was set, so the yardstick
    cannot silently become loose (or tight)."""
import numpy as np
import pytest
import torch

import grad64 as G
from helpers import rel_err

OPS = ["cos", "sin", "cos_x"]


def _small(baseop, n=60, C=8):
    rng = np.random.default_rng(17)
    span = 6                                                  # 60 of 2 x 216 cells (two batch items)
    lin = rng.choice(2 * span ** 3, n, replace=False)
    co = np.stack([lin % span, (lin // span) % span, (lin // span ** 2) % span, lin // span ** 3], 1).astype(np.int32)
    co[:, :3] -= np.array([2, 3, 1], np.int32)                # blocks on both sides of zero
    coords = torch.from_numpy(co)
    groups = 1 if baseop == "cos_x" else 2
    p = {k: (v.double() if v is not None else None) for k, v in G.make_params(C, C // groups, baseop, seed=21).items()}
    g = torch.Generator().manual_seed(22)
    feats = torch.randn(n, C, generator=g, dtype=torch.float64)
    gout = torch.randn(n, C, generator=g, dtype=torch.float64)
    return feats, coords, p, 3, 2, baseop, groups, 1.0, gout  # s = 3: blocks of several voxels, r = 2: 8 neighbour blocks


@pytest.mark.parametrize("baseop", OPS)
def test_float64_gradients_equal_central_differences(baseop):
    """d sum(out * gout) / d x by autograd against (L(x + h) - L(x - h)) / 2h for EVERY element of every input, h = 1e-6.
    Bound 1e-7 of max|gradient| per tensor: the truncation term h^2 / 6 |L'''| (|theta| < 10 here, third derivatives below
    1e3 |L'|) stays under 1e-9 and the rounding term 2^-53 |L| / h under 1e-8 of the gradients, which are O(|L|)."""
    from oracle import link_oracle as lo
    feats, coords, p, s, r, op, groups, div, gout = _small(baseop)
    g = G.reference_grads(feats, coords, p, s, r, op, groups, div, gout)
    inputs = dict({k: v for k, v in p.items() if v is not None}, feats=feats)
    assert set(g) == set(inputs) | {"out"}

    def loss(vals):
        params = {G._STATE_KEYS[k]: v for k, v in vals.items() if k != "feats"}
        out = lo.elk_core_torch(vals["feats"], coords, params, s, r, op, groups, agg=lo.aggregate_torch)
        return float((out * gout).sum())

    h = 1e-6
    for k, x in inputs.items():
        fd = torch.empty_like(x)
        work = {kk: v.clone() for kk, v in inputs.items()}
        flat, out = work[k].view(-1), fd.view(-1)
        for i in range(flat.numel()):
            x0 = float(flat[i])
            flat[i] = x0 + h
            up = loss(work)
            flat[i] = x0 - h
            dn = loss(work)
            flat[i] = x0
            out[i] = (up - dn) / (2 * h)
        assert float(g[k].abs().max()) > 0
        assert rel_err(g[k].numpy(), fd.numpy()) < 1e-7, (k, rel_err(g[k].numpy(), fd.numpy()))


@pytest.mark.parametrize("baseop", OPS)
def test_float64_gradients_do_not_depend_on_the_row_order(baseop):
    feats, coords, p, s, r, op, groups, div, gout = _small(baseop)
    a = G.reference_grads(feats, coords, p, s, r, op, groups, div, gout)
    perm = torch.randperm(feats.shape[0], generator=torch.Generator().manual_seed(5))
    b = G.reference_grads(feats[perm], coords[perm], p, s, r, op, groups, div, gout[perm])
    for k in a:
        bk = b[k]
        if k in ("out", "feats"):
            bk = torch.empty_like(b[k])
            bk[perm] = b[k]
        assert rel_err(bk.numpy(), a[k].numpy()) <= 1e-12, k


def _uniform_case():
    C, baseop, s, r = 64, "cos_x", 3, 2
    coords = G.make_frame("uniform", 6000)
    feats, gout = G.make_rows(coords.shape[0], C)
    return feats, coords, G.make_params(C, C, baseop, seed=11), s, r, baseop, 1, 1.0, gout


def _lidar_sin_case():
    C, baseop, s, r = 16, "sin", 5, 3
    coords = G.make_frame("lidar", 6000)
    feats, gout = G.make_rows(coords.shape[0], C)
    return feats, coords, G.make_params(C, C // 2, baseop, seed=11), s, r, baseop, 2, 1.0, gout


def test_gate_refuses_a_wrong_a_nan_and_a_missing_tensor():
    g64, o32 = G.cached_yardstick(("cpu", "uniform_cos_x"), _uniform_case)
    case = {"suite": "cpu_self_check"}
    exact = {k: v.clone() for k, v in g64.items()}
    G.gate(case, g64, o32, exact)
    G.gate(case, g64, o32, G.reference_grads(*_uniform_case(), dtype=torch.float32))     # e <= o32 by construction
    for k in g64:
        bad = {kk: v.clone() for kk, v in g64.items()}
        flat = bad[k].view(-1)
        flat[flat.numel() // 3] += 100.0 * o32[k] * float(g64[k].abs().max())             # one element, 100 x o32
        with pytest.raises(AssertionError, match="e > 4"):
            G.gate(case, g64, o32, bad)
        bad = {kk: v.clone() for kk, v in g64.items()}
        bad[k].view(-1)[-1] = float("nan")
        with pytest.raises(AssertionError, match="not finite"):
            G.gate(case, g64, o32, bad)
        bad = {kk: v for kk, v in g64.items() if kk != k}
        with pytest.raises(AssertionError, match="missing"):
            G.gate(case, g64, o32, bad)
    # a reference tensor that is zero everywhere has no relative error: refused, not passed
    zero = dict(g64, alpha=torch.zeros_like(g64["alpha"]))
    with pytest.raises(AssertionError, match="no relative error"):
        G.gate(case, zero, o32, zero)
    # 16-bit rows: o_round admits the rounding of the feats gradient into the row type, and nothing else
    for dt in (torch.float16, torch.bfloat16):
        o_round = G.rounding_cost(g64, dt)
        assert o_round["feats"] > 1e-4 and all(v == 0.0 for k, v in o_round.items() if k != "feats")
        rounded = dict(exact, feats=g64["feats"].to(dt))
        G.gate(case, g64, o32, rounded, o_round)
        with pytest.raises(AssertionError, match="e > 4"):
            G.gate(case, g64, o32, rounded)
        with pytest.raises(AssertionError, match="e > 4"):
            G.gate(case, g64, o32, dict(exact, ln_w=g64["ln_w"].to(dt)), o_round)


def test_gate_writes_one_row_per_tensor_before_the_verdict(tmp_path, monkeypatch):
    import json
    g64, o32 = G.cached_yardstick(("cpu", "uniform_cos_x"), _uniform_case)
    monkeypatch.delenv("LINK_AMD_PARITY_DIR", raising=False)
    G.gate({"suite": "cpu_self_check"}, g64, o32, g64)
    assert not list(tmp_path.iterdir())
    monkeypatch.setenv("LINK_AMD_PARITY_DIR", str(tmp_path))
    bad = dict(g64, w_pos=g64["w_pos"] * 1.01)
    with pytest.raises(AssertionError):
        G.gate({"suite": "cpu_self_check", "C": 64}, g64, o32, bad)
    rows = [json.loads(line) for line in (tmp_path / "train_parity.jsonl").read_text().splitlines()]
    assert [r["tensor"] for r in rows] == list(g64)
    for row in rows:
        assert row["C"] == 64 and row["o32"] == o32[row["tensor"]] and row["ok"] == (row["tensor"] != "w_pos")
        assert row["ratio"] == row["e"] / row["o32"]


def _within3(x, lo, hi):
    return lo / 3.0 <= x <= hi * 3.0


def test_o32_is_where_it_was_measured():
    """Figures of the run that set the gate (fp32 autograd of the oracle against float64, both row orders): s_uniform(grid=64)
    C64 cos_x s3 r2: 4e-7 ... 1.9e-6 over the gradient tensors; lidar_like(6000, seed=3) C16 g2 sin s5 r3: w_pos 5.9e-3 ...
    6.1e-3 (heavy cancellation), feats 8.0e-5."""
    g64, o32 = G.cached_yardstick(("cpu", "uniform_cos_x"), _uniform_case)
    print("uniform cos_x:", {k: f"{v:.2e}" for k, v in o32.items()})
    for k, v in o32.items():
        if k != "out":
            assert _within3(v, 4e-7, 1.9e-6), (k, v)
    assert 1e-8 < o32["out"] < 1e-5
    g64, o32 = G.cached_yardstick(("cpu", "lidar_sin"), _lidar_sin_case)
    print("lidar sin:", {k: f"{v:.2e}" for k, v in o32.items()})
    assert _within3(o32["w_pos"], 5.9e-3, 6.1e-3), o32["w_pos"]
    assert _within3(o32["feats"], 8.0e-5, 8.0e-5), o32["feats"]
