"""The float64 arbiter of R_core's training gradients (tests/test_gpu_train_gate.py, tests/test_gpu_train.py,
tests/test_gpu_amp_train.py; checked itself by tests/test_cpu_grad64.py).

reference_grads   autograd over oracle.link_oracle.elk_core_torch with aggregate_torch on the CPU, every tensor a leaf in `dtype`.
yardstick         (g64, o32): the float64 result and, per tensor, what evaluating the SAME formula in fp32 costs against it -- the
                  larger of two fp32 evaluations (rows as given; rows under a seeded permutation, un-permuted afterwards: the
                  order of the fp32 sums alone moves the figure by up to 2x).
gate              per tensor: finite, present, max|g64| > 0 and rel_err(got, g64) <= 4 * o32 + 2 * o_round + 2e-6 -- the forward
                  gate of tests/test_gpu_sizes.py::_gate with its factor and floor, for its reason: the kernels evaluate the
                  reference's formula in fp32 in another operation order.  Nothing in the bound comes from the code under test.
                  One row per tensor goes to $LINK_AMD_PARITY_DIR/train_parity.jsonl before the verdict (no file when unset).

The metric is helpers.rel_err: max-norm relative to max|ref|, per tensor.  Test infrastructure only: does not import link_amd."""
import json
import os

import numpy as np
import torch

from helpers import lidar_like, rel_err, s_uniform

PARAMS = ("w_pre", "pre_ln_w", "pre_ln_b", "w_pos", "alpha", "ln_w", "ln_b")
FACTOR, FLOOR = 4.0, 2e-6                      # tests/test_gpu_sizes.py::_gate
_STATE_KEYS = {"w_pre": "pre_mix.0.weight", "pre_ln_w": "pre_mix.1.weight", "pre_ln_b": "pre_mix.1.bias",
               "w_pos": "pos_weight.0.weight", "alpha": "alpha", "ln_w": "norm.weight", "ln_b": "norm.bias"}


# ------------------------------------------------------------------------------------------------------------------- inputs
def make_params(C, cg, baseop, seed):
    """The seeded parameter set of the training tests (CPU, fp32): {"w_pre", ..., "alpha" (None unless cos_x), ...}."""
    g = torch.Generator().manual_seed(seed)
    return {
        "w_pre": torch.randn(C, C, generator=g) / C ** 0.5,
        "pre_ln_w": 1 + 0.1 * torch.randn(C, generator=g), "pre_ln_b": 0.1 * torch.randn(C, generator=g),
        "w_pos": 0.3 * torch.randn(cg, 3, generator=g),
        "alpha": (1 + 0.2 * torch.randn(1, cg, generator=g)) if baseop == "cos_x" else None,
        "ln_w": 1 + 0.1 * torch.randn(C, generator=g), "ln_b": 0.1 * torch.randn(C, generator=g),
    }


def make_frame(kind, n, div=1.0):
    """int32 [n', 4] CPU coordinates: "uniform" = s_uniform(n, grid=64, seed=5) (x div for the encoder variant),
    "lidar" = lidar_like(n, seed=3) (coordinates to 2 000: |theta| in the thousands of radians)."""
    if kind == "uniform":
        coords = s_uniform(n, grid=64, seed=5)
        if div != 1.0:
            coords[:, :3] *= int(div)
        return coords
    assert kind == "lidar", kind
    coords = torch.from_numpy(lidar_like(n, seed=3))
    if div != 1.0:
        coords[:, :3] *= int(div)
    return coords


def make_rows(n, C, dtype=torch.float32):
    """(feats, gout) of the training tests (seeds 7 and 8); feats rounded into `dtype` (a 16-bit row type) where asked."""
    feats = torch.randn(n, C, generator=torch.Generator().manual_seed(7)).to(dtype)
    gout = torch.randn(n, C, generator=torch.Generator().manual_seed(8))
    return feats, gout


# ---------------------------------------------------------------------------------------------------------------- reference
def reference_grads(feats, coords, p, s, r, baseop, groups, div, gout, dtype=torch.float64):
    """{"out", "feats", "w_pre", "pre_ln_w", "pre_ln_b", "w_pos", "alpha"?, "ln_w", "ln_b"}: the oracle's R_core and the
    gradients of sum(out * gout), by autograd in `dtype` on the CPU.  Every input is a detached clone made a leaf in `dtype`
    (16-bit rows are widened: the reference is evaluated on the rows the kernels read)."""
    from oracle import link_oracle as lo
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)      # noqa: E731
    f = leaf(feats)
    q = {k: leaf(p[k]) for k in PARAMS if p.get(k) is not None}
    params = {_STATE_KEYS[k]: v for k, v in q.items()}
    variant = "encoder" if div != 1.0 else "unet"
    out = lo.elk_core_torch(f, coords.detach().cpu(), params, s, r, baseop, groups, variant=variant, tensor_stride=int(div),
                            agg=lo.aggregate_torch)
    out.backward(gout.detach().cpu().to(dtype))
    res = {"out": out.detach(), "feats": f.grad}
    res.update({k: v.grad for k, v in q.items()})
    return res


def yardstick(feats, coords, p, s, r, baseop, groups, div, gout, seed=0):
    """(g64, o32).  o32[k] = max over two fp32 evaluations of rel_err(g32[k], g64[k]): rows as given, and rows in a seeded
    permutation (results un-permuted before they are compared)."""
    args = (p, s, r, baseop, groups, div)
    g64 = reference_grads(feats, coords, *args, gout, torch.float64)
    a = reference_grads(feats, coords, *args, gout, torch.float32)
    perm = torch.randperm(feats.shape[0], generator=torch.Generator().manual_seed(1000 + seed))
    b = reference_grads(feats.cpu()[perm], coords.cpu()[perm], *args, gout.cpu()[perm], torch.float32)
    for k in ("out", "feats"):
        un = torch.empty_like(b[k])
        un[perm] = b[k]
        b[k] = un
    o32 = {k: max(rel_err(a[k].numpy(), g64[k].numpy()), rel_err(b[k].numpy(), g64[k].numpy())) for k in g64}
    return g64, o32


_CACHE = {}


def cached_yardstick(key, make):
    """yardstick(*make()) computed once per `key` and shared by every test of the session that names it; callers leave it unchanged."""
    if key not in _CACHE:
        _CACHE[key] = yardstick(*make())
    return _CACHE[key]


def rounding_cost(g64, dtype):
    """o_round of 16-bit rows: what storing the float64 feats gradient in the row type alone costs (the forward's _Rounded
    rule); 0 for every other tensor, which the kernels return in fp32."""
    o = {k: 0.0 for k in g64}
    o["feats"] = rel_err(g64["feats"].to(dtype).double().numpy(), g64["feats"].numpy())
    return o


# --------------------------------------------------------------------------------------------------------------------- gate
def _np64(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def _record(rows):
    d = os.environ.get("LINK_AMD_PARITY_DIR")
    if not d:
        return
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "train_parity.jsonl"), "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def measure(case, g64, o32, got, o_round=None):
    """One row per tensor of g64: {**case, tensor, e, o32, ratio = e / o32, bound, (o_round), ok, why}; appended to
    train_parity.jsonl.  No verdict here: gate() asserts on the rows."""
    rows = []
    for k, ref in g64.items():
        ref = _np64(ref)
        orn = float(o_round[k]) if o_round else 0.0
        bound = FACTOR * o32[k] + 2.0 * orn + FLOOR
        row = dict(case, tensor=k, e=None, o32=o32[k], ratio=None, bound=bound, **({"o_round": orn} if orn else {}))
        why = None
        if k not in got or got[k] is None:
            why = "missing"
        else:
            g = _np64(got[k])
            if g.shape != ref.shape:
                why = f"shape {g.shape} != {ref.shape}"
            elif not np.isfinite(g).all():
                why = "not finite"
            elif not float(np.abs(ref).max()) > 0.0:
                why = "max|g64| == 0: no relative error exists"
            else:
                row["e"] = e = rel_err(g, ref)
                row["ratio"] = e / o32[k] if o32[k] > 0 else None
                if not e <= bound:
                    why = "e > 4 * o32 + 2 * o_round + 2e-6"
        row["ok"], row["why"] = why is None, why
        rows.append(row)
    _record(rows)
    return rows


def gate_zero(case, g64, g32, got, keys):
    """Tensors that are analytically zero (the theta gradients of isolated voxels) have no relative error.  What is left of them
    in fp32 is rounding residue, so the kernels' is held against the residue of the oracle's own fp32 evaluation `g32`:
    max|got[k]| <= 4 * max|g32[k]| + 2e-6 * max|g64["feats"]|.  One row per tensor (e = max|got|, o32 = max|g32|)."""
    rows = []
    scale = float(g64["feats"].abs().max())
    for k in keys:
        m32 = float(g32[k].abs().max())
        bound = FACTOR * m32 + FLOOR * scale
        row = dict(case, tensor=k, zero=True, e=None, o32=m32, ratio=None, bound=bound)
        why = None
        if k not in got or got[k] is None:
            why = "missing"
        else:
            g = _np64(got[k])
            if g.shape != tuple(g64[k].shape):
                why = f"shape {g.shape} != {tuple(g64[k].shape)}"
            elif not np.isfinite(g).all():
                why = "not finite"
            else:
                row["e"] = e = float(np.abs(g).max())
                row["ratio"] = e / m32 if m32 > 0 else None
                if not e <= bound:
                    why = "max|g| > 4 * max|g32| + 2e-6 * max|g64[feats]|"
        row["ok"], row["why"] = why is None, why
        rows.append(row)
    _record(rows)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, "\n".join(json.dumps(r) for r in bad)
    return rows


def gate(case, g64, o32, got, o_round=None):
    """Every tensor of g64: present in `got`, finite, max|g64| > 0 and rel_err(got, g64) <= 4 * o32 + 2 * o_round + 2e-6.
    The rows are written before the verdict, so a failing case still leaves its figures."""
    rows = measure(case, g64, o32, got, o_round)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, "\n".join(json.dumps(r) for r in bad)
    return rows
