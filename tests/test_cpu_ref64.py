"""tests/ref64.py (the chunked float64 R_core reference of tests/test_gpu_sizes.py) against the oracle's float64 evaluation of the
same formula (oracle.link_oracle.elk_core_torch with aggregate_torch, every input and parameter in float64): small frames over the
three base operations, the unet and det variants, groups 1 / 2, r in {2, 3}, chunks smaller than a block and chunks that do not
divide n, negative coordinates and two batch indices.  Gate 1e-12 relative: the two evaluate one formula in one precision."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.ref64 import Ref64  # noqa: E402


def _frame(n, c, seed, neg=False, batches=1):
    rng = np.random.default_rng(seed)
    span = 40
    lin = rng.choice(span ** 3 * batches, n, replace=False)                 # unique voxels
    x, y, z, b = lin % span, (lin // span) % span, (lin // span ** 2) % span, lin // span ** 3
    co = np.stack([x, y, z, b], 1).astype(np.int32)
    if neg:
        co[:, :3] -= np.array([23, 17, 31], np.int32)                      # blocks on both sides of zero (floor, not truncation)
    feats = torch.from_numpy(rng.standard_normal((n, c))).double()
    return feats, torch.from_numpy(co)


def _params(c, baseop, groups, variant, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)    # noqa: E731
    pw = c if (variant == "det" or baseop == "cos_x") else c // groups
    p = {"pre_mix.0.weight": rnd(c, c) / c ** 0.5, "pre_mix.1.weight": 1 + 0.1 * rnd(c), "pre_mix.1.bias": 0.1 * rnd(c),
         "pos_weight.0.weight": rnd(pw, 3), "norm.weight": 1 + 0.1 * rnd(c), "norm.bias": 0.1 * rnd(c)}
    if baseop == "cos_x":
        p["alpha"] = 1 + 0.2 * rnd(1, c)
    return p


CASES = [  # baseop, variant, groups, r, s, n, chunk, neg, batches
    ("cos", "unet", 2, 3, 5, 3000, 1 << 20, False, 1),
    ("cos", "unet", 1, 2, 4, 2500, 997, True, 2),
    ("sin", "unet", 2, 2, 5, 4000, 3, False, 2),               # chunks far smaller than a block
    ("sin", "unet", 1, 3, 3, 1800, 1000, True, 1),
    ("cos_x", "unet", 1, 3, 4, 3500, 1234, True, 2),
    ("cos_x", "unet", 1, 2, 6, 2000, 2000, False, 1),
    ("cos", "det", 1, 3, 5, 2200, 777, True, 2),
    ("sin", "det", 1, 2, 4, 5000, 4999, False, 1),             # one full chunk + a chunk of one row
]


@pytest.mark.parametrize("baseop,variant,groups,r,s,n,chunk,neg,batches", CASES)
def test_ref64_equals_the_oracle_in_float64(baseop, variant, groups, r, s, n, chunk, neg, batches):
    from oracle import link_oracle as O
    C = 16
    feats, coords = _frame(n, C, seed=n + r, neg=neg, batches=batches)
    params = _params(C, baseop, groups, variant, seed=7 * n)
    want = O.elk_core_torch(feats, coords, params, s, r, baseop, groups, variant=variant)
    ref = Ref64(feats, coords, params, s, r, baseop, groups, variant=variant, chunk=chunk)
    got = torch.cat([ref.rows(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)])
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12
    d, m, finite = ref.compare(want)
    assert finite and d / m <= 1e-12
    # the fp32 evaluation of the same formula is close to, but measurably not, the float64 one -- what `o32` measures
    r32 = Ref64(feats.float(), coords, params, s, r, baseop, groups, variant=variant, dtype=torch.float32, chunk=chunk)
    o32, ok = ref.rel(r32)
    assert ok and 1e-10 < o32 < 1e-4


def test_ref64_sees_a_wrong_or_missing_row():
    """compare() is a gate: one perturbed value, or one NaN row (a row the kernel never wrote), fails it."""
    from oracle import link_oracle as O
    C = 16
    feats, coords = _frame(1500, C, seed=3, neg=True, batches=2)
    params = _params(C, "cos", 2, "unet", seed=4)
    want = O.elk_core_torch(feats, coords, params, 5, 3, "cos", 2).float()
    ref = Ref64(feats, coords, params, 5, 3, "cos", 2, chunk=256)
    rel, ok = ref.rel(want)
    assert ok and rel < 1e-6
    bad = want.clone()
    bad[1234, 5] += 1e-3 * float(want.abs().max())
    assert ref.rel(bad)[0] > 5e-4
    bad = want.clone()
    bad[1499] = float("nan")
    rel, ok = ref.rel(bad)
    assert not ok and rel == float("inf")


def test_ref64_coord_div_and_alpha_override():
    """coord_div divides xyz before theta (the kernels' LinkElkDesc.coord_div; encoder cos_x); `alpha` overrides params['alpha']."""
    from oracle import link_oracle as O
    C = 16
    feats, coords = _frame(1200, C, seed=11)
    params = _params(C, "cos_x", 1, "unet", seed=12)
    want = O.elk_core_torch(feats, coords, params, 4, 3, "cos_x", 1, variant="encoder", tensor_stride=2)
    a = params.pop("alpha")
    ref = Ref64(feats, coords, params, 4, 3, "cos_x", 1, variant="unet", alpha=a, coord_div=2.0, chunk=500)
    d, m, ok = ref.compare(want)
    assert ok and d / m <= 1e-12
