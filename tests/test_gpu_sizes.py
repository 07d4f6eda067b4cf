"""R_core at the frame sizes the ABI accepts and the rest of the suite never reaches (collated batches, dense frames): past 2^19
voxels (the batch insert's items), past 2^20 (the second pass of the index kernels' capped grid-stride loops) and past 2^31 bytes of
rows (8.6 M voxels at C = 64, 4.3 M at C = 128: the unsigned 32-bit byte offsets the guards promise).  Every case is gated against
the chunked float64 reference of tests/ref64.py (pinned to the oracle by tests/test_cpu_ref64.py):
  (a) every row finite -- every result buffer starts as NaN, so a row that was never written cannot pass;
  (b) rel64 = max|out - ref64| / max|ref64| < 1e-4 (north_star's gate, taken against the float64 truth);
  (c) rel64 <= 4 * o32 + 2e-6, o32 = what evaluating the same formula in fp32 costs: an error that passes 1e-4 but sits far above
      fp32 evaluation still fails;
  (d) the status words are clean (check()).
Each case's rel64 / o32 is appended to size_parity.jsonl in the directory LINK_AMD_PARITY_DIR names (no file when it is unset).
A form whose guard refuses a size is asserted to refuse it."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.helpers import s_uniform  # noqa: E402
from tests.ref64 import Ref64, gate_rows  # noqa: E402

pytestmark = pytest.mark.gpu
BOUNDS = ((0, 0, 0, 0), (255, 255, 255, 0))
TOL = 1e-4
NAN = float("nan")
BIG = 8_600_000                       # 8.6 M x 64 x 4 bytes of rows > 2^31
MID = 1_100_000                       # past 2^20: a second pass of every capped grid-stride loop


def _block(c, baseop, groups=2):
    import link_amd as la
    torch.manual_seed(2)
    blk = la.ELKBlock(c, c, groups=groups, baseop=baseop).cuda().eval()
    if baseop == "cos_x":
        with torch.no_grad():
            blk.alpha.uniform_(0.5, 1.5)
    return blk


def _bind(obj, blk):
    alpha = blk.alpha if blk.baseop == "cos_x" else None
    obj.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, alpha, blk.norm.weight,
             blk.norm.bias)
    return obj


def _frame(n, c, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    return torch.randn(n, c, generator=g, device="cuda").to(dtype), s_uniform(n, seed=seed).cuda()


def _refs(feats, coords, blk, s, r):
    """(float64 reference, o32) of one frame under `blk`'s parameters."""
    params = {k: v.detach() for k, v in blk.state_dict().items()}
    kw = dict(baseop=blk.baseop, groups=blk.groups)
    ref = Ref64(feats, coords, params, s, r, **kw)
    o32, ok = ref.rel(Ref64(feats, coords, params, s, r, dtype=torch.float32, **kw))
    assert ok
    return ref, o32


def _record(row):
    """Append one case's row to $LINK_AMD_PARITY_DIR/size_parity.jsonl (written before the case's verdicts: a failing case still
    leaves its numbers)."""
    d = os.environ.get("LINK_AMD_PARITY_DIR")
    if not d:
        return
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "size_parity.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _gate(case, ref, o32, out, dt=torch.float32):
    """(a) - (c) of the module docstring for one frame's rows (tests/ref64.py, gate_rows); the row goes to size_parity.jsonl
    before the verdicts."""
    gate_rows(dict(case, peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)), ref, o32, out, dt, record=_record)


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# the batch entry point (include/link_amd.h section H)
# ------------------------------------------------------------------------------------------------------------------------------
def _batch_case(sizes, baseop, r, s, dt=torch.float32, seed0=0, twice=False):
    """One ElkCoreBatch call over frames of `sizes` voxels: NaN-prefilled result tensors; every frame bit-equal to the per-frame
    plan (ElkCorePlan dense, k1_form 0: the body the batch's K1 role runs) on the same rows, and gated against float64."""
    import link_amd as la
    C = 64
    blk = _block(C, baseop)
    nmax = max(sizes)
    frames = [_frame(n, C, seed0 + i, dt) for i, n in enumerate(sizes)]
    batch = _bind(la.ElkCoreBatch(len(sizes), nmax, C, baseop, C // 2, r, s, BOUNDS, "cuda"), blk)
    calls = []
    for _ in range(2 if twice else 1):
        outs = [torch.full((n, C), NAN, dtype=dt, device="cuda") for n in sizes]
        got = batch.run([f for f, _ in frames], [co for _, co in frames], outs=outs)
        torch.cuda.synchronize()
        batch.check()
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
        calls.append(outs)
    del batch
    _free()
    plan = _bind(la.ElkCorePlan(nmax, C, baseop, C // 2, r, s, BOUNDS, "cuda", layout="dense", k1_form=0), blk)
    differ = []                                          # per frame and call: rows that are not bit-equal to the per-frame plan's
    for i, (f, co) in enumerate(frames):
        want = torch.full((f.shape[0], C), NAN, dtype=dt, device="cuda")
        plan.run(f, co, out=want)
        plan.check()
        assert bool(torch.isfinite(want).all())
        differ.append([int((outs[i] != want).any(1).sum()) for outs in calls])
        del want
    del plan
    _free()
    # the float64 gates first (each frame's row in size_parity.jsonl carries its bitwise verdict too), the bitwise verdict after
    for i, (f, co) in enumerate(frames):
        ref, o32 = _refs(f, co, blk, s, r)
        _gate({"path": "batch", "dtype": str(dt)[6:], "op": baseop, "r": r, "s": s, "frame": i, "rows_differing_from_plan": differ[i]},
              ref, o32, calls[0][i], dt)
        del ref
    assert all(d == [0] * len(calls) for d in differ), ("rows differ from the per-frame plan", sizes, differ)
    del calls, frames
    _free()


def test_batch_frames_around_the_insert_item_limit():
    """524 288 voxels = 2048 insert items of 256; one more voxel, 600 000, and a small frame, in ONE call (the items per frame follow
    the largest frame); a second call on the same arenas gives the same rows."""
    _batch_case([524_288, 524_289, 600_000, 20_000], "cos", 3, 7, twice=True)


def test_batch_sin_r2_s5_past_the_insert_item_limit():
    _batch_case([600_000, 3_000], "sin", 2, 5, seed0=10)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_batch_half_rows_past_the_insert_item_limit(dt):
    _batch_case([600_000, 1_000], "cos", 3, 7, dt=dt, seed0=20)


def test_batch_rows_past_2_31_bytes():
    """8.6 M voxels (8.6 M x 64 x 4 bytes of rows > 2^31: every byte offset on the path must be unsigned 32-bit or wider) + 1."""
    _batch_case([BIG, 1], "cos", 3, 7, seed0=30)


def test_batch_chunk_tails():
    """Frames of 1, 63, 64, 65, 255, 256, 257 voxels in one call: the tails of the insert's 64-lane passes and 256-voxel items."""
    _batch_case([1, 63, 64, 65, 255, 256, 257], "cos", 3, 7, seed0=40)


def test_batch_refuses_frames_of_2_24_voxels():
    """Section H's per-frame limit: 1 <= n < 2^24.  The plan a batch arena is made of refuses n_cap = 2^24 at C = 64 (rows of 2^32
    bytes) before allocating; the C entry point refuses a frame count of 2^24 or of 0 and launches nothing."""
    import ctypes
    import link_amd as la
    from link_amd import _lib as L
    with pytest.raises(L.LinkAmdError):
        la.ElkCoreBatch(1, 1 << 24, 64, "cos", 32, 3, 7, BOUNDS, "cuda")
    blk = _block(64, "cos")
    batch = _bind(la.ElkCoreBatch(2, 256, 64, "cos", 32, 3, 7, BOUNDS, "cuda"), blk)
    frames = [_frame(256, 64, 50 + i) for i in range(2)]
    k, _ = batch._fill([f for f, _ in frames], [co for _, co in frames], None)
    p0 = batch.plans[0]
    for bad in (1 << 24, 0):
        batch._n[1] = bad
        rc = batch._fn(batch._ctx, batch._bufs, batch._n, k, ctypes.byref(p0.dcg), ctypes.byref(p0.desc), L.current_stream_handle())
        assert rc == L.LINK_ERR_ARG, bad
    torch.cuda.synchronize()
    batch.check()
    outs = batch.run([f for f, _ in frames], [co for _, co in frames])             # the context still serves a valid call
    batch.check()
    assert all(bool(torch.isfinite(o).all()) for o in outs)


# ------------------------------------------------------------------------------------------------------------------------------
# ElkCorePlan: dense-cell, general (tile and four-kernel forms), lean
# ------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached_frame(n, c, baseop, r, s, groups, seed):
    """One frame, its block and its float64 reference, kept for the next test of the same frame (one at a time: they are large)."""
    key = (n, c, baseop, r, s, groups, seed)
    if key not in _CACHE:
        _CACHE.clear()
        _free()
        blk = _block(c, baseop, groups)
        f, co = _frame(n, c, seed)
        ref, o32 = _refs(f, co, blk, s, r)
        _CACHE[key] = (f, co, blk, ref, o32)
    return _CACHE[key]


def _dense_run(plan, f, co, case, ref, o32):
    """Cold (index built) and warm (index reused) steps into NaN: bit-equal, counters clean, status clean, gated."""
    plan.out.fill_(NAN)
    cold = plan.run(f, co).clone()
    plan.check()
    assert int(plan.cnt.sum()) == 0, "cell counters not cleaned by the step"
    plan.out.fill_(NAN)
    warm = plan.run(f, co, build_index=False)
    plan.check()
    assert int(plan.cnt.sum()) == 0
    assert torch.equal(cold, warm), int((cold != warm).any(1).sum())
    assert plan.blocks() == ref.M
    del cold
    _gate(case, ref, o32, warm)


@pytest.mark.parametrize("tuning", [{}, {"k1_form": 0}, {"k1_form": 2}], ids=["default", "k1_form0", "k1_form2"])
@pytest.mark.parametrize("n", [MID, BIG])
def test_dense_plan_large_frames(n, tuning):
    import link_amd as la
    f, co, blk, ref, o32 = _cached_frame(n, 64, "cos", 3, 7, 2, seed=60)
    plan = _bind(la.ElkCorePlan(n, 64, "cos", 32, 3, 7, BOUNDS, "cuda", layout="dense", **tuning), blk)
    _dense_run(plan, f, co, {"path": "dense", "op": "cos", "tuning": str(tuning)}, ref, o32)
    del plan
    _free()


def _general_forms(n, c, baseop, cg):
    """Which general-layout form a plan of n_cap = n runs, from the guards the library states: the tile form while its table stays
    below 2^32 bytes, else the four-kernel form while its block table does ((m_cap + 1) x (3C + 1) x 4 < 2^32), else refused."""
    import ctypes
    from link_amd import _lib as L
    from link_amd.elk import _OPS
    desc = L.LinkElkDesc(_OPS[baseop], c, cg, 3, 1.0, 1e-6)
    tb = int(L.lib().link_elk_tiles_table_bytes(ctypes.byref(desc), n, n))
    tiles_ok = 0 < tb < 2 ** 32 and n * c * 4 < 2 ** 32
    four_ok = (n + 1) * (3 * c + 1) * 4 < 2 ** 32 and n * c * 4 < 2 ** 32
    return tiles_ok, four_ok


@pytest.mark.parametrize("tiles", [True, False], ids=["tiles", "four_kernel"])
@pytest.mark.parametrize("n", [MID, BIG])
def test_general_plan_large_frames(n, tiles):
    """The general layout (index by count / scan / place, then the tile form or the four-kernel form); blocks() == the number of
    distinct blocks (= what the dense plan reports, test above).  Where the form's 32-bit guards refuse the size, the step raises."""
    import link_amd as la
    from link_amd import _lib as L
    f, co, blk, ref, o32 = _cached_frame(n, 64, "cos", 3, 7, 2, seed=60)
    tiles_ok, four_ok = _general_forms(n, 64, "cos", 32)
    plan = _bind(la.ElkCorePlan(n, 64, "cos", 32, 3, 7, BOUNDS, "cuda", layout="general", tiles=tiles), blk)
    assert plan.tiles == (tiles and tiles_ok)
    plan.out.fill_(NAN)
    if not (plan.tiles or four_ok):
        with pytest.raises(L.LinkAmdError):
            plan.run(f, co)
        assert n == BIG                                                      # 1.1 M fits both forms
    else:
        out = plan.run(f, co)
        plan.check()
        assert plan.blocks() == ref.M
        _gate({"path": "general_tiles" if plan.tiles else "general_four", "op": "cos"}, ref, o32, out)
    del plan
    _free()


def _lean_max_n(c, baseop, r, s):
    """The largest n_cap ElkCorePlan.lean_supported admits on BOUNDS (its table bytes grow with n_cap)."""
    from link_amd.elk import ElkCorePlan
    lo, hi = 1, 1 << 24
    assert ElkCorePlan.lean_supported(lo, c, baseop, r, s, BOUNDS) and not ElkCorePlan.lean_supported(hi, c, baseop, r, s, BOUNDS)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ElkCorePlan.lean_supported(mid, c, baseop, r, s, BOUNDS) else (lo, mid)
    return lo


@pytest.mark.parametrize("which", ["mid", "max"])
def test_lean_plan_large_frames(which):
    import link_amd as la
    from link_amd import _lib as L
    n = MID if which == "mid" else _lean_max_n(64, "cos", 3, 7)
    assert n >= MID
    f, co, blk, ref, o32 = _cached_frame(n, 64, "cos", 3, 7, 2, seed=70)
    plan = _bind(la.ElkCorePlan(n, 64, "cos", 32, 3, 7, BOUNDS, "cuda", layout="lean"), blk)
    assert plan.lean
    plan.out.fill_(NAN)
    out = plan.run(f, co)
    plan.check()
    _gate({"path": "lean", "op": "cos"}, ref, o32, out)
    del plan, out
    _free()
    if which == "max":                                                       # one voxel more: refused by the plan, nothing allocated
        with pytest.raises(L.LinkAmdError):
            la.ElkCorePlan(n + 1, 64, "cos", 32, 3, 7, BOUNDS, "cuda", layout="lean")


@pytest.mark.parametrize("layout", ["dense", "general"])
def test_cos_x_c128_rows_past_2_31_bytes(layout):
    """cos_x, C = 128, groups 1 (three-part rows of 384 floats), 4.3 M voxels: 4.3 M x 128 x 4 bytes of rows > 2^31."""
    import link_amd as la
    from link_amd import _lib as L
    n, c = 4_300_000, 128
    f, co, blk, ref, o32 = _cached_frame(n, c, "cos_x", 3, 7, 1, seed=80)
    if layout == "dense":
        plan = _bind(la.ElkCorePlan(n, c, "cos_x", c, 3, 7, BOUNDS, "cuda", layout="dense"), blk)
        _dense_run(plan, f, co, {"path": "dense", "op": "cos_x", "C": c}, ref, o32)
    else:
        tiles_ok, four_ok = _general_forms(n, c, "cos_x", c)
        plan = _bind(la.ElkCorePlan(n, c, "cos_x", c, 3, 7, BOUNDS, "cuda", layout="general"), blk)
        assert plan.tiles == tiles_ok
        plan.out.fill_(NAN)
        if not (tiles_ok or four_ok):
            with pytest.raises(L.LinkAmdError):
                plan.run(f, co)
        else:
            out = plan.run(f, co)
            plan.check()
            _gate({"path": "general", "op": "cos_x", "C": c}, ref, o32, out)
    del plan
    _CACHE.clear()
    _free()


# ------------------------------------------------------------------------------------------------------------------------------
# the drop-in surface: voxel_to_aux -> aux_to_voxel (link_amd/aggregate.py)
# ------------------------------------------------------------------------------------------------------------------------------
def _aggregate_ref(x, coords, s, r, dtype):
    """utils.py:44-84 restated with torch.unique + index_add in `dtype`: (out [n, W], small_C, idx_query, counts)."""
    c = coords.long()
    bc = torch.cat([torch.div(c[:, :3], s, rounding_mode="floor"), c[:, 3:]], 1)
    small, inv, cnt = torch.unique(bc, dim=0, return_inverse=True, return_counts=True)
    m = small.shape[0]
    S = torch.zeros(m, x.shape[1], dtype=dtype, device=x.device).index_add_(0, inv, x.to(dtype))
    # neighbour b of every block through the sorted packed keys
    lo = small.min(0).values - r
    sp = small.max(0).values + r - lo + 1
    key = lambda b: (((b[:, 0] - lo[0]) * sp[1] + b[:, 1] - lo[1]) * sp[2] + b[:, 2] - lo[2]) * sp[3] + b[:, 3] - lo[3]  # noqa: E731
    keys = key(small)
    BS, BC = torch.zeros_like(S), torch.zeros(m, dtype=dtype, device=x.device)
    ax = torch.arange(-r // 2 + 1, r // 2 + 1, device=x.device)
    for o in torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3):
        nb = small.clone()
        nb[:, :3] += o
        k = key(nb)
        pos = torch.searchsorted(keys, k).clamp(max=m - 1)
        hit = keys[pos] == k
        BS.index_add_(0, torch.nonzero(hit).view(-1), S[pos[hit]])
        BC.index_add_(0, torch.nonzero(hit).view(-1), cnt[pos[hit]].to(dtype))
    return (BS / BC[:, None])[inv], small, inv, cnt


@pytest.mark.parametrize("r", [2, 3])
def test_voxel_to_aux_aux_to_voxel_large_frame(r):
    import link_amd as la
    n, C, s = MID, 64, 7
    x, co = _frame(n, C, seed=90 + r)
    want, small_c, inv, cnt = _aggregate_ref(x, co, s, r, torch.float64)
    w32 = _aggregate_ref(x, co, s, r, torch.float32)[0]
    scale = float(want.abs().max())
    o32 = float((w32.double() - want).abs().max()) / scale
    del w32
    large = la.SparseTensor(x.clone(), co, 1)
    small, idx, counts = la.voxel_to_aux(large, s)
    assert torch.equal(small.C.long(), small_c), "block coordinates (torch.unique order)"
    assert torch.equal(idx.long(), inv), "idx_query"
    assert torch.equal(counts.long(), cnt), "counts"
    out = la.aux_to_voxel(small, large, idx, counts, r).F
    finite = bool(torch.isfinite(out).all())
    rel64 = float((out.double() - want).abs().max()) / scale if finite else float("inf")
    row = {"path": "voxel_to_aux+aux_to_voxel", "r": r, "s": s, "n": n, "rel64": rel64, "o32": o32}
    _record(row)
    assert finite and rel64 < TOL and rel64 <= 4.0 * o32 + 2e-6, row
    del want, out, large, small
    _free()
