"""The prologue of a chunk of the cell-range pre_mix kernel (csrc/dense_k1_impl.h, dc_k1_range): (A) the id-ordered records are not
written back to the slot lists where the quad-consumer gather kernel reads them -- the batch K1 role, and the inference forward of
a plan -- and (B, a build switch: -DDC_K1_LATE_PUBLISH=1) the chunk's publishing stores are issued behind the row requests of its
first two tiles; with or without B the first two tiles are requested in front of the tile loop.  None of it enters any sum: rows must
stay bit for bit those of the form that writes the records back (link_dc_tuning_t::k1_form bit 4), in either build.

Frames are the smallest that reach every branch of the prologue (s = 7: a grid of D blocks is 7 D voxels wide), all with negative
coordinates and shuffled voxel ids:
  cells   3 x 3 x 3 blocks, 55 voxels: cells of 0, 1, 2, 3 and 4 voxels in turn -- empty cells (zero rows), every inline count
  deep    3 x 3 x 3 blocks, ~1 500 voxels: every cell holds more than DC_INL = 4 records (overflow lists, several tiles and, with 27
          cells of ~55 voxels against an LDS list of 352, several chunks per range)
  strips  5 x 3 x 3 blocks, ~90 voxels: an axis of 4 m + 1 blocks, so the gather role runs rim strips (r = 3)
r in {2, 3}, cos and sin, fp32 and fp16 rows.  For each case:
  1. rows of ElkCoreBatch (three frames, the first repeated) == rows of ElkCorePlan with the write-back forced on, and == the plan's
     default (which leaves it out), bit for bit;
  2. the same batch call twice gives identical rows;
  3. a warm plan call (build_index=False) after a cold one without the write-back equals the cold rows -- also after every cell's
     records have been REVERSED in the slot lists (the rank order of the insert's atomics follows the voxel ids in frames this small;
     reversed lists cannot be in id order): the pre_mix kernel orders the records itself, the quad consumers take them in any order;
  4. rows pass the float64 gate of tests/ref64.py as tests/test_gpu_sizes.py applies it (finite; rel64 < 1e-4 fp32 / 4e-3 fp16;
     rel64 <= 4 o32 + 2 o_round + 2e-6);
  5. check() (the status words, link_dc_batch_status) is clean.
"""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.ref64 import Ref64, gate_rows  # noqa: E402

pytestmark = pytest.mark.gpu

C, GROUPS, S = 64, 2, 7
WRITEBACK = 16                                # k1_form bit 4: the id-ordered records go back to the slot lists
DC_INL = 4                                    # inline records of a cell (csrc/dense_common.h)
KINDS = ["cells", "deep", "strips"]


@functools.lru_cache(maxsize=None)
def _block(baseop):
    import link_amd as la
    torch.manual_seed(11)
    return la.ELKBlock(C, C, groups=GROUPS, baseop=baseop).cuda().eval()


def _bind(obj, blk):
    obj.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, None, blk.norm.weight,
             blk.norm.bias)
    return obj


def _geometry(kind):
    dims = (5, 3, 3) if kind == "strips" else (3, 3, 3)
    shift = -14                               # blocks -2 .. : floor division below zero
    bounds = ((shift, shift, shift, 0), tuple(S * d - 1 + shift for d in dims) + (0,))
    return dims, shift, bounds


@functools.lru_cache(maxsize=None)
def _coords(kind, seed):
    """Unique voxels of one frame (CPU int32 [n, 4]), voxel ids shuffled."""
    dims, shift, _ = _geometry(kind)
    g = torch.Generator().manual_seed(seed)
    cells = [(bx, by, bz) for bx in range(dims[0]) for by in range(dims[1]) for bz in range(dims[2])]
    if kind == "cells":
        per = [i % 5 for i in range(len(cells))]                      # 0, 1, 2, 3, 4, 0, ...: 55 voxels
        per = [per[i] for i in torch.randperm(len(cells), generator=g).tolist()]
    elif kind == "deep":
        per = torch.randint(40, 72, (len(cells),), generator=g).tolist()   # ~1 500 voxels, every cell past DC_INL
    else:
        per = torch.randint(0, 5, (len(cells),), generator=g).tolist()     # ~90 voxels
    rows = []
    for (bx, by, bz), k in zip(cells, per):
        lin = torch.randperm(S ** 3, generator=g)[:k]
        rows.append(torch.stack([S * bx + lin % S, S * by + (lin // S) % S, S * bz + lin // (S * S), torch.zeros_like(lin)], 1))
    co = torch.cat(rows)
    co[:, :3] += shift
    return co[torch.randperm(co.shape[0], generator=g)].int().contiguous()


@functools.lru_cache(maxsize=None)
def _frame(kind, seed, dt):
    co = _coords(kind, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(co.shape[0], C, generator=g).to(dt).cuda(), co.cuda()


@functools.lru_cache(maxsize=None)
def _ref(kind, seed, dt, baseop, r):
    """(float64 reference, o32) of the frame: computed once per frame and parameter set, shared and left unchanged."""
    f, co = _frame(kind, seed, dt)
    blk = _block(baseop)
    params = {k: v.detach() for k, v in blk.state_dict().items()}
    kw = dict(baseop=baseop, groups=GROUPS)
    ref = Ref64(f, co, params, S, r, **kw)
    o32, ok = ref.rel(Ref64(f, co, params, S, r, dtype=torch.float32, **kw))
    assert ok
    return ref, o32


def _reverse_cell_lists(plan):
    """Reverse every cell's records in the plan's slot lists (inline region: DC_INL records per cell; overflow region behind it:
    k - DC_INL per cell -- csrc/dense_common.h, dc_slot)."""
    k, vp = int(plan.dcg.k), int(plan.dcg.vp)
    cell_n = plan.cell_n.cpu().clamp(max=k)
    slots = plan.slots.cpu()
    new = slots.clone()
    at = lambda pc, rank: pc * DC_INL + rank if rank < DC_INL else vp * DC_INL + pc * (k - DC_INL) + rank - DC_INL
    for pc in torch.nonzero(cell_n > 1).flatten().tolist():
        nv = int(cell_n[pc])
        for rank in range(nv):
            new[at(pc, rank)] = slots[at(pc, nv - 1 - rank)]
    plan.slots.copy_(new.to(plan.slots.device))
    return int((cell_n > 1).sum()), int((cell_n > DC_INL).sum())


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("baseop", ["cos", "sin"])
@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_without_the_record_write_back(kind, r, baseop, dt):
    import link_amd as la
    blk = _block(baseop)
    _, _, bounds = _geometry(kind)
    seeds = (1, 2, 1)                                                  # three frames, the first repeated
    frames = [_frame(kind, sd, dt) for sd in seeds]
    n_cap = max(f.shape[0] for f, _ in frames)
    dev = torch.device("cuda")

    # the per-frame plan: write-back forced on (the form the others are held against), then its default; cold and warm
    plan = _bind(la.ElkCorePlan(n_cap, C, baseop, C // GROUPS, r, S, bounds, dev, layout="dense", k1_form=WRITEBACK), blk)
    assert plan.dense
    forced = [plan.run(f, co).clone() for f, co in frames]
    plan.check()
    plan.set_tuning(k1_form=0)
    for i, (f, co) in enumerate(frames):
        cold = plan.run(f, co).clone()
        plan.check()
        assert torch.equal(cold, forced[i]), (kind, i, "plan default != write-back forced on")
        warm = plan.run(f, co, build_index=False).clone()
        plan.check()
        assert torch.equal(warm, cold), (kind, i, "warm != cold")                                       # 3.
        many, deep = _reverse_cell_lists(plan)
        if i == 0:                                                     # the frames are what the docstring says they are
            assert many > 0 and (deep > 0) == (kind == "deep"), (kind, many, deep)
        again = plan.run(f, co, build_index=False).clone()
        plan.check()
        assert torch.equal(again, cold), (kind, i, "warm on reversed cell lists != cold")               # 3.
        plan.set_tuning(k1_form=WRITEBACK)                             # ... and the form with the write-back, warm on those lists
        again = plan.run(f, co, build_index=False).clone()
        plan.check()
        assert torch.equal(again, cold), (kind, i, "warm (write-back form) on reversed cell lists != cold")
        plan.set_tuning(k1_form=0)

    batch = _bind(la.ElkCoreBatch(3, n_cap, C, baseop, C // GROUPS, r, S, bounds, dev), blk)
    feats, coords = [f for f, _ in frames], [co for _, co in frames]
    first = [o.clone() for o in batch.run(feats, coords)]
    batch.check()                                                                                       # 5.
    second = [o.clone() for o in batch.run(feats, coords)]
    batch.check()
    for i in range(3):
        assert first[i].dtype == dt
        assert torch.equal(first[i], forced[i]), (kind, i, "batch != plan with the write-back forced on")   # 1.
        assert torch.equal(second[i], first[i]), (kind, i, "second batch call != first")                # 2.
    assert torch.equal(first[0], first[2])                             # the repeated frame
    for i, sd in enumerate(seeds[:2]):
        ref, o32 = _ref(kind, sd, dt, baseop, r)
        gate_rows((kind, r, baseop, str(dt), i), ref, o32, first[i], dt)                                   # 4.
