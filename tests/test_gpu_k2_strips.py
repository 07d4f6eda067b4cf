"""Rim strips of the quad-consumer box-sum + de-modulate kernel (csrc/dense_gather_quad_impl.h): where an axis of the block grid is
4 m + 1 cells long, its last cell is covered by 1 x 10 / 10 x 1 strips of output columns instead of 4 x 4 tiles.  A cell's sums are
formed in the same order in every tile shape, so the rows must equal those of the square tiling (link_dc_tuning_t::k2_form bit 4)
BIT FOR BIT, under every z-split, and sit on the oracle within the gate of the other dense tests (1e-4 relative, fp32).

Grids are the smallest that reach each path (s = 7: a grid of D blocks is 7 D voxels wide), ~2 voxels per block cell:
  5 x 5 x 5    one full tile, one x-strip of 5 cells, one y-strip of 4
  13 x 5 x 3   two y-strips, the second a 2-cell remainder
  5 x 13 x 3   the same along x
  21 x 21 x 2  strips of 10, 10 and a 1-cell remainder; fewer z-planes than z-segments
  8 x 8 x 4    remainder 0: no strips, the launch of the square tiling
  6 x 7 x 4    remainders 2 and 3: square rim tiles by rule
"""
import functools

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

C, GROUPS, BASEOP, R, S = 64, 2, "cos", 3, 7
SQUARE = 16                                   # k2_form bit 4: square rim tiles (0: strips -- ElkCoreBatch's setting; a plan's default is 16)
GRIDS = [(5, 5, 5), (13, 5, 3), (5, 13, 3), (21, 21, 2), (8, 8, 4), (6, 7, 4)]


def _tiles(dims, strips):
    """Tiles per batch item: the enumeration the launchers and the kernel share, restated (what the grids below are chosen by)."""
    dx, dy = dims[0], dims[1]
    sx, sy = strips and dx % 4 == 1, strips and dy % 4 == 1
    dxs, dys = dx - sx, dy - sy
    return -(-dxs // 4) * -(-dys // 4) + (-(-dy // 10) if sx else 0) + (-(-dxs // 10) if sy else 0)


def test_tile_counts_of_the_cases():
    assert [_tiles(d, True) for d in GRIDS] == [3, 6, 6, 30, 4, 4]
    assert [_tiles(d, False) for d in GRIDS] == [4, 8, 8, 36, 4, 4]
    assert _tiles((37, 37, 37), True) == 89 and _tiles((37, 37, 37), False) == 100


@functools.lru_cache(maxsize=None)
def _block():
    import link_amd as la
    torch.manual_seed(5)
    return la.ELKBlock(C, C, groups=GROUPS, baseop=BASEOP).cuda().eval()


def _frame(dims, seed, shift=0, batches=1):
    """Unique voxels uniform in the box of `dims` blocks (~2 per block cell and batch item), moved by `shift` voxels on every axis."""
    ext = [7 * d for d in dims]
    vol = ext[0] * ext[1] * ext[2]
    n = 2 * dims[0] * dims[1] * dims[2]
    g = torch.Generator().manual_seed(seed)
    parts = []
    for b in range(batches):
        lin = torch.randperm(vol, generator=g)[:n]
        x, y, z = lin % ext[0], (lin // ext[0]) % ext[1], lin // (ext[0] * ext[1])
        parts.append(torch.stack([x + shift, y + shift, z + shift, torch.full_like(x, b)], 1))
    coords = torch.cat(parts)
    coords = coords[torch.randperm(coords.shape[0], generator=g)].int().contiguous()
    feats = torch.randn(coords.shape[0], C, generator=g)
    bounds = ((shift, shift, shift, 0), (ext[0] - 1 + shift, ext[1] - 1 + shift, ext[2] - 1 + shift, batches - 1))
    return feats.cuda(), coords.cuda(), bounds


def _bind(obj):
    blk = _block()
    obj.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, None, blk.norm.weight,
             blk.norm.bias)
    return obj


def _plan(n, bounds, **tuning):
    import link_amd as la
    plan = _bind(la.ElkCorePlan(n, C, BASEOP, C // GROUPS, R, S, bounds, torch.device("cuda"), layout="dense", **tuning))
    assert plan.dense
    return plan


def _oracle(feats, coords):
    from oracle import link_oracle as O
    params = {k: v.detach().cpu() for k, v in _block().state_dict().items()}
    return O.elk_core_torch(feats.cpu(), coords.cpu(), params, S, R, BASEOP, GROUPS, agg=O.aggregate_c).numpy()


def _strips_against_square(dims, feats, coords, bounds):
    plan = _plan(feats.shape[0], bounds)
    ref = _oracle(feats, coords)
    for zsplit in (1, 2, 3):
        plan.set_tuning(k2_zsplit=zsplit, k2_form=SQUARE)
        square = plan.run(feats, coords).clone()
        plan.check()
        plan.set_tuning(k2_zsplit=zsplit, k2_form=0)
        strips = plan.run(feats, coords).clone()
        plan.check()
        assert torch.equal(strips, square), (dims, zsplit, rel_err(strips.cpu().numpy(), square.cpu().numpy()))
        assert rel_err(strips.cpu().numpy(), ref) < 1e-4, (dims, zsplit)


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_strips_equal_square_rim_tiles_and_the_oracle(dims):
    """(a) + (b): rows with strips == rows with square rim tiles, bit for bit, at 1, 2 and 3 z-segments; both within 1e-4 of the
    oracle (remainders 0, 2, 3: the same launch either way)."""
    feats, coords, bounds = _frame(dims, seed=sum(dims))
    _strips_against_square(dims, feats, coords, bounds)


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_strips_negative_coordinates_two_batch_items(dims):
    """(c): blocks that straddle zero (floor division) and two batch indices in one call: the same two conditions."""
    feats, coords, bounds = _frame(dims, seed=100 + sum(dims), shift=-14, batches=2)
    _strips_against_square(dims, feats, coords, bounds)


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_batch_entry_point_equals_the_plans(dims):
    """(d): three frames through ElkCoreBatch (the persistent gather role runs the same tile list) == the per-frame plans, bit for
    bit -- and the per-frame plans with square rim tiles."""
    import link_amd as la
    frames = [_frame(dims, seed=200 + 10 * i + sum(dims)) for i in range(3)]
    bounds = frames[0][2]
    n = frames[0][0].shape[0]
    plan = _plan(n, bounds, k1_form=0, k2_form=0)          # the pre_mix form the batch's K1 role runs; strips
    ref = [plan.run(f, co).clone() for f, co, _ in frames]
    plan.check()
    plan.set_tuning(k1_form=0, k2_form=SQUARE)
    square = [plan.run(f, co).clone() for f, co, _ in frames]
    plan.check()
    batch = _bind(la.ElkCoreBatch(3, n, C, BASEOP, C // GROUPS, R, S, bounds, torch.device("cuda")))
    outs = [o.clone() for o in batch.run([f for f, _, _ in frames], [co for _, co, _ in frames])]
    batch.check()
    for i in range(3):
        assert torch.equal(outs[i], ref[i]), (dims, i)
        assert torch.equal(outs[i], square[i]), (dims, i)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_strips_half_rows(dt):
    """(e): fp16 / bf16 rows at the kernel boundary (their own translation units): strips == square rim tiles, bit for bit."""
    dims = (5, 5, 5)
    feats, coords, bounds = _frame(dims, seed=7)
    feats = feats.to(dt)
    plan = _plan(feats.shape[0], bounds)
    for zsplit in (1, 2):
        plan.set_tuning(k2_zsplit=zsplit, k2_form=SQUARE)
        square = plan.run(feats, coords).clone()
        plan.check()
        plan.set_tuning(k2_zsplit=zsplit, k2_form=0)
        strips = plan.run(feats, coords).clone()
        plan.check()
        assert strips.dtype == dt and torch.equal(strips, square), (dt, zsplit)
