"""R_core's training path (link_amd.elk.elk_core_train: _ElkCoreTrain for C % 16 == 0 up to 128, torch LayerNorm / Linear around
_ElkMid otherwise) gated per tensor on the float64 arbiter of tests/grad64.py:

    rel_err(got[k], g64[k]) <= 4 * o32[k] + 2 * o_round[k] + 2e-6      for out and EVERY gradient tensor,

o32[k] = what evaluating the reference's own formula in fp32 costs for that tensor (two row orders), o_round = the rounding of
the feats gradient into a 16-bit row type.  Nothing in the bound comes from the kernels or from the op-by-op composition.

  * the dispatch lattice: every lanes-per-row instance (C = 4 ... 256), the pre_mix backward widths 80 / 96 / 112, r = 1, 2, 3,
    groups 1 / 2 / 4, on a frame with negative coordinates and two batch items; shapes a guard refuses are asserted refused;
  * row counts around the 16-row MFMA tile (1, 15, 16, 17) and past the batched weight-gradient threshold (4097);
  * |theta| in the thousands of radians (LiDAR-shaped coordinates to 2 000), the encoder variant (coord_div = 2) among them;
  * isolated voxels, where the theta gradients are analytically zero and an absolute bound replaces the relative one;
  * fp16 / bf16 rows on the cases of tests/test_gpu_amp_train.py.

Each case's figures go to train_parity.jsonl in the directory LINK_AMD_PARITY_DIR names (profiles/train_parity.jsonl is one run)."""
import pytest
import torch

import grad64 as G
from helpers import s_uniform
from test_gpu_amp_train import CORE_CASES

pytestmark = pytest.mark.gpu


def _train(feats, coords, p, s, r, baseop, groups, div, gout):
    """elk_core_train on the GPU: {"out", "feats", every parameter} as grad64.reference_grads names them."""
    import link_amd as la
    from link_amd.elk import elk_core_train
    cg = feats.shape[1] // groups
    co = coords.cuda()
    f = feats.detach().cuda().requires_grad_(True)
    q = {k: (v.detach().cuda().requires_grad_(True) if v is not None else None) for k, v in p.items()}
    index = la.BlockIndex(co, s)
    out = elk_core_train(f, co, index, q["w_pre"], q["pre_ln_w"], q["pre_ln_b"], q["w_pos"], q["alpha"], q["ln_w"], q["ln_b"],
                         baseop, cg, r, div, 1e-6)
    out.backward(gout.cuda())
    got = {"out": out.detach(), "feats": f.grad}
    got.update({k: v.grad for k, v in q.items() if v is not None})
    return got


def _case(suite, feats, coords, s, r, baseop, groups, div=1.0, dtype=torch.float32):
    C = feats.shape[1]
    return dict(suite=suite, C=C, groups=groups, op=baseop, s=s, r=r, n=int(coords.shape[0]), div=div, rows=str(dtype)[6:])


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch lattice
# ------------------------------------------------------------------------------------------------------------------------------
def _lattice_frame():
    coords = s_uniform(3000, grid=64)
    coords[:, :3] -= torch.tensor([40, 17, 70], dtype=torch.int32)     # blocks on both sides of zero in x and y, all below in z
    coords[1500:, 3] = 1                                               # two batch items
    return coords


LATTICE = [
    # C, groups, baseop, s, r.   r = 1 sums the voxel's own block alone: s = 7 keeps ~3 voxels in a block.  C = 256 at r = 3:
    # s = 8 keeps the CPU reference's [blocks, 27, 3C + 1] float64 gather below 100 MB.
    (4, 1, "cos_x", 3, 2),           # lanes per row 4, three idle
    (4, 4, "sin", 7, 1),             # one theta for every channel
    (8, 2, "cos", 3, 3),
    (20, 4, "sin", 5, 2),            # lanes per row 8 with three idle; theta tiled with period 5 across the lanes' float4s
    (20, 1, "cos_x", 7, 1),
    (48, 4, "cos", 7, 1),            # pre_mix backward width 48
    (48, 1, "cos_x", 4, 3),
    (80, 2, "sin", 3, 3),            # widths 80 / 96 / 112: _ElkCoreTrain with idle lanes in the 32-lane rows
    (80, 1, "cos_x", 5, 2),
    (96, 1, "cos_x", 4, 2),
    (96, 2, "sin", 7, 1),
    (112, 4, "cos", 5, 3),
    (112, 1, "cos_x", 7, 1),
    (160, 2, "sin", 3, 2),           # C > 128: _ElkMid on 64 lanes per row (24 idle)
    (160, 1, "cos", 7, 1),
    (256, 1, "cos_x", 8, 3),         # the whole wave is one row
    (256, 4, "cos", 5, 2),
    (256, 2, "sin", 7, 1),
]


def _refusal(C, r):
    """The guard of include/link_amd.h that refuses a training shape, or None: check_desc (0 < c <= 256, 0 < r), train_args_ok
    (the group kernels: c % 4 == 0, r <= 3)."""
    if C > 256:
        return "check_desc: c > 256"
    if C % 4:
        return "train_args_ok: c % 4 != 0 (group kernels only)"
    if r > 3:
        return "train_args_ok: r > 3 (group kernels only)"
    return None


@pytest.mark.parametrize("C,groups,baseop,s,r", LATTICE + [(6, 2, "cos", 3, 2), (260, 1, "cos", 3, 2), (64, 2, "cos", 3, 4)])
def test_dispatch_lattice(C, groups, baseop, s, r):
    from link_amd._lib import LinkAmdError
    assert C % groups == 0 and (baseop != "cos_x" or groups == 1)
    coords = _lattice_frame()
    feats, gout = G.make_rows(coords.shape[0], C)
    p = G.make_params(C, C // groups, baseop, seed=11)
    args = (feats, coords, p, s, r, baseop, groups, 1.0, gout)
    why = _refusal(C, r)
    if why is not None:                                  # refused loudly: no quiet fall-back to another path
        with pytest.raises(LinkAmdError):
            _train(*args)
        return
    g64, o32 = G.yardstick(*args)
    G.gate(_case("lattice", feats, coords, s, r, baseop, groups), g64, o32, _train(*args))


# ------------------------------------------------------------------------------------------------------------------------------
# row counts
# ------------------------------------------------------------------------------------------------------------------------------
def _edge_frame(n):
    """n voxels dense enough for blocks of several voxels with neighbours: 6^3 cells (n <= 17, s = 3) or 32^3 (n = 4097, s = 4)."""
    grid, s = (6, 3) if n <= 17 else (32, 4)
    coords = s_uniform(n, grid=grid, seed=5)
    coords[:, :3] -= torch.tensor([2, 3, 1], dtype=torch.int32)
    return coords, s


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
@pytest.mark.parametrize("C,groups,baseop,r", [(64, 2, "cos", 3), (32, 1, "cos_x", 2)])
def test_row_count_edges(C, groups, baseop, r, n):
    """The 16-row tiles of the MFMA pre_mix kernels (a part tile, a whole tile, one row into the next) and 4097 = 32 x 128 + 1:
    the batched weight gradient with a remainder of one row.  n = 1 is one isolated voxel: new = fin whatever theta is, so the
    theta gradients are analytically zero and take the absolute bound of the isolated-voxel cases."""
    coords, s = _edge_frame(n)
    feats, gout = G.make_rows(n, C)
    p = G.make_params(C, C // groups, baseop, seed=11)
    args = (feats, coords, p, s, r, baseop, groups, 1.0, gout)
    case = _case("row_edges", feats, coords, s, r, baseop, groups)
    if n == 1:
        _isolated_gate(case, args)
        return
    g64, o32 = G.yardstick(*args)
    G.gate(case, g64, o32, _train(*args))


# ------------------------------------------------------------------------------------------------------------------------------
# large theta
# ------------------------------------------------------------------------------------------------------------------------------
LARGE_THETA = [
    # C, groups, baseop, s, r, div
    (64, 2, "cos", 14, 3, 1.0),
    (64, 1, "cos_x", 16, 2, 1.0),
    (16, 2, "sin", 5, 3, 1.0),       # heavy cancellation in the w_pos gradient: o32 ~ 6e-3
    (64, 1, "cos_x", 16, 2, 2.0),    # the encoder variant: coordinates x 2, theta of xyz / 2
]


@pytest.mark.parametrize("C,groups,baseop,s,r,div", LARGE_THETA)
def test_large_theta(C, groups, baseop, s, r, div):
    g64, o32, args = _standard("lidar", 6000, C, groups, baseop, s, r, div, torch.float32)
    coords = args[1]
    assert int(coords[:, :3].max()) > 1500 * int(div)    # |theta| in the thousands of radians is what these cases are for
    G.gate(_case("large_theta", args[0], coords, s, r, baseop, groups, div), g64, o32, _train(*args))


def _standard(frame, n, C, groups, baseop, s, r, div, dtype):
    """(g64, o32, args) of a case on the frames, rows and parameters tests/test_gpu_train.py and test_gpu_amp_train.py use;
    the reference is computed once per case and session (grad64.cached_yardstick)."""
    coords = G.make_frame(frame, n, div)
    feats, gout = G.make_rows(coords.shape[0], C, dtype)
    p = G.make_params(C, C // groups, baseop, seed=11)
    args = (feats, coords, p, s, r, baseop, groups, div, gout)
    g64, o32 = G.cached_yardstick((frame, n, C, groups, baseop, s, r, div, str(dtype)), lambda: args)
    return g64, o32, args


# ------------------------------------------------------------------------------------------------------------------------------
# isolated voxels
# ------------------------------------------------------------------------------------------------------------------------------
def _isolated_gate(case, args):
    """out, the feats gradient and the LayerNorm / pre_mix parameter gradients through the gate; the theta gradients (w_pos,
    alpha), analytically zero, against the fp32 evaluation of the oracle: max|g| <= 4 max|g32| + 2e-6 max|g64["feats"]|."""
    g64, o32 = G.yardstick(*args)
    g32 = G.reference_grads(*args, dtype=torch.float32)
    zero = [k for k in ("w_pos", "alpha") if k in g64]
    for k in zero:
        assert bool(torch.isfinite(g32[k]).all()), k     # on the CPU, before anything runs on the GPU
    got = _train(*args)
    G.gate(case, {k: v for k, v in g64.items() if k not in zero}, o32, got)
    G.gate_zero(case, g64, g32, got, zero)


@pytest.mark.parametrize("C,groups,baseop,s,r", [(32, 1, "cos_x", 3, 2), (64, 2, "cos", 3, 3)])
def test_isolated_voxels(C, groups, baseop, s, r):
    """500 voxels, one per block, the blocks on a lattice of pitch r (voxels of pitch s * r, anywhere inside their block): no block
    has a neighbour among the r^3 offsets, so aggregate(X) = X and new = fin for every theta."""
    pitch = s * r
    g = torch.Generator().manual_seed(31)
    lin = torch.randperm(512, generator=g)[:500]
    cell = torch.stack([lin % 8, (lin // 8) % 8, lin // 64], 1)
    coords = torch.zeros(500, 4, dtype=torch.int32)
    coords[:, :3] = (cell * pitch + torch.randint(0, s, (500, 3), generator=g) - 4 * pitch).int()
    feats, gout = G.make_rows(500, C)
    p = G.make_params(C, C // groups, baseop, seed=11)
    _isolated_gate(_case("isolated", feats, coords, s, r, baseop, groups), (feats, coords, p, s, r, baseop, groups, 1.0, gout))


# ------------------------------------------------------------------------------------------------------------------------------
# 16-bit rows
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("C,groups,baseop,s,r,div,frame", CORE_CASES)
def test_half_rows(dtype, C, groups, baseop, s, r, div, frame):
    """The reference is evaluated on the widened rows; the feats gradient comes back in the row type, and o_round["feats"] is
    what rounding the float64 gradient into that type costs (0 for every other tensor: they are fp32)."""
    g64, o32, args = _standard(frame, 6000, C, groups, baseop, s, r, div, dtype)
    got = _train(*args)
    assert got["feats"].dtype == dtype and all(v.dtype == torch.float32 for k, v in got.items() if k != "feats")
    G.gate(_case("half_rows", args[0], args[1], s, r, baseop, groups, div, dtype), g64, o32, got, G.rounding_cost(g64, dtype))
