"""Sparse convolutions with any per-axis kernel size and stride, plain and transposed (link_amd.Conv3d / F.conv3d on the
general kernel-map builder, csrc/kmap.hip): the reference's fixtures, the maps against the hash chain and the torch
composition they replace, gradients against float64 autograd over a gather-matmul restatement of the same tables."""
import numpy as np
import pytest
import torch

from helpers import golden_files, lidar_like, load_golden, rel_err

pytestmark = pytest.mark.gpu


def _run_chain(make_tensor, make_layer, g):
    x = make_tensor(torch.from_numpy(g["feats"]).cuda(), torch.from_numpy(g["coords"]).cuda(), 1)
    x.cmaps.setdefault(x.stride, x.coords)
    outs = []
    with torch.no_grad():
        for i, lay in enumerate(g["meta"]["layers"]):
            x = make_layer(x, lay, torch.from_numpy(g[f"k{i}"]).cuda())
            outs.append(x)
    return outs


def _check_chain(outs, g, name):
    for i, (x, lay) in enumerate(zip(outs, g["meta"]["layers"])):
        assert tuple(x.s) == tuple(lay["out_stride"]), (name, i)
        assert np.array_equal(x.C.cpu().numpy(), g[f"x{i}_C"]), (name, i)
        if g["meta"]["features_valid"]:
            err = rel_err(x.F.cpu().numpy(), g[f"x{i}_F"])
            print(name, i, "rel_err", err)
            assert err < 1e-5, (name, i, err)


@pytest.mark.parametrize("name", golden_files("g_generalconv_*.npz"))
def test_reference_fixtures_through_the_module(name):
    """Every recorded chain through link_amd.Conv3d: coordinates, their order and the strides bit-exact, features < 1e-5
    (two-batch files: coordinates only -- the reference's CPU neighbour hash is defective there)."""
    import link_amd as la
    g = load_golden(name)

    def layer(x, lay, k):
        conv = la.Conv3d(lay["cin"], lay["cout"], tuple(lay["kernel_size"]), tuple(lay["stride"]), transposed=lay["transposed"]).cuda()
        assert conv.kernel.shape == k.shape
        with torch.no_grad():
            conv.kernel.copy_(k)
        return conv(x)
    _check_chain(_run_chain(la.SparseTensor, layer, g), g, name)


@pytest.mark.parametrize("name", ["g_generalconv_a.npz", "g_generalconv_c.npz"])
def test_reference_fixtures_through_the_functional_form(name):
    """... and through F.conv3d with link_amd registered under the torchsparse names, as unmodified reference code calls it."""
    import sys
    import link_amd as la
    la.install_as_torchsparse()
    try:
        import torchsparse
        import torchsparse.nn.functional as F
        g = load_golden(name)
        layer = lambda x, lay, k: F.conv3d(x, k, tuple(lay["kernel_size"]), None, stride=tuple(lay["stride"]), transposed=lay["transposed"])
        _check_chain(_run_chain(torchsparse.SparseTensor, layer, g), g, name)
    finally:
        for k in [k for k in sys.modules if k == "torchsparse" or k.startswith("torchsparse.")]:
            del sys.modules[k]


# ------------------------------------------------------------------------------------------------
# maps
# ------------------------------------------------------------------------------------------------
def _frame(ts, n=5000):
    """LiDAR-like, two batch items, negative coordinates, on the lattice of the per-axis tensor stride `ts`."""
    per = []
    for b in range(2):
        c = lidar_like(n, seed=11 + b, voxel=0.1).astype(np.int64)
        c[:, :3] -= (211, 97, 6)
        c[:, :3] = c[:, :3] // np.array(ts) * np.array(ts)
        c[:, 3] = b
        per.append(np.unique(c, axis=0))
    c = np.concatenate(per)
    return torch.from_numpy(c[np.random.default_rng(3).permutation(c.shape[0])].astype(np.int32))


def _spdownsample_composition(coords, stride, ks, ts, get_kernel_offsets):
    """The torch composition the builder replaces (this project's spdownsample as it stood before the builder)."""
    ss = torch.tensor([stride[k] * ts[k] for k in range(3)], dtype=torch.int32, device=coords.device)
    if all(stride[k] in (1, ks[k]) for k in range(3)):
        c = coords.clone()
        c[:, :3] = torch.div(c[:, :3], ss, rounding_mode="floor") * ss
    else:
        offs = get_kernel_offsets(ks, ts, device=coords.device)
        lo = coords[:, :3].min(0, keepdim=True).values
        x = (coords[:, None, :3] + offs[None]).reshape(-1, 3)
        b = coords[:, 3:].repeat_interleave(offs.shape[0], 0)
        keep = ((x % ss == 0) & (x >= lo)).all(1)
        c = torch.cat([x, b], 1)[keep]
    return torch.unique(c[:, [3, 0, 1, 2]], dim=0)[:, [1, 2, 3, 0]].contiguous()


GEOMETRIES = [((3, 1, 3), (1, 1, 1)), ((1, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 1), (2, 2, 1)), ((3, 3, 1), (2, 2, 1)),
              ((2, 2, 2), (1, 1, 1)), ((5, 5, 3), (1, 1, 1)), ((3, 2, 3), (1, 1, 1)), ((3, 3, 3), (2, 1, 3)), ((4, 3, 2), (2, 2, 1)),
              ((7, 1, 1), (3, 1, 1)), ((2, 2, 2), (2, 2, 2)), ((1, 1, 1), (2, 2, 2))]


@pytest.mark.parametrize("ts", [(1, 1, 1), (2, 2, 1)])
@pytest.mark.parametrize("ks,st", GEOMETRIES)
def test_maps_equal_hash_chain_and_torch_composition(ks, st, ts):
    """Table == sphashquery(sphash(out, offsets), sphash(in)) bit for bit; output coordinates == the Python spdownsample
    composition; the opposite direction's table == the torch nonzero construction; F.spdownsample gives the same rows."""
    import link_amd as la
    import link_amd.functional as F
    coords = _frame(ts).cuda()
    x = la.SparseTensor(torch.zeros(coords.shape[0], 4, device="cuda"), coords, ts)
    conv = la.Conv3d(4, 4, ks, st).cuda()
    table, back, _, subm, out_c, s_out = conv._route(x, need_back=True)
    assert s_out == tuple(ts[k] * st[k] for k in range(3))
    if any(v > 1 for v in st):
        want_c = _spdownsample_composition(coords, st, ks, ts, la.get_kernel_offsets)
        assert torch.equal(out_c, want_c)
        assert torch.equal(F.spdownsample(coords, st, ks, ts), want_c)
    else:
        assert out_c is x.C
    offs = la.get_kernel_offsets(ks, stride=ts, device="cuda")
    want = la.sphashquery(la.sphash(out_c, offs), la.sphash(coords)).t().contiguous().int()
    assert table.dtype == torch.int32 and torch.equal(table, want)
    assert subm == (all(k % 2 == 1 for k in ks) and all(v == 1 for v in st))
    km = x.kmaps[(x.s, ks, st, 1)]
    jj, kk = torch.nonzero(table >= 0, as_tuple=True)
    up = torch.full((coords.shape[0], table.shape[1]), -1, dtype=torch.int32, device="cuda")
    up[table[jj, kk].long(), kk] = jj.int()
    assert torch.equal(km.nbr_up, up)
    if back is not None:
        assert back is km.nbr_up


@pytest.mark.parametrize("first", [((1, 1, 1), (2, 2, 2)), ((2, 2, 2), (3, 3, 3)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 1), (2, 2, 1))])
@pytest.mark.parametrize("shift", [(0, 0, 0), (3, 1, 5), (-7, 2, -1)])
def test_chained_candidate_layers_filter_with_the_exact_minimum(first, shift):
    """Two strided layers in a row: the second one's candidate rule filters with the per-axis minimum of the FIRST one's
    sites (downsample.py:34,42), not with a lattice point below them.  Kernel < stride (k1 s2, k2 s3) leaves lattice points
    between the inputs' minimum and the first site; the frames start off the lattice.  Yardstick: the torch composition
    applied twice; tables against the hash chain."""
    import link_amd as la
    coords = _frame((1, 1, 1), n=3000)
    coords[:, :3] -= coords[:, :3].min(0).values
    coords[:, :3] += torch.tensor(shift, dtype=torch.int32)
    coords = coords.cuda()
    x = la.SparseTensor(torch.zeros(coords.shape[0], 4, device="cuda"), coords, 1)
    x.cmaps.setdefault(x.stride, x.coords)
    c, s = coords, (1, 1, 1)
    for ks, st in (first, ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (2, 2, 2))):
        with torch.no_grad():
            y = la.Conv3d(4, 4, ks, st).cuda()(x)
        want = _spdownsample_composition(c, st, ks, s, la.get_kernel_offsets)
        assert torch.equal(y.C, want), (ks, st, s, y.C.shape, want.shape)
        offs = la.get_kernel_offsets(ks, stride=s, device="cuda")
        table = x.kmaps[(s, ks, st, 1)].nbr_down
        assert torch.equal(table, la.sphashquery(la.sphash(want, offs), la.sphash(c)).t().contiguous().int())
        x, c, s = y, want, tuple(s[k] * st[k] for k in range(3))
        assert y.s == s


def test_spdownsample_on_coordinates_off_the_tensor_stride_lattice():
    """Inputs that are not multiples of tensor_stride give no site by the reference's rule ((c + j ts) % (s ts) == 0 needs
    c % ts == 0): the device path and the torch composition return the same rows."""
    import link_amd as la
    import link_amd.functional as F
    coords = _frame((1, 1, 1), n=3000).cuda()              # every residue modulo the tensor stride occurs
    for ks, st, ts in (((3, 3, 3), (2, 2, 2), (2, 2, 2)), ((3, 3, 1), (2, 2, 1), (2, 3, 1)), ((1, 1, 1), (2, 2, 2), (1, 2, 1))):
        want = _spdownsample_composition(coords, st, ks, ts, la.get_kernel_offsets)
        assert 0 < want.shape[0] < coords.shape[0] * 27
        assert torch.equal(F.spdownsample(coords, st, ks, ts), want), (ks, st, ts)


def test_map_builds_and_forwards_are_deterministic():
    import link_amd as la
    coords = _frame((1, 1, 1)).cuda()
    feats = torch.randn(coords.shape[0], 32, generator=torch.Generator().manual_seed(0)).cuda()
    conv = la.Conv3d(32, 32, 3, 2).cuda()
    res = []
    for _ in range(2):
        x = la.SparseTensor(feats, coords.clone(), 1)
        with torch.no_grad():
            y = conv(x)
        km = x.kmaps[(x.s, conv.kernel_size, conv.stride, 1)]
        res.append((km.out_coords, km.nbr_down, km.nbr_up, y.F))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fallback_beyond_the_dense_grid_limit(monkeypatch):
    """A frame whose bounding grid exceeds the dense-grid limit (second batch item four million voxels away) takes the Python
    spdownsample and the hash chain, and gives the table of the same frame shifted into range."""
    import link_amd as la
    import link_amd.elk as E
    base = _frame((1, 1, 1), n=3000)
    base[:, :3] -= base[:, :3].min(0).values
    corner = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.int32)     # both items share the minimum corner: the >= minimum
    keep = (base[:, :3] != 0).any(1)                                            # test reads the same in both frames
    base = torch.cat([corner, base[keep]])
    far = base.clone()
    far[far[:, 3] == 1, 0] += 4_000_000
    calls = []
    real = E.sphashquery
    monkeypatch.setattr(E, "sphashquery", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for ks, st in (((3, 3, 3), (2, 2, 2)), ((3, 1, 3), (1, 1, 1)), ((2, 2, 1), (2, 2, 1))):
        got = []
        for c in (base, far):
            x = la.SparseTensor(torch.zeros(c.shape[0], 4, device="cuda"), c.cuda(), 1)
            n0 = len(calls)
            table, _, _, _, out_c, _ = la.Conv3d(4, 4, ks, st).cuda()._route(x, need_back=False)
            got.append((table, out_c, len(calls) - n0))
        assert got[0][2] == 0 and got[1][2] == 1, (ks, st)            # in range: the builder; beyond: the hash chain
        assert torch.equal(got[0][0], got[1][0])
        back = got[1][1].clone()
        back[back[:, 3] == 1, 0] -= 4_000_000
        assert torch.equal(got[0][1], back)


# ------------------------------------------------------------------------------------------------
# contraction and gradients
# ------------------------------------------------------------------------------------------------
def _gather_matmul(f, table, w):
    """out[j] = sum_k f[table[j, k]] @ w[k] in float64 torch (autograd): absent entries read a zero row."""
    pad = torch.cat([f, f.new_zeros(1, f.shape[1])])
    idx = torch.where(table < 0, torch.full_like(table, f.shape[0]), table).long()
    return sum(pad[idx[:, k]] @ w[k] for k in range(table.shape[1]))


@pytest.mark.parametrize("widths", [(16, 32, 16), (6, 10, 7)])
def test_general_chain_gradients(widths):
    """k3 s2 -> (3,1,3) at tensor stride 2 -> k3 s2 transposed: forward, input, kernel and bias gradients."""
    import link_amd as la
    c0, c1, c2 = widths
    coords = _frame((1, 1, 1)).cuda()
    n = coords.shape[0]
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(n, c0, generator=g)
    torch.manual_seed(2)
    l1 = la.Conv3d(c0, c1, 3, 2, bias=True).cuda(); l2 = la.Conv3d(c1, c1, (3, 1, 3), 1).cuda()
    l3 = la.Conv3d(c1, c2, 3, 2, bias=True, transposed=True).cuda()
    f = feats.cuda().requires_grad_(True)
    x0 = la.SparseTensor(f, coords, 1); x0.cmaps.setdefault(x0.stride, x0.coords)
    x1 = l1(x0); x2 = l2(x1); x3 = l3(x2)
    assert x3.s == (1, 1, 1) and x3.C is x0.C and x2.s == (2, 2, 2)
    gout = torch.randn(n, c2, generator=g)
    x3.F.backward(gout.cuda())
    km = x0.kmaps[((1, 1, 1), (3, 3, 3), (2, 2, 2), 1)]
    t1, t3 = km.nbr_down.cpu(), km.nbr_up.cpu()
    t2 = l2._neighbor_table(x1)[0].cpu()
    fr = feats.double().requires_grad_(True)
    ws = [l.kernel.detach().cpu().double().requires_grad_(True) for l in (l1, l2, l3)]
    bs = [l.bias.detach().cpu().double().requires_grad_(True) for l in (l1, l3)]
    r = _gather_matmul(_gather_matmul(_gather_matmul(fr, t1, ws[0]) + bs[0], t2, ws[1]), t3, ws[2]) + bs[1]
    r.backward(gout.double())
    figs = {"out": rel_err(x3.F.detach().cpu().numpy(), r.detach().numpy()), "g_in": rel_err(f.grad.cpu().numpy(), fr.grad.numpy())}
    for i, (l, w) in enumerate(zip((l1, l2, l3), ws)):
        figs[f"g_k{i}"] = rel_err(l.kernel.grad.cpu().numpy(), w.grad.numpy())
    for i, (l, b) in enumerate(zip((l1, l3), bs)):
        figs[f"g_b{i}"] = rel_err(l.bias.grad.cpu().numpy(), b.grad.numpy())
    print(widths, figs)
    assert figs["out"] < 1e-5 and figs["g_in"] < 1e-5
    assert all(figs[k] < 1e-4 for k in figs if k.startswith("g_k")) and all(figs[k] < 1e-5 for k in figs if k.startswith("g_b"))


@pytest.mark.parametrize("ks,c", [((2, 2, 2), 16), ((3, 2, 1), 8), ((5, 5, 3), 16)])
def test_stride1_kernels_against_restatement(ks, c):
    """Even extents at stride 1 are not a symmetric relation: the input gradient must come from the transposed table, not
    from the flipped-weights shortcut of odd kernels.  (5,5,3): K = 75 runs the table kernel's lane = channel form."""
    import link_amd as la
    coords = _frame((1, 1, 1), n=3000).cuda()
    n = coords.shape[0]
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(n, c, generator=g)
    conv = la.Conv3d(c, c, ks, 1).cuda()
    f = feats.cuda().requires_grad_(True)
    x = la.SparseTensor(f, coords, 1)
    y = conv(x)
    gout = torch.randn(n, c, generator=g)
    y.F.backward(gout.cuda())
    table = conv._neighbor_table(x)[0]
    assert table.shape[1] == ks[0] * ks[1] * ks[2]
    fr = feats.double().requires_grad_(True)
    w = conv.kernel.detach().cpu().double().requires_grad_(True)
    r = _gather_matmul(fr, table.cpu(), w)
    r.backward(gout.double())
    figs = (rel_err(y.F.detach().cpu().numpy(), r.detach().numpy()), rel_err(f.grad.cpu().numpy(), fr.grad.numpy()),
            rel_err(conv.kernel.grad.cpu().numpy(), w.grad.numpy()))
    print(ks, figs)
    assert figs[0] < 1e-5 and figs[1] < 1e-5 and figs[2] < 1e-4


def test_table_and_pair_forms_agree_on_a_general_strided_table():
    import link_amd as la
    from link_amd.elk import subm_conv
    coords = _frame((1, 1, 1)).cuda()
    feats = torch.randn(coords.shape[0], 64, generator=torch.Generator().manual_seed(1)).cuda()
    x = la.SparseTensor(feats, coords, 1)
    conv = la.Conv3d(64, 64, (3, 3, 1), (2, 2, 1)).cuda()
    table, back, _, _, out_c, _ = conv._route(x, need_back=True)
    w = conv.kernel.detach()
    for t, src in ((table, feats), (back, torch.randn(out_c.shape[0], 64, device="cuda"))):
        a = subm_conv(src, w, t, None, form="pairs")
        b = subm_conv(src, w, t, None, form="table")
        assert not t._link_pairs.direct
        err = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print("pairs vs table", err)
        assert err < 1e-5
        ref = _gather_matmul(src.cpu().double(), t.cpu(), w.cpu().double())
        assert rel_err(a.cpu().numpy(), ref.numpy()) < 1e-5


def test_transposed_without_a_matching_map_raises_keyerror():
    import link_amd as la
    import link_amd.functional as F
    coords = _frame((1, 1, 1), n=2000).cuda()
    x = la.SparseTensor(torch.randn(coords.shape[0], 8, device="cuda"), coords, 2)
    x.cmaps.setdefault((1, 1, 1), coords)
    up = la.Conv3d(8, 8, 3, 2, transposed=True).cuda()
    with pytest.raises(KeyError):
        up(x)
    with pytest.raises(KeyError):
        la.Conv3d(8, 8, (3, 1, 3), 1, transposed=True).cuda()(x)
    with pytest.raises(KeyError):
        F.conv3d(x, up.kernel, 3, None, stride=2, transposed=True)
    # a stride-1 layer leaves its map under the reference's key: the transposed twin finds it
    y = la.Conv3d(8, 8, 3, 1).cuda()(x)
    assert (x.s, (3, 3, 3), (1, 1, 1), 1) in x.kmaps
    z = la.Conv3d(8, 8, 3, 1, transposed=True).cuda()(y)
    assert z.C is x.C and z.s == x.s


def test_strided_general_layer_under_autocast():
    """One k3 s2 layer under torch.autocast(fp16): fp16 rows, within one fp16 rounding (2^-10 of the largest value; the bound
    test_pair_form_half_rows uses for the 16-bit matrix-core path) of the fp32 run on the rounded rows and weights."""
    import link_amd as la
    coords = _frame((1, 1, 1)).cuda()
    feats = torch.randn(coords.shape[0], 64, generator=torch.Generator().manual_seed(4)).cuda()
    conv = la.Conv3d(64, 64, 3, 2).cuda()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.float16):
            a = conv(la.SparseTensor(feats, coords, 1))
        ref = la.Conv3d(64, 64, 3, 2).cuda()
        ref.kernel.copy_(conv.kernel.half().float())
        b = ref(la.SparseTensor(feats.half().float(), coords, 1))
    assert a.F.dtype == torch.float16 and b.F.dtype == torch.float32 and torch.equal(a.C, b.C) and a.s == (2, 2, 2)
    err = rel_err(a.F.float().cpu().numpy(), b.F.cpu().numpy())
    print("autocast rel_err", err)
    assert err < 2.0 ** -10


def test_fused_inference_form_on_a_general_geometry():
    """forward_affine (convolution + folded BatchNorm + ReLU in one launch) only sees a table: same rows as the parts."""
    import link_amd as la
    coords = _frame((1, 1, 1)).cuda()
    feats = torch.randn(coords.shape[0], 32, generator=torch.Generator().manual_seed(6)).cuda()
    conv = la.Conv3d(32, 32, (3, 3, 1), (2, 2, 1)).cuda()
    sc, sh = torch.rand(32, device="cuda") + 0.5, torch.randn(32, device="cuda")
    with torch.no_grad():
        a = conv.forward_affine(la.SparseTensor(feats, coords, 1), sc, sh, relu=True)
        b = conv(la.SparseTensor(feats, coords, 1))
    assert torch.equal(a.C, b.C) and a.s == b.s == (2, 2, 1)
    assert rel_err(a.F.cpu().numpy(), torch.relu(b.F * sc + sh).cpu().numpy()) < 1e-5
