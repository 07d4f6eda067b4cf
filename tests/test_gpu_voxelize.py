"""link_amd.Voxelizer / points_to_voxel / DynamicVoxelEncoder (csrc/voxelize.hip) against the fixtures recorded from the reference's
own code (tests/golden/make_golden_voxelize.py): coors, num_points, the voxel count and the padded voxels bit for bit; the per-voxel
mean within n 2^-24 max_i |x_i| of the float64 mean of the RECORDED rows (n = the voxel's point count; the worst case of summing n
float32 values in any order plus the divide, so the bound comes from the number format alone)."""
import numpy as np
import pytest
import torch

from helpers import load_golden

import voxel_oracle as VO

HARD, DYN = VO.HARD, VO.DYN

pytestmark = pytest.mark.gpu

VS = [0.075, 0.075, 0.2]
SMALL = [-6.0, -6.0, -5.0, 6.0, 6.0, 3.0]
_VOXELIZERS = {}


def voxelizer(rng, max_points=10, max_voxels=20000):
    """one Voxelizer per geometry for the whole module: every test after the first runs on a workspace earlier clouds went through"""
    import link_amd as la
    key = (tuple(float(v) for v in rng), max_points, max_voxels)
    if key not in _VOXELIZERS:
        _VOXELIZERS[key] = la.Voxelizer(VS, list(rng), max_points, max_voxels)
    return _VOXELIZERS[key]


def clouds_of(g):
    return [torch.from_numpy(g[f"points{k}"]).cuda() for k in range(g["meta"]["clouds"])]


def check_hard(g, voxels, feats, coors, num):
    """the concatenation over the fixture's clouds, bit for bit; the mean within the bound"""
    m = g["meta"]
    ks = range(m["clouds"])
    want_c = np.concatenate([np.concatenate([np.full((g[f"coors{k}"].shape[0], 1), k, np.int32), g[f"coors{k}"]], 1) for k in ks])
    want_n = np.concatenate([g[f"num{k}"] for k in ks])
    want_v = np.concatenate([g[f"voxels{k}"] for k in ks])
    assert coors.dtype == torch.int32 and num.dtype == torch.int32 and feats.dtype == torch.float32
    assert coors.shape[0] == want_c.shape[0] == sum(m["voxels"])
    assert np.array_equal(coors.cpu().numpy(), want_c) and np.array_equal(num.cpu().numpy(), want_n)
    if voxels is not None:
        assert voxels.cpu().numpy().tobytes() == want_v.tobytes()
    mean64, bound = VO.hard_mean64(want_v, want_n)
    err = np.abs(feats.cpu().numpy().astype(np.float64) - mean64)
    print("voxels", want_c.shape[0], "max |mean - float64 mean| / bound =", float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
    assert np.all(err <= bound)


@pytest.mark.parametrize("name", HARD)
def test_hard_fixture(name):
    import link_amd as la
    g = load_golden(f"voxelize_hard_{name}.npz")
    m = g["meta"]
    pts = clouds_of(g)
    if not m["reverse_index"] or name in ("n65", "onevoxel"):             # the reference's own function, one cloud
        voxels, coors, num = la.points_to_voxel(pts[0], g["voxel_size"], g["range"], m["max_points"], m["reverse_index"], m["max_voxels"])
        assert coors.dtype == torch.int32 and np.array_equal(coors.cpu().numpy(), g["coors0"])
        assert np.array_equal(num.cpu().numpy(), g["num0"]) and voxels.cpu().numpy().tobytes() == g["voxels0"].tobytes()
        if not m["reverse_index"]:
            return
    v = voxelizer(g["range"])
    assert np.array_equal(v.grid_size, g["shape"])
    arg = pts if len(pts) > 1 else pts[0]
    voxels, feats, coors, num = v.generate(arg, max_voxels=m["max_voxels"], return_voxels=True)
    check_hard(g, voxels, feats, coors, num)
    feats2, coors2, num2 = v.generate(arg, max_voxels=m["max_voxels"])   # a null voxels pointer: the same mean, bit for bit
    assert torch.equal(feats2, feats) and torch.equal(coors2, coors) and torch.equal(num2, num)


@pytest.mark.parametrize("name", DYN)
def test_dynamic_fixture(name):
    import link_amd as la
    g = load_golden(f"voxelize_dyn_{name}.npz")
    enc = la.DynamicVoxelEncoder(g["range"].tolist(), g["voxel_size"].tolist())
    voxels, coors, shape = enc(clouds_of(g))
    assert coors.dtype == torch.int64 and shape.dtype == np.int32 and np.array_equal(shape, g["shape"])
    assert np.array_equal(coors.cpu().numpy(), g["coors"])
    parts = [VO.dynamic(g[f"points{k}"], g["range"], g["voxel_size"]) for k in range(g["meta"]["clouds"])]
    mean64, bound = np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
    assert tuple(voxels.shape) == g["voxels"].shape
    got = voxels.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - mean64) <= bound)
    # and directly against the recorded reference output: both lie within `bound` of the float64 mean of the same points
    assert np.all(np.abs(g["voxels"].astype(np.float64) - mean64) <= bound) and np.all(np.abs(got - g["voxels"]) <= 2 * bound)
    again, coors2, _ = enc(clouds_of(g))                                  # the workspace was left clean; two runs are bit for bit equal
    assert torch.equal(again, voxels) and torch.equal(coors2, coors)


def test_padded_equals_variable_length_and_is_zero_after():
    g = load_golden("voxelize_hard_batch3.npz")
    v = voxelizer(g["range"])
    pts = clouds_of(g)
    mv = g["meta"]["max_voxels"]
    voxels, feats, coors, num = v.generate(pts, max_voxels=mv, return_voxels=True)
    m = coors.shape[0]
    for cap in (None, m + 77, m, m - 5):
        pv, pf, pc, pn, off = v.generate_padded(pts, max_voxels=mv, return_voxels=True, capacity=cap)
        want_cap = cap if cap is not None else min(sum(p.shape[0] for p in pts), 3 * mv)
        assert pc.shape[0] == pn.shape[0] == pf.shape[0] == pv.shape[0] == want_cap
        k = min(m, want_cap)
        counts = [min(c, want_cap) for c in np.cumsum([0] + g["meta"]["voxels"]).tolist()]
        assert off.dtype == torch.int32 and off.cpu().tolist() == counts                      # per sample, clamped to the capacity
        assert torch.equal(pv[:k], voxels[:k]) and torch.equal(pf[:k], feats[:k]) and torch.equal(pc[:k], coors[:k]) and torch.equal(pn[:k], num[:k])
        for t in (pv, pf, pc, pn):
            assert not t[k:].any()


def test_two_runs_are_bitwise_equal_and_a_second_cloud_is_correct():
    a, b = load_golden("voxelize_hard_clustered.npz"), load_golden("voxelize_hard_capped.npz")
    v = voxelizer(a["range"])
    first = v.generate(clouds_of(a)[0], return_voxels=True)
    second = v.generate(clouds_of(a)[0], return_voxels=True)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    check_hard(b, *v.generate(clouds_of(b)[0], max_voxels=3000, return_voxels=True))    # another cloud on the same workspace
    check_hard(a, *v.generate(clouds_of(a)[0], return_voxels=True))                     # and back


def test_points_that_are_not_finite_are_dropped():
    import link_amd as la
    g = load_golden("voxelize_hard_n4097.npz")
    p = g["points0"].copy()
    bad = p[:64].copy()
    for i, val in enumerate((np.nan, np.inf, -np.inf)):
        for d in range(3):
            bad[(i * 3 + d)::9, d] = val
    mixed = np.concatenate([bad[:20], p[:2000], bad[20:], p[2000:]])
    v = voxelizer(g["range"])
    got = v.generate(torch.from_numpy(mixed).cuda(), return_voxels=True)
    check_hard(g, *got)
    want = VO.dynamic(p, g["range"], g["voxel_size"])
    voxels, coors, _ = la.DynamicVoxelEncoder(g["range"].tolist(), g["voxel_size"].tolist())([torch.from_numpy(mixed).cuda()])
    assert np.array_equal(coors.cpu().numpy()[:, 1:], want[0]) and not coors[:, 0].any()
    assert np.all(np.abs(voxels.cpu().numpy().astype(np.float64) - want[2]) <= want[3])


def test_voxelizer_feeds_the_detection_backbone():
    import link_amd as la
    from link_amd.synth import s_nusc
    co, fe, pts = s_nusc(seed=3, n_az=200, return_points=True)
    rng = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
    v = voxelizer(rng, 10, 120000)
    feats, coors, num = v.generate(torch.from_numpy(pts.astype(np.float32)).cuda())
    m = coors.shape[0]
    assert coors.dtype == torch.int32 and tuple(coors.shape) == (m, 4) and tuple(feats.shape) == (m, 5) and feats.dtype == torch.float32
    c = coors.cpu().numpy().astype(np.int64)
    assert not c[:, 0].any() and (c[:, 1:] >= 0).all() and (c[:, 1:] < [40, 1440, 1440]).all()     # b, z, y, x
    lin = (c[:, 1] * 1440 + c[:, 2]) * 1440 + c[:, 3]
    assert np.unique(lin).shape[0] == m                                   # the backbone's site tables need unique rows
    mine = (co[:, 2].astype(np.int64) * 1440 + co[:, 1]) * 1440 + co[:, 0]     # the float64 host restatement of synth.s_nusc (x, y, z, b)
    assert np.intersect1d(lin, mine).shape[0] >= 0.999 * max(m, mine.shape[0])
    assert int(num.min()) >= 1 and int(num.max()) <= 10
    torch.manual_seed(0)
    net = la.SpMiddleResNetFHDELKv3(num_input_features=5).cuda().eval()
    with torch.no_grad():
        bev, scales = net(feats, coors, 1, v.grid_size)
    assert tuple(bev.shape) == (1, 256, 180, 180) and bool(torch.isfinite(bev).all())
    assert scales["conv1"].features.shape[0] == m


def test_generate_padded_in_a_captured_graph():
    g = load_golden("voxelize_hard_clustered.npz")
    v = voxelizer(g["range"])
    p = clouds_of(g)[0]
    eager = v.generate_padded(p, return_voxels=True)                      # also leaves the workspace and the offsets tensor in place
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v.generate_padded(p, return_voxels=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = v.generate_padded(p, return_voxels=True)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert torch.equal(x, y)
    m = int(out[4][-1])
    check_hard(g, out[0][:m], out[1][:m], out[2][:m], out[3][:m])
