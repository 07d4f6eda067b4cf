"""GPU checks of the segmentation front end and validation (csrc/segio.hip, section M of include/link_amd.h; link_amd/segio.py).
Every result is an integer and is compared exactly: the quantiser against the numpy oracle of tests/segio_oracle.py and the fixtures
recorded from the reference's sparse_quantize; the vote against the float64 oracle -- over all points for 16-bit rows (an fp32 sum of
at most three 16-bit values is exact), and for fp32 rows over the points whose float64 top-two gap is at least 1e-4, which must be
99.5 % of a case --; the counters against counters recomputed from the kernel's own predictions.  Sizes follow the sort tile
(link_amd.segio.SORT_TILE): one below, at, one above, several tiles."""
import numpy as np
import pytest
import torch

from helpers import load_golden

import segio_oracle as SO

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("coords", "indices", "inverse", "inverse_local", "voxel_offsets")


def _tile():
    from link_amd import segio
    return segio.SORT_TILE


def _run_int(clouds, capacity=None):
    from link_amd import _lib as L
    from link_amd import segio
    return segio._Quantizer().run([torch.from_numpy(c).to(DEV) for c in clouds], L.SEGQ_INT, capacity=capacity)


def _same(got, want, n_points):
    for name, t in zip(NAMES, got):
        assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), want[name]), name
    status = got[5].tolist()
    assert status[0] == want["total"] and status[1] == want["flags"] and status[3] == n_points, status
    return status


@pytest.mark.parametrize("which", ["0", "1", "2", "tile-1", "tile", "tile+1", "3tile+17"])
def test_quantize_sizes_around_the_sort_tile(which):
    t = _tile()
    n = {"0": 0, "1": 1, "2": 2, "tile-1": t - 1, "tile": t, "tile+1": t + 1, "3tile+17": 3 * t + 17}[which]
    cloud = SO.make_cloud(n, 40 + n % 7, offset=(-9, 4, -2))
    if n > 100:
        assert SO.duplicate_share(cloud) >= 0.3
    want = SO.quantize([cloud])
    _same(_run_int([cloud]), want, n)
    a = _run_int([cloud])
    b = _run_int([cloud])
    assert all(torch.equal(x, y) for x, y in zip(a, b))               # integers: two calls are bit for bit equal


def test_quantize_one_run_across_tiles_and_descending_points():
    same = np.tile(np.array([[5, -3, 11]], np.int32), (5000, 1))
    got = _run_int([same])
    _same(got, SO.quantize([same]), 5000)
    assert got[5].tolist()[0] == 1 and got[1][0].item() == 0 and not got[2].any()
    n = 2 * _tile() + 301
    lin = np.arange(n)[::-1]
    desc = np.stack([lin // 400 - 7, (lin // 20) % 20 - 10, lin % 20], 1).astype(np.int32)      # all distinct, descending order
    got = _run_int([desc])
    _same(got, SO.quantize([desc]), n)
    assert got[5].tolist()[0] == n and got[1].tolist() == list(range(n - 1, -1, -1))


def test_quantize_high_key_bits():
    rng = np.random.default_rng(5)
    pts = rng.integers(0, 1 << 20, (64, 3)).astype(np.int32)
    pts[0], pts[1] = 0, (1 << 20) - 1                                 # the extent is 2^20 - 1 on every axis: 60 key bits
    pts[40:] = pts[rng.integers(0, 40, 24)]
    pts -= 1 << 19
    status = _same(_run_int([pts]), SO.quantize([pts]), 64)
    assert status[1] == 0 and status[2] == 60


def test_quantize_batch_of_three():
    sizes = [1, _tile() + 5, 700]
    clouds = SO.make_batch(sizes, 3)
    want = SO.quantize(clouds)
    got = _run_int(clouds)
    _same(got, want, sum(sizes))
    assert want["voxel_offsets"][1] == 1 and want["coords"][:want["total"], 3].max() == 2
    # empty samples in front, between and behind
    clouds = SO.make_batch([0, 300, 0, 0, 41, 0], 4)
    _same(_run_int(clouds), SO.quantize(clouds), 341)


def test_quantize_round_mode_on_half_multiples():
    from link_amd import _lib as L
    from link_amd import segio
    vs = 0.25
    k = np.arange(-40, 41, dtype=np.float64)
    half = np.stack([(k + 0.5) * vs, (k[::-1] - 0.5) * vs, (2 * k + 0.5) * vs, k], 1).astype(np.float32)      # exact in fp32
    block = np.concatenate([half, SO.make_block(3000, 6, vs)])
    want = SO.quantize([block], voxel_size=vs)
    r = SO.round_coords(half, vs)
    assert np.array_equal(r[:, 0] % 2, np.zeros(81))                  # every half went to the even neighbour
    got = segio._Quantizer().run([torch.from_numpy(block).to(DEV)], L.SEGQ_ROUND, vs)
    _same(got, want, block.shape[0])
    # a voxel size that is not a power of two: the divide must be the correctly rounded one
    vs = 0.05
    block = SO.make_block(5000, 7, vs)
    edge = (np.arange(-200, 200)[:, None] + 0.5) * np.float32(vs) * np.ones((1, 4), np.float32)
    block = np.concatenate([block, edge.astype(np.float32)])
    got = segio._Quantizer().run([torch.from_numpy(block).to(DEV)], L.SEGQ_ROUND, vs)
    _same(got, SO.quantize([block], voxel_size=vs), block.shape[0])


def test_quantize_flags():
    from link_amd import _lib as L
    from link_amd import segio
    ok = SO.make_cloud(500, 8)
    far = SO.make_cloud(300, 9)
    far[17, 1] += 1 << 20
    want = SO.quantize([ok, far, ok[:40]])
    got = _run_int([ok, far, ok[:40]])
    status = _same(got, want, 840)
    assert status[1] == L.SEGQ_FLAG_EXTENT and (got[2][500:800] == -1).all() and int(got[2].max()) < status[0]
    assert want["voxel_offsets"][1] == want["voxel_offsets"][2]
    exact = SO.make_cloud(64, 10)
    exact[0, 2], exact[1, 2] = 0, (1 << 20)                           # exactly 2^20: flagged; one less is not (test_quantize_high_key_bits)
    assert _same(_run_int([exact]), SO.quantize([exact]), 64)[:2] == [0, L.SEGQ_FLAG_EXTENT]
    block = SO.make_block(600, 11)
    bad = block.copy()
    bad[5, 1], bad[77, 0] = np.nan, np.inf
    huge = block.copy()
    huge[9, 2] = 3e9
    q = segio._Quantizer()
    for clouds, flag in (([block, bad], L.SEGQ_FLAG_NONFINITE), ([huge, block], L.SEGQ_FLAG_EXTENT),
                         ([bad, huge, block], L.SEGQ_FLAG_NONFINITE | L.SEGQ_FLAG_EXTENT)):
        want = SO.quantize(clouds, voxel_size=0.05)
        got = q.run([torch.from_numpy(c).to(DEV) for c in clouds], L.SEGQ_ROUND, 0.05)
        assert _same(got, want, 600 * len(clouds))[1] == flag and want["total"] > 0
    import link_amd as la
    with pytest.raises(L.LinkAmdError):
        la.SegVoxelizer(0.05)([torch.from_numpy(bad).to(DEV)])


def test_generate_padded_capacity_and_graph():
    import link_amd as la
    vs = 0.05
    sizes = [900, _tile() + 3]
    blocks = [SO.make_block(n, 12 + i, vs) for i, n in enumerate(sizes)]
    blocks[1][:, :3] += np.float32(3.7)
    vox = la.SegVoxelizer(vs)
    full = SO.quantize(blocks, voxel_size=vs)
    cap = full["total"] - 211                                         # below the total: clamped offsets, -1 for what does not fit
    got = vox.generate_padded([torch.from_numpy(b).to(DEV) for b in blocks], capacity=cap)
    want = SO.quantize(blocks, voxel_size=vs, capacity=cap)
    status = _same(got, want, sum(sizes))
    assert status[0] == full["total"] and got[4].tolist()[-1] == cap and (got[2] == -1).any() and int(got[2].max()) == cap - 1
    # capture, then replay on new data of the same sizes
    static = [torch.from_numpy(b).to(DEV) for b in blocks]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vox.generate_padded(static)                                   # warm-up: workspace and offsets exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = vox.generate_padded(static)
    fresh = [SO.make_block(n, 30 + i, vs) for i, n in enumerate(sizes)]
    for s, f in zip(static, fresh):
        s.copy_(torch.from_numpy(f))
    graph.replay()
    torch.cuda.synchronize()
    _same(out, SO.quantize(fresh, voxel_size=vs), sum(sizes))


def test_recorded_fixtures():
    import link_amd as la
    g = load_golden("segio_quantize_int.npz")
    c, i, v = la.sparse_quantize(torch.from_numpy(g["points"]).to(DEV), return_index=True, return_inverse=True)
    assert c.dtype == torch.int32 and i.dtype == torch.int64 and v.dtype == torch.int64 and c.is_cuda
    assert np.array_equal(c.cpu().numpy(), g["coords"]) and np.array_equal(i.cpu().numpy(), g["indices"]) and np.array_equal(v.cpu().numpy(), g["inverse"])
    g = load_golden("segio_quantize_float.npz")
    c, i, v = la.sparse_quantize(torch.from_numpy(g["points"]).to(DEV), g["meta"]["voxel_size"], return_index=True, return_inverse=True)
    assert np.array_equal(c.cpu().numpy(), g["coords"]) and np.array_equal(i.cpu().numpy(), g["indices"]) and np.array_equal(v.cpu().numpy(), g["inverse"])
    g = load_golden("segio_quantize_block.npz")
    block = torch.from_numpy(g["block"]).to(DEV)
    labels = (torch.arange(block.shape[0]) % 19).to(DEV)
    d = la.SegVoxelizer(g["meta"]["voxel_size"])([block], [labels])
    idx = torch.from_numpy(g["indices"]).to(DEV)
    assert np.array_equal(d["lidar"].C[:, :3].cpu().numpy(), g["coords"]) and not d["lidar"].C[:, 3].any()
    assert torch.equal(d["lidar"].F, block[idx]) and torch.equal(d["targets"].F, labels[idx])
    assert np.array_equal(d["inverse_map"].F.cpu().numpy(), g["inverse"]) and np.array_equal(d["inverse_map"].C[:, :3].cpu().numpy(), g["pc"])
    assert torch.equal(d["targets_mapped"].F, labels)
    # the evaluator on the reference's two steps
    g = load_golden("segio_eval.npz")
    m = g["meta"]
    ev = la.SegEvaluator(m["num_classes"], m["ignore_label"])
    for step in range(2):
        off = np.concatenate([[0], np.cumsum(m["sizes"][step])])
        inv = (g[f"inv_local{step}"].reshape(m["votes"], m["points"]) + off[:-1, None]).astype(np.int32)
        pred = ev.update(torch.from_numpy(g[f"rows{step}"]).to(DEV), torch.from_numpy(g[f"labels{step}"]).to(DEV), torch.from_numpy(inv).to(DEV))
        cls, gap = SO.vote(g[f"rows{step}"], inv)
        sure = gap >= 1e-4
        assert (~sure).mean() <= 0.005 and np.array_equal(pred.cpu().numpy()[sure], cls[sure])
        assert np.array_equal(pred.cpu().numpy(), g[f"pred{step}"])    # ascending pass order in fp32: the reference's own sums
    r = ev.compute()
    c = m["num_classes"]
    for k, name in enumerate(("total_seen", "total_positive", "total_correct")):
        assert np.array_equal(np.stack([r["seen"], r["positive"], r["correct"]])[k, 1:], g[name][:c - 1].astype(np.int64)), name
    assert [f"mIoU: {r['miou']:.3%}", f"mAcc: {r['macc']:.3%}", f"oAcc: {r['oacc']:.3%}"] == m["printed"]
    g = load_golden("segio_ties.npz")
    ev = la.SegEvaluator(5, 0)
    pred = ev.update(torch.from_numpy(g["rows"]).to(DEV), torch.from_numpy(g["labels"]).to(DEV), torch.from_numpy(g["inverse"]).to(DEV))
    assert np.array_equal(pred.cpu().numpy(), g["pred"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("c", [2, 19, 20, 32])
def test_vote_eval(c, dtype):
    """every P and V of the issue for one (c, row type): predictions against the float64 oracle, counters against the kernel's own
    predictions, the lut, accumulation over two calls, predictions as input"""
    import link_amd as la
    lut = (torch.arange(c).flip(0) * 3 + 1).to(DEV)
    for p in (0, 1, 255, 256, 257, 5000):
        for votes in (1, 2, 3):
            rows, inverse, labels = SO.make_eval_case(p, c, votes, 100 + p + votes)
            x = torch.from_numpy(rows).to(dtype)
            cls, gap = SO.vote(x.double().numpy(), inverse)
            reached = ((inverse >= 0) & (inverse < rows.shape[0])).any(0)    # a point no pass reaches sums to zeros: class 0, exactly
            sure = (gap >= 1e-4) | ~reached if dtype == torch.float32 else np.ones(p, bool)
            share = float((~sure).mean()) if p else 0.0
            print(f"c={c} {dtype} P={p} V={votes}: left out {share:.4%}")
            assert share <= 0.005
            ev = la.SegEvaluator(c, 0)
            xd, yd, invd = x.to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(inverse).to(DEV)
            pred = ev.update(xd, yd, invd)
            got = pred.cpu().numpy()
            assert pred.dtype == torch.int64 and np.array_equal(got[sure], cls[sure]), (p, votes)
            if p:
                assert (labels == 255).any() or p < 20
            own = SO.count(got, labels, c, 0)
            assert np.array_equal(ev.counters.cpu().numpy(), own), (p, votes)
            pred2 = ev.update(xd, yd, invd, lut=lut)                  # second call: accumulates; the lut never reaches the counters
            assert torch.equal(pred2, lut[pred]) and np.array_equal(ev.counters.cpu().numpy(), 2 * own)
            ev.update(pred, yd)                                       # predictions as input
            assert np.array_equal(ev.counters.cpu().numpy(), 3 * own)
            if votes == 1 and p:
                ev.reset()
                direct = ev.update(xd, None)                          # no inverse: point p reads row p; no labels: nothing counted
                assert np.array_equal(direct.cpu().numpy(), SO.vote(x.double().numpy())[0])     # one value per class: nothing is rounded
                assert not ev.counters.any()
    # exact ties, integer-valued rows: the lowest class, in every row type
    rows, inverse, labels = SO.make_eval_case(3001, c, 3, 55, integer_ties=True)
    cls, gap = SO.vote(rows, inverse)
    assert (gap == 0).sum() > 100
    ev = la.SegEvaluator(c, 0)
    pred = ev.update(torch.from_numpy(rows).to(dtype).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(inverse).to(DEV))
    assert np.array_equal(pred.cpu().numpy(), cls)
    assert np.array_equal(ev.counters.cpu().numpy(), SO.count(cls, labels, c, 0))
    r = ev.compute()
    assert (r["miou"], r["macc"], r["oacc"]) == SO.metrics(SO.count(cls, labels, c, 0))


def test_nan_sums_never_win():
    import link_amd as la
    for c in (2, 19, 32):
        rows, want = SO.nan_case(c)
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            x = torch.from_numpy(rows).to(dtype)
            want_d = SO.vote(x.double().numpy())[0]
            assert (want_d[30:] == 0).all() and (want_d[:10] != 0).all()
            ev = la.SegEvaluator(c, 0)
            labels = torch.from_numpy(want_d).to(DEV)
            got = ev.update(x.to(DEV), labels)
            assert np.array_equal(got.cpu().numpy(), want_d), (c, dtype)
            inv = torch.arange(40, dtype=torch.int32, device=DEV).repeat(2, 1)
            assert np.array_equal(ev.update(x.to(DEV), None, inv).cpu().numpy(), SO.vote(x.double().numpy(), inv.cpu().numpy())[0])
            assert np.array_equal(ev.counters.cpu().numpy(), SO.count(want_d, want_d, c, 0))


def test_graph_replay_survives_a_larger_eager_call():
    """a captured generate_padded holds the address of its workspace: a larger eager call on the same voxeliser must not free it"""
    import link_amd as la
    vs = 0.05
    small = SO.make_block(1500, 40, vs)
    vox = la.SegVoxelizer(vs)
    static = torch.from_numpy(small).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vox.generate_padded([static])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = vox.generate_padded([static])
    first = vox._q._ws._buf[static.device]
    big = SO.make_block(40 * _tile(), 41, vs)
    _same(vox.generate_padded([torch.from_numpy(big).to(DEV)]), SO.quantize([big], voxel_size=vs), big.shape[0])
    second = vox._q._ws._buf[static.device]
    assert second is not first and second.numel() >= 2 * first.numel() and any(b is first for b in vox._q._ws._retired)
    filler = torch.full((first.numel(),), 255, dtype=torch.uint8, device=DEV)      # would land in the old buffer had it been freed
    fresh = SO.make_block(1500, 42, vs)
    static.copy_(torch.from_numpy(fresh))
    graph.replay()
    torch.cuda.synchronize()
    _same(out, SO.quantize([fresh], voxel_size=vs), 1500)
    assert int(filler.min()) == 255                                   # and the replay wrote nowhere else
    # sparse_quantize: a coordinate outside int32 raises on the device path too, with one read-back
    with pytest.raises(la._lib.LinkAmdError):
        la.sparse_quantize(torch.tensor([[0, 0, 0], [1 << 40, 0, 0]], device=DEV))
