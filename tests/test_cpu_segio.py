"""CPU-only checks of the segmentation front end and validation (csrc/segio.hip, section M of include/link_amd.h; link_amd/segio.py):
the numpy oracle of tests/segio_oracle.py against every fixture recorded from the reference's own sparse_quantize and MeanIoU
(tests/golden/make_golden_segio.py), the torch composition link_amd.segio runs off the GPU against the oracle, the aliased imports,
exports and prototypes, argument validation before anything touches a device, and a 2-rank gloo compute().

test_case_generator_properties checks the arbiter's own cases and needs nothing of link_amd; every other test here fails without
the feature (no fixtures, no link_amd.segio, no section M)."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, golden_files, load_golden

import segio_oracle as SO

FIXTURES = ["segio_eval.npz", "segio_quantize_block.npz", "segio_quantize_float.npz", "segio_quantize_int.npz", "segio_ties.npz"]


def test_fixtures_are_complete():
    assert golden_files("segio_*.npz") == FIXTURES
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20), name
    g = load_golden("segio_quantize_int.npz")
    assert np.array_equal(g["points"], SO.make_cloud(6000, 11, offset=(-37, 12, -5)))
    assert g["indices"].dtype == np.int64 and g["inverse"].dtype == np.int64 and g["coords"].dtype == np.int32


def test_case_generator_properties():
    for n in (100, 2047, 6000):
        assert SO.duplicate_share(SO.make_cloud(n, 1)) >= 0.3 and SO.make_cloud(n, 1).min() < 0
    batch = SO.make_batch([1, 2053, 700], 3)
    mins = [tuple(c.min(0)) for c in batch]
    assert len(set(mins)) == 3
    block = SO.make_block(3000, 4)
    assert SO.duplicate_share(SO.round_coords(block, 0.05)) >= 0.3 and block.dtype == np.float32 and block[:, :3].min() < 0


def _check_quantize(got, coords, indices, inverse):
    m = coords.shape[0]
    assert got["total"] == m and got["flags"] == 0
    assert np.array_equal(got["coords"][:m, :3], coords) and not got["coords"][:, 3].any() and not got["coords"][m:].any()
    assert np.array_equal(got["indices"][:m], indices) and np.array_equal(got["inverse"], inverse)
    assert np.array_equal(got["inverse_local"], inverse) and got["voxel_offsets"].tolist() == [0, m]


def test_oracle_reproduces_the_reference_quantize():
    g = load_golden("segio_quantize_int.npz")
    _check_quantize(SO.quantize([g["points"]]), g["coords"], g["indices"], g["inverse"])
    # the reference: voxels strictly ascending in (x, y, z), indices = first occurrence
    c = g["coords"].astype(np.int64)
    key = (c[:, 0] * (1 << 20) + c[:, 1]) * (1 << 20) + c[:, 2]
    assert (np.diff(key) > 0).all()
    first = np.full(c.shape[0], 1 << 30)
    np.minimum.at(first, g["inverse"], np.arange(g["inverse"].shape[0]))
    assert np.array_equal(first, g["indices"])
    g = load_golden("segio_quantize_block.npz")
    _check_quantize(SO.quantize([g["block"]], voxel_size=g["meta"]["voxel_size"]), g["coords"], g["indices"], g["inverse"])
    _check_quantize(SO.quantize([g["pc"]]), g["coords"], g["indices"], g["inverse"])
    g = load_golden("segio_quantize_float.npz")
    q = np.floor(g["points"] / g["meta"]["voxel_size"]).astype(np.int32)
    _check_quantize(SO.quantize([q]), g["coords"], g["indices"], g["inverse"])


def _global_inverse(g, step):
    m = g["meta"]
    off = np.concatenate([[0], np.cumsum(m["sizes"][step])])
    return (g[f"inv_local{step}"].reshape(m["votes"], m["points"]) + off[:-1, None]).astype(np.int32)


def _reference_counters(g):
    """MeanIoU's arrays hold class i + 1 at index i: -> int64 [3, c] = seen, positive, correct by class (class 0: not kept there)"""
    c = g["meta"]["num_classes"]
    out = np.zeros((3, c), np.int64)
    for k, name in enumerate(("total_seen", "total_positive", "total_correct")):
        out[k, 1:] = g[name][:c - 1].astype(np.int64)
    return out


def test_oracle_reproduces_the_reference_eval():
    g = load_golden("segio_eval.npz")
    m = g["meta"]
    c, ignore = m["num_classes"], m["ignore_label"]
    total = np.zeros((3, c), np.int64)
    for step in range(2):
        cls, gap = SO.vote(g[f"rows{step}"], _global_inverse(g, step))
        sure = gap >= 1e-4                                            # below it the reference's fp32 sum may choose otherwise
        assert (~sure).mean() <= 0.005 and np.array_equal(cls[sure], g[f"pred{step}"][sure])
        total += SO.count(g[f"pred{step}"], g[f"labels{step}"], c, ignore)
    ref = _reference_counters(g)
    assert np.array_equal(total[:, 1:], ref[:, 1:])                  # counters exact; class 0 is the ignored label: seen[0] == 0
    miou, macc, oacc = SO.metrics(total)
    assert [f"mIoU: {miou:.3%}", f"mAcc: {macc:.3%}", f"oAcc: {oacc:.3%}"] == m["printed"]
    g = load_golden("segio_ties.npz")
    cls, gap = SO.vote(g["rows"], g["inverse"])
    assert np.array_equal(cls, g["pred"]) and (gap == 0).sum() == g["meta"]["ties"] > 100


def test_torch_composition_equals_the_oracle_quantize():
    import link_amd as la
    from link_amd import segio
    q = segio._Quantizer()
    for sizes, seed in (([0], 0), ([1], 1), ([2], 2), ([2500], 3), ([1, 2053, 700], 4), ([0, 5, 0, 9, 0], 5)):
        clouds = SO.make_batch(sizes, seed)
        for cap in (None, 7):
            want = SO.quantize(clouds, capacity=cap)
            got = q.run([torch.from_numpy(c) for c in clouds], la._lib.SEGQ_INT, capacity=cap)
            names = ("coords", "indices", "inverse", "inverse_local", "voxel_offsets")
            for name, t in zip(names, got):
                assert t.dtype == torch.int32 and np.array_equal(t.numpy(), want[name]), (sizes, cap, name)
            assert got[5].tolist()[:2] == [want["total"], want["flags"]] and got[5].tolist()[3] == sum(sizes)
    # the rounding mode on .5 multiples of the voxel size: half to even, as np.round
    vs = 0.25
    block = torch.tensor([[0.125, -0.125, 0.375, 9.0], [0.625, -0.375, 0.875, 9.0], [0.1249, 0.0, 0.3751, 9.0]])
    got = q.run([block], la._lib.SEGQ_ROUND, vs)
    want = SO.quantize([block.numpy()], voxel_size=vs)
    assert np.array_equal(SO.round_coords(block.numpy(), vs)[:2], [[0, -0.0, 2], [2, -2, 4]])
    for name, t in zip(("coords", "indices", "inverse"), got):
        assert np.array_equal(t.numpy(), want[name]), name
    # flags: a flagged sample produces nothing, the others are not affected
    far = np.array([[0, 0, 0], [1 << 20, 1, 1]], np.int32)
    ok = SO.make_cloud(50, 6)
    got = q.run([torch.from_numpy(far), torch.from_numpy(ok)], la._lib.SEGQ_INT)
    want = SO.quantize([far, ok])
    assert want["flags"] == SO.FLAG_EXTENT and got[5].tolist()[:2] == [want["total"], SO.FLAG_EXTENT]
    assert np.array_equal(got[2].numpy(), want["inverse"]) and (got[2][:2] == -1).all() and got[4].tolist() == want["voxel_offsets"].tolist()
    nan = torch.tensor([[0.0, float("nan"), 0.0], [1.0, 1.0, 1.0]])
    assert q.run([nan], la._lib.SEGQ_ROUND, 1.0)[5].tolist()[:2] == [0, SO.FLAG_NONFINITE] == [0, SO.quantize([nan.numpy()], voxel_size=1.0)["flags"]]


def test_python_surface_against_the_fixtures():
    import link_amd as la
    g = load_golden("segio_quantize_int.npz")
    c, i, v = la.sparse_quantize(torch.from_numpy(g["points"]), return_index=True, return_inverse=True)
    assert c.dtype == torch.int32 and i.dtype == torch.int64 and v.dtype == torch.int64
    assert np.array_equal(c.numpy(), g["coords"]) and np.array_equal(i.numpy(), g["indices"]) and np.array_equal(v.numpy(), g["inverse"])
    assert np.array_equal(la.sparse_quantize(torch.from_numpy(g["points"])).numpy(), g["coords"])
    g = load_golden("segio_quantize_float.npz")
    c, i, v = la.sparse_quantize(g["points"], g["meta"]["voxel_size"], return_index=True, return_inverse=True)     # numpy in, numpy out
    assert isinstance(c, np.ndarray) and np.array_equal(c, g["coords"]) and np.array_equal(i, g["indices"]) and np.array_equal(v, g["inverse"])
    c2 = la.sparse_quantize(torch.from_numpy(g["points"]), (0.25, 0.25, 0.25))
    assert np.array_equal(c2.numpy(), g["coords"])
    # the voxeliser: what get_single_sample(use_aug=False) + sparse_collate_fn give for two frames
    g = load_golden("segio_quantize_block.npz")
    block = torch.from_numpy(g["block"])
    labels = torch.arange(block.shape[0]) % 19
    d = la.SegVoxelizer(g["meta"]["voxel_size"])([block, block[:100]], [labels, labels[:100]])
    m = g["coords"].shape[0]
    assert set(d) == {"lidar", "targets", "targets_mapped", "inverse_map"} and all(isinstance(t, la.SparseTensor) for t in d.values())
    assert np.array_equal(d["lidar"].C[:m, :3].numpy(), g["coords"]) and not d["lidar"].C[:m, 3].any() and (d["lidar"].C[m:, 3] == 1).all()
    assert d["lidar"].C.dtype == torch.int32 and torch.equal(d["lidar"].F[:m], block[torch.from_numpy(g["indices"])])
    assert torch.equal(d["targets"].F[:m], labels[torch.from_numpy(g["indices"])]) and torch.equal(d["targets"].C, d["lidar"].C)
    assert torch.equal(d["targets_mapped"].F, torch.cat([labels, labels[:100]])) and d["inverse_map"].F.dtype == torch.int64
    assert np.array_equal(d["inverse_map"].F[:block.shape[0]].numpy(), g["inverse"]) and int(d["inverse_map"].F[block.shape[0]:].min()) == 0
    assert np.array_equal(d["inverse_map"].C[:block.shape[0], :3].numpy(), g["pc"]) and (d["inverse_map"].C[block.shape[0]:, 3] == 1).all()
    for bad in (lambda: la.SegVoxelizer(0.05, num_points=80000), lambda: la.SegVoxelizer(0.05, use_aug=True)):
        with pytest.raises(NotImplementedError):
            bad()
    # the evaluator: two steps, the reference's counters and printed lines
    g = load_golden("segio_eval.npz")
    meta = g["meta"]
    ev = la.SegEvaluator(meta["num_classes"], meta["ignore_label"])
    for step in range(2):
        rows, inv = torch.from_numpy(g[f"rows{step}"]), torch.from_numpy(_global_inverse(g, step))
        pred = ev.update(rows, torch.from_numpy(g[f"labels{step}"]), inv)
        cls, gap = SO.vote(g[f"rows{step}"], inv.numpy())
        sure = gap >= 1e-4
        assert pred.dtype == torch.int64 and np.array_equal(pred.numpy()[sure], cls[sure])
        assert np.array_equal(pred.numpy(), g[f"pred{step}"])        # the same fp32 sums in the same order as the reference's
    r = ev.compute()
    ref = _reference_counters(g)
    assert np.array_equal(np.stack([r["seen"], r["positive"], r["correct"]])[:, 1:], ref[:, 1:])
    assert [f"mIoU: {r['miou']:.3%}", f"mAcc: {r['macc']:.3%}", f"oAcc: {r['oacc']:.3%}"] == meta["printed"]
    want = SO.metrics(np.stack([r["seen"], r["positive"], r["correct"]]))
    assert all(abs(a - b) <= 1e-12 for a, b in zip((r["miou"], r["macc"], r["oacc"]), want))
    ev.reset()
    assert not ev.counters.any()


@pytest.mark.parametrize("p,c,votes", [(0, 19, 1), (1, 2, 1), (257, 19, 3), (1000, 40, 2), (1000, 20, 2)])
def test_torch_composition_equals_the_oracle_eval(p, c, votes):
    """c = 40 lies outside the kernels' range: the composition is what runs for it on a GPU too"""
    import link_amd as la
    rows, inverse, labels = SO.make_eval_case(p, c, votes, 7)
    cls, gap = SO.vote(rows, inverse)
    ev = la.SegEvaluator(c, 0)
    lut = torch.arange(c).flip(0) * 10
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        x = torch.from_numpy(rows).to(dtype)
        cls_d, gap_d = SO.vote(x.double().numpy(), inverse)
        pred = ev.update(x, torch.from_numpy(labels), torch.from_numpy(inverse))
        sure = gap_d >= 1e-4 if dtype == torch.float32 else np.ones(p, bool)     # three 16-bit values sum exactly in fp32
        assert (~sure).mean() <= 0.005 if p else True
        assert np.array_equal(pred.numpy()[sure], cls_d[sure])
        before = ev.counters.clone()
        ev.reset()
        pred2 = ev.update(x, torch.from_numpy(labels), torch.from_numpy(inverse), lut=lut)
        assert torch.equal(pred2, lut[pred]) and torch.equal(ev.counters, before)
        assert np.array_equal(before.numpy(), SO.count(pred.numpy(), labels, c, 0))
        ev.reset()
    # exact ties: the lowest class; predictions as input; accumulation over two calls
    rows, inverse, labels = SO.make_eval_case(max(p, 8), c, votes, 8, integer_ties=True)
    cls, _ = SO.vote(rows, inverse)
    pred = ev.update(torch.from_numpy(rows), torch.from_numpy(labels), torch.from_numpy(inverse))
    assert np.array_equal(pred.numpy(), cls)
    ev.update(torch.from_numpy(cls), torch.from_numpy(labels))
    assert np.array_equal(ev.counters.numpy(), 2 * SO.count(cls, labels, c, 0))
    one = la.SegEvaluator(c, 0)
    assert np.array_equal(one.update(torch.from_numpy(rows[:5]), None).numpy(), SO.vote(rows[:5])[0]) and one.counters is None


def test_collate_matches_the_reference_semantics():
    import link_amd as la
    a = la.SparseTensor(torch.randn(3, 4), torch.randint(0, 9, (3, 3), dtype=torch.int32))
    b = la.SparseTensor(np.ones((2, 4), np.float32), np.zeros((2, 3), np.int32))
    out = la.sparse_collate([a, b])
    assert out.C.shape == (5, 4) and out.C.dtype == torch.int32 and out.C[:, 3].tolist() == [0, 0, 0, 1, 1] and out.F.shape == (5, 4)
    feed = la.sparse_collate_fn([{"lidar": a, "name": "f0", "t": torch.zeros(2), "a": np.ones(2), "d": {"lidar": a}},
                                 {"lidar": b, "name": "f1", "t": torch.ones(2), "a": np.zeros(2), "d": {"lidar": b}}])
    assert isinstance(feed["lidar"], la.SparseTensor) and feed["name"] == ["f0", "f1"] and feed["t"].shape == (2, 2)
    assert feed["a"].shape == (2, 2) and isinstance(feed["d"]["lidar"], la.SparseTensor)
    assert la.sparse_collate_fn([1, 2]) == [1, 2]


def test_aliased_imports_resolve():
    import link_amd as la
    la.install_as_torchsparse()
    try:
        from torchsparse.utils.quantize import sparse_quantize
        from torchsparse.utils.collate import sparse_collate, sparse_collate_fn
        import torchsparse.utils.quantize as Q
        from torchsparse.utils import make_ntuple
        assert sparse_quantize is la.sparse_quantize and sparse_collate_fn is la.sparse_collate_fn and sparse_collate is la.sparse_collate
        assert Q.sparse_quantize is la.sparse_quantize and make_ntuple is la.make_ntuple
    finally:
        for k in [k for k in sys.modules if k == "torchsparse" or k.startswith("torchsparse.")]:
            del sys.modules[k]


def test_section_m_symbols_and_version():
    from link_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in ("link_seg_quantize_workspace_bytes", "link_seg_quantize", "link_seg_vote_eval"):
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    assert L.lib().link_abi_version() == L.ABI_VERSION
    assert "M. Segmentation front end and validation" in hdr
    for k, v in (("LINK_SEGQ_INT", L.SEGQ_INT), ("LINK_SEGQ_ROUND", L.SEGQ_ROUND), ("LINK_SEGQ_SORT_TILE", L.SORT_TILE),
                 ("LINK_SEGQ_FLAG_EXTENT", L.SEGQ_FLAG_EXTENT), ("LINK_SEGQ_FLAG_NONFINITE", L.SEGQ_FLAG_NONFINITE),
                 ("LINK_SEGQ_FLAG_KEYBITS", L.SEGQ_FLAG_KEYBITS), ("LINK_SEGEVAL_ROWS", L.SEGEVAL_ROWS),
                 ("LINK_SEGEVAL_PREDICTIONS", L.SEGEVAL_PREDICTIONS), ("LINK_SEGEVAL_MAX_VOTES", L.SEGEVAL_MAX_VOTES)):
        assert f"#define {k} {v}\n" in hdr, k
    import link_amd as la
    assert la.segio.SORT_TILE == L.SORT_TILE and la.SegEvaluator is la.segio.SegEvaluator and la.SegVoxelizer is la.segio.SegVoxelizer
    from link_amd.build import SOURCES
    assert "segio.hip" in SOURCES


def test_section_m_validates_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)                                           # a non-null, aligned pointer nothing dereferences

    def quant(points=one, mode=L.SEGQ_INT, ndim=3, vs=1.0, po=one, batch=1, n=1000, ws=one, nbytes=None, coords=one, indices=one, cap=1000,
              inverse=one, local=None, voff=one, status=one):
        if nbytes is None:
            nbytes = lib.link_seg_quantize_workspace_bytes(n, batch)
        return lib.link_seg_quantize(points, mode, ndim, vs, po, batch, n, ws, nbytes, coords, indices, cap, inverse, local, voff, status, None)

    need = lib.link_seg_quantize_workspace_bytes(100000, 2)              # host arithmetic alone: no device needed
    assert 24 * 100000 <= need <= 25 * 100000 + 4096                     # 24.5 bytes per point, as the header documents
    assert lib.link_seg_quantize_workspace_bytes(0, 1) > 0
    for n, batch in ((-1, 1), (1 << 28, 1), (1 << 62, 1), (1000, 0), (1000, 1025), (1000, -1)):
        assert lib.link_seg_quantize_workspace_bytes(n, batch) == 0
        assert quant(n=n, batch=batch, nbytes=1 << 40) == L.LINK_ERR_ARG
    for kw in (dict(points=None), dict(po=None), dict(ws=None), dict(coords=None), dict(indices=None), dict(inverse=None), dict(voff=None),
               dict(status=None), dict(mode=2), dict(mode=-1), dict(cap=-1), dict(cap=1 << 28), dict(mode=L.SEGQ_ROUND, ndim=2),
               dict(mode=L.SEGQ_ROUND, ndim=17), dict(mode=L.SEGQ_ROUND, vs=0.0), dict(mode=L.SEGQ_ROUND, vs=-1.0),
               dict(mode=L.SEGQ_ROUND, vs=float("inf")), dict(mode=L.SEGQ_ROUND, vs=float("nan"))):
        assert quant(**kw) == L.LINK_ERR_ARG, kw
    need = lib.link_seg_quantize_workspace_bytes(1000, 1)
    assert quant(nbytes=need - 1) == L.LINK_ERR_WORKSPACE and quant(nbytes=0) == L.LINK_ERR_WORKSPACE

    def vote(rows=one, io=L.IO_F32, kind=L.SEGEVAL_ROWS, n_rows=500, c=19, inverse=one, votes=2, p=1000, labels=one, lut=None, pred=one,
             counters=one):
        return lib.link_seg_vote_eval(rows, io, kind, n_rows, c, inverse, votes, p, labels, 0, lut, pred, counters, None)

    for kw in (dict(c=1), dict(c=33), dict(p=-1), dict(p=1 << 31), dict(kind=2), dict(kind=-1), dict(io=3), dict(io=-1), dict(votes=0),
               dict(votes=17), dict(n_rows=-1), dict(n_rows=1 << 31), dict(counters=None), dict(rows=None), dict(inverse=None),
               dict(inverse=None, votes=1), dict(rows=None, kind=L.SEGEVAL_PREDICTIONS)):
        assert vote(**kw) == L.LINK_ERR_ARG, kw
    assert vote(p=0) == L.LINK_OK and vote(p=0, kind=L.SEGEVAL_PREDICTIONS, rows=None) == L.LINK_OK      # nothing to do: nothing launched


def test_python_surface_rejects_bad_arguments():
    import link_amd as la
    ev = la.SegEvaluator(19, 0)
    x, y = torch.randn(10, 19), torch.zeros(10, dtype=torch.int64)
    for bad in (lambda: ev.update(x[:, :5], y), lambda: ev.update(x, y[:5]), lambda: ev.update(x, y.float()), lambda: ev.update(x, y, y.float()),
                lambda: ev.update(x, y, torch.zeros(17, 10, dtype=torch.int64)), lambda: ev.update(y, y, y), lambda: ev.update(x, y, lut=y),
                lambda: la.SegEvaluator(1, 0), lambda: la.sparse_quantize(torch.zeros(5, 4)), lambda: la.SegVoxelizer(0.0),
                lambda: la.SegVoxelizer(0.05)([torch.zeros(5, 2)]), lambda: la.SegVoxelizer(0.05)([torch.zeros(5, 3)], [y])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(la._lib.LinkAmdError):
        la.sparse_quantize(torch.tensor([[0, 0, 0], [1 << 20, 0, 0]]))


# ------------------------------------------------------------------------------------------------------------ 2-rank compute()
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import link_amd as la
    rows, inverse, labels = SO.make_eval_case(2000, 19, 2, 9)
    ev = la.SegEvaluator(19, 0)
    half = slice(rank * 1000, rank * 1000 + 1000)
    ev.update(torch.from_numpy(rows), torch.from_numpy(labels[half]), torch.from_numpy(np.ascontiguousarray(inverse[:, half])))
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (calls.append(tuple(t.shape)), real(t, *a, **k))[1]
    r = ev.compute()
    dist.all_reduce = real
    local = ev.compute(all_reduce=False)
    dist.barrier()
    q.put((rank, calls, r["miou"], r["macc"], r["oacc"], r["seen"].tolist(), local["seen"].tolist()))
    dist.destroy_process_group()


def test_gloo_world2_compute_is_one_collective():
    import torch.multiprocessing as mp
    import link_amd as la
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rows, inverse, labels = SO.make_eval_case(2000, 19, 2, 9)
    ev = la.SegEvaluator(19, 0)
    ev.update(torch.from_numpy(rows), torch.from_numpy(labels), torch.from_numpy(inverse))
    one = ev.compute()
    for rank, calls, miou, macc, oacc, seen, local_seen in got:
        assert calls == [(3, 19)]                                     # exactly one collective, of the whole counter table
        assert (miou, macc, oacc) == (one["miou"], one["macc"], one["oacc"]) and seen == one["seen"].tolist()
        assert local_seen != seen and sum(local_seen) < sum(seen)


def test_nan_sums_never_win():
    import link_amd as la
    for c in (2, 19):
        rows, want = SO.nan_case(c)
        assert (want[30:] == 0).all() and (want[:10] != 0).all()         # a NaN in class 0 does not make class 0 win
        got = la.SegEvaluator(c, 0).update(torch.from_numpy(rows), None)
        assert np.array_equal(got.numpy(), want)
        inv = torch.arange(40, dtype=torch.int32).repeat(2, 1)           # two passes: NaN + x stays NaN
        assert np.array_equal(la.SegEvaluator(c, 0).update(torch.from_numpy(rows), None, inv).numpy(), SO.vote(rows, inv.numpy())[0])


def test_quantize_range_collate_inputs_and_idle_evaluator():
    import link_amd as la
    for bad in (torch.tensor([[0, 0, 0], [1 << 40, 0, 0]]), torch.tensor([[0.0, 0.0, 0.0], [3e10, 0.0, 0.0]]),
                torch.tensor([[0.0, float("nan"), 0.0]]), np.array([[0, 0, -(1 << 33)]])):
        with pytest.raises(la._lib.LinkAmdError):                        # never wrapped into int32 silently
            la.sparse_quantize(bad)
    assert la.sparse_quantize(torch.tensor([[1 << 40, 0, 0]]), 1 << 30).tolist() == [[0, 0, 0]]      # in range after the divide
    for vs in (0, -1.0, (1, 2), float("nan")):
        with pytest.raises(ValueError):
            la.sparse_quantize(torch.zeros(3, 3), vs)
    coords, feats = np.zeros((2, 3), np.int32), np.ones((2, 4), np.float32)
    x = la.SparseTensor(feats, coords)
    out = la.sparse_collate([x, x])
    assert x.coords is coords and x.feats is feats and out.C[:, 3].tolist() == [0, 0, 1, 1]          # the inputs stay as they were
    with pytest.raises(ValueError):
        la.sparse_collate([la.SparseTensor(torch.zeros(1, 1), torch.zeros(1, 3, dtype=torch.int32), 1),
                           la.SparseTensor(torch.zeros(1, 1), torch.zeros(1, 3, dtype=torch.int32), 2)])
    with pytest.raises(ValueError):
        la.sparse_collate([])
    # an evaluator that never saw a step: zeros, every class unseen; with `device` the counters exist from the start
    r = la.SegEvaluator(5, 0).compute()
    assert r["miou"] == 1.0 and not r["seen"].any()
    ev = la.SegEvaluator(5, 0, device="cpu")
    assert ev.counters.shape == (3, 5) and ev.counters.device.type == "cpu" and ev.compute()["macc"] == 1.0
