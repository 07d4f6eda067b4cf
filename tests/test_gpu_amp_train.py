"""Autocast training (include/link_amd.h, ABI 13): fp16 / bf16 feature rows with grad on the hand-written training kernels.

The rule every 16-bit path follows: the rows are read and written in their type at the kernel boundary only, everything in
between is fp32 -- so each result is, bit for bit, the fp32 path's result on the rows widened to fp32, rounded once into the
row type.  The convolutions follow the reference's custom_fwd(cast_inputs=torch.half) under torch.autocast
(torchsparse/nn/functional/conv.py:19): fp16 rows in and out, on the AMP kernels."""
import copy

import numpy as np
import pytest
import torch

import grad64 as G
from helpers import lidar_like, rel_err, s_uniform

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
TOL_ORACLE = {torch.float16: 6e-3, torch.bfloat16: 5e-2}     # the half-row tolerances of test_gpu_dense.py::test_dense_half_rows


def _params(C, cg, baseop, seed):
    g = torch.Generator().manual_seed(seed)
    p = {
        "w_pre": torch.randn(C, C, generator=g) / C ** 0.5,
        "pre_ln_w": 1 + 0.1 * torch.randn(C, generator=g), "pre_ln_b": 0.1 * torch.randn(C, generator=g),
        "w_pos": 0.3 * torch.randn(cg, 3, generator=g),
        "alpha": (1 + 0.2 * torch.randn(1, cg, generator=g)) if baseop == "cos_x" else None,
        "ln_w": 1 + 0.1 * torch.randn(C, generator=g), "ln_b": 0.1 * torch.randn(C, generator=g),
    }
    return {k: (v.cuda().requires_grad_(True) if v is not None else None) for k, v in p.items()}


def _run(fn, feats, coords, index, p, baseop, cg, r, div, gout):
    f = feats.detach().clone().requires_grad_(True)
    q = {k: (v.detach().clone().requires_grad_(True) if v is not None else None) for k, v in p.items()}
    out = fn(f, coords, index, q["w_pre"], q["pre_ln_w"], q["pre_ln_b"], q["w_pos"], q["alpha"], q["ln_w"],
             q["ln_b"], baseop, cg, r, div, 1e-6)
    out.backward(gout)
    grads = {"feats": f.grad}
    grads.update({k: v.grad for k, v in q.items() if v is not None})
    return out.detach(), grads


CORE_CASES = [
    # C, groups, baseop, s, r, div, frame
    (64, 2, "cos", 7, 3, 1.0, "uniform"),
    (64, 2, "sin", 7, 3, 1.0, "uniform"),
    (64, 1, "cos_x", 3, 2, 1.0, "uniform"),
    (64, 1, "cos_x", 6, 2, 2.0, "uniform"),
    (32, 1, "cos", 7, 3, 1.0, "uniform"),
    (128, 2, "cos", 7, 3, 1.0, "uniform"),
    (64, 2, "cos", 14, 3, 1.0, "lidar"),
]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("C,groups,baseop,s,r,div,frame", CORE_CASES)
def test_core_train_half_rows_bit_equal_to_widened_fp32(dtype, C, groups, baseop, s, r, div, frame):
    import link_amd as la
    from link_amd.elk import elk_core_train
    if frame == "uniform":
        coords = s_uniform(6000, grid=64, seed=5)
        if div != 1.0:
            coords[:, :3] *= int(div)
    else:
        coords = torch.from_numpy(lidar_like(20000, seed=3))
    coords = coords.cuda()
    n = coords.shape[0]
    cg = C // groups
    p = _params(C, cg, baseop, seed=11)
    f16 = torch.randn(n, C, generator=torch.Generator().manual_seed(7)).to(dtype).cuda()
    gout = torch.randn(n, C, generator=torch.Generator().manual_seed(8)).cuda()
    index = la.BlockIndex(coords, s)
    o16, g16 = _run(elk_core_train, f16, coords, index, p, baseop, cg, r, div, gout)
    o32, g32 = _run(elk_core_train, f16.float(), coords, index, p, baseop, cg, r, div, gout)
    assert o16.dtype == torch.float32 and torch.equal(o16, o32)
    assert g16["feats"].dtype == dtype and torch.equal(g16["feats"], g32["feats"].to(dtype))
    for k in g32:
        if k != "feats":
            assert g16[k].dtype == torch.float32 and torch.equal(g16[k], g32[k]), k
    # the float64 reference on the widened rows and its fp32 yardstick (tests/grad64.py; shared with test_gpu_train_gate.py)
    key = (frame, 6000 if frame == "uniform" else 20000, C, groups, baseop, s, r, div, str(dtype))
    g64, o32 = G.cached_yardstick(key, lambda: (f16, coords, p, s, r, baseop, groups, div, gout))
    case = dict(suite="half_rows_bit_equal", C=C, groups=groups, op=baseop, s=s, r=r, n=n, div=div, rows=str(dtype)[6:])
    rows = G.measure(case, g64, o32, dict(g16, out=o16), G.rounding_cost(g64, dtype))
    tol = TOL_ORACLE[dtype]
    assert rel_err(o16.cpu().numpy(), g64["out"].numpy()) < tol
    for k in g64:
        if k != "out":
            assert rel_err(g16[k].float().cpu().numpy(), g64[k].numpy()) < tol, k
    bad = [row for row in rows if not row["ok"]]
    assert not bad, bad


@pytest.mark.parametrize("dtype", HALF)
def test_tail_half_rows_bit_equal_to_widened_fp32(dtype):
    from link_amd.elk import _Tail
    n, C = 7001, 64
    g = torch.Generator().manual_seed(3)
    x16 = torch.randn(n, C, generator=g).to(dtype).cuda()
    add = torch.randn(n, C, generator=g).cuda()
    w, b = (1 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    gout = torch.randn(n, C, generator=g).cuda()

    def run(x):
        xs, a = x.clone().requires_grad_(True), add.clone().requires_grad_(True)
        ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = _Tail.apply(xs, a, ws, bs, 1e-6)
        y.backward(gout)
        return y.detach(), xs.grad, a.grad, ws.grad, bs.grad

    y16, gx16, ga16, gw16, gb16 = run(x16)
    y32, gx32, ga32, gw32, gb32 = run(x16.float())
    assert y16.dtype == torch.float32 and torch.equal(y16, y32), int((y16 != y32).sum())
    assert gx16.dtype == dtype
    bad = gx16 != gx32.to(dtype)
    assert not bad.any(), (int(bad.sum()), gx16[bad][:4].tolist(), gx32[bad][:4].tolist())
    for nm, a_, b_ in (("g_addend", ga16, ga32), ("ln_w", gw16, gw32), ("ln_b", gb16, gb32)):
        assert a_.dtype == torch.float32 and torch.equal(a_, b_), (nm, int((a_ != b_).sum()))


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_half_rows_bit_equal_to_widened_fp32(dtype, relu, monkeypatch):
    import link_amd as la
    n, C = 9003, 64
    g = torch.Generator().manual_seed(4)
    x16 = (0.5 + 2 * torch.randn(n, C, generator=g)).to(dtype).cuda()
    coords = s_uniform(n, grid=64, seed=1).cuda()
    gout16 = torch.randn(n, C, generator=g).to(dtype).cuda()
    torch.manual_seed(0)
    bn = la.BatchNorm(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    bn32 = copy.deepcopy(bn)
    calls = []
    orig = torch.nn.functional.batch_norm
    monkeypatch.setattr(torch.nn.functional, "batch_norm", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])

    def run(m, x, go):
        xs = x.clone().requires_grad_(True)
        y = m(la.SparseTensor(xs, coords, 1), relu=relu).F
        m.zero_grad()
        y.backward(go)
        return y.detach(), xs.grad, m.weight.grad.clone(), m.bias.grad.clone()

    y16, gx16, gw16, gb16 = run(bn, x16, gout16)
    y32, gx32, gw32, gb32 = run(bn32, x16.float(), gout16.float())
    assert not calls                                       # torch's batch_norm never ran
    assert y16.dtype == dtype and torch.equal(y16, y32.to(dtype))
    assert gx16.dtype == dtype and torch.equal(gx16, gx32.to(dtype))
    assert torch.equal(gw16, gw32) and torch.equal(gb16, gb32)
    assert torch.equal(bn.running_mean, bn32.running_mean) and torch.equal(bn.running_var, bn32.running_var)
    assert bn.running_mean.dtype == torch.float32
    # the training-mode fused Conv-BN-ReLU container routes 16-bit rows the same way
    if relu:
        seq = la.fuse_for_inference(torch.nn.Sequential(la.Conv3d(C, C, 3), copy.deepcopy(bn), la.ReLU(True))).cuda().train()
        with torch.autocast("cuda", torch.float16):
            out = seq(la.SparseTensor(x16.float().requires_grad_(True), coords, 1))
        out.F.float().sum().backward()
        assert out.F.dtype == torch.float16 and not calls


def _conv_frame():
    coords = torch.from_numpy(lidar_like(8000, seed=6, voxel=0.2))
    feats = torch.randn(coords.shape[0], 64, generator=torch.Generator().manual_seed(5))
    return coords, feats


def test_conv_under_autocast_fp16_rows_and_input_gradient():
    import link_amd as la
    from link_amd import elk as E
    from oracle import link_oracle as lo
    coords, feats = _conv_frame()
    n = coords.shape[0]
    torch.manual_seed(1)
    c1 = la.Conv3d(64, 64, 3).cuda()
    c2 = la.Conv3d(64, 64, 2, stride=2).cuda()
    c3 = la.Conv3d(64, 64, 2, stride=2, transposed=True).cuda()

    def chain(x, region):
        outs = []
        for m in (c1, c2, c3):
            with region():
                x = m(x)
            outs.append(x)
        return outs

    def fresh(f):
        x = la.SparseTensor(f, coords.cuda(), 1)
        x.cmaps.setdefault(x.stride, x.coords)
        return x

    class Off:
        def __enter__(self): return None
        def __exit__(self, *a): return False

    with torch.no_grad():
        ref16 = chain(fresh(feats.half().cuda()), Off)             # the modules on fp16 rows outside autocast
        for adt in (torch.float16, torch.bfloat16):
            got = chain(fresh(feats.cuda()), lambda: torch.autocast("cuda", adt))
            for a, b in zip(got, ref16):
                assert a.F.dtype == torch.float16 and torch.equal(a.F, b.F), adt
        # outside autocast: fp32 rows stay on today's fp32 path
        x = fresh(feats.cuda())
        y = c1(x)
        nbr, order = c1._neighbor_table(x)
        assert y.F.dtype == torch.float32 and torch.equal(y.F, E.subm_conv(feats.cuda(), c1.kernel, nbr, order))

    # input gradient per layer: fp16, within the half tolerance of the fp64 definition; kernel gradient fp32
    kr = [c.kernel.detach().cpu().double() for c in (c1, c2, c3)]
    cc = lo.downsample_coords(coords.numpy(), 2, 1)
    down = lo.strided_conv_table(coords.numpy(), cc, 2, 1)
    g = torch.Generator().manual_seed(9)
    x = fresh(feats.half().cuda())
    with torch.no_grad():
        y1, y2, _ = chain(x, Off)
    for layer, src in ((c1, x), (c2, y1), (c3, y2)):
        f = src.F.detach().clone().requires_grad_(True)
        st = la.SparseTensor(f, src.C, src.s)
        st.cmaps, st.kmaps = src.cmaps, src.kmaps
        layer.zero_grad()
        with torch.autocast("cuda", torch.float16):
            out = layer(st)
        gout = torch.randn(out.F.shape, generator=g).half()
        out.F.backward(gout.cuda())
        assert f.grad.dtype == torch.float16 and layer.kernel.grad.dtype == torch.float32
        fr = f.detach().cpu().double().requires_grad_(True)
        if layer is c1:
            r = lo.subm_conv_torch(fr, coords, kr[0], 1)
        elif layer is c2:
            r = lo.gather_conv_torch(fr, down, kr[1])
        else:
            r = lo.gather_conv_torch(fr, None, kr[2], n_out=n, transposed_of=down)
        r.backward(gout.double())
        assert rel_err(f.grad.float().cpu().numpy(), fr.grad.numpy()) < TOL_ORACLE[torch.float16]


def _spy(monkeypatch, owner, name, log, static=True):
    orig = getattr(owner, name)

    def spy(*a, **k):
        log.append(name)
        return orig(*a, **k)
    monkeypatch.setattr(owner, name, staticmethod(spy) if static else spy)


def test_elkblock_under_autocast_routes_to_training_kernels(monkeypatch):
    import link_amd as la
    from link_amd import elk as E
    coords = s_uniform(20000, grid=96, seed=2).cuda()
    torch.manual_seed(0)
    blk = la.ELKBlock(64, 64, groups=2, baseop="cos").cuda().train()
    feats = torch.randn(20000, 64, generator=torch.Generator().manual_seed(1)).half().cuda()
    log = []
    _spy(monkeypatch, E._ElkCoreTrain, "forward", log)
    _spy(monkeypatch, E._Tail, "forward", log)
    _spy(monkeypatch, E, "elk_core_autograd", log, static=False)

    def run():
        f = feats.clone().requires_grad_(True)
        blk.zero_grad()
        with torch.autocast("cuda", torch.float16):
            out = blk(la.SparseTensor(f, coords, 1), 7, 3).F
        out.square().sum().backward()
        return [out.detach().clone(), f.grad.clone()] + [p.grad.clone() for p in blk.parameters()]

    a = run()
    assert log == ["forward", "forward"] and "elk_core_autograd" not in log
    assert a[1].dtype == torch.float16
    b = run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_overflow_in_upstream_gradient_reaches_gradscaler():
    import link_amd as la
    coords = s_uniform(6000, grid=64, seed=4).cuda()
    torch.manual_seed(0)
    blk = la.ELKBlock(64, 64, groups=1, baseop="cos_x").cuda().train()
    before = [p.detach().clone() for p in blk.parameters()]
    opt = torch.optim.SGD(blk.parameters(), lr=0.1)
    scaler = torch.amp.GradScaler("cuda")
    f = torch.randn(6000, 64, generator=torch.Generator().manual_seed(2)).half().cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.float16):
        out = blk(la.SparseTensor(f, coords, 1), 3, 2).F
    gout = torch.ones_like(out)
    gout.view(-1)[int(out.argmax())] = float("inf")        # where the ReLU passes the gradient
    scaler.scale((out * gout).sum()).backward()
    assert not torch.isfinite(f.grad.float()).all()
    scaler.step(opt)
    scaler.update()
    for p, q in zip(blk.parameters(), before):
        assert torch.equal(p.detach(), q)                   # the step was skipped
    assert scaler.get_scale() < 65536.0


def test_unet_autocast_step_vs_fp32_step(monkeypatch):
    import link_amd as la
    from link_amd import elk as E
    from link_amd import synth
    from harness.networks import build_reference_shaped_unet
    coords, feats = synth.s_kitti(0, n_az=512)
    coords, feats = torch.from_numpy(coords).cuda(), torch.from_numpy(feats).cuda()
    labels = torch.randint(0, 19, (coords.shape[0],), generator=torch.Generator().manual_seed(3)).cuda()
    torch.manual_seed(0)
    net32 = build_reference_shaped_unet(la, cr=1.0, baseop="cos_x", groups=1, s=3, r=2, num_classes=19).cuda().train()
    net16 = copy.deepcopy(net32)

    def step(net, amp):
        opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
        scaler = torch.amp.GradScaler("cuda", enabled=amp)
        opt.zero_grad()
        with torch.autocast("cuda", torch.float16, enabled=amp):
            logits = net(la.SparseTensor(feats, coords, 1))
            loss = torch.nn.functional.cross_entropy(logits, labels)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        scaler.step(opt)
        scaler.update()
        return float(loss.detach()), grads

    net_t = copy.deepcopy(net32)
    loss32, g32 = step(net32, False)
    la.BatchNorm.hip_stats = False                          # control: the same autocast step with torch's batch_norm
    try:
        _, gt = step(net_t, True)
    finally:
        la.BatchNorm.hip_stats = True
    log, rows = [], []
    orig_bn = torch.nn.functional.batch_norm
    monkeypatch.setattr(torch.nn.functional, "batch_norm", lambda *a, **k: (log.append("batch_norm"), orig_bn(*a, **k))[1])
    _spy(monkeypatch, E._ElkCoreTrain, "forward", log)
    _spy(monkeypatch, E._Tail, "forward", log)
    _spy(monkeypatch, E, "elk_core_autograd", log, static=False)
    for i in (1, 2, 3, 4):
        getattr(net16, f"elk{i}").register_forward_pre_hook(lambda m, args: rows.append(args[0].F.dtype))
    loss16, g16 = step(net16, True)
    assert np.isfinite(loss16)
    assert rows == [torch.float16] * 4
    assert "batch_norm" not in log and "elk_core_autograd" not in log
    assert log.count("forward") == 8                        # four blocks: _ElkCoreTrain + _Tail each
    assert set(g16) == set(g32) == set(gt)

    def rel(a, b):
        return float((a.float() - b).norm() / max(float(b.norm()), 1e-12))
    e16 = np.array([rel(g16[k], g32[k]) for k in g32])
    et = np.array([rel(gt[k], g32[k]) for k in g32])
    print(f"unet autocast step: loss fp32 {loss32:.6f} fp16 {loss16:.6f}; parameter-gradient rel L2 vs fp32: median "
          f"{np.median(e16):.3e} worst {e16.max():.3e} (torch batch_norm under the same autocast: {np.median(et):.3e} / {et.max():.3e})")
    # Measured: fp16 autocast moves this network's parameter gradients at initialisation by a median 0.16 and at
    # most 0.28 relative L2 from the fp32 step -- torch's own batch_norm under the same autocast: 0.15 / 0.23.  The 3e-2 of the
    # first estimate does not hold for fp16 AMP itself; the bounds are the measurement with a 2x margin, and the native
    # kernels may not be worse than the torch path under the same autocast.
    assert np.median(e16) < 0.32 and e16.max() < 0.6
    assert np.median(e16) < 1.5 * np.median(et) and e16.max() < 2.0 * et.max()
