"""The fused segmentation criterion on the GPU (csrc/segloss.hip, section K of include/link_amd.h; link_amd/segloss.py) against the
float64 oracle of tests/segloss_oracle.py.

The gate is the project's (tests/grad64.py): for the loss, CE, Lovasz and the gradient rows outside the ambiguity mask,
rel_err(got, g64) <= 4 * o32 + 2 * o_round + 2e-6, o32 the oracle's own fp32 evaluation against float64 under the same mask and
o_round what storing the float64 gradient in the row type costs (gradient only).  Nothing in the bound comes from the kernels.
Every case prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import segloss_oracle as SO
from helpers import load_golden, rel_err

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 2e-6
SWEEP = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


def _fused(rows, labels, crit=None, upstream=None, **kw):
    """{"total", "ce", "lovasz", "grad"} of SegCriterion on the GPU (grad in the row type)"""
    import link_amd as la
    crit = crit or la.SegCriterion(**kw)
    x = rows.cuda().requires_grad_(True)
    total = crit(x, labels.cuda())
    if upstream is None:
        total.backward()
    else:
        total.backward(upstream)
    return {"total": total.detach(), "ce": crit.last_ce, "lovasz": crit.last_lovasz, "grad": x.grad}


def _gate(case, got, r64, o32, mask, o_round=0.0, scalars=("total", "ce", "lovasz")):
    keep = (~mask).numpy()
    rows = []
    for k in scalars:
        rows.append((k, rel_err(float(got[k]), float(r64[k])), FACTOR * o32[k] + FLOOR, bool(np.isfinite(float(got[k])))))
    g = got["grad"].detach().float().cpu().numpy()
    assert g.shape == tuple(r64["grad"].shape)
    rows.append(("grad", rel_err(g[keep], r64["grad"].numpy()[keep]), FACTOR * o32["grad"] + 2.0 * o_round + FLOOR, bool(np.isfinite(g).all())))
    for k, e, bound, finite in rows:
        print(f"{case} {k}: e {e:.3e} bound {bound:.3e} o32 {o32[k]:.3e} masked {float(mask.float().mean()):.4f}")
    assert float(mask.float().mean()) <= SO.MASK_CAP
    bad = [r for r in rows if not (r[3] and r[1] <= r[2])]
    assert not bad, f"{case}: {bad}"


def _o_round(r64, mask, dtype, scale=1.0):
    if dtype == torch.float32:
        return 0.0
    g = r64["grad"][~mask]
    return rel_err(((g * scale).to(dtype).double() / scale).numpy(), g.numpy())


def _case(n, C, dtype=torch.float32, scale=3.0, **kw):
    x, y = SO.make_case(n, C, 1, scale)
    x = x.to(dtype)
    key = (n, C, str(dtype), scale, tuple(sorted(kw.items())))
    return (x, y) + SO.yardstick(key, x, y, **kw)


@pytest.mark.parametrize("n", SWEEP)
def test_tile_and_chunk_edges(n):
    x, y, r64, o32, mask = _case(n, 3)
    _gate(f"({n}, 3)", _fused(x, y), r64, o32, mask)
    if n <= 65:                                   # so few rows that ignore=0 leaves next to nothing: nothing ignored as well
        x, y, r64, o32, mask = _case(n, 3, lov_ignore=None)
        _gate(f"({n}, 3) ignore None", _fused(x, y, lovasz_ignore=None), r64, o32, mask)


@pytest.mark.parametrize("n,C,dtype,scale", [(777, 5, torch.float32, 3.0), (20011, 19, torch.float32, 2.0)] +
                         [(3000, C, d, 3.0) for C in (19, 17) for d in (torch.float32, torch.float16, torch.bfloat16)])
def test_shapes_and_row_types(n, C, dtype, scale):
    x, y, r64, o32, mask = _case(n, C, dtype, scale)
    got = _fused(x, y)
    assert got["grad"].dtype == dtype and got["total"].dtype == torch.float32
    _gate(f"({n}, {C}) {dtype}", got, r64, o32, mask, _o_round(r64, mask, dtype))


def test_classes_all_with_an_absent_class_and_a_single_row_class():
    x, y, r64, o32, mask = _case(3000, 19, classes="all")
    counts = torch.bincount(y[y < 19], minlength=19)
    assert counts[18] == 0 and counts[17] == 1
    _gate("(3000, 19) all", _fused(x, y, classes="all"), r64, o32, mask)
    x, y, r64, o32, mask = _case(777, 5, classes="all", lov_ignore=None)
    _gate("(777, 5) all, ignore None", _fused(x, y, classes="all", lovasz_ignore=None), r64, o32, mask)


def test_every_row_ignored_and_every_label_255():
    x, _ = SO.make_case(300, 5, 2)
    zeros = torch.zeros(300, dtype=torch.int64)
    got = _fused(x, zeros)                                              # every row ignored by Lovasz: CE alone
    xr = x.clone().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(xr.double(), zeros)
    ce.backward()
    assert float(got["lovasz"]) == 0.0
    assert rel_err(float(got["total"]), float(ce.detach())) <= FLOOR and rel_err(got["grad"].cpu().numpy(), xr.grad.numpy()) <= FLOOR
    got = _fused(x, torch.full((300,), 255))                            # valid for Lovasz, background for every class; no CE row
    assert float(got["lovasz"]) == 0.0
    want = torch.nn.functional.cross_entropy(x, torch.full((300,), 255), ignore_index=255)
    assert bool(torch.isnan(want)) == bool(torch.isnan(got["ce"].cpu()))          # CE as torch returns it
    assert float(got["grad"].abs().max()) == 0.0


def test_exact_ties_keep_row_order():
    x = torch.zeros(64, 2)
    x[32:] = SO.make_case(32, 2, 3)[0]
    y = (torch.arange(64) % 2).long()
    r64 = SO.reference(x, y, lov_ignore=None)
    r32 = SO.reference(x, y, lov_ignore=None, dtype=torch.float32)
    assert float(torch.softmax(x[:32], 1).sub(0.5).abs().max()) == 0.0
    o32 = {k: rel_err(float(r32[k]), float(r64[k])) for k in ("total", "ce", "lovasz")}
    o32["grad"] = rel_err(r32["grad"].numpy(), r64["grad"].numpy())
    _gate("ties", _fused(x, y, lovasz_ignore=None), r64, o32, torch.zeros(64, dtype=torch.bool))


def test_probabilities_and_the_reference_signatures():
    import link_amd as la
    g = load_golden("segloss_4d.npz")
    p, lab = torch.from_numpy(g["probas"]), torch.from_numpy(g["labels"])
    flat = p.permute(0, 2, 3, 1).reshape(-1, 5)
    r64, o32, mask = SO.yardstick("4d", flat, lab.reshape(-1), lov_ignore=0, kind="probas")
    pg = p.cuda().requires_grad_(True)
    loss = la.lovasz_softmax(pg, lab.cuda(), ignore=0)
    loss.backward()
    got = {"lovasz": loss.detach(), "grad": pg.grad.permute(0, 2, 3, 1).reshape(-1, 5)}
    _gate("4d", got, r64, o32, mask, scalars=("lovasz",))
    assert abs(float(loss) - g["meta"]["per_image_False"]) <= 1e-6
    pg = p.cuda().requires_grad_(True)
    loss = la.lovasz_softmax(pg, lab.cuda(), per_image=True, ignore=0)
    loss.backward()
    per = [SO.yardstick(f"4d{b}", flat[b * 192:(b + 1) * 192], lab[b].reshape(-1), lov_ignore=0, kind="probas") for b in range(2)]
    want = sum(float(q[0]["lovasz"]) for q in per) / 2
    assert rel_err(float(loss), want) <= FACTOR * max(q[1]["lovasz"] for q in per) + FLOOR
    assert abs(float(loss) - g["meta"]["per_image_True"]) <= 1e-6
    for b in range(2):
        gb = pg.grad[b].permute(1, 2, 0).reshape(-1, 5).cpu().numpy() * 2
        keep = (~per[b][2]).numpy()
        assert rel_err(gb[keep], per[b][0]["grad"].numpy()[keep]) <= FACTOR * per[b][1]["grad"] + FLOOR
    x, y = SO.make_case(777, 5, 1)                                       # the flat form, nothing ignored
    x = torch.softmax(x, 1)
    r64, o32, mask = SO.yardstick("flat777", x, y, lov_ignore=None, kind="probas")
    xg = x.cuda().requires_grad_(True)
    loss = la.lovasz_softmax_flat(xg, y.cuda())
    loss.backward()
    _gate("flat", {"lovasz": loss.detach(), "grad": xg.grad}, r64, o32, mask, scalars=("lovasz",))


def test_two_calls_are_bit_identical():
    import link_amd as la
    x, y = SO.make_case(20011, 19, 1, 2.0)
    crit = la.SegCriterion()
    a = _fused(x, y, crit)
    b = _fused(x, y, crit)
    c = _fused(x, y)                                                       # another workspace
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_forward_and_backward_capture_in_a_graph():
    """No host round trip: forward + backward on static buffers captured on one stream, replayed on a second seeded input, equal
    eager bit for bit."""
    import link_amd as la
    x1, y1 = SO.make_case(3000, 19, 1)
    x2, y2 = SO.make_case(3000, 19, 2)
    crit = la.SegCriterion()
    xs, ys = x1.cuda().requires_grad_(True), y1.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(crit(xs, ys), xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = crit(xs, ys)
        ce_s, lov_s = crit.last_ce, crit.last_lovasz
        (grad_s,) = torch.autograd.grad(loss_s, xs)
    with torch.no_grad():
        xs.copy_(x2)
        ys.copy_(y2)
    graph.replay()
    torch.cuda.synchronize()
    eager = _fused(x2, y2)
    assert torch.equal(loss_s, eager["total"]) and torch.equal(ce_s, eager["ce"]) and torch.equal(lov_s, eager["lovasz"])
    assert torch.equal(grad_s, eager["grad"])
    r64 = SO.reference(x2, y2)
    assert rel_err(float(loss_s), float(r64["total"])) <= 1e-5          # the replay computed the second input, not the first


def test_autocast_and_gradscaler():
    import link_amd as la
    x, y, r64, o32, mask = _case(3000, 19, torch.float16)
    crit = la.SegCriterion()
    scale = 65536.0

    def step(rows16):
        w = rows16.float().cuda().requires_grad_(True)
        opt = torch.optim.SGD([w], lr=0.1)
        scaler = torch.amp.GradScaler("cuda", init_scale=scale)
        with torch.autocast("cuda", torch.float16):
            logits = w.half()
            logits.retain_grad()
            loss = crit(logits, y.cuda())
        scaler.scale(loss).backward()
        before = w.detach().clone()
        scaler.step(opt)
        scaler.update()
        return loss.detach(), logits.grad, before, w.detach(), scaler.get_scale()

    loss, grad16, before, after, s = step(x)
    assert loss.dtype == torch.float32 and grad16.dtype == torch.float16 and s == scale
    assert not torch.equal(before, after)
    got = {"total": loss, "ce": crit.last_ce, "lovasz": crit.last_lovasz, "grad": grad16.float() / scale}
    _gate("amp fp16", got, r64, o32, mask, _o_round(r64, mask, torch.float16, scale))
    xi = x.clone()
    xi[17, 3] = float("inf")
    loss, grad16, before, after, s = step(xi)
    assert not bool(torch.isfinite(loss))
    assert torch.equal(before, after) and s < scale                       # the scaler skipped the step


def test_one_network_step_against_the_torch_composition():
    """SegCriterion and the torch composition of the same formula under one UNet (cr = 0.25, 19 classes, 2 000 voxels).  Both the
    loss and the classifier's weight gradient dW = g^T x of each are held to the plain gate against float64: the oracle's g64 on the
    logits the criterion was given, times the classifier's input x (captured) in float64; o32 of dW is what g32^T x costs in fp32,
    the larger of the rows as given and in a seeded permutation (the order of an fp32 sum moves it, tests/grad64.py).  Rows under the
    ambiguity mask are taken out of both sides (the run's own logit gradient of those rows times x, subtracted in float64)."""
    import link_amd as la
    from link_amd.segloss import _torch_criterion
    from harness.networks import build_reference_shaped_unet
    g = load_golden("g_unet_cosx_s3_r2.npz")
    n = 2000
    feats, coords = torch.from_numpy(g["feats"][:n]).cuda(), torch.from_numpy(g["coords"][:n]).cuda()
    labels = SO.make_case(n, 19, 5)[1]
    net = build_reference_shaped_unet(la, cr=0.25, baseop="cos_x", groups=1, s=3, r=2, num_classes=19)
    net.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd::")}, strict=True)
    net = net.cuda().train()
    lin = net.classifier[0]
    seen = {}
    lin.register_forward_hook(lambda m, a, out: seen.update(x=a[0].detach()))
    crit = la.SegCriterion()
    res = {}
    for name in ("fused", "torch"):
        net.zero_grad()
        logits = net(la.SparseTensor(feats, coords, 1))
        logits.retain_grad()
        loss = crit(logits, labels.cuda()) if name == "fused" else _torch_criterion(logits, labels.cuda(), 255, 0, "present")[0]
        loss.backward()
        res[name] = {"loss": loss.detach().cpu(), "dW": lin.weight.grad.detach().double().cpu(), "logits": logits.detach().cpu(),
                     "g": logits.grad.double().cpu(), "x": seen["x"].double().cpu()}
    assert torch.equal(res["fused"]["logits"], res["torch"]["logits"])   # the same logits reached both criteria
    logits, x = res["torch"]["logits"], res["torch"]["x"]
    r64, o32, mask = SO.yardstick("unet", logits, labels)
    keep = ~mask
    assert float(mask.float().mean()) <= SO.MASK_CAP
    g32 = SO.reference(logits, labels, dtype=torch.float32)["grad"]
    dw64 = r64["grad"][keep].T @ x[keep]
    perm = torch.randperm(int(keep.sum()), generator=torch.Generator().manual_seed(1000))
    a, b = g32[keep], x[keep].float()
    o32_dw = max(rel_err((a.T @ b).numpy(), dw64.numpy()), rel_err((a[perm].T @ b[perm]).numpy(), dw64.numpy()))
    for name, r in res.items():
        e = rel_err(float(r["loss"]), float(r64["total"]))
        print(f"unet step {name}: loss e {e:.3e} bound {FACTOR * o32['total'] + FLOOR:.3e}")
        assert e <= FACTOR * o32["total"] + FLOOR
        dw = r["dW"] - r["g"][mask].T @ x[mask]
        e = rel_err(dw.numpy(), dw64.numpy())
        print(f"unet step {name}: classifier dW e {e:.3e} bound {FACTOR * o32_dw + FLOOR:.3e} o32 {o32_dw:.3e} masked {float(mask.float().mean()):.4f}")
        assert e <= FACTOR * o32_dw + FLOOR
