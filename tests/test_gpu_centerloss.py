"""CenterHead training on the GPU (csrc/centerloss.hip, section L of include/link_amd.h; link_amd/centerloss.py) against the oracle of
tests/centerloss_oracle.py.

Targets: ind / mask / cat, the zero cells of the heat map and the plain-fp32 columns EQUAL the oracle's; heat-map values and the
log / sin / cos columns lie within 1 fp32 ulp of the oracle's float64 value rounded to fp32 (a float64 function within one double ulp,
rounded once, lands at most one fp32 ulp from the correctly rounded value).
Loss and gradients: the project's gate (tests/grad64.py), rel_err(got, g64) <= 4 * o32 + 2 * o_round + 2e-6 per scalar and per
gradient tensor, o32 the oracle's own fp32 evaluation against float64 and o_round what storing the float64 gradient in the row type
costs.  Nothing in the bound comes from the kernels.  Every case prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import centerloss_oracle as CO
from helpers import rel_err

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 2e-6
SWEEP = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
NUSC = (1, 2, 2, 1, 2, 2)
CW10 = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]


def _assigner(tasks, W, H, max_objs):
    import link_amd as la
    return la.CenterTargetAssigner(tasks, CO.OSF, CO.VS, CO.geometry(W, H), CO.OVERLAP, max_objs, CO.MIN_RADIUS)


def _assigned(boxes, classes, tasks, W, H, max_objs):
    ex = _assigner(tasks, W, H, max_objs)(torch.from_numpy(boxes).cuda(), torch.from_numpy(classes).cuda())
    return [{k: ex[k][t].cpu().numpy() for k in ex} for t in range(len(tasks))]


def test_assign_edge_case():
    """16 x 24 (not square: an x / y swap shows), tasks (1, 2, 3), B = 3, max_objs 8; tests/test_cpu_centerloss.py::
    test_edge_case_holds_what_it_is_for asserts that every listed situation occurs in it."""
    boxes, classes = CO.edge_case()
    want = CO.assign(boxes, classes, CO.EDGE_TASKS, CO.EDGE_W, CO.EDGE_H, CO.EDGE_MAX_OBJS)
    got = _assigned(boxes, classes, CO.EDGE_TASKS, CO.EDGE_W, CO.EDGE_H, CO.EDGE_MAX_OBJS)
    for t, (g, w) in enumerate(zip(got, want)):
        print(f"edge task {t}: hm ulps {int(CO.ulps(g['hm'], w['hm64'].astype(np.float32)).max())} anno ulps "
              f"{int(CO.ulps(g['anno_box'], w['anno64'].astype(np.float32)).max())} positives {int(w['mask'].sum())}")
    CO.check_targets(got, want, ulp=1)


def test_assign_more_objects_than_threads_and_six_tasks():
    """300 object slots (more than one pass of a 256-thread workgroup), 280 of them filled, six tasks, max_objs above and below the
    number of objects of a task"""
    boxes, classes = CO.make_case(2, NUSC, 36, 40, 280, 5, n_cap=300)
    for max_objs in (500, 20):
        want = CO.assign(boxes, classes, NUSC, 40, 36, max_objs)
        got = _assigned(boxes, classes, NUSC, 40, 36, max_objs)
        CO.check_targets(got, want, ulp=1)
    a = _assigner(NUSC, 40, 36, 20)
    b, c = torch.from_numpy(boxes).cuda(), torch.from_numpy(classes).cuda()
    one, two = a(b, c), a(b, c)
    assert all(torch.equal(x, y) for k in one for x, y in zip(one[k], two[k]))


# ------------------------------------------------------------------------------------------------------------------------- loss
def _fused(preds, target, cw=CW10, weight=0.25, upstream=None, crit=None):
    import link_amd as la
    K = preds["hm"].shape[1]
    crit = crit or la.CenterHeadLoss((K,), weight, cw)
    x = {k: v.cuda().requires_grad_(True) for k, v in preds.items()}
    rets = crit({k: [v.cuda()] for k, v in target.items()}, [x])
    loss = rets["loss"][0]
    if upstream is None:
        loss.backward()
    else:
        loss.backward(upstream)
    return {"loss": loss.detach(), "hm_loss": rets["hm_loss"][0], "loc_loss": rets["loc_loss"][0].detach(), "box_loss": rets["loc_loss_elem"][0],
            "num_pos": rets["num_positive"][0], "grad": {k: v.grad for k, v in x.items()}}


def _o_round(g64, dtype, scale=1.0):
    if dtype == torch.float32:
        return 0.0
    return rel_err(((g64 * scale).to(dtype).double() / scale).numpy(), g64.numpy())


def _gate(case, got, r64, o32, dtype=torch.float32, scale=1.0, scalars=("loss", "hm_loss", "loc_loss", "box_loss")):
    rows = []
    for k in scalars:
        g = got[k].detach().double().cpu().numpy()
        rows.append((k, rel_err(g, r64[k].numpy()), FACTOR * o32[k] + FLOOR, bool(np.isfinite(g).all())))
    for k, g64 in r64["grad"].items():
        g = got["grad"][k]
        assert g.dtype == dtype and tuple(g.shape) == tuple(g64.shape), k
        g = g.detach().double().cpu().numpy() / scale
        rows.append(("d " + k, rel_err(g, g64.numpy()), FACTOR * o32["grad"][k] + 2.0 * _o_round(g64, dtype, scale) + FLOOR,
                     bool(np.isfinite(g).all())))
    for k, e, bound, finite in rows:
        print(f"{case} {k}: e {e:.3e} bound {bound:.3e}")
    bad = [r for r in rows if not (r[3] and r[1] <= r[2])]
    assert not bad, f"{case}: {bad}"
    if "num_pos" in got:
        assert float(got["num_pos"]) == float(r64["num_pos"])


def _case(B, K, H, W, M, seed=1, vel=True, dtype=torch.float32, cw=CW10, **kw):
    preds, target = CO.make_loss_case(B, K, H, W, M, seed, vel=vel, dtype=dtype, **kw)
    cw = cw if vel else cw[:6] + cw[8:]
    key = (B, K, H, W, M, seed, vel, str(dtype), tuple(sorted(kw.items())))
    return (preds, target, cw) + CO.yardstick(key, preds, target, code_weights=cw, weight=0.25)


@pytest.mark.parametrize("W", SWEEP)
def test_map_tile_and_tree_edges(W):
    preds, target, cw, r64, o32 = _case(1, 1, 1, W, 4)
    _gate(f"(1, 1, 1, {W})", _fused(preds, target, cw), r64, o32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("vel", [True, False])
def test_shapes_and_row_types(dtype, vel):
    preds, target, cw, r64, o32 = _case(2, 3, 16, 24, 8, vel=vel, dtype=dtype, npos=6)
    got = _fused(preds, target, cw)
    assert got["loss"].dtype == torch.float32 and got["box_loss"].shape == (10 if vel else 8,)
    _gate(f"(2, 3, 16, 24) {dtype} vel {vel}", got, r64, o32, dtype)


def test_full_size_map():
    preds, target, cw, r64, o32 = _case(2, 2, 180, 180, 500, npos=400)
    _gate("(2, 2, 180, 180) max_objs 500", _fused(preds, target, cw), r64, o32)


def test_no_positive_in_the_whole_batch():
    preds, target, cw, r64, o32 = _case(2, 3, 16, 24, 8, seed=2, npos=0)
    got = _fused(preds, target, cw)
    assert float(got["num_pos"]) == 0 and float(got["loc_loss"]) == 0
    _gate("num_pos 0", got, r64, o32, scalars=("loss", "hm_loss"))
    assert all(float(got["grad"][k].abs().max()) == 0 for k in got["grad"] if k != "hm")


def test_clamped_logits_have_gradient_zero():
    preds, target, cw, _, _ = _case(2, 3, 16, 24, 8, npos=6)
    preds = dict(preds, hm=torch.where(preds["hm"] > 0, 12.0, -12.0))
    r64, o32 = CO.yardstick("clamped", preds, target, code_weights=cw, weight=0.25)
    got = _fused(preds, target, cw)
    assert float(got["grad"]["hm"].abs().max()) == 0.0 and float(r64["grad"]["hm"].abs().max()) == 0.0
    _gate("logits +-12", got, r64, o32)


def test_slots_sharing_a_cell_add():
    preds, target, cw, r64, o32 = _case(2, 3, 16, 24, 8, seed=4, npos=6, duplicates=True)
    assert int(target["mask"][0].sum()) > len(set(target["ind"][0][target["mask"][0] == 1].tolist()))
    got = _fused(preds, target, cw)
    _gate("duplicates", got, r64, o32)


def test_masked_slot_is_not_read():
    preds, target, cw, r64, o32 = _case(2, 3, 16, 24, 8, npos=6)
    free = int(torch.nonzero(target["mask"][1] == 0)[0, 0])
    taken = target["ind"][1][target["mask"][1] == 1].tolist()
    cell = next(c for c in range(16 * 24) if c not in taken)
    target = {k: v.clone() for k, v in target.items()}
    target["ind"][1, free] = cell
    preds = {k: v.clone() for k, v in preds.items()}
    for name in ("reg", "dim", "rot"):
        preds[name].reshape(2, preds[name].shape[1], -1)[1, :, cell] = float("nan")
    got = _fused(preds, target, cw)
    _gate("NaN under a masked slot", got, r64, o32)


def test_probabilities_through_the_reference_signatures():
    import link_amd as la
    for vel in (True, False):
        preds, target, cw, _, _ = _case(2, 3, 16, 24, 8, seed=6, vel=vel, npos=6)
        y = torch.clamp(torch.sigmoid(preds["hm"]), 1e-4, 1 - 1e-4)
        pp = dict(preds, hm=y)
        r64, o32 = CO.yardstick(("probas", vel), pp, target, code_weights=cw, weight=0.25, kind="probas")
        names = [n for n in CO.REG_NAMES if n in preds]
        yg = y.cuda().requires_grad_(True)
        box = torch.cat([preds[n] for n in names], 1).cuda().requires_grad_(True)
        t = {k: v.cuda() for k, v in target.items()}
        hm_loss = la.FastFocalLoss()(yg, t["hm"], t["ind"], t["mask"], t["cat"])
        anno = t["anno_box"] if vel else t["anno_box"][..., CO.NOVEL]
        box_loss = la.RegLoss()(box, t["mask"], t["ind"], anno)
        loc = (box_loss * torch.tensor(cw, device="cuda")).sum()
        loss = hm_loss + 0.25 * loc
        loss.backward()
        grads, c0 = {"hm": yg.grad}, 0
        for n in names:
            grads[n] = box.grad[:, c0:c0 + CO.REG_CH[n]]
            c0 += CO.REG_CH[n]
        _gate(f"probas vel {vel}", {"loss": loss, "hm_loss": hm_loss, "loc_loss": loc, "box_loss": box_loss, "grad": grads}, r64, o32)


def test_two_calls_and_a_fresh_workspace_are_bit_identical():
    import link_amd as la
    from link_amd import centerloss as CL
    preds, target, cw, _, _ = _case(2, 2, 180, 180, 500, npos=400)
    crit = la.CenterHeadLoss((2,), 0.25, cw)
    a = _fused(preds, target, cw, crit=crit)
    b = _fused(preds, target, cw, crit=crit)
    old, CL._WS = CL._WS, CL._Workspace()
    try:
        c = _fused(preds, target, cw)
    finally:
        CL._WS = old
    for other in (b, c):
        for k in ("loss", "hm_loss", "loc_loss", "box_loss", "num_pos"):
            assert torch.equal(a[k], other[k]), k
        for k in a["grad"]:
            assert torch.equal(a["grad"][k], other["grad"][k]), k


def _six_task_inputs(seed, B=2, H=16, W=24, M=12, n=30):
    g = torch.Generator().manual_seed(seed)
    boxes, classes = CO.make_case(B, NUSC, H, W, n, seed)
    preds = []
    for K in NUSC:
        d = {"hm": torch.rand((B, K, H, W), generator=g) * 12 - 6}
        d.update({name: torch.randn((B, CO.REG_CH[name], H, W), generator=g) for name in CO.REG_NAMES})
        preds.append(d)
    return torch.from_numpy(boxes), torch.from_numpy(classes), preds


def test_assign_and_six_task_loss_capture_in_a_graph():
    """No host round trip: assign + six-task loss forward + backward on static buffers captured on one stream, replayed on a second
    seeded input, equal to eager bit for bit."""
    import link_amd as la
    assigner = _assigner(NUSC, 24, 16, 12)
    crit = la.CenterHeadLoss(NUSC, 0.25, CW10)

    def step(boxes, classes, preds):
        rets = crit(assigner(boxes, classes), preds)
        total = torch.stack(rets["loss"]).sum()
        leaves = [v for d in preds for v in d.values()]
        return total, rets["loss"], torch.autograd.grad(total, leaves)

    b1, c1, p1 = _six_task_inputs(1)
    b2, c2, p2 = _six_task_inputs(2)
    sb, sc = b1.cuda(), c1.cuda()
    sp = [{k: v.cuda().requires_grad_(True) for k, v in d.items()} for d in p1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(sb, sc, sp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total_s, losses_s, grads_s = step(sb, sc, sp)
    with torch.no_grad():
        sb.copy_(b2)
        sc.copy_(c2)
        for d, src in zip(sp, p2):
            for k in d:
                d[k].copy_(src[k])
    graph.replay()
    torch.cuda.synchronize()
    ep = [{k: v.cuda().requires_grad_(True) for k, v in d.items()} for d in p2]
    total_e, losses_e, grads_e = step(b2.cuda(), c2.cuda(), ep)
    assert torch.equal(total_s, total_e) and all(torch.equal(a, b) for a, b in zip(losses_s, losses_e))
    assert all(torch.equal(a, b) for a, b in zip(grads_s, grads_e))
    want = CO.assign(b2.numpy(), c2.numpy(), NUSC, 24, 16, 12)                       # the replay computed the second input
    ref = sum(float(CO.loss_reference(p2[t], {"hm": want[t]["hm64"], "anno_box": want[t]["anno64"], "ind": want[t]["ind"], "mask": want[t]["mask"],
                                             "cat": want[t]["cat"]}, code_weights=CW10)["loss"]) for t in range(6))
    assert rel_err(float(total_s.detach()), ref) <= 1e-5


def test_autocast_and_gradscaler():
    import link_amd as la
    preds, target, cw, r64, o32 = _case(2, 3, 16, 24, 8, dtype=torch.float16, npos=6)
    crit = la.CenterHeadLoss((3,), 0.25, cw)
    scale = 65536.0
    ex = {k: [v.cuda()] for k, v in target.items()}

    def step(p16):
        ws = {k: v.float().cuda().requires_grad_(True) for k, v in p16.items()}
        opt = torch.optim.SGD(list(ws.values()), lr=0.1)
        scaler = torch.amp.GradScaler("cuda", init_scale=scale)
        with torch.autocast("cuda", torch.float16):
            maps = {k: v.half() for k, v in ws.items()}
            for v in maps.values():
                v.retain_grad()
            rets = crit(ex, [maps])
        loss = rets["loss"][0]
        scaler.scale(loss).backward()
        before = {k: v.detach().clone() for k, v in ws.items()}
        scaler.step(opt)
        scaler.update()
        moved = any(not torch.equal(before[k], ws[k].detach()) for k in ws)
        return loss.detach(), rets, {k: v.grad for k, v in maps.items()}, moved, scaler.get_scale()

    loss, rets, grads, moved, s = step(preds)
    assert loss.dtype == torch.float32 and s == scale and moved
    got = {"loss": loss, "hm_loss": rets["hm_loss"][0], "loc_loss": rets["loc_loss"][0], "box_loss": rets["loc_loss_elem"][0], "grad": grads}
    _gate("amp fp16", got, r64, o32, torch.float16, scale)
    bad = {k: v.clone() for k, v in preds.items()}
    bad["hm"][1, 2, 3, 5] = float("inf")
    loss, rets, grads, moved, s = step(bad)
    assert not bool(torch.isfinite(loss))
    assert not moved and s < scale                                          # the scaler skipped the step


def test_one_head_step_against_the_torch_composition():
    """One step of harness.bevhead.BevCenterHead (32 input channels, a 16 x 24 map, B = 2, six tasks) under CenterHeadLoss and under the
    torch composition: the maps reaching both are bit equal, and the gradient arriving at every head output is held to the plain gate
    against the oracle evaluated at those maps."""
    import link_amd as la
    from link_amd.centerloss import _torch_loss
    from harness.bevhead import BevCenterHead
    torch.manual_seed(3)
    head = BevCenterHead(in_channels=32).cuda().train()
    x = torch.randn((2, 32, 16, 24), generator=torch.Generator().manual_seed(4)).cuda()
    boxes, classes = CO.make_case(2, NUSC, 16, 24, 30, 9)
    example = _assigner(NUSC, 24, 16, 12)(torch.from_numpy(boxes).cuda(), torch.from_numpy(classes).cuda())
    crit = la.CenterHeadLoss(NUSC, 0.25, CW10)
    state = {k: v.clone() for k, v in head.state_dict().items()}
    res = {}
    for name in ("fused", "torch"):
        head.load_state_dict(state)
        head.zero_grad()
        preds = head(x)
        for d in preds:
            for v in d.values():
                v.retain_grad()
        if name == "fused":
            losses = crit(example, preds)["loss"]
        else:
            losses = [_torch_loss(d["hm"], [d[n] for n in CO.REG_NAMES], 0, example["hm"][t], example["anno_box"][t], example["ind"][t],
                                  example["mask"][t], example["cat"][t], CW10, 0.25)[0] for t, d in enumerate(preds)]
        torch.stack(losses).sum().backward()
        res[name] = {"maps": [{k: v.detach().cpu() for k, v in d.items()} for d in preds],
                     "grads": [{k: v.grad.detach().cpu() for k, v in d.items()} for d in preds], "losses": [l.detach().cpu() for l in losses]}
    for t in range(6):
        assert all(torch.equal(res["fused"]["maps"][t][k], res["torch"]["maps"][t][k]) for k in res["fused"]["maps"][t]), t
        target = {k: example[k][t].cpu() for k in example}
        r64, o32 = CO.yardstick(("head", t), res["torch"]["maps"][t], target, code_weights=CW10, weight=0.25)
        for name, r in res.items():
            _gate(f"head step {name} task {t}", {"loss": r["losses"][t], "grad": r["grads"][t]}, r64, o32, scalars=("loss",))
