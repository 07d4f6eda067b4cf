"""CPU-only checks of CenterHead training (csrc/centerloss.hip, section L of include/link_amd.h; link_amd/centerloss.py): the oracle of
tests/centerloss_oracle.py against the fixtures recorded from the reference's own gaussian_radius / draw_umich_gaussian and
FastFocalLoss / RegLoss (tests/golden/make_golden_centerloss.py), the torch composition link_amd.centerloss runs off the GPU, exports
and prototypes, and argument validation before anything touches a device.  Every test imports link_amd.centerloss or a symbol of
section L: all of them fail without the feature.

Bounds.  Integer results, the zero cells of the heat map and the columns that are plain fp32 arithmetic: equal.  Heat-map values and
the log / sin / cos columns: 1 fp32 ulp (a float64 function within one double ulp, rounded once, lands at most one fp32 ulp from the
correctly rounded value; the fixtures' heat maps are float64 values rounded once and numpy's fp32 log / sin / cos are within one ulp
of the correctly rounded value too).  Losses and gradients: the project's gate (tests/grad64.py), rel_err(got, g64) <= 4 * o32 + 2e-6 with o32 the oracle's own fp32 evaluation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, golden_files, load_golden, rel_err

import centerloss_oracle as CO
from link_amd import centerloss as CL

FACTOR, FLOOR = 4.0, 2e-6
FIXTURES = ["centerloss_assign_edge.npz", "centerloss_assign_rand.npz", "centerloss_loss_novel.npz", "centerloss_loss_vel.npz"]


check_targets = CO.check_targets


def test_fixtures_are_complete():
    assert golden_files("centerloss_*.npz") == FIXTURES
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 17), name
    g = load_golden(FIXTURES[0])
    boxes, classes = CO.edge_case()
    assert np.array_equal(boxes, g["boxes"]) and np.array_equal(classes, g["classes"])
    assert g["meta"]["tasks"] == list(CO.EDGE_TASKS) and (g["meta"]["W"], g["meta"]["H"]) == (24, 16)


def test_edge_case_holds_what_it_is_for():
    boxes, classes = CO.edge_case()
    assert not any(CO.ambiguous(b, 24, 16) for f in range(3) for b, c in zip(boxes[f], classes[f]) if c > 0)
    t = CO.assign(boxes, classes, CO.EDGE_TASKS, 24, 16, CO.EDGE_MAX_OBJS)
    t0, t1, t2 = t
    assert (classes[0] == 1).sum() == 10 and t0["mask"][0].sum() == 8                       # more than max_objs objects
    hm = t0["hm64"][0, 0]
    assert hm[0, 0] > 0 and hm[0, 23] > 0 and hm[15, 0] > 0 and hm[15, 23] > 0               # clipped at every corner and edge
    assert t1["radius"][0].max() > 24 and (t1["hm64"][0, 1] > 0).all()                       # a radius larger than the map
    lo = CO.geometry(24, 16)
    tiny = [i for i in range(24) if classes[0, i] == 2 and boxes[0, i, 3] < 0.2]
    assert tiny and int(CO.gaussian_radius(*CO.cell_sizes(boxes[0, tiny[0]], lo)[1::-1], CO.OVERLAP)) < CO.MIN_RADIUS
    assert t1["radius"][0][t1["obj"][0] == tiny[0]] == CO.MIN_RADIUS                         # raised to min_radius
    a = t1["anno64"][0]
    assert ((a[:, 0] < 0) & (t1["ind"][0] % 24 == 0) & (t1["mask"][0] == 1)).any()           # a centre in (-1, 0) on x ...
    assert ((a[:, 1] < 0) & (t1["ind"][0] // 24 == 0) & (t1["mask"][0] == 1)).any()          # ... and on y
    m = t1["mask"][0]
    assert list(m[:6]) == [1, 1, 1, 0, 0, 1]                                                # holes: outside the map, w = 0; class 3 after class 2
    assert list(t1["cat"][0][:6]) == [0, 0, 0, 0, 0, 1]
    assert (np.abs(boxes[0, :, 8]) > np.pi).sum() >= 2                                       # rot outside [-pi, pi)
    i2 = t2["ind"][0][t2["mask"][0] == 1]
    assert len(set(i2.tolist())) < len(i2)                                                   # two objects in one cell
    assert all(x["mask"][2].sum() == 0 and (x["hm64"][2] == 0).all() for x in t)             # an empty frame
    assert classes[0, 0] == 5 and classes[0, 1] == 1                                         # classes given out of task order


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_oracle_reproduces_the_recorded_targets(name):
    g = load_golden(name)
    m = g["meta"]
    want = CO.assign(g["boxes"], g["classes"], m["tasks"], m["W"], m["H"], m["max_objs"])
    got = [{k: g[f"{k}{t}"] for k in ("hm", "anno_box", "ind", "mask", "cat")} for t in range(len(m["tasks"]))]
    check_targets(got, want, ulp=1)
    assert sum(int(x["mask"].sum()) for x in got) > 10


def _loss_fixture(name):
    g = load_golden(name)
    preds = {k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("pred_")}
    target = {k[7:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("target_")}
    return g, preds, target


@pytest.mark.parametrize("name", FIXTURES[2:])
def test_oracle_reproduces_the_recorded_losses(name):
    g, preds, target = _loss_fixture(name)
    m = g["meta"]
    assert ("vel" in preds) == m["vel"]
    p2, t2 = CO.make_loss_case(2, 3, 16, 24, 8, m["seed"], vel=m["vel"], duplicates=True)
    assert all(torch.equal(preds[k], p2[k]) for k in preds) and all(torch.equal(target[k], t2[k]) for k in target)
    r64, o32 = CO.yardstick(name, preds, target, code_weights=m["code_weights"], weight=m["weight"])
    for k in ("loss", "hm_loss", "loc_loss"):
        print(name, k, rel_err(m[k], float(r64[k])), o32[k])
        assert rel_err(m[k], float(r64[k])) <= FACTOR * o32[k] + FLOOR, k
    assert m["num_pos"] == float(r64["num_pos"])
    assert rel_err(g["box_loss"], r64["box_loss"].numpy()) <= FACTOR * o32["box_loss"] + FLOOR
    for k in preds:
        print(name, "grad", k, rel_err(g[f"grad_{k}"], r64["grad"][k].numpy()), o32["grad"][k])
        assert rel_err(g[f"grad_{k}"], r64["grad"][k].numpy()) <= FACTOR * o32["grad"][k] + FLOOR, k


def _assigner(tasks, W, H, max_objs):
    import link_amd as la
    a = la.CenterTargetAssigner(tasks, CO.OSF, CO.VS, CO.geometry(W, H), CO.OVERLAP, max_objs, CO.MIN_RADIUS)
    assert (a.W, a.H) == (W, H)
    return a


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_torch_assign_equals_the_oracle(name):
    g = load_golden(name)
    m = g["meta"]
    want = CO.assign(g["boxes"], g["classes"], m["tasks"], m["W"], m["H"], m["max_objs"])
    ex = _assigner(m["tasks"], m["W"], m["H"], m["max_objs"])(torch.from_numpy(g["boxes"]), torch.from_numpy(g["classes"]))
    got = [{k: ex[k][t].numpy() for k in ex} for t in range(len(m["tasks"]))]
    check_targets(got, want, ulp=1)


@pytest.mark.parametrize("name", FIXTURES[2:])
def test_torch_loss_equals_the_oracle(name):
    import link_amd as la
    g, preds, target = _loss_fixture(name)
    m = g["meta"]
    r64, o32 = CO.yardstick(name, preds, target, code_weights=m["code_weights"], weight=m["weight"])
    crit = la.CenterHeadLoss((3,), m["weight"], m["code_weights"])
    example = {k: [v] for k, v in target.items()}
    for dtype, tol in ((torch.float64, None), (torch.float32, 1.0)):
        x = {k: v.to(dtype).clone().requires_grad_(True) for k, v in preds.items()}
        before = {k: v.detach().clone() for k, v in x.items()}
        rets = crit(example, [x])
        assert sorted(rets) == ["hm_loss", "loc_loss", "loc_loss_elem", "loss", "num_positive"] and all(len(v) == 1 for v in rets.values())
        rets["loss"][0].backward()
        assert all(torch.equal(before[k], x[k].detach()) for k in x)                         # preds_dicts is left untouched
        bound = (lambda o: 1e-12) if tol is None else (lambda o: FACTOR * o + FLOOR)
        for k in ("loss", "hm_loss", "loc_loss"):
            assert rel_err(float(rets[k][0].detach()), float(r64[k])) <= bound(o32[k]), (dtype, k)
        assert float(rets["num_positive"][0]) == float(r64["num_pos"])
        assert rel_err(rets["loc_loss_elem"][0].detach().numpy(), r64["box_loss"].numpy()) <= bound(o32["box_loss"])
        for k in x:
            assert rel_err(x[k].grad.numpy(), r64["grad"][k].numpy()) <= bound(o32["grad"][k]), (dtype, k)
    # the two loss modules with the reference's signatures (probabilities in, the focal loss / the loss per column out)
    y = torch.clamp(torch.sigmoid(preds["hm"].double()), 1e-4, 1 - 1e-4)
    fl = la.FastFocalLoss()(y, target["hm"].double(), target["ind"], target["mask"], target["cat"])
    assert rel_err(float(fl), float(r64["hm_loss"])) <= 1e-12
    box = torch.cat([preds[n].double() for n in CO.REG_NAMES if n in preds], 1)
    tgt = target["anno_box"].double() if m["vel"] else target["anno_box"].double()[..., CO.NOVEL]
    rl = la.RegLoss()(box, target["mask"], target["ind"], tgt)
    assert rel_err(rl.numpy(), r64["box_loss"].numpy()) <= 1e-12


def test_torch_loss_edges():
    import link_amd as la
    preds, target = CO.make_loss_case(2, 2, 5, 7, 6, 3, npos=4)
    crit = la.CenterHeadLoss((2,), 0.25, [1.0] * 10)
    # num_pos == 0: -neg, selected without a host test
    empty = dict(target, mask=torch.zeros_like(target["mask"]))
    r64 = CO.loss_reference(preds, empty, code_weights=[1.0] * 10)
    rets = crit({k: [v] for k, v in empty.items()}, [preds])
    assert float(rets["num_positive"][0]) == 0 and rel_err(float(rets["loss"][0].detach()), float(r64["loss"])) <= 1e-5
    # a NaN at a masked slot's cell of a regression map is not read; an ind / cat outside the map indexes nothing
    bad = {k: v.clone() for k, v in preds.items()}
    tb = {k: v.clone() for k, v in target.items()}
    free = [m for m in range(6) if tb["mask"][0, m] == 0]
    assert free
    cell = next(c for c in range(35) if c not in tb["ind"][0][tb["mask"][0] == 1].tolist())
    tb["ind"][0, free[0]] = cell
    bad["dim"].reshape(2, 3, -1)[0, :, cell] = float("nan")
    x = {k: v.clone().requires_grad_(True) for k, v in bad.items()}
    rets = crit({k: [v] for k, v in tb.items()}, [x])
    rets["loss"][0].backward()
    r64 = CO.loss_reference(preds, target, code_weights=[1.0] * 10)
    assert rel_err(float(rets["loss"][0].detach()), float(r64["loss"])) <= 1e-5
    assert all(bool(torch.isfinite(v.grad).all()) for v in x.values())
    wild = {k: v.clone() for k, v in target.items()}
    wild["ind"][1, torch.nonzero(target["mask"][1])[0, 0]] = 10 ** 12
    wild["cat"][0, torch.nonzero(target["mask"][0])[0, 0]] = -3
    out = crit({k: [v] for k, v in wild.items()}, [preds])
    assert bool(torch.isfinite(out["loss"][0])) and float(out["num_positive"][0]) == float(target["mask"].sum())
    # an empty batch and a batch without objects
    a = _assigner((1, 2), 24, 16, 5)
    ex = a(torch.zeros((2, 0, 9)), torch.zeros((2, 0), dtype=torch.int32))
    assert ex["hm"][1].shape == (2, 2, 16, 24) and ex["mask"][0].dtype == torch.uint8 and float(ex["hm"][1].abs().max()) == 0


def test_section_l_symbols_and_version():
    from link_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in ("link_center_assign", "link_center_loss_workspace_bytes", "link_center_loss_forward", "link_center_loss_backward"):
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13                  # additive entries
    assert "L. CenterHead training" in hdr
    assert L.STRUCT_CENTER_ASSIGN_GEOM == 9 and L.lib().link_abi_struct_size(9) == ctypes.sizeof(L.LinkCenterAssignGeom) == 76
    for k, v in (("LINK_CENTER_LOGITS", L.CENTER_LOGITS), ("LINK_CENTER_PROBAS", L.CENTER_PROBAS), ("LINK_CENTER_MAX_TASKS", L.CENTER_MAX_TASKS),
                 ("LINK_CENTER_MAX_CLASSES", L.CENTER_MAX_CLASSES), ("LINK_CENTER_MAX_OBJECTS", L.CENTER_MAX_OBJECTS),
                 ("LINK_CENTER_MAX_SLOTS", L.CENTER_MAX_SLOTS), ("LINK_CENTER_MAX_BATCH", L.CENTER_MAX_BATCH)):
        assert f"#define {k} {v}\n" in hdr, k
    import link_amd as la
    assert la.CenterHeadLoss is CL.CenterHeadLoss and la.CenterTargetAssigner is CL.CenterTargetAssigner
    assert la.FastFocalLoss is CL.FastFocalLoss and la.RegLoss is CL.RegLoss
    from link_amd.build import SOURCES
    assert "centerloss.hip" in SOURCES


def test_section_l_validates_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)                                           # a non-null, aligned pointer nothing dereferences
    cw = (ctypes.c_float * 10)(*([1.0] * 10))

    def geom(**kw):
        g = L.LinkCenterAssignGeom()
        g.pc_range[0], g.pc_range[1], g.voxel_size[0], g.voxel_size[1] = -7.2, -4.8, 0.075, 0.075
        g.gaussian_overlap, g.out_size_factor, g.w, g.h, g.max_objs, g.min_radius, g.num_tasks = 0.1, 8, 24, 16, 8, 2, 2
        g.num_classes[0], g.num_classes[1] = 1, 2
        for k, v in kw.items():
            if k == "num_classes":
                g.num_classes[0] = v
            elif k == "voxel_size":
                g.voxel_size[0] = v
            else:
                setattr(g, k, v)
        return g

    table = (ctypes.c_void_p * 8)(*([256] * 8))
    null_table = (ctypes.c_void_p * 8)(256, None)

    def assign(g=None, boxes=one, classes=one, batch=2, n_cap=10, hm=table, anno=table):
        return lib.link_center_assign(ctypes.byref(g or geom()), boxes, classes, batch, n_cap, hm, anno, table, table, table, None)

    for kw in (dict(num_tasks=0), dict(num_tasks=9), dict(num_classes=0), dict(num_classes=17), dict(w=0), dict(h=0), dict(max_objs=0),
               dict(out_size_factor=0), dict(min_radius=-1), dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(gaussian_overlap=0.0),
               dict(gaussian_overlap=1.0), dict(w=1 << 20, h=1 << 20)):
        assert assign(geom(**kw)) == L.LINK_ERR_ARG, kw
    for kw in (dict(boxes=None), dict(classes=None), dict(batch=0), dict(n_cap=-1), dict(n_cap=L.CENTER_MAX_OBJECTS + 1), dict(hm=None),
               dict(hm=null_table), dict(anno=null_table)):
        assert assign(**kw) == L.LINK_ERR_ARG, kw

    def fwd(hm=one, reg=one, height=one, dim=one, vel=one, rot=one, io=L.IO_F32, kind=L.CENTER_LOGITS, target=one, anno=one, ind=one, mask=one,
            cat=one, shape=(2, 3, 16, 24, 8), weights=cw, ws=one, nbytes=None, out=one, unit_hm=one, unit_box=one):
        if nbytes is None:
            nbytes = lib.link_center_loss_workspace_bytes(*shape)
        return lib.link_center_loss_forward(hm, reg, height, dim, vel, rot, None, io, kind, target, anno, ind, mask, cat, *shape, weights, 0.25, ws,
                                            nbytes, out, unit_hm, unit_box, None)

    def bwd(unit_hm=one, unit_box=one, ind=one, mask=one, up=one, shape=(2, 3, 16, 24, 8), io=L.IO_F32, g_hm=one, g_reg=one, g_height=one,
            g_dim=one, g_vel=one, g_rot=one):
        return lib.link_center_loss_backward(unit_hm, unit_box, ind, mask, up, *shape, io, g_hm, g_reg, g_height, g_dim, g_vel, g_rot, None, None)

    need = lib.link_center_loss_workspace_bytes(2, 3, 16, 24, 8)             # host arithmetic alone: no device needed
    assert need >= 4 * 3 + 4 * 2 * 11 and lib.link_center_loss_workspace_bytes(4, 2, 180, 180, 500) > need
    for shape in ((0, 3, 16, 24, 8), (2, 0, 16, 24, 8), (2, 17, 16, 24, 8), (2, 3, 0, 24, 8), (2, 3, 16, 0, 8), (2, 3, 16, 24, 0),
                  (2, 3, 16, 24, L.CENTER_MAX_SLOTS + 1), (L.CENTER_MAX_BATCH + 1, 3, 16, 24, 8), (2, 3, 1 << 16, 1 << 16, 8),
                  (2, 3, (1 << 31) - 1, (1 << 31) - 1, 8), (1024, 16, 1 << 10, 1 << 10, 8)):
        assert lib.link_center_loss_workspace_bytes(*shape) == 0, shape
        assert fwd(shape=shape, nbytes=1 << 40) == L.LINK_ERR_ARG and bwd(shape=shape) == L.LINK_ERR_ARG, shape
    for kw in (dict(ind=None), dict(mask=None), dict(ws=None), dict(out=None), dict(io=3), dict(io=-1), dict(kind=2), dict(kind=-1),
               dict(target=None), dict(cat=None), dict(unit_hm=None), dict(anno=None), dict(weights=None), dict(unit_box=None),
               dict(height=None), dict(rot=None), dict(reg=None, height=None, dim=None, rot=None), dict(hm=None, reg=None, height=None, dim=None, vel=None, rot=None)):
        assert fwd(**kw) == L.LINK_ERR_ARG, kw
    assert fwd(nbytes=need - 1) == L.LINK_ERR_WORKSPACE and fwd(nbytes=0) == L.LINK_ERR_WORKSPACE
    for kw in (dict(ind=None), dict(mask=None), dict(up=None), dict(io=3), dict(unit_hm=None), dict(unit_box=None), dict(g_dim=None),
               dict(g_reg=None, g_height=None, g_dim=None, g_rot=None), dict(g_hm=None, g_reg=None, g_height=None, g_dim=None, g_vel=None, g_rot=None)):
        assert bwd(**kw) == L.LINK_ERR_ARG, kw


def test_python_surface_rejects_bad_arguments():
    import link_amd as la
    preds, target = CO.make_loss_case(2, 2, 5, 7, 6, 3, npos=4)
    ex = {k: [v] for k, v in target.items()}
    crit = la.CenterHeadLoss((2,), 0.25, [1.0] * 10)

    def swap(d, **kw):
        return dict(d, **kw)

    for bad in (lambda: crit(ex, [preds, preds]), lambda: crit(ex, [swap(preds, hm=preds["hm"][:, :1])]), lambda: crit(ex, [swap(preds, hm=preds["hm"][0])]),
                lambda: crit(ex, [swap(preds, dim=preds["reg"])]), lambda: crit(ex, [swap(preds, rot=preds["rot"].double())]),
                lambda: crit(ex, [swap(preds, hm=preds["hm"].long())]), lambda: crit(swap(ex, ind=[target["ind"].int()]), [preds]),
                lambda: crit(swap(ex, mask=[target["mask"].float()]), [preds]), lambda: crit(swap(ex, cat=[target["cat"][:, :3]]), [preds]),
                lambda: crit(swap(ex, hm=[target["hm"][:, :, :4]]), [preds]), lambda: crit(swap(ex, anno_box=[target["anno_box"][..., :8]]), [preds]),
                lambda: crit(swap(ex, ind=[target["ind"].to("meta")]), [preds]), lambda: crit({k: v for k, v in ex.items() if k != "cat"}, [preds]),
                lambda: crit(ex, [{k: v for k, v in preds.items() if k != "vel"}]), lambda: la.CenterHeadLoss((2,), 0.25, [1.0] * 9),
                lambda: la.CenterHeadLoss((0,)), lambda: la.FastFocalLoss()(preds["hm"], target["hm"][:, :1], target["ind"], target["mask"], target["cat"]),
                lambda: la.RegLoss()(preds["reg"], target["mask"], target["ind"], target["anno_box"]),
                lambda: la.RegLoss()(preds["reg"], target["mask"], target["ind"].float(), target["anno_box"][..., :2])):
        with pytest.raises(ValueError):
            bad()
    geo = (CO.OSF, CO.VS, CO.geometry(24, 16))
    a = la.CenterTargetAssigner([{"num_class": 1}, {"num_class": 2}], *geo)
    assert a.tasks == (1, 2) and a.max_objs == 500
    boxes, classes = (torch.from_numpy(v) for v in CO.make_case(1, (1, 2), 16, 24, 5, 0))
    for bad in (lambda: la.CenterTargetAssigner([], *geo), lambda: la.CenterTargetAssigner([1] * 9, *geo), lambda: la.CenterTargetAssigner([17], *geo),
                lambda: la.CenterTargetAssigner([1], 0, CO.VS, CO.geometry(24, 16)), lambda: la.CenterTargetAssigner([1], 8, (0.0, 0.1), CO.geometry(24, 16)),
                lambda: la.CenterTargetAssigner([1], *geo, gaussian_overlap=1.5), lambda: la.CenterTargetAssigner([1], *geo, max_objs=0),
                lambda: la.CenterTargetAssigner([1], 8, CO.VS, (0, 0, 1)), lambda: la.CenterTargetAssigner([object()], *geo),
                lambda: a(boxes[..., :7], classes), lambda: a(boxes, classes[:, :3]), lambda: a(boxes, classes.float()),
                lambda: a(boxes.long(), classes), lambda: a(boxes, classes.to("meta")), lambda: a(boxes.numpy(), classes)):
        with pytest.raises(ValueError):
            bad()
