"""Record tests/golden/centerloss_*.npz from the reference's own code.

    python tests/golden/make_golden_centerloss.py /path/to/LinK

The expected values come from the reference's det3d/core/utils/center_utils.py (gaussian_radius, draw_umich_gaussian) and
det3d/models/losses/centernet_loss.py (FastFocalLoss, RegLoss), loaded BY PATH: bare parent packages are registered in sys.modules
and a stand-in module named `numba` whose `jit` returns the function (circle_nms_jit.py decorates with it; nothing here calls it).
AssignLabel itself cannot be imported where these fixtures were recorded (its module pulls in torchvision), so the loop over objects
is the oracle's (tests/centerloss_oracle.py: assign_frame) driving the reference's two functions through its hooks, in the
reference's number formats: an fp32 heat map, np.float32 sizes into gaussian_radius, and np.log / np.sin / np.cos on fp32 values
for the anno_box columns.  The steps of CenterHead.loss around the two loss modules (sigmoid and clamp, the torch.cat of the maps,
the code weights) are written out here.  Nothing of the reference is copied into the repository."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import centerloss_oracle as CO  # noqa: E402


def load_reference(root):
    det = os.path.join(root, "detection")
    for name in ("det3d", "det3d.core", "det3d.core.utils", "det3d.models", "det3d.models.losses"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(det, *name.split("."))]
        sys.modules[name] = m
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.modules["numba"] = nb

    def by_path(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(det, *parts))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    cu = by_path("det3d.core.utils.center_utils", "det3d", "core", "utils", "center_utils.py")
    cl = by_path("det3d.models.losses.centernet_loss", "det3d", "models", "losses", "centernet_loss.py")
    return cu, cl


def record_assign(cu, name, boxes, classes, tasks, W, H, max_objs):
    radius_fn = lambda l, w, ov: cu.gaussian_radius((l, w), min_overlap=ov)                  # np.float32 sizes, as AssignLabel passes them
    splat_fn = lambda hm, ct, r: cu.draw_umich_gaussian(hm, np.array(ct, dtype=np.float32), r)
    t = CO.assign(boxes, classes, tasks, W, H, max_objs, radius_fn=radius_fn, splat_fn=splat_fn, hm_dtype=np.float32)
    out = {"boxes": boxes, "classes": classes}
    for i, task in enumerate(t):
        anno = task["anno64"].astype(np.float32)
        for b in range(boxes.shape[0]):
            for k in np.nonzero(task["mask"][b])[0]:
                g = boxes[b, task["obj"][b, k]]
                rot = CO.limit_period32(g[8])
                anno[b, k, 3:6] = np.log(g[3:6])
                anno[b, k, 8], anno[b, k, 9] = np.sin(rot), np.cos(rot)
        out.update({f"hm{i}": task["hm64"], f"anno_box{i}": anno, f"ind{i}": task["ind"], f"mask{i}": task["mask"], f"cat{i}": task["cat"]})
        assert task["hm64"].dtype == np.float32
    meta = {"tasks": list(tasks), "W": W, "H": H, "max_objs": max_objs, "overlap": CO.OVERLAP, "min_radius": CO.MIN_RADIUS}
    np.savez_compressed(os.path.join(HERE, name), meta=json.dumps(meta), **out)


def record_loss(cl, name, seed, vel, code_weights, weight):
    preds, target = CO.make_loss_case(2, 3, 16, 24, 8, seed, vel=vel, duplicates=True)
    x = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    hm = torch.clamp(torch.sigmoid(x["hm"]), min=1e-4, max=1 - 1e-4)
    hm_loss = cl.FastFocalLoss()(hm, target["hm"], target["ind"], target["mask"], target["cat"])
    box = torch.cat([x[n] for n in CO.REG_NAMES if n in x], 1)
    tgt = target["anno_box"] if vel else target["anno_box"][..., CO.NOVEL]
    box_loss = cl.RegLoss()(box, target["mask"], target["ind"], tgt)
    loc_loss = (box_loss * box_loss.new_tensor(code_weights)).sum()
    loss = hm_loss + weight * loc_loss
    loss.backward()
    out = {f"pred_{k}": v.numpy() for k, v in preds.items()}
    out.update({f"grad_{k}": v.grad.numpy() for k, v in x.items()})
    out.update({f"target_{k}": v.numpy() for k, v in target.items()})
    out["box_loss"] = box_loss.detach().numpy()
    meta = {"seed": seed, "vel": vel, "code_weights": list(code_weights), "weight": weight, "loss": float(loss.detach()), "hm_loss": float(hm_loss.detach()),
            "loc_loss": float(loc_loss.detach()), "num_pos": float(target["mask"].sum())}
    np.savez_compressed(os.path.join(HERE, name), meta=json.dumps(meta), **out)


def main(root):
    cu, cl = load_reference(root)
    boxes, classes = CO.edge_case()
    record_assign(cu, "centerloss_assign_edge.npz", boxes, classes, CO.EDGE_TASKS, CO.EDGE_W, CO.EDGE_H, CO.EDGE_MAX_OBJS)
    boxes, classes = CO.make_case(2, (2, 1), 16, 24, 20, 11)
    record_assign(cu, "centerloss_assign_rand.npz", boxes, classes, (2, 1), 24, 16, 12)
    record_loss(cl, "centerloss_loss_vel.npz", 21, True, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0], 0.25)
    record_loss(cl, "centerloss_loss_novel.npz", 22, False, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 0.25)


if __name__ == "__main__":
    main(sys.argv[1])
