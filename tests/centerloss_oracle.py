"""The arbiter of the CenterHead training tests (section L of include/link_amd.h): a restatement, in this project's own words, of
what the reference computes -- AssignLabel's loop over objects (detection/det3d/datasets/pipelines/preprocess.py:283-467 with
gaussian_radius / draw_umich_gaussian of det3d/core/utils/center_utils.py:17-63) in numpy, float64 where the contract says float64
and np.float32 scalars where it says fp32; CenterHead.loss (det3d/models/bbox_heads/center_head.py:248-293 with
det3d/models/losses/centernet_loss.py) through autograd, in float64 or float32.

The case maker draws objects by rejection so that no integer result depends on fp32 against float64: an object is rejected when its
float64 radius lies within 1e-3 of an integer or either centre coordinate within 1e-3 cells of a cell boundary.  Logits are drawn
in [-6, 6] (the clamp of CenterHead._sigmoid is never near) and regression predictions at least 0.05 from their targets (the sign
of an L1 term is never in doubt), so nothing is ambiguous and no case leaves anything out."""
import math

import numpy as np
import torch

from helpers import rel_err

VS, OSF = (0.075, 0.075), 8                 # nuScenes' voxel size and stride: a cell of 0.6 m
CELL = 0.6
OVERLAP, MIN_RADIUS = 0.1, 2
NOVEL = [0, 1, 2, 3, 4, 5, 8, 9]
F32 = np.float32


def geometry(W, H):
    """(pc_range lo x, y, hi x, y) of a W x H map centred on the origin"""
    return (-W * CELL / 2, -H * CELL / 2, W * CELL / 2, H * CELL / 2)


def gaussian_radius(height, width, overlap):
    """the smallest of the three roots, float64"""
    height, width = float(height), float(width)
    b1 = height + width
    c1 = width * height * (1 - overlap) / (1 + overlap)
    r1 = (b1 + math.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - overlap) * width * height
    r2 = (b2 + math.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * overlap
    b3 = -2 * overlap * (height + width)
    c3 = (overlap - 1) * width * height
    r3 = (b3 + math.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def splat(hm, centre, radius):
    """max of the clipped Gaussian into hm [H, W] (float64 values)"""
    H, W = hm.shape
    x, y = int(centre[0]), int(centre[1])
    sigma = (2 * radius + 1) / 6
    for py in range(max(0, y - radius), min(H, y + radius + 1)):
        for px in range(max(0, x - radius), min(W, x + radius + 1)):
            v = math.exp(-((px - x) ** 2 + (py - y) ** 2) / (2 * sigma * sigma))
            if v > hm[py, px]:
                hm[py, px] = v
    return hm


def cell_sizes(box, lo):
    """(w, l, cx, cy) in cells, every operation an fp32 one"""
    vs0, vs1, osf = F32(VS[0]), F32(VS[1]), F32(OSF)
    w = F32(box[3]) / vs0 / osf
    l = F32(box[4]) / vs1 / osf
    cx = (F32(box[0]) - F32(lo[0])) / vs0 / osf
    cy = (F32(box[1]) - F32(lo[1])) / vs1 / osf
    return w, l, cx, cy


def limit_period32(rot):
    p = F32(2 * math.pi)
    return F32(rot) - F32(np.floor(F32(rot) / p + F32(0.5))) * p


def assign_frame(boxes, classes, tasks, W, H, max_objs, radius_fn=gaussian_radius, splat_fn=splat, overlap=OVERLAP,
                 min_radius=MIN_RADIUS, hm_dtype=np.float64):
    """one frame: per task {'hm64' [K, H, W] float64, 'anno64' [max_objs, 10] float64 (fp32-exact columns hold fp32 values), 'ind',
    'mask', 'cat', 'radius' and 'obj' (per slot, -1 where nothing is drawn)}.  radius_fn / splat_fn let the fixture maker drive the reference's own
    functions with this loop."""
    boxes = np.asarray(boxes, np.float32)
    classes = np.asarray(classes)
    lo = geometry(W, H)
    out, first = [], 0
    for K in tasks:
        order = [i for c in range(K) for i in range(len(classes)) if classes[i] == first + c + 1]        # class-major, input order
        first += K
        hm = np.zeros((K, H, W), hm_dtype)
        anno = np.zeros((max_objs, 10), np.float64)
        ind, cat = np.zeros(max_objs, np.int64), np.zeros(max_objs, np.int64)
        mask, radius, who = np.zeros(max_objs, np.uint8), np.full(max_objs, -1, np.int64), np.full(max_objs, -1, np.int64)
        for k, i in enumerate(order[:max_objs]):
            b = boxes[i]
            cls = int(classes[i]) - 1 - (first - K)
            w, l, cx, cy = cell_sizes(b, lo)
            if not (w > 0 and l > 0):
                continue
            r = max(min_radius, int(radius_fn(l, w, overlap)))
            x, y = int(cx), int(cy)                                      # toward zero
            if not (0 <= x < W and 0 <= y < H):
                continue
            hm[cls] = splat_fn(hm[cls], (cx, cy), r)
            rot = limit_period32(b[8])
            anno[k] = [cx - F32(x), cy - F32(y), b[2], math.log(float(b[3])), math.log(float(b[4])), math.log(float(b[5])), b[6], b[7],
                       math.sin(float(rot)), math.cos(float(rot))]
            ind[k], cat[k], mask[k], radius[k], who[k] = y * W + x, cls, 1, r, i
        out.append({"hm64": hm, "anno64": anno, "ind": ind, "mask": mask, "cat": cat, "radius": radius, "obj": who})
    return out


def assign(boxes, classes, tasks, W, H, max_objs, **kw):
    """a batch: per task the stacked frames of assign_frame"""
    frames = [assign_frame(b, c, tasks, W, H, max_objs, **kw) for b, c in zip(np.asarray(boxes), np.asarray(classes))]
    return [{k: np.stack([f[t][k] for f in frames]) for k in frames[0][t]} for t in range(len(tasks))]


def ambiguous(box, W, H, overlap=OVERLAP):
    """would an integer result of this object depend on fp32 against float64?"""
    lo = geometry(W, H)
    b = np.asarray(box, np.float32).astype(np.float64)
    w, l = b[3] / VS[0] / OSF, b[4] / VS[1] / OSF
    cx, cy = (b[0] - lo[0]) / VS[0] / OSF, (b[1] - lo[1]) / VS[1] / OSF
    if abs(cx - round(cx)) < 1e-3 or abs(cy - round(cy)) < 1e-3:
        return True
    if w > 0 and l > 0:
        r = gaussian_radius(l, w, overlap)
        return abs(r - round(r)) < 1e-3
    return False


def ulps(a, b):
    """distance in fp32 units in the last place, elementwise (both finite or equal)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


EXACT_COLS, F64_COLS = [0, 1, 2, 6, 7], [3, 4, 5, 8, 9]


def check_targets(got, want, ulp):
    """got: per task {'hm', 'anno_box', 'ind', 'mask', 'cat'} arrays; want: the oracle's tasks"""
    for t, (g, w) in enumerate(zip(got, want)):
        for k in ("ind", "mask", "cat"):
            assert g[k].dtype == w[k].dtype and np.array_equal(g[k], w[k]), (t, k)
        hm32 = w["hm64"].astype(np.float32)
        assert g["hm"].dtype == np.float32 and g["hm"].shape == hm32.shape
        assert np.array_equal(g["hm"] == 0, hm32 == 0), t
        assert int(ulps(g["hm"], hm32).max()) <= ulp, (t, int(ulps(g["hm"], hm32).max()))
        a32 = w["anno64"].astype(np.float32)
        assert g["anno_box"].dtype == np.float32 and np.array_equal(g["anno_box"][..., EXACT_COLS], a32[..., EXACT_COLS]), t
        assert int(ulps(g["anno_box"][..., F64_COLS], a32[..., F64_COLS]).max()) <= ulp, t


def obj(cx, cy, w, l, cls, rot=0.3, z=-0.7, h=1.6, vx=0.4, vy=-1.1, W=24, H=16):
    """(box row, class) of an object given in CELLS on a W x H map"""
    lo = geometry(W, H)
    return [lo[0] + cx * CELL, lo[1] + cy * CELL, z, w * CELL, l * CELL, h, vx, vy, rot], cls


def make_case(B, tasks, H, W, n, seed, n_cap=None, max_objs=None):
    """boxes float32 [B, n_cap, 9], classes int32 [B, n_cap]: n objects per frame drawn by rejection, classes over all tasks in random
    order, a tenth of the centres outside the map, the rest of the n_cap slots empty (class 0)"""
    rng = np.random.default_rng(seed)
    n_cap = n_cap or n
    ncls = sum(tasks)
    boxes, classes = np.zeros((B, n_cap, 9), np.float32), np.zeros((B, n_cap), np.int32)
    for b in range(B):
        slots = rng.permutation(n_cap)[:n]
        for s in slots:
            while True:
                row, c = obj(rng.uniform(-2, W + 2), rng.uniform(-2, H + 2), rng.uniform(0.4, 9), rng.uniform(0.4, 9), int(rng.integers(1, ncls + 1)),
                             rot=rng.uniform(-8, 8), z=rng.uniform(-3, 1), h=rng.uniform(0.5, 3), vx=rng.normal(), vy=rng.normal(), W=W, H=H)
                if not ambiguous(row, W, H):
                    break
            boxes[b, s], classes[b, s] = row, c
    return boxes, classes


EDGE_TASKS, EDGE_W, EDGE_H, EDGE_MAX_OBJS = (1, 2, 3), 24, 16, 8


def edge_case():
    """B = 3 on a 16 x 24 map, tasks (1, 2, 3), max_objs 8 -- see tests/test_gpu_centerloss.py for what has to occur.  Frame 0 is
    constructed, frame 1 drawn, frame 2 empty."""
    f0 = [
        obj(5.3, 7.6, 3.0, 2.0, 5),                     # classes out of task order: task 2 first
        obj(0.5, 0.4, 5.0, 5.0, 1), obj(23.5, 0.6, 5.0, 5.0, 1), obj(0.4, 15.5, 5.0, 5.0, 1), obj(23.6, 15.4, 5.0, 5.0, 1),       # corners
        obj(12.3, 0.4, 5.0, 5.0, 1), obj(12.6, 15.6, 5.0, 5.0, 1), obj(0.3, 8.3, 5.0, 5.0, 1), obj(23.7, 8.6, 5.0, 5.0, 1),       # edges
        obj(7.5, 7.5, 4.0, 4.0, 1), obj(16.5, 7.5, 4.0, 4.0, 1),                                                                  # slots 8, 9: dropped
        obj(11.5, 8.5, 300.0, 300.0, 3),                # a radius larger than the map
        obj(4.4, 3.3, 0.2, 0.2, 2),                     # a radius raised to min_radius
        obj(-0.5, 5.5, 2.0, 2.0, 2), obj(6.5, -0.4, 2.0, 2.0, 2),                 # centres in (-1, 0): cell 0, negative offsets
        obj(30.5, 5.5, 2.0, 2.0, 2),                    # outside the map, in the middle of task 1's slot order: a hole in mask
        obj(9.5, 9.5, 0.0, 2.0, 2),                     # w = 0
        obj(15.4, 4.6, 6.0, 6.0, 4, rot=4.0), obj(17.6, 5.3, 3.0, 3.0, 4, rot=-7.5),   # overlapping, one class; rot outside [-pi, pi)
        obj(20.3, 11.4, 2.0, 3.0, 6), obj(20.7, 11.6, 5.0, 4.0, 6),               # two objects in one cell
        obj(3.5, 12.5, 2.5, 2.5, 3),
    ]
    n_cap = 24
    boxes, classes = np.zeros((3, n_cap, 9), np.float32), np.zeros((3, n_cap), np.int32)
    for i, (row, c) in enumerate(f0):
        boxes[0, i], classes[0, i] = row, c
    rb, rc = make_case(1, EDGE_TASKS, EDGE_H, EDGE_W, 14, 7, n_cap=n_cap)
    boxes[1], classes[1] = rb[0], rc[0]
    return boxes, classes


# ------------------------------------------------------------------------------------------------------------------- the loss
REG_NAMES = ("reg", "height", "dim", "vel", "rot")
REG_CH = {"reg": 2, "height": 1, "dim": 3, "vel": 2, "rot": 2}


def loss_reference(preds, target, dtype=torch.float64, kind="logits", code_weights=None, weight=0.25):
    """CenterHead.loss of one task restated: preds {'hm', 'reg', 'height', 'dim', 'rot'[, 'vel']} (any floating type; widened to
    `dtype`), target {'hm', 'anno_box', 'ind', 'mask', 'cat'}.  Returns {'loss', 'hm_loss', 'loc_loss', 'num_pos', 'box_loss', 'grad':
    {name: d loss / d map}}."""
    x = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in preds.items()}
    hm_t = torch.as_tensor(target["hm"]).to(dtype)
    anno = torch.as_tensor(target["anno_box"]).to(dtype)
    ind, cat = torch.as_tensor(target["ind"]).long(), torch.as_tensor(target["cat"]).long()
    mask = torch.as_tensor(target["mask"]).to(dtype)
    y = torch.clamp(torch.sigmoid(x["hm"]), min=1e-4, max=1 - 1e-4) if kind == "logits" else x["hm"]
    B, K = y.shape[:2]
    neg = (torch.log(1 - y) * y ** 2 * (1 - hm_t) ** 4).sum()
    cells = y.permute(0, 2, 3, 1).reshape(B, -1, K)                    # the permuted copy the reference makes
    picked = cells.gather(1, ind[..., None].expand(-1, -1, K)).gather(2, cat[..., None])[..., 0]
    pos = (torch.log(picked) * (1 - picked) ** 2 * mask).sum()
    num_pos = mask.sum()
    hm_loss = -neg if float(num_pos) == 0 else -(pos + neg) / num_pos
    names = [n for n in REG_NAMES if n in x]
    box = torch.cat([x[n] for n in names], 1)
    ncol = box.shape[1]
    tgt = anno if ncol == 10 else anno[..., NOVEL]
    pred = box.permute(0, 2, 3, 1).reshape(B, -1, ncol).gather(1, ind[..., None].expand(-1, -1, ncol))
    box_loss = ((pred * mask[..., None] - tgt * mask[..., None]).abs() / (num_pos + 1e-4)).sum((0, 1))
    cw = torch.ones(ncol, dtype=dtype) if code_weights is None else torch.as_tensor(code_weights, dtype=dtype)
    loc_loss = (box_loss * cw).sum()
    loss = hm_loss + weight * loc_loss
    loss.backward()
    return {"loss": loss.detach(), "hm_loss": hm_loss.detach(), "loc_loss": loc_loss.detach(), "num_pos": num_pos.detach(),
            "box_loss": box_loss.detach(), "grad": {k: v.grad for k, v in x.items()}}


def make_loss_case(B, K, H, W, M, seed, vel=True, dtype=torch.float32, npos=None, duplicates=False):
    """(preds, target) of one task: a heat-map target in [0, 1] with ones at the slots' cells, logits in [-6, 6], regression
    predictions 0.05 .. 1.05 away from their targets on either side (after rounding to `dtype`: bf16 moves a value below 4.1 by less
    than 0.02)"""
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    npos = min(M, max(1, HW // 3)) if npos is None else npos
    hm_t = torch.rand((B, K, H, W), generator=g) ** 4
    ind, cat = torch.zeros((B, M), dtype=torch.int64), torch.zeros((B, M), dtype=torch.int64)
    mask = torch.zeros((B, M), dtype=torch.uint8)
    for b in range(B):
        cells = torch.randperm(HW, generator=g)[:npos] if npos <= HW else torch.randint(0, HW, (npos,), generator=g)
        if duplicates and npos >= 3:
            cells[2] = cells[0]                                          # slots 0 and 2 share a cell
            cells[npos - 1] = cells[0]
        slots = torch.sort(torch.randperm(M, generator=g)[:npos]).values # holes in the mask
        ind[b, slots], mask[b, slots] = cells, 1
        cat[b, slots] = torch.randint(0, K, (npos,), generator=g)
        hm_t[b, cat[b, slots], cells // W, cells % W] = 1.0
    anno = torch.randn((B, M, 10), generator=g) * mask[..., None]
    preds = {"hm": (torch.rand((B, K, H, W), generator=g) * 12 - 6).to(dtype)}
    chans = 0
    for name in REG_NAMES:
        if name == "vel" and not vel:
            chans += 2
            continue
        c = REG_CH[name]
        p = torch.randn((B, c, H, W), generator=g)
        cols = list(range(chans, chans + c))
        side = torch.where(torch.rand((B, M, c), generator=g) < 0.5, -1.0, 1.0) * (0.05 + torch.rand((B, M, c), generator=g))
        flat = p.reshape(B, c, HW)
        for b in range(B):
            for m in torch.nonzero(mask[b])[:, 0].tolist()[::-1]:          # the lowest slot of a shared cell decides
                flat[b, :, ind[b, m]] = anno[b, m, cols] + side[b, m]
        preds[name] = p.to(dtype)
        chans += c
    return preds, {"hm": hm_t, "anno_box": anno, "ind": ind, "mask": mask, "cat": cat}


_CACHE = {}


def yardstick(key, preds, target, **kw):
    """(r64, o32), computed once per `key` and shared; callers leave it unchanged.  o32: the oracle's own fp32 evaluation against
    float64, per scalar and per gradient tensor."""
    if key not in _CACHE:
        r64 = loss_reference(preds, target, torch.float64, **kw)
        r32 = loss_reference(preds, target, torch.float32, **kw)
        o32 = {k: rel_err(r32[k].numpy(), r64[k].numpy()) for k in ("loss", "hm_loss", "loc_loss", "box_loss")}
        o32["grad"] = {k: rel_err(r32["grad"][k].numpy(), r64["grad"][k].numpy()) for k in r64["grad"]}
        _CACHE[key] = (r64, o32)
    return _CACHE[key]
