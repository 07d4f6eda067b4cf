"""tests/roi_oracle.py -- checkers of the two-stage ROI head (csrc/roihead.hip, section O of include/link_amd.h), in numpy.  Test
infrastructure only.

Restatements, in float32 (every product and sum rounded on its own, cos / sin computed in double and rounded once) or in float64, of
detection/det3d/models/detectors/two_stage.py:51-78 (get_box_center) and :123-153 (post_process), core/utils/center_utils.py:92-121
(bilinear_interpolate_torch) behind models/second_stage/bird_eye_view.py, models/roi_heads/target_assigner/proposal_target_layer.py,
and models/roi_heads/roi_head_template.py:43-86 (assign_targets), :88-151 (get_loss), :153-183 (generate_predicted_boxes).  The
rotated overlap is tests/box_oracle.py's.  The sampler draws from a `noise` array the way section O defines it.
"""
import numpy as np

import box_oracle as BO

CFG = {"ROI_PER_IMAGE": 128, "FG_RATIO": 0.5, "SAMPLE_ROI_BY_EACH_CLASS": True, "CLS_SCORE_TYPE": "roi_iou", "CLS_FG_THRESH": 0.75,
       "CLS_BG_THRESH": 0.25, "CLS_BG_THRESH_LO": 0.1, "HARD_BG_RATIO": 0.8, "REG_FG_THRESH": 0.55}          # the Waymo two-stage configs


def _t(dtype):
    return np.dtype(dtype).type


def _trig(h, dt):
    return np.cos(h.astype(np.float64)).astype(dt), np.sin(h.astype(np.float64)).astype(dt)


# ---- O1 -----------------------------------------------------------------------------------------------------------------------------
def box_points(boxes, num_point, dtype=np.float32, rot_col=-1):
    """get_box_center for one frame: boxes [R, L] -> [num_point, R, 2] (x, y of the centre, front, back, left, right)"""
    dt = _t(dtype)
    b = np.asarray(boxes).astype(dt)
    ctr = b[:, :2]
    if num_point == 1:
        return ctr[None]
    c, s = _trig(b[:, rot_col], dt)
    half = dt(0.5)
    norm = [(-half, -half), (-half, half), (half, half), (half, -half)]
    cor = []
    for nx, ny in norm:
        ux, uy = b[:, 3] * nx, b[:, 4] * ny
        cor.append(np.stack([(ux * c + uy * s) + b[:, 0], (ux * -s + uy * c) + b[:, 1]], 1))
    two = dt(2)
    mids = [(cor[0] + cor[1]) / two, (cor[2] + cor[3]) / two, (cor[0] + cor[3]) / two, (cor[1] + cor[2]) / two]
    return np.stack([ctr] + mids)


def map_coords(xy, pc_start, voxel_size, out_stride, dtype=np.float32):
    dt = _t(dtype)
    xy = np.asarray(xy).astype(dt)
    x = (xy[..., 0] - dt(pc_start[0])) / dt(voxel_size[0]) / dt(out_stride)
    y = (xy[..., 1] - dt(pc_start[1])) / dt(voxel_size[1]) / dt(out_stride)
    return x, y


def bilinear(im, x, y, dtype=np.float32):
    """bilinear_interpolate_torch: im [H, W, C], x / y [N] -> [N, C]"""
    dt = _t(dtype)
    im = np.asarray(im).astype(dt)
    x, y = np.asarray(x).astype(dt), np.asarray(y).astype(dt)
    H, W = im.shape[:2]
    with np.errstate(all="ignore"):
        xf = np.clip(np.nan_to_num(np.floor(x), nan=-2.0), -2, W).astype(np.int64)
        yf = np.clip(np.nan_to_num(np.floor(y), nan=-2.0), -2, H).astype(np.int64)
    x0, x1 = np.clip(xf, 0, W - 1), np.clip(xf + 1, 0, W - 1)
    y0, y1 = np.clip(yf, 0, H - 1), np.clip(yf + 1, 0, H - 1)
    wa = (x1.astype(dt) - x) * (y1.astype(dt) - y)
    wb = (x1.astype(dt) - x) * (y - y0.astype(dt))
    wc = (x - x0.astype(dt)) * (y1.astype(dt) - y)
    wd = (x - x0.astype(dt)) * (y - y0.astype(dt))
    return ((im[y0, x0] * wa[:, None] + im[y1, x0] * wb[:, None]) + im[y0, x1] * wc[:, None]) + im[y1, x1] * wd[:, None]


def bev_features(bev, boxes, labels=None, sel=None, num_point=5, pc_start=(0.0, 0.0), voxel_size=(1.0, 1.0), out_stride=1.0,
                 dtype=np.float32, rot_col=-1):
    """link_roi_bev_features: bev [B, C, H, W], boxes [B, R, L] -> [B, S, num_point C]"""
    dt = _t(dtype)
    bev, boxes = np.asarray(bev), np.asarray(boxes)
    B, C = bev.shape[:2]
    R = boxes.shape[1]
    S = R if sel is None else np.asarray(sel).shape[1]
    out = np.zeros((B, S, num_point * C), dt)
    for b in range(B):
        if R == 0:
            continue
        pts = box_points(boxes[b], num_point, dtype, rot_col)
        im = np.transpose(bev[b], (1, 2, 0))
        src = np.arange(R) if sel is None else np.asarray(sel)[b]
        ok = (src >= 0) & (src < R)
        safe = np.where(ok, src, 0)
        if labels is not None:
            ok &= np.asarray(labels)[b][safe] != 0
        for p in range(num_point):
            x, y = map_coords(pts[p][safe], pc_start, voxel_size, out_stride, dtype)
            f = bilinear(im, x, y, dtype)
            out[b, :, p * C:(p + 1) * C] = np.where(ok[:, None], f, dt(0))
    return out


# ---- O2 -----------------------------------------------------------------------------------------------------------------------------
def to_pcdet(b, dt):
    b = np.asarray(b).astype(dt)[:, [0, 1, 2, 4, 3, 5, 6]].copy()
    b[:, 6] = -b[:, 6] - dt(np.pi / 2)
    return b


def iou3d(a, b, dtype=np.float32):
    """boxes_iou3d_gpu (iou3d_nms_utils.py:35-72): a [N, 7], b [M, 7] -> [N, M]"""
    dt = _t(dtype)
    a, b = to_pcdet(a, dt), to_pcdet(b, dt)
    two = dt(2)
    amax, amin = (a[:, 2] + a[:, 5] / two)[:, None], (a[:, 2] - a[:, 5] / two)[:, None]
    bmax, bmin = (b[:, 2] + b[:, 5] / two)[None], (b[:, 2] - b[:, 5] / two)[None]
    bev = BO.pairs_matrix(BO.box_overlap, a, b, dtype=dtype).astype(dt).reshape(a.shape[0], b.shape[0])
    oh = np.maximum(np.minimum(amax, bmax) - np.maximum(amin, bmin), dt(0))
    o3 = bev * oh
    va, vb = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
    return o3 / np.maximum(va + vb - o3, dt(1e-6))


def cut_gt(gt, ncol, dtype=np.float32):
    """proposal_target_layer.py:107-111: trailing rows whose sum is 0 leave, one row stays, a row of zeros serves when there is none"""
    gt = np.asarray(gt, np.float32).reshape(-1, ncol)
    if gt.shape[0] == 0:
        return np.zeros((1, ncol), np.float32)
    k = gt.shape[0] - 1
    while k > 0 and gt[k].sum() == 0:
        k -= 1
    return gt[:k + 1]


def max_overlaps(rois, roi_labels, gt, by_class, dtype=np.float32, return_matrix=False):
    """one frame: rois [R, code], gt [n, code + 1] (already cut) -> (max_overlaps [R], gt_assignment [R])"""
    dt = _t(dtype)
    iou = iou3d(np.asarray(rois)[:, :7], gt[:, :7], dtype)
    R = iou.shape[0]
    if by_class:
        match = np.asarray(roi_labels)[:, None] == gt[:, -1].astype(np.int64)[None]
        masked = np.where(match, iou, -np.inf)
        arg = masked.argmax(1)                               # the first of equals
        mo = masked[np.arange(R), arg]
        none = ~match.any(1)
        mo, arg = np.where(none, dt(0), mo).astype(dt), np.where(none, 0, arg)
    else:
        arg = iou.argmax(1)
        mo = iou[np.arange(R), arg]
    return (mo, arg.astype(np.int32), iou) if return_matrix else (mo, arg.astype(np.int32))


def sample_lists(mo, cfg):
    """the three ordered lists of subsample_rois, thresholds as a float32 tensor op sees them"""
    f = lambda k: np.asarray(cfg[k], mo.dtype)
    fg_thresh = np.asarray(min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"]), mo.dtype)
    with np.errstate(invalid="ignore"):
        fg = np.nonzero(mo >= fg_thresh)[0]
        easy = np.nonzero(mo < f("CLS_BG_THRESH_LO"))[0]
        hard = np.nonzero((mo < f("REG_FG_THRESH")) & (mo >= f("CLS_BG_THRESH_LO")))[0]
    return fg, hard, easy


def sample_counts(nfg, nhard, neasy, cfg):
    """(fg without replacement, fg with replacement, hard, easy) slots of one frame, as subsample_rois / sample_bg_inds count them"""
    M = int(cfg["ROI_PER_IMAGE"])
    fg_per_image = int(np.round(cfg["FG_RATIO"] * M))
    nbg = nhard + neasy
    if nfg > 0 and nbg > 0:
        take, repl, bg = min(fg_per_image, nfg), 0, M - min(fg_per_image, nfg)
    elif nfg > 0:
        take, repl, bg = 0, M, 0
    elif nbg > 0:
        take, repl, bg = 0, 0, M
    else:
        return None
    if nhard > 0 and neasy > 0:
        nh = min(int(bg * cfg["HARD_BG_RATIO"]), nhard)
    elif nhard > 0:
        nh = bg
    else:
        nh = 0
    return take, repl, nh, bg - nh


def sample(mo, noise, cfg):
    """link_roi_assign's draw for one frame: noise [R + M] -> (sel int32 [M], status)"""
    M, R = int(cfg["ROI_PER_IMAGE"]), mo.shape[0]
    fg, hard, easy = sample_lists(mo, cfg)
    counts = sample_counts(len(fg), len(hard), len(easy), cfg)
    sel = np.zeros(M, np.int32)
    if counts is None:
        return sel, 1
    take, repl, nh, ne = counts
    noise = np.asarray(noise, np.float32)
    if take:
        order = np.lexsort((fg, noise[fg]))                  # by key, ties by index
        sel[:take] = fg[order[:take]]

    def draw(j, lst):
        n = len(lst)
        return lst[np.minimum(np.floor(noise[R + j] * np.float32(n)).astype(np.int64), n - 1)]
    j = np.arange(M)
    if repl:
        sel[:repl] = draw(j[:repl], fg)
    s0 = take + repl
    if nh:
        sel[s0:s0 + nh] = draw(j[s0:s0 + nh], hard)
    if ne:
        sel[s0 + nh:] = draw(j[s0 + nh:], easy)
    return sel, 0


def limit_period(v, dt, offset=0.5, period=2 * np.pi):
    return v - np.floor(v / dt(period) + dt(offset)) * dt(period)


def canonical(rois, gt_src, dtype=np.float32):
    """assign_targets (roi_head_template.py:52-82): rois [N, code], gt_src [N, code + 1] -> gt_of_rois [N, code + 1]"""
    dt = _t(dtype)
    r, g = np.asarray(rois).astype(dt), np.asarray(gt_src).astype(dt).copy()
    code = r.shape[1]
    ry = limit_period(r[:, 6], dt)
    g[:, :6] = g[:, :6] - r[:, :6]
    g[:, 6] = g[:, 6] - ry
    c, s = _trig(-ry, dt)
    x, y = g[:, 0].copy(), g[:, 1].copy()
    g[:, 0] = x * c + y * s
    g[:, 1] = x * -s + y * c
    if code == 9:
        g[:, 7:9] = g[:, 7:9] - r[:, 7:9]
    p2, pi = dt(2 * np.pi), dt(np.pi)
    h = np.mod(g[:, 6], p2)
    opp = (h > dt(np.pi * 0.5)) & (h < dt(np.pi * 1.5))
    h = np.where(opp, np.mod(h + pi, p2), h)
    h = np.where(h > pi, h - p2, h)
    g[:, 6] = np.clip(h, dt(-np.pi / 2), dt(np.pi / 2))
    return g


def cls_labels(iou, cfg):
    dt = iou.dtype.type
    fg_t, bg_t = dt(cfg["CLS_FG_THRESH"]), dt(cfg["CLS_BG_THRESH"])
    if cfg["CLS_SCORE_TYPE"] == "cls":
        lab = (iou > fg_t).astype(dt)
        lab[(iou > bg_t) & (iou < fg_t)] = -1
        return lab
    fg, bg = iou > fg_t, iou < bg_t
    lab = fg.astype(dt)
    mid = ~fg & ~bg
    lab[mid] = (iou[mid] - bg_t) / dt(cfg["CLS_FG_THRESH"] - cfg["CLS_BG_THRESH"])
    return lab


def assign(rois, roi_labels, roi_scores, gt, cfg, noise=None, sel_in=None, dtype=np.float32):
    """link_roi_assign for a batch: rois [B, R, code], gt [B, G, code + 1], noise [B, R + M] or sel_in [B, M] -> dict of arrays"""
    dt = _t(dtype)
    rois, roi_labels, roi_scores = np.asarray(rois, np.float32), np.asarray(roi_labels), np.asarray(roi_scores, np.float32)
    B, R, code = rois.shape
    M = int(cfg["ROI_PER_IMAGE"])
    out = {"max_overlaps": np.zeros((B, R), dt), "gt_assignment": np.zeros((B, R), np.int32), "sel": np.zeros((B, M), np.int32),
           "rois": np.zeros((B, M, code), np.float32), "roi_labels": np.zeros((B, M), np.int64), "roi_scores": np.zeros((B, M), np.float32),
           "gt_iou_of_rois": np.zeros((B, M), dt), "gt_of_rois_src": np.zeros((B, M, code + 1), np.float32),
           "gt_of_rois": np.zeros((B, M, code + 1), dt), "status": np.zeros(B, np.int32)}
    for b in range(B):
        g = cut_gt(np.asarray(gt)[b] if np.asarray(gt).size else np.zeros((0, code + 1)), code + 1)
        mo, ga = max_overlaps(rois[b], roi_labels[b], g, cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False), dtype)
        out["max_overlaps"][b], out["gt_assignment"][b] = mo, ga
        if sel_in is not None:
            sel, st = np.asarray(sel_in)[b].astype(np.int32), 0
        else:
            sel, st = sample(mo.astype(np.float32) if dtype == np.float32 else mo, noise[b], cfg)
        out["sel"][b], out["status"][b] = sel, st
        out["rois"][b], out["roi_labels"][b], out["roi_scores"][b] = rois[b][sel], roi_labels[b][sel], roi_scores[b][sel]
        out["gt_iou_of_rois"][b] = mo[sel]
        out["gt_of_rois_src"][b] = g[ga[sel]]
        out["gt_of_rois"][b] = canonical(rois[b][sel], g[ga[sel]], dtype)
    iou = out["gt_iou_of_rois"]
    out["reg_valid_mask"] = (iou > dt(cfg["REG_FG_THRESH"])).astype(np.int64)
    out["rcnn_cls_labels"] = cls_labels(iou, cfg)
    return out


# ---- O3 -----------------------------------------------------------------------------------------------------------------------------
def loss(cls, reg, labels, gt_of_rois, reg_valid, code_weights, cls_weight, reg_weight, dtype=np.float32):
    """get_loss with BinaryCrossEntropy / L1 -> {'out': [total, cls, reg, fg_sum], 'grad_cls': [N], 'grad_reg': [N, code]}"""
    dt = _t(dtype)
    x, r, t = np.asarray(cls).astype(dt).reshape(-1), np.asarray(reg).astype(dt), np.asarray(labels).astype(dt).reshape(-1)
    N, code = r.shape
    g = np.asarray(gt_of_rois).astype(dt).reshape(N, -1)[:, :code]
    with np.errstate(all="ignore"):
        p = dt(1) / (dt(1) + np.exp(-x))
        lp, lq = np.maximum(np.log(p), dt(-100)), np.maximum(np.log1p(-p), dt(-100))
        bce = (t - dt(1)) * lq - t * lp
        pq = (dt(1) - p) * p
        gb = ((p - t) / np.maximum(pq, dt(1e-12))) * pq
    valid = t >= 0
    vden = dt(max(int(valid.sum()), 1))
    lc = np.where(valid, bce, dt(0)).sum(dtype=dt) / vden * dt(cls_weight)
    fg = np.asarray(reg_valid).reshape(-1) > 0
    fden = dt(max(int(fg.sum()), 1))
    cw = np.asarray(code_weights).astype(dt)
    d = r - g
    lr = (np.abs(d) * cw * fg[:, None]).sum(dtype=dt) / fden * dt(reg_weight)
    return {"out": np.array([lc + lr, lc, lr, dt(fg.sum())], dt), "grad_cls": np.where(valid, gb, dt(0)) / vden * dt(cls_weight),
            "grad_reg": np.sign(d) * cw * fg[:, None] / fden * dt(reg_weight)}


# ---- O4 -----------------------------------------------------------------------------------------------------------------------------
def refine(rois, roi_labels, roi_scores, cls, reg, dtype=np.float32):
    """generate_predicted_boxes + post_process, padded: -> (boxes [B, R, code], scores [B, R], labels int64 [B, R], counts int32 [B])"""
    dt = _t(dtype)
    rois, reg = np.asarray(rois).astype(dt), np.asarray(reg).astype(dt)
    B, R, code = rois.shape
    reg, cls = reg.reshape(B, R, code), np.asarray(cls).astype(dt).reshape(B, R)
    local = rois.copy()
    local[..., :3] = 0
    v = reg + local
    c, s = _trig(rois[..., 6], dt)
    x, y = v[..., 0].copy(), v[..., 1].copy()
    v[..., 0] = (x * c + y * s) + rois[..., 0]
    v[..., 1] = (x * -s + y * c) + rois[..., 1]
    v[..., 2] = v[..., 2] + rois[..., 2]
    if code == 9:
        v = v[..., [0, 1, 2, 3, 4, 5, 7, 8, 6]]
    with np.errstate(all="ignore"):
        sc = np.sqrt(dt(1) / (dt(1) + np.exp(-cls)) * np.asarray(roi_scores).astype(dt))
    ob, os_ = np.zeros((B, R, code), dt), np.zeros((B, R), dt)
    ol, cnt = np.full((B, R), -1, np.int64), np.zeros(B, np.int32)
    for b in range(B):
        m = np.asarray(roi_labels)[b] != 0
        k = int(m.sum())
        ob[b, :k], os_[b, :k], ol[b, :k], cnt[b] = v[b][m], sc[b][m], np.asarray(roi_labels)[b][m] - 1, k
    return ob, os_, ol, cnt
