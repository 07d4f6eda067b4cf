"""tools/roibench.py -- the second stage of a two-stage CenterPoint on the device (link_amd/roihead.py on csrc/roihead.hip) against a
torch restatement of the reference's steps on the same GPU, in the same process, at the Waymo two-stage shape: B = 4, a BEV map of
512 x 188 x 188, R = 500 proposals, M = 128 sampled, G = 200 ground-truth boxes, code 7, 5 points per box.

    timeout 900 python tools/roibench.py [--windows 7] [--calls 50] [--dtype fp32]

`steps_features`, `steps_assign`, `steps_loss` and main's `steps_train` / `steps_infer` are that restatement.  They take the steps detection/det3d/models/detectors/
two_stage.py:156-199, models/second_stage/bird_eye_view.py, models/roi_heads/target_assigner/proposal_target_layer.py and
models/roi_heads/roi_head_template.py take, in their order: a permuted contiguous copy of the map, the five points of every
proposal, the bilinear gather for all R per frame, a loop over frames and classes with one 3-D IoU call each (this project's
boxes_iou3d_gpu stands for the reference's CUDA op), nonzero and numpy draws on the host, the gathers of the sampled rows, the
canonical transform, and the loss with its two .item() calls.  They are the comparison, never the code under test.  The MLP between
features and loss is left out on both sides (the same library GEMMs): the loss is taken on fixed rcnn_cls / rcnn_reg leaves.

One JSON line per measurement: per side the per-call time of --windows windows of --calls calls each (HIP events around a window, one
synchronise per window, the sides alternating), their median and spread max - min; kernel launches per call counted by the
profiler and host round trips per call counted by torch's sync debug mode.  `layout` times link_roi_bev_features for all R
reading (a) the contiguous NCHW map in place, (b) a channels_last map in place, (c) the NCHW map after a permute copy that is part
of the timed call."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOM = {"pc_start": [-75.2, -75.2], "voxel_size": [0.1, 0.1], "out_stride": 8}
CFG = {"ROI_PER_IMAGE": 128, "FG_RATIO": 0.5, "SAMPLE_ROI_BY_EACH_CLASS": True, "CLS_SCORE_TYPE": "roi_iou", "CLS_FG_THRESH": 0.75,
       "CLS_BG_THRESH": 0.25, "CLS_BG_THRESH_LO": 0.1, "HARD_BG_RATIO": 0.8, "REG_FG_THRESH": 0.55}
CW = [1.0] * 7


def make_inputs(B, R, G, seed=0):
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, G, 8), np.float32)
    gt[..., 0:2] = rng.uniform(-70, 70, (B, G, 2))
    gt[..., 2] = rng.uniform(-1, 1, (B, G))
    gt[..., 3:6] = np.exp(rng.uniform(np.log(0.6), np.log(5.0), (B, G, 3)))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (B, G))
    gt[..., 7] = rng.integers(1, 4, (B, G))
    pick = rng.integers(0, G, (B, R))
    rois = np.take_along_axis(gt, pick[..., None], 1)[..., :7].copy()
    scale = np.float32([0.02, 0.1, 0.3, 0.8, 3.0])[np.arange(R) % 5][None, :, None]
    rois[..., :3] += (rng.standard_normal((B, R, 3)) * scale).astype(np.float32)
    rois[..., 6] += (rng.standard_normal((B, R)) * 0.2).astype(np.float32)
    labels = np.take_along_axis(gt[..., 7], pick, 1).astype(np.int64)
    labels[:, -20:], rois[:, -20:] = 0, 0                      # unused slots behind the proposals
    scores = rng.uniform(0.1, 1, (B, R)).astype(np.float32)
    return rois, labels, scores, gt


# ------------------------------------------------------------------------------------------------------------- the comparison
def _points(boxes):
    """the five points of every box [R, 7] (heading in column 6) -> [5 R, 2]"""
    c, s = torch.cos(boxes[:, 6]), torch.sin(boxes[:, 6])
    cor = []
    for nx, ny in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)):
        ux, uy = boxes[:, 3] * nx, boxes[:, 4] * ny
        cor.append(torch.stack([ux * c + uy * s + boxes[:, 0], -ux * s + uy * c + boxes[:, 1]], 1))
    return torch.cat([boxes[:, :2], (cor[0] + cor[1]) / 2, (cor[2] + cor[3]) / 2, (cor[0] + cor[3]) / 2, (cor[1] + cor[2]) / 2], 0)


def _interpolate(im, x, y):
    """im [H, W, C]"""
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = x0.clamp(0, im.shape[1] - 1), x1.clamp(0, im.shape[1] - 1)
    y0, y1 = y0.clamp(0, im.shape[0] - 1), y1.clamp(0, im.shape[0] - 1)
    wa, wb = (x1.type_as(x) - x) * (y1.type_as(y) - y), (x1.type_as(x) - x) * (y - y0.type_as(y))
    wc, wd = (x - x0.type_as(x)) * (y1.type_as(y) - y), (x - x0.type_as(x)) * (y - y0.type_as(y))
    return (im[y0, x0].t() * wa).t() + (im[y1, x0].t() * wb).t() + (im[y0, x1].t() * wc).t() + (im[y1, x1].t() * wd).t()


def steps_features(bev, rois):
    nhwc = bev.permute(0, 2, 3, 1).contiguous()
    out = []
    for b in range(bev.shape[0]):
        p = _points(rois[b])
        x = (p[:, 0] - GEOM["pc_start"][0]) / GEOM["voxel_size"][0] / GEOM["out_stride"]
        y = (p[:, 1] - GEOM["pc_start"][1]) / GEOM["voxel_size"][1] / GEOM["out_stride"]
        f = _interpolate(nhwc[b], x, y)
        n = rois.shape[1]
        out.append(torch.cat([f[i * n:(i + 1) * n] for i in range(5)], 1))
    return torch.stack(out)


def _host_sample(mo, rng):
    M = CFG["ROI_PER_IMAGE"]
    fg_per = int(np.round(CFG["FG_RATIO"] * M))
    fg = (mo >= min(CFG["REG_FG_THRESH"], CFG["CLS_FG_THRESH"])).nonzero().view(-1)
    easy = (mo < CFG["CLS_BG_THRESH_LO"]).nonzero().view(-1)
    hard = ((mo < CFG["REG_FG_THRESH"]) & (mo >= CFG["CLS_BG_THRESH_LO"])).nonzero().view(-1)

    def bg(n):
        if hard.numel() and easy.numel():
            nh = min(int(n * CFG["HARD_BG_RATIO"]), len(hard))
            return torch.cat([hard[torch.randint(0, hard.numel(), (nh,)).to(hard.device)], easy[torch.randint(0, easy.numel(), (n - nh,)).to(easy.device)]])
        src = hard if hard.numel() else easy
        return src[torch.randint(0, src.numel(), (n,)).to(src.device)]
    if fg.numel() and hard.numel() + easy.numel():
        take = min(fg_per, fg.numel())
        perm = torch.from_numpy(rng.permutation(fg.numel())).type_as(mo).long()
        return torch.cat([fg[perm[:take]], bg(M - take)])
    if fg.numel():
        return fg[torch.from_numpy(np.floor(rng.random(M) * fg.numel())).type_as(mo).long()]
    return bg(M)


def steps_assign(la, rois, labels, scores, gt, feats, rng):
    B, R, code = rois.shape
    M = CFG["ROI_PER_IMAGE"]
    o_rois, o_gt = rois.new_zeros(B, M, code), rois.new_zeros(B, M, code + 1)
    o_iou, o_scores, o_labels = rois.new_zeros(B, M), rois.new_zeros(B, M), labels.new_zeros(B, M)
    o_feats = feats.new_zeros(B, M, feats.shape[-1])
    for b in range(B):
        cur_gt = gt[b]
        k = len(cur_gt) - 1
        while k > 0 and cur_gt[k].sum() == 0:                  # a host test per trailing row
            k -= 1
        cur_gt = cur_gt[:k + 1]
        mo, ga = rois.new_zeros(R), labels.new_zeros(R)
        gl = cur_gt[:, -1].long()
        for c in range(gl.min().item(), gl.max().item() + 1):
            rm, gm = labels[b] == c, gl == c
            if rm.sum() > 0 and gm.sum() > 0:
                iou = la.boxes_iou3d_gpu(rois[b][rm][:, :7].contiguous(), cur_gt[gm][:, :7].contiguous())
                v, i = iou.max(1)
                mo[rm] = v
                ga[rm] = gm.nonzero().view(-1)[i]
        sel = _host_sample(mo, rng)
        o_rois[b], o_labels[b], o_iou[b], o_scores[b] = rois[b][sel], labels[b][sel], mo[sel], scores[b][sel]
        o_gt[b], o_feats[b] = cur_gt[ga[sel]], feats[b][sel]
    valid = (o_iou > CFG["REG_FG_THRESH"]).long()
    fgm, bgm = o_iou > CFG["CLS_FG_THRESH"], o_iou < CFG["CLS_BG_THRESH"]
    cls = fgm.float()
    mid = ~fgm & ~bgm
    cls[mid] = (o_iou[mid] - CFG["CLS_BG_THRESH"]) / (CFG["CLS_FG_THRESH"] - CFG["CLS_BG_THRESH"])
    ry = o_rois[..., 6] - torch.floor(o_rois[..., 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
    g = o_gt.clone()
    g[..., :6] -= o_rois[..., :6]
    g[..., 6] -= ry
    c, s = torch.cos(-ry), torch.sin(-ry)
    zeros, ones = torch.zeros_like(c), torch.ones_like(c)
    rot = torch.stack((c, -s, zeros, s, c, zeros, zeros, zeros, ones), -1).view(-1, 3, 3)
    g = torch.cat([torch.matmul(g.view(-1, 1, code + 1)[:, :, :3], rot), g.view(-1, 1, code + 1)[:, :, 3:]], -1).view(B, M, code + 1)
    h = g[..., 6] % (2 * np.pi)
    opp = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h[opp] = (h[opp] + np.pi) % (2 * np.pi)
    flag = h > np.pi
    h[flag] = h[flag] - 2 * np.pi
    g[..., 6] = h.clamp(-np.pi / 2, np.pi / 2)
    return o_feats, cls, g, valid


def steps_loss(rcnn_cls, rcnn_reg, cls_labels, gt_of_rois, valid):
    t = cls_labels.view(-1)
    bce = torch.nn.functional.binary_cross_entropy(torch.sigmoid(rcnn_cls.view(-1)), t, reduction="none")
    m = (t >= 0).float()
    lc = (bce * m).sum() / m.sum().clamp(min=1.0)
    fgm = valid.view(-1) > 0
    fg_sum = fgm.long().sum().item()
    l1 = torch.nn.functional.l1_loss(rcnn_reg, gt_of_rois.view(-1, gt_of_rois.shape[-1])[:, :7], reduction="none") * rcnn_reg.new_tensor(CW)
    lr = (l1 * fgm.unsqueeze(-1).float()).sum() / max(fg_sum, 1)
    total = lc + lr
    total.item()
    return total


# ----------------------------------------------------------------------------------------------------------------------- timing
def windows(sides, n_windows, calls, warmup=5):
    """{name: fn} -> {name: [per-call us of each window]}, the sides alternating"""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(n_windows):
        for name, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / calls)
    return out


def summary(v):
    s = sorted(v)
    return {"median_us": round(s[len(s) // 2], 1), "spread_us": round(s[-1] - s[0], 1), "windows_us": [round(x, 1) for x in v]}


def profile(fn):
    """(kernel launches, device-to-host copies) of one call, or (None, None)"""
    try:
        from torch.profiler import ProfilerActivity, profile as prof_ctx
        fn()
        torch.cuda.synchronize()
        with prof_ctx(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = d2h = 0
        for e in prof.events():
            if not str(getattr(e, "device_type", "")).endswith("CUDA"):
                continue
            low = e.name.lower()
            if "memcpy" in low:
                d2h += "dtoh" in low or "device -> host" in low or "devicetohost" in low
            elif "memset" not in low:
                n += 1
        return (n, d2h) if n else (None, None)
    except Exception:
        return None, None


def host_round_trips(fn):
    """synchronising torch operations of one call (.item(), nonzero, boolean indexing, copies to the host), counted by torch's
    sync debug mode; None where that mode is not available"""
    import warnings
    try:
        fn()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(w.message).lower() for w in seen)
    except Exception:
        return None
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--size", type=int, default=188)
    ap.add_argument("--rois", type=int, default=500)
    ap.add_argument("--gt", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "bf16"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roibench: no GPU visible; timings are taken on the device only")
    import link_amd as la
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    B, C, S, R, G, M = a.batch, a.channels, a.size, a.rois, a.gt, CFG["ROI_PER_IMAGE"]
    shape = {"batch": B, "channels": C, "map": [S, S], "rois": R, "sampled": M, "gt": G, "dtype": a.dtype, "windows": a.windows, "calls": a.calls}
    rois_np, labels_np, scores_np, gt_np = make_inputs(B, R, G)
    dev = "cuda"
    rois, labels, scores, gt = (torch.from_numpy(v).to(dev) for v in (rois_np, labels_np, scores_np, gt_np))
    bev = torch.randn((B, C, S, S), generator=torch.Generator().manual_seed(1)).to(dev).to(dt)
    bev_cl = bev.contiguous(memory_format=torch.channels_last)
    ext = la.BEVFeatureExtractor(**GEOM)
    layer = la.ProposalTargetLayer(CFG, generator=torch.Generator(device=dev).manual_seed(2))
    rcnn_cls = torch.randn(B * M, device=dev, dtype=dt, requires_grad=True)
    rcnn_reg = torch.randn(B * M, 7, device=dev, dtype=dt, requires_grad=True)
    rcnn_cls_all, rcnn_reg_all = torch.randn(B * R, device=dev, dtype=dt), torch.randn(B * R, 7, device=dev, dtype=dt)
    batch = {"rois": rois, "roi_labels": labels, "roi_scores": scores, "gt_boxes_and_cls": gt}
    rng = np.random.default_rng(3)

    # ---- layout ------------------------------------------------------------------------------------------------------------
    la.roihead.NCHW_IN_PLACE = True
    same = torch.equal(ext.extract(bev, rois, labels, None, 5, rot_col=6), ext.extract(bev_cl, rois, labels, None, 5, rot_col=6))
    lay = windows({"nchw_in_place": lambda: ext.extract(bev, rois, labels, None, 5, rot_col=6),
                   "channels_last_in_place": lambda: ext.extract(bev_cl, rois, labels, None, 5, rot_col=6),
                   "nchw_permute_copy": lambda: ext.extract(bev.contiguous(memory_format=torch.channels_last), rois, labels, None, 5, rot_col=6)},
                  a.windows, a.calls)
    sel = layer(batch)["sel"]
    lay_s = windows({"nchw_in_place": lambda: ext.extract(bev, rois, labels, sel, 5, rot_col=6),
                     "channels_last_in_place": lambda: ext.extract(bev_cl, rois, labels, sel, 5, rot_col=6)}, a.windows, a.calls)
    print(json.dumps({"what": "layout: features of all R", **shape, "same_bits": bool(same), **{k: summary(v) for k, v in lay.items()}}), flush=True)
    print(json.dumps({"what": "layout: features of the M sampled rows", **shape, **{k: summary(v) for k, v in lay_s.items()}}), flush=True)

    # ---- training ------------------------------------------------------------------------------------------------------------
    def fused_train():
        rcnn_cls.grad = rcnn_reg.grad = None
        t = layer(batch)
        feats = ext.extract(bev, rois, labels, t["sel"], 5, rot_col=6)
        total = la.roi_loss(rcnn_cls, rcnn_reg, t["rcnn_cls_labels"], t["gt_of_rois_canonical"], t["reg_valid_mask"], CW)[0]
        total.backward()
        return feats

    def steps_train():
        rcnn_cls.grad = rcnn_reg.grad = None
        feats = steps_features(bev, rois)
        f, cls_l, g, valid = steps_assign(la, rois, labels, scores, gt, feats, rng)
        steps_loss(rcnn_cls, rcnn_reg, cls_l, g, valid).backward()
        return f
    tr = windows({"fused": fused_train, "steps": steps_train}, a.windows, max(a.calls // 5, 10))
    kf, ks = profile(fused_train)[0], profile(steps_train)[0]
    hf, hs = host_round_trips(fused_train), host_round_trips(steps_train)
    mf, ms = summary(tr["fused"]), summary(tr["steps"])
    print(json.dumps({"what": "training second-stage step: assign + features + loss forward and backward (no MLP)", **shape,
                      "calls_per_window": max(a.calls // 5, 10), "fused": mf, "steps": ms, "speedup": round(ms["median_us"] / mf["median_us"], 2),
                      "faster_by_more_than_spread": bool(ms["median_us"] - mf["median_us"] > max(ms["spread_us"], mf["spread_us"])),
                      "fused_launches": kf, "steps_launches": ks, "fused_host_round_trips": hf, "steps_host_round_trips": hs}), flush=True)

    # ---- inference -----------------------------------------------------------------------------------------------------------
    def fused_infer():
        feats = ext.extract(bev, rois, labels, None, 5, rot_col=6)
        return feats, la.roi_refine(rois, labels, scores, rcnn_cls_all, rcnn_reg_all)

    def steps_infer():
        feats = steps_features(bev, rois)
        local = rois.clone()
        local[..., :3] = 0
        v = (rcnn_reg_all.float().view(B, R, 7) + local).view(-1, 7)
        c, s = torch.cos(rois[..., 6].view(-1)), torch.sin(rois[..., 6].view(-1))
        zeros, ones = torch.zeros_like(c), torch.ones_like(c)
        rot = torch.stack((c, -s, zeros, s, c, zeros, zeros, zeros, ones), 1).view(-1, 3, 3)
        v = torch.cat([torch.matmul(v[:, None, :3], rot)[:, 0], v[:, 3:]], 1)
        v[:, :3] += rois[..., :3].reshape(-1, 3)
        v = v.view(B, R, 7)
        out = []
        for b in range(B):
            sc = torch.sqrt(torch.sigmoid(rcnn_cls_all.float().view(B, R)[b]) * scores[b])
            m = labels[b] != 0
            out.append((v[b][m], sc[m], labels[b][m] - 1))    # boolean masks: one host round trip each
        return feats, out
    inf = windows({"fused": fused_infer, "steps": steps_infer}, a.windows, a.calls)
    kf, ks = profile(fused_infer)[0], profile(steps_infer)[0]
    hf, hs = host_round_trips(fused_infer), host_round_trips(steps_infer)
    mf, ms = summary(inf["fused"]), summary(inf["steps"])
    print(json.dumps({"what": "inference: features of all R + refine", **shape, "fused": mf, "steps": ms,
                      "speedup": round(ms["median_us"] / mf["median_us"], 2),
                      "faster_by_more_than_spread": bool(ms["median_us"] - mf["median_us"] > max(ms["spread_us"], mf["spread_us"])),
                      "fused_launches": kf, "steps_launches": ks, "fused_host_round_trips": hf, "steps_host_round_trips": hs}), flush=True)


if __name__ == "__main__":
    main()
