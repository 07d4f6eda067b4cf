"""tools/centerloss_bench.py -- CenterHead training on the device (link_amd.CenterTargetAssigner + link_amd.CenterHeadLoss:
csrc/centerloss.hip) against a torch restatement of the reference's loss code on the same GPU, in the same process: the targets of a
batch, then the six-task loss forward + backward, at the nuScenes shape (B = 4, tasks (1, 2, 2, 1, 2, 2), 180 x 180, max_objs 500,
about 50 objects per frame).

    timeout 600 python tools/centerloss_bench.py [--dtypes fp32 fp16] [--warmup 10] [--calls 50] [--repeats 5]

`torch_steps_loss` below is that restatement.  It takes the steps det3d/models/bbox_heads/center_head.py:248-293 and
det3d/models/losses/centernet_loss.py take, in their order: an in-place sigmoid and a clamp, the focal loss over the map with a
permuted copy of it for the gather and a host test of the number of positives, a torch.cat of the five regression maps, a permuted
copy of that, a gather, the masked L1, and two results per task copied to the host.  It is the comparison, never the code under
test.  The reference builds its targets on the host (a numpy loop over objects per sample, in the data loader): `host_assign` below
restates that loop and is timed on the host, reported on a line of its own; the comparison's loss is timed on targets that are
already on the device.

Per dtype one JSON line: the median of --calls timed calls (HIP events around the call, one synchronise per call), repeated
--repeats times for both sides -- the five medians, their median and the spread max - min -- for `fused` (assign + loss forward +
backward), `fused_loss` (loss forward + backward alone, what the comparison times) and `steps`; the speed-up fused_loss against
steps and whether it exceeds the comparison's spread; kernel launches per call and host round trips per call (copies to the host
and host tests, counted by the profiler as device-to-host copies); the map pass's achieved bytes/s against the HBM peak bench.py's
roofline uses."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0   # as bench.py
TASKS = (1, 2, 2, 1, 2, 2)
CW = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]
REG = ("reg", "height", "dim", "vel", "rot")
REG_CH = {"reg": 2, "height": 1, "dim": 3, "vel": 2, "rot": 2}


def _cells_of(feat, ind):
    """[B, C, H, W] -> a channels-last copy -> the rows at ind [B, M]: [B, M, C]"""
    rows = feat.permute(0, 2, 3, 1).contiguous()
    rows = rows.view(rows.size(0), -1, rows.size(3))
    return rows.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), rows.size(2)))


def torch_steps_loss(example, preds, weight=0.25, code_weights=CW):
    """The comparison: the steps of the reference's loss in the order it takes them, in this project's own words."""
    losses, host = [], []
    for t, p in enumerate(preds):
        y = torch.clamp(p["hm"].sigmoid(), min=1e-4, max=1 - 1e-4)           # (the reference's sigmoid is in place)
        target, ind, cat = example["hm"][t], example["ind"][t], example["cat"][t]
        mask = example["mask"][t].float()
        neg = (torch.log(1 - y) * torch.pow(y, 2) * torch.pow(1 - target, 4)).sum()
        at_peaks = _cells_of(y, ind).gather(2, cat.unsqueeze(2))
        n_pos = mask.sum()
        pos = (torch.log(at_peaks) * torch.pow(1 - at_peaks, 2) * mask.unsqueeze(2)).sum()
        hm_loss = -neg if bool(n_pos == 0) else -(pos + neg) / n_pos        # the host asks the device for the count
        box = torch.cat([p[n] for n in REG], dim=1)
        picked = _cells_of(box, ind)
        m3 = mask.unsqueeze(2)
        per = torch.nn.functional.l1_loss(picked * m3, example["anno_box"][t] * m3, reduction="none") / (m3.sum() + 1e-4)
        per = per.transpose(2, 0).sum(dim=2).sum(dim=1)
        loc = (per * per.new_tensor(code_weights)).sum()
        losses.append(hm_loss + weight * loc)
        host.append((hm_loss.detach().cpu(), per.detach().cpu()))            # two results per task go to the host
    return losses, host


def host_assign(boxes, classes, tasks, W, H, lo, vs, osf, overlap, max_objs, min_radius):
    """The reference's target assignment restated: a numpy loop over the objects of one sample (fp32 boxes [n, 9], classes [n])."""
    out, first = [], 0
    rot = boxes[:, 8] - np.floor(boxes[:, 8] / np.float32(2 * np.pi) + np.float32(0.5)) * np.float32(2 * np.pi)
    for K in tasks:
        order = np.concatenate([np.where(classes == first + c + 1)[0] for c in range(K)])
        hm = np.zeros((K, H, W), np.float32)
        anno, ind = np.zeros((max_objs, 10), np.float32), np.zeros(max_objs, np.int64)
        mask, cat = np.zeros(max_objs, np.uint8), np.zeros(max_objs, np.int64)
        for k, i in enumerate(order[:max_objs]):
            b = boxes[i]
            w, l = b[3] / vs[0] / osf, b[4] / vs[1] / osf
            if not (w > 0 and l > 0):
                continue
            s, p = l + w, l * w
            r = min((s + np.sqrt(s * s - 4 * p * (1 - overlap) / (1 + overlap))) / 2, (2 * s + np.sqrt(4 * s * s - 16 * (1 - overlap) * p)) / 2,
                    (-2 * overlap * s + np.sqrt(4 * overlap * overlap * s * s - 16 * overlap * (overlap - 1) * p)) / 2)
            r = max(min_radius, int(r))
            ct = np.array([(b[0] - lo[0]) / vs[0] / osf, (b[1] - lo[1]) / vs[1] / osf], np.float32)
            x, y = int(ct[0]), int(ct[1])
            if not (0 <= x < W and 0 <= y < H):
                continue
            yy, xx = np.ogrid[-r:r + 1, -r:r + 1]
            sigma = (2 * r + 1) / 6
            g = np.exp(-(xx * xx + yy * yy) / (2 * sigma * sigma))
            left, right, top, bottom = min(x, r), min(W - x, r + 1), min(y, r), min(H - y, r + 1)
            cls = classes[i] - 1 - first
            window = hm[cls, y - top:y + bottom, x - left:x + right]
            np.maximum(window, g[r - top:r + bottom, r - left:r + right], out=window)
            ind[k], mask[k], cat[k] = y * W + x, 1, cls
            anno[k] = np.concatenate((ct - (x, y), b[2], np.log(b[3:6]), b[6], b[7], np.sin(rot[i]), np.cos(rot[i])), axis=None)
        first += K
        out.append((hm, anno, ind, mask, cat))
    return out


def _time_calls(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def _profile(fn):
    """(kernel launches, device-to-host copies, {kernel name: us}) of one call, or (None, None, None)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n, d2h, per = 0, 0, {}
        for e in prof.events():
            if not str(getattr(e, "device_type", "")).endswith("CUDA"):
                continue
            low = e.name.lower()
            if "memcpy" in low:
                d2h += "dtoh" in low or "device -> host" in low or "devicetohost" in low
            elif "memset" not in low:
                n += 1
                per[e.name] = per.get(e.name, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
        return (n, d2h, per) if n else (None, None, None)
    except Exception:
        return None, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"], choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=180)
    ap.add_argument("--objects", type=int, default=50)
    ap.add_argument("--max-objs", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import link_amd as la
    import centerloss_oracle as CO
    B, S, M = a.batch, a.size, a.max_objs
    boxes, classes = CO.make_case(B, TASKS, S, S, a.objects, 1, n_cap=a.objects + 14)
    geo = CO.geometry(S, S)
    assigner = la.CenterTargetAssigner(TASKS, CO.OSF, CO.VS, geo, CO.OVERLAP, M, CO.MIN_RADIUS)
    crit = la.CenterHeadLoss(TASKS, 0.25, CW)
    gb, gc = torch.from_numpy(boxes).cuda(), torch.from_numpy(classes).cuda()
    example = assigner(gb, gc)
    # the host loop, per batch
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        host = [host_assign(boxes[b], classes[b], TASKS, S, S, np.float32(geo[:2]), np.float32(CO.VS), CO.OSF, CO.OVERLAP, M, CO.MIN_RADIUS)
                for b in range(B)]
        ts.append((time.perf_counter() - t0) * 1e6)
    same = all(np.array_equal(np.stack([host[b][t][2] for b in range(B)]), example["ind"][t].cpu().numpy()) and
               np.abs(np.stack([host[b][t][0] for b in range(B)]) - example["hm"][t].cpu().numpy()).max() < 1e-6 for t in range(len(TASKS)))
    fa = sorted(_time_calls(lambda: assigner(gb, gc), a.warmup, a.calls) for _ in range(a.repeats))
    print(json.dumps({"what": "assign", "batch": B, "map": [S, S], "objects_per_frame": a.objects, "max_objs": M,
                      "host_numpy_loop_us_per_batch": round(sorted(ts)[len(ts) // 2], 1), "device_us_per_batch": round(fa[len(fa) // 2], 1),
                      "device_medians_us": [round(v, 1) for v in fa], "device_launches": 2, "same_targets": bool(same)}), flush=True)
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    g = torch.Generator().manual_seed(0)
    base = []
    for K in TASKS:
        d = {"hm": torch.rand((B, K, S, S), generator=g) * 8 - 6}
        d.update({n: torch.randn((B, REG_CH[n], S, S), generator=g) for n in REG})
        base.append(d)
    for name in a.dtypes:
        preds = [{k: v.to(dt[name]).cuda().requires_grad_(True) for k, v in d.items()} for d in base]
        leaves = [v for d in preds for v in d.values()]

        def clear():
            for v in leaves:
                v.grad = None

        def fused_loss():
            clear()
            torch.stack(crit(example, preds)["loss"]).sum().backward()

        def fused():
            clear()
            torch.stack(crit(assigner(gb, gc), preds)["loss"]).sum().backward()

        def steps():
            clear()
            torch.stack(torch_steps_loss(example, preds)[0]).sum().backward()

        lf = float(torch.stack(crit(example, preds)["loss"]).sum().detach())
        ls = float(torch.stack(torch_steps_loss(example, preds)[0]).sum().detach())
        mf, ml, ms = [], [], []
        for _ in range(a.repeats):                           # interleaved: all sides see the same drift of the machine
            mf.append(_time_calls(fused, a.warmup, a.calls))
            ml.append(_time_calls(fused_loss, a.warmup, a.calls))
            ms.append(_time_calls(steps, a.warmup, a.calls))
        kf, hf, per_f = _profile(fused)
        ks, hs, _ = _profile(steps)
        med = lambda v: sorted(v)[len(v) // 2]               # noqa: E731
        spread = max(ms) - min(ms)
        map_us = sum(v for k, v in (per_f or {}).items() if "k_loss_map" in k)
        esize = 4 if name == "fp32" else 2
        map_bytes = sum(B * K * S * S * (esize + 4 + 4) for K in TASKS)
        gbs = map_bytes / (map_us * 1e-6) / 1e9 if map_us else None
        print(json.dumps({"what": "six-task loss forward + backward", "dtype": name, "batch": B, "map": [S, S], "max_objs": M,
                          "fused_us": round(med(mf), 1), "fused_loss_us": round(med(ml), 1), "steps_us": round(med(ms), 1),
                          "fused_medians_us": [round(v, 1) for v in mf], "fused_loss_medians_us": [round(v, 1) for v in ml],
                          "steps_medians_us": [round(v, 1) for v in ms], "steps_spread_us": round(spread, 1),
                          "fused_spread_us": round(max(ml) - min(ml), 1), "saved_us": round(med(ms) - med(ml), 1),
                          "faster_by_more_than_spread": bool(med(ms) - med(ml) > max(spread, max(ml) - min(ml))),
                          "speedup": round(med(ms) / med(ml), 2), "fused_launches": kf, "steps_launches": ks,
                          "fused_host_round_trips": hf, "steps_host_round_trips": hs,
                          "map_pass_us": round(map_us, 1) if map_us else None, "map_pass_bytes": map_bytes,
                          "map_pass_gbs": round(gbs, 1) if gbs else None, "map_pass_frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4) if gbs else None,
                          "loss_fused": lf, "loss_steps": ls}), flush=True)


if __name__ == "__main__":
    main()
