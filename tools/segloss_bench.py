"""tools/segloss_bench.py -- the fused segmentation criterion (link_amd.SegCriterion: csrc/segloss.hip) against a torch restatement of
the reference's loss code on the same GPU, in the same process: forward + backward of CrossEntropyLoss(ignore_index=255) +
lovasz_softmax(softmax(logits), labels, ignore=0) on [N, 19] logits.

    timeout 600 python tools/segloss_bench.py [--n 100000 20000] [--dtypes fp32 fp16] [--warmup 10] [--calls 50] [--repeats 5]

`torch_loop_criterion` below is that restatement.  It takes the steps segmentation/core/trainers.py:64-73 and
core/lovasz_losses.py:21-33,174-225 take, in their order: the valid rows selected by index (a host wait for their number), a Python
loop over the classes, per class a mask, a presence test that reads the device back, a full sort, a gather, two running sums, a
shifted difference and a dot; under autocast rules the softmax and the cross-entropy run in fp32.  It is the comparison, never the code under test.

Per (N, dtype) one JSON line: the median of --calls timed calls (HIP events around forward + backward, one synchronise per call),
repeated --repeats times for both sides -- the five medians, their median, and the spread max - min; the speed-up and whether it
exceeds the comparison's spread; kernel launches per call and the radix sort's share of the fused kernels' time (torch.profiler,
one extra call; null when the profiler is not usable)."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _jaccard_steps(flags):
    """flags: 0/1 floats in sorted order.  Per position, how much the Jaccard loss 1 - |intersection| / |union| grows when the element
    joins the elements counted as errors: two running sums, the loss at every position, and its difference to the position before."""
    n_fg = flags.sum()
    fg_seen = flags.cumsum(0)
    bg_seen = (1.0 - flags).cumsum(0)
    loss_at = 1.0 - (n_fg - fg_seen) / (n_fg + bg_seen)
    return torch.cat([loss_at[:1], loss_at[1:] - loss_at[:-1]])


def torch_loop_criterion(logits, labels, ce_ignore=255, lov_ignore=0):
    """The comparison: the steps of the reference's loss in the order it takes them, in this project's own words."""
    wide = logits.float()
    ce_term = torch.nn.functional.cross_entropy(wide, labels, ignore_index=ce_ignore)
    prob = torch.softmax(wide, dim=1)
    keep = labels != lov_ignore
    prob_kept = prob[torch.nonzero(keep)[:, 0]]              # sized by the data: the host waits for the count
    label_kept = torch.masked_select(labels, keep)           # and again
    per_class = []
    for cls in range(prob.shape[1]):
        is_fg = (label_kept == cls).to(prob.dtype)
        if not bool(is_fg.sum() > 0):                        # the host asks the device whether the class is present
            continue
        miss = torch.abs(is_fg - prob_kept[:, cls])
        miss_desc, order = miss.sort(descending=True)
        per_class.append(torch.dot(miss_desc, _jaccard_steps(is_fg[order])))
    lovasz_term = torch.stack(per_class).mean() if per_class else prob.sum() * 0.0
    return ce_term + lovasz_term


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
    """(kernel launches of one call, {kernel name: us}) or (None, None)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n, per = 0, {}
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                n += 1
                per[e.name] = per.get(e.name, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
        return (n, per) if n else (None, None)
    except Exception:
        return None, None


def _by_kernel(per):
    """{short kernel name: us}: the k_* kernels of csrc/segloss.hip by name, torch's own kernels under `other`"""
    out = {}
    for name, us in (per or {}).items():
        m = re.search(r"\bk_[a-z_]+", name)
        key = m.group(0) if m else "other"
        out[key] = round(out.get(key, 0.0) + us, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 20000])
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"], choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import link_amd as la
    from segloss_oracle import make_case
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    for n in a.n:
        logits, labels = make_case(n, a.classes, 1)
        labels = labels.cuda()
        for name in a.dtypes:
            x = logits.to(dt[name]).cuda().requires_grad_(True)
            crit = la.SegCriterion()

            def fused():
                x.grad = None
                crit(x, labels).backward()

            def loop():
                x.grad = None
                torch_loop_criterion(x, labels).backward()

            fused()
            loop()
            lf, ll = float(crit(x, labels)), float(torch_loop_criterion(x, labels))
            mf, ml = [], []
            for _ in range(a.repeats):                       # interleaved: both sides see the same drift of the machine
                mf.append(_time_calls(fused, a.warmup, a.calls))
                ml.append(_time_calls(loop, a.warmup, a.calls))
            kf, per_f = _profile(fused)
            kl, _ = _profile(loop)
            sort_share = None
            if per_f:
                tot = sum(per_f.values())
                srt = sum(v for k, v in per_f.items() if "k_hist" in k or "k_scatter" in k)
                sort_share = round(srt / tot, 3) if tot > 0 else None
            med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
            spread = max(max(ml) - min(ml), max(mf) - min(mf))
            print(json.dumps({"n": n, "classes": a.classes, "dtype": name, "fused_us": round(med(mf), 1), "loop_us": round(med(ml), 1),
                              "fused_medians_us": [round(v, 1) for v in mf], "loop_medians_us": [round(v, 1) for v in ml],
                              "spread_us": round(spread, 1), "saved_us": round(med(ml) - med(mf), 1),
                              "faster_by_more_than_spread": bool(med(ml) - med(mf) > spread), "speedup": round(med(ml) / med(mf), 2),
                              "fused_launches": kf, "loop_launches": kl, "sort_share_of_fused_kernel_time": sort_share,
                              "fused_kernel_time_us": round(sum(per_f.values()), 1) if per_f else None,
                              "fused_kernel_us": _by_kernel(per_f),
                              "loss_fused": lf, "loss_loop": ll}), flush=True)


if __name__ == "__main__":
    main()
