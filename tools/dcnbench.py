"""tools/dcnbench.py -- deformable convolution on the device (link_amd/dcn.py on csrc/dcn.hip) against torch compositions of the same
formula on the same GPU, in the same process, at the nuScenes CenterHead shape: B = 4, 64 -> 64 channels, a 180 x 180 map, 3 x 3
taps, 4 deformable groups.

    timeout 900 python tools/dcnbench.py [--windows 7] [--calls 20] [--dtype fp32] [--offset-std 1.5]

Two compositions are the comparison, never the code under test: `gather` (link_amd.deform_conv_torch: gathered corners, one
contraction -- what the library itself runs outside the native envelope) and `grid_sample` (F.grid_sample per tap and group followed
by a 1 x 1 contraction).  The native path is compared with the faster of the two.

One JSON line per measurement: per side the per-call time of --windows windows of --calls calls each (HIP events around a window, one
synchronise per window, the sides alternating), their median and spread max - min.  Measurements: one DeformConv forward; forward +
backward (all three gradients); the native backward's two entries on their own; a whole DCNSepHead set of twelve FeatureAdaptions
(six tasks, two each), forward.  The forward line also gives the fraction of the f32 matrix peak (157.3 TF) and of the HBM
roofline (8 TB/s) on algorithmic bytes: input + offsets + output."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_PEAK, HBM_PEAK = 157.3e12, 8.0e12


def grid_sample_conv(x, offset, weight, pad, dg, relu=False):
    """stride 1, dilation 1: F.grid_sample(bilinear, zeros, align_corners=True) per tap and group + a 1 x 1 contraction"""
    B, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    cg = C // dg
    off = offset.view(B, dg, kh * kw, 2, H, W)
    hh = torch.arange(H, device=x.device, dtype=x.dtype).view(1, H, 1) - pad
    ww = torch.arange(W, device=x.device, dtype=x.dtype).view(1, 1, W) - pad
    out = None
    for g in range(dg):
        xs = x[:, g * cg:(g + 1) * cg]
        for t in range(kh * kw):
            h, w = hh + t // kw + off[:, g, t, 0], ww + t % kw + off[:, g, t, 1]
            grid = torch.stack([2 * w / (W - 1) - 1, 2 * h / (H - 1) - 1], -1)
            s = F.grid_sample(xs, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            y = torch.einsum("bchw,oc->bohw", s, weight[:, g * cg:(g + 1) * cg, t // kw, t % kw])
            out = y if out is None else out + y
    return torch.relu(out) if relu else out


def windows(sides, n_windows, calls):
    for fn in sides.values():                 # warm-up: code objects, library algorithm choices, the allocator, the workspace
        for _ in range(3):
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


def verdict(native, others):
    best = min(others, key=lambda k: others[k]["median_us"])
    gap = others[best]["median_us"] - native["median_us"]
    return {"native": native, **others, "faster_composition": best, "speedup": round(others[best]["median_us"] / native["median_us"], 2),
            "faster_by_more_than_spread": bool(gap > max(native["spread_us"], others[best]["spread_us"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--size", type=int, default=180)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--tasks", type=int, default=6)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--offset-std", type=float, default=1.5, help="standard deviation of the random offsets, in pixels")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcnbench: no GPU visible; timings are taken on the device only")
    import link_amd as la
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    B, C, S, dg = a.batch, a.channels, a.size, a.groups
    dev = "cuda"
    shape = {"batch": B, "channels": C, "map": [S, S], "taps": 9, "deformable_groups": dg, "dtype": a.dtype, "offset_std": a.offset_std, "windows": a.windows,
             "calls": a.calls}
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, C, S, S), generator=g).to(dev).to(dt).requires_grad_(True)
    off = (torch.randn((B, dg * 18, S, S), generator=g) * a.offset_std).to(dev).to(dt).requires_grad_(True)
    w = (torch.randn((C, C, 3, 3), generator=g) / (C * 9) ** 0.5).to(dev).to(dt).requires_grad_(True)
    go = torch.randn((B, C, S, S), generator=g).to(dev).to(dt)
    assert la.deform_conv_native(x, off, w, 1, 1, 1, 1, dg)
    with torch.no_grad():
        ref = la.deform_conv_torch(x, off, w, 1, 1, 1, 1, dg)
        agree = {"native_vs_gather": float((la.deform_conv(x, off, w, 1, 1, 1, 1, dg) - ref).abs().max()),
                 "grid_sample_vs_gather": float((grid_sample_conv(x, off, w, 1, dg) - ref).abs().max()), "largest": float(ref.abs().max())}

    fwd = {"native": lambda: la.deform_conv(x, off, w, 1, 1, 1, 1, dg), "gather": lambda: la.deform_conv_torch(x, off, w, 1, 1, 1, 1, dg),
           "grid_sample": lambda: grid_sample_conv(x, off, w, 1, dg)}

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def train(fn, leaves):
        def run():
            return torch.autograd.grad(fn(), leaves, go)
        return run
    t = {k: summary(v) for k, v in windows({k: no_grad(f) for k, f in fwd.items()}, a.windows, a.calls).items()}
    nat = t.pop("native")
    flop = 2.0 * B * S * S * C * C * 9
    item = torch.empty((), dtype=dt).element_size()
    nbytes = item * (x.numel() + off.numel() + go.numel())
    print(json.dumps({"what": "DeformConv forward", **shape, **verdict(nat, t), "max_abs_difference": agree, "gflop": round(flop / 1e9, 2),
                      "fraction_of_f32_mfma_peak": round(flop / (nat["median_us"] * 1e-6) / MFMA_F32_PEAK, 4),
                      "algorithmic_mbytes": round(nbytes / 1e6, 1),
                      "fraction_of_hbm_roofline": round(nbytes / HBM_PEAK / (nat["median_us"] * 1e-6), 4)}), flush=True)

    calls = max(a.calls // 4, 3)
    t = {k: summary(v) for k, v in windows({k: train(f, (x, off, w)) for k, f in fwd.items()}, a.windows, calls).items()}
    nat = t.pop("native")
    print(json.dumps({"what": "DeformConv forward + backward (grad_input, grad_offset, grad_weight)", **shape, "calls_per_window": calls,
                      **verdict(nat, t)}), flush=True)
    xd, od, wd = x.detach(), off.detach(), w.detach()                                 # needs_input_grad follows the leaves of the call
    parts = windows({"forward": no_grad(fwd["native"]),
                     "forward_backward_data": train(lambda: la.deform_conv(x, off, wd, 1, 1, 1, 1, dg), (x, off)),
                     "forward_backward_weight": train(lambda: la.deform_conv(xd, od, w, 1, 1, 1, 1, dg), (w,))}, a.windows, calls)
    print(json.dumps({"what": "native entries: forward alone, with link_deform_conv_backward_data, with link_deform_conv_backward_weight",
                      **shape, "calls_per_window": calls, **{k: summary(v) for k, v in parts.items()}}), flush=True)

    # ---- the head's twelve adaptions ---------------------------------------------------------------------------------------------
    torch.manual_seed(1)
    mods = [la.FeatureAdaption(C, C, deformable_groups=dg).to(dev).to(dt) for _ in range(2 * a.tasks)]
    for m in mods:
        torch.nn.init.normal_(m.conv_offset.weight, 0, 0.05)
    xin = x.detach()

    def head_native():
        with torch.no_grad():
            return [m(xin) for m in mods]

    def head_with(comp):
        def run():
            with torch.no_grad():
                return [comp(xin, m.conv_offset(xin), m.conv_adaption.weight) for m in mods]
        return run
    sides = {"native": head_native, "gather": head_with(lambda i, o, k: torch.relu(la.deform_conv_torch(i, o, k, 1, 1, 1, 1, dg))),
             "grid_sample": head_with(lambda i, o, k: grid_sample_conv(i, o, k, 1, dg, relu=True))}
    t = {k: summary(v) for k, v in windows(sides, a.windows, max(a.calls // 4, 3)).items()}
    nat = t.pop("native")
    print(json.dumps({"what": f"DCNSepHead set: {2 * a.tasks} FeatureAdaptions forward (offset convolution + deformable convolution + ReLU)",
                      **shape, "calls_per_window": max(a.calls // 4, 3), **verdict(nat, t)}), flush=True)


if __name__ == "__main__":
    main()
