"""tools/pillarbench.py -- the fused PointPillars reader (link_amd.PillarReader on csrc/pillar.hip: padded voxels -> BEV canvas in one
kernel after the zero fill) against torch compositions of the reference's steps on the same GPU, in the same process, at the two
production shapes: nuScenes (B = 4, 30 000 pillars per frame, T = 20, D = 5, [64, 64], 512 x 512) and Waymo (B = 4, 32 000 pillars
per frame, 468 x 468).

    timeout 900 python tools/pillarbench.py [--windows 7] [--calls 10] [--mean-points 4]

Two compositions are the comparison, never the code under test: `reference_form` (decoration, mask, every one of the T rows through
Linear / BatchNorm1d / ReLU / max, then the reference's per-sample masked assignment, which reads a mask's size back once per sample)
and `index_put` (the same reader with one index_put for the whole batch: no read-back).  The fused path is compared with the faster.

One JSON line per shape and output type: per side the per-call time of --windows windows of --calls calls each (HIP events around a
window, one synchronise per window, the sides alternating), their median and spread max - min; the device launches per call (counted
by torch.profiler; null where the profiler gives none) and the host round trips per call (synchronising calls seen by
torch.cuda.set_sync_debug_mode); and every median as a multiple of the byte floor, the time to zero-fill (that is, write) the canvas
once: canvas bytes / 8 TB/s, the HBM rate bench.py's roofline uses."""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
SHAPES = {"nuscenes": dict(B=4, per_frame=30000, T=20, D=5, filters=(64, 64), ny=512, nx=512, voxel=(0.2, 0.2, 8.0),
                           rng=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)),
          "waymo": dict(B=4, per_frame=32000, T=20, D=5, filters=(64, 64), ny=468, nx=468, voxel=(0.32, 0.32, 6.0),
                        rng=(-74.88, -74.88, -2.0, 74.88, 74.88, 4.0))}


def make_inputs(sh, mean_points, dev):
    """distinct cells per frame, 1 .. T points per pillar (mean about --mean-points), points inside their pillar"""
    g = torch.Generator().manual_seed(0)
    B, n, T, D, ny, nx = sh["B"], sh["per_frame"], sh["T"], sh["D"], sh["ny"], sh["nx"]
    coors = []
    for b in range(B):
        cell = torch.randperm(ny * nx, generator=g)[:n]
        coors.append(torch.stack([torch.full_like(cell, b), torch.zeros_like(cell), cell // nx, cell % nx], 1))
    coors = torch.cat(coors).int()
    P = coors.shape[0]
    num = (1 + torch.poisson(torch.full((P,), float(mean_points - 1)), generator=g)).clamp(1, T).int()
    x = torch.rand(P, T, D, generator=g)
    x[:, :, 0] = sh["rng"][0] + (coors[:, 3:4] + x[:, :, 0]) * sh["voxel"][0]
    x[:, :, 1] = sh["rng"][1] + (coors[:, 2:3] + x[:, :, 1]) * sh["voxel"][1]
    x[:, :, 2] = sh["rng"][2] + x[:, :, 2] * (sh["rng"][5] - sh["rng"][2])
    x = x * (torch.arange(T).view(1, T) < num.view(P, 1)).float()[..., None]
    return x.to(dev), num.to(dev), coors.to(dev)


def reference_scatter(rows, coords, batch_size, ny, nx):
    """the reference's PointPillarsScatter.forward step by step: a canvas, a mask and an indexed assignment per sample, a stack"""
    out = []
    for b in range(batch_size):
        canvas = torch.zeros(rows.shape[1], ny * nx, dtype=rows.dtype, device=rows.device)
        mask = coords[:, 0] == b
        this = coords[mask, :]
        idx = (this[:, 2] * nx + this[:, 3]).long()
        canvas[:, idx] = rows[mask, :].t()
        out.append(canvas)
    return torch.stack(out, 0).view(batch_size, rows.shape[1], ny, nx)


def windows(sides, n_windows, calls):
    for fn in sides.values():
        for _ in range(2):
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


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception:                  # no device tracing in this build: not measured
        return None


def round_trips(fn):
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return sum(1 for x in w if "synchron" in str(x.message).lower())
    except Exception:
        return None
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--mean-points", type=float, default=4.0, help="mean valid rows per pillar (1 .. T)")
    ap.add_argument("--shapes", default="nuscenes,waymo")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pillarbench: no GPU visible; timings are taken on the device only")
    import link_amd as la
    from link_amd.pillar import scatter_torch
    dev = "cuda"
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        x, num, coors = make_inputs(sh, a.mean_points, dev)
        B, ny, nx, C = sh["B"], sh["ny"], sh["nx"], sh["filters"][-1]
        torch.manual_seed(1)
        m = la.PillarFeatureNet(sh["D"], sh["filters"], False, sh["voxel"], sh["rng"]).to(dev)
        with torch.no_grad():
            for layer in m.pfn_layers:                                    # defaults would make every padded row exactly 0
                layer.norm.running_mean.normal_(0, 0.5)
                layer.norm.running_var.uniform_(0.5, 1.5)
                layer.norm.weight.uniform_(0.5, 1.5)
                layer.norm.bias.normal_(0, 0.5)
        m.eval()
        assert la.pillar_native(m, x)
        fused = la.PillarReader(m)

        def reference_form():
            with torch.no_grad():
                return reference_scatter(m.forward_torch(x, num, coors), coors, B, ny, nx)

        def index_put():
            with torch.no_grad():
                return scatter_torch(m.forward_torch(x, num, coors), coors, B, ny, nx)

        want = index_put()
        agree = {"fused_vs_index_put": float((fused(x, num, coors, B, (nx, ny, 1)) - want).abs().max()),
                 "reference_form_vs_index_put": float((reference_form() - want).abs().max()), "largest": float(want.abs().max())}
        del want
        for out_name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
            def native():
                return fused(x, num, coors, B, (nx, ny, 1), out_dtype=dt)

            sides = {"fused": native, "reference_form": reference_form, "index_put": index_put}
            t = {k: summary(v) for k, v in windows(sides, a.windows, a.calls).items()}
            floor_us = 1.0 * B * C * ny * nx * torch.empty((), dtype=dt).element_size() / HBM_PEAK * 1e6
            nat = t["fused"]
            best = min(("reference_form", "index_put"), key=lambda k: t[k]["median_us"])
            gap = t[best]["median_us"] - nat["median_us"]
            print(json.dumps({"what": "PillarFeatureNet + PointPillarsScatter, eval", "shape": name, "batch": B, "pillars": int(x.shape[0]),
                              "T": sh["T"], "D": sh["D"], "filters": list(sh["filters"]), "canvas": [ny, nx], "out": out_name,
                              "mean_points": round(float(num.float().mean()), 2), "windows": a.windows, "calls": a.calls, **t,
                              "launches_per_call": {k: launches(f) for k, f in sides.items()},
                              "host_round_trips_per_call": {k: round_trips(f) for k, f in sides.items()},
                              "faster_composition": best, "speedup": round(t[best]["median_us"] / nat["median_us"], 2),
                              "faster_by_more_than_spread": bool(gap > max(nat["spread_us"], t[best]["spread_us"])),
                              "byte_floor_us": round(floor_us, 1),
                              "multiples_of_byte_floor": {k: round(v["median_us"] / floor_us, 2) for k, v in t.items()},
                              "max_abs_difference": agree}), flush=True)
        del x, num, coors, m, fused
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
