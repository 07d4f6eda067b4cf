#!/usr/bin/env python
"""bench.py -- throughput of one LinK (3x7)^3 block on MI355X (BASELINE.json metric).

Step      = one pass of the hot path R_core (pre_mix -> theta -> modulate ->
            voxel_to_aux -> aux_to_voxel -> de-modulate -> norm) over ONE synthetic frame, index
            structures rebuilt inside the step ("cold", as the reference does on every call).
            Frames are independent (the unit the path shards by), so `--streams` frames are kept in
            flight on separate HIP streams with separate buffers and NO cross-stream dependency: the
            kernels of one frame fill the latency bubbles of another's.  `single_stream_value` is the
            same measurement with one frame in flight.
Workload  = BASELINE.json configs[1]: 100k unique voxels uniform in a 256^3 grid (S-uniform generator,
            seed = rank), C = 64, baseop cos, groups 2, r = 3, s = 7, fp32.
N GPUs    = one process per GPU, one independent frame per rank per step, NO data-path collective
            (weak scaling); after the timed region the per-rank summaries (voxels, blocks, checksum,
            elapsed) are all-gathered over RCCL -- the "trivial result gather".
Timing    = W warm-up steps, barrier + synchronize, EXACTLY K steps, synchronize + barrier, max over
            ranks; value = voxels processed by all ranks / that time.  Inputs are resident in HBM.

Rank 0 prints ONE JSON line (contract in the task statement) with two extra objects:
  roofline      dominant kernel: algorithmic bytes / its average duration,
                measured with HIP events on the launch stream in a second, instrumented replay of the
                same K steps (so the events do not perturb `value`); peak 8.0 TB/s HBM.
  cpu_baseline  the scalar C/torch oracle port (oracle/) timed on this host, rank 0, N=1 only.

A plain run (no --full) sets up, settles, warms up, times the K steps through both paths (three streams, batch
entry point) and prints the line.  What needs runs of its own is null there: cpu_baseline, regions, gpu_state,
single_stream_value, warm_index_value, three_frame_step, batch_period_events, timed_configuration_check; `roofline`
holds only the timed region's fraction, `multi_gpu` only the collective check.  --full runs all of it after the
timed region, as every run did before the option existed.  --dump-outputs DIR writes the rows the headline path
returned in its last timed step (dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The HIP runtime multiplexes streams onto a few hardware queues (4 by default); this process uses the three frame streams, the batch
# context's three role streams and two caller streams.  Kernels of streams that share a hardware queue run one after the other (round
# 6, tools/batch_bench.py: the batch entry point 42.5 us / frame with the default, 35.9 with 8 queues; the three-stream figure moves
# within its box-to-box noise).  Set before the runtime initialises, unless the caller has chosen a value.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

SHADER_CLOCK_HZ = 2.4e9     # nominal; the line carries the MEASURED shader clock (gpu_state) and prices mfma_util with it when it is known
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def gpu_state_during(run, device_index=0, period_s=0.001):
    """Shader clock / memory clock / socket power of the device WHILE `run()` keeps it busy (a replay of the timed steps, never the
    timed region itself: the sampler thread shares the interpreter with the launch loop).  amdsmi, sampled every `period_s` from a
    thread; returns medians / extremes, or {"available": False, ...} when the library or the permission is missing -- a line
    without it is still a valid line (box-to-box spread is 5 x a round's gain and the line said nothing about the
    clock / power state it was measured in)."""
    import threading
    try:
        import amdsmi
        amdsmi.amdsmi_init()
        handles = amdsmi.amdsmi_get_processor_handles()
        h = handles[device_index if device_index < len(handles) else 0]
    except Exception as e:  # noqa: BLE001
        run()
        return {"available": False, "error": repr(e)[:160]}
    samples, stop = [], threading.Event()

    def one():
        row = {}
        try:
            ci = amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.GFX)
            row["sclk"], row["sclk_max"] = ci.get("clk"), ci.get("max_clk")
        except Exception:  # noqa: BLE001
            pass
        try:
            mi = amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.MEM)
            row["mclk"] = mi.get("clk")
        except Exception:  # noqa: BLE001
            pass
        try:
            pi = amdsmi.amdsmi_get_power_info(h)
            row["power"] = pi.get("current_socket_power") if isinstance(pi.get("current_socket_power"), (int, float)) else pi.get("average_socket_power")
            row["power_limit"] = pi.get("power_limit")
        except Exception:  # noqa: BLE001
            pass
        return row

    def sampler():
        while not stop.is_set():
            samples.append(one())
            stop.wait(period_s)
    idle = one()
    th = threading.Thread(target=sampler, daemon=True)
    th.start()
    try:
        run()
    finally:
        stop.set()
        th.join()
        try:
            amdsmi.amdsmi_shut_down()
        except Exception:  # noqa: BLE001
            pass

    def stat(key):
        v = sorted(x[key] for x in samples if isinstance(x.get(key), (int, float)))
        return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]} if v else None
    out = {"available": bool(samples), "samples": len(samples), "sclk_mhz": stat("sclk"), "mclk_mhz": stat("mclk"),
           "socket_power_w": stat("power"), "idle_before": idle,
           "note": "amdsmi, sampled every ms during a REPLAY of the timed steps (same plans, streams and launch geometry)"}
    mx = [x.get("sclk_max") for x in samples if isinstance(x.get("sclk_max"), (int, float))]
    if mx:
        out["sclk_max_mhz"] = max(mx)
    return out


ROUNDS = max(1, int(os.environ.get("LINK_BENCH_ROUNDS", "8")))   # a step = ROUNDS rounds of the frames in flight (see timed())
SETTLE_STEPS = int(os.environ.get("LINK_BENCH_SETTLE", "60"))      # untimed steps before the warm-up (clock ramp); reported in the line.
# (500 until the step became a batch of 24 frames: three regions of the timed shape are 50 ms at the driver's --steps 20, and the
# figure is the same with 60 as with 500 -- 34.7 / 35.0 against 35.3 / 35.7 us/frame, alternating on one box)
SETTLE_REGION_MAX = 200     # steps per settling region at most: with a large K the settling stays ~0.5 s instead of growing with K


def settle_shape(steps):
    """(regions, steps per region) of the untimed settling phase before the warm-up: regions of the timed shape (K steps between
    synchronisations), at least 3 and at least SETTLE_STEPS steps in all, a region capped at SETTLE_REGION_MAX steps (a timed
    region that long is no short burst; below the cap the shape is K steps, as it always was)."""
    k = max(1, min(steps, SETTLE_REGION_MAX))
    return max(3, -(-SETTLE_STEPS // k)), k


DUMP_BYTES = 64 * 1000 * 1000    # --dump-outputs: at most 64 MB in all


def dump_outputs(dirname, rows):
    """--dump-outputs: frame j's result rows -- what the timed path returned for it in its last step -- as float32 DIR/frame<j>.npy.
    When the frames hold more than DUMP_BYTES in all (cfg2: 3 x 100k x 64 x 4 B = 76.8 MB), every frame keeps the same fixed sample of
    rows: seed 0, row indices sorted, the same for every run with the same arguments."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    n, c = rows[0].shape
    keep = min(n, DUMP_BYTES // (4 * c * len(rows)))
    idx = None if keep == n else np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
    for j, r in enumerate(rows):
        a = r.float().cpu().numpy()
        np.save(os.path.join(dirname, f"frame{j}.npy"), a if idx is None else a[idx])


def s_uniform(n, grid=256, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    lin = torch.randperm(grid ** 3, generator=g)[:n]
    return torch.stack([lin % grid, (lin // grid) % grid, lin // (grid * grid), torch.zeros_like(lin)], 1).int()


def alg_bytes(n, m, c, parts=2, esz=4):
    """B_alg = N*16 + N*4C + N*4C + 2*M*4*(W+1), and its per-kernel split
    (each term charged once, to the kernel that must move it).  esz = bytes per feature element at the
    boundary (fp16 / bf16 rows: 2C instead of 4C; the block table stays fp32)."""
    w = parts * c
    table = m * 4 * (w + 1)
    return {"total": n * 16 + 2 * n * esz * c + 2 * table,
            "premix_ln": n * esz * c,
            "modulate_block_sum": n * 16 + table,
            "block_gather": table,
            "voxel_demod_ln": n * esz * c}


def _cpu_info():
    model, phys = "unknown", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                pid = line.split(":")[1].strip()
            elif line.startswith("core id"):
                cid = line.split(":")[1].strip()
                phys.add((pid, cid))
    except OSError:
        pass
    return model, (len(phys) or os.cpu_count() or 1)


def cpu_baseline(blk, feats, coords, out, N, C, S_, R, G):
    """SURVEY.md section 8d CPU baseline on this host: R_core through oracle/ (baseline only; the roofline
    fraction is the quality measure).  Bounded: the OpenMP leg runs a sub-frame sized for ~10 s."""
    import torch
    from oracle import link_oracle as O
    model, phys = _cpu_info()
    params = {k: v.detach().cpu() for k, v in blk.state_dict().items()}
    fc, cc = feats.cpu(), coords.cpu()
    torch.set_num_threads(1)
    reps, t_cpu, ref = 0, 0.0, None
    while reps < 20 and t_cpu < 8.0:                     # scalar port, one core, full frame
        t0 = time.perf_counter()
        ref = O.elk_core_torch(fc, cc, params, S_, R, "cos", G, agg=O.aggregate_c)
        t_cpu += time.perf_counter() - t0
        reps += 1
    err = float((out.cpu() - ref).abs().max() / ref.abs().max())
    one_core = N * reps / t_cpu
    # OpenMP leg: the reference's pragma placement (a parallel region per voxel in spvoxelize, voxelize_cpu.cpp:17) makes
    # the thread count matter enormously -- 128 threads fork/join 100k times.  Sweep it (bounded: ~2.5 s per point) and
    # report the BEST point as `value`; the all-physical-cores figure SURVEY.md 8d asks for stays as a named sub-field.
    import ctypes
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
    except OSError:
        gomp = None

    def set_threads(k):
        os.environ["OMP_NUM_THREADS"] = str(k)
        if gomp is not None:
            gomp.omp_set_num_threads(int(k))
        torch.set_num_threads(int(k))

    O.set_omp(True)
    sweep = {}
    try:
        def omp_pass(nv):
            t0 = time.perf_counter()
            O.elk_core_torch(fc[:nv], cc[:nv], params, S_, R, "cos", G, agg=O.aggregate_c)
            return time.perf_counter() - t0
        for k in sorted({t for t in (1, 8, 16, 32, 64, phys) if t <= phys}):
            set_threads(k)
            probe = omp_pass(min(N, 4000))
            nv = int(min(N, max(4000, 4000 * 2.5 / max(probe, 1e-3))))
            t = omp_pass(nv)
            sweep[k] = {"voxels_per_s": round(nv / t, 1), "sample_voxels": nv, "seconds": round(t, 2)}
    finally:
        O.set_omp(False)
        set_threads(1)
    best = max(sweep, key=lambda k: sweep[k]["voxels_per_s"])
    # the reference's OWN compiled CPU ops (oracle/_ref/ref_backend.so: hash_cpu.cpp, count_cpu.cpp, voxelize_cpu.cpp compiled
    # where they lie by oracle/build_ref.py in the build container; the .so travels like any built .so) on this frame's index
    # and modulated rows -- the three reference ops of voxel_to_aux that ARE buildable and correct here (devoxelize_cpu.cpp is
    # 8-neighbour-only: invalid at r = 3; query_cpu.cpp needs sparsehash).  A labelled sub-field, kind "reference".
    ref_ops = None
    try:
        from oracle import build_ref
        if os.path.exists(build_ref.SO):
            rb = build_ref.load_module()
            _, idx_q, cnts = O.voxel_to_aux_index(cc.numpy(), S_)
            idx_t, cnt_t = torch.from_numpy(idx_q.astype("int32")), torch.from_numpy(cnts.astype("int32"))
            xrows = torch.randn(N, 2 * C, generator=torch.Generator().manual_seed(3))
            cc32 = cc.int().contiguous()

            def tmin(fn, reps=3):
                best_t = 1e9
                for _ in range(reps):
                    t0 = time.perf_counter(); fn(); best_t = min(best_t, time.perf_counter() - t0)
                return best_t
            ref_ops = {"kind": "reference", "threads": 1,
                       "hash_cpu_ms": round(1e3 * tmin(lambda: rb.hash_cpu(cc32)), 3),
                       "count_cpu_ms": round(1e3 * tmin(lambda: rb.count_cpu(idx_t, int(cnt_t.numel()))), 3),
                       "voxelize_forward_cpu_ms": round(1e3 * tmin(lambda: rb.voxelize_forward_cpu(xrows, idx_t, cnt_t)), 2),
                       "note": f"compiled reference ops on the full frame (N={N}, W={2 * C}), OMP_NUM_THREADS = 1 (the best point "
                               "of the sweep), best of 3"}
    except Exception as e:  # noqa: BLE001 -- a baseline sub-field must never take the bench line down
        ref_ops = {"kind": "reference", "error": repr(e)[:200]}
    return {"value": sweep[best]["voxels_per_s"], "unit": "voxels/s", "cores": best, "kind": "port", "cpu_model": model,
            "sample": f"R_core on the first {sweep[best]['sample_voxels']} voxels of the same frame (C={C}) through oracle/'s OpenMP twin "
                      f"(pragmas at the reference's loop placement, voxelize_cpu.cpp:17, devoxelize_cpu.cpp:16) at the best thread "
                      f"count of the sweep {sorted(sweep)}: OMP_NUM_THREADS = torch threads = {best}; {sweep[best]['seconds']} s",
            "thread_sweep": {str(k): v for k, v in sweep.items()},
            "all_physical_cores": dict(sweep[phys], cores=phys, note="the figure SURVEY.md 8d specifies: one parallel region per voxel "
                                                                      "at every physical core -- fork/join bound, not a fair baseline"),
            "single_core_port": {"value": round(one_core, 1), "cores": 1,
                                 "sample": f"{reps} full passes (N={N}) through the scalar C restatement + single-thread "
                                           f"torch dense ops, {t_cpu:.1f} s"},
            "reference_ops": ref_ops,
            "host_cpus": os.cpu_count(), "gpu_vs_oracle_max_rel_err": err}


def timed_regions(la, blk, feats, coords, C, s, r, iters=30):
    """The other timed regions of SURVEY.md section 8d on the same frame, device-event medians in us:
    R_agg = voxel_to_aux + aux_to_voxel through the drop-in surface on X[N,2C]; R_block = ELKBlock.forward
    (local_mix + R_core + norm_local/add/ReLU).  cold = fresh SparseTensor (nothing cached), warm = the
    tensor's kmaps/cmaps carried over (what the 2nd..4th block of a network stage sees)."""
    import torch
    dev = feats.device
    x = torch.randn(feats.shape[0], 2 * C, generator=torch.Generator().manual_seed(5)).to(dev)

    def med(fn):
        for _ in range(3):
            fn()
        ev = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        v = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
        return round(v[len(v) // 2], 1)

    st0 = la.SparseTensor(x, coords, 1)
    la.voxel_to_aux(st0, s)

    def r_agg(warm):
        st = la.SparseTensor(x, coords, 1)
        if warm:
            st.kmaps, st.cmaps = st0.kmaps, st0.cmaps
        small, idx, counts = la.voxel_to_aux(st, s)
        return la.aux_to_voxel(small, st, idx, counts, r).F

    stb = la.SparseTensor(feats, coords, 1)
    with torch.no_grad():
        blk(stb, s, r)

    def r_block(warm):
        st = la.SparseTensor(feats, coords, 1)
        if warm:
            st.kmaps, st.cmaps = stb.kmaps, stb.cmaps
        with torch.no_grad():
            return blk(st, s, r).F

    from link_amd import elk as _elk
    calls0 = dict(_elk.BLOCK_DRIVER_CALLS)
    res = {"R_agg_cold_us": med(lambda: r_agg(False)), "R_agg_warm_us": med(lambda: r_agg(True)),
           "R_block_cold_us": med(lambda: r_block(False)), "R_block_warm_us": med(lambda: r_block(True))}
    res["block_driver_calls"] = {k: _elk.BLOCK_DRIVER_CALLS[k] - calls0[k] for k in calls0}    # how R_block cold ran: link_elk_block_forward done / missed
    return {**res,
            "note": "host-inclusive device-event medians through the Python module surface (allocating path); "
                    "R_core cold/warm are `value`/`warm_index_value` (arena path, one FFI call per step)"}


def core_roofline(torch, blocks, step, iters=20):
    """R_core of every LinK block of a network against the HBM roofline: wraps each block's `_core`
    with HIP events on the launch stream (`step()` runs the network once, warm kernel maps), and prices the measured time
    against B_alg = N*16 + 2*N*esz*C + 2*M*4*(W+1) with the stage's own N, M (occupied blocks at its s_eff), C, W.
    Returns the `roofline` object of the JSON line: the sum over the blocks + one entry per block."""
    rec = [{"ev": [], "meta": None} for _ in blocks]
    saved = [b._core for b in blocks]

    def wrap(i, f0):
        def core(st, s_eff, r, w_pos, alpha, cg, coord_div):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f0(st, s_eff, r, w_pos, alpha, cg, coord_div)
            e1.record()
            rec[i]["ev"].append((e0, e1))
            if rec[i]["meta"] is None:
                rec[i]["call"] = (st.C.contiguous(), st.F.contiguous(), int(s_eff), int(r), w_pos, alpha, int(cg), float(coord_div))
                ts_ = getattr(st, "s", 1)
                rec[i]["stride"] = int(ts_[0] if isinstance(ts_, (tuple, list)) else ts_)
                c = st.C
                blk = torch.cat([torch.div(c[:, :3], int(s_eff), rounding_mode="floor"), c[:, 3:]], 1)
                m = int(torch.unique(blk, dim=0).shape[0])
                parts = 3 if blocks[i].baseop == "cos_x" else 2
                rec[i]["meta"] = {"voxels": int(c.shape[0]), "blocks": m, "channels": int(st.F.shape[1]),
                                  "w": parts * int(st.F.shape[1]), "s_eff": int(s_eff), "r": int(r),
                                  "esz": st.F.element_size()}
            return out
        return core
    for i, b in enumerate(blocks):
        b._core = wrap(i, saved[i])
    try:
        for _ in range(3):
            step()
        for r_ in rec:
            r_["ev"].clear()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
    finally:
        for b, f0 in zip(blocks, saved):
            b._core = f0
    # the same stage frames through ElkCorePlan (preallocated arena, one FFI call per step, no module / allocator around it):
    # device time of R_core with the block index REBUILT every step -- what the reference does per call (utils.py:44-58) -- next
    # to the warm-index time, HIP events over back-to-back steps
    from link_amd.elk import ElkCorePlan
    from link_amd.index import coords_bounds
    from link_amd.parallel import streams_on_own_queues
    n_inflight = max(2, int(os.environ.get("LINK_BENCH_LIDAR_INFLIGHT", "3")))
    inflight_streams, _ = streams_on_own_queues(n_inflight, blocks[0].norm.weight.device)

    def plan_times(i):
        coords, feats, s_eff, r, w_pos, alpha, cg, coord_div = rec[i]["call"]
        b = blocks[i]
        # voxel sites a block can hold at this tensor stride (coordinates are multiples of the stride)
        ts = max(int(rec[i]["stride"]), 1)
        cap = max(1, int(s_eff) // ts) ** 3 if int(s_eff) % ts == 0 else int(s_eff) ** 3
        best = None
        for form, kw in (("tiles", dict(layout="general")), ("lean", dict(layout="lean", slot_cap=min(cap, 352)))):
            try:
                plan = ElkCorePlan(feats.shape[0], feats.shape[1], b.baseop, cg, r, s_eff, coords_bounds(coords), feats.device,
                                   coord_div=coord_div, **kw)
            except Exception:  # noqa: BLE001 -- widths / block sizes the form does not take
                continue
            plan.bind(b.pre_mix[0].weight, b.pre_mix[1].weight, b.pre_mix[1].bias, w_pos, alpha, b.norm.weight, b.norm.bias)
            out = {"form": form}
            for key, rebuild in (("rebuilt", True), ("warm", False)):
                for _ in range(5):
                    plan.run(feats, coords, build_index=rebuild)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    plan.run(feats, coords, build_index=rebuild)
                e1.record()
                torch.cuda.synchronize()
                out[key] = 1e3 * e0.elapsed_time(e1) / 50
            if form == "lean":
                plan.check()                                  # no voxel dropped: the slot capacity held
            # the reference trains / evaluates with TWO frames per GPU (segmentation/configs/semantic_kitti/default.yaml:20, det
            # samples_per_gpu = 2): the same stage frame twice as one collated batch (batch column 0 / 1) through ONE launch set --
            # the launches' fixed cost is paid once for both frames
            try:
                c2 = torch.cat([coords, coords + torch.tensor([0, 0, 0, 1], dtype=coords.dtype, device=coords.device)], 0).contiguous()
                f2 = torch.cat([feats, feats], 0).contiguous()
                plan2 = ElkCorePlan(f2.shape[0], f2.shape[1], b.baseop, cg, r, s_eff, coords_bounds(c2), f2.device, coord_div=coord_div, **kw)
                plan2.bind(b.pre_mix[0].weight, b.pre_mix[1].weight, b.pre_mix[1].bias, w_pos, alpha, b.norm.weight, b.norm.bias)
                for _ in range(5):
                    o2 = plan2.run(f2, c2, build_index=True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    o2 = plan2.run(f2, c2, build_index=True)
                e1.record()
                torch.cuda.synchronize()
                n1 = feats.shape[0]
                same = bool(torch.equal(o2[:n1], o2[n1:]))    # two copies of one frame: identical rows, whatever the batch column
                out["batch2"] = {"us_per_frame": round(1e3 * e0.elapsed_time(e1) / 100, 2), "rows_identical_across_the_two_frames": same}
                del plan2
            except Exception as e:  # noqa: BLE001
                out["batch2"] = {"error": repr(e)[:120]}
            # ... and THREE frames in flight (three arenas, three streams on hardware queues of their own), as the headline keeps them:
            # the launches of a LiDAR stage frame are latency-bound, so the launches of other frames fit beside them
            try:
                plans3 = [plan]
                for _ in range(n_inflight - 1):
                    p3 = ElkCorePlan(feats.shape[0], feats.shape[1], b.baseop, cg, r, s_eff, coords_bounds(coords), feats.device, coord_div=coord_div, **kw)
                    p3.bind(b.pre_mix[0].weight, b.pre_mix[1].weight, b.pre_mix[1].bias, w_pos, alpha, b.norm.weight, b.norm.bias)
                    plans3.append(p3)
                main = torch.cuda.current_stream()

                def burst(k_):
                    for s_ in inflight_streams:
                        s_.wait_stream(main)
                    for _ in range(k_):
                        for j_, p3 in enumerate(plans3):
                            p3.run(feats, coords, build_index=True, stream=inflight_streams[j_].cuda_stream)
                    for s_ in inflight_streams:
                        main.wait_stream(s_)
                burst(5)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                burst(40)
                e1.record()
                torch.cuda.synchronize()
                for p3 in plans3:
                    p3.check()
                o_a, o_b = plans3[0].run(feats, coords, build_index=True).clone(), plans3[-1].run(feats, coords, build_index=True)
                out["inflight3"] = {"frames_in_flight": n_inflight, "us_per_frame": round(1e3 * e0.elapsed_time(e1) / (40 * n_inflight), 2), "rows_identical_across_arenas": bool(torch.equal(o_a, o_b))}
                del plans3[1:]
            except Exception as e:  # noqa: BLE001
                out["inflight3"] = {"error": repr(e)[:120]}
            out["launches_rebuilt"] = 3 if form == "lean" else (6 if getattr(plan, "tiles", False) else 8)
            out["by_form"] = dict(best["by_form"]) if best else {}
            out["by_form"][form] = {"rebuilt_us": round(out["rebuilt"], 2), "warm_us": round(out["warm"], 2),
                                    "launches_rebuilt": out["launches_rebuilt"], "batch_of_2_rebuilt": out.get("batch2"),
                                    "three_frames_in_flight_rebuilt": out.get("inflight3")}
            if best is None or out["rebuilt"] < best["rebuilt"]:
                best = out
            else:
                best["by_form"] = out["by_form"]
            del plan
        return best
    stages, tot_b, tot_t, tot_reb, tot_b2, tot_f3 = [], 0.0, 0.0, 0.0, 0.0, 0.0
    for i, r_ in enumerate(rec):
        m = r_["meta"]
        v = sorted(1e3 * a.elapsed_time(b) for a, b in r_["ev"])
        us = v[len(v) // 2]
        alg = m["voxels"] * 16 + 2 * m["voxels"] * m["esz"] * m["channels"] + 2 * m["blocks"] * 4 * (m["w"] + 1)
        gbs = alg / (us * 1e-6) / 1e9
        st_row = {**{k: m[k] for k in ("voxels", "blocks", "channels", "w", "s_eff", "r")}, "us": round(us, 2),
                  "alg_bytes": alg, "achieved": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4)}
        pt = plan_times(i)
        if pt:
            st_row.update({"plan_us_rebuilt_index": round(pt["rebuilt"], 2), "plan_us_warm_index": round(pt["warm"], 2),
                           "frac_rebuilt_index": round(alg / (pt["rebuilt"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                           "frac_warm_index": round(alg / (pt["warm"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                           "launches_rebuilt": pt["launches_rebuilt"], "form_rebuilt": pt["form"], "rebuilt_by_form": pt["by_form"]})
            tot_reb += pt["rebuilt"]
            b2 = [v["batch_of_2_rebuilt"]["us_per_frame"] for v in pt["by_form"].values()
                  if v.get("batch_of_2_rebuilt") and "us_per_frame" in v["batch_of_2_rebuilt"]]
            if b2:
                st_row["plan_us_rebuilt_index_batch_of_2_per_frame"] = min(b2)
                st_row["frac_rebuilt_index_batch_of_2"] = round(alg / (min(b2) * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
                tot_b2 += min(b2)
            f3 = [v["three_frames_in_flight_rebuilt"]["us_per_frame"] for v in pt["by_form"].values()
                  if v.get("three_frames_in_flight_rebuilt") and "us_per_frame" in v["three_frames_in_flight_rebuilt"]]
            if f3:
                st_row["plan_us_rebuilt_index_3_in_flight_per_frame"] = min(f3)
                st_row["frac_rebuilt_index_3_in_flight"] = round(alg / (min(f3) * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
                tot_f3 += min(f3)
        stages.append(st_row)
        tot_b += alg
        tot_t += us
    ach = tot_b / (tot_t * 1e-6) / 1e9
    return {"bound": "hbm", "region": "R_core of the network's LinK blocks (HIP events on the launch stream around each core, "
                                      "host-inclusive: the module path allocates and launches per call; warm kernel maps)",
            "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
            "traffic": None, "alg_bytes": tot_b, "us": round(tot_t, 2),
            "rebuilt_index": ({"us": round(tot_reb, 2), "frac": round(tot_b / (tot_reb * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                               "note": "sum over the stages of ElkCorePlan steps with the block index rebuilt every step (device time, "
                                       "one FFI call per step): what the reference's per-call index corresponds to"} if tot_reb else None),
            "rebuilt_index_batch_of_2": ({"us_per_frame": round(tot_b2, 2), "frac": round(tot_b / (tot_b2 * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                          "note": "the same, two frames per launch set (the reference's batch size), best form per stage, per frame"}
                                         if tot_b2 else None),
            "rebuilt_index_three_frames_in_flight": ({"us_per_frame": round(tot_f3, 2), "frac": round(tot_b / (tot_f3 * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                                      "note": "the same with three frames in flight per stage (three arenas, three streams on hardware queues of "
                                                              "their own -- how the cfg2 headline keeps its frames), best form per stage, per frame"}
                                                     if tot_f3 else None),
            "stages": stages}


def conv_roofline(torch, la, step, iters=10):
    """Row N1 (missing 5): every sparse convolution of the network against ITS roofline.  Wraps link_amd.Conv3d.forward /
    forward_affine with HIP events on the launch stream (`step()` runs the network once on warm kernel maps) and prices the device time of a
    call -- all its launches: pair GEMM / table kernel + finish -- against
        bytes = rows in (N_in * Cin * esz) + rows out (N_out * Cout * esz) + weights (K * Cin * Cout * 4) + pair list (pairs * 8)
        flops = 2 * pairs * Cin * Cout                    (pairs = valid (output, offset) entries of the kernel map)
    (nn/functional/conv.py:16-147, convolution_cuda.cu:53-165: gather -> GEMM per offset -> scatter moves the same rows K times; the
    algorithmic floor moves them once).  Roofline time = max(bytes / 8 TB/s, flops / 157.3 TF/s: the exact-fp32 matrix peak of
    MI355X_MICROARCH.md -- the fp16 hi | lo split the pair GEMM uses is three f16 products per fp32 one, priced as fp32 work).
    Returns per distinct shape (stage voxels, Cin -> Cout, kernel, stride): calls, mean us, bytes, flops, bound, frac; and the sums."""
    from link_amd.elk import Conv3d
    rec = {}
    f_plain, f_aff = Conv3d.forward, Conv3d.forward_affine

    def pairs_of(m, x):
        try:
            if m.kernel_volume == 1:
                return int(x.F.shape[0])
            if m.stride[0] == 1:
                nbr, _ = m._neighbor_table(x)
                return int((nbr >= 0).sum().item())
            km = m._strided_map(x) if not m.transposed else x.kmaps[(tuple(x.s[k] // m.stride[k] for k in range(3)), m.kernel_size, m.stride, m.dilation)]
            return int((km.nbr_down >= 0).sum().item())
        except Exception:  # noqa: BLE001
            return -1

    def wrap(f0):
        def fwd(self, x, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n_in, cin = int(x.F.shape[0]), int(x.F.shape[1])
            e0.record()
            y = f0(self, x, *a, **kw)
            e1.record()
            key = (id(self), n_in)
            r = rec.get(key)
            if r is None:
                r = rec[key] = {"n_in": n_in, "n_out": int(y.F.shape[0]), "cin": cin, "cout": int(y.F.shape[1]), "kvol": int(self.kernel_volume),
                                "stride": int(self.stride[0]), "transposed": bool(self.transposed), "esz": x.F.element_size(), "ev": [],
                                "pairs": pairs_of(self, x), "fused_epilogue": f0 is f_aff}
            r["ev"].append((e0, e1))
            return y
        return fwd
    Conv3d.forward, Conv3d.forward_affine = wrap(f_plain), wrap(f_aff)
    try:
        for _ in range(2):
            step()
        for r in rec.values():
            r["ev"].clear()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
    finally:
        Conv3d.forward, Conv3d.forward_affine = f_plain, f_aff
    shapes = {}
    for r in rec.values():
        if not r["ev"] or r["pairs"] < 0:
            continue
        us = 1e3 * sum(a.elapsed_time(b) for a, b in r["ev"]) / len(r["ev"])
        k = (r["n_in"], r["n_out"], r["cin"], r["cout"], r["kvol"], r["stride"], r["transposed"])
        s_ = shapes.setdefault(k, {"layers": 0, "us": 0.0, "pairs": r["pairs"], "esz": r["esz"]})
        s_["layers"] += 1
        s_["us"] += us
    out, tot_us, tot_roof = [], 0.0, 0.0
    for (n_in, n_out, cin, cout, kvol, stride, tr), s_ in sorted(shapes.items(), key=lambda kv: -kv[1]["us"]):
        by = n_in * cin * s_["esz"] + n_out * cout * s_["esz"] + kvol * cin * cout * 4 + s_["pairs"] * 8
        fl = 2.0 * s_["pairs"] * cin * cout
        t_mem, t_mm = by / (HBM_PEAK_GBS * 1e9), fl / 157.3e12
        us = s_["us"] / s_["layers"]
        roof = max(t_mem, t_mm) * 1e6
        out.append({"n_in": n_in, "n_out": n_out, "cin": cin, "cout": cout, "kernel_volume": kvol, "stride": stride, "transposed": tr,
                    "layers": s_["layers"], "pairs": s_["pairs"], "us_per_call": round(us, 2), "alg_bytes": int(by), "flops": int(fl),
                    "bound": "hbm" if t_mem >= t_mm else "mfma_f32", "roofline_us": round(roof, 3), "frac": round(roof / us, 4),
                    "achieved_gbs": round(by / (us * 1e-6) / 1e9, 1), "achieved_tflops": round(fl / (us * 1e-6) / 1e12, 2)})
        tot_us += s_["us"]
        tot_roof += roof * s_["layers"]
    return {"what": "every link_amd.Conv3d call of one eval forward (warm kernel maps), HIP events on the launch stream around the call: device "
                    "time of all its launches against max(bytes / 8 TB/s, 2 * pairs * Cin * Cout / 157.3 TF/s)",
            "sum_us": round(tot_us, 1), "sum_roofline_us": round(tot_roof, 2), "frac": round(tot_roof / tot_us, 4) if tot_us else None,
            "shapes": out}


def cfg3_mode(args, la, dev, rank, world, dist):
    """BASELINE.json configs[2] shape (labelled, NOT the headline): the encoder common to both segmentation models
    (stem -> 4 x [k2-s2 down, 2 residual blocks + tail || ELKBlock cos_x (2x3)^3 + tail, add/ReLU],
    linkencoder.py:186-368; assembled in harness/networks.py from link_amd modules) on one S-kitti frame per
    rank (link_amd/synth.py, seed = rank; full size, ~113k voxels), warm kernel maps.  A step = one eval
    forward; the line also carries forward+backward (sum-of-squares loss on stage 4) and the time inside the
    four ELK blocks."""
    import torch
    from harness import networks as LE
    from link_amd.synth import s_kitti, block_stats
    co, fe = s_kitti(seed=rank)
    coords, feats = torch.from_numpy(co).to(dev), torch.from_numpy(fe).to(dev)
    n = coords.shape[0]
    torch.manual_seed(0)
    # the reference's ELKEncoder encoder half, class by class (harness/networks.py mirrors linkencoder.py:186-290
    # with the reference's attribute names), its Conv3d -> BatchNorm -> ReLU runs fused for inference
    net = la.fuse_for_inference(LE.build_reference_shaped_encoder(la, 64, "cos_x", 1)).to(dev)
    net.elk = [getattr(net, f"elk{i}") for i in (1, 2, 3, 4)]
    st0 = la.SparseTensor(feats, coords, 1)
    with torch.no_grad():
        sizes = [o.C.shape[0] for o in net.eval()(st0, 3, 2)[1]]

    def step(train):
        f = feats.detach().requires_grad_(train)
        x = la.SparseTensor(f, coords, 1)
        x.kmaps, x.cmaps = st0.kmaps, st0.cmaps
        if train:
            net.zero_grad(set_to_none=True)       # what a training loop does between steps (optimizer.zero_grad): without it every
            net(x, 3, 2)[1][-1].F.square().sum().backward()   # step also ADDS its ~110 parameter gradients onto the previous step's
        else:
            with torch.no_grad():
                net(x, 3, 2)

    def timed(train, k, w):
        net.train(train)
        for _ in range(w):
            step(train)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            step(train)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = torch.tensor([time.perf_counter() - t0], device=dev)
        if world > 1:
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        return float(dt.item())

    k = min(args.steps, 50)
    w = min(args.warmup, 5)
    t_fwd = timed(False, k, w)
    t_tr = timed(True, max(3, k // 2), max(w, 5))      # (2 warm-up + k/4 timed steps read 9.5 ms where 20-step loops read 8.0-8.3: the
                                                       # first training steps still finalise pair plans and grow the allocator's pools)
    # time inside the ELK blocks (eval), stream-synchronised per call: an upper bound of their share
    elk_t = [0.0]
    saved = [m.forward for m in net.elk]

    def wrap(f0):
        def fwd(*a, **kw):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            o = f0(*a, **kw)
            torch.cuda.synchronize(); elk_t[0] += time.perf_counter() - t0
            return o
        return fwd
    for m in net.elk:
        m.forward = wrap(m.forward)
    net.eval()
    for _ in range(5):
        step(False)
    for m, f0 in zip(net.elk, saved):
        m.forward = f0
    roof = core_roofline(torch, net.elk, lambda: step(False)) if rank == 0 else None
    net.eval()
    conv_roof = conv_roofline(torch, la, lambda: step(False)) if rank == 0 else None
    nv = torch.tensor([float(n)], device=dev)
    if world > 1:
        dist.all_reduce(nv)
    if rank == 0:
        print(json.dumps({
            "metric": "voxels_per_second", "value": float(nv.item()) * k / t_fwd, "unit": "voxels/s", "n_gpus": world,
            "steps": k, "warmup": w, "ms_per_step": 1e3 * t_fwd / k, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic (S-kitti ray-cast frame, SURVEY.md 8d; random-init weights)",
            "headline": False,
            "config": {"workload": "cfg3 (labelled secondary mode): encoder half of ELKEncoder (stem + 4 stages), eval forward, "
                                   "C=64 cos_x (2x3)^3 r=2, Conv-BN-ReLU runs fused, one S-kitti frame per GPU, warm kernel maps",
                       "voxels": n, "stage_voxels": sizes, "blocks_s6_on_input_voxels": int(block_stats(co, 6)[1]),
                       "parallelism": f"dp{world}"},
            "fwd_bwd_ms": 1e3 * t_tr / max(3, k // 2), "elk_blocks_fwd_ms": 1e3 * elk_t[0] / 5,
            "roofline": roof, "conv_roofline": conv_roof, "cpu_baseline": None}))
    if world > 1:
        dist.destroy_process_group()


def cfg4_mode(args, la, dev, rank, world, dist):
    """BASELINE.json configs[3] (labelled, NOT the headline): a batch of 8 S-kitti frames (seeds 0..7) sharded over
    the ranks by independent frames (link_amd/parallel.py::shard_frames: 8 / 4 / 2 / 1 rounds at 1 / 2 / 4 / 8 GPUs)
    -- STRONG scaling, no data-path collective; afterwards the per-frame summaries are all-gathered (the "trivial
    result gather").  A step = the whole batch once: every rank runs the encoder half of ELKEncoder (eval forward,
    Conv-BN-ReLU fused) on its frames, kernel maps built per frame as the reference does."""
    import torch
    from harness import networks as LE
    from link_amd.parallel import gather_frame_rows, shard_frames
    from link_amd.synth import s_kitti
    mine = shard_frames(8, world, rank)
    frames = []
    for fid in mine:
        co, fe = s_kitti(seed=fid)
        frames.append((fid, torch.from_numpy(co).to(dev), torch.from_numpy(fe).to(dev)))
    torch.manual_seed(0)
    net = la.fuse_for_inference(LE.build_reference_shaped_encoder(la, 64, "cos_x", 1)).to(dev).eval()

    def batch():
        rows = []
        with torch.no_grad():
            for fid, coords, feats in frames:
                _, outs = net(la.SparseTensor(feats, coords, 1), 3, 2)
                rows.append((fid, coords.shape[0], outs[-1].C.shape[0], outs[-1].F.double().sum()))
        return rows

    k, w = min(args.steps, 10), min(args.warmup, 2)
    for _ in range(w):
        batch()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        rows = batch()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = torch.tensor([time.perf_counter() - t0], device=dev)
    if world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    summ = torch.tensor([[float(a), float(b), float(c), float(d)] for a, b, c, d in rows], dtype=torch.float64, device=dev).view(-1, 4)
    allrows = gather_frame_rows(summ)                  # frame id, voxels, stage-4 voxels, checksum: every rank gets all 8
    if rank == 0:
        nvox = float(allrows[:, 1].sum().item())
        print(json.dumps({
            "metric": "voxels_per_second", "value": nvox * k / float(dt.item()), "unit": "voxels/s", "n_gpus": world,
            "steps": k, "warmup": w, "ms_per_step": 1e3 * float(dt.item()) / k, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic (8 S-kitti ray-cast frames, SURVEY.md 8d; random-init weights)",
            "headline": False,
            "config": {"workload": "cfg4 (labelled secondary mode): 8 S-kitti frames sharded by frame over the ranks, encoder half "
                                   "of ELKEncoder, eval forward, kernel maps per frame",
                       "frames": int(allrows.shape[0]), "voxels": nvox, "frames_per_rank": len(mine), "parallelism": f"dp{world}"},
            "frame_checksums": [float(v) for v in allrows[allrows[:, 0].argsort(), 3].tolist()],
            "roofline": None, "cpu_baseline": None}))
    if world > 1:
        dist.destroy_process_group()


def cfg5_mode(args, la, dev, rank, world, dist):
    """BASELINE.json configs[4] shape (labelled, NOT the headline): the sparse half of the detection backbone
    SpMiddleResNetFHDELKv3 (scn.py:452-626: conv_input, 4 x [2 SparseBasicBlocks + tail || TSELKBlock (3x7)^3 + tail],
    3 k3-s2 SparseConv3d, extra_conv, dense -> BEV [1, 256, 180, 180]) on one S-nusc frame per rank
    (link_amd/synth.py, seed = rank; ~150k voxels, 5 features, grid 1440 x 1440 x 40), eval forward, random-init
    weights; fp32, or with `--io f16|bf16` the AMP form BASELINE.json quotes this configuration in (16-bit rows and
    weights on the 16-bit matrix cores, fp32 accumulation / BatchNorm folds; the TSELKBlock core in fp32).  A step builds every kernel map of the frame (as the reference does per frame); the line also carries
    the warm-map time.  The dense BEV half (RPN, CenterHead) is plain torch in the reference and not timed."""
    import torch
    from link_amd.synth import s_nusc
    co, fe = s_nusc(seed=rank)
    indices = torch.from_numpy(co[:, [3, 2, 1, 0]].copy()).int().to(dev)
    feats = torch.from_numpy(fe).to(dev).to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.io])
    n = indices.shape[0]
    torch.manual_seed(0)
    net = la.SpMiddleResNetFHDELKv3(num_input_features=5).to(dev).eval()
    shape = [1440, 1440, 40]

    def timed(k, w, maps):
        with torch.no_grad():
            for _ in range(w):
                net(feats, indices, 1, shape, indice_dict=maps)
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                net(feats, indices, 1, shape, indice_dict=maps)
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = torch.tensor([time.perf_counter() - t0], device=dev)
        if world > 1:
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        return float(dt.item())

    k, w = min(args.steps, 30), min(args.warmup, 3)
    t_cold = timed(k, w, None)
    t_warm = timed(k, w, {})
    with torch.no_grad():
        bev, scales = net(feats, indices, 1, shape)
    bev_ms = with_bev_ms = None
    if args.bev:
        # what BASELINE.json's configs[4] names in full: backbone + CenterPoint head.  The BEV half is plain torch in the
        # reference as well (vendor dense-convolution library), outside the LinK hot path: timed separately and together
        from harness.bevhead import BevHalf
        half = BevHalf(num_input_features=bev.shape[1]).to(dev).eval()
        half = half.to(feats.dtype) if feats.dtype != torch.float32 else half

        def both(maps):
            b, _ = net(feats, indices, 1, shape, indice_dict=maps)
            return half(b.to(feats.dtype))
        with torch.no_grad():
            for _ in range(3):
                preds = both(None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                both(None)
            torch.cuda.synchronize()
            with_bev_ms = 1e3 * (time.perf_counter() - t0) / k
            x = bev.to(feats.dtype)
            t0 = time.perf_counter()
            for _ in range(k):
                half(x)
            torch.cuda.synchronize()
            bev_ms = 1e3 * (time.perf_counter() - t0) / k
        assert len(preds) == 6 and preds[0]["hm"].shape[-2:] == bev.shape[-2:]
    roof = None
    if rank == 0:
        warm_maps = {}

        def one():
            with torch.no_grad():
                net(feats, indices, 1, shape, indice_dict=warm_maps)
        roof = core_roofline(torch, [net.elk1, net.elk2, net.elk3, net.elk4], one)
    nv = torch.tensor([float(n)], device=dev)
    if world > 1:
        dist.all_reduce(nv)
    if rank == 0:
        print(json.dumps({
            "metric": "voxels_per_second", "value": float(nv.item()) * k / t_cold, "unit": "voxels/s", "n_gpus": world,
            "steps": k, "warmup": w, "ms_per_step": 1e3 * t_cold / k, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if args.io == "f32" else f"{args.io} rows and convolution weights (16-bit MFMA, f32 accumulation); block core f32",
            "data": "synthetic (S-nusc ray-cast frame, SURVEY.md 8d; random-init weights)",
            "headline": False,
            "config": {"workload": "cfg5 (labelled secondary mode): sparse half of SpMiddleResNetFHDELKv3, eval forward, kernel "
                                   "maps built per frame, one S-nusc frame per GPU",
                       "voxels": n, "stage_voxels": [scales[f"conv{i}"].features.shape[0] for i in (1, 2, 3, 4)],
                       "bev": list(bev.shape), "parallelism": f"dp{world}"},
            "warm_maps_ms": 1e3 * t_warm / k, "bev_half_ms": bev_ms, "backbone_plus_bev_half_ms": with_bev_ms,
            "roofline": roof, "cpu_baseline": None}))
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--voxels", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--streams", type=int, default=3, help="independent frames in flight per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--full", action="store_true",
                    help="cfg2: also run the side measurements and checks of the line (one frame in flight, warm index, three-frame step, "
                         "batch period events, clock / power state, timed-geometry check, instrumented per-kernel roofline, CPU baseline, "
                         "module-surface regions, N > 1 gather figures); without it the run times the headline and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="cfg2: after the timed steps, write the rows the timed path returned in its last step, one float32 "
                         "DIR/frame<j>.npy per frame in flight (a fixed, seeded row sample when all frames exceed 64 MB)")
    ap.add_argument("--bev", action="store_true",
                    help="cfg5: also run the dense BEV half (RPN + CenterHead in plain torch, harness/bevhead.py) behind the backbone")
    ap.add_argument("--io", choices=("f32", "f16", "bf16"), default="f32",
                    help="feature-row type at the kernel boundary (f32 = the headline; f16/bf16: AMP rows, fp32 inside)")
    ap.add_argument("--workload", choices=("cfg2", "cfg3", "cfg4", "cfg5"), default="cfg2",
                    help="cfg2 = the headline (R_core, S-uniform); cfg3 = labelled secondary mode: forward and "
                         "forward+backward of the LinK encoder stages on one S-kitti frame per rank; cfg4 = labelled: 8 S-kitti "
                         "frames sharded over the ranks (strong scaling), encoder eval forward, maps built per frame; cfg5 = labelled: "
                         "sparse half of the detection backbone (SpMiddleResNetFHDELKv3) on one S-nusc frame per rank")
    args = ap.parse_args()
    if args.dump_outputs is not None and args.workload != "cfg2":
        raise SystemExit("bench.py: --dump-outputs is implemented for the headline workload (cfg2) only")

    import torch
    import torch.distributed as dist

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU
        import subprocess
        port = 29500 + os.getpid() % 2000
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(args.gpus, 1):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         "(python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...)")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path exists in the product)")
    # LINK_BENCH_BACKEND=gloo lets several ranks share one GPU (debugging the N>1 logic on a 1-GPU box);
    # the real multi-GPU run uses "nccl" (= RCCL over xGMI), one rank per GPU.
    backend = os.environ.get("LINK_BENCH_BACKEND", "nccl")
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    import link_amd as la
    from link_amd import _lib as L
    from link_amd.parallel import pin_rank_to_gpu_numa

    # Host placement: with several ranks on one node every rank pins itself to CPUs of ITS GPU's NUMA node
    # (its own slice of them when ranks share a node) -- the issuing thread spends 12-20 us per 35 us frame, and an unpinned rank may
    # sit on the far socket.  One rank alone is left where the launcher put it (the cpu_baseline thread sweep needs every core);
    # LINK_BENCH_PIN=1 / 0 forces either.  The record of every rank is in the line (`cpu_affinity`).
    pin_env = os.environ.get("LINK_BENCH_PIN", "")
    if (world > 1 and pin_env != "0") or pin_env == "1":
        affinity = pin_rank_to_gpu_numa(local_rank, local_rank, min(world, torch.cuda.device_count()))
    else:
        affinity = {"pinned": False, "numa_node": None, "cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 0,
                    "first_cpu": None, "reason": "single rank: left where the launcher put it"}

    if args.workload == "cfg3":
        return cfg3_mode(args, la, dev, rank, world, dist)
    if args.workload == "cfg5":
        return cfg5_mode(args, la, dev, rank, world, dist)
    if args.workload == "cfg4":
        return cfg4_mode(args, la, dev, rank, world, dist)

    N, C, G, R, S_ = args.voxels, args.channels, 2, 3, 7
    torch.manual_seed(2)
    blk = la.ELKBlock(C, C, groups=G, baseop="cos").to(dev).eval()
    NS = max(1, args.streams)
    frames, plans, streams = [], [], []
    for k in range(NS):                    # NS distinct frames per rank (seeds differ per rank and slot)
        seed = rank * 64 + k
        io_t = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.io]
        frames.append((torch.randn(N, C, generator=torch.Generator().manual_seed(1 + seed)).to(dev).to(io_t),
                       s_uniform(N, seed=seed).to(dev)))
        pl = la.ElkCorePlan(N, C, "cos", C // G, R, S_, ((0, 0, 0, 0), (255, 255, 255, 0)), dev, frames_in_flight=NS)
        pl.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight,
                None, blk.norm.weight, blk.norm.bias)
        plans.append(pl)
    # the frame streams: NS streams on hardware queues of their own (two streams the runtime puts on one queue run their frames one after
    # the other -- the single-stream rate; one of six triples of consecutive torch streams did, tools/stream_placement.py)
    from link_amd.parallel import streams_on_own_queues
    streams, frame_stream_check = streams_on_own_queues(NS, dev)
    feats, coords = frames[0]
    plan = plans[0]
    # The batch entry point (side measurement at the end, `batch_entry_point`).  Two calls are kept in flight on two arena sets: call s + 1
    # is SUBMITTED before call s is JOINED, all from one stream (link_dc_batch_submit / link_dc_batch_join).  The first form of this
    # measurement alternated two caller streams instead, and read 37 or 50 us / frame depending on the streams it happened to get: two
    # streams the runtime multiplexes onto one hardware queue serialise the calls (the wait of one stream's call sits in front of the
    # other's submission; tools/batch_overlap.py shows call s + 1 starting when call s has ended).  What is left of the placement is
    # measured: ElkCoreBatch.calibrate -- LINK_BENCH_BATCH_TRIALS contexts (default 8) on the SAME arenas, 2 x 8 calls each (0.3 s in all), the fastest kept,
    # every trial in the line.
    for j_ in range(NS):                   # the frame streams' first use comes BEFORE the trials: the runtime binds a stream to a hardware queue
        with torch.cuda.stream(streams[j_]):   # when it is first used, and the headline's placement must not depend on a side measurement
            plans[j_].run(*frames[j_])
    torch.cuda.synchronize()
    bsets = None
    btrials = []
    n_trials = int(os.environ.get("LINK_BENCH_BATCH_TRIALS", "8"))      # 0: no batch path (a context is in one of three states: 31.8 / 33.1-33.8 / 39.5 us per frame at 48 frames per call)

    def batch_calls(k_, stream_):
        """k_ calls alternating the two arena sets, submit(s + 1) before join(s), from one stream; seconds"""
        h_ = stream_.cuda_stream
        torch.cuda.synchronize()
        t0_ = time.perf_counter()
        prev_ = None
        for s_ in range(k_):
            _, tk_ = bsets[s_ % 2].submit(bfe0, bco0, stream=h_)
            if prev_ is not None:
                bsets[0].join(prev_, stream=h_)
            prev_ = tk_
        bsets[0].join(prev_, stream=h_)
        torch.cuda.synchronize()
        return time.perf_counter() - t0_

    if (plan.dense and C == 64 and G == 2 and NS == 3 and n_trials > 0 and (N, C) == (100000, 64)
            and not (world > 1 and backend != "nccl")):     # (ranks sharing ONE device over gloo: persistent kernels of two processes would take turns)
        try:
            FB = int(os.environ.get("LINK_BENCH_BATCH_FRAMES", "48"))   # frames per call: 48 = one launch set of the entry point (two steps' worth of frames)
            bsets = [la.ElkCoreBatch(FB, N, C, "cos", C // G, R, S_, ((0, 0, 0, 0), (255, 255, 255, 0)), dev)]
            bsets.append(la.ElkCoreBatch(FB, N, C, "cos", C // G, R, S_, ((0, 0, 0, 0), (255, 255, 255, 0)), dev, share=bsets[0]))
            for b_ in bsets:
                b_.bind(blk.pre_mix[0].weight, blk.pre_mix[1].weight, blk.pre_mix[1].bias, blk.pos_weight[0].weight, None, blk.norm.weight,
                        blk.norm.bias)
            bfe0, bco0 = [frames[i % NS][0] for i in range(FB)], [frames[i % NS][1] for i in range(FB)]
            bstream = torch.cuda.Stream(device=dev)
            btrials = bsets[0].calibrate(bfe0, bco0, partner=bsets[1], tries=n_trials, calls=8, stream=bstream.cuda_stream)
            if os.environ.get("LINK_BENCH_BATCH_PROBE") == "1":
                print(f"[batch trials] {btrials} us/frame; queue delays of the kept context {bsets[0].probe_streams(bstream.cuda_stream)}", file=sys.stderr, flush=True)
        except Exception as e:  # noqa: BLE001
            bsets = repr(e)[:200]

    def barrier():
        if world > 1:
            dist.barrier()

    def batch_probe(tag):                               # LINK_BENCH_BATCH_PROBE=1: the batch side measurement at several points of the run (stderr)
        if os.environ.get("LINK_BENCH_BATCH_PROBE") != "1" or bsets is None or isinstance(bsets, str):
            return
        batch_calls(50, bstream)
        print(f"[batch probe] {tag}: {1e6 * batch_calls(50, bstream) / (50 * FB):.2f} us/frame; queue delays "
              f"{bsets[0].probe_streams(bstream.cuda_stream)}", file=sys.stderr, flush=True)

    batch_probe("after creation")

    def geometry(ns):
        """Launch geometry for the number of frames kept in flight (dense-cell layout) -- per-plan state
        (ElkCorePlan.set_tuning / link_dc_tuning_t; nothing process-global): one frame alone wants every kernel spread over
        2 workgroups per CU (512 workgroups of the fused pre_mix kernel, z-segments of the gather kernel by tile count);
        with several frames in flight the kernels of different frames share the CUs, so each runs at one workgroup per CU
        and the gather kernel takes 2 z-segments -- fewer halo planes summed twice.  LINK_BENCH_<KEY> overrides for sweeps
        (K1_WGS, K2_ZSPLIT, K1_FORM, K2_FORM, K1_PAD, K2_PAD)."""
        env = {"k1_wgs": "LINK_BENCH_K1_WGS", "k2_zsplit": "LINK_BENCH_K2_ZSPLIT", "k1_form": "LINK_BENCH_K1_FORM",
               "k2_form": "LINK_BENCH_K2_FORM", "k1_lds_pad": "LINK_BENCH_K1_PAD", "k2_lds_pad": "LINK_BENCH_K2_PAD"}
        kw = {k: int(os.environ[e]) for k, e in env.items() if os.environ.get(e) not in (None, "")}
        for pl in plans:
            if pl.dense:
                pl.frames_in_flight = ns
                pl.set_tuning(**kw)

    last_out = [None] * NS                 # what each plan's latest step RETURNED (fp32 rows: the plan's own buffer; half rows:
                                           # its per-dtype buffer -- never read `plan.out` directly, it is the fp32 one)

    def timed(k, build_index=True, ns=NS, rounds=ROUNDS):
        """EXACTLY k steps; a step = one batch of `rounds * ns` independent frames per GPU, `ns` of them in flight at a time
        (one per stream: the unit the path shards by), so k steps are k * rounds * ns frames; barrier + synchronize on both
        sides.  Round 5: the batch is ROUNDS = 8 rounds of the frames in flight (24 frames) instead of one (3).  A timed region
        pays a fixed ~150 us for filling and draining the three-deep pipeline around its two synchronisations
        (tools/host_issue.py, one box: 20 steps x 3 frames 37.2 us/frame, x 12 frames 34.9, x 24 frames 34.7 = what 200 steps
        x 3 frames give; the host issues a frame in 12-20 us, so it is not the host) -- at the driver's --steps 20 a 3-frame
        step made that 7 % of the figure.  The 3-frame-step figure is still measured and reported (`three_frame_step`)."""
        geometry(ns)
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            for _r in range(rounds):
                for j in range(ns):
                    with torch.cuda.stream(streams[j]):
                        last_out[j] = plans[j].run(frames[j][0], frames[j][1], build_index=build_index)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        barrier()
        return t1 - t0

    # the device comes out of process start-up (imports, allocations, the library build check) at idle clocks: an untimed
    # settling phase of SETTLE_STEPS of the same steps (~60 ms) brings it to operating clocks before the W warm-up steps and the timed
    # K (at the driver's --steps 20 --warmup 5 the timed region is 2.5 ms: 41.8 us/frame without it, 39-40 with, the
    # figure a 200-step run reports either way)
    # Round 5: the settling steps are issued in REGIONS OF THE TIMED SHAPE -- K steps between synchronisations -- instead of one
    # long run.  tools/graphstep.py, 20-step regions back to back on one box: 39.3 38.8 38.3 37.2 36.7 36.1 ... settling at 34.8-35.0
    # us/frame after ~10 regions (a 600-step run on the same box: 33.2): a device that has just worked through one long burst
    # answers the first short bursts 10 % slower, so a 2 ms timed region has to be preceded by bursts of its own length.  Same
    # step count as before (>= SETTLE_STEPS; a fixed number of regions: every rank passes the same barriers).  Regions are capped at
    # SETTLE_REGION_MAX steps (settle_shape), so that the untimed time of a run does not grow with K.
    import gc
    settle_regions, settle_k = settle_shape(args.steps)
    for _ in range(settle_regions):
        timed(settle_k)
    gc.collect()
    gc.disable()                                     # no collection inside the warm-up / timed regions (re-enabled right after)
    timed(max(args.warmup, 1))
    elapsed = timed(args.steps)                      # THE measurement (cold: index rebuilt for every frame)
    outs_timed = [o.clone() for o in last_out]       # the rows the timed steps wrote, in the row type they were written in
    elapsed_r1 = timed(args.steps, rounds=1) if args.full else None   # the same K steps with the 3-frame batch of rounds 1-4 (continuity)
    # ---- the same K steps through the BATCH entry point (include/link_amd.h section H): the frames of a step go through calls of FB
    # frames (two steps' worth; a last call takes what is left), two arena sets, submit(s + 1) before join(s) from one stream.  Same
    # contract: settling regions of the timed shape, W warm-up steps, EXACTLY K steps between barrier + synchronize.  The faster of the
    # two ways to run the K steps is the line's `value` (both are in the line: `paths`); rows are bit-equal (checked below).
    elapsed_batch, batch_fail, outs_batch = None, None, None
    batch_last = [None]                              # the rows the last call of the latest timed_batch returned

    def timed_batch(k):
        frames_total, done, s_, prev_ = k * NS * ROUNDS, 0, 0, None
        h_ = bstream.cuda_stream
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while done < frames_total:
            nb = min(FB, frames_total - done)
            batch_last[0], tk_ = bsets[s_ % 2].submit(bfe0[:nb], bco0[:nb], stream=h_)
            if prev_ is not None:
                bsets[0].join(prev_, stream=h_)
            prev_, done, s_ = tk_, done + nb, s_ + 1
        bsets[0].join(prev_, stream=h_)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        barrier()
        return t1 - t0

    batch_usable = bsets is not None and not isinstance(bsets, str)
    if world > 1:                                    # every rank must take the same branch (the barriers inside timed_batch)
        flag = torch.tensor([1.0 if batch_usable else 0.0], dtype=torch.float64, device=dev if backend == "nccl" else torch.device("cpu"))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        batch_usable = bool(flag.item() == 1.0)
    if batch_usable:
        try:
            for _ in range(3):
                timed_batch(settle_k)
            timed_batch(max(args.warmup, 1))
            elapsed_batch = timed_batch(args.steps)
            if args.dump_outputs is not None:        # frames 0 .. NS - 1 of the last call (call item i runs frame i % NS)
                outs_batch = [o.clone() for o in batch_last[0][:NS]]
            bsets[0].check()
        except Exception as e:  # noqa: BLE001
            if world > 1:
                raise                                # (ranks would part ways at the next barrier: better to stop loudly)
            batch_fail, elapsed_batch = repr(e)[:200], None
    gc.enable()
    # what was just timed is what gets checked: every plan's output under the timed configuration (NS frames in flight,
    # their launch geometry), kept (outs_timed, above) for the comparison with the single-frame geometry below and with the oracle
    batch_probe("after the timed region")
    for pl in plans:
        pl.check()
    # device-event view of the same configuration (SURVEY.md 8d asks for event medians): one event per stream after every
    # frame; the interval between consecutive completions on ONE stream is the period of a batch in steady state
    def batch_period_events(k):
        geometry(NS)
        torch.cuda.synchronize()
        evs = [[] for _ in range(NS)]
        for _ in range(k + 1):
            for j in range(NS):
                with torch.cuda.stream(streams[j]):
                    plans[j].run(frames[j][0], frames[j][1])
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    evs[j].append(e)
        torch.cuda.synchronize()
        per = sorted(1e3 * a.elapsed_time(b) for ev in evs for a, b in zip(ev[:-1], ev[1:]))
        return {"median_us": round(per[len(per) // 2], 2), "mean_us": round(sum(per) / len(per), 2), "n": len(per),
                "note": "HIP events, one per stream after every frame: interval between consecutive completions on one stream = "
                        "time of one batch of the frames in flight, steady state"}
    M = plan.blocks()
    checksum = float(outs_timed[0].double().sum().item())   # frame 0's rows as the timed steps wrote them
    batch_ev = gpu_state = elapsed_single = timed_check = elapsed_warm = out = None
    if args.full:                                   # the side measurements of the line: runs of their own after the timed region
        batch_ev = batch_period_events(max(50, min(args.steps, 200)))
        # clock / power state of the device under this very load (a replay of >= 30 ms of the timed steps; rank 0 reports it)
        if rank == 0:
            gpu_state = gpu_state_during(lambda: timed(max(args.steps, 1000), rounds=1), local_rank)
        else:
            gpu_state = None
            timed(max(args.steps, 1000), rounds=1)       # every rank passes the same barriers
        elapsed_single = timed(args.steps * NS, ns=1)    # the same number of frames, one in flight
        timed_check = {"frames": NS, "bitwise_equal_to_single_frame_geometry": True, "max_rel_err_vs_single_frame_geometry": 0.0}
        for j in range(NS):
            o1 = plans[j].run(frames[j][0], frames[j][1])          # same frame, single-frame launch geometry
            torch.cuda.synchronize()
            d = float((outs_timed[j].float() - o1.float()).abs().max() / o1.float().abs().max())
            timed_check["max_rel_err_vs_single_frame_geometry"] = max(timed_check["max_rel_err_vs_single_frame_geometry"], d)
            timed_check["bitwise_equal_to_single_frame_geometry"] &= bool(torch.equal(outs_timed[j], o1))
        out = plan.run(feats, coords)
        torch.cuda.synchronize()
        elapsed_warm = timed(args.steps, build_index=False)

    # ---- max over ranks + the trivial result gather (per-frame summaries only; link_amd/parallel.py)
    multi = None
    if world > 1:
        from link_amd.parallel import gather_frame_rows
        cdev = dev if backend == "nccl" else "cpu"
        # SURVEY.md section 8e side figures (not the graded throughput): (1) the collective backend really spans `world` ranks
        # (an all_reduce of ones), (2) END-TO-END = the timed K steps again, followed by the summary gather, one clock around both,
        # (3) the FULL-TENSOR result gather -- every rank's [N_i, C] output rows all-gathered with the reference's two-phase
        # pattern (sizes, then payload padded to the longest; det3d/torchie/trainer/utils.py:114-155) -- timed on its own.
        ones = torch.ones(1, dtype=torch.float64, device=cdev)
        dist.all_reduce(ones)
        if float(ones.item()) != float(world):           # fail loudly: a job whose collective does not span --gpus ranks measured something else
            raise SystemExit(f"bench.py: all_reduce of ones gave {float(ones.item())} on rank {rank}, expected {world} "
                             f"(backend {dist.get_backend()}): the process group does not span --gpus {args.gpus} ranks")
        multi = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "all_reduce_of_ones": float(ones.item()),
                 "collective_spans_all_ranks": bool(float(ones.item()) == float(world))}
        if args.full:
            barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps * ROUNDS):
                for j in range(NS):
                    with torch.cuda.stream(streams[j]):
                        last_out[j] = plans[j].run(frames[j][0], frames[j][1])
            torch.cuda.synchronize()
            probe = torch.tensor([[float(rank), float(N), float(M), checksum]], dtype=torch.float64, device=cdev)
            gather_frame_rows(probe)
            if backend == "nccl":
                torch.cuda.synchronize()
            t_e2e = time.perf_counter() - t0
            payload = out.float() if backend == "nccl" else out.float().cpu()
            gather_frame_rows(payload[:16])                   # warm the collective up
            t_full = []
            for _ in range(3):
                barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                full = gather_frame_rows(payload)
                if backend == "nccl":
                    torch.cuda.synchronize()
                t_full.append(time.perf_counter() - t0)
            full_ok = bool(full.shape[0] == world * N and torch.equal(full[rank * N:(rank + 1) * N].to(payload.device), payload))
            side = torch.tensor([t_e2e, min(t_full), 1.0 if full_ok else 0.0], dtype=torch.float64, device=cdev)
            dist.all_reduce(side[:2], op=dist.ReduceOp.MAX)
            dist.all_reduce(side[2:], op=dist.ReduceOp.MIN)
            multi.update({"end_to_end_ms": round(1e3 * float(side[0]), 4),
                          "end_to_end_note": f"{args.steps} timed steps + the per-frame summary gather, one host clock around both, max over ranks",
                          "full_tensor_gather_ms": round(1e3 * float(side[1]), 4),
                          "full_tensor_gather_bytes_per_rank": int(N * C * 4),
                          "full_tensor_gather_ok": bool(float(side[2]) == 1.0),
                          "full_tensor_gather_note": "all_gather of every rank's fp32 [N, C] result rows (sizes, then padded payload), best of 3, max "
                                                     "over ranks; reported separately, never inside `value` (SURVEY.md 8e)"})

        def neg(x):                                      # a figure this run did not measure (no --full) travels as -1
            return -1.0 if x is None else float(x)
        mine = torch.tensor([[float(rank), float(N), float(M), checksum, elapsed, neg(elapsed_warm), neg(elapsed_single), neg(elapsed_r1),
                              1.0 if affinity["pinned"] else 0.0, float(-1 if affinity["numa_node"] is None else affinity["numa_node"]),
                              float(affinity["cpus"]), float(-1 if affinity["first_cpu"] is None else affinity["first_cpu"]),
                              neg(elapsed_batch)]],
                            dtype=torch.float64, device=cdev)
        rows = gather_frame_rows(mine).cpu()
        elapsed = float(rows[:, 4].max())
        if args.full:
            elapsed_warm = float(rows[:, 5].max())
            elapsed_single = float(rows[:, 6].max())
            elapsed_r1 = float(rows[:, 7].max())
        elapsed_batch = float(rows[:, 12].max()) if bool((rows[:, 12] > 0).all()) else None
        total_vox = float(rows[:, 1].sum())
        rank_rows = [{"rank": int(r[0]), "voxels": int(r[1]), "blocks": int(r[2]), "checksum": float(r[3])}
                     for r in rows[rows[:, 0].argsort()].tolist()]
        affinity_rows = [{"rank": int(r[0]), "pinned": bool(r[8]), "numa_node": (None if r[9] < 0 else int(r[9])), "cpus": int(r[10]),
                          "first_cpu": (None if r[11] < 0 else int(r[11]))} for r in rows[rows[:, 0].argsort()].tolist()]
    else:
        total_vox = float(N)
        rank_rows = [{"rank": 0, "voxels": N, "blocks": int(M), "checksum": checksum}]
        affinity_rows = [dict(rank=0, **{k: affinity[k] for k in ("pinned", "numa_node", "cpus", "first_cpu")})]

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    esz = 4 if args.io == "f32" else 2
    ab = alg_bytes(N, M, C, esz=esz)
    us_frame = 1e6 * elapsed / (args.steps * NS * ROUNDS)
    # The headline of the object is the TIMED REGION: B_alg of a frame over the region's time per frame.  The step is three kernels of
    # similar length that overlap across the frames in flight, so no single launch "is" the step; `kernel` names the longest launch of
    # the timed geometry and `timed_geometry.kernels` carries every launch's own figures (rocprofv3 averages of the committed CSV).
    roofline = {"bound": "hbm", "achieved": round(ab["total"] / (us_frame * 1e-6) / 1e9, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ab["total"] / (us_frame * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                "what": "timed region: B_alg of one frame (SURVEY.md 8d) / measured time per frame / 8 TB/s -- the same number as whole_step.frac",
                "alg_bytes_per_frame": ab["total"], "layout": "dense-cell" if plan.dense else "general",
                "whole_step": {"alg_bytes": ab["total"], "us": round(us_frame, 2),
                               "frac": round(ab["total"] / (us_frame * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                               "note": "per frame: B_alg of one frame over the timed region's time per frame"}}
    tg = kab = cpu = regions = None
    if args.full:
        # ---- instrumented replay: per-kernel durations with HIP events on the launch stream ---------
        import ctypes
        lib = L.lib()
        geometry(1)
        st = torch.cuda.current_stream().cuda_stream
        b, desc = plan.buf, plan.desc
        if plan.dense:
            g = plan.dcg
            # the three launches of one step (index -> pre_mix+modulate+cell sums -> box sum+de-modulate); C = 64
            stages = {
                "index": (lambda: lib.link_dc_index_ids(coords.data_ptr(), N, ctypes.byref(g), b.cnt, b.sid, b.vcell, b.hdr, st))
                if b.tune.k1_form == 1 else
                (lambda: lib.link_dc_index(coords.data_ptr(), N, ctypes.byref(g), b.cnt, b.slots, b.vcell, b.hdr, st)),
                "premix_modsum": lambda: lib.link_dc_premix_modsum(ctypes.byref(b), ctypes.byref(g), ctypes.byref(desc), N, 0, st),
                "gather_demod": lambda: lib.link_dc_gather_demod(ctypes.byref(b), ctypes.byref(g), ctypes.byref(desc), N, st),
            }
            table = ab["block_gather"]
            kab = {"index": N * 16, "premix_modsum": N * esz * C + table, "gather_demod": table + N * esz * C}
            if C != 64:                                   # other widths: box sum and de-modulation are two kernels
                del stages["gather_demod"], kab["gather_demod"]
                stages["gather"] = lambda: lib.link_dc_gather(b.S, b.cell_n, ctypes.byref(desc), ctypes.byref(g), b.A, st)
                stages["demod"] = lambda: lib.link_dc_demod(b.A, b.fin, coords.data_ptr(), b.vcell, b.w_pos, b.alpha, b.ln_w,
                                                            b.ln_b, ctypes.byref(desc), ctypes.byref(g), N, b.out, 0, st)
                kab.update({"gather": table, "demod": N * esz * C})
        elif getattr(plan, "tiles", False):
            grid = plan.grid                               # general layout, tile form: index + two launches
            stages = {
                "index_build(4 kernels)": lambda: lib.link_index_build(
                    coords.data_ptr(), N, ctypes.byref(grid), b.cell_counts, b.scratch, b.scratch_bytes, b.cell_blk,
                    b.vox_blk, b.idx_query, b.perm, b.vox_sorted, b.pos_blk, b.blk_start, b.blk_coords, b.counts, b.hdr, st),
                "premix_modsum_tiles": lambda: lib.link_elk_premix_modsum_tiles(
                    b.feats, b.vox_sorted, b.pos_blk, b.blk_start, b.hdr, b.w_pre, b.pre_ln_w, b.pre_ln_b, b.w_pos, b.alpha,
                    ctypes.byref(desc), N, N, b.S, b.s_bytes, b.fin, st),
                "gather_demod_tiles": lambda: lib.link_elk_gather_demod_tiles(
                    b.S, b.fin, b.vox_sorted, b.pos_blk, b.blk_coords, b.cell_blk, ctypes.byref(grid), b.hdr, b.w_pos, b.alpha,
                    b.ln_w, b.ln_b, ctypes.byref(desc), N, N, b.out, st),
            }
            table = ab["block_gather"]
            kab = {"premix_modsum_tiles": N * 16 + N * esz * C + table, "gather_demod_tiles": table + N * esz * C}
        else:
            grid = plan.grid
            stages = {
                "index_build(4 kernels)": lambda: lib.link_index_build(
                    coords.data_ptr(), N, ctypes.byref(grid), b.cell_counts, b.scratch, b.scratch_bytes, b.cell_blk,
                    b.vox_blk, b.idx_query, b.perm, b.vox_sorted, b.pos_blk, b.blk_start, b.blk_coords, b.counts, b.hdr, st),
                "premix_ln": lambda: lib.link_premix_ln(b.feats, b.w_pre, b.pre_ln_w, b.pre_ln_b, N, C, 1e-6, b.fin, st),
                "modulate_block_sum": lambda: lib.link_modulate_block_sum(
                    b.fin, b.vox_sorted, b.w_pos, b.alpha, b.blk_start, b.hdr, ctypes.byref(desc), N, N, b.S, st),
                "block_gather": lambda: lib.link_block_gather(
                    b.S, b.blk_coords, b.cell_blk, ctypes.byref(grid), b.hdr, ctypes.byref(desc), N, b.A, st),
                "voxel_demod_ln": lambda: lib.link_voxel_demod_ln(
                    b.A, b.fin, b.vox_sorted, b.pos_blk, b.w_pos, b.alpha, b.ln_w, b.ln_b, b.hdr, ctypes.byref(desc),
                    N, b.out, st),
            }
            kab = {k: ab[k] for k in ("premix_ln", "modulate_block_sum", "block_gather", "voxel_demod_ln")}
        assert abs(sum(kab.values()) - ab["total"]) <= 16 * N, "per-kernel split must add up to B_alg"
        k_inst = min(args.steps, 100)
        evs = {name: [] for name in stages}
        for _ in range(k_inst):
            for name, fn in stages.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs[name].append((e0, e1))
        torch.cuda.synchronize()
        kern_us = {name: 1e3 * sum(x.elapsed_time(y) for x, y in v) / len(v) for name, v in evs.items()}
        # whole single-frame steps, device-event timed one by one: median and mean
        step_ev = []
        for _ in range(max(50, min(args.steps, 200))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plan.run(feats, coords)
            e1.record()
            step_ev.append((e0, e1))
        torch.cuda.synchronize()
        step_us = sorted(1e3 * x.elapsed_time(y) for x, y in step_ev)
        core = {k: v for k, v in kern_us.items() if k in kab}
        dom1 = max(core, key=core.get)
        # ---- the same three stages in the TIMED geometry (NS frames in flight on NS streams), device events around every launch: what a
        # kernel costs while the other frames' kernels run beside it.  (An instrumented replay: the timed region itself is never touched.)
        live = None
        if plan.dense and C == 64 and NS > 1:
            geometry(NS)
            sh = [s_.cuda_stream for s_ in streams]
            bj = [plans[j].buf for j in range(NS)]
            for j in range(NS):
                bj[j].feats, bj[j].coords = frames[j][0].data_ptr(), frames[j][1].data_ptr()
            tev = {k: [] for k in ("index", "premix_modsum", "gather_demod")}
            for it in range(min(args.steps, 60) + 5):
                for j in range(NS):
                    with torch.cuda.stream(streams[j]):
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                        ev[0].record()
                        lib.link_dc_index(bj[j].coords, N, ctypes.byref(g), bj[j].cnt, bj[j].slots, bj[j].vcell, bj[j].hdr, sh[j])
                        ev[1].record()
                        lib.link_dc_premix_modsum(ctypes.byref(bj[j]), ctypes.byref(g), ctypes.byref(desc), N, 0, sh[j])
                        ev[2].record()
                        lib.link_dc_gather_demod(ctypes.byref(bj[j]), ctypes.byref(g), ctypes.byref(desc), N, sh[j])
                        ev[3].record()
                    if it >= 5:
                        for q, k in enumerate(tev):
                            tev[k].append((ev[q], ev[q + 1]))
            torch.cuda.synchronize()
            live = {k: round(1e3 * sum(a.elapsed_time(b_) for a, b_ in v) / len(v), 2) for k, v in tev.items()}
            geometry(1)
        # ---- per-kernel figures of the TIMED geometry from the committed rocprofv3 files (profiles/timed_geometry.json, built by
        # tools/r06_profiles.sh + tools/timed_geometry_json.py from the kernel trace of THIS command and the PMC passes over the same
        # geometry): frac = algorithmic bytes per launch / (csv average us) / 8 TB/s -- reproducible from profiles/ by hand
        tg, tg_kern, traffic_frame = None, {}, None
        tgp = os.path.join(ROOT, "profiles", "timed_geometry.json")
        if os.path.exists(tgp) and (N, C) == (100000, 64) and args.io == "f32" and plan.dense:
            tg = json.load(open(tgp))
            for k, v in tg.get("kernels", {}).items():
                if k in kab:
                    tg_kern[k] = {"rocprof_name": v["rocprof_name"], "avg_us": v["avg_us"], "launches": v["launches"], "alg_bytes_per_launch": kab[k],
                                  "achieved_gbs": round(kab[k] / (v["avg_us"] * 1e-6) / 1e9, 1),
                                  "frac": round(kab[k] / (v["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                  "traffic_bytes_per_launch": v.get("traffic_bytes_per_launch"),
                                  "live_event_us_this_run": (live or {}).get(k)}
            if tg_kern and all(v.get("traffic_bytes_per_launch") for v in tg_kern.values()):
                traffic_frame = int(sum(v["traffic_bytes_per_launch"] for v in tg_kern.values()))
        clock_hz, clock_src = SHADER_CLOCK_HZ, "nominal 2.4 GHz (no amdsmi reading)"
        if gpu_state and gpu_state.get("sclk_mhz"):
            clock_hz, clock_src = gpu_state["sclk_mhz"]["median"] * 1e6, "amdsmi median shader clock during a replay of the timed steps"
        dom = max(tg_kern, key=lambda k: tg_kern[k]["avg_us"]) if tg_kern else dom1
        mfma_cyc = (tg or {}).get("kernels", {}).get("premix_modsum", {}).get("mfma_busy_cycles_per_launch")
        mfma_us = tg_kern.get("premix_modsum", {}).get("avg_us")
        roofline.update({"kernel": (tg_kern[dom]["rocprof_name"] if tg_kern else dom), "traffic": traffic_frame,
                         "traffic_what": ("memory-side bytes per FRAME in the timed geometry (sum over the three launches; rocprofv3 --pmc, 2*FETCH_SIZE + WRITE_SIZE)"
                                          if traffic_frame else None),
                         "timed_geometry": ({"source_kernel_stats": tg["source_kernel_stats"], "source_pmc": tg["source_pmc"], "commit": tg["commit"],
                                             "geometry": tg["geometry"], "dominant": dom, "kernels": tg_kern,
                                             "sum_of_launches_over_frames_in_flight_us": round(sum(v["avg_us"] for v in tg_kern.values()) / NS, 2),
                                             "frac_if_the_launches_tiled_without_gaps": round(ab["total"] / (sum(v["avg_us"] for v in tg_kern.values()) / NS * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                             "note": "frac = alg_bytes_per_launch / (avg_us of the committed CSV) / 8 TB/s; live_event_us_this_run = the same "
                                                     "launch bracketed by HIP events on its stream in an instrumented replay of the timed geometry (the bracket holds the stream-ordered "
                                                     "launch boundary too: 3-6 us more than the kernel's own duration in the trace).  The launches "
                                                     "of the frames in flight share the chip (about three are running at any moment), so a launch's OWN fraction "
                                                     "is about a third of what the chip sustains meanwhile: the region's fraction is `roofline.frac`, and the sum "
                                                     "of the three launch durations over the frames in flight is its lower bound for these kernels"}
                                            if tg_kern else None),
                         # north_star: MFMA utilisation of the kernel that holds the dense contraction = SQ_VALU_MFMA_BUSY_CYCLES (cycles, summed over the
                         # chip's 1024 SIMDs; PMC pass in the timed geometry) / (its rocprofv3 duration x 1024 SIMDs x clock)
                         "mfma_util": ({"kernel": "premix_modsum", "busy_cycles_per_launch": mfma_cyc,
                                        "frac": round(mfma_cyc / (mfma_us * 1e-6 * 1024 * clock_hz), 4), "clock_hz": clock_hz, "clock_source": clock_src,
                                        "note": "SQ_VALU_MFMA_BUSY_CYCLES / (kernel us x 1024 SIMDs x shader clock); the contraction is 0.82 GFLOP per frame -- "
                                                "not a grading bound (SURVEY.md 8d)"} if mfma_cyc and mfma_us else None),
                         "single_frame_geometry": {"what": "ONE frame in flight (other launch geometry: matrix-core sums pre_mix at 1024 workgroups): per-stage HIP events "
                                                           "around the stage calls, and whole steps one by one -- NOT the timed region",
                                                   "kernel_us_events": {k: round(v, 2) for k, v in kern_us.items()},
                                                   "dominant": dom1, "dominant_frac": round(kab[dom1] / (core[dom1] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                                   "step_median_us": round(step_us[len(step_us) // 2], 2), "step_mean_us": round(sum(step_us) / len(step_us), 2),
                                                   "n": len(step_us),
                                                   "frac": round(ab["total"] / (step_us[len(step_us) // 2] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}})

        # ---- CPU baseline: the oracle on this host (rank 0, N=1 only) -------------------------------------
        # (1) the OpenMP twin of the C restatement -- pragmas exactly where the reference's CPU ops have them
        #     (voxelize_cpu.cpp:17 inner loop, devoxelize_cpu.cpp:16 outer loop), OMP_NUM_THREADS = physical
        #     cores -- on a bounded sample of the same frame; (2) the same code scalar, one core, full frame.
        if world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline(blk, feats.float(), coords, outs_timed[0].float(), N, C, S_, R, G)   # the TIMED configuration's output

        batch_probe("before the module-surface regions")
        regions = timed_regions(la, blk, feats.float(), coords, C, S_, R) if (world == 1 and args.io == "f32") else None
        batch_probe("after the module-surface regions")
    ms = 1e3 * elapsed / args.steps
    frames_timed = args.steps * NS * ROUNDS          # per GPU
    line = {
        "metric": "voxels/s through one LinK (3x7)^3 block, 100k active voxels C=64",
        "value": round(total_vox * frames_timed / elapsed, 1), "unit": "voxels/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "settle_steps_before_warmup": settle_regions * settle_k, "ms_per_step": round(ms, 5),
        "ms_per_step_event_median": round(batch_ev["median_us"] * ROUNDS * 1e-3, 5) if batch_ev else None, "batch_period_events": batch_ev,
        "frames_per_step": NS * ROUNDS * world,
        "step_definition_version": 2,   # 1 (rounds 1-4): a step = one batch of the 3 frames in flight; 2 (round 5 on): 8 such batches = 24 frames
                                        # per GPU.  `three_frame_step` is the version-1 figure of the same run
        "three_frame_step": {"us_per_frame": round(1e6 * elapsed_r1 / (args.steps * NS), 2), "ms_per_step": round(1e3 * elapsed_r1 / args.steps, 5),
                             "frac": round(97520688 / (elapsed_r1 / (args.steps * NS)) / 1e9 / HBM_PEAK_GBS, 4) if (N, C) == (100_000, 64) else None,
                             "note": f"the same {args.steps} steps with a batch of {NS} frames per step (what rounds 1-4 timed): a region pays ~150 us "
                                     "for filling / draining the pipeline around its two synchronisations"} if elapsed_r1 is not None else None,
        "us_per_frame": round(1e6 * elapsed / frames_timed, 2), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.io == "f32" else f"{args.io} rows at the boundary, f32 contraction / block table / statistics",
        "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[1]: S-uniform 100k voxels in 256^3, C=64, one LinK "
                               "cos:(3x7)^3 block forward (R_core, index rebuilt every step)",
                   "voxels_per_frame": N, "blocks_per_frame": M, "channels": C, "baseop": "cos", "groups": G,
                   "r": R, "s": S_, "frames_in_flight_per_gpu": NS,
                   "contraction": ("fp16 hi/lo split of both operands on the f16 matrix cores, fp32 accumulate (22-bit operands, "
                                   "exact products; fp32 instruction outside the fp16 range)" if args.io != "f16" else
                                   "fp16 rows x fp16 hi/lo split weights on the f16 matrix cores, fp32 accumulate"),
                   "step": f"one batch of {NS * ROUNDS} independent frames per GPU, {NS} in flight at a time (one per HIP stream; "
                           f"{ROUNDS} rounds); value = voxels of all timed frames / time",
                   "parallelism": f"{world} GPU(s) x {NS} independent frames in flight (one HIP stream each), "
                                  "no data-path collective"},
        "single_stream_value": round(total_vox * frames_timed / elapsed_single, 1) if elapsed_single is not None else None,
        "warm_index_value": round(total_vox * frames_timed / elapsed_warm, 1) if elapsed_warm is not None else None,
        "timed_configuration_check": timed_check,
        "gpu_state": gpu_state,        # shader / memory clock and socket power under this load (amdsmi)
        "ranks": rank_rows,          # the trivial result gather: one summary row per rank (frame 0 of each rank)
        "cpu_affinity": {"ranks": affinity_rows, "rank0_reason": affinity["reason"],
                         "note": "N > 1: every rank pins itself to CPUs of its GPU's NUMA node (link_amd.parallel.pin_rank_to_gpu_numa); "
                                 "LINK_BENCH_PIN=0/1 overrides"},
        "multi_gpu": multi,          # N > 1 only: backend, all_reduce check, end-to-end time, full-tensor gather
        "roofline": roofline, "cpu_baseline": cpu, "regions": regions,
        "frame_streams": frame_stream_check,         # the NS frame streams sit on hardware queues of their own (link_streams_share_queue)
    }
    # ---- the two ways through the K steps: three plans on three streams (what the fields above describe) and the batch entry point
    # (include/link_amd.h section H: one insert kernel + two persistent, queue-fed role kernels per call of FB frames, two arena sets,
    # submit(s + 1) before join(s)).  Same frames, same rows (checked bit for bit), both timed under the same contract; the faster one
    # is `value` / `ms_per_step` / `us_per_frame` / `roofline` of the line, both are in `paths`.
    streams_path = {"us_per_frame": round(1e6 * elapsed / frames_timed, 2), "ms_per_step": round(ms, 5), "value": round(total_vox * frames_timed / elapsed, 1),
                    "frac": roofline["frac"], "what": f"{NS} ElkCorePlan on {NS} HIP streams, one link_elk_core_dense_forward call (3 launches) per frame"}
    line["paths"] = {"streams": streams_path, "batch": None, "headline": "streams"}
    line["config"]["path"] = "streams"
    if isinstance(bsets, str) or batch_fail:
        line["batch_entry_point"] = {"error": bsets if isinstance(bsets, str) else batch_fail}
    elif bsets is not None and elapsed_batch is not None:
        try:
            ok = True
            for b_ in bsets:                             # the rows of a full call against the rows the streams' timed steps wrote
                outs_b = b_.run(bfe0, bco0)
                torch.cuda.synchronize()
                b_.check()
                ok &= all(torch.equal(outs_b[i], outs_timed[i % NS]) for i in range(FB))
            # the three kernels of a launch set bracketed by timed events on their own streams, in steady state (the last of four calls)
            live_b = None
            if args.full:
                bsets[0].set_timing(True)
                prev_ = None
                for s_ in range(4):
                    _, tk_ = bsets[s_ % 2].submit(bfe0, bco0, stream=bstream.cuda_stream)
                    if prev_ is not None:
                        bsets[0].join(prev_, stream=bstream.cuda_stream)
                    prev_ = tk_
                bsets[0].join(prev_, stream=bstream.cuda_stream)
                torch.cuda.synchronize()
                live_b = bsets[0].kernel_times_us(prev_)
                bsets[0].set_timing(False)
            usb = 1e6 * elapsed_batch / frames_timed
            fracb = round(ab["total"] / (usb * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
            tgb, bk = (tg or {}).get("batch"), {}
            names = {"insert": "index", "premix_modsum": "premix_modsum", "gather_demod": "gather_demod"}
            if tgb and tgb.get("frames_per_call") == FB and args.io == "f32":
                for i_, (k_, kk) in enumerate(names.items()):
                    v = tgb["kernels"].get(k_)
                    if v:
                        ablb = kab[kk] * FB
                        bk[k_] = {"rocprof_name": v["rocprof_name"], "avg_us": v["avg_us"], "launches": v["launches"], "frames_per_launch": FB,
                                  "alg_bytes_per_launch": ablb, "achieved_gbs": round(ablb / (v["avg_us"] * 1e-6) / 1e9, 1),
                                  "frac": round(ablb / (v["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "traffic_bytes_per_launch": None,
                                  "live_event_us_this_run": round(live_b[i_], 1)}
            batch_path = {"us_per_frame": round(usb, 2), "ms_per_step": round(1e3 * elapsed_batch / args.steps, 5),
                          "value": round(total_vox * frames_timed / elapsed_batch, 1), "frac": fracb,
                          "what": f"ElkCoreBatch / link_dc_batch_submit + link_dc_batch_join: calls of {FB} frames (3 launches per call: slot insert of the "
                                  "batch + persistent pre_mix and gather role kernels fed by per-XCD cursors, per-frame arrival counters instead of "
                                  "launch boundaries), two arena sets, call s + 1 submitted before call s is joined (DESIGN.md 4i)",
                          "frames_per_call": FB, "placement_trials_us_per_frame": btrials, "bitwise_equal_to_the_streams_rows": bool(ok),
                          "kernel_brackets_us_this_run": ({"insert": round(live_b[0], 1), "premix_modsum": round(live_b[1], 1),
                                                           "gather_demod": round(live_b[2], 1)} if live_b else None)}
            line["paths"]["batch"] = batch_path
            line["batch_entry_point"] = {**batch_path, "calls_in_flight": "submit(s + 1) before join(s), one caller stream", "arena_sets_in_flight": 2,
                                         "bitwise_equal_to_timed_configuration": bool(ok)}
            if ok and elapsed_batch < elapsed and os.environ.get("LINK_BENCH_HEADLINE", "") != "streams":
                # the batch entry point is the faster way through the K steps: it is the line's headline
                line["paths"]["headline"] = "batch"
                line["config"]["path"] = "batch"
                line["config"]["step"] = (f"one batch of {NS * ROUNDS} independent frames per GPU through link_dc_batch_submit / _join in calls of {FB} frames "
                                          "(two arena sets, two calls in flight); value = voxels of all timed frames / time")
                line["config"]["parallelism"] = f"{world} GPU(s) x calls of {FB} independent frames (persistent role kernels), no data-path collective"
                line["value"], line["ms_per_step"], line["us_per_frame"] = batch_path["value"], batch_path["ms_per_step"], batch_path["us_per_frame"]
                rl = dict(roofline)
                rl["streams_path"] = {k_: roofline[k_] for k_ in ("kernel", "achieved", "frac", "traffic", "traffic_what", "timed_geometry", "whole_step") if k_ in roofline}
                domb = max(bk, key=lambda k_: bk[k_]["avg_us"]) if bk else "gather_demod"
                rl.update({"kernel": bk[domb]["rocprof_name"] if bk else "k_dc_batch_k2", "achieved": round(ab["total"] / (usb * 1e-6) / 1e9, 1), "frac": fracb,
                           "what": "timed region (batch entry point): B_alg of one frame (SURVEY.md 8d) / measured time per frame / 8 TB/s -- the same number as whole_step.frac",
                           "traffic": None, "traffic_what": None,
                           "whole_step": {"alg_bytes": ab["total"], "us": round(usb, 2), "frac": fracb,
                                          "note": "per frame: B_alg of one frame over the timed region's time per frame"},
                           "timed_geometry": ({"source_kernel_stats": tg["source_kernel_stats"], "source_pmc": None, "commit": tg["commit"],
                                               "geometry": tgb.get("geometry"), "dominant": domb, "kernels": bk,
                                               "note": "frac = alg_bytes_per_launch (frames_per_launch x the kernel's bytes per frame) / (avg_us of the committed "
                                                       "CSV) / 8 TB/s; live_event_us_this_run = the launch bracketed by timed events on its own stream in THIS "
                                                       "run (link_dc_batch_kernel_times).  The three kernels of a call run side by side for the whole call "
                                                       "(and beside the neighbouring calls' kernels), so a kernel's own fraction is below the region's; "
                                                       "the CSV's averages include the calls of the calibration's other contexts"} if bk else None)})
                line["roofline"] = rl
        except Exception as e:                          # a second path must never cost the line
            line["batch_entry_point"] = {"error": repr(e)[:200]}
    del bsets
    if args.dump_outputs is not None:
        dump_outputs(args.dump_outputs, outs_batch if line["paths"]["headline"] == "batch" else outs_timed)
    print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
