"""tools/amp_train_step.py -- one training step of the reference-shaped ELKUNet and encoder (harness/networks.py, C = 64,
cos_x, s = 3, r = 2) on an S-kitti frame (link_amd/synth.py), in fp32 and under fp16 torch.autocast + GradScaler (the
reference trainer's amp_enabled mode): forward, cross-entropy (UNet) / sum of squares (encoder), backward, SGD step.

    python tools/amp_train_step.py [--net unet|encoder|both] [--steps 5] [--warmup 2] [--n-az 4608] [--profile]
                                   [--criterion cross_entropy|lovasz_softmax] [--lovasz-impl fused|torch_loop]

--criterion lovasz_softmax is the loss the reference's configs train with (CrossEntropyLoss(ignore_index=255) + lovasz_softmax(...,
ignore=0), trainers.py:64-73): by default link_amd.SegCriterion (csrc/segloss.hip), with --lovasz-impl torch_loop the torch
restatement of the reference's loop in tools/segloss_bench.py.  The default stays plain cross-entropy.

Prints one JSON line per (net, mode): ms per step (median of --steps after --warmup, HIP events), peak memory of the
timed steps.  --profile re-runs every (net, mode) in a child process under `rocprofv3 --kernel-trace --stats` and adds
the per-step count of the at::native batch-norm / layer-norm / elementwise kernels still launched (calls of the
profiled run divided by its steps, warm-up included)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _run(net_name: str, amp: bool, steps: int, warmup: int, n_az: int, criterion: str = "cross_entropy", impl: str = "fused") -> dict:
    import torch
    import link_amd as la
    from harness import networks as N
    from link_amd.synth import s_kitti
    dev = torch.device("cuda", 0)
    co, fe = s_kitti(seed=0, n_az=n_az)
    coords, feats = torch.from_numpy(co).to(dev), torch.from_numpy(fe).to(dev)
    torch.manual_seed(0)
    if net_name == "unet":
        net = N.build_reference_shaped_unet(la, cr=1.0, baseop="cos_x", groups=1, s=3, r=2, num_classes=19)
        labels = torch.randint(0, 19, (coords.shape[0],), generator=torch.Generator().manual_seed(1)).to(dev)
    else:
        net = N.build_reference_shaped_encoder(la, 64, "cos_x", 1)
    net = net.to(dev).train()
    if criterion == "cross_entropy":
        crit = torch.nn.functional.cross_entropy
    elif impl == "fused":
        crit = la.SegCriterion()
    else:
        from segloss_bench import torch_loop_criterion as crit
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    scaler = torch.amp.GradScaler("cuda", enabled=amp)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", torch.float16, enabled=amp):
            x = la.SparseTensor(feats, coords, 1)
            if net_name == "unet":
                loss = crit(net(x), labels)
            else:
                _, outs = net(x, 3, 2)
                loss = outs[-1].F.float().square().mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = step()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"net": net_name, "mode": "fp16_autocast" if amp else "fp32", "voxels": int(coords.shape[0]),
            "criterion": criterion if criterion == "cross_entropy" or net_name != "unet" else f"{criterion}:{impl}",
            "ms_per_step": round(times[len(times) // 2], 2), "ms_min": round(times[0], 2),
            "peak_mem_mib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1), "loss": float(loss)}


def _classify(name: str):
    if "at::native" not in name:
        return None
    low = name.lower()
    if "batch_norm" in low:
        return "batch_norm"
    if "layer_norm" in low:
        return "layer_norm"
    if "elementwise" in low:
        return "elementwise"
    return None


def _profile(net_name: str, amp: bool, steps: int, warmup: int, n_az: int) -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--net", net_name, "--mode", "amp" if amp else "fp32",
               "--steps", str(steps), "--warmup", str(warmup), "--n-az", str(n_az)] + EXTRA
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        counts = {"batch_norm": 0, "layer_norm": 0, "elementwise": 0}
        total = 0
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                calls = int(row.get("Calls", 0))
                total += calls
                k = _classify(row.get("Name", ""))
                if k:
                    counts[k] += calls
    per = steps + warmup
    return {"kernels_per_step": round(total / per, 1),
            **{f"at_native_{k}_per_step": round(v / per, 1) for k, v in counts.items()}}


EXTRA = []                                                     # --criterion / --lovasz-impl, handed on to the profiled child


def main():
    global EXTRA
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="both", choices=["unet", "encoder", "both"])
    ap.add_argument("--mode", default="both", choices=["fp32", "amp", "both"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=4608)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--criterion", default="cross_entropy", choices=["cross_entropy", "lovasz_softmax"])
    ap.add_argument("--lovasz-impl", default="fused", choices=["fused", "torch_loop"])
    a = ap.parse_args()
    EXTRA = ["--criterion", a.criterion, "--lovasz-impl", a.lovasz_impl]
    nets = ["unet", "encoder"] if a.net == "both" else [a.net]
    modes = [False, True] if a.mode == "both" else [a.mode == "amp"]
    for net in nets:
        for amp in modes:
            res = _run(net, amp, a.steps, a.warmup, a.n_az, a.criterion, a.lovasz_impl)
            if a.profile:
                res.update(_profile(net, amp, 3, 1, a.n_az))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
