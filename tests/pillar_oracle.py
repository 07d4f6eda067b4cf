"""tests/pillar_oracle.py -- the arbiter of the PointPillars reader tests (section S of include/link_amd.h): a restatement, in this
project's own words, of what the reference's PillarFeatureNet and PointPillarsScatter compute, in plain torch on the CPU, in
whatever float type the inputs have (float64 is the truth, float32 measures what evaluating the same formula in fp32 costs).  The
recordings under tests/golden/pillar_*.npz were made from the reference's own classes (tools/make_pillar_golden.py); the CPU tests
hold this file to them, the GPU tests hold the kernels to this file.

State dicts use the reference's names: pfn_layers.{i}.linear.weight, pfn_layers.{i}.norm.{weight, bias, running_mean, running_var,
num_batches_tracked}.  A `cfg` is a dict: num_filters, with_distance, voxel_size, pc_range (and D, T for the case builders).

rows = "all"      every one of the T rows goes through every layer and into the max (the reference)
       "valid"    the max runs over the rows t < num only -- NOT what the reference computes; the tests show the difference
       "compact"  the rows t < num and ONE padded row where num < T: equal to "all", a fraction of the arithmetic
"""
import glob
import os

import numpy as np
import torch

EPS, MOMENTUM = 1e-3, 0.01
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def n_layers(cfg):
    return len(cfg["num_filters"])


def units(cfg, i):
    f = cfg["num_filters"][i]
    return f if i == n_layers(cfg) - 1 else f // 2


def in_width(cfg, i, D):
    return D + 5 + int(bool(cfg["with_distance"])) if i == 0 else cfg["num_filters"][i - 1] // 2 * 2


def decorate(x, num, coors, cfg):
    """[P, T, D] -> masked [P, T, D + 5 (+ 1)]"""
    P, T, _ = x.shape
    dt = x.dtype
    vx, vy = cfg["voxel_size"][0], cfg["voxel_size"][1]
    x_off, y_off = vx / 2 + cfg["pc_range"][0], vy / 2 + cfg["pc_range"][1]
    xyz = x[:, :, :3]
    mean = xyz.sum(dim=1, keepdim=True) / num.to(dt).view(P, 1, 1)
    cx = coors[:, 3].to(dt).view(P, 1) * vx + x_off
    cy = coors[:, 2].to(dt).view(P, 1) * vy + y_off
    cols = [x, xyz - mean, (x[:, :, 0] - cx)[..., None], (x[:, :, 1] - cy)[..., None]]
    if cfg["with_distance"]:
        cols.append(xyz.pow(2).sum(-1, keepdim=True).sqrt())
    mask = (torch.arange(T).view(1, T) < num.view(P, 1)).to(dt)[..., None]
    return torch.cat(cols, -1) * mask


def _bn_eval(y, sd, i):
    p = f"pfn_layers.{i}.norm."
    return (y - sd[p + "running_mean"]) / torch.sqrt(sd[p + "running_var"] + EPS) * sd[p + "weight"] + sd[p + "bias"]


def _bn_train(y, sd, i, new_stats):
    p = f"pfn_layers.{i}.norm."
    flat = y.reshape(-1, y.shape[-1])
    n = flat.shape[0]
    mean = flat.mean(0)
    var = ((flat - mean) ** 2).mean(0)
    if new_stats is not None:
        new_stats[p + "running_mean"] = ((1 - MOMENTUM) * sd[p + "running_mean"] + MOMENTUM * mean).detach()
        new_stats[p + "running_var"] = ((1 - MOMENTUM) * sd[p + "running_var"] + MOMENTUM * var * n / (n - 1)).detach()
        new_stats[p + "num_batches_tracked"] = sd[p + "num_batches_tracked"] + 1
    return (y - mean) / torch.sqrt(var + EPS) * sd[p + "weight"] + sd[p + "bias"]


def _layers(dec, sd, cfg, keep=None, training=False, new_stats=None):
    """dec [P, R, K] -> [P, C]; keep [P, R] bool: the rows that enter the max (None: all)"""
    x = dec
    for i in range(n_layers(cfg)):
        y = x @ sd[f"pfn_layers.{i}.linear.weight"].t()
        y = _bn_train(y, sd, i, new_stats) if training else _bn_eval(y, sd, i)
        y = torch.relu(y)
        cand = y if keep is None else torch.where(keep[..., None], y, torch.full_like(y, -float("inf")))
        top = cand.max(dim=1, keepdim=True)[0]
        if i == n_layers(cfg) - 1:
            return top[:, 0]
        x = torch.cat([y, top.expand(-1, y.shape[1], -1)], -1)


def reader(x, num, coors, sd, cfg, rows="all", training=False, new_stats=None):
    """-> [P, C] in x's type.  sd's tensors must have x's type.  training: batch statistics over all P T rows (rows = "all" only);
    new_stats, a dict, receives the updated running statistics."""
    dec = decorate(x, num, coors, cfg)
    P, T, _ = dec.shape
    if rows == "all":
        return _layers(dec, sd, cfg, training=training, new_stats=new_stats)
    assert not training
    if rows == "valid":
        return _layers(dec, sd, cfg, keep=torch.arange(T).view(1, T) < num.view(P, 1))
    assert rows == "compact"
    out = []
    for p in range(P):
        n = int(num[p])
        r = dec[p, :n]
        if n < T:
            r = torch.cat([r, torch.zeros_like(dec[p, :1])])
        out.append(_layers(r[None], sd, cfg)[0])
    return torch.stack(out)


def scatter(rows, coors, B, ny, nx):
    """rows [P, C] -> [B, C, ny, nx]; cells are unique in every case here"""
    canvas = torch.zeros((B, rows.shape[1], ny, nx), dtype=rows.dtype)
    c = coors.long()
    canvas[c[:, 0], :, c[:, 2], c[:, 3]] = rows
    return canvas


def cast_sd(sd, dt):
    return {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def make_state(cfg, D, seed):
    """randomised weights AND BatchNorm parameters and running statistics: with the defaults (gamma 1, beta 0, mean 0, var 1) a padded
    row leaves a layer as exactly 0 and cannot win a max, which would hide the reference's padded-row behaviour"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(n_layers(cfg)):
        u, k = units(cfg, i), in_width(cfg, i, D)
        p = f"pfn_layers.{i}."
        sd[p + "linear.weight"] = torch.randn(u, k, generator=g) / k ** 0.5
        sd[p + "norm.weight"] = 0.5 + torch.rand(u, generator=g)
        sd[p + "norm.bias"] = 0.5 * torch.randn(u, generator=g)
        sd[p + "norm.running_mean"] = 0.5 * torch.randn(u, generator=g)
        sd[p + "norm.running_var"] = 0.5 + torch.rand(u, generator=g)
        sd[p + "norm.num_batches_tracked"] = torch.tensor(3, dtype=torch.long)
    return sd


def make_cfg(num_filters, D, T, with_distance=False, family="near"):
    """0.2 m pillars.  family "far": the canvas starts at x = 50 m, y = -50.6 m, so f_cluster and f_center cancel 50 m against
    50 m in fp32 (the production situation at the edge of the range); "near": it starts at the origin."""
    x0, y0 = (50.0, -50.6) if family == "far" else (0.0, -0.6)
    return {"num_filters": tuple(num_filters), "with_distance": bool(with_distance), "voxel_size": (0.2, 0.2, 8.0),
            "pc_range": (x0, y0, -5.0, x0 + 102.4, y0 + 102.4, 3.0), "D": int(D), "T": int(T)}


def make_nums(P, T, pattern, g):
    if pattern == "ones":
        return torch.ones(P, dtype=torch.int32)
    if pattern == "full":
        return torch.full((P,), T, dtype=torch.int32)
    if pattern == "tm1":
        return torch.full((P,), max(T - 1, 1), dtype=torch.int32)
    assert pattern == "mixed"
    n = torch.randint(1, T + 1, (P,), generator=g, dtype=torch.int32)
    n[0] = T                                      # the representative padded row absent ...
    if P > 1:
        n[1] = 1                                  # ... and present, whatever the draw
    return n


def make_case(P, cfg, B, ny, nx, pattern="mixed", seed=0):
    """-> features float32 [P, T, D] (padded rows zero), num int32 [P], coors int32 [P, 4] = b, z, y, x.  The cells are distinct, the
    four corners of sample 0 come first, and with B > 1 sample 1 has no pillar.  P <= (B - 1 or 1) ny nx."""
    T, D = cfg["T"], cfg["D"]
    g = torch.Generator().manual_seed(1000 + seed)
    samples = [b for b in range(B) if not (B > 1 and b == 1)]
    cells = [(b, y, x) for b in samples for y in range(ny) for x in range(nx)]
    assert P <= len(cells), (P, len(cells))
    corners = [(samples[0], 0, 0), (samples[0], 0, nx - 1), (samples[0], ny - 1, 0), (samples[0], ny - 1, nx - 1)]
    corners = list(dict.fromkeys(corners))
    rest = [c for c in cells if c not in corners]
    perm = torch.randperm(len(rest), generator=g).tolist()
    chosen = (corners + [rest[i] for i in perm])[:P]
    coors = torch.tensor([[b, 0, y, x] for b, y, x in chosen], dtype=torch.int32).reshape(P, 4)
    num = make_nums(P, T, pattern, g)
    vx, vy = cfg["voxel_size"][0], cfg["voxel_size"][1]
    u = torch.rand(P, T, 2, generator=g)
    feats = torch.zeros(P, T, D)
    feats[:, :, 0] = cfg["pc_range"][0] + (coors[:, 3:4].float() + u[:, :, 0]) * vx
    feats[:, :, 1] = cfg["pc_range"][1] + (coors[:, 2:3].float() + u[:, :, 1]) * vy
    feats[:, :, 2] = -5.0 + 8.0 * torch.rand(P, T, generator=g)
    if D > 3:
        feats[:, :, 3:] = torch.rand(P, T, D - 3, generator=g)
    feats = feats * (torch.arange(T).view(1, T) < num.view(P, 1)).float()[..., None]
    return feats, num, coors


# ---- recordings -----------------------------------------------------------------------------------------------------------------------
def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "pillar_*.npz")))


def load_golden(path):
    """-> dict: cfg, B, ny, nx, features, num, coors, sd (float32 tensors), and every recorded array as a tensor under its own name"""
    z = np.load(path)
    out = {k: torch.from_numpy(z[k]) for k in z.files}
    cfg = {"num_filters": tuple(int(v) for v in z["cfg_num_filters"]), "with_distance": bool(z["cfg_with_distance"]),
           "voxel_size": tuple(float(v) for v in z["cfg_voxel_size"]), "pc_range": tuple(float(v) for v in z["cfg_pc_range"]),
           "D": int(z["features"].shape[2]), "T": int(z["features"].shape[1])}
    out["cfg"] = cfg
    out["B"], out["ny"], out["nx"] = int(z["B"]), int(z["ny"]), int(z["nx"])
    out["train"] = bool(z["train"])
    out["sd"] = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    return out
