"""Restatements of deformable convolution (DCN v1) for the tests of link_amd/dcn.py and csrc/dcn.hip.  Not a test file.

  1. dcn(x, offset, weight, ...) on float64 tensors: the formula of include/link_amd.h section R with gathered corners and
     torch.where for the range test, so a non-finite offset yields 0 and not NaN.  Differentiable: autograd gives the three
     reference gradients.
  2. The same code on float32 tensors: the stand-in for the reference's float32 error (the reference runs on CUDA only and no
     recording of it exists).
  3. dcn_grid_sample: F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True) per tap and group followed by a 1 x 1
     contraction -- an independent second definition (finite offsets only).
"""
import numpy as np
import torch
import torch.nn.functional as F


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(H, W, kh, kw, stride, pad, dil):
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(pad), pair(dil)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def coords(offset, H, W, kh, kw, stride, pad, dil, dg):
    """sample coordinates h, w [B, dg, K, Ho, Wo] in offset's type"""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(pad), pair(dil)
    B, _, Ho, Wo = offset.shape
    off = offset.reshape(B, dg, kh * kw, 2, Ho, Wo)
    hs, ws = [], []
    for i in range(kh):
        for j in range(kw):
            t = i * kw + j
            hs.append((torch.arange(Ho, dtype=offset.dtype) * sh - ph + i * dh).view(1, 1, Ho, 1) + off[:, :, t, 0])
            ws.append((torch.arange(Wo, dtype=offset.dtype) * sw - pw + j * dw).view(1, 1, 1, Wo) + off[:, :, t, 1])
    return torch.stack(hs, 2), torch.stack(ws, 2)


def columns(x, offset, kh, kw, stride, pad, dil, dg):
    """[B, C, K, Ho, Wo]"""
    B, C, H, W = x.shape
    cg = C // dg
    h, w = coords(offset, H, W, kh, kw, stride, pad, dil, dg)
    K, Ho, Wo = h.shape[2:]
    ok = (h > -1) & (w > -1) & (h < H) & (w < W)
    zero = torch.zeros((), dtype=x.dtype)
    h, w = torch.where(ok, h, zero), torch.where(ok, w, zero)
    h0, w0 = torch.floor(h), torch.floor(w)
    lh, lw = h - h0, w - w0
    xg = x.reshape(B, dg, cg, 1, H * W).expand(B, dg, cg, K, H * W)
    total = 0
    for a, b, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        hi, wi = (h0 + a).long(), (w0 + b).long()
        inb = ok & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        idx = (hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1)).reshape(B, dg, 1, K, Ho * Wo).expand(B, dg, cg, K, Ho * Wo)
        total = total + torch.gather(xg, 4, idx) * torch.where(inb, wt, zero).reshape(B, dg, 1, K, Ho * Wo)
    return total.reshape(B, C, K, Ho, Wo)


def dcn(x, offset, weight, stride=1, pad=0, dil=1, dg=1, relu=False):
    O, C, kh, kw = weight.shape
    cols = columns(x, offset, kh, kw, stride, pad, dil, dg)
    out = torch.einsum("bckhw,ock->bohw", cols, weight.reshape(O, C, kh * kw))
    return torch.relu(out) if relu else out


def dcn_grid_sample(x, offset, weight, stride=1, pad=0, dil=1, dg=1):
    B, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    cg = C // dg
    h, w = coords(offset, H, W, kh, kw, stride, pad, dil, dg)
    out = 0
    for g in range(dg):
        for t in range(kh * kw):
            grid = torch.stack([2 * w[:, g, t] / (W - 1) - 1, 2 * h[:, g, t] / (H - 1) - 1], -1)
            s = F.grid_sample(x[:, g * cg:(g + 1) * cg], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            out = out + torch.einsum("bchw,oc->bohw", s, weight[:, g * cg:(g + 1) * cg, t // kw, t % kw])
    return out


def grads(fn, x, offset, weight, grad_out, **kw):
    """(out, grad_x, grad_offset, grad_weight) of fn under the upstream gradient grad_out"""
    xr, fr, wr = (t.detach().clone().requires_grad_(True) for t in (x, offset, weight))
    out = fn(xr, fr, wr, **kw)
    gx, gf, gw = torch.autograd.grad(out, (xr, fr, wr), grad_out)
    return out.detach(), gx, gf, gw


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def off_grid(a, rng, shape):
    """values of `a` moved so that each lies at least 1/16 from an integer (base coordinates are integers, so the sample coordinates
    do as well): the fraction is redrawn in [1/16, 15/16]"""
    return np.floor(a) + rng.uniform(1 / 16, 15 / 16, shape)


def make_offsets(family, shape, seed):
    """float32 offsets [B, dg 2 K, Ho, Wo] of one family: zeros, uniform (+-0.9), normal (sigma 3), integer ([-3, 3]), nonfinite (normal
    with a sprinkling of NaN, +-inf, +-1e30).  The random real-valued families keep 1/16 away from the integers.  -> (offsets, mask of
    the non-finite or huge entries)."""
    rng = np.random.default_rng(seed)
    bad = np.zeros(shape, bool)
    if family == "zeros":
        off = np.zeros(shape)
    elif family == "uniform":
        off = off_grid(rng.uniform(-0.9, 0.9, shape), rng, shape)
        off = np.clip(off, -0.9, 0.9)                                                  # +-0.9 is 0.1 from an integer
    elif family == "integer":
        off = rng.integers(-3, 4, shape).astype(np.float64)
    elif family in ("normal", "nonfinite"):
        off = off_grid(rng.normal(0, 3, shape), rng, shape)
        if family == "nonfinite":
            pick = rng.uniform(size=shape) < 0.08
            vals = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30]), shape)
            off = np.where(pick, vals, off)
            bad = pick
    else:
        raise ValueError(family)
    return off.astype(np.float32), bad


def make_case(B, C, O, dg, H, W, kh, kw, stride, pad, dil, family, seed):
    """float32 tensors (x, offset, weight, grad_out) and the mask of bad offset entries; the float32 values are the case: the float64
    oracle runs on their exact widenings"""
    rng = np.random.default_rng(1000 + seed)
    Ho, Wo = out_hw(H, W, kh, kw, stride, pad, dil)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    wgt = (rng.standard_normal((O, C, kh, kw)) / np.sqrt(C * kh * kw)).astype(np.float32)
    off, bad = make_offsets(family, (B, dg * 2 * kh * kw, Ho, Wo), seed)
    go = rng.standard_normal((B, O, Ho, Wo)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, off, wgt, go)) + (torch.from_numpy(bad),)
