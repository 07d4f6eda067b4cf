"""The arbiter of the segmentation criterion (tests/test_cpu_segloss.py, tests/test_gpu_segloss.py): cross-entropy + Lovasz-softmax as
include/link_amd.h section K states them, in torch on the CPU through autograd, in float64 or float32.

make_case        seeded inputs: skewed class frequencies, an absent class, a class with one row, ~3 % of rows labelled 255, label 0
                 present; logits scale * randn with + 1.5 at the label, so foreground and background errors interleave.
reference        {"total", "ce", "lovasz", "grad"} in `dtype`; one class at a time, stable descending sort, lovasz_grad in closed form.
closed_form_g / jaccard_g   the closed form and the reference's Jaccard differences (lovasz_losses.py:21-33) on a 0/1 vector.
ambiguous_rows   rows whose gradient an fp32 evaluation may legitimately order differently (mask for gradient comparisons only).
yardstick        (r64, o32, mask): the float64 result, what evaluating the SAME formula in fp32 costs against it per tensor
                 (gradient outside the mask), and the mask.

Test infrastructure only: imports nothing from link_amd."""
import numpy as np
import torch

from helpers import rel_err

MASK_CAP = 0.02


def make_case(n, C, seed, scale=3.0):
    """(logits float32 [n, C], labels int64 [n])"""
    g = torch.Generator().manual_seed(seed)
    absent, single = C - 1, C - 2                                           # for C < 4 a class may play two parts: see below
    w = 1.0 / (torch.arange(C, dtype=torch.float64) + 1)
    if C > 2:
        w[absent] = 0
    if C > 3:
        w[single] = 0
    labels = torch.multinomial(w, n, replacement=True, generator=g)
    if n >= 4:
        labels[0] = 0                                                      # label 0 present: ignore=0 bites
        if C > 3:
            labels[n // 2] = single                                        # a class with exactly one row
        n255 = max(1, int(0.03 * n))
        idx = torch.randperm(n - 1, generator=g)[:n255] + 1
        idx = idx[idx != n // 2]
        labels[idx] = 255
    logits = scale * torch.randn(n, C, generator=g)
    inside = labels < C
    logits[inside, labels[inside]] += 1.5
    return logits.float(), labels


def closed_form_g(fg_sorted):
    """g_k of a 0/1 vector in sorted order, float64: 1 / U_k (foreground), (n_c - F_k) / (U_{k-1} U_k) (background), U_k = n_c + B_k"""
    fg = fg_sorted.to(torch.float64)
    n_c = fg.sum()
    F = fg.cumsum(0)
    U = n_c + (1 - fg).cumsum(0)
    Up = U - 1
    bg = torch.where(Up > 0, (n_c - F) / (Up * U).clamp_min(1), torch.ones_like(U))
    return torch.where(fg > 0, 1 / U.clamp_min(1), bg)


def jaccard_g(fg_sorted):
    """lovasz_grad of the reference (lovasz_losses.py:21-33), restated in float64"""
    fg = fg_sorted.to(torch.float64)
    gts = fg.sum()
    inter = gts - fg.cumsum(0)
    union = gts + (1 - fg).cumsum(0)
    j = 1.0 - inter / union
    if len(fg) > 1:
        j[1:] = j[1:] - j[:-1].clone()
    return j


def lovasz_flat(p, labels, classes="present", ignore=None):
    """p [n, C] (requires grad or not), labels int64 [n] -> scalar, in p's dtype"""
    valid = torch.ones_like(labels, dtype=torch.bool) if ignore is None else labels != ignore
    pv, lv = p[valid], labels[valid]
    losses = []
    if pv.shape[0] > 0:
        for c in range(p.shape[1]):
            fg = lv == c
            if classes == "present" and int(fg.sum()) == 0:
                continue
            err = (fg.to(p.dtype) - pv[:, c]).abs()
            es, perm = torch.sort(err, descending=True, stable=True)
            losses.append((es * closed_form_g(fg[perm]).to(p.dtype)).sum())
    if not losses:
        return p.sum() * 0.0
    return torch.stack(losses).sum() / len(losses)


def reference(rows, labels, ce_ignore=255, lov_ignore=0, classes="present", dtype=torch.float64, kind="logits"):
    """rows are widened as given (16-bit rows: the values the kernels read).  kind="probas": rows are probabilities, no CE."""
    x = rows.detach().cpu().to(dtype).clone().requires_grad_(True)
    labels = labels.detach().cpu()
    if kind == "logits":
        keep = (labels != ce_ignore) & (labels >= 0) & (labels < x.shape[1])
        logp = torch.log_softmax(x, 1)
        safe = labels.clamp(0, x.shape[1] - 1)
        ce = -(logp.gather(1, safe[:, None])[:, 0] * keep.to(dtype)).sum() / keep.sum().to(dtype)
        lov = lovasz_flat(torch.softmax(x, 1), labels, classes, lov_ignore)
    else:
        ce = x.sum() * 0.0
        lov = lovasz_flat(x, labels, classes, lov_ignore)
    total = ce + lov
    total.backward()
    return {"total": total.detach(), "ce": ce.detach(), "lovasz": lov.detach(), "grad": x.grad}


def ambiguous_rows(rows, labels, lov_ignore=0, delta=2e-6, kind="logits"):
    """bool [n]: rows holding a (row, class) entry whose float64 error lies within `delta` of an entry of the OTHER flag in the same
    class, chains included (entries linked by gaps <= delta form one group; a group holding both flags is ambiguous as a whole).
    Computed from the float64 reference's errors alone."""
    x = rows.detach().cpu().double()
    labels = labels.detach().cpu()
    p = torch.softmax(x, 1) if kind == "logits" else x
    n, C = p.shape
    valid = torch.ones(n, dtype=torch.bool) if lov_ignore is None else labels != lov_ignore
    rows_v = torch.nonzero(valid)[:, 0].numpy()
    mask = np.zeros(n, bool)
    if len(rows_v) == 0:
        return torch.from_numpy(mask)
    pv, lv = p[valid].numpy(), labels[valid].numpy()
    for c in range(C):
        fg = lv == c
        err = np.abs(fg.astype(np.float64) - pv[:, c])
        order = np.argsort(-err, kind="stable")
        es, fs = err[order], fg[order]
        brk = np.concatenate([[True], (es[:-1] - es[1:]) > delta])          # a new group starts here
        gid = np.cumsum(brk) - 1
        ng = gid[-1] + 1
        nfg = np.bincount(gid, weights=fs, minlength=ng)
        cnt = np.bincount(gid, minlength=ng)
        mixed = (nfg > 0) & (nfg < cnt)
        mask[rows_v[order[mixed[gid]]]] = True
    return torch.from_numpy(mask)


_CACHE = {}


def yardstick(key, rows, labels, **kw):
    """(r64, o32, mask), computed once per `key` and shared; callers leave it unchanged.  o32 = {"total", "ce", "lovasz", "grad"}."""
    if key not in _CACHE:
        r64 = reference(rows, labels, dtype=torch.float64, **kw)
        r32 = reference(rows, labels, dtype=torch.float32, **kw)
        mask = ambiguous_rows(rows, labels, kw.get("lov_ignore", 0), kind=kw.get("kind", "logits"))
        keep = ~mask
        o32 = {k: abs(float(r32[k]) - float(r64[k])) / max(abs(float(r64[k])), 1e-30) for k in ("total", "ce", "lovasz")}
        o32["grad"] = rel_err(r32["grad"][keep].numpy(), r64["grad"][keep].numpy()) if keep.any() else 0.0
        _CACHE[key] = (r64, o32, mask)
    return _CACHE[key]
