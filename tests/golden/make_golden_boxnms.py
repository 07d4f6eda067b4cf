"""tests/golden/make_golden_boxnms.py -- records the fixtures of tests/test_cpu_boxnms.py and tests/test_gpu_boxnms.py.  The tests
do not run it.

The expected IoU values come from the reference's own CPU routine (detection/det3d/ops/iou3d_nms/src/iou3d_cpu.cpp::
boxes_iou_bev_cpu), compiled from where the reference checkout lies (argument 1 or $LINK_REFERENCE) with two empty headers standing
in for cuda.h / cuda_runtime_api.h and a three-line binding written to a temporary directory; nothing of the reference is copied
here.  If it does not compile, every fixture's meta says so ("source": "float32 restatement") and tests/box_oracle.py's float32
restatement is the pin.

Stable inputs only: the routine is discontinuous at its strict inequalities and an NMS decision at its threshold.  A pair is unstable
when its float64 result moves by more than 1e-6 with the corner margin varied by +-1e-4 or the crossing test s1 s2 > 0 replaced by
> +-1e-9, when the float32 reference is more than 1e-4 from the float64 result, when its IoU (rotated, rotated after the pcdet
transform among the first PRE boxes, axis-aligned) lies within 1e-3 of THR, or its squared centre distance within 1e-3 of RADIUS.
One box of every unstable pair is replaced by an isolated far-away box; fewer than 2 % of the boxes may be replaced.
The degenerate cases planted in the sets of 400 boxes and more (sample_boxes) are mostly unstable by this very rule: the exact
duplicate, the edge-sharing neighbours and the zero-area box leave again; the same-centre 45 degree pair and the small box inside
a large one stay, in the NMS sets.  tests/test_gpu_boxnms.py::test_degenerate_pairs builds all of them directly instead.
BOXNMS_ONLY_NMS=1000,4097 regenerates only those NMS sets (the committed two large sets were recorded that way, so a full run
draws other boxes for them: the fixtures pin the recorded arrays, not the seed).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import box_oracle as BO  # noqa: E402

THR, PRE, POST, RADIUS = 0.2, 1000, 83, 4.0
PAIR_SHAPES = [(1, 1), (17, 63), (64, 64), (65, 130), (256, 192)]
ONLY_NMS = [int(v) for v in os.environ.get("BOXNMS_ONLY_NMS", "").split(",") if v]         # regenerate some NMS sets only
NMS_SIZES = [0, 1, 64, 65, 1000, 4097]


def compile_reference(ref_root):
    try:
        import torch
        from torch.utils.cpp_extension import load
        src = os.path.join(ref_root, "detection", "det3d", "ops", "iou3d_nms", "src")
        tmp = tempfile.mkdtemp(prefix="boxnms_ref_")
        for h in ("cuda.h", "cuda_runtime_api.h"):
            open(os.path.join(tmp, h), "w").close()
        with open(os.path.join(tmp, "bind.cpp"), "w") as f:
            f.write('#include <torch/extension.h>\n#include "iou3d_cpu.h"\n'
                    'PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("boxes_iou_bev_cpu", &boxes_iou_bev_cpu); }\n')
        mod = load(name="boxnms_ref_cpu", sources=[os.path.join(src, "iou3d_cpu.cpp"), os.path.join(tmp, "bind.cpp")],
                   extra_include_paths=[tmp, src], extra_cflags=["-O2", "-D__device__=", "-ffp-contract=off", "-w"],
                   build_directory=tmp, verbose=False)

        def iou(a, b):
            out = torch.zeros(a.shape[0], b.shape[0])
            if a.shape[0] and b.shape[0]:
                mod.boxes_iou_bev_cpu(torch.from_numpy(np.ascontiguousarray(a, np.float32)),
                                      torch.from_numpy(np.ascontiguousarray(b, np.float32)), out)
            return out.numpy()
        return iou, "iou3d_cpu.cpp::boxes_iou_bev_cpu compiled from the reference checkout"
    except Exception as e:                                  # noqa: BLE001
        print("reference routine did not compile:", repr(e)[:300])
        return (lambda a, b: BO.pairs_matrix(BO.iou_bev, a, b).astype(np.float32)), "float32 restatement (the reference file did not compile)"


def sample_boxes(n, rng, extent, specials=True):
    ncl = max(1, n // 10)
    cl = rng.uniform(-extent, extent, (ncl, 2))
    b = np.zeros((n, 7), np.float32)
    which = rng.integers(0, ncl, n)
    b[:, :2] = cl[which] + rng.normal(0, 1.5, (n, 2))
    b[:, 2] = rng.uniform(-2, 1, n)
    b[:, 3:5] = np.exp(rng.uniform(np.log(0.2), np.log(12.0), (n, 2)))
    b[:, 5] = rng.uniform(0.5, 3, n)
    b[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n)
    if specials and n >= 400:          # the degenerate cases: most of them are unstable by construction and leave again below
        b[1] = b[0]                                                       # exact duplicate
        b[3] = b[2]; b[3, 6] = b[2, 6] + np.float32(np.pi / 4); b[3, 3:5] = b[2, 3:5] = 4.0      # same centre, 45 degrees: an octagon
        b[4, 3:5] = (4.0, 2.0); b[4, 6] = 0
        b[5] = b[4]; b[5, 0] = b[4, 0] + 4.0                              # shares an edge
        b[6, 3] = 0.0                                                     # zero area
        b[7, 3:5] = (12.0, 12.0)
        b[8] = b[7]; b[8, 3:5] = (0.25, 0.2); b[8, 0] += 1.0              # a small box inside a large one
    return b


def far_box(k):
    return np.array([1000.0 + 30.0 * k, 1000.0, 0.0, 2.0, 1.0, 1.5, 0.3], np.float32)


def candidates(a, b):
    """pairs whose circumscribed circles (grown by the margin) meet: every other pair has no point and is exactly 0"""
    ra = 0.5 * np.hypot(a[:, 3], a[:, 4]) + 0.05
    rb = 0.5 * np.hypot(b[:, 3], b[:, 4]) + 0.05
    out = []
    for s in range(0, a.shape[0], 256):
        d = np.hypot(a[s:s + 256, None, 0] - b[None, :, 0], a[s:s + 256, None, 1] - b[None, :, 1])
        i, j = np.nonzero(d <= ra[s:s + 256, None] + rb[None, :])
        out.append(np.stack([i + s, j], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def chunked(fn, a, b, **kw):
    out = [fn(a[s:s + 100000], b[s:s + 100000], **kw) for s in range(0, a.shape[0], 100000)]
    return np.concatenate(out) if out else np.zeros(0)


def unstable_pairs(a, b, ref, same):
    """-> (indices [U, 2] of unstable pairs, d = max |ref - float64| over all pairs)"""
    c = candidates(a, b)
    if same:
        c = c[c[:, 0] != c[:, 1]]
    A, B = a[c[:, 0]], b[c[:, 1]]
    base = chunked(BO.iou_bev, A, B, dtype=np.float64)
    bad = ~np.isfinite(base)
    for kw in ({"margin": BO.MARGIN + 1e-4}, {"margin": BO.MARGIN - 1e-4}, {"cross_eps": 1e-9}, {"cross_eps": -1e-9}):
        v = chunked(BO.iou_bev, A, B, dtype=np.float64, **kw)
        bad |= ~(np.abs(v - base) <= 1e-6)
    r = ref[c[:, 0], c[:, 1]].astype(np.float64)
    err = np.abs(r - base)
    bad |= ~(err <= 1e-4)
    bad |= np.abs(r - THR) < 1e-3
    full = ref.astype(np.float64).copy()
    full[c[:, 0], c[:, 1]] = 0
    if same:
        np.fill_diagonal(full, 0)
    stray = np.argwhere(full != 0)                           # outside the candidate set the reference must be exactly 0
    d = float(err[~bad].max()) if (~bad).any() else 0.0
    return np.concatenate([c[bad], stray]), d


def stabilise_pairs(a, b, iou_ref):
    replaced = 0
    for _ in range(20):
        ref = iou_ref(a, b)
        u, d = unstable_pairs(a, b, ref, same=False)
        if not len(u):
            return b, ref, d, replaced
        for j in np.unique(u[:, 1]):
            b[j] = far_box(replaced)
            replaced += 1
    raise RuntimeError("pairs did not stabilise")


def nms_unstable(boxes, order, iou_ref):
    """unstable boxes (indices into `boxes`) of every decision the NMS fixtures take; -> (set, rotated ref IoU of the sorted boxes)"""
    s = boxes[order]
    ref = iou_ref(s, s)
    u, _ = unstable_pairs(s, s, ref, same=True)
    bad = set(order[u[:, 1]].tolist())
    p = BO.to_pcdet(s[:PRE])
    refp = iou_ref(p, p)
    up, _ = unstable_pairs(p, p, refp, same=True)
    bad |= set(order[up[:, 1]].tolist())
    c = candidates(s, s)
    c = c[c[:, 0] < c[:, 1]]
    nrm = BO.iou_normal(s[c[:, 0]], s[c[:, 1]])
    bad |= set(order[c[np.abs(nrm.astype(np.float64) - THR) < 1e-3, 1]].tolist())
    n = s.shape[0]
    for st in range(0, n, 512):
        d2 = (s[st:st + 512, None, 0].astype(np.float64) - s[None, :, 0]) ** 2 + (s[st:st + 512, None, 1].astype(np.float64) - s[None, :, 1]) ** 2
        i, j = np.nonzero(np.abs(d2 - RADIUS) < 1e-3)
        bad |= set(order[j[(i + st) != j]].tolist())
    return bad, ref, refp


def extent_for(n, rng, lo=0.07, hi=0.12):
    """cluster spread at which a fraction lo..hi of the pairs overlap (measured on a sample of pairs with the float32 restatement)"""
    ext = 2.0
    for _ in range(30):
        b = sample_boxes(n, np.random.default_rng(1), ext, specials=False)
        i, j = rng.integers(0, n, 20000), rng.integers(0, n, 20000)
        frac = float((BO.iou_bev(b[i], b[j])[i != j] > 0).mean())
        if frac > hi:
            ext *= 1.3
        elif frac < lo:
            ext /= 1.15
        else:
            break
    return ext


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LINK_REFERENCE", "")
    iou_ref, source = compile_reference(ref_root)
    rng = np.random.default_rng(20261017)
    for na, nb in ([] if ONLY_NMS else PAIR_SHAPES):
        ext = extent_for(na + nb, rng) if na + nb > 8 else 1.0
        for attempt in range(100):                           # small sets: redraw until fewer than 2 % of the boxes had to leave
            allb = sample_boxes(na + nb, rng, ext)
            perm = rng.permutation(na + nb) if na + nb > 2 else np.arange(na + nb)
            a, b = allb[perm[:na]].copy(), allb[perm[na:]].copy()
            if na == 1:
                b[0] = a[0]; b[0, 0] += 0.7; b[0, 6] += 0.4
            b, ref, d, replaced = stabilise_pairs(a, b, iou_ref)
            if replaced < 0.02 * (na + nb) or replaced == 0:
                break
        assert replaced < 0.02 * (na + nb) or replaced == 0, (na, nb, replaced)
        ov32 = BO.pairs_matrix(BO.box_overlap, a, b).astype(np.float32)
        meta = {"source": source, "overlap_source": "float32 restatement (the reference has no CPU overlap entry)", "d": d,
                "replaced": replaced, "overlap_fraction": float((ref > 0).mean()), "thr": THR}
        np.savez_compressed(os.path.join(HERE, f"boxnms_pairs_{na}x{nb}.npz"), a=a, b=b, iou=ref.astype(np.float32), overlap=ov32,
                            meta=json.dumps(meta))
        print("pairs", na, nb, meta)
    for n in (ONLY_NMS or NMS_SIZES):
        # 5-15 % of the pairs overlap in the sets up to 65 boxes.  The large sets cannot have that AND fewer than 2 % unstable boxes: a
        # box with hundreds of overlapping partners almost surely has one within 1e-3 of a threshold.  They get about five partners
        # per box (the density of a detector's candidates), which is what meta["overlap_fraction"] records.
        ext = (extent_for(n, rng) if n < 400 else extent_for(n, rng, 4.0 / n, 7.0 / n)) if n > 8 else 1.0
        for attempt in range(100):
            boxes = sample_boxes(n, rng, ext)
            scores = (rng.permutation(n).astype(np.float32) + 1) / np.float32(n + 1)         # distinct
            order = np.argsort(-scores, kind="stable")
            replaced = 0
            for _ in range(30):
                bad, ref, refp = nms_unstable(boxes, order, iou_ref)
                if not bad:
                    break
                for j in sorted(bad):
                    boxes[j] = far_box(replaced)
                    replaced += 1
            else:
                raise RuntimeError("box set did not stabilise")
            if replaced < 0.02 * n or replaced == 0:
                break
        assert replaced < 0.02 * n or replaced == 0, (n, replaced)
        s = boxes[order]
        keep_rot = order[BO.greedy_nms(ref > np.float32(THR))]
        keep_pre = order[BO.greedy_nms(ref[:PRE, :PRE] > np.float32(THR))]
        nrm = BO.pairs_matrix(BO.iou_normal, s, s)
        keep_nrm = order[BO.greedy_nms(nrm > np.float32(THR))]
        keep_pcdet = order[BO.greedy_nms(refp > np.float32(THR))][:POST]
        dets = np.concatenate([boxes[:, :2], scores[:, None]], 1).astype(np.float32)
        keep_circle = BO.circle_nms(dets, RADIUS)[:POST]
        meta = {"source": source, "replaced": replaced, "overlap_fraction": float((ref > 0).mean()) if n else 0.0, "thr": THR, "pre": PRE,
                "post": POST, "radius": RADIUS}
        np.savez_compressed(os.path.join(HERE, f"boxnms_nms_{n}.npz"), boxes=boxes, scores=scores, keep_rotate=keep_rot,
                            keep_rotate_pre=keep_pre, keep_normal=keep_nrm, keep_pcdet=keep_pcdet, keep_circle=keep_circle,
                            meta=json.dumps(meta))
        print("nms", n, meta, len(keep_rot), len(keep_nrm), len(keep_pcdet), len(keep_circle), flush=True)


if __name__ == "__main__":
    main()
