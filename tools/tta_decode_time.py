"""tools/tta_decode_time.py -- the test-time-augmentation decode and the fusion of passes on the device against their compositions.

    python tools/tta_decode_time.py [--reps 20] [--out FILE.json]

At the nuScenes shape (one frame x 4 views, six tasks of 1, 2, 2, 1, 2, 2 classes, 180 x 180, vel on) it times
  decode   CenterHeadTTADecoder.decode over the six tasks (link_center_decode_flip4: two launches per task) against the
           torch-on-device composition of center_head.py:320-421 and the masks of :461-467 (tests/tta_oracle.py::decode run on GPU
           tensors: the permutes, the in-place flips, sigmoid / exp, the means, atan2, the concatenation);
  fusion   fuse_detections for 3 passes x 500 boxes x 10 classes (one class-wise mask, one scan) against a per-class loop over the
           existing rotate_nms_pcdet followed by the sort that keeps the best 500 (nms_better2.py:266-297), and the padded form.
Device times: 7 windows of `reps` calls each after 10 warm-up calls, [min, median, max] per call in ms.  Also reported: the aten
operators each side dispatches per call (an upper bound of its launches; the library calls are counted by hand) and the read-backs
of each side (Tensor.item / tolist / cpu / numpy; the synchronisation inside a boolean selection, which the per-class loop has once
per class, is not counted).  Not imported by bench.py or any test.  No GPU: fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import tta_oracle as TO  # noqa: E402

import link_amd as la  # noqa: E402

CFG = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 83,
                                                                                      "nms_iou_threshold": 0.2},
       "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075], "double_flip": True}
TASKS = [1, 2, 2, 1, 2, 2]
THR10 = [0.1, 0.1, 0.1, 0.25, 0.1, 0.1, 0.1, 0.15, 0.1, 0.05]


def device_ms(fn, reps, windows=7):
    """per call: [min, median, max] over `windows` timed windows of `reps` calls each, after 10 warm-up calls"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / reps)
    per.sort()
    return [per[0], per[len(per) // 2], per[-1]]


class Ops(TorchDispatchMode):
    """counts the aten operators dispatched (views included: an upper bound of the launches)"""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


class ReadBacks:
    """counts the calls that bring a device tensor's values to the host"""

    def __enter__(self):
        self.n = 0
        self._saved = {k: getattr(torch.Tensor, k) for k in ("item", "tolist", "cpu", "numpy")}
        for k, f in self._saved.items():
            def wrap(t, *a, _f=f, **kw):
                self.n += 1 if t.is_cuda else 0
                return _f(t, *a, **kw)
            setattr(torch.Tensor, k, wrap)
        return self

    def __exit__(self, *exc):
        for k, f in self._saved.items():
            setattr(torch.Tensor, k, f)


def counted(fn):
    with Ops() as ops:
        fn()
    with ReadBacks() as rb:
        fn()
    return {"aten_ops": ops.n, "read_backs": rb.n}


def per_class_loop(passes, thr, max_dets=500):
    """nms_better2.py:266-297 with the existing pieces: a boolean selection and one rotate_nms_pcdet per class, then the sort"""
    boxes = torch.cat([p["box3d_lidar"] for p in passes])
    scores = torch.cat([p["scores"] for p in passes])
    labels = torch.cat([p["label_preds"] for p in passes])
    kb, ks, kl = [], [], []
    for c in range(len(thr)):
        m = labels == c
        b, s = boxes[m], scores[m]
        sel = la.rotate_nms_pcdet(b[:, [0, 1, 2, 3, 4, 5, -1]], s, thr[c])
        kb.append(b[sel]); ks.append(s[sel]); kl.append(labels[m][sel])
    kb, ks, kl = torch.cat(kb), torch.cat(ks), torch.cat(kl)
    order = ks.sort(descending=True)[1][:max_dets]
    return kb[order], ks[order], kl[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_decode_time: no GPU visible; a CPU run gives no time")
    gen = torch.Generator().manual_seed(5)
    H = W = 180
    preds = []
    for k in TASKS:
        pd = {"reg": torch.rand(4, 2, H, W, generator=gen), "height": torch.randn(4, 1, H, W, generator=gen) * 2 - 1,
              "dim": torch.randn(4, 3, H, W, generator=gen) * 0.5, "rot": torch.randn(4, 2, H, W, generator=gen),
              "hm": torch.randn(4, k, H, W, generator=gen) * 1.5 - 3.0, "vel": torch.randn(4, 2, H, W, generator=gen)}
        preds.append({n: t.cuda() for n, t in pd.items()})
    dec = la.CenterHeadTTADecoder(CFG, TASKS)

    def fused():
        return [dec.decode(pd) for pd in preds]

    def composed():
        return [TO.decode(pd, CFG) for pd in preds]
    differ = 0                                   # random maps are not drawn away from the decisions: a cell or two may sit on one
    for (fb, fl, fs, _), (cb, cl, cs, cm, _) in zip(fused(), composed()):
        both = (fs > float("-inf")) & cm
        differ += int(((fs > float("-inf")) != cm).sum()) + int((fl.long()[both] != cl[both]).sum())
        assert torch.allclose(fb[..., :-1], cb[..., :-1], rtol=1e-4, atol=1e-4), "the fused decode disagrees with the composition"
    assert differ <= 6, differ
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "shape": {"views": 4, "tasks": TASKS, "H": H, "W": W, "vel": True},
           "decode": {"cells_that_decide_differently": differ, "fused_ms": device_ms(fused, args.reps),
                      "composed_ms": device_ms(composed, args.reps),
                      "fused": dict(counted(fused), library_launches=2 * len(TASKS)), "composed": counted(composed)}}
    print(json.dumps(out["decode"]))

    import make_golden_boxnms as MB
    rng = np.random.default_rng(9)
    n, npass = 1500, 3
    boxes7 = MB.sample_boxes(n, rng, MB.extent_for(n, rng, 4.0 / n, 7.0 / n), specials=False)
    boxes = np.concatenate([boxes7[:, :6], rng.normal(0, 1, (n, 2)).astype(np.float32), boxes7[:, 6:]], 1)
    scores = (rng.permutation(n).astype(np.float32) + 1) / np.float32(n + 1)
    labels = rng.integers(0, 10, n)
    passes = [{"box3d_lidar": torch.from_numpy(boxes[i::npass]).cuda(), "scores": torch.from_numpy(scores[i::npass]).cuda(),
               "label_preds": torch.from_numpy(labels[i::npass]).cuda()} for i in range(npass)]
    cat = {k: torch.cat([p[k] for p in passes]) for k in passes[0]}

    def fuse():
        return la.fuse_detections(passes, THR10)

    def fuse_padded():
        return la.fuse_detections_padded(cat["box3d_lidar"], cat["scores"], cat["label_preds"], THR10)

    def loop():
        return per_class_loop(passes, THR10)
    a, b = fuse(), loop()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "fuse_detections disagrees with the per-class loop"
    out["fusion"] = {"boxes": n, "passes": npass, "classes": 10, "kept": int(a[1].shape[0]),
                     "fuse_ms": device_ms(fuse, args.reps), "fuse_padded_ms": device_ms(fuse_padded, args.reps),
                     "per_class_loop_ms": device_ms(loop, args.reps),
                     "fuse": dict(counted(fuse), library_launches=2), "fuse_padded": dict(counted(fuse_padded), library_launches=2),
                     "per_class_loop": dict(counted(loop), library_launches=2 * 10)}
    print(json.dumps(out["fusion"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
