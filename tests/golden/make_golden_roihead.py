"""Record tests/golden/roihead_*.npz from the reference's own second stage.  Run by hand; the tests do not run it.

    python tests/golden/make_golden_roihead.py /path/to/LinK

The expected values come from the reference's modules loaded BY PATH (bare parent packages and empty registries are registered in
sys.modules first): det3d/core/utils/center_utils.py (bilinear_interpolate_torch), det3d/core/bbox/box_torch_ops.py,
det3d/models/second_stage/bird_eye_view.py (BEVFeatureExtractor), det3d/models/detectors/two_stage.py (get_box_center,
post_process), det3d/models/roi_heads/roi_head.py, roi_head_template.py and target_assigner/proposal_target_layer.py.  The only
stand-in is det3d.ops.iou3d_nms.iou3d_nms_utils.boxes_iou3d_gpu, whose CUDA extension cannot be built where these fixtures are
recorded: its BEV overlap is the reference's own iou3d_cpu.cpp::box_overlap, compiled in place behind a binding written to a temporary
directory (as make_golden_boxnms.py does), else tests/box_oracle.py's float32 restatement; every fixture's meta says which.  The
sampler's draws are recorded by wrapping subsample_rois.  Nothing of the reference is copied into the repository.

Stable inputs only (the rule of make_golden_boxnms.py).  An ROI is unstable when its float64 maximal overlap lies within 1e-3 of one of
the four thresholds, when its best two overlaps with different ground-truth boxes differ by less than 1e-4, when the reference's
float32 overlap is more than 1e-4 from the float64 one, or when its canonical heading lies within 1e-4 of +-pi / 2 or of the fold's
boundaries; a box of the feature sets is unstable when one of its sample points lies within 1e-4 of an integer cell coordinate.  An
unstable ROI is replaced by an isolated far-away box; at most 2 % of a set may be replaced.  Every float output's meta entry e_<name>
is the distance of the reference's float32 recording from the float64 oracle (tests/roi_oracle.py).
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import box_oracle as BO  # noqa: E402
import roi_oracle as RO  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def compile_overlap(ref_root):
    try:
        from torch.utils.cpp_extension import load
        src = os.path.join(ref_root, "detection", "det3d", "ops", "iou3d_nms", "src")
        tmp = tempfile.mkdtemp(prefix="roihead_ref_")
        for h in ("cuda.h", "cuda_runtime_api.h"):
            open(os.path.join(tmp, h), "w").close()
        with open(os.path.join(tmp, "bind.cpp"), "w") as f:
            f.write('#include <torch/extension.h>\n#include "iou3d_cpu.cpp"\n'
                    'void overlaps(at::Tensor a, at::Tensor b, at::Tensor out) {\n'
                    '  const float *pa = a.data_ptr<float>(), *pb = b.data_ptr<float>(); float *po = out.data_ptr<float>();\n'
                    '  const int64_t n = a.size(0), m = b.size(0);\n'
                    '  for (int64_t i = 0; i < n; i++) for (int64_t j = 0; j < m; j++) po[i * m + j] = box_overlap(pa + i * 7, pb + j * 7);\n}\n'
                    'PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("overlaps", &overlaps); }\n')
        mod = load(name="roihead_ref_cpu", sources=[os.path.join(tmp, "bind.cpp")], extra_include_paths=[tmp, src],
                   extra_cflags=["-O2", "-D__device__=", "-ffp-contract=off", "-w"], build_directory=tmp, verbose=False)

        def overlap(a, b):
            out = torch.zeros(a.shape[0], b.shape[0])
            if a.shape[0] and b.shape[0]:
                mod.overlaps(a.float().contiguous(), b.float().contiguous(), out)
            return out
        return overlap, "iou3d_cpu.cpp::box_overlap compiled from the reference checkout"
    except Exception as e:                                  # noqa: BLE001
        print("reference routine did not compile:", repr(e)[:300])

        def overlap(a, b):
            return torch.from_numpy(BO.pairs_matrix(BO.box_overlap, a.numpy(), b.numpy()).astype(np.float32).reshape(a.shape[0], b.shape[0]))
        return overlap, "float32 restatement (the reference file did not compile)"


def load_reference(root, overlap):
    det = os.path.join(root, "detection")
    for name in ("det3d", "det3d.core", "det3d.core.utils", "det3d.core.bbox", "det3d.models", "det3d.models.detectors", "det3d.models.second_stage",
                 "det3d.models.roi_heads", "det3d.models.roi_heads.target_assigner", "det3d.ops", "det3d.ops.iou3d_nms"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(det, *name.split("."))]
        sys.modules[name] = m
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.modules["numba"] = nb

    class Registry:
        def register_module(self, cls):
            return cls
    reg = types.ModuleType("det3d.models.registry")
    reg.DETECTORS = reg.SECOND_STAGE = reg.ROI_HEAD = Registry()
    sys.modules["det3d.models.registry"] = reg
    base = types.ModuleType("det3d.models.detectors.base")
    base.BaseDetector = torch.nn.Module
    sys.modules["det3d.models.detectors.base"] = base
    sys.modules["det3d.models.builder"] = sys.modules["det3d.models"].builder = types.ModuleType("det3d.models.builder")

    def by_path(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(det, *parts))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    by_path("det3d.core.utils.center_utils", "det3d", "core", "utils", "center_utils.py")
    bto = by_path("det3d.core.bbox.box_torch_ops", "det3d", "core", "bbox", "box_torch_ops.py")
    sys.modules["det3d.core"].box_torch_ops = sys.modules["det3d.core.bbox"].box_torch_ops = bto
    utils = types.ModuleType("det3d.ops.iou3d_nms.iou3d_nms_utils")

    def boxes_iou3d_gpu(boxes_a, boxes_b):                  # iou3d_nms_utils.py:35-72 with the compiled CPU overlap for the CUDA one
        assert boxes_a.shape[1] == boxes_b.shape[1] == 7
        to = lambda b: torch.cat([b[:, :3], b[:, 4:5], b[:, 3:4], b[:, 5:6], -b[:, 6:7] - np.pi / 2], 1)      # noqa: E731
        a, b = to(boxes_a), to(boxes_b)
        amax, amin = (a[:, 2] + a[:, 5] / 2).view(-1, 1), (a[:, 2] - a[:, 5] / 2).view(-1, 1)
        bmax, bmin = (b[:, 2] + b[:, 5] / 2).view(1, -1), (b[:, 2] - b[:, 5] / 2).view(1, -1)
        oh = torch.clamp(torch.min(amax, bmax) - torch.max(amin, bmin), min=0)
        o3 = overlap(a, b) * oh
        va, vb = (a[:, 3] * a[:, 4] * a[:, 5]).view(-1, 1), (b[:, 3] * b[:, 4] * b[:, 5]).view(1, -1)
        return o3 / torch.clamp(va + vb - o3, min=1e-6)
    utils.boxes_iou3d_gpu = boxes_iou3d_gpu
    sys.modules["det3d.ops.iou3d_nms.iou3d_nms_utils"] = utils
    bev = by_path("det3d.models.second_stage.bird_eye_view", "det3d", "models", "second_stage", "bird_eye_view.py")
    by_path("det3d.models.roi_heads.target_assigner.proposal_target_layer", "det3d", "models", "roi_heads", "target_assigner",
            "proposal_target_layer.py")
    by_path("det3d.models.roi_heads.roi_head_template", "det3d", "models", "roi_heads", "roi_head_template.py")
    head = by_path("det3d.models.roi_heads.roi_head", "det3d", "models", "roi_heads", "roi_head.py")
    two = by_path("det3d.models.detectors.two_stage", "det3d", "models", "detectors", "two_stage.py")
    return bev, head, two


def far_box(k, code):
    b = np.zeros(code, np.float32)
    b[:7] = [900.0 + 40.0 * k, 900.0, 0.0, 2.0, 1.0, 1.5, 0.3]
    return b


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0.0))


# ---- features ----------------------------------------------------------------------------------------------------------------------
GEOM = {"pc_start": [-3.5, -2.5], "voxel_size": [0.25, 0.25], "out_stride": 4}       # a 7 x 5 map covers [-3.5, 3.5] x [-2.5, 2.5]


def record_features(bev_mod, two, source):
    rng = np.random.default_rng(411)
    B, C, H, W, R = 2, 6, 5, 7, 40
    bev = rng.standard_normal((B, C, H, W)).astype(np.float32)
    boxes = np.zeros((B, R, 9), np.float32)
    boxes[..., 0] = rng.uniform(-5.5, 5.5, (B, R))           # off the map on both sides
    boxes[..., 1] = rng.uniform(-4.5, 4.5, (B, R))
    boxes[..., 2] = rng.uniform(-1, 1, (B, R))
    boxes[..., 3:6] = rng.uniform(0.3, 3.0, (B, R, 3))
    boxes[..., 6:8] = rng.standard_normal((B, R, 2))
    boxes[..., 8] = rng.uniform(-2 * np.pi, 2 * np.pi, (B, R))
    boxes[0, 0, 8], boxes[0, 1, 8] = np.pi, -np.pi
    replaced = 0
    for b in range(B):
        for i in range(R):
            for _ in range(50):
                pts = RO.box_points(boxes[b, i:i + 1], 5, np.float64)
                x, y = RO.map_coords(pts, GEOM["pc_start"], GEOM["voxel_size"], GEOM["out_stride"], np.float64)
                if min(np.abs(x - np.round(x)).min(), np.abs(y - np.round(y)).min()) >= 1e-4:
                    break
                boxes[b, i, :2] += np.float32(0.0137)
                replaced += 1
    out = {"bev": bev, "boxes": boxes}
    meta = {"source": source, "replaced": replaced, "rois": B * R, **GEOM}
    ext = bev_mod.BEVFeatureExtractor(**GEOM)
    nhwc = torch.from_numpy(bev).permute(0, 2, 3, 1).contiguous()
    for P in (1, 5):
        det = types.SimpleNamespace(num_point=P)
        centers = two.TwoStageDetector.get_box_center(det, [{"box3d_lidar": torch.from_numpy(boxes[b])} for b in range(B)])
        feats = ext.forward({"bev_feature": nhwc}, centers, P)
        out[f"points{P}"] = np.stack([c.numpy() for c in centers])
        out[f"features{P}"] = np.stack([f.numpy() for f in feats])
        f64 = RO.bev_features(bev, boxes, None, None, P, dtype=np.float64, **GEOM)
        meta[f"e_features{P}"] = dist(out[f"features{P}"], f64)
        if P > 1:
            p64 = np.stack([RO.box_points(boxes[b], P, np.float64).reshape(-1, 2) for b in range(B)])
            meta["e_points5"] = dist(out["points5"][..., :2], p64)
    np.savez_compressed(os.path.join(HERE, "roihead_features.npz"), meta=json.dumps(meta), **out)
    print("features", meta)


# ---- assign -------------------------------------------------------------------------------------------------------------------------
def draw_frame(rng, R, G, G_pad, code, classes, scales=(0.02, 0.1, 0.3, 0.8, 3.0)):
    gt = np.zeros((G_pad, code + 1), np.float32)
    gt[:G, 0:2] = rng.uniform(-40, 40, (G, 2))
    gt[:G, 2] = rng.uniform(-1, 1, G)
    gt[:G, 3:6] = np.exp(rng.uniform(np.log(0.6), np.log(5.0), (G, 3)))
    gt[:G, 6] = rng.uniform(-np.pi, np.pi, G)
    if code == 9:
        gt[:G, 7:9] = rng.standard_normal((G, 2))
    gt[:G, -1] = rng.integers(1, classes + 1, G)
    rois = np.zeros((R, code), np.float32)
    labels = np.zeros(R, np.int64)
    for i in range(R):
        if G == 0:
            rois[i] = far_box(i, code) * 0.01
            labels[i] = 1
            continue
        j = rng.integers(0, G)
        s = scales[i % len(scales)]
        rois[i] = gt[j, :code]
        rois[i, :3] += rng.normal(0, s, 3).astype(np.float32)
        rois[i, 3:6] *= np.exp(rng.normal(0, 0.3 * min(s, 1.0), 3)).astype(np.float32)
        rois[i, 6] += np.float32(rng.normal(0, 0.3 * min(s, 1.0)) + (np.pi if i % 7 == 0 else 0.0))
        labels[i] = int(gt[j, -1]) if i % 11 else classes + 1          # some ROIs of a class the ground truth does not hold
    return rois, labels, gt


def unstable_rois(rois, labels, gt, cfg, iou_ref):
    g = RO.cut_gt(gt, gt.shape[1])
    by_class = cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False)
    mo, ga, iou = RO.max_overlaps(rois, labels, g, by_class, np.float64, return_matrix=True)
    bad = np.zeros(len(rois), bool)
    for k in ("CLS_FG_THRESH", "CLS_BG_THRESH", "CLS_BG_THRESH_LO", "REG_FG_THRESH"):
        bad |= np.abs(mo - cfg[k]) < 1e-3
    m = iou.copy()
    if by_class:
        m[labels[:, None] != g[:, -1].astype(np.int64)[None]] = -1.0
    if m.shape[1] > 1:
        top = np.sort(m, 1)[:, -2:]
        bad |= (top[:, 1] > 0) & (top[:, 1] - top[:, 0] < 1e-4)
    ref = iou_ref(torch.from_numpy(rois[:, :7]), torch.from_numpy(g[:, :7])).numpy().astype(np.float64)
    bad |= np.abs(ref - iou).max(1) > 1e-4
    can = RO.canonical(rois, g[ga], np.float64)
    raw = np.mod(g[ga][:, 6] - RO.limit_period(rois[:, 6].astype(np.float64), np.float64), 2 * np.pi)
    for edge in (0.5 * np.pi, 1.5 * np.pi):
        bad |= np.abs(raw - edge) < 1e-4
    bad |= np.abs(np.abs(can[:, 6]) - np.pi / 2) < 1e-4
    return bad


def record_assign(head, iou_ref, source, name, seed, B, R, G, G_pad, code, cfg, classes=3):
    rng = np.random.default_rng(seed)
    for attempt in range(50):
        frames = [draw_frame(rng, R, G if b == 0 else max(G - 1, 0), G_pad, code, classes) for b in range(B)]
        replaced = 0
        for rois, labels, gt in frames:
            for _ in range(10):
                bad = unstable_rois(rois, labels, gt, cfg, iou_ref)
                if not bad.any():
                    break
                for i in np.nonzero(bad)[0]:
                    rois[i] = far_box(replaced, code)
                    replaced += 1
            else:
                raise RuntimeError("ROIs did not stabilise")
        if replaced <= 0.02 * B * R:
            break
    assert replaced <= 0.02 * B * R, (name, replaced)
    rois = np.stack([f[0] for f in frames]); labels = np.stack([f[1] for f in frames]); gt = np.stack([f[2] for f in frames])
    scores = rng.uniform(0.1, 1.0, (B, R)).astype(np.float32)
    tmpl = head.RoIHead.__mro__[1]
    layer = head.RoIHead.__mro__[1].__init__.__globals__["ProposalTargetLayer"](roi_sampler_cfg=Cfg(cfg))
    drawn, overlaps = [], []
    inner = layer.subsample_rois

    def wrapped(max_overlaps):
        inds = inner(max_overlaps=max_overlaps)
        drawn.append(inds.numpy().astype(np.int32)); overlaps.append(max_overlaps.numpy().copy())
        return inds
    layer.subsample_rois = wrapped
    np.random.seed(seed); torch.manual_seed(seed)
    self = types.SimpleNamespace(proposal_target_layer=layer)
    batch = {"batch_size": B, "rois": torch.from_numpy(rois), "roi_scores": torch.from_numpy(scores), "roi_labels": torch.from_numpy(labels),
             "gt_boxes_and_cls": torch.from_numpy(gt), "roi_features": torch.zeros(B, R, 1)}
    t = tmpl.assign_targets(self, batch)
    out = {"in_rois": rois, "in_roi_labels": labels, "in_roi_scores": scores, "in_gt": gt, "sampled_inds": np.stack(drawn),
           "max_overlaps": np.stack(overlaps)}
    for k in ("rois", "roi_labels", "roi_scores", "gt_iou_of_rois", "gt_of_rois_src", "gt_of_rois", "reg_valid_mask", "rcnn_cls_labels"):
        out[k] = t[k].numpy()
    o64 = RO.assign(rois, labels, scores, gt, cfg, sel_in=out["sampled_inds"], dtype=np.float64)
    lists = [RO.sample_lists(mo, cfg) for mo in out["max_overlaps"]]
    meta = {"source": source, "replaced": replaced, "rois": B * R, "cfg": cfg, "code": code, "seed": seed,
            "lists": [[len(v) for v in l] for l in lists]}
    for k in ("max_overlaps", "gt_iou_of_rois", "gt_of_rois", "rcnn_cls_labels"):
        meta["e_" + k] = dist(out[k], o64[k])
    np.savez_compressed(os.path.join(HERE, name), meta=json.dumps(meta), **out)
    print(name, {k: v for k, v in meta.items() if k != "cfg"})


# ---- loss ---------------------------------------------------------------------------------------------------------------------------
LOSS_W = {"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}


def record_loss(head, name, seed, N, code, soft, extreme, weights):
    rng = np.random.default_rng(seed)
    cls = rng.uniform(-30, 30, N).astype(np.float32) if N > 1 else np.float32([0.7])
    if extreme:
        cls[:4] = [200.0, -200.0, 200.0, -200.0]
    reg = rng.standard_normal((N, code)).astype(np.float32)
    gt = np.concatenate([rng.standard_normal((N, code)), rng.integers(1, 4, (N, 1))], 1).astype(np.float32)
    iou = rng.uniform(0, 1, N).astype(np.float32)
    # 0 / 1 labels only: torch's binary_cross_entropy refuses the -1 of the ignore band, so the masked rows are pinned on the float64
    # oracle alone (tests/test_gpu_roihead.py)
    labels = (iou if soft else np.where(iou > 0.6, 1.0, 0.0)).astype(np.float32)
    if extreme:
        labels[:4] = [1.0, 0.0, 0.0, 1.0] if not soft else [1.0, 0.0, 0.25, 0.5]
    valid = (iou > 0.55).astype(np.int64)
    tmpl = head.RoIHead.__mro__[1]
    self = types.SimpleNamespace(model_cfg=Cfg(LOSS_CONFIG=Cfg(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="L1", LOSS_WEIGHTS=weights)))
    x, r = torch.from_numpy(cls).requires_grad_(True), torch.from_numpy(reg).requires_grad_(True)
    ret = {"rcnn_cls": x.view(N, 1), "rcnn_reg": r, "rcnn_cls_labels": torch.from_numpy(labels), "gt_of_rois": torch.from_numpy(gt).view(1, N, -1),
           "reg_valid_mask": torch.from_numpy(valid)}
    lc, _ = tmpl.get_box_cls_layer_loss(self, ret)
    lr, _ = tmpl.get_box_reg_layer_loss(self, ret)
    (lc + lr).backward()
    out = {"cls": cls, "reg": reg, "labels": labels, "gt_of_rois": gt, "reg_valid_mask": valid, "grad_cls": x.grad.numpy(), "grad_reg": r.grad.numpy(),
           "out": np.float32([float(lc + lr), float(lc), float(lr), float(valid.sum())])}
    o64 = RO.loss(cls, reg, labels, gt, valid, weights["code_weights"], weights["rcnn_cls_weight"], weights["rcnn_reg_weight"], np.float64)
    meta = {"weights": weights, "code": code, "soft": soft, "extreme": extreme, "e_out": dist(out["out"], o64["out"]),
            "e_grad_cls": dist(out["grad_cls"], o64["grad_cls"]), "e_grad_reg": dist(out["grad_reg"], o64["grad_reg"])}
    np.savez_compressed(os.path.join(HERE, name), meta=json.dumps(meta), **out)
    print(name, meta)


# ---- refine -------------------------------------------------------------------------------------------------------------------------
def record_refine(head, two, name, seed, B, R, code):
    rng = np.random.default_rng(seed)
    rois = rng.uniform(-40, 40, (B, R, code)).astype(np.float32)
    rois[..., 3:6] = rng.uniform(0.5, 5, (B, R, 3))
    rois[..., 6] = rng.uniform(-2 * np.pi, 2 * np.pi, (B, R))
    labels = rng.integers(0, 4, (B, R)).astype(np.int64)
    labels[-1] = 0                                           # a frame whose labels are all 0
    scores = rng.uniform(0.05, 1, (B, R)).astype(np.float32)
    cls = rng.uniform(-6, 6, (B * R, 1)).astype(np.float32)
    reg = (rng.standard_normal((B * R, code)) * 0.3).astype(np.float32)
    tmpl = head.RoIHead.__mro__[1]
    cp, bp = tmpl.generate_predicted_boxes(None, B, torch.from_numpy(rois), torch.from_numpy(cls), torch.from_numpy(reg))
    preds = two.TwoStageDetector.post_process(None, {"batch_size": B, "batch_box_preds": bp, "batch_cls_preds": cp, "roi_labels": torch.from_numpy(labels),
                                                     "roi_scores": torch.from_numpy(scores), "metadata": [None] * B})
    out = {"rois": rois, "roi_labels": labels, "roi_scores": scores, "cls": cls, "reg": reg, "batch_box_preds": bp.numpy()}
    b64, s64, l64, c64 = RO.refine(rois, labels, scores, cls, reg, np.float64)
    eb = es = 0.0
    for b, p in enumerate(preds):
        out[f"f{b}_box3d_lidar"], out[f"f{b}_scores"], out[f"f{b}_label_preds"] = (p[k].numpy() for k in ("box3d_lidar", "scores", "label_preds"))
        n = len(p["scores"])
        assert n == c64[b] and np.array_equal(out[f"f{b}_label_preds"], l64[b, :n])
        eb, es = max(eb, dist(out[f"f{b}_box3d_lidar"], b64[b, :n])), max(es, dist(out[f"f{b}_scores"], s64[b, :n]))
    meta = {"code": code, "e_boxes": eb, "e_scores": es, "counts": [int(v) for v in c64]}
    np.savez_compressed(os.path.join(HERE, name), meta=json.dumps(meta), **out)
    print(name, meta)


MODEL_CFG = {"CLASS_AGNOSTIC": True, "SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256], "DP_RATIO": 0.3,
             "TARGET_CONFIG": RO.CFG, "LOSS_CONFIG": {"CLS_LOSS": "BinaryCrossEntropy", "REG_LOSS": "L1", "LOSS_WEIGHTS": LOSS_W}}


def record_keys(head):
    cfg = Cfg({k: (Cfg(v) if isinstance(v, dict) else v) for k, v in MODEL_CFG.items()})
    m = head.RoIHead(input_channels=40, model_cfg=cfg, num_class=1, code_size=7)
    sd = m.state_dict()
    meta = {"model_cfg": MODEL_CFG, "input_channels": 40, "keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()],
            "reg_last_std": float(m.reg_layers[-1].weight.std())}
    np.savez_compressed(os.path.join(HERE, "roihead_keys.npz"), meta=json.dumps(meta))
    print("keys", len(meta["keys"]))


def main(root):
    overlap, source = compile_overlap(root)
    bev_mod, head, two = load_reference(root, overlap)
    iou_ref = sys.modules["det3d.ops.iou3d_nms.iou3d_nms_utils"].boxes_iou3d_gpu
    only = os.environ.get("ROIHEAD_ONLY", "")
    if not only:
        record_features(bev_mod, two, source)
        record_assign(head, iou_ref, source, "roihead_assign_waymo.npz", 500, 1, 500, 40, 48, 7, dict(RO.CFG))
        record_assign(head, iou_ref, source, "roihead_assign_code9.npz", 501, 2, 65, 6, 9, 9,
                      dict(RO.CFG, ROI_PER_IMAGE=8, CLS_SCORE_TYPE="cls", CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.45, FG_RATIO=0.3125))
        record_assign(head, iou_ref, source, "roihead_assign_allclass.npz", 502, 2, 64, 1, 4, 7,
                      dict(RO.CFG, ROI_PER_IMAGE=8, SAMPLE_ROI_BY_EACH_CLASS=False), classes=1)
    record_loss(head, "roihead_loss_1.npz", 600, 1, 7, True, False, LOSS_W)
    record_loss(head, "roihead_loss_8.npz", 601, 8, 7, False, True, LOSS_W)
    record_loss(head, "roihead_loss_512.npz", 602, 512, 9, True, True,
                {"rcnn_cls_weight": 0.7, "rcnn_reg_weight": 1.3, "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.2, 0.2]})
    record_refine(head, two, "roihead_refine_7.npz", 701, 3, 65, 7)
    record_refine(head, two, "roihead_refine_9.npz", 702, 2, 1, 9)
    record_keys(head)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LINK_REFERENCE", ""))
