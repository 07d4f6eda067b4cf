"""tests/tta_oracle.py -- checkers of the CenterHead test-time augmentation (csrc/dettta.hip, section N of include/link_amd.h), on
the CPU in numpy / torch, in float32 (the reference's arithmetic) or float64 (the arbiter).  Test infrastructure only.

views restates detection/det3d/datasets/pipelines/test_aug.py:12-32 after preprocess.py:153-156 over core/bbox/box_np_ops.py:
182-204; decode restates models/bbox_heads/center_head.py:314-421 and the masks of :461-467 statement by statement in torch (the
in-place writes on views of the maps included); rotate_back restates :489-503; classwise_nms restates detection/nms_better2.py:
266-297 over the reference IoU of tests/box_oracle.py.  The float64 forms take the same fp32 inputs -- the maps, the points, and
the fp32 entries of the rotation matrix -- and evaluate the same formulas in double.
"""
import numpy as np
import torch

import box_oracle as BO


def rot_mat_T(angle, dtype):
    """box_np_ops.py:184-195 with axis=2: built in the points' dtype (float32) -- float64 takes those fp32 entries"""
    s, c = np.sin(angle), np.cos(angle)
    m = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    return m.astype(dtype)


def rotate_points(xyz, angle, dtype=np.float32):
    """rotation_points_single_angle(points, angle, axis=2) = points @ rot_mat_T.  The float64 form, and the float32 form used
    where numpy's matmul is not wanted, spell the product out: x c + y s, -x s + y c, z."""
    m = rot_mat_T(angle, dtype)
    p = np.asarray(xyz).astype(dtype)
    return np.stack([p[:, 0] * m[0, 0] + p[:, 1] * m[1, 0], p[:, 0] * m[0, 1] + p[:, 1] * m[1, 1], p[:, 2]], 1)


def views(clouds, angle=0.0, dtype=np.float32):
    """list of B [N_i, C] float32 clouds -> the list of 4 B clouds, frame-major, view-minor"""
    out = []
    for pts in clouds:
        p = np.asarray(pts, np.float32).astype(dtype).copy()
        if angle != 0:                                           # preprocess.py:153-156
            p[:, :3] = rotate_points(p[:, :3], angle, dtype)
        y = p.copy(); y[:, 1] = -y[:, 1]                         # test_aug.py:14-15
        x = p.copy(); x[:, 0] = -x[:, 0]                         # :20-21
        d = p.copy(); d[:, 0] = -d[:, 0]; d[:, 1] = -d[:, 1]     # :26-28
        out += [p, y, x, d]
    return out


def decode(pd, cfg, dtype=torch.float32):
    """One task's NCHW maps of batch 4 B (fp32 tensors on the CPU) -> boxes [B, H W, 7 | 9], labels [B, H W], scores [B, H W],
    mask [B, H W], hm [B, H W, K] in `dtype`: center_head.py:314-421 with double_flip, and the masks of :461-467"""
    # :314-316 (on a copy: permute().contiguous() of a one-channel map is the map itself, and what follows writes in place)
    pd = {k: v.to(dtype).clone().permute(0, 2, 3, 1).contiguous() for k, v in pd.items()}
    batch_size = pd["hm"].shape[0]
    assert batch_size % 4 == 0, batch_size
    batch_size = batch_size // 4
    for k in pd:                                                                              # :331-335
        _, H, W, C = pd[k].shape
        pd[k] = pd[k].reshape(batch_size, 4, H, W, C)
        pd[k][:, 1] = torch.flip(pd[k][:, 1], dims=[1])
        pd[k][:, 2] = torch.flip(pd[k][:, 2], dims=[2])
        pd[k][:, 3] = torch.flip(pd[k][:, 3], dims=[1, 2])
    batch_hm = torch.sigmoid(pd["hm"])
    batch_dim = torch.exp(pd["dim"])
    batch_rots, batch_rotc = pd["rot"][..., 0:1], pd["rot"][..., 1:2]
    batch_reg, batch_hei = pd["reg"], pd["height"]
    batch_hm, batch_hei, batch_dim = batch_hm.mean(dim=1), batch_hei.mean(dim=1), batch_dim.mean(dim=1)
    batch_reg[:, 1, ..., 1] = 1 - batch_reg[:, 1, ..., 1]                                     # :359-364
    batch_reg[:, 2, ..., 0] = 1 - batch_reg[:, 2, ..., 0]
    batch_reg[:, 3, ..., 0] = 1 - batch_reg[:, 3, ..., 0]
    batch_reg[:, 3, ..., 1] = 1 - batch_reg[:, 3, ..., 1]
    batch_reg = batch_reg.mean(dim=1)
    batch_rotc[:, 1] *= -1                                                                    # :370-382
    batch_rots[:, 2] *= -1
    batch_rots[:, 3] *= -1
    batch_rotc[:, 3] *= -1
    batch_rotc, batch_rots = batch_rotc.mean(dim=1), batch_rots.mean(dim=1)
    batch_rot = torch.atan2(batch_rots, batch_rotc)
    batch, H, W, K = batch_hm.size()
    batch_reg, batch_hei = batch_reg.reshape(batch, H * W, 2), batch_hei.reshape(batch, H * W, 1)
    batch_rot, batch_dim, batch_hm = batch_rot.reshape(batch, H * W, 1), batch_dim.reshape(batch, H * W, 3), batch_hm.reshape(batch, H * W, K)
    ys, xs = torch.meshgrid([torch.arange(0, H), torch.arange(0, W)], indexing="ij")
    ys = ys.view(1, H, W).repeat(batch, 1, 1).to(batch_hm)
    xs = xs.view(1, H, W).repeat(batch, 1, 1).to(batch_hm)
    xs = xs.view(batch, -1, 1) + batch_reg[:, :, 0:1]
    ys = ys.view(batch, -1, 1) + batch_reg[:, :, 1:2]
    xs = xs * cfg["out_size_factor"] * cfg["voxel_size"][0] + cfg["pc_range"][0]
    ys = ys * cfg["out_size_factor"] * cfg["voxel_size"][1] + cfg["pc_range"][1]
    parts = [xs, ys, batch_hei, batch_dim]
    if "vel" in pd:                                                                           # :405-418
        batch_vel = pd["vel"]
        batch_vel[:, 1, ..., 1] *= -1
        batch_vel[:, 2, ..., 0] *= -1
        batch_vel[:, 3] *= -1
        parts.append(batch_vel.mean(dim=1).reshape(batch, H * W, 2))
    boxes = torch.cat(parts + [batch_rot], dim=2)
    scores, labels = torch.max(batch_hm, dim=-1)                                              # :461-467
    r = torch.tensor(cfg["post_center_limit_range"], dtype=batch_hm.dtype, device=batch_hm.device)
    mask = (scores > cfg["score_threshold"]) & (boxes[..., :3] >= r[:3]).all(-1) & (boxes[..., :3] <= r[3:]).all(-1)
    return boxes, labels, scores, mask, batch_hm


def rotate_back(boxes, tt_rotation, dtype=np.float32):
    """center_head.py:489-503 on [m, 7 | 9] rows (fp32 in) -> [m, C] in `dtype`"""
    b = np.asarray(boxes, np.float32).astype(dtype).copy()
    rev = -tt_rotation
    b[:, :3] = rotate_points(b[:, :3], rev, dtype)
    if b.shape[1] > 7:
        b[:, 6:8] = rotate_points(np.hstack([b[:, 6:8], np.zeros((b.shape[0], 1), dtype)]), rev, dtype)[:, :2]
    b[:, -1] += np.float32(rev).astype(dtype)                    # a float32 array += a Python float adds the fp32 value
    return b


def nms_pcdet(boxes, scores, thr, pre=None, post=None):
    """box_torch_ops.py:248-277 on numpy rows [n, 7 | 9] (det3d lidar format) -> kept indices, best first"""
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores)
    order = np.argsort(-scores, kind="stable")
    if pre is not None:
        order = order[:pre]
    if not len(order):
        return order.astype(np.int64)
    p = BO.to_pcdet(boxes[order][:, [0, 1, 2, 3, 4, 5, -1]])
    sup = suppression(p, np.float32(thr))
    return order[BO.greedy_nms(sup, post)]


def suppression(p, thr):
    """IoU > thr over the pairs whose circumscribed circles meet (every other pair has no point and IoU 0)"""
    n = len(p)
    r = 0.5 * np.hypot(p[:, 3], p[:, 4]) + 0.05
    near = np.argwhere(np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) <= r[:, None] + r[None, :])
    sup = np.zeros((n, n), bool)
    if len(near):
        sup[near[:, 0], near[:, 1]] = BO.iou_bev(p[near[:, 0]], p[near[:, 1]]) > thr
    return sup


def classwise_nms(boxes, scores, labels, class_thresholds, max_dets=500):
    """nms_better2.py:266-297: per class rotate_nms_pcdet with that class's threshold and no pre-max cut, the survivors of all
    classes sorted by score, the max_dets best -> indices into the inputs, best first"""
    boxes, scores, labels = np.asarray(boxes, np.float32), np.asarray(scores), np.asarray(labels)
    kept = []
    for c in np.unique(labels):
        idx = np.nonzero(labels == c)[0]
        kept.append(idx[nms_pcdet(boxes[idx], scores[idx], class_thresholds[int(c)])])
    kept = np.concatenate(kept) if kept else np.zeros(0, np.int64)
    return kept[np.argsort(-scores[kept], kind="stable")][:max_dets]


def predict(preds, cfg, num_classes, dtype=torch.float32):
    """CenterHead.predict with double_flip on the CPU: list of per-task map dicts -> list of B dicts of numpy arrays, the boxes
    rotated back when cfg has tt_rotation; "kept" holds, per task, the kept cells of the frame (NMS order)"""
    rets = []
    for pd in preds:
        boxes, labels, scores, mask, _ = decode({k: v.clone() for k, v in pd.items()}, cfg, dtype)
        frames = []
        for b in range(boxes.shape[0]):
            cells = torch.nonzero(mask[b]).reshape(-1).numpy()
            bp, sc, lab = boxes[b][mask[b]].numpy(), scores[b][mask[b]].numpy(), labels[b][mask[b]].numpy()
            sel = nms_pcdet(bp.astype(np.float32), sc.astype(np.float32), cfg["nms"]["nms_iou_threshold"], cfg["nms"]["nms_pre_max_size"],
                            cfg["nms"]["nms_post_max_size"])
            kb = bp[sel]
            if cfg.get("tt_rotation", 0) != 0:
                kb = rotate_back(kb.astype(np.float32), cfg["tt_rotation"], np.float64 if dtype == torch.float64 else np.float32)
            frames.append({"box3d_lidar": kb, "scores": sc[sel], "label_preds": lab[sel], "kept": cells[sel]})
        rets.append(frames)
    out = []
    for b in range(len(rets[0])):
        flag, labs = 0, []
        for j, ncls in enumerate(num_classes):                   # center_head.py:440-445
            labs.append(rets[j][b]["label_preds"] + flag)
            flag += ncls
        out.append({"box3d_lidar": np.concatenate([r[b]["box3d_lidar"] for r in rets]), "scores": np.concatenate([r[b]["scores"] for r in rets]),
                    "label_preds": np.concatenate(labs), "kept": [r[b]["kept"] for r in rets]})
    return out


def gate(dev, r32, r64):
    """The tolerance of the decode and rotation tests, per component (column): with S = the mean magnitude of the column's float64
    values (its scale), the error of a value v against the float64 value t is |v - t| / max(|t|, S) -- relative to the value, and
    relative to the scale where the value is smaller than it (an absolute floor for values near 0, where a sum of four terms
    carries the rounding of the terms, not of the result).  The device passes with an error of at most 4 x the float32
    restatement's (a different order of four terms, expf / atan2f a unit or two apart) or one fp32 ulp (2^-23), whichever is larger.
    -> (ok, e_dev [C], e_ref [C])"""
    dev, r32, r64 = (np.asarray(a, np.float64).reshape(-1, np.asarray(r64).shape[-1]) for a in (dev, r32, r64))
    if r64.shape[0] == 0:
        z = np.zeros(r64.shape[1])
        return True, z, z
    scale = np.maximum(np.abs(r64).mean(0), 1e-30)
    den = np.maximum(np.abs(r64), scale)
    e_dev, e_ref = (np.abs(dev - r64) / den).max(0), (np.abs(r32 - r64) / den).max(0)
    return bool(np.all(e_dev <= np.maximum(4 * e_ref, 2.0 ** -23))), e_dev, e_ref
