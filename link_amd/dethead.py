"""link_amd/dethead.py -- CenterHead.predict on the device: the decode of the head's maps (csrc/boxnms.hip: k_center_decode) followed by
NMS (link_amd/boxnms.py), as detection/det3d/models/bbox_heads/center_head.py:296-510 composes them.

CenterHeadDecoder takes what the head's forward returns -- a list with one dict of NCHW maps per task (hm, reg, height, dim, rot and
optionally vel) -- and returns the reference's ret_list.  predict is the variable-length form: like the reference it selects the
unmasked cells by boolean indexing and returns variable-length tensors, so it synchronises with the host several times per frame and
task (the mask selections and the size of the NMS result).  predict_padded has fixed shapes and no host round trip, so it can be
captured in a graph.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Sequence

import torch

from . import _lib as L
from .boxnms import circle_nms, nms_sorted, rotate_nms_pcdet


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class CenterHeadDecoder:
    def __init__(self, test_cfg, num_classes: Sequence[int]):
        for flag in ("double_flip", "per_class_nms"):
            if _get(test_cfg, flag, False):
                raise NotImplementedError(f"CenterHeadDecoder: test_cfg.{flag} is not built")
        if _get(test_cfg, "tt_rotation", 0) != 0:
            raise NotImplementedError("CenterHeadDecoder: test_cfg.tt_rotation is not built")
        self.num_classes = [int(c) for c in num_classes]
        nms = _get(test_cfg, "nms")
        self.thr = float(_get(nms, "nms_iou_threshold"))
        self.pre = int(_get(nms, "nms_pre_max_size"))
        self.post = int(_get(nms, "nms_post_max_size"))
        self.circular = bool(_get(test_cfg, "circular_nms", False))
        self.min_radius = [float(r) for r in (_get(test_cfg, "min_radius") or [])]
        if self.circular and len(self.min_radius) < len(self.num_classes):
            raise ValueError("circular_nms needs one min_radius per task")
        rng = [float(v) for v in _get(test_cfg, "post_center_limit_range")]
        if len(rng) != 6:
            raise ValueError("post_center_limit_range holds six numbers")
        g = L.LinkCenterGeom()
        g.out_size_factor = float(_get(test_cfg, "out_size_factor"))
        vs, pc = _get(test_cfg, "voxel_size"), _get(test_cfg, "pc_range")
        g.voxel_size[0], g.voxel_size[1] = float(vs[0]), float(vs[1])
        g.pc_range[0], g.pc_range[1] = float(pc[0]), float(pc[1])
        g.score_threshold = float(_get(test_cfg, "score_threshold"))
        for i, v in enumerate(rng):
            g.post_center_range[i] = v
        self.geom = g

    def decode(self, pd: Dict[str, torch.Tensor]):
        """One task's maps -> (boxes [B, H W, 7 | 9], labels int32 [B, H W], scores [B, H W] with -inf at masked cells, counts int32 [B])"""
        hm = pd["hm"]
        if not hm.is_cuda:
            raise L.LinkAmdError("CenterHeadDecoder: link_amd runs on the GPU only; there is no CPU fallback")
        maps = {k: pd[k].contiguous().float() for k in ("hm", "reg", "height", "dim", "rot")}
        vel = pd["vel"].contiguous().float() if "vel" in pd else None
        B, K, H, W = maps["hm"].shape
        boxes = torch.empty((B, H * W, 9 if vel is not None else 7), dtype=torch.float32, device=hm.device)
        labels = torch.empty((B, H * W), dtype=torch.int32, device=hm.device)
        scores = torch.empty((B, H * W), dtype=torch.float32, device=hm.device)
        counts = torch.zeros(B, dtype=torch.int32, device=hm.device)
        with torch.cuda.device(hm.device):
            L.check(L.lib().link_center_decode(maps["hm"].data_ptr(), maps["reg"].data_ptr(), maps["height"].data_ptr(), maps["dim"].data_ptr(),
                                               maps["rot"].data_ptr(), vel.data_ptr() if vel is not None else None, B, K, H, W,
                                               ctypes.byref(self.geom), boxes.data_ptr(), labels.data_ptr(), scores.data_ptr(),
                                               counts.data_ptr(), L.current_stream_handle()), "link_center_decode")
        return boxes, labels, scores, counts

    @torch.no_grad()
    def predict(self, preds: List[Dict[str, torch.Tensor]]) -> List[Dict[str, torch.Tensor]]:
        rets = []
        for task_id, pd in enumerate(preds):
            boxes, labels, scores, _ = self.decode(pd)
            frames = []
            for b in range(boxes.shape[0]):
                mask = scores[b] > float("-inf")
                box_preds, sc, lab = boxes[b][mask], scores[b][mask], labels[b][mask].long()
                for_nms = box_preds[:, [0, 1, 2, 3, 4, 5, -1]]
                if self.circular:
                    sel = circle_nms(torch.cat([for_nms[:, :2], sc.view(-1, 1)], 1), self.min_radius[task_id], self.post)
                else:
                    sel = rotate_nms_pcdet(for_nms, sc, self.thr, self.pre, self.post)
                frames.append({"box3d_lidar": box_preds[sel], "scores": sc[sel], "label_preds": lab[sel]})
            rets.append(frames)
        out = []
        for b in range(len(rets[0])):
            flag, labs = 0, []
            for j, ncls in enumerate(self.num_classes):                     # center_head.py:440-445
                labs.append(rets[j][b]["label_preds"] + flag)
                flag += ncls
            out.append({"box3d_lidar": torch.cat([r[b]["box3d_lidar"] for r in rets]), "scores": torch.cat([r[b]["scores"] for r in rets]),
                        "label_preds": torch.cat(labs), "metadata": None})
        return out

    @torch.no_grad()
    def predict_padded(self, preds: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
        """-> box3d_lidar [B, T post, C], scores [B, T post], label_preds int64 [B, T post] (-1 in unused slots), counts int32 [B, T]:
        task t's detections of frame b are the first counts[b, t] slots of [t post, (t + 1) post)."""
        post = self.post
        all_boxes, all_scores, all_labels, all_counts = [], [], [], []
        flag = 0
        for task_id, pd in enumerate(preds):
            boxes, labels, scores, counts = self.decode(pd)
            B, HW, C = boxes.shape
            pre = min(self.pre, HW)
            top_s, top_i = scores.topk(pre, dim=1, sorted=True)                 # the reference's mask, sort, cut to pre_maxsize
            cand = torch.gather(boxes, 1, top_i.unsqueeze(-1).expand(B, pre, C))
            cand_l = torch.gather(labels, 1, top_i).long()
            n_valid = counts.clamp(max=pre)
            tb = torch.zeros((B, post, C), dtype=torch.float32, device=boxes.device)
            ts = torch.zeros((B, post), dtype=torch.float32, device=boxes.device)
            tl = torch.full((B, post), -1, dtype=torch.int64, device=boxes.device)
            tc = torch.zeros(B, dtype=torch.int32, device=boxes.device)
            m = min(post, pre)
            for b in range(B):
                c = cand[b]                          # columns by slices: an index list would be a host-to-device copy
                if self.circular:
                    nb = torch.zeros((pre, 7), dtype=torch.float32, device=boxes.device)
                    nb[:, :2] = c[:, :2]
                    keep, count = nms_sorted(nb, self.min_radius[task_id], "circle", post_max=post, n_dev=n_valid[b:b + 1])
                else:                                # to_pcdet: extents swapped, heading -> -heading - pi / 2
                    nb = torch.cat([c[:, 0:3], c[:, 4:5], c[:, 3:4], c[:, 5:6], -c[:, -1:] - math.pi / 2], 1)
                    keep, count = nms_sorted(nb, self.thr, "rotate", post_max=post, n_dev=n_valid[b:b + 1])
                k = keep[:m]
                ok = k >= 0
                kc = k.clamp(min=0)
                tb[b, :m] = cand[b][kc] * ok.unsqueeze(-1)
                ts[b, :m] = torch.where(ok, top_s[b][kc], ts[b, :m])
                tl[b, :m] = torch.where(ok, cand_l[b][kc] + flag, tl[b, :m])
                tc[b:b + 1] = count
            flag += self.num_classes[task_id]
            all_boxes.append(tb); all_scores.append(ts); all_labels.append(tl); all_counts.append(tc)
        return {"box3d_lidar": torch.cat(all_boxes, 1), "scores": torch.cat(all_scores, 1), "label_preds": torch.cat(all_labels, 1),
                "counts": torch.stack(all_counts, 1)}
