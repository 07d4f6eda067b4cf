"""harness/pillars.py -- a detector of the reference's `PointPillars` shape (detection/det3d/models/detectors/point_pillars.py: reader,
backbone = scatter, neck, bbox_head) from padded voxels to the CenterHead's maps: link_amd's PillarFeatureNet and PointPillarsScatter
(fused into one kernel in eval mode, link_amd.PillarReader), then the plain-torch BevRPN and BevCenterHead of harness/bevhead.py.
The pillar half carries the reference's parameter names (`reader.pfn_layers.{i}...`); the dense half has this harness's own layout
(see bevhead.py).  `fused=False` runs reader and scatter as two modules, as the reference's extract_feat does."""
from typing import Dict, List, Sequence

import torch
import torch.nn as nn

from .bevhead import BevCenterHead, BevRPN


class PointPillars(nn.Module):
    """The nuScenes pp config's shapes by default (configs/nusc/pp/nusc_centerpoint_pp_02voxel_two_pfn_10sweep.py): D = 5, two PFN
    layers of 64, a three-level RPN on the 64-channel pseudo-image, six tasks.  The config's up-sampling strides are (0.5, 1, 2); BevRPN
    has no strided deblock, so they are (1, 2, 4) here and the head maps come out at half, not a quarter, of the canvas."""

    def __init__(self, num_input_features: int = 5, num_filters: Sequence[int] = (64, 64), with_distance: bool = False,
                 voxel_size=(0.2, 0.2, 8), pc_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), layer_nums: Sequence[int] = (3, 5, 5),
                 ds_layer_strides: Sequence[int] = (2, 2, 2), ds_num_filters: Sequence[int] = (64, 128, 256),
                 us_layer_strides: Sequence[int] = (1, 2, 4), us_num_filters: Sequence[int] = (128, 128, 128),
                 num_classes: Sequence[int] = BevCenterHead.NUSC_TASKS, fused: bool = True, la=None):
        super().__init__()
        if la is None:
            import link_amd as la
        self.reader = la.PillarFeatureNet(num_input_features, num_filters, with_distance, voxel_size, pc_range)
        self.backbone = la.PointPillarsScatter(self.reader.out_channels)
        self.fused = bool(fused)
        # the fused form shares reader and backbone; kept outside the module tree so that the state dict names them once
        object.__setattr__(self, "_reader_scatter", la.PillarReader(self.reader, self.backbone))
        self.neck = BevRPN(layer_nums, ds_layer_strides, ds_num_filters, us_layer_strides, us_num_filters, self.reader.out_channels)
        self.bbox_head = BevCenterHead(self.neck.out_channels, num_classes)

    def extract_feat(self, voxels, num_points, coors, batch_size, input_shape, count=None) -> torch.Tensor:
        if self.fused:
            canvas = self._reader_scatter(voxels, num_points, coors, batch_size, input_shape, count=count)
        else:
            rows = self.reader(voxels, num_points, coors, count=count)
            canvas = self.backbone(rows, coors, batch_size, input_shape, count=count)
        return self.neck(canvas)

    def forward(self, voxels, num_points, coors, batch_size, input_shape, count=None) -> List[Dict[str, torch.Tensor]]:
        return self.bbox_head(self.extract_feat(voxels, num_points, coors, batch_size, input_shape, count))
