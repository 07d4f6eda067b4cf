"""link_amd -- MI355X-native (gfx950, hand-written HIP) implementation of LinK's linear-kernel
sparse 3-D aggregation hot path, behind the Python surface the reference's backbones call.

Reference: MCG-NJU/LinK (segmentation/core/models/utils.py:44-84,
segmentation/core/models/semantic_kitti/linkunet.py:94-185, detection/det3d/models/utils/ts_elk.py).
The HIP library (link_amd/lib/liblink_amd.so, ABI in include/link_amd.h) is mandatory: there is no
CPU or eager-PyTorch fallback.
"""
from . import _lib, backend, functional
from .aggregate import (aux_to_voxel, large_to_small, link_index_of, small_to_large_v2, upsample_voxel,
                        voxel_to_aux)
from .elk import (Conv3d, ELKBlock, ElkCoreBatch, ElkCorePlan, SparseConvTensor, TSELKBlock, elk_core_autograd, elk_core_fused,
                  invalidate_derived_weights, spconv2ts, ts2spconv)
from . import boxnms, centerloss, dcn, detaug, dethead, dettta, pillar, roihead, segio, segloss, tracker, voxelize
from .boxnms import (boxes_iou3d_gpu, boxes_iou_bev, boxes_overlap_bev, circle_nms, install_as_iou3d_nms, nms_gpu, nms_normal_gpu,
                     nms_padded, rotate_nms_pcdet, to_pcdet)
from .centerloss import CenterHeadLoss, CenterTargetAssigner, FastFocalLoss, RegLoss
from .dcn import (DCNSepHead, DeformConv, DeformConvPack, FeatureAdaption, SepHead, deform_conv, deform_conv_native, deform_conv_relu,
                  deform_conv_torch)
from .detaug import (DatabaseSampler, DetTrainAugmenter, GTDatabase, box_collision_test, center_to_corner_box2d, install_as_box_np_ops,
                     points_count_rbbox, points_in_rbbox)
from .dethead import CenterHeadDecoder
from .dettta import CenterHeadTTADecoder, fuse_detections, fuse_detections_padded, tta_views
from .detstage import ELKv3Stage, SparseBasicBlock, SparseConv3d, SpMiddleResNetFHDELKv3, SubMConv3d, to_dense
from .functional import calc_ti_weights, spcount, spdevoxelize, sphash, sphashquery, spvoxelize
from .index import BlockIndex, coords_bounds
from .modules import BatchNorm, LeakyReLU, ReLU, fapply, fuse_for_inference
from .segio import SegEvaluator, SegVoxelizer, sparse_collate, sparse_collate_fn, sparse_quantize
from .segloss import SegCriterion, lovasz_softmax, lovasz_softmax_flat
from .roihead import BEVFeatureExtractor, ProposalTargetLayer, RoIHead, TwoStageRefiner, roi_box_points, roi_loss, roi_refine
from .pillar import (PFNLayer, PillarFeatureNet, PillarReader, PointPillarsScatter, pillar_bev, pillar_config_native, pillar_decorate,
                     pillar_native, pillar_scatter)
from .pointvoxel import initial_voxelize, point_to_voxel, voxel_to_point
from .tensor import PointTensor, SparseTensor, cat
from .tracker import CenterTracker, boxes_to_global
from .utils import get_kernel_offsets, make_ntuple
from .voxelize import DynamicVoxelEncoder, Voxelizer, points_to_voxel

__version__ = "0.1.0"


def install_as_torchsparse() -> None:
    """Register link_amd under the module names the reference imports (`torchsparse`,
    `torchsparse.nn`, `torchsparse.nn.functional`, `torchsparse.nn.utils`, `torchsparse.utils`,
    `torchsparse.utils.quantize`, `torchsparse.utils.collate`, `torchsparse.backend`) so that unmodified reference code such as
    `import torchsparse.nn.functional as F; from torchsparse import SparseTensor` resolves here."""
    import sys
    import types
    ts = types.ModuleType("torchsparse")
    ts.SparseTensor, ts.PointTensor, ts.cat = SparseTensor, PointTensor, cat
    nn_mod = types.ModuleType("torchsparse.nn")
    nn_mod.Conv3d, nn_mod.BatchNorm, nn_mod.ReLU, nn_mod.LeakyReLU = Conv3d, BatchNorm, ReLU, LeakyReLU
    nn_mod.functional = functional
    nn_utils = types.ModuleType("torchsparse.nn.utils")
    nn_utils.get_kernel_offsets = get_kernel_offsets
    nn_utils.fapply = fapply
    nn_mod.utils = nn_utils
    utils_mod = types.ModuleType("torchsparse.utils")
    utils_mod.make_ntuple = make_ntuple
    quantize_mod = types.ModuleType("torchsparse.utils.quantize")
    quantize_mod.sparse_quantize = sparse_quantize
    collate_mod = types.ModuleType("torchsparse.utils.collate")
    collate_mod.sparse_collate, collate_mod.sparse_collate_fn = sparse_collate, sparse_collate_fn
    utils_mod.quantize, utils_mod.collate = quantize_mod, collate_mod
    utils_mod.__path__ = []                                         # a package: `import torchsparse.utils.quantize` resolves
    ts.nn, ts.utils, ts.backend = nn_mod, utils_mod, backend
    ts.__version__ = "1.4.0+link_amd"
    sys.modules.update({"torchsparse": ts, "torchsparse.nn": nn_mod, "torchsparse.nn.functional": functional,
                        "torchsparse.nn.utils": nn_utils, "torchsparse.utils": utils_mod,
                        "torchsparse.utils.quantize": quantize_mod, "torchsparse.utils.collate": collate_mod,
                        "torchsparse.backend": backend})
