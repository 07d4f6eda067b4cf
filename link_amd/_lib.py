"""link_amd/_lib.py -- ctypes binding of liblink_amd.so (the C ABI declared in include/link_amd.h).

The product path is HIP-only: if the shared library is missing this module raises at import of the
first symbol -- there is no CPU or PyTorch fallback (the oracle under oracle/ is test infrastructure
and is never imported from here).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "lib", "liblink_amd.so")

LINK_OK, LINK_ERR_ARG, LINK_ERR_LAUNCH, LINK_ERR_WORKSPACE, LINK_BATCH_TIMEOUT = 0, -1, -2, -3, -4
HDR_M, HDR_STATUS, HDR_NVALID, HDR_STATUS_ACC, HDR_WORDS = 0, 1, 2, 3, 8
OP_COS, OP_SIN, OP_COSX = 0, 1, 2
ELK_LANE_CHANNEL, ELK_NO_PAIR, ELK_FUSED_GATHER, ELK_NO_DENSE_GRID, ELK_TILES = 1, 2, 4, 8, 16     # link_elk_desc_t::flags
ELK_LEAN_CS, ELK_LEAN_NO_CS, ELK_LEAN_PM, ELK_LEAN_NO_PM = 32, 64, 128, 256
IO_F32, IO_F16, IO_BF16 = 0, 1, 2
ABI_VERSION = 13
# LINK_AMD_DEBUG=1: read the device status word back after every core call (one 32-byte D2H sync per call) and
# raise when the index dropped a voxel -- the sync-free default trusts the caller's bounds
DEBUG = os.environ.get("LINK_AMD_DEBUG", "0") not in ("", "0")


class LinkGrid(Structure):
    """link_grid_t"""
    _fields_ = [("s", c_int32), ("lo", c_int32 * 4), ("dim", c_int32 * 4)]

    @property
    def cells(self) -> int:
        v = 1
        for d in self.dim:
            v *= int(d)
        return v

    def key(self):
        return (int(self.s), tuple(int(x) for x in self.lo), tuple(int(x) for x in self.dim))


class LinkElkDesc(Structure):
    """link_elk_desc_t"""
    _fields_ = [("op", c_int32), ("c", c_int32), ("cg", c_int32), ("r", c_int32),
                ("coord_div", c_float), ("eps", c_float), ("flags", c_int32)]


class LinkElkBuffers(Structure):
    """link_elk_buffers_t"""
    _fields_ = [(k, c_void_p) for k in ("feats", "coords", "w_pre", "pre_ln_w", "pre_ln_b", "w_pos", "alpha",
                                        "ln_w", "ln_b", "cell_counts", "scratch")] + \
               [("scratch_bytes", c_size_t)] + \
               [(k, c_void_p) for k in ("cell_blk", "vox_blk", "idx_query", "perm", "vox_sorted", "pos_blk", "blk_start",
                                        "blk_coords", "counts", "hdr", "fin", "S", "A", "out")] + \
               [("s_bytes", c_int64), ("io_dtype", c_int32), ("reserved", c_int32), ("cell_pair", c_void_p)]


class LinkDcGrid(Structure):
    """link_dc_grid_t (dense-cell path: padded grid + slot capacity)"""
    _fields_ = [("s", c_int32), ("lo", c_int32 * 4), ("dim", c_int32 * 4), ("pdim", c_int32 * 3),
                ("k", c_int32), ("vp", c_int64)]

    @property
    def interior_cells(self) -> int:
        v = 1
        for d in self.dim:
            v *= int(d)
        return v


class LinkDcTuning(Structure):
    """link_dc_tuning_t: launch geometry / kernel selection of ONE plan (all zero = defaults)"""
    _fields_ = [(k, c_int32) for k in ("k1_wgs", "k2_zsplit", "k1_lds_pad", "k2_lds_pad", "k1_form", "k2_form", "mode",
                                       "reserved0", "reserved")] + [("k1_dbg", c_void_p), ("k2_dbg", c_void_p)]


class LinkDcBuffers(Structure):
    """link_dc_buffers_t"""
    _fields_ = [(k, c_void_p) for k in ("feats", "coords", "w_pre", "pre_ln_w", "pre_ln_b", "w_pos", "alpha",
                                        "ln_w", "ln_b", "cnt", "slots", "sid", "vrec", "vcell", "cell_n", "hdr", "fin",
                                        "S", "A", "out")] + [("io_dtype", c_int32), ("tune", LinkDcTuning)]


class LinkLeanBuffers(Structure):
    """link_lean_buffers_t (lean form of R_core: three launches with the index rebuilt)"""
    _fields_ = [(k, c_void_p) for k in ("feats", "coords", "w_pre", "pre_ln_w", "pre_ln_b", "w_pos", "alpha", "ln_w", "ln_b",
                                        "cnt", "cnt_prev", "list", "rec2", "occ", "occ_prev", "ctrl", "ctrl_prev", "X", "S",
                                        "hdr", "out")] + [("seg_cap", c_int64), ("k", c_int32), ("io_dtype", c_int32), ("cnt_shift", c_int32), ("reserved", c_int32)]


LEAN_KMAX, LEAN_SEGS, LEAN_CHUNK = 352, 16, 32
BLOCK_DONE, BLOCK_MISS = 0, 1


class LinkBlockArgs(Structure):
    """link_block_args_t (section G: one host call per LinK block on a new coordinate set)"""
    _fields_ = [("buf", POINTER(LinkDcBuffers)), ("g", POINTER(LinkDcGrid)), ("desc", POINTER(LinkElkDesc)), ("n", c_int64),
                ("mean_max", c_int32), ("cell_max", c_int32), ("ts", c_int32), ("subm", c_int32),
                ("nbr", c_void_p), ("pair_arena", c_void_p),
                ("pair_arena_words", c_int64), ("contrib", c_void_p), ("contrib_rows", c_int64), ("w", c_void_p), ("ws", c_void_p),
                ("w_big", c_void_p), ("nl_w", c_void_p), ("nl_b", c_void_p), ("nl_eps", c_float), ("flags", c_int32),
                ("out", c_void_p), ("bbox", c_int32 * 8), ("stats", c_int32 * 4), ("verdict", c_int32), ("reserved", c_int32)]


NMS_ROTATE, NMS_NORMAL, NMS_CIRCLE = 0, 1, 2


class LinkCenterGeom(Structure):
    """link_center_geom_t (section I: CenterHead decode)"""
    _fields_ = [("out_size_factor", c_float), ("voxel_size", c_float * 2), ("pc_range", c_float * 2), ("score_threshold", c_float),
                ("post_center_range", c_float * 6)]


VOXELIZE_HARD, VOXELIZE_DYNAMIC = 0, 1
STRUCT_VOXELIZE_GEOM = 8                                      # its id for link_abi_struct_size (its place in the tuple lib() checks)


class LinkVoxelizeGeom(Structure):
    """link_voxelize_geom_t (section J: point clouds to voxels)"""
    _fields_ = [("lo", c_float * 3), ("hi", c_float * 3), ("vs", c_float * 3), ("grid", c_int32 * 3), ("max_points", c_int32),
                ("max_voxels", c_int32), ("ndim", c_int32), ("mode", c_int32)]


SEGLOSS_LOGITS, SEGLOSS_PROBAS = 0, 1                         # link_segloss_forward::input_kind
SEGLOSS_PRESENT, SEGLOSS_ALL = 0, 1                           # link_segloss_forward::classes
SEGLOSS_MIN_CLASSES, SEGLOSS_MAX_CLASSES = 2, 32


SEGQ_INT, SEGQ_ROUND = 0, 1                                   # link_seg_quantize::mode
SEGQ_FLAG_EXTENT, SEGQ_FLAG_NONFINITE, SEGQ_FLAG_KEYBITS = 1, 2, 4
SORT_TILE = 2048                                              # LINK_SEGQ_SORT_TILE: pairs per tile of the quantiser's radix sort
SEGEVAL_ROWS, SEGEVAL_PREDICTIONS = 0, 1                      # link_seg_vote_eval::input_kind
SEGEVAL_MAX_VOTES = 16


ROI_MAX_ROIS, ROI_MAX_GT, ROI_MAX_SAMPLES, ROI_MAX_LOSS_ROWS = 4096, 512, 1024, 1 << 20     # section O limits
ROI_STATUS_NO_CANDIDATE, ROI_STATUS_BAD_INDEX = 1, 2
CENTER_LOGITS, CENTER_PROBAS = 0, 1                           # link_center_loss_forward::input_kind
CENTER_MAX_TASKS, CENTER_MAX_CLASSES, CENTER_MAX_OBJECTS, CENTER_MAX_SLOTS, CENTER_MAX_BATCH = 8, 16, 2048, 4096, 1024
STRUCT_CENTER_ASSIGN_GEOM = 9                                 # its id for link_abi_struct_size


class LinkCenterAssignGeom(Structure):
    """link_center_assign_geom_t (section L: CenterHead target assignment)"""
    _fields_ = [("pc_range", c_float * 2), ("voxel_size", c_float * 2), ("gaussian_overlap", c_float), ("out_size_factor", c_int32),
                ("w", c_int32), ("h", c_int32), ("max_objs", c_int32), ("min_radius", c_int32), ("num_tasks", c_int32),
                ("num_classes", c_int32 * 8)]


DETAUG_MAX_GROUPS, DETAUG_MAX_CANDIDATES, DETAUG_MAX_BOXES = 16, 64, 1024     # section P limits
DETAUG_STATUS_BAD_INDEX, DETAUG_STATUS_POINTS_CUT, DETAUG_STATUS_BOXES_CUT = 1, 2, 4
STRUCT_DETAUG_SAMPLE_CFG, STRUCT_DETAUG_TRANSFORM_CFG = 11, 12       # their ids for link_abi_struct_size (10 is kept unassigned)


class LinkDetaugSampleCfg(Structure):
    """link_detaug_sample_cfg_t (section P: the ground-truth sampler's scan)"""
    _fields_ = [("rate", c_double)] + [(k, c_int32) for k in ("n_groups", "max_candidates", "max_gt", "min_points", "box_len", "reserved")] + \
               [("group_class", c_int32 * 16), ("group_max", c_int32 * 16)]


class LinkDetaugTransformCfg(Structure):
    """link_detaug_transform_cfg_t (section P: paste, global transforms, range filter)"""
    _fields_ = [(k, c_double) for k in ("rot_lo", "rot_hi", "scale_lo", "scale_hi")] + \
               [("translate_std", c_double * 3), ("flip_probability", c_double), ("range", c_double * 4), ("max_objs", c_int32),
                ("point_capacity", c_int32)]


TRACK_MAX_LABELS, TRACK_MAX_CAPACITY, TRACK_STATUS_OVERFLOW = 32, 1024, 1      # section Q limits
TRACK_HDR_BYTES = 32                                          # int32 n_tracks, id_count, status, capacity, 4 x reserved
STRUCT_TRACK_CFG = 13                                         # its id for link_abi_struct_size


class LinkTrackCfg(Structure):
    """link_track_cfg_t (section Q: the tracker's settings)"""
    _fields_ = [(k, c_int32) for k in ("n_det_labels", "n_track_labels", "max_age", "capacity")] + \
               [("score_thresh", c_float), ("reserved", c_int32), ("label_map", c_int32 * 32), ("max_dist", c_float * 32)]


DCN_MAX_TAPS, DCN_MAX_CHANNELS, DCN_RELU = 49, 256, 1         # section R limits and flag
STRUCT_DEFORM_CONV_GEOM = 14                                  # its id for link_abi_struct_size


class LinkDeformConvGeom(Structure):
    """link_deform_conv_geom_t (section R: deformable convolution)"""
    _fields_ = [(k, c_int32) for k in ("batch", "c", "h", "w", "o", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w", "dil_h", "dil_w",
                                       "groups", "deformable_groups", "offset_channels", "io_dtype", "flags")]


PILLAR_MAX_T, PILLAR_MAX_D, PILLAR_MAX_WIDTH = 64, 8, 128      # section S: the reader's native range


class LinkPillarGeom(Structure):
    """link_pillar_geom_t (section S: the PointPillars reader); struct_bytes carries its own size, the entries check it"""
    _fields_ = [(k, c_int32) for k in ("struct_bytes", "t", "d", "with_distance", "layers")] + [("width", c_int32 * 2)] + \
               [(k, c_int32) for k in ("batch", "ny", "nx", "io_dtype")] + [(k, c_float) for k in ("vx", "vy", "x_offset", "y_offset")]


class LinkPillarLayer(Structure):
    """link_pillar_layer_t (section S: one PFN layer's Linear.weight and BatchNorm1d tensors)"""
    _fields_ = [(k, c_void_p) for k in ("weight", "gamma", "beta", "running_mean", "running_var")] + [("eps", c_float), ("reserved", c_int32)]


# name -> (restype, argtypes); every symbol include/link_amd.h declares
SIGNATURES = {
    "link_abi_version": (c_int, []),
    "link_abi_struct_size": (c_int32, [c_int32]),
    "link_last_error": (c_char_p, []),
    "link_hash": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "link_kernel_hash": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "link_hash_query_workspace_bytes": (c_size_t, [c_int64]),
    "link_hash_query": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "link_count": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "link_ti_weights": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_void_p, c_void_p]),
    "link_voxelize_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                      c_void_p]),
    "link_voxelize_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "link_voxelize_backward_n1": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "link_devoxelize_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                        c_void_p]),
    "link_devoxelize_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                         c_void_p, c_void_p]),
    "link_grid_from_bounds": (c_int64, [POINTER(c_int32), POINTER(c_int32), c_int32, POINTER(LinkGrid)]),
    "link_coords_bbox": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "link_index_scratch_bytes": (c_size_t, [c_int64, c_int64]),
    "link_index_build": (c_int, [c_void_p, c_int64, POINTER(LinkGrid), c_void_p, c_void_p, c_size_t,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_index_build_first": (c_int, [c_void_p, c_int64, POINTER(LinkGrid), c_void_p, c_void_p, c_size_t] + [c_void_p] * 11),
    "link_block_gather": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(LinkGrid), c_void_p,
                                  POINTER(LinkElkDesc), c_int64, c_void_p, c_void_p]),
    "link_voxel_demod_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, POINTER(LinkElkDesc), c_int64, c_void_p, c_void_p]),
    "link_neighbor_map": (c_int, [c_void_p, c_void_p, POINTER(LinkGrid), c_void_p, c_int64, c_int32,
                                  c_int32, c_int32, c_void_p, c_void_p]),
    "link_cell_table_build": (c_int, [c_void_p, c_int64, POINTER(LinkGrid), c_void_p, c_void_p, c_void_p]),
    "link_conv_site_table": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "link_conv_gather_table": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                       c_void_p]),
    "link_cell_table_clear": (c_int, [c_void_p, c_int64, POINTER(LinkGrid), c_void_p, c_void_p]),
    "link_block_mean": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                c_void_p, c_void_p]),
    "link_aux_to_voxel_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                          c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_aux_to_voxel_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                           c_void_p]),
    "link_premix_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float,
                               c_void_p, c_void_p]),
    "link_modulate_block_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, POINTER(LinkElkDesc), c_int64, c_int64, c_void_p,
                                        c_void_p]),
    "link_gather_demod_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, POINTER(LinkGrid), c_void_p,
                                     POINTER(LinkElkDesc), c_int64, c_int64, c_void_p, c_void_p]),
    "link_elk_core_forward": (c_int, [POINTER(LinkElkBuffers), POINTER(LinkGrid), POINTER(LinkElkDesc),
                                      c_int64, c_int64, c_int32, c_void_p]),
    "link_elk_tiles_table_bytes": (c_int64, [POINTER(LinkElkDesc), c_int64, c_int64]),
    "link_elk_premix_modsum_tiles": (c_int, [c_void_p] * 10 + [POINTER(LinkElkDesc), c_int64, c_int64, c_void_p, c_int64,
                                             c_void_p, c_void_p]),
    "link_elk_gather_demod_tiles": (c_int, [c_void_p] * 6 + [POINTER(LinkGrid)] + [c_void_p] * 5 +
                                    [POINTER(LinkElkDesc), c_int64, c_int64, c_void_p, c_void_p]),
    "link_elk_premix_modsum_tiles_io": (c_int, [c_void_p, c_int32] + [c_void_p] * 9 + [POINTER(LinkElkDesc), c_int64, c_int64, c_void_p,
                                                c_int64, c_void_p, c_void_p]),
    "link_elk_gather_demod_tiles_io": (c_int, [c_void_p] * 6 + [POINTER(LinkGrid)] + [c_void_p] * 5 +
                                       [POINTER(LinkElkDesc), c_int64, c_int64, c_void_p, c_int32, c_void_p]),
    "link_elk_mid_forward": (c_int, [c_void_p] * 6 + [POINTER(LinkGrid), c_void_p, c_void_p, c_void_p,
                                     POINTER(LinkElkDesc), c_void_p, c_void_p, c_int64, c_int64] + [c_void_p] * 5),
    "link_elk_out_ln_backward": (c_int, [c_void_p] * 9 + [POINTER(LinkElkDesc), c_int64, c_void_p, c_void_p,
                                         c_void_p]),
    "link_subm_conv_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                       c_void_p, c_void_p]),
    "link_aux_to_voxel_forward_grid": (c_int, [c_void_p] * 4 + [POINTER(LinkGrid), c_void_p, c_void_p, c_int64,
                                               c_int64, c_int32, c_int32] + [c_void_p] * 5),
    "link_aux_to_voxel_forward_scatter": (c_int, [c_void_p] * 4 + [POINTER(LinkGrid), c_void_p, c_void_p, c_void_p, c_int64,
                                                  c_int64, c_int32, c_int32] + [c_void_p] * 4),
    "link_conv_pairs_supported": (c_int, [c_int32, c_int32]),
    "link_conv_pairs_gemm": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "link_conv_pairs_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p,
                                    c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "link_index_cells": (c_int, [c_void_p, c_int64, POINTER(LinkGrid), c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "link_conv_out_candidate_count": (c_int32, [c_void_p, c_void_p]),
    "link_conv_out_candidates": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # kernel maps of any per-axis kernel size / stride (csrc/kmap.hip)
    "link_kmap_candidate_count": (c_int32, [c_void_p, c_void_p]),
    "link_kmap_out_candidates": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_kmap_box_table": (c_int, [c_void_p, c_int64, c_void_p, POINTER(LinkGrid), c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_kmap_transpose": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p]),
    "link_conv_pairs_gemm_io": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "link_conv_pairs_sum_io": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p,
                                       c_float, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "link_conv_centre_sum_io": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                        c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "link_conv_pairs_gemm_amp": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "link_conv_centre_sum_amp": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                         c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "link_bn_partial_workgroups": (c_int32, [c_int64, c_int32]),
    "link_bn_forward_stats": (c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_bn_backward_reduce": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "link_bn_apply_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "link_bn_backward_reduce_relu": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_bn_apply_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "link_conv_pairs_gemm_split": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "link_pair_plan_count": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_pair_plan_fill": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "link_subm_conv_resident_amp": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                            c_void_p, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "link_pair_plan_build": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int64] + [c_void_p] * 13),
    "link_pair_plan_layout": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "link_conv_pairs_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64,
                                      c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_conv_centre_sum": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                     c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "link_subm_conv_wgrad_chunks": (c_int32, []),
    "link_subm_conv_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "link_subm_conv_wgrad_split": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "link_subm_conv_wgrad_reduce": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "link_subm_conv_ln_add_relu": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                           c_void_p, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "link_ln_add_relu_forward": (c_int, [c_void_p] * 4 + [c_int64, c_int32, c_float, c_void_p, c_void_p]),
    "link_ln_add_relu_backward": (c_int, [c_void_p] * 4 + [c_int64, c_int32, c_float] + [c_void_p] * 4),
    "link_sum_partials": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_void_p,
                                  c_void_p]),
    "link_premix_ln_backward": (c_int, [c_void_p] * 4 + [c_int64, c_int32, ctypes.c_float] + [c_void_p] * 4),
    # autocast training (ABI 13): 16-bit rows at the boundary of the training kernels (io_dtype = IO_*)
    "link_premix_ln_io": (c_int, [c_void_p, c_int32] + [c_void_p] * 3 + [c_int64, c_int32, c_float, c_void_p, c_void_p]),
    "link_premix_ln_backward_io": (c_int, [c_void_p, c_int32] + [c_void_p] * 3 + [c_int64, c_int32, c_float] + [c_void_p] * 4),
    "link_ln_add_relu_forward_io": (c_int, [c_void_p, c_int32] + [c_void_p] * 3 + [c_int64, c_int32, c_float, c_void_p, c_void_p]),
    "link_ln_add_relu_backward_io": (c_int, [c_void_p] * 3 + [c_int32, c_void_p, c_int64, c_int32, c_float] + [c_void_p] * 4),
    "link_bn_forward_stats_io": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_float, c_float] + [c_void_p] * 10),
    "link_bn_apply_forward_io": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "link_bn_backward_reduce_io": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int32] + [c_void_p] * 6),
    "link_bn_backward_reduce_relu_io": (c_int, [c_void_p, c_void_p, c_int32] + [c_void_p] * 4 + [c_int64, c_int32] + [c_void_p] * 6),
    "link_bn_apply_backward_io": (c_int, [c_void_p, c_void_p, c_int32] + [c_void_p] * 4 + [c_int64, c_int32, c_void_p, c_void_p]),
    "link_elk_mid_partial_rows": (c_int32, []),
    "link_dc_grid_from": (c_int64, [POINTER(LinkGrid), c_int32, POINTER(LinkDcGrid)]),
    "link_dc_premix_insert": (c_int, [c_void_p] * 5 + [c_int64, c_int32, c_float, POINTER(LinkDcGrid), c_int32] +
                              [c_void_p] * 7),
    "link_dc_modsum": (c_int, [c_void_p] * 6 + [POINTER(LinkElkDesc), POINTER(LinkDcGrid), c_int32, c_void_p,
                               c_void_p, c_void_p]),
    "link_dc_gather": (c_int, [c_void_p, c_void_p, POINTER(LinkElkDesc), POINTER(LinkDcGrid), c_void_p, c_void_p]),
    "link_elk_core_dense_forward": (c_int, [POINTER(LinkDcBuffers), POINTER(LinkDcGrid), POINTER(LinkElkDesc),
                                            c_int64, c_int32, c_void_p]),
    "link_elk_core_lean_forward": (c_int, [POINTER(LinkLeanBuffers), POINTER(LinkGrid), POINTER(LinkElkDesc), c_int64, c_int64,
                                           c_int32, c_void_p]),
    "link_dc_index_probe": (c_int, [POINTER(LinkDcBuffers), POINTER(LinkDcGrid), c_int64, c_void_p, c_void_p]),
    "link_dc_index_ids": (c_int, [c_void_p, c_int64, POINTER(LinkDcGrid)] + [c_void_p] * 5),
    "link_dc_index": (c_int, [c_void_p, c_int64, POINTER(LinkDcGrid)] + [c_void_p] * 5),
    "link_dc_premix_modsum": (c_int, [POINTER(LinkDcBuffers), POINTER(LinkDcGrid), POINTER(LinkElkDesc), c_int64,
                                      c_int32, c_void_p]),
    "link_dc_gather_demod": (c_int, [POINTER(LinkDcBuffers), POINTER(LinkDcGrid), POINTER(LinkElkDesc), c_int64, c_void_p]),
    "link_dc_demod": (c_int, [c_void_p] * 8 + [POINTER(LinkElkDesc), POINTER(LinkDcGrid), c_int64, c_void_p, c_int32,
                              c_void_p]),
    "link_block_ctx_create": (c_int, [POINTER(c_void_p)]),
    "link_block_ctx_destroy": (c_int, [c_void_p]),
    "link_pair_plan_arena": (c_int64, [c_int64, c_int32, c_int32, POINTER(c_int64)]),
    "link_dc_neighbor_map": (c_int, [c_void_p, c_int64, POINTER(LinkDcGrid), c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "link_elk_block_forward": (c_int, [c_void_p, POINTER(LinkBlockArgs), c_void_p]),
    "link_dc_batch_create": (c_int, [POINTER(c_void_p)]),
    "link_dc_batch_destroy": (c_int, [c_void_p]),
    "link_elk_core_dense_forward_batch": (c_int, [c_void_p, POINTER(LinkDcBuffers), POINTER(c_int64), c_int32, POINTER(LinkDcGrid),
                                                  POINTER(LinkElkDesc), c_void_p]),
    "link_dc_batch_submit": (c_int, [c_void_p, POINTER(LinkDcBuffers), POINTER(c_int64), c_int32, POINTER(LinkDcGrid),
                                     POINTER(LinkElkDesc), c_void_p, POINTER(c_int64)]),
    "link_dc_batch_join": (c_int, [c_void_p, c_int64, c_void_p]),
    "link_dc_batch_set_timing": (c_int, [c_void_p, c_int32]),
    "link_dc_batch_kernel_times": (c_int, [c_void_p, c_int64, POINTER(c_float)]),
    "link_dc_batch_status": (c_int, [c_void_p, POINTER(c_int32)]),
    "link_dc_batch_set_debug": (c_int, [c_void_p, c_void_p, c_void_p]),
    "link_dc_batch_probe_streams": (c_int, [c_void_p, c_void_p, POINTER(ctypes.c_double)]),
    "link_streams_share_queue": (c_int, [c_void_p, c_void_p, POINTER(ctypes.c_double)]),
    "link_elk_mid_backward": (c_int, [c_void_p] * 9 + [POINTER(LinkGrid), c_void_p, c_void_p, c_void_p,
                                      POINTER(LinkElkDesc), c_int64, c_int64] + [c_void_p] * 5),
    # section I: detection post-processing (csrc/boxnms.hip)
    "link_boxes_overlap_bev": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "link_boxes_iou_bev": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "link_nms_workspace_bytes": (c_size_t, [c_int64]),
    "link_nms_mask": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_float, c_void_p, c_void_p]),
    "link_nms_reduce": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_nms_bev": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_float, c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "link_center_decode": (c_int, [c_void_p] * 6 + [c_int32] * 4 + [POINTER(LinkCenterGeom)] + [c_void_p] * 5),
    # section J: point clouds to voxels (csrc/voxelize.hip)
    "link_voxelize_workspace_bytes": (c_size_t, [POINTER(LinkVoxelizeGeom), c_int64, c_int32]),
    "link_voxelize": (c_int, [POINTER(LinkVoxelizeGeom), c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_size_t] + [c_void_p] * 4 +
                      [c_int64, c_void_p, c_void_p]),
    # section K: segmentation criterion, cross-entropy + Lovasz-softmax (csrc/segloss.hip)
    "link_segloss_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "link_segloss_forward": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_int64, c_int32, c_int64, c_int64, c_int32, c_int32, c_void_p,
                                     c_size_t, c_void_p, c_void_p, c_void_p]),
    "link_segloss_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    # section L: CenterHead training -- target assignment, focal + L1 loss (csrc/centerloss.hip)
    "link_center_assign": (c_int, [POINTER(LinkCenterAssignGeom), c_void_p, c_void_p, c_int32, c_int32] + [POINTER(c_void_p)] * 5 + [c_void_p]),
    "link_center_loss_workspace_bytes": (c_size_t, [c_int32] * 5),
    "link_center_loss_forward": (c_int, [c_void_p] * 6 + [POINTER(c_int64), c_int32, c_int32] + [c_void_p] * 5 + [c_int32] * 5 + [POINTER(c_float), c_float, c_void_p,
                                         c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_center_loss_backward": (c_int, [c_void_p] * 5 + [c_int32] * 6 + [c_void_p] * 6 + [POINTER(c_int64), c_void_p]),
    # section M: segmentation front end and validation -- quantise, vote, count (csrc/segio.hip)
    "link_seg_quantize_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "link_seg_quantize": (c_int, [c_void_p, c_int32, c_int32, c_float, c_void_p, c_int32, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                                  c_int64] + [c_void_p] * 5),
    "link_seg_vote_eval": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_int32, c_void_p, c_int32, c_int64, c_void_p, c_int64] +
                           [c_void_p] * 4),
    # section N: CenterHead test-time augmentation -- views, fused decode, class-wise NMS mask, rotation back (csrc/dettta.hip)
    "link_tta_views": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "link_center_decode_flip4": (c_int, [c_void_p] * 6 + [c_int32] * 4 + [POINTER(LinkCenterGeom)] + [c_void_p] * 5),
    "link_nms_mask_classwise": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "link_tta_rotate_back": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_float, c_float, c_float, c_void_p, c_void_p]),
    # section O: two-stage ROI head -- BEV features, target assignment, loss, refinement (csrc/roihead.hip)
    "link_roi_bev_features": (c_int, [c_void_p, c_int32, POINTER(c_int64), c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_int32, c_int32,
                                      c_void_p, c_void_p, c_int64, c_int32, POINTER(c_float), POINTER(c_float), c_float, c_void_p, c_void_p]),
    "link_roi_assign": (c_int, [c_void_p] * 6 + [c_int32, c_int64, c_int64, c_int64, c_int32, c_double, c_int32, c_int32] + [c_double] * 5 +
                        [c_void_p] * 13),
    "link_roi_loss_forward": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p, POINTER(c_float), c_float,
                                      c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "link_roi_loss_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_roi_refine": (c_int, [c_void_p] * 5 + [c_int32, c_int32, c_int64, c_int32] + [c_void_p] * 5),
    # section P: geometry of the detection training front end -- points in rotated boxes, BEV corners, collisions (csrc/detaug.hip)
    "link_points_in_rbbox": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_box2d_corners": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p, c_void_p]),
    "link_box_collision": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "link_detaug_sample": (c_int, [POINTER(LinkDetaugSampleCfg), c_int32] + [c_void_p] * 8 + [c_int64] + [c_void_p] * 8),
    "link_detaug_transform": (c_int, [POINTER(LinkDetaugTransformCfg), c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                      c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int32] + [c_void_p] * 6),
    # section Q: multi-object tracker -- greedy centre matching for a batch of sequences (csrc/track.hip)
    "link_track_state_bytes": (c_size_t, [c_int32]),
    "link_track_step": (c_int, [POINTER(LinkTrackCfg), c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32] + [c_void_p] * 8),
    # section R: deformable convolution, DCN v1 (csrc/dcn.hip)
    "link_deform_conv_workspace_bytes": (c_size_t, [POINTER(LinkDeformConvGeom)]),
    "link_deform_conv_forward": (c_int, [POINTER(LinkDeformConvGeom)] + [c_void_p] * 5),
    "link_deform_conv_backward_data": (c_int, [POINTER(LinkDeformConvGeom)] + [c_void_p] * 8),
    "link_deform_conv_backward_weight": (c_int, [POINTER(LinkDeformConvGeom)] + [c_void_p] * 6 + [c_size_t, c_void_p]),
    # section S: the PointPillars reader and its BEV scatter (csrc/pillar.hip)
    "link_pillar_native": (c_int, [POINTER(LinkPillarGeom)]),
    "link_pillar_reader": (c_int, [POINTER(LinkPillarGeom)] + [c_void_p] * 3 + [c_int64, c_void_p, POINTER(LinkPillarLayer),
                                   POINTER(LinkPillarLayer)] + [c_void_p] * 3),
    "link_pillar_scatter": (c_int, [POINTER(LinkPillarGeom), c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_pillar_gather": (c_int, [POINTER(LinkPillarGeom), c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "link_pillar_decorate": (c_int, [POINTER(LinkPillarGeom), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
}

_lib = None


class LinkAmdError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load liblink_amd.so (once).  Fails loudly: no fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise LinkAmdError(
                f"{SO_PATH} not found: the HIP extension is not built. Run `python link_amd/build.py` "
                "(or __graft_entry__.build()). link_amd has no CPU/PyTorch fallback.")
        handle = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)   # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if handle.link_abi_version() != ABI_VERSION:
            raise LinkAmdError("liblink_amd.so ABI version mismatch; rebuild with link_amd/build.py")
        structs = list(enumerate((LinkGrid, LinkElkDesc, LinkElkBuffers, LinkDcGrid, LinkDcTuning, LinkDcBuffers, LinkLeanBuffers, LinkBlockArgs,
                                  LinkVoxelizeGeom, LinkCenterAssignGeom)))
        structs += [(STRUCT_DETAUG_SAMPLE_CFG, LinkDetaugSampleCfg), (STRUCT_DETAUG_TRANSFORM_CFG, LinkDetaugTransformCfg),
                    (STRUCT_TRACK_CFG, LinkTrackCfg), (STRUCT_DEFORM_CONV_GEOM, LinkDeformConvGeom)]
        for which, cls in structs:
            if handle.link_abi_struct_size(which) != ctypes.sizeof(cls):
                raise LinkAmdError(f"liblink_amd.so: layout of {cls.__name__} differs from include/link_amd.h "
                                   f"({ctypes.sizeof(cls)} bytes here, {handle.link_abi_struct_size(which)} in the library)")
        _lib = handle
    return _lib


def current_stream_handle() -> int:
    """hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream() builds a Python
    Stream object (~10 us); the raw query is what torch's own compiled code uses (~0.3 us) -- it matters on the
    module path, where a stage is a dozen FFI calls."""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:                      # private API moved: fall back to the public one
        return torch.cuda.current_stream().cuda_stream


def check(rc: int, what: str) -> None:
    if rc != LINK_OK:
        msg = {LINK_ERR_ARG: "invalid argument", LINK_ERR_LAUNCH: "HIP launch failure",
               LINK_ERR_WORKSPACE: "workspace too small",
               LINK_BATCH_TIMEOUT: "a bounded wait inside a persistent batch kernel gave up"}.get(rc, f"error {rc}")
        detail = lib().link_last_error()
        raise LinkAmdError(f"{what}: {msg}" + (f" ({detail.decode()})" if detail else ""))


def ptr(t):
    """the data pointer of an optional tensor: None stays None (NULL)"""
    return None if t is None else t.data_ptr()


def point_offsets(cache: dict, device, sizes):
    """int32 [B + 1] on the device, the running sum of `sizes`; kept in the caller's `cache` per tuple of sizes, so a call with sizes
    seen before copies nothing from the host (a captured graph has fixed sizes: the call that warms it up leaves the tensor here).
    A cache that holds 64 entries is emptied first."""
    import numpy as np
    import torch
    key = (device, tuple(sizes))
    t = cache.get(key)
    if t is None:
        if len(cache) >= 64:
            cache.clear()
        t = cache[key] = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32).to(device)
    return t


def grid_from_bounds(lo, hi, s: int) -> LinkGrid:
    """Host helper (no GPU needed): block grid covering voxel coords lo..hi (inclusive)."""
    g = LinkGrid()
    lo_a = (c_int32 * 4)(*[int(x) for x in lo])
    hi_a = (c_int32 * 4)(*[int(x) for x in hi])
    v = lib().link_grid_from_bounds(lo_a, hi_a, int(s), ctypes.byref(g))
    if v < 0:
        raise LinkAmdError(f"grid_from_bounds({list(lo)}, {list(hi)}, s={s}): bounds invalid or grid "
                           ">= 2^30 cells")
    return g


def dc_grid_from(grid: LinkGrid, k: int = 0):
    """Padded dense-cell grid of `grid` (slot capacity k, 0 = s^3), or None when the dense-cell path cannot
    address it (>= 2^30 cells or >= 2^31 slots)."""
    g = LinkDcGrid()
    v = lib().link_dc_grid_from(ctypes.byref(grid), int(k), ctypes.byref(g))
    return g if v > 0 else None
