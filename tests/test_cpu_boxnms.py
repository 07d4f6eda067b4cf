"""CPU-only checks of the detection post-processing entries (csrc/boxnms.hip, section I of include/link_amd.h): exports and prototypes,
argument validation before anything touches a device, the workspace size, the checkers of tests/box_oracle.py against the fixtures
recorded from the reference's compiled CPU routine, the resource shape of the kernels, and the det3d module aliases."""
import os
import sys

import numpy as np
import pytest

from helpers import ROOT, golden_files, load_golden

import box_oracle as BO

SECTION_I = ("link_boxes_overlap_bev", "link_boxes_iou_bev", "link_nms_mask", "link_nms_reduce", "link_nms_bev", "link_nms_workspace_bytes",
             "link_center_decode")
PAIR_FILES = ["boxnms_pairs_1x1.npz", "boxnms_pairs_17x63.npz", "boxnms_pairs_64x64.npz", "boxnms_pairs_65x130.npz",
              "boxnms_pairs_256x192.npz"]
NMS_SIZES = [0, 1, 64, 65, 1000, 4097]


def test_section_i_symbols_exported_and_prototyped():
    import ctypes
    from link_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in SECTION_I:
        assert name + "(" in hdr, name
        assert name in L.SIGNATURES, name
        assert hasattr(handle, name), name
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13      # additive entries
    assert ctypes.sizeof(L.LinkCenterGeom) == 12 * 4


def test_section_i_validates_arguments_without_gpu():
    import ctypes
    from link_amd import _lib as L
    lib = L.lib()
    OK, ARG = L.LINK_OK, L.LINK_ERR_ARG
    one = ctypes.c_void_p(64)                                            # a non-null pointer nothing dereferences
    for fn in (lib.link_boxes_overlap_bev, lib.link_boxes_iou_bev):
        assert fn(None, 0, None, 0, None, None) == OK
        assert fn(None, 0, None, 5, None, None) == OK                    # an empty matrix
        assert fn(None, 3, None, 5, None, None) == ARG                   # null buffers with n > 0
        assert fn(one, 3, one, 5, None, None) == ARG
        assert fn(one, -1, one, 5, one, None) == ARG
    assert lib.link_nms_mask(None, 0, None, L.NMS_ROTATE, 0.2, None, None) == OK
    assert lib.link_nms_mask(None, 10, None, L.NMS_ROTATE, 0.2, None, None) == ARG
    assert lib.link_nms_mask(one, 10, None, 3, 0.2, one, None) == ARG    # unknown predicate
    assert lib.link_nms_mask(one, 10, None, -1, 0.2, one, None) == ARG
    assert lib.link_nms_mask(one, 10, None, L.NMS_NORMAL, float("nan"), one, None) == ARG
    assert lib.link_nms_mask(one, 10, None, L.NMS_CIRCLE, float("inf"), one, None) == ARG
    assert lib.link_nms_reduce(None, 0, None, 0, None, None, None) == OK
    assert lib.link_nms_reduce(None, 10, None, 0, None, None, None) == ARG
    assert lib.link_nms_reduce(one, 10, None, -1, one, one, None) == ARG
    assert lib.link_nms_bev(None, 0, None, L.NMS_ROTATE, 0.2, 0, None, 0, None, None, None) == OK
    assert lib.link_nms_bev(None, 10, None, L.NMS_ROTATE, 0.2, 0, None, 0, None, None, None) == ARG
    assert lib.link_nms_bev(one, 10, None, 7, 0.2, 0, one, 80, one, one, None) == ARG
    assert lib.link_nms_bev(one, 10, None, L.NMS_ROTATE, float("nan"), 0, one, 80, one, one, None) == ARG
    assert lib.link_nms_bev(one, 10, None, L.NMS_ROTATE, 0.2, 0, one, 79, one, one, None) == L.LINK_ERR_WORKSPACE
    g = L.LinkCenterGeom()
    assert lib.link_center_decode(None, None, None, None, None, None, 0, 1, 8, 8, ctypes.byref(g), None, None, None, None, None) == OK
    assert lib.link_center_decode(None, None, None, None, None, None, 2, 1, 8, 8, ctypes.byref(g), None, None, None, None, None) == ARG
    assert lib.link_center_decode(one, one, one, one, one, None, 2, 0, 8, 8, ctypes.byref(g), one, one, one, one, None) == ARG
    assert lib.link_center_decode(one, one, one, one, one, None, 2, 1, 8, 8, None, one, one, one, one, None) == ARG
    g.score_threshold = float("nan")
    assert lib.link_center_decode(one, one, one, one, one, None, 2, 1, 8, 8, ctypes.byref(g), one, one, one, one, None) == ARG


def test_nms_workspace_bytes():
    from link_amd import _lib as L
    lib = L.lib()
    for n in (1, 63, 64, 65, 130, 1000, 4097, 100000):
        assert lib.link_nms_workspace_bytes(n) == 8 * n * ((n + 63) // 64), n
    assert lib.link_nms_workspace_bytes(0) == 0 and lib.link_nms_workspace_bytes(-5) == 0


def test_fixtures_are_complete():
    assert golden_files("boxnms_pairs_*.npz") == sorted(PAIR_FILES)
    assert golden_files("boxnms_nms_*.npz") == sorted(f"boxnms_nms_{n}.npz" for n in NMS_SIZES)
    for name in PAIR_FILES + [f"boxnms_nms_{n}.npz" for n in NMS_SIZES]:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20), name
        meta = load_golden(name)["meta"]
        n = sum(int(v) for v in name.split("_")[-1].split(".")[0].split("x"))          # boxes of the set / of both sets
        assert meta["replaced"] < 0.02 * n or meta["replaced"] == 0, (name, meta["replaced"])


@pytest.mark.parametrize("name", PAIR_FILES)
def test_float32_restatement_equals_compiled_reference(name):
    """Every pair of the fixtures is a stable pair (the generator replaced a box of every other one)."""
    g = load_golden(name)
    mine = BO.pairs_matrix(BO.iou_bev, g["a"], g["b"])
    err = float(np.abs(mine.astype(np.float64) - g["iou"]).max())
    print(name, g["meta"]["source"], "max |float32 restatement - fixture| =", err, "d =", g["meta"]["d"])
    assert err <= 1e-6, err
    assert np.array_equal(mine == 0, g["iou"] == 0)
    ov = BO.pairs_matrix(BO.box_overlap, g["a"], g["b"])
    assert np.array_equal(ov, g["overlap"])
    # and the float64 restatement lies within the recorded distance d of the reference
    d64 = float(np.abs(BO.pairs_matrix(BO.iou_bev, g["a"], g["b"], dtype=np.float64) - g["iou"]).max())
    assert d64 <= g["meta"]["d"] * (1 + 1e-9) + 1e-12, (d64, g["meta"]["d"])


@pytest.mark.parametrize("n", NMS_SIZES)
def test_numpy_greedy_rule_reproduces_keep_lists(n):
    g = load_golden(f"boxnms_nms_{n}.npz")
    m = g["meta"]
    boxes, scores = g["boxes"], g["scores"]
    assert len(np.unique(scores)) == n
    order = np.argsort(-scores, kind="stable")
    s = boxes[order]
    nrm = BO.pairs_matrix(BO.iou_normal, s, s) > np.float32(m["thr"])
    assert np.array_equal(order[BO.greedy_nms(nrm)], g["keep_normal"])
    assert np.array_equal(order[BO.greedy_from_words(BO.pack_mask(nrm), n)], g["keep_normal"])     # the word form of the same rule
    dets = np.concatenate([boxes[:, :2], scores[:, None]], 1).astype(np.float32)
    assert np.array_equal(BO.circle_nms(dets, m["radius"])[:m["post"]], g["keep_circle"])
    d2 = BO.pairs_matrix(BO.centre_dist2, s, s) <= np.float32(m["radius"])
    assert np.array_equal(order[BO.greedy_nms(d2, m["post"])], g["keep_circle"])                   # circle_nms is the greedy rule too

    def rotated(bx):
        """IoU > thr over the pairs whose centres are closer than two 12 m x 12 m half diagonals (the others cannot touch)"""
        near = np.argwhere(np.hypot(bx[:, None, 0] - bx[None, :, 0], bx[:, None, 1] - bx[None, :, 1]) < 17.2)
        sup = np.zeros((len(bx), len(bx)), bool)
        if len(near):
            sup[near[:, 0], near[:, 1]] = BO.iou_bev(bx[near[:, 0]], bx[near[:, 1]]) > np.float32(m["thr"])
        return sup
    assert np.array_equal(order[BO.greedy_nms(rotated(s))], g["keep_rotate"])
    assert np.array_equal(order[BO.greedy_nms(rotated(BO.to_pcdet(s[:m["pre"]])), m["post"])], g["keep_pcdet"])
    assert np.array_equal(g["keep_rotate_pre"], g["keep_rotate"][np.isin(g["keep_rotate"], order[:m["pre"]])])


def test_boxnms_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_table
    from link_amd import build as hip_build
    hip_build.build()
    rows = kernel_table(os.path.join(ROOT, "link_amd", "lib", "obj", "boxnms.o"))
    names = [r[0] for r in rows]
    for k, count in (("k_boxes_pair", 2), ("k_nms_mask", 3), ("k_nms_reduce", 1), ("k_center_decode", 2), ("k_center_count", 1)):
        assert sum(k in nm for nm in names) == count, (k, names)
    for name, vgpr, agpr, sgpr, lds, scratch, wg in rows:
        print(name, vgpr, agpr, sgpr, lds, scratch, wg)
        assert int(scratch) == 0, (name, scratch)          # the 24-point list of the pair routine stays in registers
        assert int(wg) == 256, (name, wg)


def test_install_as_iou3d_nms():
    import link_amd as la
    la.install_as_iou3d_nms()
    try:
        from det3d.ops.iou3d_nms import iou3d_nms_cuda, iou3d_nms_utils
        import det3d.ops.iou3d_nms.iou3d_nms_cuda as direct
        assert direct is iou3d_nms_cuda is la.boxnms.iou3d_nms_cuda
        for name in ("boxes_overlap_bev_gpu", "boxes_iou_bev_gpu", "nms_gpu", "nms_normal_gpu"):
            assert callable(getattr(iou3d_nms_cuda, name)), name
        assert iou3d_nms_utils.nms_gpu is la.nms_gpu and iou3d_nms_utils.boxes_iou3d_gpu is la.boxes_iou3d_gpu
    finally:
        for k in [k for k in sys.modules if k == "det3d" or k.startswith("det3d.")]:
            del sys.modules[k]


def test_cpu_tensors_fail_loudly():
    import torch
    import link_amd as la
    from link_amd._lib import LinkAmdError
    b = torch.zeros(3, 7)
    with pytest.raises(LinkAmdError):
        la.boxes_iou_bev(b, b)
    with pytest.raises(LinkAmdError):
        la.nms_gpu(b, torch.arange(3.0), 0.2)
    with pytest.raises(NotImplementedError):
        la.CenterHeadDecoder({"double_flip": True}, [1])
