"""CPU-only checks of the CenterHead test-time augmentation (csrc/dettta.hip, section N of include/link_amd.h; link_amd/dettta.py): the
restatements of tests/tta_oracle.py against the fixtures recorded from the reference's own functions (tests/golden/
make_golden_dettta.py), exports and prototypes, argument validation before anything touches a device, loud failure on CPU tensors,
and that CenterHeadDecoder still refuses the flags the new decoder takes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, golden_files, load_golden

import tta_oracle as TO

SECTION_N = ("link_tta_views", "link_center_decode_flip4", "link_nms_mask_classwise", "link_tta_rotate_back")
FUSE_CASES = [(0, 1, 2), (1, 1, 2), (64, 3, 2), (65, 3, 3), (1000, 10, 3), (1000, 3, 2)]
FUSE_FILES = [f"dettta_fuse_{n}_c{c}_p{p}.npz" for n, c, p in FUSE_CASES]
CFG = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 83,
                                                                                      "nms_iou_threshold": 0.2},
       "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075]}


def test_fixtures_are_complete():
    assert golden_files("dettta_*.npz") == sorted(FUSE_FILES + ["dettta_views.npz", "dettta_predict_rot0.npz", "dettta_predict_rot1.npz"])
    for name in golden_files("dettta_*.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20), name
    for (n, c, p), name in zip(FUSE_CASES, FUSE_FILES):
        g = load_golden(name)
        m = g["meta"]
        assert m["replaced"] < 0.02 * n or m["replaced"] == 0, (name, m["replaced"])          # the 2 % cap of the stabilisation
        assert g["boxes"].shape == (n, 9) and len(np.unique(g["scores"])) == n and len(m["thresholds"]) == c and len(m["split"]) == p - 1
        assert (g["labels"] >= 0).all() and (g["labels"] < c).all() and m["kept"] == len(g["keep"])


def test_views_restatement_equals_the_reference_rotation():
    g = load_golden("dettta_views.npz")
    m = g["meta"]
    clouds = [g[f"points{i}"] for i in range(m["clouds"])]
    v32, v64 = TO.views(clouds, m["angle"], np.float32), TO.views(clouds, m["angle"], np.float64)
    assert len(v32) == 4 * m["clouds"]
    for i, src in enumerate(clouds):
        want = g[f"rotated{i}"]
        p, y, x, d = v32[4 * i:4 * i + 4]
        # one fp32 ulp of the largest coordinate: the reference's product is a matrix multiplication, whose sum may be fused
        ulp = np.spacing(np.float32(np.abs(src[:, :2]).max())) if len(src) else 0.0
        assert np.abs(p.astype(np.float64) - want).max(initial=0.0) <= ulp, (m["source"], i)
        assert np.abs(v64[4 * i] - want).max(initial=0.0) <= 2 * ulp
        assert np.array_equal(p[:, 2:], src[:, 2:])
        assert np.array_equal(y, p * np.float32([1, -1, 1, 1, 1])) and np.array_equal(x, p * np.float32([-1, 1, 1, 1, 1]))
        assert np.array_equal(d, p * np.float32([-1, -1, 1, 1, 1]))
    same = TO.views(clouds, 0.0)
    assert all(np.array_equal(same[4 * i], c) for i, c in enumerate(clouds))


@pytest.mark.parametrize("rot", [0, 1])
def test_predict_restatement_equals_the_reference_head(rot):
    g = load_golden(f"dettta_predict_rot{rot}.npz")
    m = g["meta"]
    preds = [{k[len(f"t{t}_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"t{t}_")} for t in range(len(m["num_classes"]))]
    out = TO.predict(preds, m["cfg"], m["num_classes"])
    assert len(out) == m["frames"] and sum(m["kept"]) > 0
    for b, r in enumerate(out):
        print(m["source"], "frame", b, "kept", len(r["scores"]))
        assert np.array_equal(r["label_preds"], g[f"f{b}_label_preds"])
        assert np.allclose(r["scores"], g[f"f{b}_scores"], rtol=1e-6, atol=0)
        assert r["box3d_lidar"].shape == g[f"f{b}_box3d_lidar"].shape == (m["kept"][b], 9)
        assert np.allclose(r["box3d_lidar"], g[f"f{b}_box3d_lidar"], rtol=2e-6, atol=2e-6)
    # and the float64 form decides alike on these maps
    out64 = TO.predict(preds, m["cfg"], m["num_classes"], torch.float64)
    for r, r64 in zip(out, out64):
        assert np.array_equal(r["label_preds"], r64["label_preds"]) and np.allclose(r["box3d_lidar"], r64["box3d_lidar"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", FUSE_FILES)
def test_classwise_rule_reproduces_the_keep_lists(name):
    g = load_golden(name)
    keep = TO.classwise_nms(g["boxes"], g["scores"], g["labels"], g["meta"]["thresholds"], max_dets=len(g["scores"]) + 1)
    assert np.array_equal(keep, g["keep"])
    assert np.array_equal(TO.classwise_nms(g["boxes"], g["scores"], g["labels"], g["meta"]["thresholds"], max_dets=3), g["keep"][:3])


def test_decode_restatement_leaves_its_inputs_alone():
    pd = {"hm": torch.randn(4, 1, 3, 5), "reg": torch.rand(4, 2, 3, 5), "height": torch.randn(4, 1, 3, 5), "dim": torch.randn(4, 3, 3, 5),
          "rot": torch.randn(4, 2, 3, 5), "vel": torch.randn(4, 2, 3, 5)}
    before = {k: v.clone() for k, v in pd.items()}
    boxes, labels, scores, mask, hm = TO.decode(pd, CFG)
    assert boxes.shape == (1, 15, 9) and all(torch.equal(pd[k], before[k]) for k in pd)
    # a frame whose four views are flips of one map decodes to that map's single-view values
    one = {k: v[:1] for k, v in pd.items()}
    sym = {k: torch.cat([one[k], one[k].flip(2), one[k].flip(3), one[k].flip(2, 3)]) for k in one}
    sym["reg"][1, 1] = 1 - sym["reg"][1, 1]; sym["reg"][2, 0] = 1 - sym["reg"][2, 0]; sym["reg"][3] = 1 - sym["reg"][3]
    sym["rot"][1, 1] *= -1; sym["rot"][2, 0] *= -1; sym["rot"][3] *= -1
    sym["vel"][1, 1] *= -1; sym["vel"][2, 0] *= -1; sym["vel"][3] *= -1
    b4 = TO.decode(sym, CFG, torch.float64)[0]
    hm1 = torch.sigmoid(one["hm"].double())
    assert torch.allclose(TO.decode(sym, CFG, torch.float64)[2].reshape(3, 5), hm1[0, 0], atol=1e-12)
    assert torch.allclose(b4[0, :, 2].reshape(3, 5), one["height"][0, 0].double(), atol=1e-6)
    assert torch.allclose(b4[0, :, -1].reshape(3, 5), torch.atan2(one["rot"][0, 0], one["rot"][0, 1]).double(), atol=1e-6)


def test_section_n_symbols_exported_and_prototyped():
    from link_amd import _lib as L
    from link_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in SECTION_N:
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13      # additive entries
    assert L.lib().link_abi_struct_size(99) == -1 and L.lib().link_abi_struct_size(10) == -1          # no new struct
    assert "dettta.hip" in SOURCES
    import link_amd as la
    for name in ("tta_views", "CenterHeadTTADecoder", "fuse_detections", "fuse_detections_padded"):
        assert callable(getattr(la, name)), name


def test_section_n_validates_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    OK, ARG = L.LINK_OK, L.LINK_ERR_ARG
    one = ctypes.c_void_p(64)                                            # a non-null pointer nothing dereferences
    assert lib.link_tta_views(None, None, 1, 0, 4, 1.0, 0.0, None, None, None) == ARG          # the offsets are always needed
    assert lib.link_tta_views(None, one, 1, 5, 4, 1.0, 0.0, None, one, None) == ARG
    assert lib.link_tta_views(one, one, 0, 5, 4, 1.0, 0.0, one, one, None) == ARG
    assert lib.link_tta_views(one, one, 1, 5, 2, 1.0, 0.0, one, one, None) == ARG
    assert lib.link_tta_views(one, one, 1, 5, 17, 1.0, 0.0, one, one, None) == ARG
    assert lib.link_tta_views(one, one, 1, 1 << 29, 4, 1.0, 0.0, one, one, None) == ARG
    assert lib.link_tta_views(one, one, 1, 5, 4, float("nan"), 0.0, one, one, None) == ARG
    g = L.LinkCenterGeom()
    dec = lib.link_center_decode_flip4
    assert dec(None, None, None, None, None, None, 0, 1, 8, 8, ctypes.byref(g), None, None, None, None, None) == OK
    assert dec(None, None, None, None, None, None, 2, 1, 8, 8, ctypes.byref(g), None, None, None, None, None) == ARG
    assert dec(one, one, one, one, one, None, 2, 0, 8, 8, ctypes.byref(g), one, one, one, one, None) == ARG
    assert dec(one, one, one, one, one, None, 2, 1, 8, 8, None, one, one, one, one, None) == ARG
    assert dec(one, one, one, one, one, None, 16384, 1, 8, 8, ctypes.byref(g), one, one, one, one, None) == ARG   # 4 frames > 65535
    assert dec(one, one, one, one, one, None, 2, 1, 4096, 4096, ctypes.byref(g), one, one, one, one, None) == ARG  # h w >= 2^24
    g.pc_range[0] = float("inf")
    assert dec(one, one, one, one, one, None, 2, 1, 8, 8, ctypes.byref(g), one, one, one, one, None) == ARG
    assert lib.link_nms_mask_classwise(None, None, 0, None, None, 3, None, None) == OK
    assert lib.link_nms_mask_classwise(None, None, 10, None, None, 3, None, None) == ARG
    assert lib.link_nms_mask_classwise(one, one, 10, None, one, 0, one, None) == ARG
    assert lib.link_nms_mask_classwise(one, one, -1, None, one, 3, one, None) == ARG
    assert lib.link_nms_mask_classwise(one, one, 65535 * 16 + 1, None, one, 3, one, None) == ARG
    assert lib.link_tta_rotate_back(None, 0, 7, None, 0, 1.0, 0.0, 0.0, None, None) == OK
    assert lib.link_tta_rotate_back(one, 5, 8, None, 5, 1.0, 0.0, 0.0, one, None) == ARG         # 7 or 9 columns
    assert lib.link_tta_rotate_back(one, 5, 9, None, 5, 1.0, 0.0, float("nan"), one, None) == ARG
    assert lib.link_tta_rotate_back(None, 5, 9, None, 5, 1.0, 0.0, 0.3, one, None) == ARG
    assert lib.link_tta_rotate_back(one, 5, 9, None, 5, 1.0, 0.0, 0.3, None, None) == ARG


def test_dettta_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_table
    from link_amd import build as hip_build
    hip_build.build()
    rows = kernel_table(os.path.join(ROOT, "link_amd", "lib", "obj", "dettta.o"))
    names = [r[0] for r in rows]
    for k, count in (("k_tta_views", 2), ("k_center_decode_flip4", 2), ("k_tta_count", 1), ("k_nms_mask_classwise", 1), ("k_tta_rotate_back", 4)):
        assert sum(k in nm for nm in names) == count, (k, names)
    for name, vgpr, agpr, sgpr, lds, scratch, wg in rows:
        print(name, vgpr, agpr, sgpr, lds, scratch, wg)
        assert int(scratch) == 0, (name, scratch)
        assert int(wg) == 256, (name, wg)


def test_cpu_tensors_and_bad_batches_fail_loudly():
    import link_amd as la
    from link_amd._lib import LinkAmdError
    with pytest.raises(LinkAmdError):
        la.tta_views([torch.zeros(3, 4)])
    with pytest.raises(LinkAmdError):
        la.tta_views(torch.zeros(3, 4), 0.3925)
    dec = la.CenterHeadTTADecoder(dict(CFG, double_flip=True, tt_rotation=0.3925), [1])
    assert dec.tt_rotation == 0.3925
    maps = lambda n: {"hm": torch.zeros(n, 1, 4, 4), "reg": torch.zeros(n, 2, 4, 4), "height": torch.zeros(n, 1, 4, 4),    # noqa: E731
                      "dim": torch.zeros(n, 3, 4, 4), "rot": torch.zeros(n, 2, 4, 4)}
    with pytest.raises(LinkAmdError):
        dec.decode(maps(4))
    for n in (1, 6):
        with pytest.raises(ValueError):
            dec.decode(maps(n))                                          # not four views per frame
        with pytest.raises(ValueError):
            dec.predict_padded([maps(n)])
    one = {"box3d_lidar": torch.zeros(3, 9), "scores": torch.arange(3.0), "label_preds": torch.zeros(3, dtype=torch.int64)}
    with pytest.raises(LinkAmdError):
        la.fuse_detections([one, one], [0.1])
    with pytest.raises(LinkAmdError):
        la.fuse_detections_padded(one["box3d_lidar"], one["scores"], one["label_preds"], [0.1])


def test_which_decoder_takes_which_flags():
    import link_amd as la
    for flags in ({"double_flip": True}, {"tt_rotation": 0.3925}, {"per_class_nms": True}):
        with pytest.raises(NotImplementedError):
            la.CenterHeadDecoder(dict(CFG, **flags), [1])                # the single-view decoder is unchanged
    la.CenterHeadDecoder(CFG, [1])
    with pytest.raises(ValueError):
        la.CenterHeadTTADecoder(CFG, [1])                                # double_flip must be true here
    with pytest.raises(NotImplementedError):
        la.CenterHeadTTADecoder(dict(CFG, double_flip=True, per_class_nms=True), [1])
    dec = la.CenterHeadTTADecoder(dict(CFG, double_flip=True), [1, 2])
    assert dec.tt_rotation == 0 and dec.num_classes == [1, 2] and isinstance(dec, la.CenterHeadDecoder)


def test_nothing_new_is_registered_under_the_reference_names():
    import link_amd as la
    la.install_as_iou3d_nms()
    try:
        from det3d.ops.iou3d_nms import iou3d_nms_utils
        for name in ("fuse_detections", "tta_views", "CenterHeadTTADecoder"):
            assert not hasattr(iou3d_nms_utils, name), name
    finally:
        for k in [k for k in sys.modules if k == "det3d" or k.startswith("det3d.")]:
            del sys.modules[k]
