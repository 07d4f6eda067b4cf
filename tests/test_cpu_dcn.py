"""CPU checks of deformable convolution: the restatements of tests/dcn_oracle.py against each other and against F.conv2d, the CPU path
of link_amd/dcn.py against them, the modules' parameter names, and the argument checks of section R of include/link_amd.h (which are
made before anything touches a device)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_oracle as DO

CASES = [  # B, C, O, dg, H, W, kh, kw, stride, pad, dil
    (2, 8, 6, 4, 5, 7, 3, 3, 1, 1, 1),
    (1, 4, 4, 1, 6, 6, 3, 3, 2, 0, 2),
    (2, 12, 5, 3, 9, 11, 3, 1, (2, 1), (1, 0), 1),
    (1, 6, 3, 2, 4, 5, 1, 1, 1, 0, 1),
]
HEADS = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}


def _case64(case, family, seed):
    x, off, w, go, bad = DO.make_case(*case, family, seed)
    return x.double(), off.double(), w.double(), go.double(), bad


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", ["uniform", "normal"])
def test_gathered_corners_equal_grid_sample(case, family):
    x, off, w, go, _ = _case64(case, family, 3)
    kw = dict(stride=case[8], pad=case[9], dil=case[10], dg=case[3])
    a = DO.grads(DO.dcn, x, off, w, go, **kw)
    b = DO.grads(DO.dcn_grid_sample, x, off, w, go, **kw)
    for name, u, v in zip(("out", "grad_input", "grad_offset", "grad_weight"), a, b):
        assert float((u - v).abs().max()) <= 1e-12 * max(float(u.abs().max()), 1.0), name


@pytest.mark.parametrize("case", CASES)
def test_zero_offsets_are_conv2d(case):
    x, off, w, _, _ = _case64(case, "zeros", 0)
    out = DO.dcn(x, off, w, case[8], case[9], case[10], case[3])
    want = F.conv2d(x, w, None, case[8], case[9], case[10])
    assert float((out - want).abs().max()) <= 1e-13


def test_integer_offsets_are_a_shifted_conv2d():
    """A constant integer offset (dy, dx) reads x[h + dy, w + dx]: a convolution of the shifted map.  The map is zero on a rim as wide
    as the largest shift, so that the convolution's zero padding and the samples just off the shifted window agree."""
    B, C, O, H, W = 2, 4, 3, 10, 11
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    x[:, :, :3], x[:, :, -3:], x[:, :, :, :3], x[:, :, :, -3:] = 0, 0, 0, 0
    w = torch.randn(O, C, 3, 3, generator=g, dtype=torch.float64)
    for dy, dx in ((1, -2), (-3, 0), (0, 3)):
        off = torch.zeros(B, 18, H, W, dtype=torch.float64)
        off[:, 0::2], off[:, 1::2] = dy, dx
        shifted = torch.zeros_like(x)                                                # shifted[h, w] = x[h + dy, w + dx]
        hs, ws = slice(max(-dy, 0), H - max(dy, 0)), slice(max(-dx, 0), W - max(dx, 0))
        hd, wd = slice(max(dy, 0), H - max(-dy, 0)), slice(max(dx, 0), W - max(-dx, 0))
        shifted[:, :, hs, ws] = x[:, :, hd, wd]
        want = F.conv2d(shifted, w, None, 1, 1)
        assert float(want.abs().max()) > 1 and float((DO.dcn(x, off, w, 1, 1, 1, 1) - want).abs().max()) <= 1e-13


def test_gradcheck_off_the_integers():
    x, off, w, _, _ = _case64((1, 4, 3, 2, 4, 5, 3, 3, 1, 1, 1), "normal", 5)
    x.requires_grad_(True), off.requires_grad_(True), w.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: DO.dcn(a, b, c, 1, 1, 1, 2), (x, off, w), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_nonfinite_offsets_count_zero():
    case = (2, 8, 6, 4, 5, 7, 3, 3, 1, 1, 1)
    x, off, w, go, bad = _case64(case, "nonfinite", 2)
    assert bad.any() and not torch.isfinite(off[bad]).all()
    out, gx, gf, gw = DO.grads(DO.dcn, x, off, w, go, stride=1, pad=1, dil=1, dg=4)
    assert all(torch.isfinite(t).all() for t in (out, gx, gf, gw)) and not gf[bad].any()
    far = torch.where(bad, torch.full_like(off, 1e4), off)                            # far off the map: contributes 0 as well
    assert torch.equal(out, DO.dcn(x, far, w, 1, 1, 1, 4))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", ["normal", "nonfinite", "integer"])
def test_module_cpu_path_is_the_oracle(case, family):
    import link_amd as la
    x, off, w, go, _ = _case64(case, family, 7)
    kw = dict(stride=case[8], pad=case[9], dil=case[10], dg=case[3])
    want = DO.grads(DO.dcn, x, off, w, go, **kw)
    assert not la.deform_conv_native(x, off, w, case[8], case[9], case[10], 1, case[3])
    got = DO.grads(lambda a, b, c: la.deform_conv(a, b, c, case[8], case[9], case[10], 1, case[3], 64), x, off, w, go)
    for name, u, v in zip(("out", "grad_input", "grad_offset", "grad_weight"), got, want):
        assert float((u - v).abs().max()) <= 1e-12 * max(float(v.abs().max()), 1.0), name
    relu = la.deform_conv_relu(x, off, w, case[8], case[9], case[10], 1, case[3])
    assert torch.equal(relu, torch.relu(got[0]))


def test_groups_on_the_cpu_path():
    import link_amd as la
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 8, 5, 6, generator=g, dtype=torch.float64), torch.randn(6, 4, 3, 3, generator=g, dtype=torch.float64)
    off = torch.zeros(2, 2 * 18, 5, 6, dtype=torch.float64)
    assert float((la.deform_conv(x, off, w, 1, 1, 1, 2, 2) - F.conv2d(x, w, None, 1, 1, 1, 2)).abs().max()) <= 1e-13


def test_pad_path_for_a_2x2_input():
    import link_amd as la
    torch.manual_seed(0)
    m = la.DeformConv(4, 3, 3, padding=1, deformable_groups=2).double()
    x = torch.randn(1, 4, 2, 2, dtype=torch.float64)
    off = torch.randn(1, 36, 2, 2, dtype=torch.float64)
    out = m(x, off)
    assert out.shape == (1, 3, 2, 2)
    xp, op = F.pad(x, (0, 1, 0, 1)), F.pad(off, (0, 1, 0, 1))
    assert torch.equal(out, DO.dcn(xp, op, m.weight.detach(), 1, 1, 1, 2)[:, :, :2, :2])
    with pytest.raises(AssertionError):
        la.DeformConv(4, 3, 3, bias=True)
    with pytest.raises(ValueError):
        la.deform_conv(x, off[:, :34], m.weight, 1, 1, 1, 1, 2)


def test_modules_parameters_and_state_dict_names():
    import link_amd as la
    torch.manual_seed(0)
    head = la.DCNSepHead(64, 2, HEADS, head_conv=64, final_kernel=3, bn=True)
    want = ["feature_adapt_cls.conv_offset.weight", "feature_adapt_cls.conv_offset.bias", "feature_adapt_cls.conv_adaption.weight",
            "feature_adapt_reg.conv_offset.weight", "feature_adapt_reg.conv_offset.bias", "feature_adapt_reg.conv_adaption.weight",
            "cls_head.0.weight", "cls_head.0.bias", "cls_head.1.weight", "cls_head.1.bias", "cls_head.1.running_mean",
            "cls_head.1.running_var", "cls_head.1.num_batches_tracked", "cls_head.3.weight", "cls_head.3.bias"]
    for h in HEADS:
        want += [f"task_head.{h}.0.weight", f"task_head.{h}.0.bias", f"task_head.{h}.1.weight", f"task_head.{h}.1.bias",
                 f"task_head.{h}.1.running_mean", f"task_head.{h}.1.running_var", f"task_head.{h}.1.num_batches_tracked",
                 f"task_head.{h}.3.weight", f"task_head.{h}.3.bias"]
    assert list(head.state_dict().keys()) == want
    plain = la.DCNSepHead(64, 2, HEADS)
    assert [k for k in plain.state_dict() if k.startswith("task_head.reg")] == ["task_head.reg.0.weight", "task_head.reg.0.bias",
                                                                                  "task_head.reg.2.weight", "task_head.reg.2.bias"]
    other = la.DCNSepHead(64, 2, HEADS, head_conv=64, final_kernel=3, bn=True)
    other.load_state_dict({k: v.clone() for k, v in head.state_dict().items()}, strict=True)
    fa = head.feature_adapt_cls
    assert fa.conv_offset.weight.shape == (72, 64, 1, 1) and not fa.conv_offset.weight.any()
    assert fa.conv_adaption.weight.shape == (64, 64, 3, 3) and fa.conv_adaption.deformable_groups == 4
    assert float(fa.conv_adaption.weight.detach().abs().max()) <= 1 / np.sqrt(64 * 9)
    assert float(head.cls_head[-1].bias[0]) == pytest.approx(-2.19) and not head.task_head.reg[-1].bias.any()
    pack = la.DeformConvPack(8, 4, 3, padding=1, deformable_groups=2)
    assert list(pack.state_dict().keys()) == ["weight", "conv_offset.weight", "conv_offset.bias"]
    x = torch.randn(1, 8, 5, 5)
    assert float((pack(x) - F.conv2d(x, pack.weight, None, 1, 1)).abs().max()) < 1e-5
    out = head.eval()(torch.randn(1, 64, 5, 6))
    assert set(out) == set(HEADS) | {"hm"} and out["hm"].shape == (1, 2, 5, 6) and out["dim"].shape == (1, 3, 5, 6)


def _geom(**kw):
    from link_amd import _lib as L
    g = L.LinkDeformConvGeom()
    base = dict(batch=2, c=8, h=5, w=7, o=6, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, groups=1,
                deformable_groups=4, offset_channels=72, io_dtype=L.IO_F32, flags=0)
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


def test_abi_and_argument_errors():
    from link_amd import _lib as L
    lib = L.lib()
    assert lib.link_abi_version() == 13
    assert lib.link_abi_struct_size(L.STRUCT_DEFORM_CONV_GEOM) == ctypes.sizeof(L.LinkDeformConvGeom) == 72
    assert L.STRUCT_DEFORM_CONV_GEOM == 14 and lib.link_abi_struct_size(15) == -1
    p = 4096                                                                         # a non-null pointer that is never followed
    good = _geom()
    assert lib.link_deform_conv_workspace_bytes(ctypes.byref(good)) > 0
    bad = [_geom(groups=2), _geom(c=10), _geom(offset_channels=36), _geom(kh=8, kw=8, offset_channels=4 * 2 * 64), _geom(c=260, o=6),
           _geom(o=257), _geom(stride_h=0), _geom(pad_w=-1), _geom(io_dtype=7), _geom(h=1, w=1, pad_h=0, pad_w=0), _geom(flags=2),
           _geom(batch=1 << 20, h=1 << 10, w=1 << 10)]
    for g in bad:
        assert lib.link_deform_conv_workspace_bytes(ctypes.byref(g)) == 0
        assert lib.link_deform_conv_forward(ctypes.byref(g), p, p, p, p, None) == L.LINK_ERR_ARG
        assert lib.link_deform_conv_backward_data(ctypes.byref(g), p, p, p, p, p, p, p, None) == L.LINK_ERR_ARG
        assert lib.link_deform_conv_backward_weight(ctypes.byref(g), p, p, p, p, p, p, 1 << 30, None) == L.LINK_ERR_ARG
    # null pointers
    assert lib.link_deform_conv_forward(None, p, p, p, p, None) == L.LINK_ERR_ARG
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert lib.link_deform_conv_forward(ctypes.byref(good), *args, None) == L.LINK_ERR_ARG
    assert lib.link_deform_conv_backward_data(ctypes.byref(good), p, p, p, None, None, p, p, None) == L.LINK_ERR_ARG      # grad_out
    assert lib.link_deform_conv_backward_data(ctypes.byref(good), p, p, p, None, p, None, None, None) == L.LINK_ERR_ARG   # no gradient asked
    assert lib.link_deform_conv_backward_data(ctypes.byref(_geom(flags=1)), p, p, p, None, p, p, p, None) == L.LINK_ERR_ARG  # ReLU without output
    assert lib.link_deform_conv_backward_data(ctypes.byref(_geom(io_dtype=L.IO_F16)), p, p, p, p, p, p, p, None) == L.LINK_ERR_ARG
    assert lib.link_deform_conv_backward_weight(ctypes.byref(good), p, p, None, p, None, p, 1 << 30, None) == L.LINK_ERR_ARG
    assert lib.link_deform_conv_backward_weight(ctypes.byref(good), p, p, None, p, p, p, 16, None) == L.LINK_ERR_WORKSPACE
