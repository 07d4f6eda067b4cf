"""CPU-only checks of the autocast-training entries (ABI 13): the 16-bit row variants of the training kernels are
declared, bound and exported, and they reject bad arguments before touching the device."""
import ctypes
import os
import re

from helpers import ROOT

NEW_ENTRIES = ("link_premix_ln_io", "link_premix_ln_backward_io", "link_ln_add_relu_forward_io", "link_ln_add_relu_backward_io",
               "link_bn_forward_stats_io", "link_bn_apply_forward_io", "link_bn_backward_reduce_io",
               "link_bn_backward_reduce_relu_io", "link_bn_apply_backward_io")


def _lib():
    from link_amd import _lib as L
    from link_amd import build as hip_build
    hip_build.build()
    return L, L.lib()


def test_new_entries_declared_bound_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    declared = set(re.findall(r"\b(link_[a-z0-9_]+)\s*\(", hdr))
    handle = ctypes.CDLL(L.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in L.SIGNATURES, name
        assert hasattr(handle, name), name
    assert L.ABI_VERSION == 13
    assert lib.link_abi_version() == 13


def test_bad_row_type_width_and_null_rejected_without_gpu():
    L, lib = _lib()
    ERR, OK = L.LINK_ERR_ARG, L.LINK_OK
    for bad in (-1, 3, 7):
        assert lib.link_premix_ln_io(None, bad, None, None, None, 10, 64, 1e-6, None, None) == ERR
        assert lib.link_premix_ln_backward_io(None, bad, None, None, None, 10, 64, 1e-6, None, None, None, None) == ERR
        assert lib.link_ln_add_relu_forward_io(None, bad, None, None, None, 10, 64, 1e-6, None, None) == ERR
        assert lib.link_ln_add_relu_backward_io(None, None, None, bad, None, 10, 64, 1e-6, None, None, None, None) == ERR
        assert lib.link_bn_forward_stats_io(None, bad, 10, 64, 1e-3, 0.1, None, None, None, None, None, None, None, None, None,
                                            None) == ERR
        assert lib.link_bn_apply_forward_io(None, bad, None, None, None, 10, 64, 0, None, None) == ERR
        assert lib.link_bn_backward_reduce_io(None, None, bad, None, None, 10, 64, None, None, None, None, None, None) == ERR
        assert lib.link_bn_backward_reduce_relu_io(None, None, bad, None, None, None, None, 10, 64, None, None, None, None, None,
                                                   None) == ERR
        assert lib.link_bn_apply_backward_io(None, None, bad, None, None, None, None, 10, 64, None, None) == ERR
    for io in (L.IO_F16, L.IO_BF16):
        # widths: the MFMA path of pre_mix (C % 16 == 0, C <= 128), C % 4 == 0 (<= 256) for the tail, 4..1024 for BatchNorm
        for c in (0, 24, 144, 256):
            assert lib.link_premix_ln_io(None, io, None, None, None, 10, c, 1e-6, None, None) == ERR, c
            assert lib.link_premix_ln_backward_io(None, io, None, None, None, 10, c, 1e-6, None, None, None, None) == ERR, c
        for c in (0, 6, 260):
            assert lib.link_ln_add_relu_forward_io(None, io, None, None, None, 10, c, 1e-6, None, None) == ERR, c
            assert lib.link_ln_add_relu_backward_io(None, None, None, io, None, 10, c, 1e-6, None, None, None, None) == ERR, c
        for c in (0, 6, 2048):
            assert lib.link_bn_forward_stats_io(None, io, 10, c, 1e-3, 0.1, None, None, None, None, None, None, None, None, None,
                                                None) == ERR, c
            assert lib.link_bn_apply_forward_io(None, io, None, None, None, 10, c, 0, None, None) == ERR, c
        # null buffers at a valid width
        assert lib.link_premix_ln_io(None, io, None, None, None, 10, 64, 1e-6, None, None) == ERR
        assert lib.link_premix_ln_backward_io(None, io, None, None, None, 10, 64, 1e-6, None, None, None, None) == ERR
        assert lib.link_ln_add_relu_forward_io(None, io, None, None, None, 10, 64, 1e-6, None, None) == ERR
        assert lib.link_ln_add_relu_backward_io(None, None, None, io, None, 10, 64, 1e-6, None, None, None, None) == ERR
        assert lib.link_bn_forward_stats_io(None, io, 10, 64, 1e-3, 0.1, None, None, None, None, None, None, None, None, None,
                                            None) == ERR
        assert lib.link_bn_apply_forward_io(None, io, None, None, None, 10, 64, 1, None, None) == ERR
        assert lib.link_bn_backward_reduce_io(None, None, io, None, None, 10, 64, None, None, None, None, None, None) == ERR
        assert lib.link_bn_backward_reduce_relu_io(None, None, io, None, None, None, None, 10, 64, None, None, None, None, None,
                                                   None) == ERR
        assert lib.link_bn_apply_backward_io(None, None, io, None, None, None, None, 10, 64, None, None) == ERR
        # empty input is a no-op (no launch)
        assert lib.link_premix_ln_io(None, io, None, None, None, 0, 64, 1e-6, None, None) == OK
        assert lib.link_premix_ln_backward_io(None, io, None, None, None, 0, 64, 1e-6, None, None, None, None) == OK
        assert lib.link_ln_add_relu_forward_io(None, io, None, None, None, 0, 64, 1e-6, None, None) == OK
