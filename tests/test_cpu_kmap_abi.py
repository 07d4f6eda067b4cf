"""CPU-only checks of the general kernel-map builder (csrc/kmap.hip): argument validation before anything touches a device,
the candidate count, and the resource shape of its kernels read from the built code object."""
import ctypes
import os
import sys

from helpers import ROOT


def test_kmap_entries_validate_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    i3 = ctypes.c_int32 * 3
    i4 = ctypes.c_int32 * 4
    assert lib.link_kmap_candidate_count(i3(3, 3, 3), i3(2, 2, 2)) == 8
    assert lib.link_kmap_candidate_count(i3(3, 3, 1), i3(2, 2, 1)) == 4
    assert lib.link_kmap_candidate_count(i3(5, 5, 3), i3(1, 1, 1)) == 75
    assert lib.link_kmap_candidate_count(i3(7, 2, 1), i3(3, 2, 4)) == 3
    assert lib.link_kmap_candidate_count(i3(8, 3, 3), i3(2, 2, 2)) == -1          # extents 1..7
    assert lib.link_kmap_candidate_count(i3(3, 3, 3), i3(0, 2, 2)) == -1
    lo = i4(0, 0, 0, 0)
    assert lib.link_kmap_out_candidates(None, 0, i3(3, 3, 3), i3(2, 2, 2), i3(1, 1, 1), lo, None, None) == L.LINK_OK
    assert lib.link_kmap_out_candidates(None, 5, i3(3, 3, 3), i3(2, 2, 2), i3(1, 1, 1), lo, None, None) == L.LINK_ERR_ARG    # null buffers
    assert lib.link_kmap_out_candidates(None, 0, i3(3, 3, 3), i3(2, 2, 2), i3(0, 1, 1), lo, None, None) == L.LINK_ERR_ARG    # tensor stride
    assert lib.link_kmap_out_candidates(None, 0, i3(9, 3, 3), i3(2, 2, 2), i3(1, 1, 1), lo, None, None) == L.LINK_ERR_ARG
    g = L.grid_from_bounds((0, 0, 0, 0), (15, 15, 15, 0), 1)
    assert lib.link_kmap_box_table(None, 0, None, ctypes.byref(g), i3(3, 1, 3), i3(1, 1, 1), None, None) == L.LINK_OK
    assert lib.link_kmap_box_table(None, 9, None, ctypes.byref(g), i3(3, 1, 3), i3(1, 1, 1), None, None) == L.LINK_ERR_ARG
    assert lib.link_kmap_box_table(None, 0, None, ctypes.byref(g), i3(3, 0, 3), i3(1, 1, 1), None, None) == L.LINK_ERR_ARG
    assert lib.link_kmap_box_table(None, 0, None, ctypes.byref(g), i3(3, 1, 3), i3(1, 0, 1), None, None) == L.LINK_ERR_ARG
    assert lib.link_kmap_box_table(None, 0, None, ctypes.byref(L.LinkGrid()), i3(3, 1, 3), i3(1, 1, 1), None, None) == L.LINK_ERR_ARG
    assert lib.link_kmap_transpose(None, 0, 27, 0, None, None) == L.LINK_OK
    assert lib.link_kmap_transpose(None, 10, 27, 10, None, None) == L.LINK_ERR_ARG
    assert lib.link_kmap_transpose(None, 10, 0, 10, None, None) == L.LINK_ERR_ARG
    assert lib.link_kmap_transpose(None, 1 << 27, 27, 10, None, None) == L.LINK_ERR_ARG                                   # >= 2^31 entries
    assert L.ABI_VERSION == 13                           # additive entries: the ABI version does not move


def test_kmap_kernels_resource_shape():
    """Index kernels, one lane per element: no scratch, no LDS, no accumulation registers, 256-lane workgroups."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_table
    from link_amd import build as hip_build
    hip_build.build()
    rows = [r for r in kernel_table(os.path.join(ROOT, "link_amd", "lib", "obj", "kmap.o")) if "k_kmap" in r[0]]
    assert len(rows) == 3, [r[0] for r in rows]
    for name, vgpr, agpr, sgpr, lds, scratch, wg in rows:
        print(name, vgpr, agpr, sgpr, lds, scratch, wg)
        assert int(scratch) == 0 and int(lds) == 0 and int(agpr) == 0 and int(wg) == 256, (name, scratch, lds, agpr, wg)
        assert int(vgpr) <= 64, (name, vgpr)             # full occupancy: eight waves per SIMD
