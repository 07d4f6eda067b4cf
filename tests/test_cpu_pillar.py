"""CPU-only checks of the PointPillars reader (csrc/pillar.hip, section S of include/link_amd.h; link_amd/pillar.py): the restatement of
tests/pillar_oracle.py against the recordings of the reference's own classes (tests/golden/pillar_*.npz, made by
tools/make_pillar_golden.py), the reference's padded-row behaviour, the module surface, the native-range table and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import link_amd.pillar as LP
import pillar_oracle as PO
from link_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = PO.golden_files()
IDS = [os.path.basename(f)[7:-4] for f in FILES]


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def test_the_recordings_cover_what_they_must():
    zs = [PO.load_golden(f) for f in FILES]
    assert len(zs) >= 6
    assert {len(z["cfg"]["num_filters"]) for z in zs} == {1, 2}
    assert {z["cfg"]["with_distance"] for z in zs} == {False, True}
    assert {z["cfg"]["D"] for z in zs} >= {4, 5} and {z["cfg"]["T"] for z in zs} >= {5, 20}
    assert any(z["train"] for z in zs) and any(z["features"].shape[0] == 1 for z in zs)
    for f in FILES:
        assert os.path.getsize(f) < (1 << 20), f                                       # the cap of every committed file
    # arrays and settings only
    for f in FILES:
        assert all(v.dtype.kind in "fiub" for v in np.load(f).values()), f


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_oracle_reproduces_the_reference(path):
    z = PO.load_golden(path)
    cfg, B, ny, nx = z["cfg"], z["B"], z["ny"], z["nx"]
    for tag, dt, tol in (("64", torch.float64, 1e-12), ("32", torch.float32, 2e-5)):
        sd = PO.cast_sd(z["sd"], dt)
        for v in sd.values():
            v.requires_grad_(v.is_floating_point() and z["train"])
        new = {}
        rows = PO.reader(z["features"].to(dt), z["num"], z["coors"], sd, cfg, training=z["train"], new_stats=new)
        canvas = PO.scatter(rows, z["coors"], B, ny, nx)
        assert rows.dtype == dt and rel(rows, z["rows" + tag]) <= tol, (tag, rel(rows, z["rows" + tag]))
        assert rel(canvas, z["canvas" + tag]) <= tol
        assert torch.equal(canvas == 0, z["canvas" + tag] == 0)                        # the zero pattern, exactly
        if z["train"]:
            (canvas * z["g"].to(dt)).sum().backward()
            for k in (k for k in z if k.startswith(f"grad{tag}.")):
                name = k.split(".", 1)[1]
                assert rel(sd[name].grad, z[k]) <= tol * 100, (k, rel(sd[name].grad, z[k]))   # a gradient: sums of P T terms
            keys = [k for k in z if k.startswith(f"new{tag}.")]
            assert len(keys) == 3 * len(cfg["num_filters"])
            for k in keys:
                name = k.split(".", 1)[1]
                if "num_batches" in k:
                    assert int(new[name]) == int(z[k]) == int(z["sd"][name]) + 1
                else:
                    assert rel(new[name], z[k]) <= tol, k


@pytest.mark.parametrize("path", [f for f in FILES if "train" not in f], ids=[i for i in IDS if "train" not in i])
def test_padded_rows_take_part_in_the_max_and_can_be_evaluated_once(path):
    z = PO.load_golden(path)
    x, sd = z["features"].double(), PO.cast_sd(z["sd"], torch.float64)
    full = PO.reader(x, z["num"], z["coors"], sd, z["cfg"])
    valid = PO.reader(x, z["num"], z["coors"], sd, z["cfg"], rows="valid")
    compact = PO.reader(x, z["num"], z["coors"], sd, z["cfg"], rows="compact")
    assert (z["num"] < z["cfg"]["T"]).any()
    assert rel(valid, z["rows64"]) > 1e-3, "a max over the valid rows alone must NOT reproduce the reference"
    assert rel(compact, full) <= 1e-13 and rel(compact, z["rows64"]) <= 1e-12


def test_reference_squeezes_one_pillar_and_the_module_does_not():
    z = PO.load_golden(os.path.join(PO.GOLDEN, "pillar_l2_p1.npz"))
    assert z["rows_squeezed_shape"].tolist() == [64]
    m = _module(z)
    out = m(z["features"], z["num"], z["coors"])
    assert out.shape == (1, 64) and rel(out, z["rows32"]) <= 2e-5


def _module(z, dt=torch.float32):
    cfg = z["cfg"]
    m = LP.PillarFeatureNet(cfg["D"], cfg["num_filters"], cfg["with_distance"], cfg["voxel_size"], cfg["pc_range"])
    m.load_state_dict(z["sd"], strict=True)
    return m.to(dt).train(z["train"])


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_module_composition_on_the_cpu_and_state_dict_names(path):
    """what runs outside the native range: the torch composition, here on CPU tensors in float64 and float32"""
    z = PO.load_golden(path)
    cfg = z["cfg"]
    m = _module(z, torch.float64)
    want = set()
    for i in range(len(cfg["num_filters"])):
        want |= {f"pfn_layers.{i}.linear.weight"} | {f"pfn_layers.{i}.norm.{k}" for k in
                                                     ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(m.state_dict()) == want == set(z["sd"])
    assert not LP.pillar_native(m, z["features"].double())
    rows = m(z["features"].double(), z["num"], z["coors"])
    assert rel(rows, z["rows64"]) <= 1e-12
    scat = LP.PointPillarsScatter(cfg["num_filters"][-1])
    canvas = scat(rows, z["coors"], z["B"], (z["nx"], z["ny"], 1))
    assert canvas.shape == z["canvas64"].shape and rel(canvas, z["canvas64"]) <= 1e-12 and torch.equal(canvas == 0, z["canvas64"] == 0)
    if z["train"]:
        for k in (k for k in z if k.startswith("new64.") and "num_batches" not in k):
            assert rel(m.state_dict()[k.split(".", 1)[1]], z[k]) <= 1e-12
    # count: rows at or past it are zero rows and write nothing
    P = rows.shape[0]
    if P > 2 and not z["train"]:
        count = torch.tensor([P - 2], dtype=torch.int32)
        part = m(z["features"].double(), z["num"], z["coors"], count=count)
        assert torch.equal(part[:P - 2], rows[:P - 2]) and not part[P - 2:].any()
        c2 = LP.PillarReader(m, scat)(z["features"].double(), z["num"], z["coors"], z["B"], (z["nx"], z["ny"], 1), count=count)
        assert torch.equal(c2, PO.scatter(rows[:P - 2], z["coors"][:P - 2], z["B"], z["ny"], z["nx"]))


def test_virtual_raises_and_zero_points_give_no_nan():
    with pytest.raises(NotImplementedError):
        LP.PillarFeatureNet(virtual=True)
    z = PO.load_golden(os.path.join(PO.GOLDEN, "pillar_l2.npz"))
    m = _module(z)
    num = z["num"].clone()
    num[3] = 0
    x = z["features"].clone()
    x[3] = 0
    out = m(x, num, z["coors"])
    assert torch.isfinite(out).all()
    assert not torch.isfinite(PO.reader(x, num, z["coors"], z["sd"], z["cfg"])[3]).any()      # the reference: 0 / 0


def test_native_range_table():
    ok = LP.pillar_config_native
    for filters in ((64,), (64, 64), (16,), (32, 128), (128, 64), (128, 128), (16, 16)):
        assert ok(5, 20, filters), filters
    for filters in ((), (64, 64, 64), (8,), (144,), (24,), (64, 72), (256,)):
        assert not ok(5, 20, filters), filters
    assert [ok(d, 20, (64,)) for d in (2, 3, 8, 9)] == [False, True, True, False]
    assert [ok(5, t, (64, 64)) for t in (0, 1, 64, 65)] == [False, True, True, False]
    assert not ok(5, 20, (64, 64), virtual=True)
    m = LP.PillarFeatureNet(5, (64, 64)).eval()
    assert not LP.pillar_native(m, torch.zeros(3, 20, 5))                               # a CPU tensor


def test_abi_entries_and_version():
    from link_amd.build import SOURCES
    assert "pillar.hip" in SOURCES
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    names = ["link_pillar_native", "link_pillar_reader", "link_pillar_scatter", "link_pillar_gather", "link_pillar_decorate"]
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr) and n in L.SIGNATURES and hasattr(L.lib(), n), n
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13
    assert "Mean contract" in hdr and "pillar_encoder.py:116-162" in hdr
    assert ctypes.sizeof(L.LinkPillarGeom) == 15 * 4
    assert (L.PILLAR_MAX_T, L.PILLAR_MAX_D, L.PILLAR_MAX_WIDTH) == tuple(
        int(re.search(r"#define LINK_PILLAR_%s (\d+)" % k, hdr).group(1)) for k in ("MAX_T", "MAX_D", "MAX_WIDTH"))
    # a geometry of another size is refused before anything touches a device
    g = LP._geom(20, 5, False, (64, 64))
    assert L.lib().link_pillar_native(ctypes.byref(g)) == 1
    g.struct_bytes -= 4
    assert L.lib().link_pillar_native(ctypes.byref(g)) == 0
    assert L.lib().link_pillar_scatter(ctypes.byref(g), None, None, 0, 64, None, None, None) == L.LINK_ERR_ARG
    # sizes no grid holds are refused as arguments, not at the launch (the pointers are never touched: 1 stands for non-null)
    g = LP._geom(batch=1, ny=4, nx=4)
    for entry in (L.lib().link_pillar_scatter, L.lib().link_pillar_gather):
        assert entry(ctypes.byref(g), 1, 1, 1 << 31, 1 << 8, None, 1, None) == L.LINK_ERR_ARG
        assert entry(ctypes.byref(g), 1, 1, (1 << 31) + 1, 1, None, 1, None) == L.LINK_ERR_ARG


def test_out_dtype_and_parameter_device_are_checked():
    m = LP.PillarFeatureNet(5, (64, 64)).eval()
    x, num, coors = torch.zeros(3, 20, 5), torch.ones(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(TypeError):
        m(x, num, coors, out_dtype=torch.float64)
    assert m(x, num, coors, out_dtype=torch.bfloat16).dtype == torch.bfloat16
