"""CPU-only checks of the segmentation criterion (csrc/segloss.hip, section K of include/link_amd.h; link_amd/segloss.py): the
float64 oracle of tests/segloss_oracle.py against every fixture recorded from the reference's own lovasz_losses.py and
nn.CrossEntropyLoss (tests/golden/make_golden_segloss.py), the closed form of lovasz_grad, the cap of the ambiguity mask, the torch
composition link_amd.segloss runs off the GPU, exports and prototypes, and argument validation before anything touches a device.

test_closed_form_equals_jaccard_differences and test_mask_cap_of_the_gpu_cases check the arbiter itself (tests/segloss_oracle.py):
they need nothing of link_amd and pass without the feature; every other test here fails without it.

Measured when the fixtures were recorded (oracle in float64 against the reference in fp32, every fixture and `classes`): the loss
agrees to 6.6e-8 relative (bound 1e-6); the gradient to 1.95e-5 of max|g| (bound 2e-4) -- that is what the reference's fp32
lovasz_grad, a difference of two nearly equal Jaccard values, costs; the oracle's own fp32 evaluation of the closed form costs
3.3e-6 at most.  The mask takes 0.27 % of rows at (3000, 19) ignore 0, 0.47 % with ignore None, 0.30 % at (3000, 17), 0.26 % /
1.03 % at (777, 5)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, golden_files, load_golden, rel_err

import segloss_oracle as SO

FLAT = [f"segloss_{n}x{C}_ign{ig}.npz" for n, C in ((3000, 19), (3000, 17), (777, 5)) for ig in (0, "None")]


def test_fixtures_are_complete():
    assert golden_files("segloss_*.npz") == sorted(FLAT + ["segloss_4d.npz"])
    for name in golden_files("segloss_*.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20), name
    g = load_golden(FLAT[0])
    x, y = SO.make_case(3000, 19, g["meta"]["seed"])
    assert np.array_equal(x.numpy(), g["logits"]) and np.array_equal(y.numpy(), g["labels"])
    counts = np.bincount(g["labels"][g["labels"] < 19], minlength=19)
    assert counts[18] == 0 and counts[17] == 1 and counts[0] > counts[1] > counts[2] and (g["labels"] == 255).sum() > 60


@pytest.mark.parametrize("n,nfg,seed", [(1, 1, 0), (1, 0, 0), (2, 1, 0), (50, 0, 1), (50, 50, 2), (50, 7, 3), (3000, 1, 4), (3000, 400, 5)])
def test_closed_form_equals_jaccard_differences(n, nfg, seed):
    fg = torch.zeros(n, dtype=torch.bool)
    fg[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:nfg]] = True
    a, b = SO.closed_form_g(fg), SO.jaccard_g(fg)
    assert float((a - b).abs().max()) <= 1e-12
    assert abs(float(a.sum()) - 1.0) <= 1e-12                        # the differences telescope to the last Jaccard value: 1


@pytest.mark.parametrize("name", FLAT)
def test_oracle_reproduces_the_reference(name):
    g = load_golden(name)
    m = g["meta"]
    x, y = torch.from_numpy(g["logits"]), torch.from_numpy(g["labels"])
    mask = SO.ambiguous_rows(x, y, m["ignore"])
    assert float(mask.float().mean()) <= SO.MASK_CAP
    keep = (~mask).numpy()
    for classes in ("present", "all"):
        r = SO.reference(x, y, lov_ignore=m["ignore"], classes=classes)
        ref_total = m[classes]["ce"] + m[classes]["lovasz"]
        print(name, classes, "loss", abs(float(r["total"]) - ref_total) / ref_total, "grad", rel_err(g[f"grad_{classes}"][keep], r["grad"].numpy()[keep]))
        assert abs(float(r["total"]) - ref_total) <= 1e-6 * ref_total
        assert abs(float(r["ce"]) - m[classes]["ce"]) <= 1e-6 * m[classes]["ce"]
        assert abs(float(r["lovasz"]) - m[classes]["lovasz"]) <= 1e-6 * ref_total
        assert rel_err(g[f"grad_{classes}"][keep], r["grad"].numpy()[keep]) <= 2e-4


def _flat4d(p):
    return p.permute(0, 2, 3, 1).reshape(-1, p.shape[1])


def test_oracle_reproduces_the_reference_4d():
    g = load_golden("segloss_4d.npz")
    p, y = torch.from_numpy(g["probas"]), torch.from_numpy(g["labels"])
    r = SO.reference(_flat4d(p), y.reshape(-1), lov_ignore=0, kind="probas")
    assert abs(float(r["lovasz"]) - g["meta"]["per_image_False"]) <= 1e-6
    got = r["grad"].reshape(2, 12, 16, 5).permute(0, 3, 1, 2).numpy()
    assert rel_err(g["grad_per_image_False"], got) <= 2e-4
    per = [SO.reference(_flat4d(p[b:b + 1]), y[b].reshape(-1), lov_ignore=0, kind="probas") for b in range(2)]
    assert abs(sum(float(q["lovasz"]) for q in per) / 2 - g["meta"]["per_image_True"]) <= 1e-6


SWEEP = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (n, C, scale, row type, lovasz ignore) of every gated case of tests/test_gpu_segloss.py (`classes` does not enter the mask)
GPU_MASK_CASES = [(n, 3, 3.0, F32, 0) for n in SWEEP] + [(n, 3, 3.0, F32, None) for n in SWEEP if n <= 65] + \
                 [(777, 5, 3.0, F32, 0), (777, 5, 3.0, F32, None), (20011, 19, 2.0, F32, 0)] + \
                 [(3000, C, 3.0, d, 0) for C in (19, 17) for d in (F32, F16, BF16)]


@pytest.mark.parametrize("n,C,scale,dtype,ignore", GPU_MASK_CASES)
def test_mask_cap_of_the_gpu_cases(n, C, scale, dtype, ignore):
    x, y = SO.make_case(n, C, 1, scale)
    assert float(SO.ambiguous_rows(x.to(dtype), y, ignore).float().mean()) <= SO.MASK_CAP


@pytest.mark.parametrize("n,C,ignore,classes", [(777, 5, 0, "present"), (777, 5, None, "all"), (3000, 19, 0, "present"), (3000, 19, 0, "all"),
                                                (300, 40, 0, "present"), (64, 3, 0, "present")])
def test_torch_composition_equals_the_oracle(n, C, ignore, classes):
    """The project's gate (tests/grad64.py): rel_err(got, g64) <= 4 * o32 + 2e-6 with o32 the oracle's own fp32 evaluation; in
    float64 the composition is the oracle's formula in another operation order: 1e-12."""
    import link_amd as la
    from link_amd.segloss import _torch_lovasz_flat
    x, y = SO.make_case(n, C, 1)
    r64, o32, mask = SO.yardstick(("cpu", n, C, ignore, classes), x, y, lov_ignore=ignore, classes=classes)
    keep = (~mask).numpy()
    xx = x.double().requires_grad_(True)                             # the module widens to fp32 (autocast's rule): the formula itself
    lov = _torch_lovasz_flat(torch.softmax(xx, 1), y, classes, ignore)
    total = torch.nn.functional.cross_entropy(xx, y, ignore_index=255) + lov
    total.backward()
    assert rel_err(float(total.detach()), float(r64["total"])) <= 1e-12 and rel_err(float(lov.detach()), float(r64["lovasz"])) <= 1e-12
    assert rel_err(xx.grad.numpy(), r64["grad"].numpy()) <= 1e-12     # exact ties aside, float64 orders as the oracle does: no mask
    xx = x.clone().requires_grad_(True)
    crit = la.SegCriterion(lovasz_ignore=ignore, classes=classes)
    total = crit(xx, y)
    total.backward()
    got = {"total": total.detach(), "ce": crit.last_ce, "lovasz": crit.last_lovasz}
    for k in got:
        assert got[k].dtype == torch.float32 and rel_err(float(got[k]), float(r64[k])) <= 4 * o32[k] + 2e-6, k
    assert rel_err(xx.grad.numpy()[keep], r64["grad"].numpy()[keep]) <= 4 * o32["grad"] + 2e-6


def test_torch_composition_edges_and_the_reference_signatures():
    import link_amd as la
    x, y = SO.make_case(200, 5, 2)
    for labels in (torch.zeros(200, dtype=torch.int64), torch.full((200,), 255)):
        xx = x.clone().requires_grad_(True)
        crit = la.SegCriterion(lovasz_ignore=0 if labels[0] == 0 else None)
        total = crit(xx, labels)
        assert float(crit.last_lovasz) == 0.0
        if labels[0] == 0:
            total.backward()
            ce = torch.nn.functional.cross_entropy(x.clone().requires_grad_(True), labels)
            assert abs(float(total.detach()) - float(ce.detach())) < 1e-6
        else:
            assert not np.isfinite(float(total))                     # CE over no row: 0 / 0, as torch returns it
    # exact ties: stable in row order
    xt = torch.zeros(64, 2)
    xt[32:] = SO.make_case(32, 2, 3)[0]
    yt = (torch.arange(64) % 2).long()
    r = SO.reference(xt, yt, lov_ignore=None)
    xx = xt.clone().requires_grad_(True)
    la.SegCriterion(lovasz_ignore=None)(xx, yt).backward()
    assert rel_err(xx.grad.numpy(), r["grad"].float().numpy()) <= 2e-6
    # the reference's signatures on the 4-D fixture
    g = load_golden("segloss_4d.npz")
    p, lab = torch.from_numpy(g["probas"]).requires_grad_(True), torch.from_numpy(g["labels"])
    loss = la.lovasz_softmax(p, lab, ignore=0)
    loss.backward()
    assert abs(float(loss) - g["meta"]["per_image_False"]) <= 1e-6 and rel_err(p.grad.numpy(), g["grad_per_image_False"]) <= 2e-4
    p2 = torch.from_numpy(g["probas"]).requires_grad_(True)
    loss = la.lovasz_softmax(p2, lab, per_image=True, ignore=0)
    loss.backward()
    assert abs(float(loss) - g["meta"]["per_image_True"]) <= 1e-6 and rel_err(p2.grad.numpy(), g["grad_per_image_True"]) <= 2e-4
    p5 = torch.from_numpy(g["probas"]).reshape(2, 5, 3, 4, 16)
    assert abs(float(la.lovasz_softmax(p5, lab.reshape(2, 3, 4, 16), ignore=0)) - g["meta"]["per_image_False"]) <= 1e-6
    flat = _flat4d(torch.from_numpy(g["probas"]))
    assert float(la.lovasz_softmax_flat(flat, lab.reshape(-1))) > 0


def test_section_k_symbols_and_version():
    from link_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "link_amd.h")).read()
    handle = ctypes.CDLL(L.SO_PATH)
    for name in ("link_segloss_workspace_bytes", "link_segloss_forward", "link_segloss_backward"):
        assert name + "(" in hdr and name in L.SIGNATURES and hasattr(handle, name), name
    assert L.ABI_VERSION == 13 and L.lib().link_abi_version() == 13                  # additive entries
    assert "K. Segmentation criterion" in hdr
    for k, v in (("LINK_SEGLOSS_LOGITS", L.SEGLOSS_LOGITS), ("LINK_SEGLOSS_PROBAS", L.SEGLOSS_PROBAS), ("LINK_SEGLOSS_PRESENT", L.SEGLOSS_PRESENT),
                 ("LINK_SEGLOSS_ALL", L.SEGLOSS_ALL), ("LINK_SEGLOSS_MIN_CLASSES", L.SEGLOSS_MIN_CLASSES),
                 ("LINK_SEGLOSS_MAX_CLASSES", L.SEGLOSS_MAX_CLASSES)):
        assert f"#define {k} {v}\n" in hdr, k
    import link_amd as la
    assert la.SegCriterion is la.segloss.SegCriterion and callable(la.lovasz_softmax) and callable(la.lovasz_softmax_flat)
    from link_amd.build import SOURCES
    assert "segloss.hip" in SOURCES


def test_section_k_validates_arguments_without_gpu():
    from link_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)                                           # a non-null, aligned pointer nothing dereferences

    def fwd(rows=one, io=L.IO_F32, kind=L.SEGLOSS_LOGITS, labels=one, n=1000, c=19, classes=L.SEGLOSS_PRESENT, ws=one, nbytes=None, out=one,
            unit=one):
        if nbytes is None:
            nbytes = lib.link_segloss_workspace_bytes(n, c)
        return lib.link_segloss_forward(rows, io, kind, labels, n, c, 255, 0, 1, classes, ws, nbytes, out, unit, None)

    need = lib.link_segloss_workspace_bytes(1000, 19)                    # host arithmetic alone: no device needed
    assert need >= 20 * 1000 * 19 and lib.link_segloss_workspace_bytes(100000, 19) > 20 * 100000 * 19
    assert lib.link_segloss_workspace_bytes(1000, 32) > need > lib.link_segloss_workspace_bytes(1000, 2) > 0
    for n, c in ((-1, 19), (1000, 1), (1000, 33), (1000, 0), (1 << 27, 19), (1 << 31, 2), (1 << 62, 4), ((1 << 63) - 1, 2)):
        assert lib.link_segloss_workspace_bytes(n, c) == 0
        assert fwd(n=n, c=c, nbytes=1 << 40) == L.LINK_ERR_ARG
        assert lib.link_segloss_backward(one, one, n, c, L.IO_F32, one, None) == L.LINK_ERR_ARG
    for kw in (dict(rows=None), dict(labels=None), dict(ws=None), dict(out=None), dict(unit=None), dict(io=3), dict(io=-1), dict(kind=2),
               dict(kind=-1), dict(classes=2)):
        assert fwd(**kw) == L.LINK_ERR_ARG, kw
    assert fwd(nbytes=need - 1) == L.LINK_ERR_WORKSPACE and fwd(nbytes=0) == L.LINK_ERR_WORKSPACE
    assert lib.link_segloss_backward(None, one, 1000, 19, L.IO_F32, one, None) == L.LINK_ERR_ARG
    assert lib.link_segloss_backward(one, None, 1000, 19, L.IO_F32, one, None) == L.LINK_ERR_ARG
    assert lib.link_segloss_backward(one, one, 1000, 19, L.IO_F32, None, None) == L.LINK_ERR_ARG
    assert lib.link_segloss_backward(one, one, 1000, 19, 3, one, None) == L.LINK_ERR_ARG


def test_python_surface_rejects_bad_arguments():
    import link_amd as la
    x, y = SO.make_case(50, 5, 0)
    crit = la.SegCriterion()
    for bad in (lambda: crit(x, y.int()), lambda: crit(x, y[:-1]), lambda: crit(x[None], y), lambda: crit(x, y[:, None]),
                lambda: crit(x.long(), y), lambda: crit(x, y.to("meta")), lambda: la.lovasz_softmax_flat(x, y.float()),
                lambda: la.lovasz_softmax(x, y), lambda: la.SegCriterion(classes="some")):
        with pytest.raises(ValueError):
            bad()
    p4 = torch.softmax(torch.randn(2, 5, 4, 4), 1)
    y4 = torch.randint(0, 5, (2, 4, 4))
    for nyi in (lambda: la.lovasz_softmax(p4, y4, classes=[1, 2]), lambda: la.lovasz_softmax(p4[:, 0], y4),
                lambda: la.lovasz_softmax(p4[:, :1], y4), lambda: la.SegCriterion(classes=[0, 1]), lambda: crit(x[:, :1], y)):
        with pytest.raises(NotImplementedError):
            nyi()
