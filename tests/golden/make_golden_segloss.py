"""tests/golden/make_golden_segloss.py -- records the fixtures of tests/test_cpu_segloss.py and tests/test_gpu_segloss.py
(tests/golden/segloss_*.npz).  The tests do not run it.

The expected values come from the reference's own code on the CPU, run from where the reference checkout lies (argument 1 or
$LINK_REFERENCE): segmentation/core/lovasz_losses.py, loaded by path, and nn.CrossEntropyLoss(ignore_index=255), composed as
segmentation/core/trainers.py:64-73 composes them (the [N, C] logits reshaped to [1, C, N, 1]).  Nothing of the reference is copied
here.  Inputs are tests/segloss_oracle.py::make_case(n, C, seed=SEED) in fp32.

segloss_{n}x{C}_ign{0|None}.npz   logits, labels, and per `classes` in (present, all): ce, lovasz (fp32 scalars), grad_{classes}
                                  (the autograd gradient of ce + lovasz with respect to the logits)
segloss_4d.npz                    probas [2, 5, 12, 16] (a softmax), labels [2, 12, 16], ignore 0: lovasz and d lovasz / d probas
                                  with per_image False and True
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from segloss_oracle import make_case  # noqa: E402

SEED = 1
CASES = ((3000, 19), (3000, 17), (777, 5))


def load_reference(ref_root):
    path = os.path.join(ref_root, "segmentation", "core", "lovasz_losses.py")
    spec = importlib.util.spec_from_file_location("ref_lovasz_losses", path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # `classes is 'present'`: a SyntaxWarning on current Pythons
        spec.loader.exec_module(mod)
    return mod


def trainer_loss(ref, logits, labels, ignore, classes):
    x = logits.clone().requires_grad_(True)
    ce = torch.nn.CrossEntropyLoss(ignore_index=255)(x, labels)
    xr = x.transpose(0, 1).unsqueeze(0).unsqueeze(-1)
    lr = labels.unsqueeze(0).unsqueeze(-1)
    lov = ref.lovasz_softmax(torch.nn.functional.softmax(xr, dim=1), lr, classes=sys.intern(classes), ignore=ignore)
    (ce + lov).backward()
    return float(ce), float(lov), x.grad.numpy()


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["LINK_REFERENCE"]
    ref = load_reference(ref_root)
    for n, C in CASES:
        logits, labels = make_case(n, C, SEED)
        for ignore in (0, None):
            out = {"logits": logits.numpy(), "labels": labels.numpy()}
            meta = {"n": n, "C": C, "seed": SEED, "ignore": ignore, "ce_ignore": 255}
            for classes in ("present", "all"):
                ce, lov, grad = trainer_loss(ref, logits, labels, ignore, classes)
                meta[classes] = {"ce": ce, "lovasz": lov}
                out[f"grad_{classes}"] = grad
            np.savez(os.path.join(HERE, f"segloss_{n}x{C}_ign{ignore}.npz"), meta=json.dumps(meta), **out)
    g = torch.Generator().manual_seed(SEED)
    probas = torch.softmax(2.0 * torch.randn(2, 5, 12, 16, generator=g), 1)
    labels = torch.randint(0, 5, (2, 12, 16), generator=g)
    labels[1][labels[1] == 4] = 3                              # class 4 absent from the second image only
    out, meta = {"probas": probas.numpy(), "labels": labels.numpy()}, {"ignore": 0, "seed": SEED}
    for per_image in (False, True):
        p = probas.clone().requires_grad_(True)
        loss = ref.lovasz_softmax(p, labels, classes=sys.intern("present"), per_image=per_image, ignore=0)
        loss.backward()
        meta[f"per_image_{per_image}"] = float(loss)
        out[f"grad_per_image_{per_image}"] = p.grad.numpy()
    np.savez(os.path.join(HERE, "segloss_4d.npz"), meta=json.dumps(meta), **out)


if __name__ == "__main__":
    main()
