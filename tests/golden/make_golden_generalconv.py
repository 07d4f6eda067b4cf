"""tests/golden/make_golden_generalconv.py -- golden fixtures for sparse convolutions with per-axis kernel sizes and
strides: the reference's spnn.Conv3d (torchsparse/nn/modules/conv.py; CPU branch of nn/functional/conv.py:47-61, kernel
maps of conv.py:103-122 and nn/functional/downsample.py:11-51) chained over one small frame.  Imported reference, build
container only.  Run:  python tests/golden/make_golden_generalconv.py

Every file: coords / feats of the input (tensor stride 1), and per layer i of the chain its kernel k{i}, the offsets
offs{i} the reference enumerates for it (get_kernel_offsets(kernel_size, input stride)), and the output x{i}_F / x{i}_C;
meta["layers"][i] = kernel_size, stride, transposed, cin, cout, in_stride, out_stride."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402

torchsparse, backend = build_ref.import_reference_python()
from torchsparse import SparseTensor  # noqa: E402
import torchsparse.nn as spnn  # noqa: E402
from torchsparse.nn.utils import get_kernel_offsets  # noqa: E402

META = {"generator": "tests/golden/make_golden_generalconv.py",
        "reference": "MCG-NJU/LinK @ 2024_08_07, imported through oracle/build_ref.py",
        "hash_query_cpu": "oracle restatement (sparsehash absent; oracle/ref_bind.cpp)", "torch": torch.__version__}

# (kernel_size, stride, transposed, cout) per layer; cin of the first layer = 8
CHAINS = {
    "a": [((3, 1, 3), 1, False, 16), ((1, 3, 3), 1, False, 16), ((1, 3, 3), 1, True, 12), ((3, 1, 3), 1, True, 8)],
    "b": [(3, 2, False, 16), (3, 1, False, 24), (3, 2, True, 8)],
    "c": [((2, 2, 1), (2, 2, 1), False, 16), (3, 1, False, 16), (3, 1, True, 12), ((2, 2, 1), (2, 2, 1), True, 8)],
    "d": [((3, 3, 1), (2, 2, 1), False, 16)],
    "e": [(2, 1, False, 16)],
    "f": [((5, 5, 3), 1, False, 16)],
}


def frame(n, grid, batches, seed):
    g = torch.Generator().manual_seed(seed)
    per = []
    for b in range(batches):
        lin = torch.randperm(grid ** 3, generator=g)[: n // batches]
        per.append(torch.stack([lin % grid, (lin // grid) % grid, lin // (grid * grid), torch.full_like(lin, b)], 1))
    coords = torch.cat(per).int()
    return coords, torch.randn(coords.shape[0], 8, generator=g), g


def run(tag, chain, n, grid, batches, seed):
    coords, feats, _ = frame(n, grid, batches, seed)
    torch.manual_seed(seed)
    x = SparseTensor(feats, coords, 1)
    x.cmaps.setdefault(x.stride, x.coords)
    arrays, layers, cin = dict(coords=coords.numpy(), feats=feats.numpy()), [], 8
    for i, (ks, st, tr, cout) in enumerate(chain):
        conv = spnn.Conv3d(cin, cout, kernel_size=ks, stride=st, transposed=tr)
        in_stride = tuple(x.s)
        offs_stride = tuple(in_stride[k] // conv.stride[k] for k in range(3)) if tr else in_stride
        y = conv(x)
        arrays[f"k{i}"] = conv.kernel.detach().numpy()
        arrays[f"offs{i}"] = get_kernel_offsets(conv.kernel_size, offs_stride).numpy()
        arrays[f"x{i}_C"] = y.C.numpy()
        if batches == 1:
            arrays[f"x{i}_F"] = y.F.detach().numpy()
        layers.append(dict(kernel_size=list(conv.kernel_size), stride=list(conv.stride), transposed=tr, cin=cin, cout=cout,
                           in_stride=list(in_stride), out_stride=list(y.s)))
        if tag == "b" and i == 0 and batches == 1:
            # the candidate rule must show: not the floored set, and a site above the inputs' maximum (no upper filter)
            floored = {tuple(r) for r in (coords[:, :3] // 2 * 2).tolist()}
            assert {tuple(r) for r in y.C[:, :3].tolist()} != floored, "k3 s2: the candidate rule gave the floored set"
            assert int(y.C[:, :3].max()) > int(coords[:, :3].max()), "k3 s2: no site above the input maximum"
        x, cin = y, cout
    m = dict(META)
    m.update(layers=layers, batches=batches, features_valid=(batches == 1),
             note="batches > 1: the reference CPU kernel_hash uses row 0's batch index for every row (hash_cpu.cpp:29), so "
                  "neighbour maps of batch > 0 rows -- and the features -- are defective on CPU; only the coordinate outputs "
                  "are stored" if batches > 1 else "")
    name = f"g_generalconv_{tag}.npz" if batches == 1 else f"g_generalconv_{tag}_b{batches}.npz"
    np.savez_compressed(os.path.join(HERE, name), meta=np.array(json.dumps(m)), **arrays)
    print("wrote", name, {k: v.shape for k, v in arrays.items()})


def main():
    for tag, chain in CHAINS.items():
        run(tag, chain, 1500, 14, 1, 0)
    # coordinates only, two batch items: the strided layers of every chain in one file each would repeat the frame; the
    # k3 s2 chain and the anisotropic one cover both coordinate rules
    run("b", CHAINS["b"], 1200, 12, 2, 1)
    run("c", CHAINS["c"], 1200, 12, 2, 1)


if __name__ == "__main__":
    main()
