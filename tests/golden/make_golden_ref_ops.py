"""tests/golden/make_golden_ref_ops.py -- g_ref_ops.json: digests of the reference's compiled CPU ops' outputs (build container only).

Runs the ops oracle/build_ref.py compiles from the reference (hash_cpu, kernel_hash_cpu, count_cpu, voxelize_forward_cpu,
voxelize_backward_cpu, devoxelize_forward_cpu) on the seeded inputs of tests/helpers.py::ref_ops_cases and stores shape, dtype and
sha256 of every output: what tests/test_oracle_golden.py::test_oracle_vs_compiled_reference_ops checks the oracle against where
oracle/_ref is not built.  Run:  python tests/golden/make_golden_ref_ops.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from helpers import array_digest, ref_ops_cases  # noqa: E402
from oracle import build_ref  # noqa: E402


def main():
    ref = build_ref.load_module()
    out = {"meta": {"generator": "tests/golden/make_golden_ref_ops.py", "inputs": "tests/helpers.py::ref_ops_cases",
                    "torch": torch.__version__},
           "ops": {}}
    for name, (args, _) in ref_ops_cases().items():
        targs = [torch.from_numpy(a) if hasattr(a, "dtype") else a for a in args]
        out["ops"][name] = array_digest(getattr(ref, name)(*targs).numpy())
    with open(os.path.join(HERE, "g_ref_ops.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
