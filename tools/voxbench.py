"""tools/voxbench.py -- median device time of one full-size S-nusc frame (the points behind synth.s_nusc, grid 1440 x 1440 x 40)
through Voxelizer.generate_padded, with and without the padded voxels.  Device events around the call on one stream, five warm-up calls,
thirty timed ones; the allocations of the Python surface are included.  Prints one JSON line (DESIGN 4k says what it measures)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import link_amd as la  # noqa: E402
from link_amd.synth import s_nusc  # noqa: E402


def main():
    co, _, pts = s_nusc(seed=0, return_points=True)
    p = torch.from_numpy(pts.astype(np.float32)).cuda()
    v = la.Voxelizer([0.075, 0.075, 0.2], [-54, -54, -5.0, 54, 54, 3.0], 10, 200000)
    out = {"points": int(p.shape[0]), "host_restatement_voxels": int(co.shape[0])}
    for rv in (False, True):
        for _ in range(5):
            r = v.generate_padded(p, return_voxels=rv)
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = v.generate_padded(p, return_voxels=rv)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        out["with_voxels" if rv else "mean_only"] = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}
        out["voxels"] = int(r[-1][-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
