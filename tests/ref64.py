"""A float64 R_core reference that scales to frames of millions of voxels (tests/test_gpu_sizes.py).

The arbiters of oracle/link_oracle.py (elk_core_torch over aggregate_torch / aggregate_c) run on the CPU and hold n x P*C
matrices; at 8.6 M voxels and C = 64 that is 17 GB of float64 per matrix.  This evaluates the same formula -- pre_mix linear,
LayerNorm, theta, modulation into P parts, the block sums of voxel_to_aux, the r^3 box sums of aux_to_voxel (utils.py:44-84,
devoxelize_cuda.cu:11-34: sum of the neighbours' sums over the sum of their counts, absent neighbours skipped), de-modulation
and the final LayerNorm -- with plain torch ops on any device, in chunks of voxels, in three passes:

  1. per chunk of rows: pre_mix, LayerNorm, theta, modulation; index_add into per-block sums and counts (blocks numbered by
     torch.unique over the block coordinates with the batch column: the reference's order of small_x.C);
  2. per block: the box sums of sums and counts over the r^3 neighbour blocks;
  3. per chunk of rows again: the blocks' means gathered, de-modulated, LayerNorm -- compared with the kernel's rows of the chunk.

Memory is O(chunk + blocks): no n-row float64 matrix ever exists.  `dtype=torch.float32` evaluates the same formula in fp32 (what
fp32 evaluation costs against the float64 truth: `o32`).  Test infrastructure only: does not import link_amd."""
import json
import os

import torch
import torch.nn.functional as TF

from oracle.link_oracle import theta_torch


def _offsets(r: int) -> torch.Tensor:
    """get_kernel_offsets(r) as a set (the box sum does not depend on the order): [-r//2 + 1, r//2] per axis."""
    ax = torch.arange(-r // 2 + 1, r // 2 + 1)
    g = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return g.to(torch.int64)


class Ref64:
    """R_core of one collated frame (coords [n, 4] int: x, y, z, batch) evaluated in `dtype` on feats.device, chunk by chunk.

    Parameters as oracle.link_oracle.elk_core_torch takes them: `params` (state_dict keys 'pre_mix.0.weight', 'pre_mix.1.weight',
    'pre_mix.1.bias', 'pos_weight.0.weight', 'norm.weight', 'norm.bias', optionally 'alpha'), s, r, baseop, groups, variant,
    tensor_stride; `alpha` (overrides params['alpha']) and `coord_div` (theta of xyz / coord_div: the kernels' LinkElkDesc.coord_div)."""

    def __init__(self, feats, coords, params, s, r, baseop="cos", groups=1, variant="unet", tensor_stride=1, alpha=None,
                 coord_div=1.0, eps=1e-6, dtype=torch.float64, chunk=1 << 20):
        assert feats.dim() == 2 and coords.dim() == 2 and coords.shape[1] == 4 and coords.shape[0] == feats.shape[0]
        assert baseop in ("cos", "sin", "cos_x") and chunk >= 1
        self.feats, self.coords = feats, coords
        self.dev, self.dtype, self.chunk = feats.device, dtype, int(chunk)
        self.n, self.C = feats.shape
        self.s, self.r, self.baseop, self.groups, self.variant = int(s), int(r), baseop, int(groups), variant
        self.tensor_stride, self.coord_div, self.eps = tensor_stride, float(coord_div), float(eps)
        self.P = 3 if baseop == "cos_x" else 2
        p = {k: (v.detach().to(self.dev, dtype) if torch.is_tensor(v) else v) for k, v in params.items()}
        if alpha is not None:
            p["alpha"] = alpha.detach().to(self.dev, dtype) if torch.is_tensor(alpha) else alpha
        self.p = p
        self._index()
        self._block_means()

    # ---------------------------------------------------------------------------------------------------- block numbering
    def _index(self):
        """Block of every voxel: floor(xyz / s) with the batch column, numbered by torch.unique (sorted: x, y, z, batch
        lexicographic over a packed key, as torch.unique(dim=0) orders the rows)."""
        c = self.coords.to(self.dev, torch.int64)
        bc = torch.cat([torch.div(c[:, :3], self.s, rounding_mode="floor"), c[:, 3:4]], 1)
        pad = self.r                                                          # room for the neighbour offsets in the packed key
        self._lo = bc.min(0).values - pad
        span = bc.max(0).values + pad - self._lo + 1
        assert float(span.double().prod()) < 2.0 ** 62, "block coordinates too far apart for a packed int64 key"
        self._span = span
        keys, self.inv = torch.unique(self._key(bc), sorted=True, return_inverse=True)
        self.keys = keys
        self.M = keys.shape[0]
        self.blk = bc                                                         # (only for the box sums' neighbour keys below)

    def _key(self, bc):
        u = bc - self._lo
        sp = self._span
        return ((u[:, 0] * sp[1] + u[:, 1]) * sp[2] + u[:, 2]) * sp[3] + u[:, 3]

    def _rows(self, lo, hi):
        """fin (pre_mix + LayerNorm), theta, sin, cos of rows lo .. hi."""
        f = self.feats[lo:hi].to(self.dtype)
        p = self.p
        fin = TF.layer_norm(TF.linear(f, p["pre_mix.0.weight"]), (self.C,), p["pre_mix.1.weight"], p["pre_mix.1.bias"], self.eps)
        xyz = self.coords[lo:hi, :3].to(self.dtype)
        if self.coord_div != 1.0:
            xyz = xyz / self.coord_div
        th = theta_torch(xyz, p["pos_weight.0.weight"], self.baseop, self.groups, p.get("alpha"), self.variant, self.tensor_stride)
        return fin, th, torch.sin(th), torch.cos(th)

    def _modulate(self, fin, th, sin, cos):
        if self.baseop == "sin":
            return torch.cat([fin * sin, fin * cos], 1)
        if self.baseop == "cos":
            return torch.cat([fin * cos, fin * sin], 1)
        return torch.cat([fin * cos, fin * sin, fin * th], 1)

    # ------------------------------------------------------------------------------------------------------ passes 1 and 2
    def _block_means(self):
        W = self.P * self.C
        S = torch.zeros(self.M, W, dtype=self.dtype, device=self.dev)
        cnt = torch.zeros(self.M, dtype=self.dtype, device=self.dev)
        for lo in range(0, self.n, self.chunk):
            hi = min(lo + self.chunk, self.n)
            idx = self.inv[lo:hi]
            S.index_add_(0, idx, self._modulate(*self._rows(lo, hi)))
            cnt.index_add_(0, idx, torch.ones(hi - lo, dtype=self.dtype, device=self.dev))
        # pass 2: the blocks' own coordinates (a voxel of each), then the box sums over the r^3 neighbours
        first = torch.empty(self.M, dtype=torch.int64, device=self.dev)
        first.scatter_(0, self.inv, torch.arange(self.n, device=self.dev))
        bc = self.blk[first]
        del self.blk
        BS = torch.zeros_like(S)
        BC = torch.zeros_like(cnt)
        for o in _offsets(self.r).to(self.dev):
            nb = bc.clone()
            nb[:, :3] += o
            k = self._key(nb)
            pos = torch.searchsorted(self.keys, k).clamp(max=self.M - 1)
            hit = self.keys[pos] == k                                         # absent neighbours are skipped
            pos, rows = pos[hit], torch.nonzero(hit).view(-1)
            BS.index_add_(0, rows, S[pos])
            BC.index_add_(0, rows, cnt[pos])
        self.V = BS / BC[:, None]                                             # utils.py:80: every block is its own neighbour: BC >= 1

    # -------------------------------------------------------------------------------------------------------------- pass 3
    def rows(self, lo, hi):
        """The reference's result rows lo .. hi ([hi - lo, C] in self.dtype)."""
        fin, th, sin, cos = self._rows(lo, hi)
        v = self.V[self.inv[lo:hi]]
        C = self.C
        if self.baseop == "sin":
            new = v[:, :C] * cos - v[:, C:] * sin
        elif self.baseop == "cos":
            new = v[:, :C] * cos + v[:, C:] * sin
        else:
            new = v[:, :C] * cos + v[:, C:2 * C] * sin + (v[:, 2 * C:] - fin * th)
        p = self.p
        return TF.layer_norm(new, (C,), p["norm.weight"], p["norm.bias"], self.eps)

    def compare(self, other):
        """(max|other - ref|, max|ref|, every row of `other` finite) over all rows, chunk by chunk in float64.  `other`: the
        kernel's rows ([n, C] tensor, any float type, any device) or anything with `rows(lo, hi)` (another Ref64 of the same frame: the fp32 evaluation)."""
        assert hasattr(other, "rows") or tuple(other.shape) == (self.n, self.C), (tuple(other.shape), (self.n, self.C))
        dmax, rmax, finite = 0.0, 0.0, True
        for lo in range(0, self.n, self.chunk):
            hi = min(lo + self.chunk, self.n)
            ref = self.rows(lo, hi).to(torch.float64)
            got = other.rows(lo, hi) if hasattr(other, "rows") else other[lo:hi]
            got = got.to(self.dev, torch.float64)
            ok = bool(torch.isfinite(got).all())
            finite = finite and ok
            dmax = max(dmax, float((got - ref).abs().max()) if ok else float("inf"))     # (max() would drop a NaN)
            rmax = max(rmax, float(ref.abs().max()))
        return dmax, rmax, finite

    def rel(self, other):
        """max|other - ref| / max|ref|, and whether `other` is finite everywhere."""
        d, m, ok = self.compare(other)
        return d / max(m, 1e-300), ok


class Rounded:
    """The float64 truth rounded to a half row type: what storing the result in that type alone costs."""

    def __init__(self, ref, dt):
        self.ref, self.dt = ref, dt

    def rows(self, lo, hi):
        return self.ref.rows(lo, hi).to(self.dt)


def record_row(row, name="dense_parity.jsonl"):
    """Append one case's row to `name` in the directory LINK_AMD_PARITY_DIR names; nothing is written when it is unset."""
    d = os.environ.get("LINK_AMD_PARITY_DIR")
    if not d:
        return
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def gate_rows(case, ref, o32, out, dt=torch.float32, absolute=True, record=None, o_round=None):
    """The float64 gate of one frame's rows `out` against `ref` (a Ref64 of the frame):
      (a) every row finite -- the callers' result buffers start as NaN, so a row that was never written cannot pass;
      (b) rel64 = max|out - ref| / max|ref| < 1e-4 for fp32 rows, 4e-3 for fp16, 3e-2 for bf16 (the result is rounded to the row
          type at the kernel boundary) -- dropped with absolute=False, for frames whose theta is so large that evaluating the
          formula itself in fp32 costs more than 1e-4 (tests/test_gpu_train_gate.py gates the same way);
      (c) rel64 <= 4 * o32 + 2 * o_round + 2e-6, o32 = what evaluating the same formula in fp32 costs against the float64 truth,
          o_round = what rounding the truth to the row type costs: an error that passes (b) but sits far above fp32 evaluation
          still fails.
    Nothing in a bound comes from the kernels under test.  `case`: a dict of the case's fields, or any label (kept under "case").
    `record`: None, True (the row goes to dense_parity.jsonl, record_row) or a callable taking the row -- written BEFORE the
    verdicts, so a failing case still leaves its figures.  `o_round`: None, or the caller's own reference-side measurement of what
    the contract's roundings cost (a contract that rounds more than once: tests/conv64.py).  `ref`: a Ref64, or anything with its
    n, rows() and rel() (tests/conv64.py: Conv64).  Returns the row."""
    rel64, finite = ref.rel(out)
    if o_round is None:
        o_round = 0.0 if dt == torch.float32 else ref.rel(Rounded(ref, dt))[0]
    row = dict(case) if isinstance(case, dict) else dict(case=case)
    row.update(n=int(ref.n), rel64=rel64, o32=o32, o_round=o_round)
    if record is True:
        record_row(row)
    elif record is not None:
        record(row)
    assert finite, row
    if absolute:
        assert rel64 < (1e-4 if dt == torch.float32 else (4e-3 if dt == torch.float16 else 3e-2)), row
    assert rel64 <= 4.0 * o32 + 2.0 * o_round + 2e-6, row
    return row


def gate_zero_rows(case, ref, ref32, out, scale, record=None):
    """The gate for a frame whose rows are analytically ZERO before the final LayerNorm (sin on a voxel alone in its neighbourhood:
    f sin cos - f cos sin), so that max|ref| is rounding residue and a relative error means nothing.  As tests/grad64.py, gate_zero:
    what the kernels leave is held against the residue of the reference's own fp32 evaluation `ref32` (a Ref64 of the frame with
    dtype=torch.float32): max|out - ref| <= 4 max|ref32 - ref| + 2e-6 `scale` (the size rows have when they are not zero: the norm
    weights), with the float64 rows themselves below 1e-9 `scale`.  fp32 rows only."""
    e, m64, finite = ref.compare(out)
    o32 = ref.compare(ref32)[0]
    row = dict(case) if isinstance(case, dict) else dict(case=case)
    row.update(n=int(ref.n), zero=True, e=e, o32=o32, max_ref=m64, bound=4.0 * o32 + 2e-6 * scale)
    if record is True:
        record_row(row)
    elif record is not None:
        record(row)
    assert finite and out.dtype == torch.float32, row
    assert m64 <= 1e-9 * scale, row
    assert e <= row["bound"], row
    return row
