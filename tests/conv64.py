"""A float64 reference of the sparse convolution, written from the definition (tests/test_gpu_conv_lattice.py; checked itself by
tests/test_cpu_conv_frames.py against the oracle, torch's dense conv3d and autograd).

For a table nbr int32 [n_out, kvol] (-1 = absent), rows f [n_in, cin] and weights w [kvol, cin, cout]:

  out[j] = sum_k f[nbr[j, k]] @ w[k]                                    Conv64.rows
  A[j]   = sum_k |f[nbr[j, k]]| @ |w[k]|                                Conv64.magnitude   (float64: the per-element yardstick)
  B[j]   = sum_k (sum_ci |f[nbr[j, k], ci]| + sum_ci |w[k, ci, :]|)     Conv64.magnitude1  (the split form's absolute term)
  epilogue(x) = relu?(addend? + LayerNorm(x) * ln_w + ln_b)  or, affine: relu?(addend? + x * ln_w + ln_b)
  g_f[i] = sum_{(j, k): nbr[j, k] = i} g_out[j] @ w[k]^T,   g_w[k] = sum_{j: nbr[j, k] >= 0} f[nbr[j, k]]^T (x) g_out[j]      grads

Plain torch (index_select / matmul) on the tensors' device, in chunks of rows, so a 270 k-row case costs milliseconds on the GPU and
no [n, kvol, cin] tensor ever exists.  dtype=torch.float32 evaluates the same formula in fp32 (what evaluating it in fp32 costs
against the float64 truth: `o32`).  16-bit rows: the truth is float64 over the ROUNDED inputs the contract states (the caller hands
in rows and weights already rounded to the row type); `contract` restates, in float64 arithmetic, where the contract rounds on the
way -- ("end", rt): once, at the store (the resident AMP form; the pair-list form with fp32 contribution rows);
("offset", rt, centre): every offset's product row to rt except offset `centre` (the submanifold centre, formed in the accumulators;
None: every offset), summed, and once more at the store (the pair-list fp16 form) -- and `o_round` is measured from that
restatement.  Test infrastructure only: does not import link_amd."""
import torch
import torch.nn.functional as TF

U32 = 2.0 ** -24                       # unit roundoff of fp32
UNIT = {torch.float32: U32, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
F16_SUB = 2.0 ** -25                   # absolute error of rounding into fp16's subnormal range (spacing 2^-24)


def epilogue(x, ln_w, ln_b, eps, addend=None, relu=False, affine=False):
    """The store phase of subm_conv_ln_add_relu on rows x, in x's dtype."""
    dt = x.dtype
    lw, lb = ln_w.to(x.device, dt), ln_b.to(x.device, dt)
    y = x * lw + lb if affine else TF.layer_norm(x, (x.shape[1],), lw, lb, eps)
    if addend is not None:
        y = addend.to(x.device, dt) + y
    return torch.relu(y) if relu else y


class Conv64:
    """The convolution of one (table, rows, weights) triple evaluated in `dtype`, chunk by chunk; `ep` = None or a dict of
    epilogue()'s keyword arguments (addend: all n_out rows).  The interface tests/ref64.py's gate_rows takes: n, rows(), rel()."""

    def __init__(self, f, w, nbr, dtype=torch.float64, chunk=1 << 15, ep=None, contract=None):
        assert f.dim() == 2 and w.dim() == 3 and nbr.dim() == 2 and w.shape[0] == nbr.shape[1] and w.shape[1] == f.shape[1]
        assert contract is None or dtype == torch.float64
        self.dev, self.dtype, self.chunk = f.device, dtype, int(chunk)
        self.n, self.kvol = int(nbr.shape[0]), int(nbr.shape[1])
        self.n_in, self.cin, self.C = int(f.shape[0]), int(w.shape[1]), int(w.shape[2])
        assert self.n == 0 or int(nbr.max()) < self.n_in, "the table names a row past the input"
        self.nbr = nbr.to(self.dev, torch.int64)
        # one zero row behind the input: what an absent neighbour gathers
        self.f = torch.cat([f.detach().to(dtype), torch.zeros(1, self.cin, dtype=dtype, device=self.dev)])
        self.w = w.detach().to(self.dev, dtype)
        self.ep, self.contract = ep, contract
        self._amax = None

    def _idx(self, lo, hi, k):
        i = self.nbr[lo:hi, k]
        return torch.where(i < 0, torch.full_like(i, self.n_in), i)

    def plain(self, lo, hi):
        """sum_k f[nbr[j, k]] @ w[k] of rows lo .. hi (no epilogue), with the contract's roundings where one is set."""
        out = torch.zeros(hi - lo, self.C, dtype=self.dtype, device=self.dev)
        for k in range(self.kvol):
            p = self.f.index_select(0, self._idx(lo, hi, k)) @ self.w[k]
            if self.contract is not None and self.contract[0] == "offset" and k != self.contract[2]:
                p = p.to(self.contract[1]).to(self.dtype)
            out += p
        return out

    def rows(self, lo, hi):
        x = self.plain(lo, hi)
        if self.ep is not None:
            ep = dict(self.ep)
            if ep.get("addend") is not None:
                ep["addend"] = ep["addend"][lo:hi]
            x = epilogue(x, **ep)
        if self.contract is not None:
            x = x.to(self.contract[1]).to(self.dtype)
        return x

    def magnitude(self, lo, hi):
        """A of rows lo .. hi, float64."""
        out = torch.zeros(hi - lo, self.C, dtype=torch.float64, device=self.dev)
        fa, wa = self.f.abs().double(), self.w.abs().double()
        for k in range(self.kvol):
            out += fa.index_select(0, self._idx(lo, hi, k)) @ wa[k]
        return out

    def magnitude1(self, lo, hi):
        """B of rows lo .. hi, float64: per present (row, offset) the row's sum of |f| plus the column sums of |w[k]|."""
        out = torch.zeros(hi - lo, self.C, dtype=torch.float64, device=self.dev)
        fs, ws = self.f.abs().double().sum(1), self.w.abs().double().sum(1)          # [n_in + 1], [kvol, cout]
        for k in range(self.kvol):
            present = (self.nbr[lo:hi, k] >= 0).double()[:, None]
            out += fs.index_select(0, self._idx(lo, hi, k))[:, None] + present * ws[k][None, :]
        return out

    def max_magnitude(self):
        if self._amax is None:
            self._amax = max([float(self.magnitude(lo, min(lo + self.chunk, self.n)).max())
                              for lo in range(0, self.n, self.chunk)] + [0.0])
        return self._amax

    def absent_rows(self):
        """bool [n_out]: rows whose table row is all -1."""
        return (self.nbr < 0).all(1)

    def compare(self, other):
        """(max|other - ref|, max|ref|, every element of `other` finite) over all rows; `other`: [n_out, cout] or anything with rows()."""
        assert hasattr(other, "rows") or tuple(other.shape) == (self.n, self.C), (tuple(other.shape), (self.n, self.C))
        dmax, rmax, finite = 0.0, 0.0, True
        for lo in range(0, self.n, self.chunk):
            hi = min(lo + self.chunk, self.n)
            ref = self.rows(lo, hi).to(torch.float64)
            got = (other.rows(lo, hi) if hasattr(other, "rows") else other[lo:hi]).to(self.dev, torch.float64)
            ok = bool(torch.isfinite(got).all())
            finite = finite and ok
            dmax = max(dmax, float((got - ref).abs().max()) if ok else float("inf"))
            rmax = max(rmax, float(ref.abs().max()))
        return dmax, rmax, finite

    def rel(self, other):
        d, m, ok = self.compare(other)
        return d / max(m, 1e-300), ok

    def worst_ratio(self, out, bound, need_b=True):
        """max over elements of |out - plain| / bound(A, B, |plain|) -- `bound` maps the chunk's float64 [rows, cout] magnitudes to
        the per-element bound (tests/conv_frames.py: element_bound; B is None with need_b=False: only the split form's bound reads it).
        The comparison is with the convolution BEFORE any epilogue."""
        worst = 0.0
        for lo in range(0, self.n, self.chunk):
            hi = min(lo + self.chunk, self.n)
            ref = self.plain(lo, hi).double()
            d = (out[lo:hi].to(self.dev, torch.float64) - ref).abs()
            b = bound(self.magnitude(lo, hi), self.magnitude1(lo, hi) if need_b else None, ref.abs())
            r = torch.where(d > 0, d / b, torch.zeros_like(d))                       # (0 / 0 on an all-absent row: no error)
            worst = max(worst, float(r.max()) if bool(torch.isfinite(r).all()) else float("inf"))
        return worst


def grads(f, w, nbr, g_out, dtype=torch.float64, chunk=1 << 15):
    """(g_f [n_in, cin], g_w [kvol, cin, cout]) of sum(out * g_out) for the plain form, from the definition, in `dtype`."""
    dev = f.device
    n_in, cin = f.shape
    kvol, _, cout = w.shape
    f64 = f.detach().to(dtype)
    wd, g = w.detach().to(dev, dtype), g_out.detach().to(dev, dtype)
    g_f = torch.zeros(n_in, cin, dtype=dtype, device=dev)
    g_w = torch.zeros(kvol, cin, cout, dtype=dtype, device=dev)
    for lo in range(0, nbr.shape[0], chunk):
        hi = min(lo + chunk, nbr.shape[0])
        idx = nbr[lo:hi].to(dev, torch.int64)
        for k in range(kvol):
            rows = torch.nonzero(idx[:, k] >= 0).view(-1)                            # the pairs of offset k in this chunk
            src, gk = idx[rows, k], g[lo:hi].index_select(0, rows)
            g_f.index_add_(0, src, gk @ wd[k].t())
            g_w[k] += f64.index_select(0, src).t() @ gk
    return g_f, g_w


def grad_magnitudes(f, w, nbr, g_out):
    """(A_f, A_w, pairs): the gradients of the same table over |f|, |w|, |g_out| in float64 -- what the terms of every element's
    sum add up to in magnitude -- and the pairs of every offset (the term count of g_w[k]'s sums)."""
    a_f, a_w = grads(f.abs(), w.abs(), nbr, g_out.abs())
    return a_f, a_w, (nbr >= 0).sum(0)
