"""link_amd/segio.py -- the segmentation front end and the validation back end on the device (csrc/segio.hip, section M of
include/link_amd.h) behind the surfaces the reference's segmentation pipeline uses on the host:

    sparse_quantize(coords, voxel_size, return_index, return_inverse)    torchsparse/utils/quantize.py:24-46
    sparse_collate(inputs), sparse_collate_fn(inputs)                    torchsparse/utils/collate.py:11-59
    SegVoxelizer(voxel_size)(blocks, labels)                             core/datasets/semantic_kitti.py:219-248 (use_aug=False) for
                                                                         every frame of a batch, then sparse_collate_fn
    SegEvaluator(num_classes, ignore_label)                              evaluate.py:120-134 (inverse map, vote, argmax) and
                                                                         core/callbacks.py:36-79 (MeanIoU)

A frame goes from raw points to mIoU counters with ONE read-back (the voxel total, the size of what the voxeliser returns);
`SegVoxelizer.generate_padded` has fixed shapes and none, `SegEvaluator.update` has none, `SegEvaluator.compute` has one for the
epoch (after one all_reduce of the [3, c] counters when torch.distributed is initialised).

GPU tensors run the kernels (for the evaluator: 2..32 classes in fp32 / fp16 / bf16, or integer predictions).  Everything else -- CPU
tensors, other class counts, rows of another floating type -- runs `_torch_*` below: the same definitions as a torch composition,
which is also what the CPU tests check.  That composition is a second implementation for the inputs the kernels are not built for,
not a stand-in for a missing library: on a GPU tensor in the built range a missing library raises.
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .tensor import SparseTensor

_IO = {torch.float32: L.IO_F32, torch.float16: L.IO_F16, torch.bfloat16: L.IO_BF16}
SORT_TILE = L.SORT_TILE
MAX_BATCH = 1024
_EXT = 1 << 20


# ------------------------------------------------------------------------------------------------------------- torch composition
def _torch_round(points: torch.Tensor, voxel_size: float) -> torch.Tensor:
    """rint(p / float32(vs)) in fp32, half to even -> float32 [n, 3] (LINK_SEGQ_ROUND before the conversion)"""
    return torch.round(points[:, :3].float() / torch.tensor(voxel_size, dtype=torch.float32, device=points.device))


def _torch_quantize(clouds: Sequence[torch.Tensor], mode: int, voxel_size: float, capacity: int):
    """link_seg_quantize as a torch composition, sample by sample (it reads sizes back: the composition is not the hot path).
    -> coords int32 [cap, 4], indices int32 [cap], inverse int32 [n], inverse_local int32 [n], voxel_offsets int32 [B + 1],
    status int32 [4]"""
    device = clouds[0].device
    n = sum(int(c.shape[0]) for c in clouds)
    coords = torch.zeros((capacity, 4), dtype=torch.int32, device=device)
    indices = torch.zeros((capacity,), dtype=torch.int32, device=device)
    inverse = torch.full((n,), -1, dtype=torch.int32, device=device)
    inverse_local = torch.full((n,), -1, dtype=torch.int32, device=device)
    voff = [0]
    flags, total, p0, ext_max, good = 0, 0, 0, [0, 0, 0], []
    for b, c in enumerate(clouds):
        m = int(c.shape[0])
        q, bad = None, 0
        if m:
            if mode == L.SEGQ_INT:
                q = c[:, :3].to(torch.int64)
            else:
                r = _torch_round(c, voxel_size)
                if not bool(torch.isfinite(r).all()):
                    bad |= L.SEGQ_FLAG_NONFINITE
                if bool((r[torch.isfinite(r)].abs() >= 2147483648.0).any()):
                    bad |= L.SEGQ_FLAG_EXTENT
                if not bad:
                    q = r.to(torch.int64)
            if not bad:
                q = q - q.min(0, keepdim=True).values
                ext = [int(v) for v in q.max(0).values]
                if max(ext) >= _EXT:
                    bad |= L.SEGQ_FLAG_EXTENT
                else:
                    ext_max = [max(a, e) for a, e in zip(ext_max, ext)]
        flags |= bad
        good.append((b, p0, m, q if (m and not bad) else None))
        p0 += m
    nbits = sum(int(e).bit_length() for e in ext_max) + (len(clouds) - 1).bit_length()
    if nbits > 64:
        flags |= L.SEGQ_FLAG_KEYBITS
        nbits = (len(clouds) - 1).bit_length()
        good = [(b, p, m, None) for b, p, m, _ in good]
    for b, p, m, q in good:
        if q is not None:
            key = (q[:, 0] * _EXT + q[:, 1]) * _EXT + q[:, 2]
            uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
            k = int(uniq.shape[0])
            first = torch.full((k,), m, dtype=torch.int64, device=device).scatter_reduce(0, inv, torch.arange(m, device=device), "amin")
            keep = max(0, min(k, capacity - total))
            coords[total:total + keep, :3] = q[first[:keep]].to(torch.int32)
            coords[total:total + keep, 3] = b
            indices[total:total + keep] = (first[:keep] + p).to(torch.int32)
            fits = inv + total < capacity
            inverse[p:p + m] = torch.where(fits, inv + total, torch.full_like(inv, -1)).to(torch.int32)
            inverse_local[p:p + m] = torch.where(fits, inv, torch.full_like(inv, -1)).to(torch.int32)
            total += k
        voff.append(min(total, capacity))
    voxel_offsets = torch.tensor(voff, dtype=torch.int32, device=device)
    status = torch.tensor([total, flags, nbits, n], dtype=torch.int32, device=device)
    return coords, indices, inverse, inverse_local, voxel_offsets, status


def _torch_vote(rows: torch.Tensor, inverse: Optional[torch.Tensor]) -> torch.Tensor:
    """rows [n_rows, c], inverse int [V, P] or None -> the class of every point, int64 [P]: the votes summed in fp32 in ascending pass
    order, the lowest class index among equals, a NaN sum counting as -inf"""
    n_rows, c = rows.shape
    if inverse is None:
        acc = rows.float()
    else:
        acc = torch.zeros((inverse.shape[1], c), dtype=torch.float32, device=rows.device)
        for v in range(inverse.shape[0]):
            idx = inverse[v].long()
            ok = (idx >= 0) & (idx < n_rows)
            if n_rows:
                acc = acc + torch.where(ok[:, None], rows[idx.clamp(0, n_rows - 1)].float(), acc.new_zeros(()))
    acc = torch.where(torch.isnan(acc), acc.new_full((), float("-inf")), acc)      # a NaN never wins
    best = acc.max(1, keepdim=True).values
    cls = torch.arange(c, device=rows.device)[None, :].expand_as(acc)
    return torch.where(acc == best, cls, torch.full_like(cls, c)).min(1).values.clamp_max(c - 1)


def _torch_count(cls: torch.Tensor, labels: torch.Tensor, c: int, ignore_label: int) -> torch.Tensor:
    """-> int64 [3, c] = seen, positive, correct over the points with label != ignore_label"""
    cls, labels = cls.long(), labels.long()
    counts = labels != ignore_label
    y_in = counts & (labels >= 0) & (labels < c)
    p_in = counts & (cls >= 0) & (cls < c)
    one = lambda mask, v: torch.bincount(v[mask], minlength=c)[:c]
    return torch.stack([one(y_in, labels), one(p_in, cls), one(y_in & (cls == labels), labels)])


# ------------------------------------------------------------------------------------------------------------------ quantisation
class _Workspace:
    """Byte buffers per device, grown on demand (one stream at a time, as the C entry asks).  A buffer that was handed out is never
    freed while the workspace lives: a graph captured from an earlier call holds its address, and a replay after a larger eager call
    must still write into memory that is this workspace's.  Growth at least doubles, so what is retained stays below the size of the
    current buffer."""

    def __init__(self):
        self._buf = {}
        self._retired = []

    def get(self, device, n: int, batch: int):
        need = L.lib().link_seg_quantize_workspace_bytes(n, batch)
        if need == 0:
            raise L.LinkAmdError(f"link_seg_quantize: {n} points in {batch} clouds outside what the kernels address "
                                 f"(fewer than 2^28 points, 1..{MAX_BATCH} clouds)")
        buf = self._buf.get(device)
        if buf is None or buf.numel() < need:
            if buf is not None:
                self._retired.append(buf)
                need = max(need, 2 * buf.numel())
            buf = self._buf[device] = torch.empty(need, dtype=torch.uint8, device=device)
        return buf


class _Quantizer:
    """The launch of link_seg_quantize, its workspaces and the point offsets of the batch shapes seen."""

    def __init__(self):
        self._ws = _Workspace()
        self._offsets = {}

    def run(self, clouds: Sequence[torch.Tensor], mode: int, voxel_size: float = 1.0, capacity: Optional[int] = None):
        """-> (coords int32 [cap, 4] = x, y, z, b, indices int32 [cap], inverse int32 [n], inverse_local int32 [n],
        voxel_offsets int32 [B + 1], status int32 [4]), all on the clouds' device"""
        clouds = list(clouds)
        if not 1 <= len(clouds) <= MAX_BATCH:
            raise ValueError(f"quantize: 1..{MAX_BATCH} clouds expected, got {len(clouds)}")
        device = clouds[0].device
        for c in clouds:
            if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] < 3 or c.shape[1] != clouds[0].shape[1]:
                raise ValueError("quantize: every cloud is a tensor [n, d] with the same d >= 3")
            if c.device != device:
                raise ValueError(f"quantize: clouds on {device} and {c.device}")
            if mode == L.SEGQ_INT and (c.is_floating_point() or c.shape[1] != 3):
                raise ValueError("quantize: integer coordinates [n, 3] expected")
            if mode == L.SEGQ_ROUND and not c.is_floating_point():
                raise ValueError("quantize: floating point blocks expected")
        if mode == L.SEGQ_ROUND and not (float(voxel_size) > 0 and np.isfinite(voxel_size)):
            raise ValueError(f"quantize: voxel size {voxel_size} is not positive and finite")
        sizes = [int(c.shape[0]) for c in clouds]
        n = sum(sizes)
        cap = n if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError(f"quantize: capacity {cap}")
        if not device.type == "cuda":
            return _torch_quantize(clouds, mode, float(voxel_size), cap)
        ndim = int(clouds[0].shape[1])
        pts = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
        pts = pts.to(torch.int32 if mode == L.SEGQ_INT else torch.float32).contiguous()
        if mode == L.SEGQ_ROUND and ndim > 16:
            pts, ndim = pts[:, :3].contiguous(), 3
        ws = self._ws.get(device, n, len(clouds))
        offs = L.point_offsets(self._offsets, device, sizes)
        coords = torch.empty((cap, 4), dtype=torch.int32, device=device)
        indices = torch.empty((cap,), dtype=torch.int32, device=device)
        inverse = torch.empty((2, n), dtype=torch.int32, device=device)
        voff = torch.empty((len(clouds) + 1,), dtype=torch.int32, device=device)
        status = torch.empty((4,), dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            L.check(L.lib().link_seg_quantize(pts.data_ptr(), mode, ndim, float(voxel_size), offs.data_ptr(), len(clouds), n, ws.data_ptr(),
                                              ws.numel(), coords.data_ptr(), indices.data_ptr(), cap, inverse[0].data_ptr(),
                                              inverse[1].data_ptr(), voff.data_ptr(), status.data_ptr(), L.current_stream_handle()),
                    "link_seg_quantize")
        return coords, indices, inverse[0], inverse[1], voff, status


_QUANTIZER = _Quantizer()


def _raise_flags(flags: int, what: str):
    if flags:
        names = [n for n, f in (("an axis extent of 2^20 or more", L.SEGQ_FLAG_EXTENT), ("a coordinate that is not finite", L.SEGQ_FLAG_NONFINITE),
                                ("a sort key wider than 64 bits", L.SEGQ_FLAG_KEYBITS)) if flags & f]
        raise L.LinkAmdError(f"{what}: " + ", ".join(names) + " (the sample produced no voxels)")


def _voxel_size3(voxel_size):
    """one edge length, or one per axis -> three floats"""
    vs = [voxel_size] * 3 if np.isscalar(voxel_size) else list(voxel_size)
    if len(vs) != 3 or not all(np.isfinite(float(v)) and float(v) > 0 for v in vs):
        raise ValueError(f"sparse_quantize: voxel_size is one positive number or three, got {voxel_size!r}")
    return [float(v) for v in vs]


def sparse_quantize(coords, voxel_size=1, *, return_index: bool = False, return_inverse: bool = False):
    """torchsparse.utils.quantize.sparse_quantize on a tensor [n, 3] (a GPU tensor runs the kernels; a numpy array is taken through
    the torch composition and numpy comes back): the distinct voxels of floor(coords / voxel_size), minus their minimum per axis (the
    reference's ravel_hash subtracts it in place), in ascending (x, y, z) order as int32 [m, 3]; with return_index the first point of
    every voxel, with return_inverse the voxel of every point, both int64; a single result comes back bare, several as a list.
    A voxel coordinate outside int32 raises.  One read-back: m, with the verdict of the range test beside it."""
    vs = _voxel_size3(voxel_size)
    as_numpy = isinstance(coords, np.ndarray)
    c = torch.from_numpy(np.ascontiguousarray(coords)) if as_numpy else coords
    if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
        raise ValueError("sparse_quantize: coords [n, 3] expected")
    if c.is_floating_point() or vs != [1.0, 1.0, 1.0]:
        c = torch.floor(c.double() / torch.tensor(vs, dtype=torch.float64, device=c.device))     # the reference divides in float64
    narrow = c.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8)
    # the range test stays on the device and travels with the voxel total: still one read-back
    out_of_range = torch.zeros((), dtype=torch.bool, device=c.device) if narrow else ~((c >= -2147483648) & (c <= 2147483647)).all()
    vox, first, inverse, _, _, status = _QUANTIZER.run([c.to(torch.int32)], L.SEGQ_INT)
    total, flags, wrapped = (int(v) for v in torch.cat([status[:2], out_of_range.to(torch.int32)[None]]).tolist())
    if wrapped:                                                          # a NaN fails both comparisons
        raise L.LinkAmdError("sparse_quantize: a voxel coordinate leaves int32 or is not finite")
    _raise_flags(flags, "sparse_quantize")
    wanted = [(True, vox[:total, :3]), (return_index, first[:total].long()), (return_inverse, inverse.long())]
    results = [t.numpy() if as_numpy else t for want, t in wanted if want]
    return results if len(results) > 1 else results[0]


def _as_tensor(v, what):
    if isinstance(v, np.ndarray):
        return torch.from_numpy(v)
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"sparse_collate: {what} must be a tensor or an array, got {type(v).__name__}")
    return v


def sparse_collate(inputs: Sequence[SparseTensor]) -> SparseTensor:
    """torchsparse.utils.collate.sparse_collate: one SparseTensor of all rows, the position of every input in the list appended
    to its coordinates as a last (batch) column of int32.  Arrays are accepted for coords / feats; the inputs are left as they are."""
    inputs = list(inputs)
    if not inputs:
        raise ValueError("sparse_collate: at least one SparseTensor expected")
    stride = inputs[0].stride
    if any(x.stride != stride for x in inputs):
        raise ValueError(f"sparse_collate: strides differ: {[x.stride for x in inputs]}")
    coords = torch.cat([_as_tensor(x.coords, "coords") for x in inputs])
    feats = torch.cat([_as_tensor(x.feats, "feats") for x in inputs])
    sizes = torch.tensor([int(x.coords.shape[0]) for x in inputs], device=coords.device)
    batch = torch.repeat_interleave(torch.arange(len(inputs), dtype=torch.int32, device=coords.device), sizes)
    return SparseTensor(feats, torch.cat([coords, batch[:, None].to(coords.dtype)], dim=1), stride)


def _stack(values):
    return torch.stack([_as_tensor(v, "an entry") for v in values])


# how sparse_collate_fn joins the values of one key, chosen by the type of the first sample's value
_COLLATORS = ((dict, lambda values: sparse_collate_fn(values)), (SparseTensor, sparse_collate), ((np.ndarray, torch.Tensor), _stack))


def sparse_collate_fn(inputs: List[Any]) -> Any:
    """torchsparse.utils.collate.sparse_collate_fn: a list of per-sample dicts becomes one dict -- nested dicts recursively, arrays and
    tensors stacked along a new first axis, SparseTensors through sparse_collate, any other value kept as the list of the samples'
    values; a list of anything else comes back as it is"""
    if not inputs or not isinstance(inputs[0], dict):
        return inputs
    out = {}
    for key, first in inputs[0].items():
        join = next((fn for kind, fn in _COLLATORS if isinstance(first, kind)), list)
        out[key] = join([sample[key] for sample in inputs])
    return out


class SegVoxelizer:
    """get_single_sample(use_aug=False) of core/datasets/semantic_kitti.py:219-248 for every frame of a batch, followed by
    sparse_collate_fn, on the device.  blocks: a list of [n, >= 3] floating tensors (x, y, z first; the whole row becomes the voxel's
    feature).  The coordinate is round(block[:, :3] / voxel_size) in fp32, half to even, minus the frame's minimum per axis.  One
    SegVoxelizer serves one stream at a time (its workspace is its own)."""

    def __init__(self, voxel_size: float, num_points: Optional[int] = None, use_aug: bool = False):
        if num_points is not None:
            raise NotImplementedError("SegVoxelizer: the random subsample to num_points draws from the host's generator and is not built")
        if use_aug:
            raise NotImplementedError("SegVoxelizer: the rotation / scale / flip augmentations draw from the host's generator and are not built")
        self.voxel_size = float(voxel_size)
        if not (self.voxel_size > 0 and np.isfinite(self.voxel_size)):
            raise ValueError(f"SegVoxelizer: voxel size {voxel_size}")
        self._q = _Quantizer()

    @staticmethod
    def _blocks(blocks):
        blocks = [blocks] if isinstance(blocks, torch.Tensor) else list(blocks)
        for b in blocks:
            if not isinstance(b, torch.Tensor) or not b.is_floating_point() or b.dim() != 2 or b.shape[1] < 3:
                raise ValueError("SegVoxelizer: blocks are floating tensors [n, >= 3]")
        return blocks

    @torch.no_grad()
    def generate_padded(self, blocks, capacity: Optional[int] = None):
        """Fixed shapes, no host round trip, capturable in a graph: (coords int32 [cap, 4] = x, y, z, b, indices int32 [cap],
        inverse int32 [n] (rows of coords), inverse_local int32 [n] (counted inside the frame), voxel_offsets int32 [B + 1],
        status int32 [4] = voxel total before clamping, flags, key bits, points).  cap = `capacity`, by default the number of points;
        rows past voxel_offsets[B] are zero, a point whose voxel does not fit has inverse -1.  A captured call keeps the address of
        the workspace it ran with; the voxeliser never frees a workspace it has used (a larger later call gets a new one beside it), so
        a replay stays valid for as long as the SegVoxelizer lives -- keep it alive with the graph."""
        return self._q.run(self._blocks(blocks), L.SEGQ_ROUND, self.voxel_size, capacity)

    @torch.no_grad()
    def __call__(self, blocks, labels=None):
        """-> {'lidar', 'targets', 'targets_mapped', 'inverse_map'}: link_amd.SparseTensors with the batch column appended.  One
        read-back: the voxel total."""
        blocks = self._blocks(blocks)
        device = blocks[0].device
        n = sum(int(b.shape[0]) for b in blocks)
        if labels is None:
            lab = torch.zeros((n,), dtype=torch.int64, device=device)     # the test split's labels_
        else:
            labels = [labels] if isinstance(labels, torch.Tensor) else list(labels)
            if len(labels) != len(blocks) or any(int(y.shape[0]) != int(b.shape[0]) for y, b in zip(labels, blocks)):
                raise ValueError("SegVoxelizer: one label per point expected")
            lab = labels[0] if len(labels) == 1 else torch.cat(labels)
        coords, indices, inverse, inverse_local, _, status = self._q.run(blocks, L.SEGQ_ROUND, self.voxel_size, None)
        total, flags = (int(v) for v in status[:2].tolist())
        _raise_flags(flags, "SegVoxelizer")
        feats = blocks[0] if len(blocks) == 1 else torch.cat(blocks)
        pc = coords[:total]
        inds = indices[:total].long()
        pc_ = pc[inverse.long()]                                          # every point's own coordinate is its voxel's
        return {"lidar": SparseTensor(feats[inds], pc), "targets": SparseTensor(lab[inds], pc),
                "targets_mapped": SparseTensor(lab, pc_), "inverse_map": SparseTensor(inverse_local.long(), pc_)}


# -------------------------------------------------------------------------------------------------------------------- validation
class SegEvaluator:
    """MeanIoU of core/callbacks.py with the vote of evaluate.py:120-134 in front, on the device.

    update(outputs, targets, inverse=None, lut=None) -> the predicted class of every point (int64), no read-back:
        outputs floating [n_rows, c]: logits; inverse int [P] or [V, P] names the row of every point per test-time-augmentation pass
            (rows of the batched output: SegVoxelizer.generate_padded's `inverse`); without it point p reads row p;
        outputs integer [P]: predictions (the training-time callback receives arg-maxed outputs);
        targets int64 [P] or None (then nothing is counted); lut int [c] remaps the returned classes, never the counters.
    compute(all_reduce=True) -> {'miou', 'macc', 'oacc', 'ious', 'accs', 'seen', 'positive', 'correct'}: one all_reduce of the
        [3, c] counters when torch.distributed is initialised, one read-back, then callbacks.py:63-79 over the classes 1..c-1.
    The counters live on the device of the first update, or on `device` when it is given (give it where a rank may reach compute()
    without an update: its zeros must lie where the other ranks' counters do; without it such a rank uses the current GPU under
    nccl and the CPU otherwise)."""

    def __init__(self, num_classes: int, ignore_label: int, device=None):
        self.num_classes = int(num_classes)
        self.ignore_label = int(ignore_label)
        if self.num_classes < 2:
            raise ValueError(f"SegEvaluator: num_classes {num_classes}")
        self.counters = None if device is None else torch.zeros((3, self.num_classes), dtype=torch.int64, device=device)

    def reset(self):
        if self.counters is not None:
            self.counters.zero_()

    def _counters(self, device):
        if self.counters is None:
            self.counters = torch.zeros((3, self.num_classes), dtype=torch.int64, device=device)
        elif self.counters.device != device:
            raise ValueError(f"SegEvaluator: counters on {self.counters.device}, inputs on {device}")
        return self.counters

    @torch.no_grad()
    def update(self, outputs: torch.Tensor, targets: Optional[torch.Tensor], inverse: Optional[torch.Tensor] = None,
               lut: Optional[torch.Tensor] = None) -> torch.Tensor:
        c = self.num_classes
        if not isinstance(outputs, torch.Tensor):
            raise ValueError("SegEvaluator: tensors expected")
        device = outputs.device
        rows_kind = outputs.is_floating_point()
        if rows_kind:
            if outputs.dim() != 2 or outputs.shape[1] != c:
                raise ValueError(f"SegEvaluator: logits [n, {c}] expected, got {tuple(outputs.shape)}")
            if inverse is not None:
                if inverse.is_floating_point() or inverse.dim() not in (1, 2) or inverse.device != device:
                    raise ValueError("SegEvaluator: inverse is an integer tensor [P] or [V, P] on the outputs' device")
                inverse = inverse[None] if inverse.dim() == 1 else inverse
                if not 1 <= inverse.shape[0] <= L.SEGEVAL_MAX_VOTES:
                    raise ValueError(f"SegEvaluator: 1..{L.SEGEVAL_MAX_VOTES} passes expected, got {inverse.shape[0]}")
            p = int(outputs.shape[0]) if inverse is None else int(inverse.shape[1])
        else:
            if outputs.dim() != 1 or inverse is not None:
                raise ValueError("SegEvaluator: predictions are an integer tensor [P], without an inverse")
            p = int(outputs.shape[0])
        if targets is not None and (targets.dim() != 1 or targets.shape[0] != p or targets.is_floating_point() or targets.device != device):
            raise ValueError(f"SegEvaluator: targets are an integer tensor [{p}] on the outputs' device")
        if lut is not None and (lut.dim() != 1 or lut.shape[0] != c or lut.is_floating_point() or lut.device != device):
            raise ValueError(f"SegEvaluator: lut is an integer tensor [{c}] on the outputs' device")
        counters = self._counters(device) if targets is not None else None
        fused = device.type == "cuda" and L.SEGLOSS_MIN_CLASSES <= c <= L.SEGLOSS_MAX_CLASSES and (not rows_kind or outputs.dtype in _IO)
        if not fused:
            cls = _torch_vote(outputs, inverse) if rows_kind else outputs.long()
            if targets is not None:
                counters += _torch_count(cls, targets, c, self.ignore_label)
            if lut is None:
                return cls
            return torch.where((cls >= 0) & (cls < c), lut.long()[cls.clamp(0, c - 1)], cls)
        rows = outputs.contiguous() if rows_kind else outputs.long().contiguous()
        inv = None if inverse is None else inverse.to(torch.int32).contiguous()
        lab = None if targets is None else targets.long().contiguous()
        lut32 = None if lut is None else lut.to(torch.int32).contiguous()
        pred = torch.empty((p,), dtype=torch.int32, device=device)
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(device):
            L.check(L.lib().link_seg_vote_eval(rows.data_ptr(), _IO[outputs.dtype] if rows_kind else L.IO_F32,
                                               L.SEGEVAL_ROWS if rows_kind else L.SEGEVAL_PREDICTIONS, int(rows.shape[0]), c, ptr(inv),
                                               1 if inv is None else int(inv.shape[0]), p, ptr(lab), self.ignore_label, ptr(lut32),
                                               pred.data_ptr(), ptr(counters), L.current_stream_handle()), "link_seg_vote_eval")
        return pred.long()

    def compute(self, all_reduce: bool = True) -> dict:
        c = self.num_classes
        reduce = all_reduce and torch.distributed.is_available() and torch.distributed.is_initialized()
        if self.counters is not None:
            counters = self.counters
        else:
            # a rank that saw no step still takes part in the collective, with zeros where the backend expects them
            on_gpu = reduce and torch.distributed.get_backend() == "nccl"
            counters = torch.zeros((3, c), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()) if on_gpu else "cpu")
        if reduce:
            counters = counters.clone()
            torch.distributed.all_reduce(counters)
        return mean_iou(counters.cpu().numpy())


def mean_iou(counters: np.ndarray) -> dict:
    """callbacks.py:63-79 on int64 [3, c] = seen, positive, correct: IoU and accuracy of the classes 1..c-1 (1 where the class was
    never seen), their means, and the overall accuracy, in float64 as the reference's numpy arrays are"""
    seen, positive, correct = (counters[k, 1:].astype(np.float64) for k in range(3))
    none = seen == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ious = np.where(none, 1.0, correct / (seen + positive - correct))
        accs = np.where(none, 1.0, correct / seen)
        oacc = np.sum(correct) / np.sum(seen)
    return {"miou": float(np.mean(ious)), "macc": float(np.mean(accs)), "oacc": float(oacc), "ious": ious, "accs": accs,
            "seen": counters[0].copy(), "positive": counters[1].copy(), "correct": counters[2].copy()}
