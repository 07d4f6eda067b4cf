"""tests/box_oracle.py -- checkers of the detection post-processing kernels (csrc/boxnms.hip), in numpy.  Test infrastructure only.

box_overlap / iou_bev restate the reference's routine statement by statement (detection/det3d/ops/iou3d_nms/src/
iou3d_nms_kernel.cu:35-234 and its CPU twin iou3d_cpu.cpp:59-229), evaluated in float32 (every product and sum rounded on its own, as
the host compiler of the CPU twin does) or in float64.  Every statement is the scalar routine's, applied to P pairs at once:
arrays of shape [P] stand where the routine has a float, and the point list is [P, 24] with the routine's order of insertion.
greedy_from_words is iou3d_nms.cpp:116-132, greedy_nms the same rule on a boolean matrix, circle_nms circle_nms_jit.py:5-28.
"""
import numpy as np

EPS = 1e-8           # iou3d_nms_kernel.cu:14
MARGIN = 1e-2        # :53
NPTS = 24            # 16 crossings + 8 corners (the reference's list holds 16 and overflows past that)


def _trig(h, dt):
    """cos / sin of an angle as the host libm's float routines give them for float32 (computed in double and rounded once),
    in double for float64"""
    return np.cos(h.astype(np.float64)).astype(dt), np.sin(h.astype(np.float64)).astype(dt)


def _corners(box, dt):
    """:108-149 -> ([P, 4] x, [P, 4] y) of the rotated corners"""
    x, y, dx, dy, h = (box[:, k].astype(dt) for k in (0, 1, 3, 4, 6))
    two = dt(2)
    dxh, dyh = dx / two, dy / two
    x1, y1, x2, y2 = x - dxh, y - dyh, x + dxh, y + dyh
    c, s = _trig(h, dt)
    px, py = [x1, x2, x2, x1], [y1, y1, y2, y2]
    cx = np.stack([(px[k] - x) * c + (py[k] - y) * (-s) + x for k in range(4)], 1)          # rotate_around_center :94-98
    cy = np.stack([(px[k] - x) * s + (py[k] - y) * c + y for k in range(4)], 1)
    return cx, cy


def _cross(p1x, p1y, p2x, p2y, p0x, p0y):
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y)                            # :39-41


def _in_box(box, px, py, dt, margin):
    """check_in_box2d :51-61"""
    x, y, dx, dy, h = (box[:, k].astype(dt) for k in (0, 1, 3, 4, 6))
    c, s = _trig(-h, dt)
    rx = (px - x) * c + (py - y) * (-s)
    ry = (px - x) * s + (py - y) * c
    return (np.abs(rx) < dx / dt(2) + dt(margin)) & (np.abs(ry) < dy / dt(2) + dt(margin))


def box_overlap(a, b, dtype=np.float32, margin=MARGIN, cross_eps=0.0, return_count=False):
    """box_overlap(:104-225) of the pairs (a[p], b[p]).  margin / cross_eps vary the two strict inequalities that decide which
    points exist (the stability probes of the fixture generator); the defaults are the reference's."""
    dt = np.dtype(dtype).type
    a = np.asarray(a).reshape(-1, 7)
    b = np.asarray(b).reshape(-1, 7)
    P = a.shape[0]
    with np.errstate(all="ignore"):
        acx, acy = _corners(a, dt)
        bcx, bcy = _corners(b, dt)
        px = np.zeros((P, NPTS), dt)
        py = np.zeros((P, NPTS), dt)
        valid = np.zeros((P, NPTS), bool)
        for i in range(4):
            for j in range(4):
                p1x, p1y, p0x, p0y = acx[:, (i + 1) & 3], acy[:, (i + 1) & 3], acx[:, i], acy[:, i]
                q1x, q1y, q0x, q0y = bcx[:, (j + 1) & 3], bcy[:, (j + 1) & 3], bcx[:, j], bcy[:, j]
                rect = ((np.minimum(p0x, p1x) <= np.maximum(q0x, q1x)) & (np.minimum(q0x, q1x) <= np.maximum(p0x, p1x)) &
                        (np.minimum(p0y, p1y) <= np.maximum(q0y, q1y)) & (np.minimum(q0y, q1y) <= np.maximum(p0y, p1y)))      # :43-49
                s1 = _cross(q0x, q0y, p1x, p1y, p0x, p0y)                                                                     # :68-71
                s2 = _cross(p1x, p1y, q1x, q1y, p0x, p0y)
                s3 = _cross(p0x, p0y, q1x, q1y, q0x, q0y)
                s4 = _cross(q1x, q1y, p1x, p1y, q0x, q0y)
                ok = rect & (s1 * s2 > dt(cross_eps)) & (s3 * s4 > dt(cross_eps))                                             # :73
                s5 = _cross(q1x, q1y, p1x, p1y, p0x, p0y)
                ax = (s5 * q0x - s1 * q1x) / (s5 - s1)                                                                        # :78-79
                ay = (s5 * q0y - s1 * q1y) / (s5 - s1)
                a0, b0, c0 = p0y - p1y, p1x - p0x, p0x * p1y - p1x * p0y                                                      # :83-88
                a1, b1, c1 = q0y - q1y, q1x - q0x, q0x * q1y - q1x * q0y
                D = a0 * b1 - a1 * b0
                near = ~(np.abs(s5 - s1) > dt(EPS))
                ax = np.where(near, (b0 * c1 - b1 * c0) / D, ax)
                ay = np.where(near, (a1 * c0 - a0 * c1) / D, ay)
                px[:, i * 4 + j], py[:, i * 4 + j], valid[:, i * 4 + j] = ax, ay, ok
        for k in range(4):                                                                                                    # :177-194
            px[:, 16 + 2 * k], py[:, 16 + 2 * k] = bcx[:, k], bcy[:, k]
            valid[:, 16 + 2 * k] = _in_box(a, bcx[:, k], bcy[:, k], dt, margin)
            px[:, 17 + 2 * k], py[:, 17 + 2 * k] = acx[:, k], acy[:, k]
            valid[:, 17 + 2 * k] = _in_box(b, acx[:, k], acy[:, k], dt, margin)
        sx, sy = np.zeros(P, dt), np.zeros(P, dt)
        for s in range(NPTS):                                        # the centroid's sum in the order of insertion
            sx = np.where(valid[:, s], sx + px[:, s], sx)
            sy = np.where(valid[:, s], sy + py[:, s], sy)
        cnt = valid.sum(1)
        mx, my = sx / cnt.astype(dt), sy / cnt.astype(dt)                                                                     # :196-197
        key = np.arctan2((py - my[:, None]).astype(np.float64), (px - mx[:, None]).astype(np.float64)).astype(dt)             # :100-102
        key = np.where(valid, key, np.inf)
        order = np.argsort(key, axis=1, kind="stable")              # what the bubble sort of :201-209 (swap on a strict >) leaves
        px, py = np.take_along_axis(px, order, 1), np.take_along_axis(py, order, 1)
        area = np.zeros(P, dt)
        for k in range(NPTS - 1):                                                                                             # :219-222
            t = (px[:, k] - px[:, 0]) * (py[:, k + 1] - py[:, 0]) - (py[:, k] - py[:, 0]) * (px[:, k + 1] - px[:, 0])
            area = np.where(k + 1 < cnt, area + t, area)
        out = np.abs(area) / dt(2)
    return (out, cnt) if return_count else out


def iou_bev(a, b, dtype=np.float32, **kw):
    """:227-234"""
    dt = np.dtype(dtype).type
    a = np.asarray(a).reshape(-1, 7)
    b = np.asarray(b).reshape(-1, 7)
    ov = box_overlap(a, b, dtype, **kw)
    sa = a[:, 3].astype(dt) * a[:, 4].astype(dt)
    sb = b[:, 3].astype(dt) * b[:, 4].astype(dt)
    return ov / np.maximum(sa + sb - ov, dt(EPS))


def pairs_matrix(fn, a, b, chunk=1 << 17, **kw):
    """fn over all pairs -> [na, nb]"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = a.shape[0], b.shape[0]
    ii, jj = np.divmod(np.arange(na * nb), max(nb, 1))
    out = None
    for s in range(0, na * nb, chunk):
        r = fn(a[ii[s:s + chunk]], b[jj[s:s + chunk]], **kw)
        if out is None:
            out = np.zeros(na * nb, r.dtype)
        out[s:s + chunk] = r
    if out is None:
        out = np.zeros(0, np.float32)
    return out.reshape(na, nb)


def iou_normal(a, b, dtype=np.float32):
    """:314-325"""
    dt = np.dtype(dtype).type
    a = np.asarray(a).reshape(-1, 7).astype(dt)
    b = np.asarray(b).reshape(-1, 7).astype(dt)
    two = dt(2)
    left = np.maximum(a[:, 0] - a[:, 3] / two, b[:, 0] - b[:, 3] / two)
    right = np.minimum(a[:, 0] + a[:, 3] / two, b[:, 0] + b[:, 3] / two)
    top = np.maximum(a[:, 1] - a[:, 4] / two, b[:, 1] - b[:, 4] / two)
    bottom = np.minimum(a[:, 1] + a[:, 4] / two, b[:, 1] + b[:, 4] / two)
    inter = np.maximum(right - left, dt(0)) * np.maximum(bottom - top, dt(0))
    return inter / np.maximum(a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - inter, dt(EPS))


def centre_dist2(a, b, dtype=np.float32):
    """circle_nms_jit.py:23"""
    dt = np.dtype(dtype).type
    a = np.asarray(a).astype(dt)
    b = np.asarray(b).astype(dt)
    ddx, ddy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    return ddx * ddx + ddy * ddy


def pack_mask(sup):
    """boolean [n, n] (sup[i, j] = i suppresses j) -> the kernels' words uint64[n, ceil(n / 64)], bits j > i only"""
    n = sup.shape[0]
    nblk = (n + 63) // 64
    m = np.triu(np.asarray(sup, bool), 1)
    pad = np.zeros((n, nblk * 64), bool)
    pad[:, :n] = m
    w = (pad.reshape(n, nblk, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64)
    return w


def greedy_from_words(words, n, post_max=None):
    """iou3d_nms.cpp:116-132 on mask words uint64[n, stride] (only the words j >= i / 64 of row i are read)"""
    words = np.asarray(words, np.uint64)
    nblk = (n + 63) // 64
    remv = np.zeros(nblk, np.uint64)
    keep = []
    one = np.uint64(1)
    for i in range(n):
        if post_max is not None and len(keep) >= post_max:
            break
        nb, ib = divmod(i, 64)
        if not (remv[nb] >> np.uint64(ib)) & one:
            keep.append(i)
            remv[nb:] |= words[i, nb:nblk]
    return np.asarray(keep, np.int64)


def greedy_nms(sup, post_max=None):
    """the same rule on a boolean matrix: walk the boxes in order, keep what no kept box suppresses"""
    sup = np.asarray(sup, bool)
    n = sup.shape[0]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if post_max is not None and len(keep) >= post_max:
            break
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= sup[i, i + 1:]
    return np.asarray(keep, np.int64)


def circle_nms(dets, thresh):
    """circle_nms_jit.py:5-28: dets [n, 3] = x, y, score -> kept indices into dets, best first"""
    dets = np.asarray(dets)
    order = dets[:, 2].argsort()[::-1]
    n = dets.shape[0]
    suppressed = np.zeros(n, bool)
    keep = []
    for _i in range(n):
        i = order[_i]
        if suppressed[i]:
            continue
        keep.append(int(i))
        rest = order[_i + 1:]
        dist = (dets[i, 0] - dets[rest, 0]) ** 2 + (dets[i, 1] - dets[rest, 1]) ** 2
        suppressed[rest[dist <= thresh]] = True
    return np.asarray(keep, np.int64)


def to_pcdet(boxes):
    """iou3d_nms_utils.py:29-33 / box_torch_ops.py:255-257 in float32"""
    b = np.asarray(boxes, np.float32)[:, [0, 1, 2, 4, 3, 5, 6]].copy()
    b[:, 6] = -b[:, 6] - np.float32(np.pi / 2)
    return b
