"""Checker of ibvh_nearest_leaves (include/ibvh.h): a numpy brute force of the DEFINITION of the answer, in the leaf float
type, every operation its own numpy operation (so each rounds once, nothing fused): the centre of every leaf's volume, its
squared distance to every query point in dist3sq's order, and per point the k lexicographically smallest (d2, index) among
the leaves with d2 <= max_d2 — a stable lexicographic sort, comparisons false on NaN.  Unfilled slots hold 0 / +Inf.  A
plain module (no tests, no fixtures): tests/test_host_nearest_leaves.py checks it against a naive per-point loop of its own,
tests/test_gpu_nearest_leaves.py pins the kernel to it bit for bit."""
import numpy as np


def centers(volumes):
    """(n, 4) spheres (x, r) -> x (bsphere.jl:142); (n, 6) boxes (lo, up) -> T(0.5) * (lo + up) (bbox.jl:100-102)"""
    v = np.asarray(volumes)
    assert v.ndim == 2 and v.shape[1] in (4, 6) and v.dtype in (np.float32, np.float64)
    if v.shape[1] == 4:
        return v[:, :3].copy()
    with np.errstate(all="ignore"):
        s = v[:, :3] + v[:, 3:]
        return v.dtype.type(0.5) * s


def leaf_boxes(volumes):
    """the box the walk bounds a leaf with: a sphere's x -/+ r in the leaf float type (merge.jl:47-51), a box itself"""
    v = np.asarray(volumes)
    if v.shape[1] == 6:
        return v[:, :3], v[:, 3:]
    with np.errstate(all="ignore"):
        return v[:, :3] - v[:, 3:4], v[:, :3] + v[:, 3:4]


def distances2(c, p):
    """(m, n) d2 of every point to every centre: e = p - c; (e0*e0 + e1*e1) + e2*e2, each operation rounded once"""
    assert c.dtype == p.dtype and c.shape[1] == 3 and p.shape[1] == 3
    with np.errstate(all="ignore"):
        e0 = p[:, None, 0] - c[None, :, 0]
        e1 = p[:, None, 1] - c[None, :, 1]
        e2 = p[:, None, 2] - c[None, :, 2]
        s0 = e0 * e0
        s1 = e1 * e1
        s2 = e2 * e2
        s01 = s0 + s1
        return s01 + s2


def box_lower_bound(lo, up, p):
    """lb(B) of include/ibvh.h for broadcastable lo, up, p (..., 3): clamp, subtract, square, add — d2's operation order"""
    with np.errstate(all="ignore"):
        c = np.where(p < lo, lo, np.where(p > up, up, p))
        f = p - c
        s0 = f[..., 0] * f[..., 0]
        s1 = f[..., 1] * f[..., 1]
        s2 = f[..., 2] * f[..., 2]
        s01 = s0 + s1
        return s01 + s2


class Nearest:
    """index (m, k), d2 (m, k) as the entry point returns them; count (m,) answers per row; ties (m,) among the leaves
    that are answers or tied with the last answer, how many repeat a d2 already seen (> 0: the smaller-index rule decided the
    order of the row, or what entered it)"""


def brute_force(volumes, indices, points, k, max_d2=None, idt=np.int32):
    v = np.asarray(volumes)
    dt = v.dtype.type
    p = np.ascontiguousarray(points, dtype=v.dtype)
    idx = np.asarray(indices).astype(np.int64)
    n, m = len(v), len(p)
    assert idx.shape == (n,) and k >= 1
    max_d2 = dt(np.inf) if max_d2 is None else dt(max_d2)
    d2 = distances2(centers(v), p)
    with np.errstate(invalid="ignore"):
        valid = d2 <= max_d2                                   # false on NaN, of d2 or of the radius
    key = np.where(valid, d2, dt(np.inf))
    idx2 = np.broadcast_to(idx[None, :], d2.shape)
    # stable lexicographic sort, per row: not-valid last, then d2, then index (np.lexsort: the LAST key is the primary one)
    order = np.lexsort((idx2, key, ~valid), axis=1)[:, :k]
    rows = np.arange(m)[:, None]
    count = np.minimum(valid.sum(axis=1), k)
    filled = np.arange(order.shape[1])[None, :] < count[:, None]
    out = Nearest()
    out.index = np.zeros((m, k), idt)
    out.d2 = np.full((m, k), np.inf, v.dtype)
    kk = order.shape[1]                                        # min(k, n)
    out.index[:, :kk] = np.where(filled, idx2[rows, order], 0).astype(idt)
    out.d2[:, :kk] = np.where(filled, d2[rows, order], dt(np.inf))
    out.count = count
    last = np.where(count > 0, d2[np.arange(m), order[np.arange(m), np.maximum(count, 1) - 1]], dt(np.nan))
    with np.errstate(invalid="ignore"):
        sel = valid & (d2 <= last[:, None])                    # the answers and everything tied with the last one
    n_sel = sel.sum(axis=1)
    s = np.sort(np.where(sel, d2, dt(np.inf)), axis=1)
    differ = (s[:, 1:] != s[:, :-1]) & (np.arange(1, n)[None, :] < n_sel[:, None])
    out.ties = n_sel - ((n_sel > 0) + differ.sum(axis=1))
    return out
