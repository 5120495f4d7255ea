"""Checker of ibvh_closest_triangles (include/ibvh.h): a numpy restatement of the point-triangle evaluation in the INPUT dtype
(float32 inputs are never promoted: every numpy operation below rounds once, like the kernel's, which is compiled without
contraction and with a correctly rounded divide), the brute force over all triangles with the tie rule — the definition of
the result — the point-box lower bound the walk prunes with, and the query points the tests share.  Host only."""
import numpy as np

FACE, EDGES, VERTICES = (6,), (2, 4, 5), (0, 1, 3)


def _dot(x, y):
    """(x0*y0 + x1*y1) + x2*y2"""
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _min3(a, b, c):
    """BBox{T}(p1, p2, p3): `x < y ? x : y` ternaries (NaN semantics are theirs, not np.minimum's)"""
    return np.where(a < b, np.where(a < c, a, c), np.where(b < c, b, c))


def _max3(a, b, c):
    return np.where(a > b, np.where(a > c, a, c), np.where(b > c, b, c))


def _clamp(x, lo, up):
    return np.where(x < lo, lo, np.where(x > up, up, x))


def _evaluate(tri, p):
    """tri (..., 9), p (..., 3) of ONE float dtype, broadcast against each other -> q (..., 3), d2 (...), region (...)"""
    dt = tri.dtype
    assert dt in (np.float32, np.float64) and p.dtype == dt, (tri.dtype, p.dtype)
    a, b, c = tri[..., 0:3], tri[..., 3:6], tri[..., 6:9]
    one = dt.type(1)
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        cases = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        region = np.select(cases, [0, 1, 2, 3, 4, 5], 6).astype(np.int8)
        v2 = (d1 / (d1 - d3))[..., None]
        w4 = (d2 / (d2 - d6))[..., None]
        w5 = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
        den = one / ((va + vb) + vc)
        v6, w6 = (vb * den)[..., None], (vc * den)[..., None]
        shape = region.shape + (3,)
        full = lambda x: np.broadcast_to(x, shape)
        r = region[..., None]
        q = np.where(r == 0, full(a), np.where(r == 1, full(b), np.where(r == 2, a + v2 * ab, np.where(
            r == 3, full(c), np.where(r == 4, a + w4 * ac, np.where(r == 5, b + w5 * (c - b), (a + v6 * ab) + w6 * ac))))))
        q = _clamp(q, _min3(a, b, c), _max3(a, b, c))
        e = p - q
        dist2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    assert q.dtype == dt and dist2.dtype == dt  # nothing was promoted on the way
    return q, dist2, region


def evaluate(tris, p, chunk=128):
    """tris (n, 9), p (m, 3) -> q (m, n, 3), d2 (m, n), region (m, n) for ALL pairs, `chunk` points at a time"""
    m, n = len(p), len(tris)
    q = np.empty((m, n, 3), tris.dtype)
    d2 = np.empty((m, n), tris.dtype)
    region = np.empty((m, n), np.int8)
    for s in range(0, m, chunk):
        q[s:s + chunk], d2[s:s + chunk], region[s:s + chunk] = _evaluate(tris[None], p[s:s + chunk, None, :])
    return q, d2, region


class Closest:
    """index (m,) of `idt` (0 = none), d2 (m,) (+Inf = none), point (m, 3) (0 = none), region (m,) (-1 = none),
    ties (m,): how many qualifying triangles share the winner's d2 (0 = none)."""


def brute_force(tris, p, max_d2=None, idt=np.int32, chunk=128):
    """The definition of the result: per point the lexicographic minimum of (d2_k, k) over all k with d2_k <= max_d2
    (every comparison false on NaN); max_d2 None = +Inf."""
    dt = tris.dtype
    max_d2 = dt.type(np.inf) if max_d2 is None else dt.type(max_d2)
    m = len(p)
    out = Closest()
    out.index = np.zeros(m, idt)
    out.d2 = np.full(m, np.inf, dt)
    out.point = np.zeros((m, 3), dt)
    out.region = np.full(m, -1, np.int8)
    out.ties = np.zeros(m, np.int64)
    for s in range(0, m, chunk):
        q, d2, region = _evaluate(tris[None], p[s:s + chunk, None, :])
        with np.errstate(invalid="ignore"):
            valid = d2 <= max_d2
        key = np.where(valid, d2, dt.type(np.inf))
        cand = valid & (key == key.min(axis=1, keepdims=True))  # (a qualifying +Inf still beats nothing)
        has = cand.any(axis=1)
        k = cand.argmax(axis=1)                                 # the first = the smallest index
        rows = np.arange(len(k))
        sl = slice(s, s + len(k))
        out.index[sl] = np.where(has, k + 1, 0)
        out.d2[sl] = np.where(has, d2[rows, k], dt.type(np.inf))
        out.point[sl] = np.where(has[:, None], q[rows, k], dt.type(0))
        out.region[sl] = np.where(has, region[rows, k], -1)
        out.ties[sl] = cand.sum(axis=1)
    return out


def box_lower_bound(lo, up, p):
    """lb(B): c = clamp(p, lo, up) per component; f = p - c; (f0*f0 + f1*f1) + f2*f2 — the operation order of d2"""
    assert lo.dtype == up.dtype == p.dtype
    with np.errstate(all="ignore"):
        f = p - _clamp(p, lo, up)
        return (f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2]


def triangle_boxes(tris):
    a, b, c = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
    return _min3(a, b, c), _max3(a, b, c)


def query_points(tris, dt, n_box=600, n_surface=200, seed=7):
    """n_box points uniform in the mesh's box inflated by 25 % each way, then n_surface points ON the surface: random
    barycentric points of random triangles, computed in float64 and rounded to `dt`.  (n_box + n_surface, 3) of `dt`."""
    rng = np.random.default_rng(seed)
    t64 = tris.astype(np.float64)
    v = t64.reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = hi - lo
    box = (lo - 0.25 * ext) + 1.5 * ext * rng.random((n_box, 3))
    k = rng.integers(0, len(tris), n_surface)
    w = rng.dirichlet((1.0, 1.0, 1.0), n_surface)
    surf = (w[:, :, None] * t64[k].reshape(-1, 3, 3)).sum(axis=1)
    return np.concatenate([box, surf]).astype(dt)


def region_counts(region):
    """winners by class: (face, edges, vertices)"""
    return tuple(int(np.isin(region, cls).sum()) for cls in (FACE, EDGES, VERTICES))
