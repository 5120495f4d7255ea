"""Checker of ibvh_triangle_distances (include/ibvh.h): a numpy restatement of the pair evaluation in the INPUT dtype (float32
inputs are never promoted: every numpy operation below rounds once, like the kernel's) — the cut rule on
triangle_contacts_checker's edge tests, the fifteen candidates on closest_point_checker's point-triangle evaluation and the
segment-segment evaluation stated here —, the brute force over ALL pairs with the tie rule — the definition of the result —,
the box-box bound the walk prunes with, an independent float64 certificate, and the inputs the tests share.  Host only."""
import functools

import numpy as np

import closest_point_checker as cpc
import triangle_contacts_checker as tcc
from closest_point_checker import _clamp, _dot

CUT = 15
EDGES = ((0, 3), (3, 6), (6, 0))   # where an edge's two ends start in a row of nine: ab / p1p2, bc / p2p3, ca / p3p1


def _unit(x):
    zero, one = x.dtype.type(0), x.dtype.type(1)
    return np.where(x < 0, zero, np.where(x > 1, one, x))


def closest_on_segments(p1, q1, p2, q2):
    """the segments p1 -> q1 and p2 -> q2, (..., 3) of ONE float dtype, broadcast against each other -> x1, x2 (..., 3), d2 (...)"""
    dt = p1.dtype
    assert dt in (np.float32, np.float64) and q1.dtype == p2.dtype == q2.dtype == dt
    zero = dt.type(0)
    with np.errstate(all="ignore"):
        d1, d2v, r = q1 - p1, q2 - p2, p1 - p2
        A, E, F = _dot(d1, d1), _dot(d2v, d2v), _dot(d2v, r)
        Cc, B = _dot(d1, r), _dot(d1, d2v)
        den = A * E - B * B
        s_in = np.where(den > 0, _unit((B * F - Cc * E) / den), zero)
        t_in = (B * s_in + F) / E
        s_lo, s_up = _unit(-Cc / A), _unit((B - Cc) / A)
        s_gen = np.where(t_in < 0, s_lo, np.where(t_in > 1, s_up, s_in))
        t_gen = _unit(t_in)
        s = np.where(A == 0, zero, np.where(E == 0, s_lo, s_gen))
        t = np.where(A == 0, np.where(E != 0, _unit(F / E), zero), np.where(E == 0, zero, t_gen))
        x1 = _clamp(p1 + s[..., None] * d1, np.where(p1 < q1, p1, q1), np.where(p1 > q1, p1, q1))
        x2 = _clamp(p2 + t[..., None] * d2v, np.where(p2 < q2, p2, q2), np.where(p2 > q2, p2, q2))
        e = x1 - x2
        dist2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    assert x1.dtype == x2.dtype == dist2.dtype == dt   # nothing was promoted on the way
    return x1, x2, dist2


def candidates(q, k):
    """q, k (..., 9) of ONE float dtype, broadcast against each other -> the candidate rule's (d2, xQ, xK, kind): candidate 0
    starts the result, a later one replaces it iff its d2 is strictly smaller"""
    shape = np.broadcast_shapes(q.shape[:-1], k.shape[:-1])
    best = None
    for c in range(15):
        if c < 3:      # a vertex of Q against K
            v = q[..., 3 * c:3 * c + 3]
            x, d2, _ = cpc._evaluate(k, v)
            xq, xk = v, x
        elif c < 6:    # a vertex of K against Q
            v = k[..., 3 * (c - 3):3 * (c - 3) + 3]
            x, d2, _ = cpc._evaluate(q, v)
            xq, xk = x, v
        else:          # edge i of Q against edge j of K
            (i0, i1), (j0, j1) = EDGES[(c - 6) // 3], EDGES[(c - 6) % 3]
            xq, xk, d2 = closest_on_segments(q[..., i0:i0 + 3], q[..., i1:i1 + 3], k[..., j0:j0 + 3], k[..., j1:j1 + 3])
        d2, xq, xk = np.broadcast_to(d2, shape), np.broadcast_to(xq, shape + (3,)), np.broadcast_to(xk, shape + (3,))
        if best is None:
            best = [d2.copy(), xq.copy(), xk.copy(), np.zeros(shape, np.uint8)]
            continue
        with np.errstate(invalid="ignore"):
            better = d2 < best[0]
        best[0][better], best[1][better], best[2][better], best[3][better] = d2[better], xq[better], xk[better], c
    return tuple(best)


def boxes_apart(qlo, qup, lo, up):
    """six strict comparisons, each false on NaN; (..., 3) each, broadcast against each other"""
    with np.errstate(invalid="ignore"):
        return ((qup < lo) | (qlo > up)).any(axis=-1)


def cut_rule(q, k):
    """q, k (P, 9): P pairs -> (decided (P,) bool, the point (P, 3)): under the box clause on the two EXACT boxes, the first of
    triangle_contacts' six edge tests that hits"""
    qlo, qup = tcc.fold_box(q)
    klo, kup = tcc.fold_box(k)
    near = ~boxes_apart(qlo, qup, klo, kup)
    mask, points = tcc.six_tests(q[near], k[near])
    decided = np.zeros(len(q), bool)
    point = np.zeros((len(q), 3), q.dtype)
    decided[near] = mask != 0
    point[near] = points[:, 0]
    return decided, point


def pairs(q, k):
    """q, k (P, 9): P pairs -> (d2 (P,), xQ (P, 3), xK (P, 3), kind (P,) uint8): the evaluation of include/ibvh.h, both rules"""
    d2, xq, xk, kind = candidates(q, k)
    cut, x = cut_rule(q, k)
    d2[cut], xq[cut], xk[cut], kind[cut] = 0, x[cut], x[cut], CUT
    return d2, xq, xk, kind


def box_bound(lo, up, qlo, qup):
    """g_k = max(0, lo_k - qup_k, qlo_k - up_k), both differences rounded; (g0*g0 + g1*g1) + g2*g2 — d2's operation order"""
    assert lo.dtype == up.dtype == qlo.dtype == qup.dtype
    with np.errstate(all="ignore"):
        below, above = lo - qup, qlo - up
        m = np.where(below > above, below, above)
        g = np.where(m > 0, m, m.dtype.type(0))
        return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


class Distances:
    """index (m,) of `idt` (0 = none), d2 (m,) (+Inf = none), point_query, point_mesh (m, 3) (0 = none), kind (m,) uint8
    (0 = none), ties (m,): how many qualifying triangles share the winner's d2 (0 = none)."""


def brute_force(tris, queries, max_d2=None, skip_shared=False, idt=np.int64, chunk=64):
    """The definition of the result.  tris (n, 9), queries (m, 9) of ONE float dtype: per query the lexicographic minimum of
    (d2, index) over ALL triangles with d2 <= max_d2 (every comparison false on NaN; None = +Inf) and, with skip_shared, no
    vertex equal to one of the query's.  A query with a NaN coordinate has no answer."""
    dt = tris.dtype
    queries = queries.reshape(len(queries), 9)
    assert dt in (np.float32, np.float64) and queries.dtype == dt, (dt, queries.dtype)
    n, m = len(tris), len(queries)
    max_d2 = dt.type(np.inf) if max_d2 is None else dt.type(max_d2)
    out = Distances()
    out.index, out.d2 = np.zeros(m, idt), np.full(m, np.inf, dt)
    out.point_query, out.point_mesh = np.zeros((m, 3), dt), np.zeros((m, 3), dt)
    out.kind, out.ties = np.zeros(m, np.uint8), np.zeros(m, np.int64)
    alive = ~np.isnan(queries).any(axis=1)
    klo, kup = tcc.fold_box(tris)
    qlo, qup = tcc.fold_box(queries)
    for s in range(0, m if n else 0, chunk):
        sl = slice(s, min(s + chunk, m))
        q = queries[sl]
        d2, xq, xk, kind = candidates(q[:, None, :], tris[None])
        # the cut rule, on the pairs whose exact boxes are not apart
        rows, cols = np.nonzero(~boxes_apart(qlo[sl, None], qup[sl, None], klo[None], kup[None]))
        mask, points = tcc.six_tests(q[rows], tris[cols])
        cut = mask != 0
        rows, cols = rows[cut], cols[cut]
        d2[rows, cols], xq[rows, cols], xk[rows, cols], kind[rows, cols] = 0, points[cut, 0], points[cut, 0], CUT
        with np.errstate(invalid="ignore"):
            valid = (d2 <= max_d2) & alive[sl, None]
        if skip_shared:
            for r in range(len(q)):
                valid[r] &= ~tcc.shares_vertex(np.broadcast_to(q[r], tris.shape), tris)
        key = np.where(valid, d2, dt.type(np.inf))
        cand = valid & (key == key.min(axis=1, keepdims=True))   # (a qualifying +Inf still beats nothing)
        has = cand.any(axis=1)
        j = cand.argmax(axis=1)                                  # the first = the smallest index
        r = np.arange(len(j))
        out.index[sl] = np.where(has, j + 1, 0)
        out.d2[sl] = np.where(has, d2[r, j], dt.type(np.inf))
        out.point_query[sl] = np.where(has[:, None], xq[r, j], dt.type(0))
        out.point_mesh[sl] = np.where(has[:, None], xk[r, j], dt.type(0))
        out.kind[sl] = np.where(has, kind[r, j], 0)
        out.ties[sl] = cand.sum(axis=1)
    return out


def limited(bf, max_d2):
    """the unbounded result `bf` under a radius: the winner if its d2 <= max_d2, else none (the lexicographic minimum of a
    subset that is cut off by d2 alone)"""
    dt = bf.d2.dtype
    keep = (bf.index != 0) & (bf.d2 <= dt.type(max_d2))
    out = Distances()
    out.index, out.d2 = np.where(keep, bf.index, 0).astype(bf.index.dtype), np.where(keep, bf.d2, dt.type(np.inf))
    out.point_query, out.point_mesh = np.where(keep[:, None], bf.point_query, dt.type(0)), np.where(keep[:, None], bf.point_mesh, dt.type(0))
    out.kind, out.ties = np.where(keep, bf.kind, 0).astype(np.uint8), np.where(keep, bf.ties, 0)
    return out


def global_minimum(bf):
    """what mesh_distance reports -> (d2, 1-based query position, index): the smallest d2, among equal ones the lowest query
    position; (inf, 0, 0) when no query has an answer"""
    if not (bf.index != 0).any():
        return np.inf, 0, 0
    pos = int(np.flatnonzero(bf.d2 == bf.d2.min())[0])
    return bf.d2[pos], pos + 1, int(bf.index[pos])


# ---- the independent certificate ---------------------------------------------------------------------------------------
def certificate(q, k, xq, xk):
    """float64, for P pairs with a positive distance -> (on, sep), each (P,): how far, relative to the pair's extent, xQ and xK
    lie from their triangles (the residual of the barycentric fit, and how far the coordinates leave the simplex), and the
    deviation from |n| of the gap by which n = xQ - xK separates the two triangles' vertex projections, relative to the pair's
    extent too.  Two convex sets, points x and y of them: |x - y| is the distance iff the direction x - y separates them by
    exactly |x - y|.  (Relative to the extent, not to |n|: the points carry a rounding error that is a fraction of the
    coordinates' size however small the gap, so a deviation relative to |n| has no bound as pairs approach touching.)"""
    q, k, xq, xk = (np.asarray(a, np.float64) for a in (q, k, xq, xk))
    extent = np.concatenate([q, k], axis=1).reshape(len(q), 6, 3)
    extent = np.linalg.norm(extent.max(axis=1) - extent.min(axis=1), axis=1)

    def off(tri, x):
        a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
        out = np.empty(len(tri))
        for i in range(len(tri)):
            basis = np.stack([b[i] - a[i], c[i] - a[i]], axis=1)
            (u, v), *_ = np.linalg.lstsq(basis, x[i] - a[i], rcond=None)
            resid = np.linalg.norm(basis @ np.array([u, v]) - (x[i] - a[i]))
            out[i] = max(resid / extent[i], -u, -v, u + v - 1, 0.0)
        return out
    n = xq - xk
    length = np.linalg.norm(n, axis=1)
    proj = lambda tri: np.einsum("pvk,pk->pv", tri.reshape(-1, 3, 3), n)
    gap = (proj(q).min(axis=1) - proj(k).max(axis=1)) / length
    return np.maximum(off(q, xq), off(k, xk)), np.abs(gap - length) / extent


# ---- the shared inputs -------------------------------------------------------------------------------------------------
def random_pairs(dt, n=4000, seed=41):
    """n pairs of random triangles in the unit cube, K shifted by up to 1.5 along a random direction: apart, close and cutting"""
    rng = np.random.default_rng(seed)
    q = rng.random((n, 9))
    k = rng.random((n, 9)) + np.repeat(rng.normal(size=(n, 3)) * rng.random((n, 1)) * 0.9, 3, axis=0).reshape(n, 9)
    return q.astype(dt), k.astype(dt)


def mesh_queries(tris, dt, n=600, seed=43):
    """n query triangles taken from the mesh itself, moved three ways: a third from the mesh rotated and shifted so that it cuts
    the mesh (triangle_contacts_checker.other; half of them triangles that do cut it, half whatever comes), a third shifted
    clear of it by about two mean edge lengths along z, a third far away -> (n, 9) of `dt`"""
    from sphere_contacts_checker import mean_edge
    rng = np.random.default_rng(seed)
    third = n // 3
    t64 = tris.astype(np.float64)
    moved = tcc.other(t64)
    cuts = np.flatnonzero(tcc.brute_force(t64, moved).counts > 0)
    cutting = moved[np.concatenate([rng.choice(cuts, third // 2, replace=False), rng.choice(len(tris), third - third // 2, replace=False)])]
    pick = rng.choice(len(tris), n - third, replace=False)
    height = t64.reshape(-1, 3)[:, 2].max() - t64.reshape(-1, 3)[:, 2].min()
    clear = t64[pick[:third]] + np.tile([0.013, 0.007, height + 2 * mean_edge(t64)], 3)
    far = t64[pick[third:]] * 0.5 + np.tile([40.0, -25.0, 30.0], 3)
    return np.concatenate([cutting, clear, far]).astype(dt)


@functools.lru_cache(maxsize=None)
def reference(mesh, dt, n=600):
    """(triangles, queries, the unbounded brute force) of a named mesh, computed once and read-only"""
    import mesh_query_kit as kit
    from implicitbvh_amd.synthetic import torus_mesh
    tris = torus_mesh(*kit.MESHES[mesh]).astype(dt)
    queries = mesh_queries(tris, dt, n)
    bf = brute_force(tris, queries)
    for a in (tris, queries) + tuple(vars(bf).values()):
        a.setflags(write=False)
    return tris, queries, bf
