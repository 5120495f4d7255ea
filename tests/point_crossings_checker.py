"""Checker of ibvh_point_crossings (include/ibvh.h): a numpy restatement of rules 1 to 4 — guard, canonical edges, orientation,
depth — in the INPUT dtype (float32 inputs are never promoted: every numpy operation below rounds once, like the kernel's,
which is compiled without contraction), all points times all triangles; the brute force over all triangles — the definition
of the result; the uncanonicalised rule it is compared against on the host; the analytic inside test of torus_mesh; the
guard on a box, which is what the walk prunes with; and the query points the tests share.  Host only."""
import numpy as np

from closest_point_checker import _max3, _min3, triangle_boxes  # noqa: F401  (the `x < y ? x : y` ternaries of BBox{T}(p1, p2, p3))


def cyclic(axis):
    """u, v, w = (axis + 1) % 3, (axis + 2) % 3, axis: cyclic, so orientation is preserved"""
    assert axis in (0, 1, 2)
    return (axis + 1) % 3, (axis + 2) % 3, axis


def _edge_side(x, y, p, canonical=True):
    """side of p (u, v) of the directed edge x -> y, all in (u, v, w): the edge function on the CANONICAL pair, a tie goes
    left of the canonical edge, the answer turned back for a flipped edge.  canonical=False: the edge as given, e >= 0."""
    if canonical:
        flipped = (y[..., 0] < x[..., 0]) | ((y[..., 0] == x[..., 0]) & (
            (y[..., 1] < x[..., 1]) | ((y[..., 1] == x[..., 1]) & (y[..., 2] < x[..., 2]))))
        f = flipped[..., None]
        x, y = np.where(f, y, x), np.where(f, x, y)
    else:
        flipped = np.zeros(np.broadcast(x[..., 0], y[..., 0]).shape, bool)
    e = (y[..., 0] - x[..., 0]) * (p[..., 1] - x[..., 1]) - (y[..., 1] - x[..., 1]) * (p[..., 0] - x[..., 0])
    assert e.dtype == p.dtype
    return (e >= 0) ^ flipped


def _evaluate(tri, p, axis, canonical=True):
    """tri (..., 9), p (..., 3) of ONE float dtype, broadcast against each other -> hit (...) bool, sign (...) int8: +1 a
    ccw crossing, -1 a cw one, 0 none"""
    dt = tri.dtype
    assert dt in (np.float32, np.float64) and p.dtype == dt, (tri.dtype, p.dtype)
    perm = list(cyclic(axis))
    a, b, c = tri[..., 0:3][..., perm], tri[..., 3:6][..., perm], tri[..., 6:9][..., perm]
    p = p[..., perm]
    with np.errstate(all="ignore"):
        lo, up = _min3(a, b, c), _max3(a, b, c)
        guard = ((p[..., 0] >= lo[..., 0]) & (p[..., 0] <= up[..., 0]) & (p[..., 1] >= lo[..., 1]) & (p[..., 1] <= up[..., 1])
                 & (up[..., 2] >= p[..., 2]))
        s0, s1, s2 = (_edge_side(x, y, p, canonical) for x, y in ((a, b), (b, c), (c, a)))
        ccw, cw = s0 & s1 & s2, ~(s0 | s1 | s2)
        ab, ac, d = b - a, c - a, p - a
        n0 = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1]
        n1 = ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2]
        n2 = ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
        s = (n0 * d[..., 0] + n1 * d[..., 1]) + n2 * d[..., 2]
        assert s.dtype == dt and lo.dtype == dt  # nothing was promoted on the way
        pos, neg = guard & ccw & (s < 0), guard & cw & (s > 0)
    return pos | neg, pos.astype(np.int8) - neg.astype(np.int8)


def evaluate(tris, pts, axis, chunk=128, canonical=True):
    """tris (n, 9), pts (m, 3) -> hit (m, n) bool, sign (m, n) int8 for ALL pairs, `chunk` points at a time"""
    m, n = len(pts), len(tris)
    hit, sign = np.empty((m, n), bool), np.empty((m, n), np.int8)
    for s in range(0, m, chunk):
        hit[s:s + chunk], sign[s:s + chunk] = _evaluate(tris[None], pts[s:s + chunk, None, :], axis, canonical)
    return hit, sign


class Crossings:
    """crossings (m,) of `idt`: the number of crossing triangles; winding (m,) of `idt`: ccw crossings minus cw ones"""


def _count(hit, sign, idt):
    out = Crossings()
    out.crossings = hit.sum(axis=1).astype(idt)
    out.winding = sign.sum(axis=1, dtype=np.int64).astype(idt)
    return out


def brute_force(tris, pts, axis, idt=np.int32):
    """The definition of the result: both counts over ALL triangles."""
    return _count(*evaluate(tris, pts, axis), idt)


def naive(tris, pts, axis, idt=np.int32):
    """The rule WITHOUT the canonical edge order (e >= 0 on the three edges as given): what the canonical order is there
    to repair.  For the host test only."""
    return _count(*evaluate(tris, pts, axis, canonical=False), idt)


def box_guard(lo, up, pts, axis):
    """the guard's five comparisons on a box: what the walk enters a node or a leaf on"""
    u, v, w = cyclic(axis)
    with np.errstate(invalid="ignore"):
        return ((pts[..., u] >= lo[..., u]) & (pts[..., u] <= up[..., u]) & (pts[..., v] >= lo[..., v]) & (pts[..., v] <= up[..., v])
                & (up[..., w] >= pts[..., w]))


def analytic_inside(pts):
    """For synthetic.torus_mesh, in float64 from the mesh's own formula (tube radius r(a, b) = 0.35 + 0.05 sin 7a cos 5b around
    the unit circle): inside = hypot(rho - 1, z) < r(a, b), and the distance margin | hypot(rho - 1, z) - r(a, b) |."""
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    rho = np.hypot(x, y)
    a, b = np.arctan2(y, x), np.arctan2(z, rho - 1.0)
    r = 0.35 + 0.05 * np.sin(7 * a) * np.cos(5 * b)
    t = np.hypot(rho - 1.0, z)
    return t < r, np.abs(t - r)


N_BOX, N_VERTEX_RAYS, N_VERTICES, N_CENTROIDS = 400, 200, 100, 100
BOX, VERTEX_RAYS, VERTICES, CENTROIDS = slice(0, 400), slice(400, 600), slice(600, 700), slice(700, 800)
OFF_SURFACE = np.r_[0:600, 700:800]  # everything but the mesh vertices themselves


def query_points(tris, dt, axis, seed=3):
    """800 points of `dt` for rays along `axis`: 400 uniform in the mesh's box inflated by 0.1; 200 vertex rays — a random
    vertex's u and v kept BIT FOR BIT, w redrawn across the inflated span; 100 mesh vertices themselves (on the surface: s
    near 0); 100 triangle centroids moved to 0.05 below the box along the axis (their rays run through the whole body)."""
    rng = np.random.default_rng(seed + axis)
    t = tris.astype(dt)
    verts = t.reshape(-1, 3)
    lo, hi = verts.min(axis=0).astype(np.float64) - 0.1, verts.max(axis=0).astype(np.float64) + 0.1
    box = (lo + (hi - lo) * rng.random((N_BOX, 3))).astype(dt)
    rays = verts[rng.integers(0, len(verts), N_VERTEX_RAYS)].copy()
    rays[:, axis] = (lo[axis] + (hi[axis] - lo[axis]) * rng.random(N_VERTEX_RAYS)).astype(dt)
    on = verts[rng.integers(0, len(verts), N_VERTICES)].copy()
    cen = t[rng.integers(0, len(t), N_CENTROIDS)].astype(np.float64).reshape(-1, 3, 3).mean(axis=1).astype(dt)
    cen[:, axis] = dt(lo[axis] + 0.05)  # (a centroid on the silhouette can round to a ray that misses: the host test pins that none does)
    return np.ascontiguousarray(np.concatenate([box, rays, on, cen]).astype(dt))


def non_vacuity(bf):
    """(odd, even above 0, none, vertex rays with a crossing, fewest crossings of a centroid ray) of a brute force over
    query_points()"""
    c = bf.crossings.astype(np.int64)
    return (int((c % 2 == 1).sum()), int(((c % 2 == 0) & (c > 0)).sum()), int((c == 0).sum()), int((c[VERTEX_RAYS] > 0).sum()),
            int(c[CENTROIDS].min()))


def assert_non_vacuous(bf):
    odd, even, none, vray, cen = non_vacuity(bf)
    assert odd >= 200 and even >= 150 and none >= 200 and vray >= 100 and cen >= 2, (odd, even, none, vray, cen)
