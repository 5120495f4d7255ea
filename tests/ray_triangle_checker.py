"""Checker of ibvh_rays_resolve_triangles (include/ibvh.h): a numpy restatement of the exact ray-triangle arithmetic in the
INPUT dtype (float32 inputs are never promoted: every numpy operation below rounds once, like the kernel's, which is
compiled without contraction and with a correctly rounded divide), the segmented closest hit with the tie rule over a given
(counts, contacts), a brute-force variant over all triangles for small meshes, an independent float64 solve of the same
intersection, and the ray sets the tests share.  Host only."""
import numpy as np


def _cross(x, y):
    """a cross-product component is x1*y2 - x2*y1: two rounded products, one rounded subtraction"""
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def _dot(x, y):
    """(x0*y0 + x1*y1) + x2*y2"""
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def ray_triangle(tri, p, d):
    """tri (..., 9) = p1 p2 p3, p and d (..., 3), all of ONE float dtype (broadcast against each other) -> (hit, t, u, v):
    hit iff det != 0 and u >= 0 and v >= 0 and u + v <= 1 and t >= 0; every comparison false on NaN; two-sided, forwards."""
    dt = tri.dtype
    assert dt in (np.float32, np.float64) and p.dtype == dt and d.dtype == dt, (tri.dtype, p.dtype, d.dtype)
    a, b, c = tri[..., 0:3], tri[..., 3:6], tri[..., 6:9]
    with np.errstate(all="ignore"):
        e1 = b - a
        e2 = c - a
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        inv = dt.type(1) / det
        tv = p - a
        u = _dot(tv, pv) * inv
        qv = _cross(tv, e1)
        v = _dot(d, qv) * inv
        t = _dot(e2, qv) * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
    for x in (t, u, v):
        assert x.dtype == dt  # nothing was promoted on the way
    return hit, t, u, v


class Resolved:
    """index (nr,) of the contacts' dtype (0 = miss), t (nr,) (+Inf = miss), uv (nr, 2) (0, 0 on a miss), candidate_t (H,)
    (t of an exact hit, +Inf otherwise), accepted (H,) bool, bad (H,) bool: candidates whose index lies outside 1..n."""


def _closest(ray, hit, t, u, v, index, nr, idt):
    """The winner per ray among candidates in LIST order (`ray` ascending, 0-based): the smallest t, on equal t
    (-0 == +0) the earlier candidate.  A hit whose t is +Inf still beats no hit."""
    dt = t.dtype
    k = np.arange(len(t))
    tkey = np.where(hit, np.where(t == 0, dt.type(0), t), dt.type(np.inf))
    order = np.lexsort((k, ~hit, tkey, ray))  # by ray, then t, then hits first, then position
    first = np.ones(len(order), bool)
    first[1:] = ray[order][1:] != ray[order][:-1]
    win = order[first]
    win = win[hit[win]]
    out = Resolved()
    out.index = np.zeros(nr, idt)
    out.t = np.full(nr, np.inf, dt)
    out.uv = np.zeros((nr, 2), dt)
    out.index[ray[win]] = index[win]
    out.t[ray[win]] = t[win]
    out.uv[ray[win], 0] = u[win]
    out.uv[ray[win], 1] = v[win]
    out.winner = np.full(nr, -1, np.int64)  # position of the winning candidate
    out.winner[ray[win]] = win
    return out


def resolve(counts, contacts, triangles, points, directions):
    """The library's result for one list.  counts: (nr,) inclusive scanned counts; contacts: (>= total, 2) (leaf.index, iray);
    triangles (n, 9); points / directions (nr, 3).  Bit for bit what the kernel must produce."""
    nr = len(counts)
    idt = contacts.dtype
    dt = triangles.dtype.type
    total = int(counts[-1]) if nr else 0
    ends = counts.astype(np.int64)
    lens = np.diff(np.concatenate([[0], ends]))
    assert (lens >= 0).all() and total <= len(contacts)
    ray = np.repeat(np.arange(nr), lens)
    index = contacts[:total, 0]
    assert (contacts[:total, 1] == ray + 1).all(), "the list is grouped by ray (an LVT list)"
    bad = (index < 1) | (index > len(triangles))
    rows = np.where(bad, 0, index.astype(np.int64) - 1)
    if len(triangles):
        hit, t, u, v = ray_triangle(triangles[rows], points[ray], directions[ray])
    else:
        hit, t = np.zeros(total, bool), np.full(total, np.inf, dt)
        u, v = t.copy(), t.copy()
    hit = hit & ~bad
    out = _closest(ray, hit, t, u, v, index, nr, idt)
    out.candidate_t = np.where(hit, t, dt(np.inf)).astype(dt)
    out.accepted, out.bad = hit, bad
    return out


def brute_force(triangles, points, directions, idt=np.int64, chunk=256):
    """The same arithmetic over ALL triangles in index order (ties: the lower index), for small meshes."""
    nr, n = len(points), len(triangles)
    parts = []
    for s in range(0, nr, chunk):
        e = min(nr, s + chunk)
        hit, t, u, v = ray_triangle(triangles[None, :, :], points[s:e, None, :], directions[s:e, None, :])
        ray = np.repeat(np.arange(e - s), n)
        index = np.tile(np.arange(1, n + 1, dtype=idt), e - s)
        parts.append(_closest(ray, hit.ravel(), t.ravel(), u.ravel(), v.ravel(), index, e - s, idt))
    out = Resolved()
    out.index = np.concatenate([q.index for q in parts])
    out.t = np.concatenate([q.t for q in parts])
    out.uv = np.concatenate([q.uv for q in parts])
    return out


def solve_float64(triangles, points, directions):
    """An independent float64 formulation for well-conditioned cases: solve [-d e1 e2] (t u v)^T = p - a per (ray,
    triangle) with a general linear solver.  -> (hit, margin) of shape (nr, n): margin is the distance of (t, u, v) from
    the nearest acceptance boundary and |det| relative to the edge lengths, so callers can drop ill-conditioned pairs."""
    tri = triangles.astype(np.float64)
    p, d = points.astype(np.float64), directions.astype(np.float64)
    a, e1, e2 = tri[:, 0:3], tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
    nr, n = len(p), len(tri)
    m = np.empty((nr, n, 3, 3))
    m[..., 0] = -d[:, None, :]
    m[..., 1] = e1[None]
    m[..., 2] = e2[None]
    rhs = p[:, None, :] - a[None]
    det = np.linalg.det(m)
    scale = np.linalg.norm(d, axis=1)[:, None] * (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))[None]
    ok = np.abs(det) > 1e-6 * scale
    m[~ok] = np.eye(3)
    x = np.linalg.solve(m, rhs[..., None])[..., 0]
    t, u, v = x[..., 0], x[..., 1], x[..., 2]
    hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
    margin = np.minimum.reduce([np.abs(u), np.abs(v), np.abs(1 - u - v), np.abs(t) / (1 + np.abs(t))])
    margin = np.where(ok, margin, 0.0)
    return hit, margin


# ---- the ray sets ------------------------------------------------------------------------------------------------------
def mesh_box(triangles):
    pts = triangles.reshape(-1, 3)
    return pts.min(0), pts.max(0)


def aimed_rays(n, triangles, dtype=np.float32):
    """Rays that must hit: origins on a sphere of radius |hi - lo| around the box centre, directions through
    Dirichlet(1, 1, 1)-weighted interior points of random triangles; default_rng(7)."""
    rng = np.random.default_rng(7)
    lo, hi = mesh_box(triangles.astype(np.float64))
    centre, radius = 0.5 * (lo + hi), np.linalg.norm(hi - lo)
    g = rng.normal(size=(n, 3))
    origin = centre + radius * g / np.linalg.norm(g, axis=1, keepdims=True)
    which = rng.integers(0, len(triangles), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    corners = triangles[which].astype(np.float64).reshape(n, 3, 3)
    target = (w[:, :, None] * corners).sum(1)
    return origin.astype(dtype), (target - origin).astype(dtype)
