"""Checker of ibvh_cast_rays (include/ibvh.h): a numpy restatement of the definition in the INPUT dtype (float32 inputs are
never promoted: every numpy operation below rounds once, like the kernel's, which is compiled without contraction and with a
correctly rounded divide) — the slab test of a box with its own rule for a zero direction component, the exact ray-triangle
test (tests/ray_triangle_checker.py: the one the resolve is pinned to), the clamped hit parameter t* = max(t, entry of the
triangle's leaf box), the ray limit L — and the brute force over ALL triangles, which is the definition of the result: the
lexicographic minimum of (t*, index) over the hits for the closest hit, "a hit exists" for any hit.  Per ray it also reports
how many exact hits there are, whether the winner's clamp was active and whether the winning t* is tied.  And the rays the
tests share.  Host only."""
import numpy as np

from closest_point_checker import triangle_boxes  # noqa: F401  (the `x < y ? x : y` ternaries of BBox{T}(p1, p2, p3))
from ray_triangle_checker import ray_triangle


def slab_entry(lo, up, p, d):
    """lo, up, p, d (..., 3) of ONE float dtype, broadcast against each other -> (entry, admitted): entry = tmin where the
    box is admitted, +Inf where it is not.  The selects are the header's, so a NaN goes where the header says it goes."""
    dt = p.dtype
    assert dt in (np.float32, np.float64) and lo.dtype == dt and up.dtype == dt and d.dtype == dt, (lo.dtype, up.dtype, p.dtype, d.dtype)
    inf = dt.type(np.inf)
    shape = np.broadcast(lo[..., 0], up[..., 0], p[..., 0], d[..., 0]).shape
    tmin, tmax, ok = np.full(shape, -inf, dt), np.full(shape, inf, dt), np.ones(shape, bool)
    with np.errstate(all="ignore"):
        inv = dt.type(1) / d
        for k in range(3):
            still = d[..., k] == 0
            t1, t2 = (lo[..., k] - p[..., k]) * inv[..., k], (up[..., k] - p[..., k]) * inv[..., k]
            tnear, tfar = np.where(t2 < t1, t2, t1), np.where(t2 > t1, t2, t1)
            nmin, nmax = np.where(tnear > tmin, tnear, tmin), np.where(tfar < tmax, tfar, tmax)
            ok = ok & (~still | ((lo[..., k] <= p[..., k]) & (p[..., k] <= up[..., k])))
            tmin, tmax = np.where(still, tmin, nmin), np.where(still, tmax, nmax)
        admitted = ok & (tmin <= tmax) & (tmax >= 0)
    entry = np.where(admitted, tmin, inf)
    assert entry.dtype == dt and inv.dtype == dt  # nothing was promoted on the way
    return entry, admitted


def limit(t_max, n, dt):
    """L per ray: min(t_max, the largest finite value) by the header's select (a NaN stays a NaN); None = unbounded"""
    dt = np.dtype(dt)
    big = np.finfo(dt).max
    given = np.full(n, np.inf, dt) if t_max is None else np.asarray(t_max, dt)
    assert given.shape == (n,)
    with np.errstate(invalid="ignore"):
        return np.where(given > big, big, given).astype(dt)


class Cast:
    """index (m,) of `idt` (0 = miss), t (m,) (+Inf = miss), uv (m, 2) (0, 0 on a miss), occluded (m,) uint8: the outputs;
    hits (m,) the number of hits within the limit, exact (m,) the number of triangles passing the exact test, clamped (m,)
    bool: the winner's entry exceeded its t, tied (m,) bool: more than one hit carries the winning t*."""


def brute_force(tris, p, d, t_max=None, idt=np.int64, boxes=None, chunk=64):
    """The definition of the result.  tris (n, 9), p, d (m, 3) of one dtype; t_max None or (m,); boxes: the leaves' stored
    (lo, up), (n, 3) each — default: the triangles' exact boxes, what volumes-from-triangles stores."""
    dt = tris.dtype
    assert p.dtype == dt and d.dtype == dt and p.shape == d.shape
    m, n = len(p), len(tris)
    lo, up = triangle_boxes(tris) if boxes is None else boxes
    assert lo.dtype == dt and up.dtype == dt
    L = limit(t_max, m, dt)
    inf = dt.type(np.inf)
    out = Cast()
    out.index, out.t, out.uv = np.zeros(m, idt), np.full(m, inf, dt), np.zeros((m, 2), dt)
    out.occluded, out.hits, out.exact = np.zeros(m, np.uint8), np.zeros(m, np.int64), np.zeros(m, np.int64)
    out.clamped, out.tied = np.zeros(m, bool), np.zeros(m, bool)
    if n == 0:
        return out
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        ps, ds = p[s:e, None, :], d[s:e, None, :]
        exact, t, u, v = ray_triangle(tris[None], ps, ds)
        entry, admitted = slab_entry(lo[None], up[None], ps, ds)
        with np.errstate(invalid="ignore"):
            ts = np.where(entry > t, entry, t)
            hit = exact & admitted & (ts <= L[s:e, None])
            key = np.where(hit, ts, inf)
            best = key.min(axis=1)
            winners = hit & (key == best[:, None])      # (-0 == +0: equal)
        k = winners.argmax(axis=1)                       # the smallest index among them
        any_ = hit.any(axis=1)
        r = np.arange(e - s)
        out.index[s:e] = np.where(any_, k + 1, 0)
        out.t[s:e] = np.where(any_, ts[r, k], inf)
        out.uv[s:e, 0], out.uv[s:e, 1] = np.where(any_, u[r, k], 0), np.where(any_, v[r, k], 0)
        out.occluded[s:e] = any_
        out.hits[s:e], out.exact[s:e] = hit.sum(axis=1), exact.sum(axis=1)
        with np.errstate(invalid="ignore"):
            out.clamped[s:e] = any_ & (entry[r, k] > t[r, k])
        out.tied[s:e] = any_ & (winners.sum(axis=1) > 1)
    assert out.t.dtype == dt and out.uv.dtype == dt
    return out


def second_hit(tris, p, d, chunk=64):
    """(t1, t2) per ray: the smallest and the second smallest t* over the hits of the unbounded ray (+Inf where there is none)"""
    dt = tris.dtype
    lo, up = triangle_boxes(tris)
    first, second = np.full(len(p), np.inf, dt), np.full(len(p), np.inf, dt)
    for s in range(0, len(p), chunk):
        ps, ds = p[s:s + chunk, None, :], d[s:s + chunk, None, :]
        exact, t, _, _ = ray_triangle(tris[None], ps, ds)
        entry, admitted = slab_entry(lo[None], up[None], ps, ds)
        with np.errstate(invalid="ignore"):
            key = np.sort(np.where(exact & admitted & np.isfinite(t), np.where(entry > t, entry, t), dt.type(np.inf)), axis=1)
        first[s:s + chunk] = key[:, 0]
        if key.shape[1] > 1:
            second[s:s + chunk] = key[:, 1]
    return first, second


# ---- the rays ----------------------------------------------------------------------------------------------------------
N_RAYS = 800
ZERO_X, ZERO_Y, INSIDE = slice(0, None, 10), slice(5, None, 10), slice(3, None, 20)


def all_nonzero(d):
    """the rays whose three direction components are all non-zero: a selection on the INPUT"""
    return (d != 0).all(axis=1)


def rays(tris, dt, n=N_RAYS, seed=19):
    """n rays of `dt`: origins uniform in the mesh's box inflated by 0.5 each way, every ray aimed at a random triangle's
    centroid (d = centroid - origin: the target sits at t = 1); every 10th ray with d_x = 0 and every 10th, offset by 5,
    with d_y = 0 (so they leave their target); every 20th (offset 3) starting INSIDE the mesh's boxes, at a uniform point of
    a random triangle's box (its entry into that box is negative)."""
    rng = np.random.default_rng(seed)
    t = tris.astype(dt)
    verts = t.reshape(-1, 3).astype(np.float64)
    lo, hi = verts.min(axis=0) - 0.5, verts.max(axis=0) + 0.5
    origin = lo + (hi - lo) * rng.random((n, 3))
    blo, bup = (x.astype(np.float64) for x in triangle_boxes(t))
    home = rng.integers(0, len(t), n)
    inside = blo[home] + (bup[home] - blo[home]) * rng.random((n, 3))
    origin[INSIDE] = inside[INSIDE]
    target = t[rng.integers(0, len(t), n)].astype(np.float64).reshape(-1, 3, 3).mean(axis=1)
    p = origin.astype(dt)
    d = (target - p.astype(np.float64)).astype(dt)
    d[ZERO_X, 0] = 0
    d[ZERO_Y, 1] = 0
    return np.ascontiguousarray(p), np.ascontiguousarray(d)


def non_vacuity(bf, d):
    """(rays that hit, rays that miss, hitting rays with two or more exact hits, exact hits in all, hitting rays with a zero
    direction component, clamped winners, tied winners) of an unbounded brute force over rays()"""
    hit = bf.index != 0
    return (int(hit.sum()), int((~hit).sum()), int((hit & (bf.exact >= 2)).sum()), int(bf.exact.sum()),
            int((hit & ~all_nonzero(d)).sum()), int(bf.clamped.sum()), int(bf.tied.sum()))


def assert_non_vacuous(bf, d):
    n = len(d)
    hit, miss, multi, _, zero, clamped, tied = non_vacuity(bf, d)
    assert 2 * hit >= n and 20 * miss >= n and 4 * multi >= hit and zero >= 1 and clamped == 0 and tied == 0, non_vacuity(bf, d)


def floor_case(dt, n=200, seed=23):
    """An axis-aligned floor — two triangles in the plane z = 0.3, so each lies flat in a face of its own box (lo_z == up_z) —
    and n rays from above aimed at points of it: the z slab's entry and the exact test's t are two roundings of the same
    distance, so on some rays the entry is the larger and the clamp is active.  -> (tris (2, 9), p, d)"""
    rng = np.random.default_rng(seed)
    z = 0.3
    tris = np.array([[-1.3, -1.1, z, 1.7, -0.9, z, 1.2, 1.4, z], [-1.3, -1.1, z, 1.2, 1.4, z, -0.8, 1.3, z]], dt)  # (no power-of-two edges:
    # with those Moeller-Trumbore's t and the slab's entry are the same bits)
    p = np.stack([rng.random(n) * 2 - 1, rng.random(n) * 2 - 1, 0.5 + 1.5 * rng.random(n)], axis=1).astype(dt)
    aim = np.stack([rng.random(n) * 1.6 - 0.8, rng.random(n) * 1.6 - 0.8, np.full(n, z)], axis=1)
    d = (aim - p.astype(np.float64)).astype(dt)
    return tris, np.ascontiguousarray(p), np.ascontiguousarray(d)
