"""Checker of ibvh_capsule_contacts and ibvh_segment_distances (include/ibvh.h): a numpy restatement of the segment-triangle
evaluation in the INPUT dtype (float32 inputs are never promoted: every numpy operation below rounds once, like the kernel's)
— the cut rule on ray_triangle_checker's exact test, the two ends on closest_point_checker's point-triangle evaluation, the
three edges on triangle_distance_checker's segment-segment evaluation —, the two brute forces over ALL triangles that define
the results (the contacts with the slab clause on ray_cast_checker's slab test of the stored box grown by r, in a caller-
supplied leaf order; the distances with the tie rule), the bounds the walks prune with, and the inputs the tests share.  QUERY
describes the list query to mesh_query_kit.  Host only."""
import functools

import numpy as np

import closest_point_checker as cpc
import mesh_query_kit as kit
import triangle_contacts_checker as tcc
from implicitbvh_amd import abi
from ray_cast_checker import slab_entry
from ray_triangle_checker import ray_triangle
from triangle_distance_checker import EDGES, box_bound, boxes_apart, closest_on_segments

CUT = 5
KIND_NAMES = ("end a", "end b", "edge p1p2", "edge p2p3", "edge p3p1", "cut")
QUERY = kit.ListQuery("ibvh_capsule_contacts", "capsules_walk_kernel", "capsule", abi.CAPSULES_COUNT, abi.CAPSULES_WRITE,
                      {"i": kit.Column("index", "index", "index", (), -7), "d": kit.Column("d2", "distance2", "float", (), -7.0),
                       "s": kit.Column("point_segment", "point_segment", "float", (3,), -7.0),
                       "m": kit.Column("point_mesh", "point_mesh", "float", (3,), -7.0),
                       "k": kit.Column("kind", "kind", "uint8", (), 249)})


def segment_box(a, b):
    """S's exact box: `a < b ? a : b` / `a > b ? a : b` per component"""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, a, b), np.where(a > b, a, b)


def triangle_box(k):
    """K's exact box for k (..., 9): triangle_contacts_checker.fold_box's fold, from the first vertex"""
    p1, p2, p3 = k[..., 0:3], k[..., 3:6], k[..., 6:9]
    with np.errstate(invalid="ignore"):
        lo = np.where(p2 < p1, p2, p1)
        lo = np.where(p3 < lo, p3, lo)
        up = np.where(p2 > p1, p2, p1)
        up = np.where(p3 > up, p3, up)
    return lo, up


def pairs(a, b, k):
    """a, b (..., 3), k (..., 9) of ONE float dtype, broadcast against each other -> (d2 (...), xs (..., 3), xk (..., 3), kind
    (...) uint8): the evaluation of include/ibvh.h, both rules"""
    dt = k.dtype
    assert dt in (np.float32, np.float64) and a.dtype == dt and b.dtype == dt, (dt, a.dtype, b.dtype)
    shape = np.broadcast(a[..., 0], b[..., 0], k[..., 0]).shape
    full = lambda x: np.broadcast_to(x, shape + (3,))
    # the candidate rule: candidate 0 starts the result, a later one replaces it iff its d2 is strictly smaller
    x, d2, _ = cpc._evaluate(k, a)
    best = [np.broadcast_to(d2, shape).copy(), full(a).copy(), full(x).copy(), np.zeros(shape, np.uint8)]

    def offer(d2, xs, xk, c):
        d2, xs, xk = np.broadcast_to(d2, shape), full(xs), full(xk)
        with np.errstate(invalid="ignore"):
            better = d2 < best[0]
        best[0][better], best[1][better], best[2][better], best[3][better] = d2[better], xs[better], xk[better], c
    x, d2, _ = cpc._evaluate(k, b)
    offer(d2, b, x, 1)
    for c, (j0, j1) in enumerate(EDGES):
        xs, xk, d2 = closest_on_segments(a, b, k[..., j0:j0 + 3], k[..., j1:j1 + 3])
        offer(d2, xs, xk, 2 + c)
    # the cut rule, on the pairs whose exact boxes are not apart
    slo, sup = segment_box(a, b)
    klo, kup = triangle_box(k)
    with np.errstate(all="ignore"):
        d = b - a
        hit, t, _, _ = ray_triangle(k, a, d)
        cut = np.broadcast_to(~boxes_apart(slo, sup, klo, kup) & hit & (t <= 1), shape)
        x = full(a + t[..., None] * d)
    assert x.dtype == dt and best[0].dtype == dt and best[1].dtype == dt and best[2].dtype == dt   # nothing was promoted
    best[0][cut], best[1][cut], best[2][cut], best[3][cut] = 0, x[cut], x[cut], CUT
    return tuple(best)


def grown_entry(lo, up, r, a, b):
    """clause (i)'s entry: the slab test of the ray p = a, d = b - a against the box grown by r (lo - r, up + r, each rounded
    once); lo, up, a, b (..., 3), r (...)"""
    with np.errstate(all="ignore"):
        glo, gup, d = lo - r[..., None], up + r[..., None], b - a
    assert glo.dtype == a.dtype and gup.dtype == a.dtype
    return slab_entry(glo, gup, a, d)[0]


def refused(lo, up, r, a, b):
    """what the contacts' walk refuses a box for -> (by the gap, by the slab): the squared gap to S's exact box exceeds r * r;
    the entry into the box grown by r exceeds 1 (both false on NaN)"""
    slo, sup = segment_box(a, b)
    with np.errstate(all="ignore"):
        return box_bound(lo, up, slo, sup) > r * r, grown_entry(lo, up, r, a, b) > 1


class Contacts:
    """counts (m,) int64, offsets (m + 1,) int64, and per contact, grouped by capsule and within a capsule in leaf order:
    index (M,) of `idt`, d2 (M,), point_segment, point_mesh (M, 3), kind (M,) uint8, capsule (M,) 0-based; r2 (m,) the squared
    radii; slab_dropped: how many pairs pass the distance clause and fail the slab clause."""


def brute_force_contacts(tris, a, b, radii, leaf_order=None, leaf_boxes=None, idt=np.int64, chunk=64):
    """The definition of the result.  tris (n, 9), a, b (m, 3), radii (m,) of ONE float dtype.  leaf_order: the user indices
    (1-based) of the leaves in the order they lie in bvh.leaves, None = 1..n; an entry outside 1..n names no triangle and is
    skipped (the entry point's guard).  leaf_boxes (n, 6): the boxes stored in the leaves, by triangle; None = tight boxes.
    A contact iff entry(stored box grown by r) <= 1 and d2 <= r * r (false on NaN); none for !(r >= 0) or a NaN in a or b."""
    dt = tris.dtype
    assert a.dtype == dt and b.dtype == dt and radii.dtype == dt and a.shape == b.shape and radii.shape == (len(a),)
    n, m = len(tris), len(a)
    boxes = tcc.tight_boxes(tris) if leaf_boxes is None else np.asarray(leaf_boxes)
    assert boxes.shape == (n, 6) and boxes.dtype == dt
    order = np.arange(1, n + 1, dtype=np.int64) if leaf_order is None else np.asarray(leaf_order).astype(np.int64)
    order = order[(order >= 1) & (order <= n)]
    cols = order - 1
    with np.errstate(all="ignore"):
        r2 = radii * radii
        alive = (radii >= 0) & ~np.isnan(a).any(axis=1) & ~np.isnan(b).any(axis=1)
    fields = ("capsule", "index", "d2", "point_segment", "point_mesh", "kind")
    parts = {k: [] for k in fields}
    dropped = 0
    for s in range(0, m if n else 0, chunk):
        sl = slice(s, min(s + chunk, m))
        d2, xs, xk, kind = pairs(a[sl, None], b[sl, None], tris[None])
        entry = grown_entry(boxes[None, :, 0:3], boxes[None, :, 3:6], radii[sl, None], a[sl, None], b[sl, None])
        with np.errstate(invalid="ignore"):
            near = (d2 <= r2[sl, None]) & alive[sl, None]
            hit = near & (entry <= 1)
        dropped += int((near & ~hit).sum())
        rows, js = np.nonzero(hit[:, cols])   # row-major: by capsule, then by leaf position
        k = cols[js]
        for key, value in zip(fields, (rows + s, order[js], d2[rows, k], xs[rows, k], xk[rows, k], kind[rows, k])):
            parts[key].append(value)
    out = Contacts()
    cat = lambda key, shape, t: np.concatenate(parts[key]).astype(t) if parts[key] else np.empty(shape, t)
    out.capsule, out.index = cat("capsule", (0,), np.int64), cat("index", (0,), idt)
    out.d2, out.kind = cat("d2", (0,), dt), cat("kind", (0,), np.uint8)
    out.point_segment, out.point_mesh = cat("point_segment", (0, 3), dt), cat("point_mesh", (0, 3), dt)
    out.counts = np.bincount(out.capsule, minlength=m).astype(np.int64)
    out.offsets = np.concatenate([[0], np.cumsum(out.counts)]).astype(np.int64)
    out.r2, out.slab_dropped = r2, dropped
    return out


in_leaf_order = functools.partial(kit.in_leaf_order, owner="capsule", fields=("d2", "point_segment", "point_mesh", "kind"))


class Distances:
    """index (m,) of `idt` (0 = none), d2 (m,) (+Inf = none), point_segment, point_mesh (m, 3) (0 = none), kind (m,) uint8
    (0 = none), ties (m,): how many qualifying triangles share the winner's d2 (0 = none)."""


FIELDS = ("index", "d2", "point_segment", "point_mesh", "kind")


def brute_force_distances(tris, a, b, max_d2=None, idt=np.int64, chunk=64):
    """The definition of the result.  tris (n, 9), a, b (m, 3) of ONE float dtype: per segment the lexicographic minimum of
    (d2, index) over ALL triangles with d2 <= max_d2 (every comparison false on NaN; None = +Inf).  A segment with a NaN
    coordinate, and every segment under a NaN radius, has no answer."""
    dt = tris.dtype
    assert a.dtype == dt and b.dtype == dt and a.shape == b.shape
    n, m = len(tris), len(a)
    max_d2 = dt.type(np.inf) if max_d2 is None else dt.type(max_d2)
    out = Distances()
    out.index, out.d2 = np.zeros(m, idt), np.full(m, np.inf, dt)
    out.point_segment, out.point_mesh = np.zeros((m, 3), dt), np.zeros((m, 3), dt)
    out.kind, out.ties = np.zeros(m, np.uint8), np.zeros(m, np.int64)
    alive = ~np.isnan(a).any(axis=1) & ~np.isnan(b).any(axis=1)
    for s in range(0, m if n else 0, chunk):
        sl = slice(s, min(s + chunk, m))
        d2, xs, xk, kind = pairs(a[sl, None], b[sl, None], tris[None])
        with np.errstate(invalid="ignore"):
            valid = (d2 <= max_d2) & alive[sl, None]
        key = np.where(valid, d2, dt.type(np.inf))
        cand = valid & (key == key.min(axis=1, keepdims=True))   # (a qualifying +Inf still beats nothing)
        has = cand.any(axis=1)
        j = cand.argmax(axis=1)                                  # the first = the smallest index
        r = np.arange(len(j))
        out.index[sl] = np.where(has, j + 1, 0)
        out.d2[sl] = np.where(has, d2[r, j], dt.type(np.inf))
        out.point_segment[sl] = np.where(has[:, None], xs[r, j], dt.type(0))
        out.point_mesh[sl] = np.where(has[:, None], xk[r, j], dt.type(0))
        out.kind[sl] = np.where(has, kind[r, j], 0)
        out.ties[sl] = cand.sum(axis=1)
    return out


def limited(bf, max_d2):
    """the unbounded result `bf` under a radius: the winner if its d2 <= max_d2, else none (the lexicographic minimum of a
    subset that is cut off by d2 alone)"""
    dt = bf.d2.dtype
    with np.errstate(invalid="ignore"):
        keep = (bf.index != 0) & (bf.d2 <= dt.type(max_d2))
    out = Distances()
    out.index, out.d2 = np.where(keep, bf.index, 0).astype(bf.index.dtype), np.where(keep, bf.d2, dt.type(np.inf))
    out.point_segment = np.where(keep[:, None], bf.point_segment, dt.type(0))
    out.point_mesh = np.where(keep[:, None], bf.point_mesh, dt.type(0))
    out.kind, out.ties = np.where(keep, bf.kind, 0).astype(np.uint8), np.where(keep, bf.ties, 0)
    return out


# ---- the shared inputs -------------------------------------------------------------------------------------------------
N_CAPSULES = 400
ZERO_LENGTH = slice(0, 20)     # b == a
ONE_AXIS_STILL = slice(20, 60)  # one component of b - a is exactly 0, cycling through x, y, z


def capsules(tris, dt, n=N_CAPSULES, seed=61):
    """n capsules near the surface, e the mean length of edge ab: starts at a mesh vertex plus normal noise of two e, lengths
    rng * 12 e in random directions — the first 20 of length zero, the next 40 with one axis still —, radii 0.5 e .. 3 e
    -> (a (n, 3), b (n, 3), radii (n,)) of `dt`"""
    from sphere_contacts_checker import mean_edge
    rng = np.random.default_rng(seed)
    t64 = tris.astype(np.float64)
    e = mean_edge(t64)
    vertex = t64.reshape(-1, 3)[rng.integers(0, 3 * len(t64), n)]
    a = (vertex + rng.normal(size=(n, 3)) * 2 * e).astype(dt)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    length = rng.random(n) * 12 * e
    length[ZERO_LENGTH] = 0
    b = (a.astype(np.float64) + direction * length[:, None]).astype(dt)
    b[ZERO_LENGTH] = a[ZERO_LENGTH]
    rows = np.arange(n)[ONE_AXIS_STILL]
    b[rows, rows % 3] = a[rows, rows % 3]
    radii = ((0.5 + 2.5 * rng.random(n)) * e).astype(dt)
    return a, b, radii


@functools.lru_cache(maxsize=None)
def reference(mesh, dt, n=N_CAPSULES):
    """(triangles, a, b, radii, the contacts in index order with tight boxes, the unbounded distances) of a named mesh,
    computed once and read-only"""
    from implicitbvh_amd.synthetic import torus_mesh
    tris = torus_mesh(*kit.MESHES[mesh]).astype(dt)
    a, b, radii = capsules(tris, dt, n)
    contacts = brute_force_contacts(tris, a, b, radii)
    distances = brute_force_distances(tris, a, b)
    # (a, b and radii go through torch.from_numpy, which wants a writable array)
    for x in (tris,) + tuple(v for bf in (contacts, distances) for v in vars(bf).values() if isinstance(v, np.ndarray)):
        x.setflags(write=False)
    return tris, a, b, radii, contacts, distances


# ---- the hand-made inputs of the GPU tests (capsule contacts, segment distances, box contacts) -----------------------------
CAPSULES_PER_MESH = {"torus40": N_CAPSULES, "torus64x63": 100}   # 3,200 triangles; 8,064: a leaf count that is no power of two
nan, inf = np.nan, np.inf
FLAT = [0, 0, 0, 1, 0, 0, 0, 1, 0]
HAND = [FLAT,
        [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5],       # FLAT moved up by 0.5
        [5, 5, 5, 6, 6, 6, 7, 7, 7],             # zero area: collinear
        [3, 0, 0, 4, 0, 0, 3, 1, 0],
        [0, 0, 3, 1, 0, 3, 0, 1, 3]]
# (a, b, r): through FLAT's face; parallel above it at height r exactly and one unit below; end-on above a vertex; crossing
# an edge at a skew; zero length, off and on the face; INSIDE FLAT's plane, over the face and beside it; a long diagonal one;
# negative, NaN, -0.0 and infinite radii; a NaN in a and in b; an infinite end
HAND_CAPSULES = [((0.25, 0.25, -1), (0.25, 0.25, 1), 0), ((0.25, 0.25, 0.25), (0.5, 0.25, 0.25), 0.25),
                 ((0.25, 0.25, 0.25), (0.5, 0.25, 0.25), float(np.nextafter(np.float32(0.25), np.float32(0)))),
                 ((0, 0, 3.5), (0, 0, 3.25), 0.25), ((0.25, -1, -1), (0.75, -1, 1), 1), ((0.25, 0.25, 0.25), (0.25, 0.25, 0.25), 0.25),
                 ((0.25, 0.25, 0), (0.25, 0.25, 0), 0), ((0.125, 0.125, 0), (0.5, 0.25, 0), 0.125), ((1.5, 1.5, 0), (3, -1, 0), 1),
                 ((-1, -1, -1), (7, 7, 7.5), 0.5), ((0.25, 0.25, 0.25), (0.5, 0.25, 0.25), -1), ((0.25, 0.25, 0.25), (0.5, 0.25, 0.25), nan),
                 ((0.25, 0.25, 0), (0.5, 0.25, 0), -0.0), ((0.25, 0.25, 0.25), (0.5, 0.25, 0.25), inf), ((0.25, 0.25, -inf), (0.5, 0.25, 0.25), -inf),
                 ((nan, 0.25, 0.25), (0.5, 0.25, 0.25), 1), ((0.25, 0.25, 0.25), (0.5, nan, 0.25), inf), ((0.25, 0.25, 0.25), (0.5, 0.25, inf), 1)]
