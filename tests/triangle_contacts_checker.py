"""Checker of ibvh_triangle_contacts (include/ibvh.h): the brute force over all triangles — the definition of the result —
built on ray_triangle_checker's evaluation (the input dtype throughout, every operation rounded once), and the query sets the
tests share.  Per query triangle Q: every mesh triangle K whose stored leaf box is not apart from Q's box and that one of the
six edge-against-triangle tests finds, in a caller-supplied leaf order.  QUERY describes the query to mesh_query_kit, whose
in_leaf_order, comparators and two-pass driver serve both list queries.  Host only."""
import functools

import numpy as np

import mesh_query_kit as kit
import ray_triangle_checker as rtc
from implicitbvh_amd import abi

QUERY = kit.ListQuery("ibvh_triangle_contacts", "tritri_walk_kernel", "query", abi.TRIS_COUNT, abi.TRIS_WRITE,
                      {"i": kit.Column("index", "index", "index", (), -7), "m": kit.Column("mask", "mask", "uint8", (), 249),
                       "p": kit.Column("points", "points", "float", (2, 3), -7.0)})
BIT_NAMES = ("a->b against K", "b->c against K", "c->a against K", "p1->p2 against Q", "p2->p3 against Q", "p3->p1 against Q")


class Contacts:
    """counts (m,) int64, offsets (m + 1,) int64, and per contact, grouped by query and within a query in leaf order:
    index (M,) of `idt`, mask (M,) uint8, points (M, 2, 3), query (M,) 0-based."""


def fold_box(tris):
    """(lo, up), each (n, 3): the minimum / maximum of the three vertices per coordinate, folded from the first vertex with
    `x < m ? x : m` / `x > m ? x : m` (a NaN in the second or third vertex is dropped, one in the first stays)"""
    a, b, c = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
    with np.errstate(invalid="ignore"):
        lo = np.where(b < a, b, a)
        lo = np.where(c < lo, c, lo)
        up = np.where(b > a, b, a)
        up = np.where(c > up, c, up)
    return lo, up


def tight_boxes(tris):
    """(n, 6) lo up: the boxes of leaves that hold exactly their triangles"""
    return np.concatenate(fold_box(tris), axis=1)


def seg(p0, p1, tri):
    """the segment p0 -> p1 against tri: the ray test with d = p1 - p0, and t <= 1 -> (hit, the point p0 + t * d)"""
    with np.errstate(all="ignore"):
        d = p1 - p0
        hit, t, _, _ = rtc.ray_triangle(tri, p0, d)
        hit = hit & (t <= 1)
        x = p0 + t[..., None] * d
    assert x.dtype == tri.dtype
    return hit, x


def six_tests(q, k):
    """q, k (P, 9): P pairs (Q, K) -> mask (P,) uint8 and points (P, 2, 3): the points of the lowest and the highest set bit
    (zeros where mask == 0)"""
    qa, qb, qc = q[:, 0:3], q[:, 3:6], q[:, 6:9]
    k1, k2, k3 = k[:, 0:3], k[:, 3:6], k[:, 6:9]
    mask = np.zeros(len(q), np.uint8)
    points = np.zeros((len(q), 2, 3), q.dtype)
    for bit, (p0, p1, tri) in enumerate(((qa, qb, k), (qb, qc, k), (qc, qa, k), (k1, k2, q), (k2, k3, q), (k3, k1, q))):
        hit, x = seg(p0, p1, tri)
        first = hit & (mask == 0)
        points[first, 0] = x[first]
        points[hit, 1] = x[hit]
        mask[hit] |= np.uint8(1 << bit)
    return mask, points


def shares_vertex(q, k):
    """q, k (P, 9) -> (P,) bool: a vertex of Q equals a vertex of K (== on all three coordinates, nine pairs)"""
    out = np.zeros(len(q), bool)
    for i in range(3):
        for j in range(3):
            out |= (q[:, 3 * i:3 * i + 3] == k[:, 3 * j:3 * j + 3]).all(axis=1)
    return out


def brute_force(tris, queries, leaf_order=None, leaf_boxes=None, query_ids=None, skip_shared=False, idt=np.int64, chunk=512):
    """The definition of the result.  tris (n, 9), queries (m, 9) of ONE float dtype.  leaf_order: the user indices (1-based)
    of the leaves in the order they lie in bvh.leaves, None = 1..n; an entry outside 1..n names no triangle and is skipped
    (the entry point's guard).  leaf_boxes (n, 6): the boxes stored in the leaves, by triangle; None = tight boxes.
    query_ids (m,): K is a contact of query i only if its index > query_ids[i].  skip_shared: no contact between triangles
    with an equal vertex.  A query with a NaN coordinate has no contacts."""
    dt = tris.dtype
    queries = queries.reshape(len(queries), 9)
    assert dt in (np.float32, np.float64) and queries.dtype == dt, (dt, queries.dtype)
    n, m = len(tris), len(queries)
    boxes = tight_boxes(tris) if leaf_boxes is None else np.asarray(leaf_boxes)
    assert boxes.shape == (n, 6) and boxes.dtype == dt
    order = np.arange(1, n + 1, dtype=np.int64) if leaf_order is None else np.asarray(leaf_order).astype(np.int64)
    order = order[(order >= 1) & (order <= n)]
    cols = order - 1
    qlo, qup = fold_box(queries)
    alive = ~np.isnan(queries).any(axis=1)
    lo, up = np.ascontiguousarray(boxes[cols, 0:3].T), np.ascontiguousarray(boxes[cols, 3:6].T)   # (3, leaves) in leaf order
    parts = {k: [] for k in ("query", "index", "mask", "points")}
    for s in range(0, m if n else 0, chunk):
        sl = slice(s, min(s + chunk, m))
        with np.errstate(invalid="ignore"):
            apart = np.zeros((sl.stop - sl.start, len(cols)), bool)
            for k in range(3):   # six strict comparisons
                apart |= qup[sl, k, None] < lo[k][None, :]
                apart |= qlo[sl, k, None] > up[k][None, :]
        near = ~apart & alive[sl, None]
        if query_ids is not None:
            near &= order[None, :] > np.asarray(query_ids)[sl, None].astype(np.int64)
        rows, js = np.nonzero(near)   # row-major: by query, then by leaf position
        q, k = queries[rows + s], tris[cols[js]]
        mask, points = six_tests(q, k)
        keep = mask != 0
        if skip_shared:
            keep &= ~shares_vertex(q, k)
        parts["query"].append(rows[keep] + s)
        parts["index"].append(order[js[keep]])
        parts["mask"].append(mask[keep])
        parts["points"].append(points[keep])
    out = Contacts()
    cat = lambda key, shape, t: np.concatenate(parts[key]).astype(t) if parts[key] else np.empty(shape, t)
    out.query = cat("query", (0,), np.int64)
    out.index = cat("index", (0,), idt)
    out.mask = cat("mask", (0,), np.uint8)
    out.points = cat("points", (0, 2, 3), dt)
    out.counts = np.bincount(out.query, minlength=m).astype(np.int64)
    out.offsets = np.concatenate([[0], np.cumsum(out.counts)]).astype(np.int64)
    return out


in_leaf_order = functools.partial(kit.in_leaf_order, owner="query", fields=("mask", "points"))


def swap_mask(mask):
    """the mask of (K, Q) from that of (Q, K): bits 0-2 and 3-5 exchanged"""
    mask = np.asarray(mask, np.uint8)
    return ((mask >> 3) | ((mask & 7) << 3)).astype(np.uint8)


# ---- the shared inputs -------------------------------------------------------------------------------------------------
# hand-made triangles of the host tests
FLAT = [0, 0, 0, 1, 0, 0, 0, 1, 0]                           # in the plane z = 0
PIERCING = [0.25, 0.25, -1, 0.25, 0.25, 1, 2, 2, 1]          # its edge ab goes through FLAT, FLAT's edge p2p3 through it
TOUCHING = [0.25, 0.25, 0, 0.25, 0.25, 1, 1, 1, 1]           # its vertex a lies on FLAT's face
COPLANAR = [0.125, 0.125, 0, 0.75, 0.125, 0, 0.125, 0.75, 0]  # overlaps FLAT in its plane
DISJOINT = [0.25, 0.25, 0.5, 0.25, 0.25, 1, 2, 2, 1]          # boxes overlap, nothing meets
FAR = [5, 5, 5, 6, 5, 5, 5, 6, 5]                             # boxes apart
SHIFT = (0.9, 0.05, 0.02)
ANGLE = 0.5
SLICERS = [[-3, -3, 0.013, 3, -3, 0.021, 0.1, 3, 0.017],
           [0.011, -3, -2, 0.023, 3, -2, 0.017, 0.2, 3],
           [-3, 0.5, -1, 3, 0.52, -1, 0.1, 0.49, 2]]


def other(tris):
    """the mesh rotated by 0.5 rad about the x axis (y' = c y - s z, z' = s y + c z), then shifted by (0.9, 0.05, 0.02);
    computed in float64 and cast to the dtype"""
    p = tris.astype(np.float64).reshape(-1, 3)
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    out = np.stack([p[:, 0] + SHIFT[0], c * p[:, 1] - s * p[:, 2] + SHIFT[1], s * p[:, 1] + c * p[:, 2] + SHIFT[2]], axis=1)
    return out.reshape(-1, 9).astype(tris.dtype)


def pipeline_queries(tris):
    """The whole-pipeline test's queries: the three slicing triangles, then other(tris) -> (3 + n, 9)"""
    return np.concatenate([np.array(SLICERS, tris.dtype), other(tris)])


def non_vacuity(bf):
    """what makes a comparison against `bf` mean something -> dict of the quantities the tests assert on"""
    bits = [int(((bf.mask >> b) & 1).sum()) for b in range(6)]
    set_bits = np.unpackbits(bf.mask[:, None], axis=1).sum(axis=1) if len(bf.mask) else np.zeros(0, np.int64)
    return dict(pairs=int(len(bf.index)), none=int((bf.counts == 0).sum()), one=int((bf.counts == 1).sum()),
                several=int((bf.counts >= 2).sum()), per_bit=bits, largest=int(bf.counts.max(initial=0)),
                two_bits=int((set_bits == 2).sum()))


def assert_non_vacuous(nv):
    """the thresholds of the whole-pipeline test (conditions the brute force alone meets on both meshes and both dtypes)"""
    assert nv["pairs"] >= 300 and nv["one"] >= 50 and nv["several"] >= 100, nv
    assert len(nv["per_bit"]) == 6 and min(nv["per_bit"]) >= 100, nv
    assert nv["largest"] >= 128 and nv["none"] >= 1000, nv
