"""Checker of ibvh_box_contacts (include/ibvh.h): a numpy restatement of the contract in the INPUT dtype (float32 inputs are
never promoted: every numpy operation below rounds once, like the kernel's, in the header's order) — the hull of a box, the
local coordinates of a vertex, the 13 separating axes family by family, the inside mask —, the brute force over ALL triangles
that defines the result (the box clause on the STORED leaf boxes, in a caller-supplied leaf order), which family of axes
refuses a pair first, hand-made pairs with known answers, and the inputs the tests share.  QUERY describes the list query to
mesh_query_kit.  Host only."""
import functools

import numpy as np

import mesh_query_kit as kit
import triangle_contacts_checker as tcc
from implicitbvh_amd import abi
from triangle_distance_checker import boxes_apart

QUERY = kit.ListQuery("ibvh_box_contacts", "boxes_walk_kernel", "box", abi.BOXES_COUNT, abi.BOXES_WRITE,
                      {"i": kit.Column("index", "index", "index", (), -7), "m": kit.Column("inside", "inside", "uint8", (), 249)})
FAMILIES = ("box axes", "normal", "edge axes")


def identity(dt, shape=()):
    """the rotation that rotations=None stands for: (..., 3, 3) of `dt`"""
    return np.broadcast_to(np.eye(3, dtype=dt), tuple(shape) + (3, 3))


def hull(c, h, R):
    """Q = c -+ e, e_k = ((|R_0k| * h_0 + |R_1k| * h_1) + |R_2k| * h_2); c, h (..., 3), R (..., 3, 3) -> (lo, up) (..., 3)"""
    with np.errstate(all="ignore"):
        e = np.stack([(np.abs(R[..., 0, k]) * h[..., 0] + np.abs(R[..., 1, k]) * h[..., 1]) + np.abs(R[..., 2, k]) * h[..., 2]
                      for k in range(3)], axis=-1)
        return c - e, c + e


def local(c, R, p):
    """the local coordinates of p: w = p - c, v[k] = ((u_k0 * w_0 + u_k1 * w_1) + u_k2 * w_2) -> [v[0], v[1], v[2]]"""
    with np.errstate(all="ignore"):
        w = [p[..., j] - c[..., j] for j in range(3)]
        return [(R[..., k, 0] * w[0] + R[..., k, 1] * w[1]) + R[..., k, 2] * w[2] for k in range(3)]


def axis_overlaps(p1, p2, p3, rad):
    """min <= rad and max >= -rad, folded from p1 with `x < m ? x : m` / `x > m ? x : m`; false on NaN"""
    with np.errstate(invalid="ignore"):
        mn = np.where(p2 < p1, p2, p1)
        mn = np.where(p3 < mn, p3, mn)
        mx = np.where(p2 > p1, p2, p1)
        mx = np.where(p3 > mx, p3, mx)
        return (mn <= rad) & (mx >= -rad)


def valid(c, h, R):
    """every h_k >= 0, every value of c and R finite"""
    with np.errstate(invalid="ignore"):
        return (h >= 0).all(axis=-1) & np.isfinite(c).all(axis=-1) & np.isfinite(R).all(axis=(-1, -2))


def pairs(k, c, h, R=None):
    """k (..., 9), c, h (..., 3), R (..., 3, 3) or None of ONE float dtype, broadcast against each other -> (box_ok, normal_ok,
    edge_ok (...) bool: no axis of the family separates; inside (...) uint8).  The SAT clause is the AND of the three."""
    dt = k.dtype
    assert dt in (np.float32, np.float64) and c.dtype == dt and h.dtype == dt and (R is None or R.dtype == dt), (dt, c.dtype, h.dtype)
    R = identity(dt) if R is None else R
    v = [local(c, R, k[..., 3 * i:3 * i + 3]) for i in range(3)]      # v[i][k]
    H = [h[..., j] for j in range(3)]
    with np.errstate(all="ignore"):
        box_ok = np.ones(np.broadcast(v[0][0], H[0]).shape, bool)
        for j in range(3):
            box_ok = box_ok & axis_overlaps(v[0][j], v[1][j], v[2][j], H[j])
        e = [[v[1][j] - v[0][j] for j in range(3)], [v[2][j] - v[1][j] for j in range(3)], [v[0][j] - v[2][j] for j in range(3)]]
        n = [e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]]
        d = (n[0] * v[0][0] + n[1] * v[0][1]) + n[2] * v[0][2]
        rad = (np.abs(n[0]) * H[0] + np.abs(n[1]) * H[1]) + np.abs(n[2]) * H[2]
        normal_ok = (d <= rad) & (d >= -rad)
        edge_ok = np.ones(box_ok.shape, bool)
        for ex, ey, ez in e:
            edge_ok = edge_ok & axis_overlaps(*[ey * v[i][2] - ez * v[i][1] for i in range(3)], np.abs(ez) * H[1] + np.abs(ey) * H[2])
            edge_ok = edge_ok & axis_overlaps(*[ez * v[i][0] - ex * v[i][2] for i in range(3)], np.abs(ez) * H[0] + np.abs(ex) * H[2])
            edge_ok = edge_ok & axis_overlaps(*[ex * v[i][1] - ey * v[i][0] for i in range(3)], np.abs(ey) * H[0] + np.abs(ex) * H[1])
        inside = np.zeros(box_ok.shape, np.uint8)
        for i in range(3):
            held = (np.abs(v[i][0]) <= H[0]) & (np.abs(v[i][1]) <= H[1]) & (np.abs(v[i][2]) <= H[2])
            inside = inside | (held.astype(np.uint8) << np.uint8(i))
    assert all(x.dtype == dt for x in (d, rad, n[0], e[0][0], v[0][0]))   # nothing was promoted
    return box_ok, normal_ok, edge_ok, inside


class Contacts:
    """counts (m,) int64, offsets (m + 1,) int64, and per contact, grouped by box and within a box in leaf order: index (M,)
    of `idt`, inside (M,) uint8, box (M,) 0-based; refused_first (3,): among the pairs of a valid box and a triangle that pass
    the box clause, how many the box axes, the normal, the edge axes refuse first (in that order)."""


def brute_force_contacts(tris, c, h, R, leaf_order=None, leaf_boxes=None, idt=np.int64, chunk=64):
    """The definition of the result.  tris (n, 9), c, h (m, 3), R (m, 3, 3) or None (the identity) of ONE float dtype.
    leaf_order: the user indices (1-based) of the leaves in the order they lie in bvh.leaves, None = 1..n; an entry outside
    1..n names no triangle and is skipped (the entry point's guard).  leaf_boxes (n, 6): the boxes stored in the leaves, by
    triangle; None = tight boxes.  A contact iff the stored box is not apart from the hull and no axis separates; none for an
    invalid box."""
    dt = tris.dtype
    assert c.dtype == dt and h.dtype == dt and c.shape == h.shape == (len(c), 3)
    n, m = len(tris), len(c)
    R = np.array(identity(dt, (m,))) if R is None else R
    assert R.dtype == dt and R.shape == (m, 3, 3)
    boxes = tcc.tight_boxes(tris) if leaf_boxes is None else np.asarray(leaf_boxes)
    assert boxes.shape == (n, 6) and boxes.dtype == dt
    order = np.arange(1, n + 1, dtype=np.int64) if leaf_order is None else np.asarray(leaf_order).astype(np.int64)
    order = order[(order >= 1) & (order <= n)]
    cols = order - 1
    alive = valid(c, h, R)
    qlo, qup = hull(c, h, R)
    fields = ("box", "index", "inside")
    parts = {k: [] for k in fields}
    refused = np.zeros(3, np.int64)
    for s in range(0, m if n else 0, chunk):
        sl = slice(s, min(s + chunk, m))
        near = ~boxes_apart(qlo[sl, None], qup[sl, None], boxes[None, :, 0:3], boxes[None, :, 3:6]) & alive[sl, None]
        # (the 13 axes only where clause (i) passed: the result is their AND with it, over all pairs)
        r, j = np.nonzero(near)
        box_ok, normal_ok, edge_ok, mask = pairs(tris[j], c[s + r], h[s + r], R[s + r])
        refused += [int((~box_ok).sum()), int((box_ok & ~normal_ok).sum()), int((box_ok & normal_ok & ~edge_ok).sum())]
        hit, inside = np.zeros(near.shape, bool), np.zeros(near.shape, np.uint8)
        hit[r, j], inside[r, j] = box_ok & normal_ok & edge_ok, mask
        rows, js = np.nonzero(hit[:, cols])   # row-major: by box, then by leaf position
        k = cols[js]
        for key, value in zip(fields, (rows + s, order[js], inside[rows, k])):
            parts[key].append(value)
    out = Contacts()
    cat = lambda key, t: np.concatenate(parts[key]).astype(t) if parts[key] else np.empty((0,), t)
    out.box, out.index, out.inside = cat("box", np.int64), cat("index", idt), cat("inside", np.uint8)
    out.counts = np.bincount(out.box, minlength=m).astype(np.int64)
    out.offsets = np.concatenate([[0], np.cumsum(out.counts)]).astype(np.int64)
    out.refused_first = refused
    return out


in_leaf_order = functools.partial(kit.in_leaf_order, owner="box", fields=("inside",))


def first(bf, count):
    """the lists of the first `count` boxes of `bf`"""
    out = Contacts()
    rows = bf.box < count
    out.box, out.index, out.inside = bf.box[rows], bf.index[rows], bf.inside[rows]
    out.counts, out.offsets, out.refused_first = bf.counts[:count], bf.offsets[:count + 1], bf.refused_first
    return out


# ---- hand-made pairs with known answers ------------------------------------------------------------------------------------
S = float(np.sqrt(0.5))
RZ90 = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]      # the box's axis 0 is world y, its axis 1 is world -x: exact
RZ45 = [[S, S, 0], [-S, S, 0], [0, 0, 1]]      # a quarter of that
EYE = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
FLAT = tcc.FLAT                                # (0,0,0) (1,0,0) (0,1,0)
BIG = [-10, -10, 0, 10, -10, 0, 0, 10, 0]
CORNER = [0.5, 2.5, 0, 2.5, 0.5, 0, 2.5, 2.5, 0]               # in the plane z = 0, beyond the line x + y = 3
SLANTED = [23.5, -10, -10, -10, 23.5, -10, -10, -10, 23.5]     # in the plane x + y + z = 3.5, huge
ON_FACE = [1, 0, 0, 1, 0.5, 0, 1, 0, 0.5]                      # in the plane x = 1
UPRIGHT = [0, 0, -1, 0.5, 0, 1, 0, 0.5, 1]                     # through the plane z = 0
# a vertex 0.01 beyond the face's middle, the rest fanning away, given in the frame of a box turned by RZ45 about z
_FAN_LOCAL = np.array([[1.01, 0, 0], [3, 2, 1], [4, -2, -1.5]])
FAN = (_FAN_LOCAL @ np.array(RZ45)).reshape(9).tolist()        # world = R^T local (c = 0)
nan, inf = np.nan, np.inf
# name: (triangle, [(c, h, R), ...], (i) passes, box axes / normal / edge axes pass, inside or None); R None = no rotations
HAND = {
    "wholly inside": (FLAT, [((0.25, 0.25, 0), (2, 2, 1), None), ((0.25, 0.25, 0), (2, 2, 1), EYE), ((0.25, 0.25, 0), (2, 2, 1), RZ90),
                             ((0.25, 0.25, 0), (2, 2, 1), RZ45)], True, (True, True, True), 7),
    "pierced, no vertex inside": (BIG, [((0, 0, 0), (1, 1, 1), None), ((0, 0, 0), (1, 2, 1), RZ90), ((0, 0, 0), (1, 2, 1), RZ45)],
                                  True, (True, True, True), 0),
    "only an edge axis separates": (CORNER, [((0, 0, 0), (1, 1, 1), None), ((0, 0, 0), (1, 1, 1), RZ90)], True, (True, True, False), None),
    "only the normal separates": (SLANTED, [((0, 0, 0), (1, 1, 1), None), ((0, 0, 0), (1, 1, 1), RZ90)], True, (True, False, True), None),
    "only a box axis separates, the hulls overlap": (FAN, [((0, 0, 0), (1, 1, 1), RZ45)], True, (False, True, True), None),
    "the same without the rotation: the hulls are apart": (_FAN_LOCAL.reshape(9).tolist(), [((0, 0, 0), (1, 1, 1), None), ((0, 0, 0), (1, 1, 1), EYE)],
                                                            False, (False, True, True), None),
    "touching a face": (ON_FACE, [((0, 0, 0), (1, 1, 1), None), ((0, 0, 0), (1, 1, 1), RZ90), ((-1, 0, 0), (2, 1, 3), None),
                                  ((-1, 0, 0), (1, 2, 3), RZ90)], True, (True, True, True), 7),
    "a plate cuts it": (UPRIGHT, [((0, 0, 0), (1, 1, 0), None), ((0, 0, 0), (1, 1, 0), RZ45)], True, (True, True, True), 0),
    "a plate holds it": (FLAT, [((0, 0, 0), (1, 1, 0), None), ((0, 0, 0), (1, 1, 0), RZ90)], True, (True, True, True), 7),
    "a point on its face": (FLAT, [((0.25, 0.25, 0), (0, 0, 0), None), ((0.25, 0.25, 0), (0, 0, 0), RZ45)], True, (True, True, True), 0),
    "a segment through it": (FLAT, [((0.25, 0.25, 0), (0, 0, 1), None), ((0.25, 0.25, 0), (0, 0, 1), RZ90)], True, (True, True, True), 0),
}
# boxes that touch nothing, around a triangle they would hold
INVALID = [((0.25, 0.25, 0), (2, -1, 1), None), ((0.25, 0.25, 0), (2, 2, nan), RZ90), ((0.25, nan, 0), (2, 2, 1), None),
           ((0.25, 0.25, inf), (2, 2, 1), RZ45), ((0.25, 0.25, 0), (2, 2, 1), [[1, 0, 0], [0, nan, 0], [0, 0, 1]]),
           ((0.25, 0.25, 0), (2, 2, 1), [[1, 0, 0], [0, 1, 0], [0, -inf, 1]]), ((0.25, 0.25, 0), (-0.0, 2, -inf), None)]


def hand_boxes(dt):
    """every box of HAND and INVALID as one batch, rotations spelled out -> (c (n, 3), h (n, 3), R (n, 3, 3)) of `dt`; the
    first IDENTITY of them are unrotated"""
    rows = [b for case in HAND.values() for b in case[1]] + INVALID
    rows.sort(key=lambda b: not (b[2] is None or b[2] == EYE))
    c, h = np.array([b[0] for b in rows], dt), np.array([b[1] for b in rows], dt)
    R = np.array([EYE if b[2] is None else b[2] for b in rows], dt)
    return c, h, R


IDENTITY = sum(1 for case in HAND.values() for b in case[1] if b[2] is None or b[2] == EYE) + sum(1 for b in INVALID if b[2] is None)


# ---- the shared inputs -----------------------------------------------------------------------------------------------------
N_BOXES = 300


def boxes(tris, dt, n=N_BOXES, seed=71):
    """n boxes near the surface, e the mean length of edge ab: centres at a mesh vertex plus normal noise of two e, half
    extents 0.25 e .. 3 e per axis, rotations the orthonormal factor of a normal matrix (made proper) — the first quarter
    exactly the identity -> (c (n, 3), h (n, 3), R (n, 3, 3)) of `dt`"""
    from sphere_contacts_checker import mean_edge
    rng = np.random.default_rng(seed)
    t64 = tris.astype(np.float64)
    e = mean_edge(t64)
    vertex = t64.reshape(-1, 3)[rng.integers(0, 3 * len(t64), n)]
    c = (vertex + rng.normal(size=(n, 3)) * 2 * e).astype(dt)
    h = ((0.25 + 2.75 * rng.random((n, 3))) * e).astype(dt)
    q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    q[:, 2] *= np.linalg.det(q)[:, None]
    q[:n // 4] = np.eye(3)
    return c, h, q.astype(dt)


@functools.lru_cache(maxsize=None)
def reference(mesh, dt, n=N_BOXES):
    """(triangles, c, h, R, the contacts in index order with tight boxes) of a named mesh, computed once and read-only"""
    from implicitbvh_amd.synthetic import torus_mesh
    tris = torus_mesh(*kit.MESHES[mesh]).astype(dt)
    c, h, R = boxes(tris, dt, n)
    contacts = brute_force_contacts(tris, c, h, R)
    # (c, h and R go through torch.from_numpy, which wants a writable array)
    for x in (tris,) + tuple(v for v in vars(contacts).values() if isinstance(v, np.ndarray)):
        x.setflags(write=False)
    return tris, c, h, R, contacts
