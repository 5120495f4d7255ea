"""Checker of ibvh_cast_spheres (include/ibvh.h): a numpy restatement of the definition in the INPUT dtype (float32 inputs are
never promoted: every numpy operation below rounds once, like the kernel's, which is compiled without contraction and with a
correctly rounded divide and square root) — steps 1 to 3, the touching test of iscontact(BSphere, BSphere) and the ray-against-
sphere quadratic; steps 4 and 5, the slab entry (tests/ray_cast_checker.py) of the leaf's own box and of the STORED box directly
above the leaf, both grown by the query's radius; the clamped time, the limit, the skipped leaf — and the brute force over ALL
leaves, which is the definition of the result: the lexicographic minimum of (t*, index) over the hits, "a hit exists" for any
hit.  It needs no walk of the tree: only the leaf order and the stored boxes of one level (tree_inputs).  Per query it also
reports the runner-up, whether the winner touches at the start, whether a clamp was active, whether the winning t* is tied,
and the answer WITHOUT step 5.  And the clouds and queries the tests share (reference).  Host only."""
import functools

import numpy as np

from ray_cast_checker import limit, slab_entry


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _max(a, b):
    """the header's select a > b ? a : b"""
    with np.errstate(invalid="ignore"):
        return np.where(a > b, a, b)


def first_touch(c, R, p, d, r):
    """Steps 1 to 3 for c, p, d (..., 3) and R, r (...) of ONE float dtype, broadcast against each other -> t_k: 0 where the two
    spheres touch at the start, else the smaller root where it is valid, +Inf where there is none (a NaN anywhere: +Inf)"""
    dt = p.dtype
    assert dt in (np.float32, np.float64) and all(x.dtype == dt for x in (c, R, d, r))
    inf = dt.type(np.inf)
    with np.errstate(all="ignore"):
        S = R + r
        m = p - c
        mm = _dot(m, m)
        S2 = S * S
        B = _dot(m, d)
        dd = _dot(d, d)
        Cq = mm - S2
        disc = B * B - dd * Cq
        t = (-B - np.sqrt(disc)) / dd
        valid = (mm > S2) & (dd > 0) & (disc >= 0) & (t >= 0)
        out = np.where(mm <= S2, dt.type(0), np.where(valid, t, inf))
    assert out.dtype == dt
    return out


def sphere_boxes(spheres):
    """(lo, up) = (c - R, c + R) in the spheres' dtype: convert(BSphere -> BBox), merge.jl:47-51"""
    return spheres[:, :3] - spheres[:, 3:4], spheres[:, :3] + spheres[:, 3:4]


def grown_entry(lo, up, p, d, r):
    """entry of the ray (p, d) into the box (lo, up) grown by r, all broadcast against each other, in ONE dtype"""
    e, _ = slab_entry(lo - r[..., None], up + r[..., None], p, d)
    return e


def parent_level(levels, virtual_leaves, built_level):
    """(first row, rows) of the level directly above the leaves in the node array, None where step 5 does not apply"""
    if not (levels >= 2 and built_level <= levels - 1):
        return None
    v = virtual_leaves >> 2                                    # level_skips(levels, virtual_leaves, levels - 1)
    skips = 2 * v - bin(v).count("1")
    return (1 << (levels - 2)) - skips - 1, (1 << (levels - 2)) - (virtual_leaves >> 1)


def tree_inputs(leaf_index, nodes, levels, virtual_leaves, built_level):
    """what the brute force needs of a built BVH: leaf_order (n,) the user index of the leaf at each position, and parent_boxes
    (ceil(n / 2), 6) the stored boxes of the level directly above the leaves (the leaf at position j is below row j >> 1), or
    None where that level does not exist or is not built"""
    order = np.asarray(leaf_index).astype(np.int64)
    lvl = parent_level(int(levels), int(virtual_leaves), int(built_level))
    if lvl is None:
        return order, None
    boxes = np.asarray(nodes).reshape(-1, 6)[lvl[0]:lvl[0] + lvl[1]]
    assert len(boxes) == (len(order) + 1) // 2
    return order, boxes.copy()


def host_tree(spheres, node_dt=None, built_level=1):
    """the CPU oracle's build (tests/oracle_lib.py) over `spheres` -> (leaf_order, parent_boxes, the host BVH)"""
    import oracle_lib
    from implicitbvh_amd import abi
    flt = {np.float32: abi.F32, np.float64: abi.F64}
    node_dt = spheres.dtype.type if node_dt is None else node_dt
    types = abi.make_types(abi.BSPHERE, flt[spheres.dtype.type], abi.BBOX, flt[node_dt])
    bvh = oracle_lib.build(spheres, types, built_level=built_level)
    nodes = np.concatenate([bvh.nodes["lo"], bvh.nodes["up"]], axis=1) if len(bvh.nodes) else np.zeros((0, 6), node_dt)
    order, boxes = tree_inputs(bvh.leaves["index"], nodes, bvh.tree.levels, bvh.tree.virtual_leaves, built_level)
    return order, boxes, bvh


class Cast:
    """index (m,) of `idt` (0 = miss), t (m,) (+Inf = miss), touched (m,) uint8: the outputs.  hits (m,): the number of hits
    within the limit; second_index, second_t: the runner-up (0, +Inf: none); tied (m,): the runner-up has the winner's t*;
    start (m,): the winner touches at the start (t_k == 0); clamp_own, clamp_parent (m,): the winner's own / parent entry
    exceeds what came before it in step 6; index_no5, t_no5: the answer without step 5"""


def _two_smallest(ts, hit, idx):
    """per row the lexicographic minimum of (ts, idx) over `hit` and the runner-up -> (i1, t1, i2, t2); 0 / +Inf: none"""
    inf = ts.dtype.type(np.inf)
    m = len(ts)
    rows = np.arange(m)
    out = []
    key = np.where(hit, ts, inf)
    left = hit.copy()
    for _ in range(2):
        best = key.min(axis=1) if key.shape[1] else np.full(m, inf, ts.dtype)
        cand = left & (key == best[:, None])
        who = np.where(cand, idx[None, :], np.iinfo(np.int64).max).min(axis=1) if key.shape[1] else np.zeros(m, np.int64)
        has = cand.any(axis=1)
        out += [np.where(has, who, 0), np.where(has, best, inf)]
        # the winner leaves (ONE leaf: among leaves of one index and one t* the first position)
        pos = np.argmax(cand & (idx[None, :] == who[:, None]), axis=1)
        left[rows[has], pos[has]] = False
        key = np.where(left, key, inf)
    return out


def brute_force(spheres, leaf_order, parent_boxes, p, d, r, t_max=None, skip=None, idt=np.int64, chunk=100):
    """Steps 1 to 8 of include/ibvh.h.  spheres (n, 4): the cloud in the USER's order (user index k = row k - 1); leaf_order,
    parent_boxes: tree_inputs(); p, d (m, 3), r (m,) of the spheres' dtype; t_max (m,) or None; skip (m,) user indices or None"""
    v = np.asarray(spheres)
    dt = v.dtype.type
    assert dt in (np.float32, np.float64) and p.dtype == dt and d.dtype == dt and r.dtype == dt, (v.dtype, p.dtype, d.dtype, r.dtype)
    order = np.asarray(leaf_order).astype(np.int64)
    n, m = len(order), len(p)
    leaves = v[order - 1]                                       # by position
    c, R = leaves[:, :3], leaves[:, 3]
    lo, up = sphere_boxes(leaves)
    if parent_boxes is not None:
        pb = np.asarray(parent_boxes).astype(dt)[np.arange(n) >> 1]     # narrowed to T (exact), one row per leaf
    L = limit(t_max, m, dt)
    s = np.zeros(m, np.int64) if skip is None else np.asarray(skip).astype(np.int64)
    with np.errstate(invalid="ignore"):
        asks = ~np.isnan(p).any(axis=1) & ~np.isnan(d).any(axis=1) & (r >= 0) & (L >= 0)
    out = Cast()
    cols = {k: [] for k in ("index", "t", "hits", "second_index", "second_t", "start", "clamp_own", "clamp_parent", "index_no5", "t_no5")}
    inf = dt(np.inf)
    for a in range(0, m, chunk):
        q = slice(a, a + chunk)
        P, D, Rq = p[q, None, :], d[q, None, :], r[q, None]
        tk = first_touch(c[None], R[None], P, D, Rq)
        own = grown_entry(lo[None], up[None], P, D, Rq)
        t4 = _max(tk, own)
        if parent_boxes is not None:
            above = grown_entry(pb[None, :, :3], pb[None, :, 3:], P, D, Rq)
            ts = _max(t4, above)
        else:
            above = np.full_like(t4, -inf)
            ts = t4
        assert ts.dtype == dt
        with np.errstate(invalid="ignore"):
            can = asks[q, None] & (order[None, :] != s[q, None])
            hit, hit4 = can & (ts <= L[q, None]), can & (t4 <= L[q, None])
        i1, t1, i2, t2 = _two_smallest(ts, hit, order)
        j1, u1, _, _ = _two_smallest(t4, hit4, order)
        # facts about the winner (the leaf of index i1 with t* == t1; duplicated spheres share them)
        win = hit & (order[None, :] == i1[:, None]) & (ts == t1[:, None])
        pos = np.argmax(win, axis=1)
        rows = np.arange(len(pos))
        has = i1 != 0
        with np.errstate(invalid="ignore"):
            cols["start"].append(has & (tk[rows, pos] == 0))
            cols["clamp_own"].append(has & (own[rows, pos] > tk[rows, pos]))
            cols["clamp_parent"].append(has & (above[rows, pos] > t4[rows, pos]))
        for k, x in (("index", i1), ("t", t1), ("hits", hit.sum(axis=1)), ("second_index", i2), ("second_t", t2), ("index_no5", j1), ("t_no5", u1)):
            cols[k].append(x)
    for k, parts in cols.items():
        setattr(out, k, np.concatenate(parts) if parts else np.zeros(0))
    out.index, out.second_index, out.index_no5 = out.index.astype(idt), out.second_index.astype(idt), out.index_no5.astype(idt)
    out.t, out.second_t, out.t_no5 = out.t.astype(dt), out.second_t.astype(dt), out.t_no5.astype(dt)
    out.touched = (out.index != 0).astype(np.uint8)
    out.tied = (out.second_index != 0) & (out.second_t == out.t)
    return out


# ---- the shared cases ---------------------------------------------------------------------------------------------------------
def cloud(dt, seed=7):
    """3,000 spheres in the unit cube, radii 0.01 to 0.04, and the first 300 again as leaves 3,001 to 3,300 (exact ties); 800
    queries from [-0.2, 1.2]^3, directions of length 0.2 to 0.8, r in 0 to 0.03 with every fourth r = 0"""
    rng = np.random.default_rng(seed)
    base = np.concatenate([rng.random((3000, 3)), 0.01 + 0.03 * rng.random((3000, 1))], axis=1)
    spheres = np.concatenate([base, base[:300]]).astype(dt)
    p = (rng.random((800, 3)) * 1.4 - 0.2).astype(dt)
    u = rng.normal(size=(800, 3))
    d = (u / np.linalg.norm(u, axis=1, keepdims=True) * (0.2 + 0.6 * rng.random((800, 1)))).astype(dt)
    r = (0.03 * rng.random(800)).astype(dt)
    r[::4] = 0
    return spheres, p, d, r


def lattice(dt, seed=11):
    """an 8 x 8 x 8 jittered grid of spheres, radii 0.02 to 0.05; 600 axis-parallel queries aimed at leaf centres from outside
    the cube, two of three with r = 0"""
    rng = np.random.default_rng(seed)
    g = (np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) / 8
    spheres = np.concatenate([g + 0.02 * (rng.random(g.shape) - 0.5), 0.02 + 0.03 * rng.random((len(g), 1))], axis=1).astype(dt)
    target = spheres[rng.integers(0, len(spheres), 600), :3]
    axis, sign = rng.integers(0, 3, 600), rng.choice([-1.0, 1.0], 600)
    p = target.copy()
    d = np.zeros((600, 3), dt)
    rows = np.arange(600)
    p[rows, axis] = np.where(sign > 0, -0.5 - rng.random(600), 1.5 + rng.random(600)).astype(dt)   # outside, looking in
    d[rows, axis] = (sign * (0.5 + rng.random(600))).astype(dt)
    r = (0.02 * rng.random(600)).astype(dt)
    r[np.arange(600) % 3 != 0] = 0
    return spheres, p, d, r


def nested_pairs(dt, pairs=150, seed=13, candidates=60000):
    """Pairs of spheres internally tangent along a coordinate axis for which the merge's shortcut fires (length + q <= R in
    rounded arithmetic) AND the inner sphere's box pokes out of the outer's -> spheres (2 * pairs, 4): rows 2i (outer) and
    2i + 1 (inner); axis, sign (pairs,): where it pokes; how many candidates fired, how many of those poke.  That takes an
    outer centre whose coordinate along the axis is of the radii's size (a far larger one is rounded so coarsely that a pair
    which pokes does not fire), so the pairs sit far apart in the OTHER two coordinates: one pair per cell, 8 wide, of a
    15 x 15 grid in the plane across its axis."""
    rng = np.random.default_rng(seed)
    cell = np.arange(candidates) % 225
    axis, sign = rng.integers(0, 3, candidates), rng.choice([-1, 1], candidates)
    rows = np.arange(candidates)
    across = np.stack([cell // 15, cell % 15], axis=1) * 8.0 + 4.0 + rng.random((candidates, 2)) * 2 - 1
    C = np.empty((candidates, 3))
    C[rows, axis], C[rows, (axis + 1) % 3], C[rows, (axis + 2) % 3] = rng.random(candidates) - 0.5, across[:, 0], across[:, 1]
    C = C.astype(dt)
    R = (0.2 + 0.3 * rng.random(candidates)).astype(dt)
    q = (R * (0.1 + 0.8 * rng.random(candidates)).astype(dt)).astype(dt)
    ci = C.copy()
    ci[rows, axis] = C[rows, axis] + sign.astype(dt) * (R - q)
    e = ci - C
    length = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])          # dist3 of the merge
    fires = length + q <= R
    tip_in, tip_out = ci[rows, axis] + sign.astype(dt) * q, C[rows, axis] + sign.astype(dt) * R
    pokes = np.where(sign > 0, tip_in > tip_out, tip_in < tip_out)
    assert length.dtype == dt and tip_in.dtype == dt
    good = np.flatnonzero(fires & pokes)
    _, first = np.unique(cell[good], return_index=True)              # one pair per cell
    keep = good[np.sort(first)][:pairs]
    spheres = np.empty((2 * len(keep), 4), dt)
    spheres[0::2] = np.concatenate([C[keep], R[keep, None]], axis=1)
    spheres[1::2] = np.concatenate([ci[keep], q[keep, None]], axis=1)
    return spheres, axis[keep], sign[keep], int(fires.sum()), int((fires & pokes).sum())


def nested(dt, seed=13):
    """the nested pairs, a tip query per pair — from the poking tip of the inner sphere's box, not moving along that axis,
    r = 0, skipping the outer sphere — and 200 random queries -> spheres, p, d, r, skip, (axis, sign)"""
    spheres, axis, sign, _, _ = nested_pairs(dt, seed=seed)
    k = len(axis)
    rng = np.random.default_rng(seed + 1)
    inner = spheres[1::2]
    rows = np.arange(k)
    tip = inner[:, :3].copy()
    tip[rows, axis] = inner[rows, axis] + sign.astype(dt) * inner[:, 3]
    dtip = (rng.random((k, 3)) - 0.5).astype(dt)
    dtip[rows, axis] = 0
    which = rng.integers(0, k, 200)
    pr = (spheres[2 * which, :3] + (rng.random((200, 3)) * 2 - 1)).astype(dt)
    dr = (rng.random((200, 3)) * 2 - 1).astype(dt)
    p, d = np.concatenate([tip, pr]), np.concatenate([dtip, dr])
    r = np.concatenate([np.zeros(k, dt), (0.1 * rng.random(200)).astype(dt)])
    skip = np.concatenate([2 * rows + 1, np.zeros(200, np.int64)])         # the outer sphere's user index
    return spheres, p, d, r, skip, (axis, sign)


def sibling_pairs(spheres, leaf_order, parent_boxes):
    """which pairs (rows 2i, 2i + 1 of nested_pairs) are siblings whose stored parent box has the bits of the outer sphere's
    box -> bool (pairs,)"""
    order = np.asarray(leaf_order).astype(np.int64)
    position = np.empty(len(order), np.int64)
    position[order - 1] = np.arange(len(order))
    outer, inner = position[0::2], position[1::2]
    lo, up = sphere_boxes(spheres[0::2])
    box = np.concatenate([lo, up], axis=1).astype(parent_boxes.dtype)
    return ((outer >> 1) == (inner >> 1)) & (parent_boxes[outer >> 1] == box).all(axis=1)


@functools.lru_cache(maxsize=None)
def reference(dt):
    """name -> (spheres, p, d, r, skip or None), computed once, shared, read-only"""
    out = {}
    out["cloud"] = cloud(dt) + (None,)
    out["lattice"] = lattice(dt) + (None,)
    out["nested"] = nested(dt)[:5]
    for arrays in out.values():
        for x in arrays:
            if x is not None:
                x.setflags(write=False)
    return out
