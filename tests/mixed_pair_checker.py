"""A numpy restatement of the reference's leaf-vs-tree pair walk (lvt/traverse_pair.jl:1-52, 176-244) for two BVHs of any
two volume types: the checker of IBVH_PAIR_MIXED_TYPES.  It is the independent statement the oracle's own mixed walk
(oracle/ibvh_oracle.cpp, pair_lvt with IBVH_PAIR_MIXED_TYPES) is pinned to: tests/test_host_mixed_pair.py pins it to the
oracle on every same-type pair, and the oracle's mixed lists to it on every pair of two types.

A plain module, not a conftest: the tests import it.  Works on oracle_lib.HostBVH (numpy records).

The walk's result, stated without the walk: the driving BVH (more leaves; fewer with IBVH_PAIR_SMALLER_DRIVES) supplies
the queries q in leaf-position order; leaf j of the walked tree is reported for q iff
  * NodeType(q.volume) touches every ancestor of j from the walked tree's start level down to the leaf parents
    (:196-197 — the query converted to the walked tree's node type; the ancestors of a real leaf are real), and
  * iscontact(q.volume, j.volume) on the raw mixed types (iscontact.jl:2-28), and
  * narrow(bvh1 leaf, bvh2 leaf),
each query's partners in increasing position.  Arithmetic is Julia's: a conversion rounds once, a sphere's box is formed
in the sphere's own float type, mixed comparisons and sphere-sphere distances promote; no fused multiply-add (the
library is built with -ffp-contract=off).
"""
import numpy as np

from implicitbvh_amd import abi

NARROW_NONE, NARROW_MORTON_LT, NARROW_INDEX_LT = abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT


class Refused(Exception):
    """NodeType(query) does not exist: a BBox query against a tree of BSphere nodes (no BSphere(::BBox) method)."""


def _flt(flt):
    return abi.FLOAT_DTYPES[flt]


def as_fields(vols, kind):
    """Structured volumes -> dict of (n, 3) / (n,) arrays in their own float type."""
    if kind == abi.BSPHERE:
        return {"kind": kind, "x": np.asarray(vols["x"]).reshape(-1, 3), "r": np.asarray(vols["r"]).reshape(-1)}
    return {"kind": kind, "lo": np.asarray(vols["lo"]).reshape(-1, 3), "up": np.asarray(vols["up"]).reshape(-1, 3)}


def to_node_type(v, node_kind, node_flt):
    """NodeType(volume) (merge.jl:47-51 and the float conversions): one rounding into the node float type; a sphere's box
    is x -/+ r computed in the sphere's float type first."""
    t = _flt(node_flt)
    if node_kind == abi.BSPHERE:
        if v["kind"] != abi.BSPHERE:
            raise Refused("no method matching BSphere(::BBox)")
        return {"kind": abi.BSPHERE, "x": v["x"].astype(t), "r": v["r"].astype(t)}
    if v["kind"] == abi.BSPHERE:
        lo, up = _box_of(v)
        with np.errstate(over="ignore", invalid="ignore"):
            return {"kind": abi.BBOX, "lo": lo.astype(t), "up": up.astype(t)}
    with np.errstate(over="ignore"):
        return {"kind": abi.BBOX, "lo": v["lo"].astype(t), "up": v["up"].astype(t)}


def _box_of(v):
    if v["kind"] == abi.BBOX:
        return v["lo"], v["up"]
    with np.errstate(over="ignore", invalid="ignore"):  # (in the sphere's own float type, iscontact.jl:16-24)
        return v["x"] - v["r"][:, None], v["x"] + v["r"][:, None]


def contact_matrix(a, b):
    """iscontact(a[i], b[j]) for all i, j -> (len(a), len(b)) bool; a, b as as_fields() / to_node_type() give them."""
    if a["kind"] == abi.BSPHERE and b["kind"] == abi.BSPHERE:
        t = np.promote_types(a["x"].dtype, b["x"].dtype)
        ax, bx = a["x"].astype(t), b["x"].astype(t)
        with np.errstate(over="ignore", invalid="ignore"):  # (Inf and NaN are data here, as on the device)
            d = [ax[:, None, k] - bx[None, :, k] for k in range(3)]
            dist = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            rr = a["r"].astype(t)[:, None] + b["r"].astype(t)[None, :]
            return dist <= rr * rr
    alo, aup = _box_of(a)
    blo, bup = _box_of(b)
    m = np.ones((alo.shape[0], blo.shape[0]), bool)
    for k in range(3):  # (numpy compares float32 with float64 exactly, after promotion)
        m &= (aup[:, None, k] >= blo[None, :, k]) & (alo[:, None, k] <= bup[None, :, k])
    return m


def iscontact(kind_a, flt_a, a, kind_b, flt_b, b):
    """The leaf test on two single volumes given as numbers (the oracle_lib.iscontact signature)."""
    va = np.asarray(a, _flt(flt_a)).reshape(1, -1)
    vb = np.asarray(b, _flt(flt_b)).reshape(1, -1)
    fa = {"kind": kind_a, "x": va[:, :3], "r": va[:, 3]} if kind_a == abi.BSPHERE else {"kind": kind_a, "lo": va[:, :3], "up": va[:, 3:]}
    fb = {"kind": kind_b, "x": vb[:, :3], "r": vb[:, 3]} if kind_b == abi.BSPHERE else {"kind": kind_b, "lo": vb[:, :3], "up": vb[:, 3:]}
    return bool(contact_matrix(fa, fb)[0, 0])


def _level_first_mem(tree, level):
    """0-based position in the nodes array of the first real node of `level` (implicit index 2^(level-1))."""
    import oracle_lib as orc
    return orc.level_indices(tree, level)[0] - 1


def driver_of(bvh1, bvh2, smaller_drives=False):
    """-> flip: True when bvh2 supplies the work items (:15-36; IBVH_PAIR_SMALLER_DRIVES the other way round)."""
    n1, n2 = bvh1.tree.real_leaves, bvh2.tree.real_leaves
    return n1 > n2 if smaller_drives else not (n1 >= n2)


def traverse_pair_lvt(bvh1, bvh2, start_level1=None, start_level2=None, narrow=0, positions=False, smaller_drives=False):
    """The reference's contact list of traverse(bvh1, bvh2, LVTTraversal()) as an (m, 2) int64 array of (bvh1, bvh2) user
    indices (positions=True: 1-based leaf positions), in the reference's order.  Raises Refused for the combination the
    reference has no NodeType conversion for."""
    sl1 = max(1, bvh1.built_level) if start_level1 is None else start_level1
    sl2 = max(1, bvh2.built_level) if start_level2 is None else start_level2
    flip = driver_of(bvh1, bvh2, smaller_drives)
    drv, oth, sl = (bvh2, bvh1, sl1) if flip else (bvh1, bvh2, sl2)
    dt, ot = drv.types, oth.types
    q = as_fields(drv.leaves["volume"], dt.leaf_kind)
    qn = to_node_type(q, ot.node_kind, ot.node_float)
    lv = as_fields(oth.leaves["volume"], ot.leaf_kind)
    hit = contact_matrix(q, lv)  # (queries, walked leaves)
    levels = oth.tree.levels
    nl = oth.tree.real_leaves
    leaf_implicit = (1 << (levels - 1)) + np.arange(nl, dtype=np.int64)
    for level in range(sl, levels):  # every ancestor from the start level down to the leaf parents
        implicit = leaf_implicit >> (levels - level)
        uniq, inv = np.unique(implicit, return_inverse=True)
        rows = _level_first_mem(oth.tree, level) + (uniq - (1 << (level - 1)))
        nodes = as_fields(oth.nodes[rows], ot.node_kind)
        hit &= contact_matrix(qn, nodes)[:, inv]
    if narrow != NARROW_NONE:
        if narrow == NARROW_MORTON_LT:  # Julia promotes two Morton widths: compare as UInt64
            kq, ko = drv.leaves["morton"].astype(np.uint64), oth.leaves["morton"].astype(np.uint64)
        elif narrow == NARROW_INDEX_LT:
            kq, ko = drv.leaves["index"].astype(np.int64), oth.leaves["index"].astype(np.int64)
        else:
            raise ValueError(f"narrow {narrow} is not on the pair menu")
        hit &= (ko[None, :] < kq[:, None]) if flip else (kq[:, None] < ko[None, :])  # narrow(bvh1 leaf, bvh2 leaf)
    qi, li = np.nonzero(hit)  # row-major: queries in position order, each one's partners in increasing position
    if positions:
        a, b = qi.astype(np.int64) + 1, li.astype(np.int64) + 1
    else:
        a, b = drv.leaves["index"][qi].astype(np.int64), oth.leaves["index"][li].astype(np.int64)
    return np.stack([b, a], axis=1) if flip else np.stack([a, b], axis=1)


def random_volumes(rng, n, kind, flt, scale=6.0, size=1.0, origin=0.0):
    """(n, 4 | 6) random spheres / boxes in the float type flt: centres in [origin, origin + scale)^3, extents ~ size."""
    f = _flt(flt)
    c = (origin + scale * rng.random((n, 3))).astype(f)
    if kind == abi.BSPHERE:
        r = (size * (0.1 + 0.9 * rng.random((n, 1)))).astype(f)
        return np.concatenate([c, r], axis=1)
    h = (size * (0.1 + 0.9 * rng.random((n, 3)))).astype(f)
    return np.concatenate([c - h, c + h], axis=1)


# every (leaf, node) combination the library instantiates: NodeType(leaf) exists (no BSphere(::BBox)), any two float types
LEAF_NODE_COMBOS = [(lk, lf, nk, nf) for lk in (abi.BSPHERE, abi.BBOX) for lf in (abi.F32, abi.F64)
                    for nk in (abi.BSPHERE, abi.BBOX) for nf in (abi.F32, abi.F64) if not (nk == abi.BSPHERE and lk == abi.BBOX)]
