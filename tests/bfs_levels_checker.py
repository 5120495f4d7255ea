"""A numpy restatement of the level-synchronous (breadth-first) walk, step by step as the library plans it
(csrc/ibvh_bfs.hip: run_self / run_pair / run_rays): the checker of the BFS level kernel's per-step counters and queues.
tests/test_host_bfs_levels.py pins it to the oracle's BFS (contact set, num_checks) on every type combination.

A plain module, not a conftest: the tests import it.  Works on oracle_lib.HostBVH (numpy records).

Definition.  A step GENERATES pairs and CHECKS them at once; what passes is the next step's SOURCE.  Step 0 generates the
initial queue (fill_initial_bvtt_*: bfs/traverse_single.jl:102-167, traverse_pair.jl:195-219,
raytrace/breadth_first/breadth_first.jl:116-137) and checks it at the start level(s); step s > 0 generates the children of
its source pairs and checks them one level further down; what passes the last step — the leaf test and `narrow` — is the
contact list.  Every generated pair is one check of the reference (bfs/traverse_single.jl:25,48): num_checks is the sum of
the generated counts.  The rules, from the files the kernel's policies cite:
  self   (traverse_single_cpu.jl:64-133, 184-219): the initial queue holds (i, j), i <= j, of the start level — i < j only
         when that is the leaf level; a node pair (a, a) passes untested; its children are (2a, 2a), (2a, 2a+1), (2a+1, 2a+1)
         while self_checks = level < levels - 1, else only (2a, 2a+1); a virtual right child drops every pair that names it;
         (a, b), a < b: {2a, 2a+1} x {2b, 2b+1}; contacts are (min, max) of the two user indices.
  pair   (traverse_pair.jl:50-143, traverse_pair_cpu.jl): the six phases of run_pair — both sides descend while both are
         above their leaf parents, then the deeper side alone down to its leaf parents, then a side whose partner is at leaf
         level descends alone to its leaves, else one last joint step; then leaf against leaf.  Contacts are
         (leaf1.index, leaf2.index), not re-ordered.
  rays   (raytrace_cpu.jl:62-101, 151-182): pairs are (node, ray); every real node of the start level against every ray.
Contact tests are mixed_pair_checker.contact_matrix on the volumes' own types (Julia's promotion, no contraction); ray tests
are the oracle's scalar isintersection (oracle_lib.brute_force_rays over one level's volumes); narrowing reads the Morton
and index columns.
"""
import numpy as np

import mixed_pair_checker as mpc
import oracle_lib as orc
from implicitbvh_amd import abi

# The level kernel's geometry (csrc/ibvh_bfs.hip; tests/test_host_bfs_levels.py reads the source and compares): what the
# route tests' preconditions are worked out from.
TPB = 256        # lanes of a workgroup = source pairs of a chunk
GEN_SLOTS = 16   # words per step the workgroups spread their check counts over
STAGE = 3072     # pairs a workgroup stages in LDS: 24 KB of Int32 pairs, 48 KB of Int64 pairs
MAXOUT = {"initial": 1, "self": 4, "pair": 4, "rays": 2}  # most pairs a lane produces: step 0, the later steps of each traversal


def flush_threshold(kind):
    """a workgroup flushes inside its loop once it has staged more than this many pairs"""
    return STAGE - MAXOUT[kind] * TPB


class Step:
    """source: sorted (m, 2) int64 implicit-index pairs the step reads (step 0: the initial queue); generated: pairs it
    generates and checks; passed: pairs that pass = the next step's source count, or the number of contacts."""

    def __init__(self, source, generated, passed):
        self.source, self.generated, self.passed = source, int(generated), int(passed)


class Trace:
    def __init__(self, steps, contacts, positions):
        self.steps, self.contacts, self.positions = steps, contacts, positions
        self.num_checks = sum(s.generated for s in steps)
        self.num_contacts = len(contacts)


def sort_pairs(p):
    p = np.asarray(p, np.int64).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def level_num_real(tree, level):
    return (1 << (level - 1)) - (tree.virtual_leaves >> (tree.levels - level))


def _right_child_virtual(tree, level, x):
    """is 2x + 1 (a child of x on `level`) virtual?"""
    return (2 * x + 1 - (1 << level)) >= level_num_real(tree, level + 1)


def _level_volumes(bvh, level):
    """the real volumes of one level in implicit order, as structured records, with their kind and float type"""
    n = level_num_real(bvh.tree, level)
    if level == bvh.tree.levels:
        return bvh.leaves["volume"][:n], bvh.types.leaf_kind, bvh.types.leaf_float
    first = mpc._level_first_mem(bvh.tree, level)
    return bvh.nodes[first:first + n], bvh.types.node_kind, bvh.types.node_float


def _contact_table(tables, bvh1, l1, bvh2, l2):
    key = ("c", id(bvh1), l1, id(bvh2), l2)
    if key not in tables:
        v1, k1, _ = _level_volumes(bvh1, l1)
        v2, k2, _ = _level_volumes(bvh2, l2)
        tables[key] = mpc.contact_matrix(mpc.as_fields(v1, k1), mpc.as_fields(v2, k2))
    return tables[key]


def _narrow_ok(narrow, l1, p1, l2, p2):
    """narrow(leaf1, leaf2) for 0-based leaf positions p1 into l1, p2 into l2"""
    if narrow == abi.NARROW_NONE:
        return np.ones(len(p1), bool)
    if narrow == abi.NARROW_MORTON_LT:
        return l1["morton"][p1].astype(np.uint64) < l2["morton"][p2].astype(np.uint64)
    if narrow == abi.NARROW_INDEX_LT:
        return l1["index"][p1].astype(np.int64) < l2["index"][p2].astype(np.int64)
    raise ValueError(f"narrow {narrow} is not on the pair menu")


def _pairs(a, b):
    return np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64)], axis=1)


def _cat(parts):
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 2), np.int64)


# ---------------------------------------------------------------------------------------------
# one BVH against itself
# ---------------------------------------------------------------------------------------------
def self_initial(bvh, start_level):
    n = level_num_real(bvh.tree, start_level)
    first = 1 << (start_level - 1)
    i, j = np.triu_indices(n, k=0 if start_level != bvh.tree.levels else 1)
    return _pairs(first + i, first + j)


def _self_children(tree, level, src):
    self_checks = level < tree.levels - 1
    a, b = src[:, 0], src[:, 1]
    same = a == b
    s = a[same]
    sv = _right_child_virtual(tree, level, s)
    out = []
    if self_checks:
        out.append(_pairs(2 * s, 2 * s))
        out.append(_pairs(2 * s[~sv], 2 * s[~sv] + 1))
        out.append(_pairs(2 * s[~sv] + 1, 2 * s[~sv] + 1))
    else:
        out.append(_pairs(2 * s[~sv], 2 * s[~sv] + 1))
    a, b = a[~same], b[~same]  # (a is left of b: its children are real)
    bv = _right_child_virtual(tree, level, b)
    out.append(_pairs(2 * a, 2 * b))
    out.append(_pairs(2 * a + 1, 2 * b))
    out.append(_pairs(2 * a[~bv], 2 * b[~bv] + 1))
    out.append(_pairs(2 * a[~bv] + 1, 2 * b[~bv] + 1))
    return _cat(out)


def trace_self(bvh, start_level, narrow=abi.NARROW_NONE, tables=None):
    tables = {} if tables is None else tables
    tree, levels = bvh.tree, bvh.tree.levels
    gen, src, level, steps = self_initial(bvh, start_level), None, start_level, []
    while True:
        first = 1 << (level - 1)
        a, b = gen[:, 0] - first, gen[:, 1] - first
        ok = _contact_table(tables, bvh, level, bvh, level)[a, b]
        if level == levels:
            ok = ok & _narrow_ok(narrow, bvh.leaves, a, bvh.leaves, b)
        else:
            ok = ok | (a == b)  # a node against itself is not tested
        passed = gen[ok]
        steps.append(Step(sort_pairs(gen if src is None else src), len(gen), len(passed)))
        if level == levels:
            break
        src, gen, level = passed, _self_children(tree, level, passed), level + 1
    first = 1 << (levels - 1)
    idx = bvh.leaves["index"].astype(np.int64)
    ia, ib = idx[passed[:, 0] - first], idx[passed[:, 1] - first]
    return Trace(steps, _pairs(np.minimum(ia, ib), np.maximum(ia, ib)), passed - first + 1)


# ---------------------------------------------------------------------------------------------
# two BVHs
# ---------------------------------------------------------------------------------------------
def pair_plan(levels1, levels2, sl1, sl2):
    """run_pair's list: (level1, level2, side 1 descends, side 2 descends) of every step's CHECK; the flags say how the
    next step's pairs are generated from what passes (the last entry, leaf against leaf, descends nowhere)."""
    plan, l1, l2 = [], sl1, sl2
    while l1 < levels1 - 1 and l2 < levels2 - 1:
        plan.append((l1, l2, True, True))
        l1, l2 = l1 + 1, l2 + 1
    while l1 < levels1 - 1 and l2 == levels2 - 1:
        plan.append((l1, l2, True, False))
        l1 += 1
    while l2 < levels2 - 1 and l1 == levels1 - 1:
        plan.append((l1, l2, False, True))
        l2 += 1
    while l2 == levels2 and l1 < levels1:
        plan.append((l1, l2, True, False))
        l1 += 1
    while l1 == levels1 and l2 < levels2:
        plan.append((l1, l2, False, True))
        l2 += 1
    if l1 == levels1 - 1 and l2 == levels2 - 1:
        plan.append((l1, l2, True, True))
        l1, l2 = l1 + 1, l2 + 1
    assert (l1, l2) == (levels1, levels2)
    plan.append((l1, l2, False, False))
    return plan


def pair_phase_names(levels1, levels2, sl1, sl2):
    """the branch of run_pair's plan each step belongs to (the route tests assert which ones a shape reaches)"""
    names = []
    for l1, l2, d1, d2 in pair_plan(levels1, levels2, sl1, sl2):
        leaf1, leaf2 = l1 == levels1, l2 == levels2
        if leaf1 and leaf2:
            names.append("leaf-leaf")
        elif leaf2:
            names.append("leaf 2 fixed, 1 descends")
        elif leaf1:
            names.append("leaf 1 fixed, 2 descends")
        elif d1 and d2:
            names.append("last joint step" if (l1, l2) == (levels1 - 1, levels2 - 1) else "both descend")
        else:
            names.append("only 1 descends" if d1 else "only 2 descends")
    return names


def pair_initial(bvh1, bvh2, sl1, sl2):
    n1, n2 = level_num_real(bvh1.tree, sl1), level_num_real(bvh2.tree, sl2)
    i, j = np.divmod(np.arange(n1 * n2, dtype=np.int64), max(n2, 1))
    return _pairs((1 << (sl1 - 1)) + i, (1 << (sl2 - 1)) + j)


def _pair_children(t1, l1, t2, l2, d1, d2, src):
    a, b = src[:, 0], src[:, 1]
    if d1 and d2:
        v1, v2 = _right_child_virtual(t1, l1, a), _right_child_virtual(t2, l2, b)
        return _cat([_pairs(2 * a, 2 * b), _pairs(2 * a[~v2], 2 * b[~v2] + 1), _pairs(2 * a[~v1] + 1, 2 * b[~v1]),
                     _pairs(2 * a[~v1 & ~v2] + 1, 2 * b[~v1 & ~v2] + 1)])
    if d1:
        v1 = _right_child_virtual(t1, l1, a)
        return _cat([_pairs(2 * a, b), _pairs(2 * a[~v1] + 1, b[~v1])])
    v2 = _right_child_virtual(t2, l2, b)
    return _cat([_pairs(a, 2 * b), _pairs(a[~v2], 2 * b[~v2] + 1)])


def trace_pair(bvh1, bvh2, sl1, sl2, narrow=abi.NARROW_NONE, tables=None):
    tables = {} if tables is None else tables
    t1, t2 = bvh1.tree, bvh2.tree
    gen, src, steps = pair_initial(bvh1, bvh2, sl1, sl2), None, []
    plan = pair_plan(t1.levels, t2.levels, sl1, sl2)
    for k, (l1, l2, d1, d2) in enumerate(plan):
        a, b = gen[:, 0] - (1 << (l1 - 1)), gen[:, 1] - (1 << (l2 - 1))
        ok = _contact_table(tables, bvh1, l1, bvh2, l2)[a, b]
        if k == len(plan) - 1:
            ok = ok & _narrow_ok(narrow, bvh1.leaves, a, bvh2.leaves, b)
        passed = gen[ok]
        steps.append(Step(sort_pairs(gen if src is None else src), len(gen), len(passed)))
        if k < len(plan) - 1:
            src, gen = passed, _pair_children(t1, l1, t2, l2, d1, d2, passed)
    pos = _pairs(passed[:, 0] - (1 << (t1.levels - 1)) + 1, passed[:, 1] - (1 << (t2.levels - 1)) + 1)
    contacts = _pairs(bvh1.leaves["index"].astype(np.int64)[pos[:, 0] - 1], bvh2.leaves["index"].astype(np.int64)[pos[:, 1] - 1])
    return Trace(steps, contacts, pos)


# ---------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------
def _ray_table(tables, bvh, level, p, d):
    key = ("r", id(bvh), level, id(p), id(d))
    if key not in tables:
        vols, kind, flt = _level_volumes(bvh, level)
        hit = np.zeros((len(vols), len(p)), bool)
        plain = np.ascontiguousarray(vols).view(abi.FLOAT_DTYPES[flt]).reshape(len(vols), abi.volume_width(kind))
        h = orc.brute_force_rays(kind, flt, plain, p, d)  # 1-based (volume, ray)
        hit[h[:, 0] - 1, h[:, 1] - 1] = True
        tables[key] = hit
    return tables[key]


def _origin_outside(leaves, kind, pos, pts):
    """IBVH_NARROW_RAY_ORIGIN_OUTSIDE: strictly outside the sphere; beyond a face of the box on some axis"""
    v = leaves["volume"][pos]
    with np.errstate(all="ignore"):
        if kind == abi.BSPHERE:
            dd = pts - v["x"]
            return dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2] > v["r"] * v["r"]
        return ((pts < v["lo"]) | (pts > v["up"])).any(axis=1)


def trace_rays(bvh, points, directions, start_level, narrow=abi.NARROW_NONE, tables=None):
    """points, directions: (num_rays, 3) arrays of the leaf float type"""
    tables = {} if tables is None else tables
    tree, levels = bvh.tree, bvh.tree.levels
    nr = len(points)
    n0 = level_num_real(tree, start_level)
    i, j = np.divmod(np.arange(n0 * nr, dtype=np.int64), max(nr, 1))
    gen, src, level, steps = _pairs((1 << (start_level - 1)) + i, 1 + j), None, start_level, []
    while True:
        a, r = gen[:, 0] - (1 << (level - 1)), gen[:, 1] - 1
        ok = _ray_table(tables, bvh, level, points, directions)[a, r]
        if level == levels and narrow == abi.NARROW_RAY_ORIGIN_OUTSIDE:
            ok = ok & _origin_outside(bvh.leaves, bvh.types.leaf_kind, a, points[r])
        elif narrow != abi.NARROW_NONE and narrow != abi.NARROW_RAY_ORIGIN_OUTSIDE:
            raise ValueError(f"narrow {narrow} is not on the ray menu")
        passed = gen[ok]
        steps.append(Step(sort_pairs(gen if src is None else src), len(gen), len(passed)))
        if level == levels:
            break
        x, ray = passed[:, 0], passed[:, 1]
        v = _right_child_virtual(tree, level, x)
        src, gen, level = passed, _cat([_pairs(2 * x, ray), _pairs(2 * x[~v] + 1, ray[~v])]), level + 1
    pos = passed[:, 0] - (1 << (levels - 1)) + 1
    return Trace(steps, _pairs(bvh.leaves["index"].astype(np.int64)[pos - 1], passed[:, 1]), _pairs(pos, passed[:, 1]))


# ---------------------------------------------------------------------------------------------
# the device counters (the layout comment above level_kernel)
# ---------------------------------------------------------------------------------------------
def decode_counters(counters, total_levels):
    """counters: the buffer of ibvh_bfs_counters_bytes(total_levels) as bytes or uint64 words ->
    (flag, source[s], generated[s]): flag = 0 or 1 + the first step whose destination was too small; source[s] = entries
    in the source queue of step s (source[s + 1] = what step s produced, counted on past the capacity); generated[s] =
    pairs step s generated and checked, summed over the GEN_SLOTS words."""
    w = np.ascontiguousarray(np.asarray(counters)).view(np.uint64).astype(np.int64)
    chk = total_levels + 8  # the length of one block
    assert len(w) == chk * (1 + GEN_SLOTS), (len(w), chk)
    generated = w[chk:].reshape(GEN_SLOTS, chk).sum(axis=0)
    return int(w[0]), w[1:chk].copy(), generated
