"""The checker of the bottom-up merge (aggregate<L, N>() in csrc/ibvh_aggregate.hip, behind ibvh_aggregate, ibvh_refit and
ibvh_build): inputs that are NOT in Morton order, two references that do not use the library, and the table of launches.

A plain module, not a conftest: tests/test_gpu_aggregate_routes.py and tests/test_host_aggregate.py import it.

Notation: L = tree.levels (1 for one leaf, else ceil(log2 n) + 1), R(l) = ceil(n / 2^(L - l)) real nodes on level l.  The node
array holds levels 1 .. L-1 one after the other, real nodes only, so level l starts at R(1) + ... + R(l-1).

1. The oracle: oracle_lib.aggregate(types, tree, 1, leaves) (aggregate_oibvh!, build.jl:366-523), once per case at built_level
   1.  A build at level b writes the nodes from first_built_node(tree, b) on; they must be those bytes.
2. A flat reduction for BBox nodes, in numpy.  min and max are exact and associative, so a node of level l <= L-2 is, bit for
   bit, the minimum / maximum over the 2^(L-1-l) nodes of level L-1 below it (np.minimum.reduceat / np.maximum.reduceat),
   and for BBox leaves level L-1 is the flat min / max of the leaf pairs cast to the node type.  No tree is walked: a wrong
   level start, a wrong real-node count or a lost lone child shows even where the oracle had the same mistake.  BSphere nodes
   have no such reference (the sphere merge is not associative); the oracle alone checks them.

Both checks return how many levels and nodes they compared; the tests assert those numbers, so nothing passes by comparing
nothing."""
import collections

import numpy as np

import mixed_pair_checker as mpc
import oracle_lib as orc
from implicitbvh_amd import abi

# csrc/ibvh_aggregate.hip as it stands (tests/test_host_aggregate.py reads the source and fails when one of them moves)
AGG_TPB, CH_LEVELS, AGG_TOP_TPB, AGG_TOP_MAX, AGG_TOP_LDS_BYTES = 256, 9, 1024, 4096, 128 * 1024
CONSTANTS = {"AGG_TPB": AGG_TPB, "CH_LEVELS": CH_LEVELS, "AGG_TOP_TPB": AGG_TOP_TPB, "AGG_TOP_MAX": AGG_TOP_MAX,
             "AGG_TOP_LDS_BYTES": AGG_TOP_LDS_BYTES}

# the launch profile's labels (the stringified kernel of IBVH_LAUNCH), blanks and the outer parentheses removed
FIRST = "aggregate_kernel<L,N,true>"
MIDDLE = "aggregate_kernel<L,N,false>"
TOP_LDS = "aggregate_top_kernel<N,true>"
TOP_GLOBAL = "aggregate_top_kernel<N,false>"
REFIT_FIRST = "refit_kernel<L,N,I>"
MERGE_KERNELS = (FIRST, MIDDLE, TOP_LDS, TOP_GLOBAL, REFIT_FIRST)

# the smallest n that reach each route (the route depends on n, the node size and built_level alone)
SMALL_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 514, 1000, 1025, 4097)
LARGE_SIZES = ((1 << 20) + 1, 1_397_760, 1_397_761, 1 << 21, (1 << 21) + 1)
MIDDLE_SIZE = (1 << 21) + 1


def label(name):
    """'(aggregate_kernel<L, N, true>)' -> 'aggregate_kernel<L,N,true>'"""
    return name.replace(" ", "").strip("()")


# ---------------------------------------------------------------------------------------------
# the shape of the tree, in integers
# ---------------------------------------------------------------------------------------------
def levels_of(n):
    return 1 if n == 1 else (n - 1).bit_length() + 1


def real_on(n, level):
    """R(level)"""
    s = levels_of(n) - level
    return (n + (1 << s) - 1) >> s


def level_offset(n, level):
    """0-based position in the node array of the first node of `level`"""
    return sum(real_on(n, j) for j in range(1, level))


def num_nodes(n):
    return level_offset(n, levels_of(n))


def first_built_node(tree, built_level):
    """0-based position in the node array of the first node a build writes (test_gpu_refit.first_built_node)."""
    return orc.memory_index(tree, 2 ** (min(built_level, tree.levels - 1) - 1)) - 1 if tree.levels > 1 else 0


def built_levels(n, built_level):
    """the levels a merge at built_level writes, leaf parents first (the last-level merge always runs, build.jl:369)"""
    L = levels_of(n)
    return list(range(L - 1, min(built_level, L - 1) - 1, -1)) if L > 1 else []


def large_built_levels(n):
    L = levels_of(n)
    out = {1, 2, L - 10, L - 9, L - 8, L - 1, L}
    if n == MIDDLE_SIZE:
        out |= {L - 19, L - 18, L - 17}
    return sorted(out)


# ---------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------
def expected_launches(n, node_bytes, built_level):
    """What aggregate<L, N>() launches for n leaves under nodes of node_bytes: the first launch makes levels L-1 .. L-9; while
    levels are left, one workgroup folds them all if at most AGG_TOP_MAX nodes are left (in LDS if they fit), else another
    launch makes nine more."""
    L = levels_of(n)
    if L == 1:
        return []
    names = [FIRST]
    in_level = L - CH_LEVELS
    while in_level - 1 >= built_level and in_level - 1 >= 1:
        have = real_on(n, in_level)
        if have <= AGG_TOP_MAX:
            names.append(TOP_LDS if have * node_bytes <= AGG_TOP_LDS_BYTES else TOP_GLOBAL)
            break
        names.append(MIDDLE)
        in_level -= CH_LEVELS
    return names


def second_node_levels(n, node_bytes, built_level):
    """The levels on which a thread of the LDS top kernel owns a second node (mine[1]): more than AGG_TOP_TPB nodes."""
    names = expected_launches(n, node_bytes, built_level)
    if TOP_LDS not in names:
        return []
    top_in = levels_of(n) - CH_LEVELS * (len(names) - 1)
    return [l for l in range(top_in - 1, max(built_level, 1) - 1, -1) if real_on(n, l) > AGG_TOP_TPB]


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _plant(vols, kind, base):
    """Leaf pairs that take the sphere merge's containment branches (merge.jl:6, :10, :62-67), from leaf `base` (even) on."""
    n = len(vols)
    if kind == abi.BBOX:
        if base + 1 < n:
            vols[base + 1] = vols[base]  # an identical pair
        return
    t = vols.dtype.type
    if base + 1 < n:  # the right sphere inside the left one
        vols[base + 1, :3] = vols[base, :3] + t(0.01)
        vols[base + 1, 3] = vols[base, 3] * t(0.5)
    if base + 3 < n:  # the left sphere inside the right one
        vols[base + 2, :3] = vols[base + 3, :3] - t(0.01)
        vols[base + 2, 3] = vols[base + 3, 3] * t(0.25)
    if base + 5 < n:  # an identical pair
        vols[base + 5] = vols[base + 4]
    if base + 7 < n:  # two small spheres inside that pair's: their parent lies inside its sibling (sphere nodes, one level up)
        for k, d in ((6, 0.001), (7, -0.001)):
            vols[base + k, :3] = vols[base + 4, :3] + t(d)
            vols[base + k, 3] = vols[base + 4, 3] * t(0.1)


def make_leaves(types, n, seed):
    """n leaf records of abi.leaf_dtype(types) in NO Morton order: random volumes that overlap heavily, .index a random
    permutation of 1..n, .morton arbitrary."""
    rng = np.random.default_rng(seed)
    vols = mpc.random_volumes(rng, n, types.leaf_kind, types.leaf_float, scale=10.0, size=0.45)
    _plant(vols, types.leaf_kind, 0)
    if n > 4096:
        _plant(vols, types.leaf_kind, 2 * int(rng.integers(1024, n // 2 - 8)))
    leaves = np.zeros(n, abi.leaf_dtype(types))
    leaves["volume"] = orc.as_volumes(vols, types.leaf_kind, types.leaf_float)
    leaves["index"] = rng.permutation(n) + 1
    leaves["morton"] = rng.integers(0, 1 << abi.MORTON_BITS[types.morton_type], n, dtype=np.uint64)
    return leaves


# ---------------------------------------------------------------------------------------------
# the flat reduction (BBox nodes)
# ---------------------------------------------------------------------------------------------
def _raw(a):
    """the bytes of a (contiguous) record array, one row per record"""
    return a.view(np.uint8).reshape(len(a), -1)


def _first_difference(got, exp, what):
    bad = np.nonzero((_raw(got) != _raw(exp)).any(axis=1))[0]
    return "%s: %d of %d nodes differ, first at %d: %r, expected %r" % (what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]])


def flat_nodes(types, n, leaves, nodes):
    """The node array the flat reduction states: level L-1 from the leaf pairs for BBox leaves (else that of `nodes`, which
    it has no statement about), every level above from level L-1 of `nodes` itself."""
    assert types.node_kind == abi.BBOX
    L = levels_of(n)
    out = np.zeros(num_nodes(n), abi.node_dtype(types))
    if L == 1:
        return out
    have = real_on(n, L - 1)
    off = level_offset(n, L - 1)
    lo, up = np.ascontiguousarray(nodes["lo"][off:off + have]), np.ascontiguousarray(nodes["up"][off:off + have])
    if types.leaf_kind == abi.BBOX:
        t = abi.FLOAT_DTYPES[types.node_float]
        pairs = np.arange(0, n, 2)
        out["lo"][off:] = np.minimum.reduceat(np.ascontiguousarray(leaves["volume"]["lo"]), pairs, axis=0).astype(t)
        out["up"][off:] = np.maximum.reduceat(np.ascontiguousarray(leaves["volume"]["up"]), pairs, axis=0).astype(t)
    else:
        out[off:] = nodes[off:]
    for level in range(L - 2, 0, -1):
        starts = np.arange(0, have, 1 << (L - 1 - level))
        assert len(starts) == real_on(n, level)
        o = level_offset(n, level)
        out["lo"][o:o + len(starts)] = np.minimum.reduceat(lo, starts, axis=0)
        out["up"][o:o + len(starts)] = np.maximum.reduceat(up, starts, axis=0)
    return out


def flat_check(types, n, leaves, nodes, built_level, stated=None):
    """`nodes` from built_level down pass the flat reduction, component for component in bits.  -> (levels, nodes) compared.
    stated: flat_nodes() of nodes whose level L-1 is known to be that of `nodes`, to be used again."""
    exp = flat_nodes(types, n, leaves, nodes) if stated is None else stated
    levels = count = 0
    for level in flat_levels_stated(types, n, built_level):
        off, have = level_offset(n, level), real_on(n, level)
        if not np.array_equal(_raw(nodes[off:off + have]), _raw(exp[off:off + have])):
            raise AssertionError(_first_difference(nodes[off:off + have], exp[off:off + have], "flat reduction, level %d" % level))
        levels += 1
        count += have
    return levels, count


def flat_levels_stated(types, n, built_level):
    """the levels flat_check compares for a merge at built_level"""
    L = levels_of(n)
    return [l for l in built_levels(n, built_level) if l <= L - 2 or types.leaf_kind == abi.BBOX]


# ---------------------------------------------------------------------------------------------
# one case: its inputs and both references, made once
# ---------------------------------------------------------------------------------------------
Compared = collections.namedtuple("Compared", "levels nodes flat_levels flat_nodes per_level")


class Case:
    """n leaves of `types`, the oracle's nodes at built_level 1, and (BBox nodes) the flat reduction's verdict on them."""

    def __init__(self, types, n, seed):
        assert abi.combo_supported(types)
        self.types, self.n, self.levels = types, n, levels_of(n)
        self.tree = orc.tree_shape(n)
        assert self.tree.levels == self.levels and self.tree.real_nodes - n == num_nodes(n)
        self.leaves = make_leaves(types, n, seed)
        self.leaves.setflags(write=False)
        self.oracle = orc.aggregate(types, self.tree, 1, self.leaves)
        self.oracle.setflags(write=False)
        self.node_bytes = self.oracle.dtype.itemsize
        self.boxes = types.node_kind == abi.BBOX
        self.flat = None
        if self.boxes:  # the two references agree on every level
            self.flat = flat_nodes(types, n, self.leaves, self.oracle)
            assert flat_check(types, n, self.leaves, self.oracle, 1, self.flat) == (len(flat_levels_stated(types, n, 1)), sum(
                real_on(n, l) for l in flat_levels_stated(types, n, 1)))

    def first_built_node(self, built_level):
        return first_built_node(self.tree, built_level)

    def check(self, nodes, built_level):
        """`nodes` (the whole node array of a merge at built_level, as the node dtype) hold the oracle's bytes from the first
        built node on and, for BBox nodes, pass the flat reduction there.  -> Compared"""
        nodes = nodes.view(self.oracle.dtype).reshape(-1)
        assert len(nodes) == len(self.oracle)
        per_level = {}
        for level in built_levels(self.n, built_level):
            off, have = level_offset(self.n, level), real_on(self.n, level)
            got, exp = nodes[off:off + have], self.oracle[off:off + have]
            if not np.array_equal(_raw(got), _raw(exp)):
                raise AssertionError(_first_difference(got, exp, "oracle, level %d (built_level %d, n %d)" % (level, built_level, self.n)))
            per_level[level] = have
        assert self.first_built_node(built_level) + sum(per_level.values()) == len(nodes)
        # level L-1 is the oracle's by now, so the flat reduction over it is the one the constructor has made
        fl = flat_check(self.types, self.n, self.leaves, nodes, built_level, self.flat) if self.boxes else (0, 0)
        return Compared(len(per_level), sum(per_level.values()), fl[0], fl[1], per_level)
