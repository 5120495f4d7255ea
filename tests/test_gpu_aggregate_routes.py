"""The bottom-up merge (aggregate<L, N>() in csrc/ibvh_aggregate.hip) on every launch route, node type and built level, called
directly through ibvh_aggregate and once each behind ibvh_refit and ibvh_build.

The route depends on the tree size, the node size and built_level alone (aggregate_checker.expected_launches; L = levels,
R(l) = real nodes on level l):
    n <= 512                          the first launch, aggregate_kernel<L, N, true>, makes every level
    513 <= n <= 2^21, R(L-9) <= 4096  then ONE workgroup folds the rest: aggregate_top_kernel<N, true> out of LDS, or
                                      aggregate_top_kernel<N, false> through memory when R(L-9) nodes exceed 128 KiB (48-byte
                                      BBox{Float64} nodes from 1,397,761 leaves on); above 2^20 leaves a thread of the LDS
                                      kernel owns a second node
    n >= 2^21 + 1                     aggregate_kernel<L, N, false> makes nine more levels in between
and built_level cuts it short: at L-10 the top kernel makes one level, from L-9 on nothing follows the first launch, which
stops early from L-8 on (L-19, L-18, L-17 behind the middle launch).

Leaf records are made on the host and are NOT in Morton order (aggregate_checker.make_leaves).  Each case asserts the status,
the nodes from the first built node on against the oracle byte for byte and (BBox nodes) against the flat min / max
reduction, that nothing else was written (a byte pattern in the nodes above built_level and in a 4 KiB guard behind the
node array; the leaf records), and the launches the library's launch profile reports."""
import ctypes as C

import numpy as np
import pytest

import aggregate_checker as chk
import mixed_pair_checker as mpc
import oracle_lib as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, lib  # noqa: E402
from test_gpu_lvt_blocks import _kernels_of  # noqa: E402
from test_gpu_parity import assert_bvh_equal  # noqa: E402
from test_gpu_refit import assert_refit, build, combo_id, cuda, first_built_node, snapshot  # noqa: E402

COMBOS = mpc.LEAF_NODE_COMBOS
MORTONS = (abi.U16, abi.U32, abi.U64)
GUARD = 4096
PATTERN = 0xA5
S32, S64, B64 = (abi.BSPHERE, abi.F32), (abi.BSPHERE, abi.F64), (abi.BBOX, abi.F64)
# (leaf, node) of the large sizes: every node type; BBox{F64} nodes under both leaf strides
LARGE_COMBOS = [S32 + (abi.BBOX, abi.F32), S32 + (abi.BBOX, abi.F64), B64 + (abi.BBOX, abi.F64), S32 + (abi.BSPHERE, abi.F32),
                S64 + (abi.BSPHERE, abi.F64)]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Device:
    """A case's leaf records on the device and a node buffer with a guard behind it."""

    def __init__(self, case):
        self.case = case
        lay = orc.layout_of(case.types)  # the buffers are exactly what the library will address
        assert (lay.leaf_bytes, lay.node_bytes) == (case.leaves.dtype.itemsize, case.node_bytes)
        assert case.tree.real_leaves == len(case.leaves) and case.tree.real_nodes - case.tree.real_leaves == len(case.oracle)
        self.leaves = cuda(raw(case.leaves).copy())  # (the case's own records are read-only)
        self.node_bytes = case.oracle.nbytes
        self.buf = torch.empty(self.node_bytes + GUARD, dtype=torch.uint8, device="cuda")

    def aggregate(self, built_level, null_nodes=False):
        """-> (status, launches, host copy of the node buffer with its guard)"""
        case = self.case
        self.buf.fill_(PATTERN)
        out = {}
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def go():
            out["status"] = lib.call("ibvh_aggregate", C.byref(case.types), C.byref(case.tree), built_level, self.leaves.data_ptr(),
                                     None if null_nodes else self.buf.data_ptr(), stream)

        names = [chk.label(s) for s in _kernels_of(go)]
        return out["status"], names, self.buf.cpu().numpy()


def run_case(dev, built_level, what):
    """One ibvh_aggregate call and everything a case asserts.  -> (launches, Compared)"""
    case = dev.case
    n, L = case.n, case.levels
    status, names, host = dev.aggregate(built_level)
    assert status == abi.OK, what
    assert names == chk.expected_launches(n, case.node_bytes, built_level), what
    assert names[:1] == ([chk.FIRST] if n > 1 else []) and (built_level < L - 9 or len(names) <= 1), what
    lo = case.first_built_node(built_level)
    assert lo == first_built_node(case.tree, built_level)
    got = case.check(host[:dev.node_bytes].view(case.oracle.dtype), built_level)
    # what was compared: every level from built_level (the leaf parents at the latest) down, all their nodes
    levels = L - min(built_level, L - 1) if L > 1 else 0
    assert got.levels == levels and sorted(got.per_level) == list(range(L - levels, L)), what
    assert got.nodes == len(case.oracle) - lo == sum(chk.real_on(n, l) for l in range(L - levels, L)), what
    if case.boxes:
        stated = [l for l in range(L - levels, L) if l <= L - 2 or case.types.leaf_kind == abi.BBOX]
        assert got.flat_levels == len(stated) and got.flat_nodes == sum(chk.real_on(n, l) for l in stated), what
    # what must not be written: the nodes above built_level, the guard behind the array, the leaf records
    assert (host[:lo * case.node_bytes] == PATTERN).all(), what
    assert len(host) == dev.node_bytes + GUARD and (host[dev.node_bytes:] == PATTERN).all(), what
    assert np.array_equal(dev.leaves.cpu().numpy(), raw(case.leaves)), what
    return names, got


# ---------------------------------------------------------------------------------------------
# 1. ibvh_aggregate: the small trees, every type and every built_level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["I32", "I64"])
@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_small_trees_on_every_built_level(combo, idx):
    """1 .. 4097 leaves: no nodes at all, the first launch alone (partial workgroups, lone right children), the smallest top
    launches over 2 .. 9 nodes."""
    morton = MORTONS[(COMBOS.index(combo) + idx) % 3]
    types = abi.make_types(*combo, idx, morton)
    routes = {}
    for n in chk.SMALL_SIZES:
        case = chk.Case(types, n, 100 * COMBOS.index(combo) + 7 * idx + n)
        dev = Device(case)
        for b in range(1, case.levels + 1):
            names, got = run_case(dev, b, (n, b))
            routes.setdefault(n, set()).add(tuple(names))
        if n == 1:  # no nodes: NULL is accepted, nothing is launched, and a buffer that is given stays untouched
            status, names, host = dev.aggregate(1, null_nodes=True)
            assert status == abi.OK and names == [] and (host == PATTERN).all() and len(case.oracle) == 0
    assert routes[1] == {()}
    for n in chk.SMALL_SIZES[1:]:
        assert routes[n] == ({(chk.FIRST,)} if n <= 512 else {(chk.FIRST,), (chk.FIRST, chk.TOP_LDS)}), n
    print("routes", combo_id(combo), {n: sorted(r) for n, r in routes.items() if n in (1, 2, 512, 513, 4097)})


# ---------------------------------------------------------------------------------------------
# 2. ibvh_aggregate: the sizes where the route changes above 2^20 leaves
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["I32", "I64"])
@pytest.mark.parametrize("combo", LARGE_COMBOS, ids=combo_id)
@pytest.mark.parametrize("n", chk.LARGE_SIZES)
def test_large_trees_on_the_route_of_their_size(n, combo, idx):
    types = abi.make_types(*combo, idx, MORTONS[(LARGE_COMBOS.index(combo) + idx) % 3])
    case = chk.Case(types, n, n % 1000 + 13 * LARGE_COMBOS.index(combo) + idx)
    assert case.leaves.nbytes <= 134_217_792 and case.oracle.nbytes <= 101_000_000
    dev = Device(case)
    L, nb = case.levels, case.node_bytes
    seen = {}
    for b in chk.large_built_levels(n):
        names, got = run_case(dev, b, (n, combo_id(combo), b))
        seen[b] = names
        for level in chk.second_node_levels(n, nb, b):  # the k = 1 half of the LDS top kernel made nodes, and they were compared
            assert chk.TOP_LDS in names and got.per_level[level] > chk.AGG_TOP_TPB
    # the route of this row of the table, spelt out
    global_top = nb == 48 and n in (1_397_761, 1 << 21)
    top = chk.TOP_GLOBAL if global_top else chk.TOP_LDS
    if n == chk.MIDDLE_SIZE:
        assert L == 23 and chk.real_on(n, 14) == 4097 and chk.real_on(n, 5) == 9
        assert seen == {1: [chk.FIRST, chk.MIDDLE, chk.TOP_LDS], 2: [chk.FIRST, chk.MIDDLE, chk.TOP_LDS], 4: [chk.FIRST, chk.MIDDLE, chk.TOP_LDS],
                        5: [chk.FIRST, chk.MIDDLE], 6: [chk.FIRST, chk.MIDDLE], 13: [chk.FIRST, chk.MIDDLE], 14: [chk.FIRST],
                        15: [chk.FIRST], 22: [chk.FIRST], 23: [chk.FIRST]}
        second = []
    else:
        assert L == 22 and chk.real_on(n, 13) == {(1 << 20) + 1: 2049, 1_397_760: 2730, 1_397_761: 2731, 1 << 21: 4096}[n]
        assert seen == {1: [chk.FIRST, top], 2: [chk.FIRST, top], 12: [chk.FIRST, top], 13: [chk.FIRST], 14: [chk.FIRST],
                        21: [chk.FIRST], 22: [chk.FIRST]}
        second = [] if global_top else [12]
        assert chk.real_on(n, 12) == {(1 << 20) + 1: 1025, 1_397_760: 1365, 1_397_761: 1366, 1 << 21: 2048}[n]
        if n == 1 << 21 and nb == 32:
            assert chk.real_on(n, 13) * nb == chk.AGG_TOP_LDS_BYTES  # BSphere{F64}: the LDS request filled to the byte
    assert chk.second_node_levels(n, nb, 1) == second
    print("routes", n, combo_id(combo), "R(L-9)=%d" % chk.real_on(n, L - 9),
          {" + ".join(r): [b for b in sorted(seen) if seen[b] == list(r)] for r in sorted({tuple(s) for s in seen.values()}, key=len)},
          "global top: %d calls" % sum(chk.TOP_GLOBAL in s for s in seen.values()),
          "second node: %d calls" % sum(bool(chk.second_node_levels(n, nb, b)) for b in seen))


# ---------------------------------------------------------------------------------------------
# 3. the same routes behind ibvh_refit and ibvh_build
# ---------------------------------------------------------------------------------------------
def merge_launches(names):
    return [s for s in map(chk.label, names) if s in chk.MERGE_KERNELS]


@pytest.mark.parametrize("n, combo, top", [(1_397_761, S32 + (abi.BBOX, abi.F64), chk.TOP_GLOBAL), ((1 << 20) + 1, S32 + (abi.BSPHERE, abi.F32), chk.TOP_LDS)],
                         ids=["global-top", "second-node"])
def test_refit_gathers_into_the_same_routes(n, combo, top):
    """ibvh.refit(g, volumes): refit_kernel is the first launch, the top kernel of the size follows."""
    rng = np.random.default_rng(n % 977)
    types = abi.make_types(*combo)
    a = mpc.random_volumes(rng, n, types.leaf_kind, types.leaf_float, scale=100.0, size=2.0)
    g = build(a, types)
    snap = snapshot(g)
    b = a[rng.permutation(n)]  # a maximally incoherent tree: large, heavily overlapping nodes
    dev_b = cuda(b)
    names = _kernels_of(lambda: ibvh.refit(g, dev_b))
    assert merge_launches(names) == [chk.REFIT_FIRST, top]
    assert chk.expected_launches(n, abi.node_dtype(types).itemsize, 1) == [chk.FIRST, top]
    assert_refit(g, snap, b[snap[0]["index"].astype(np.int64) - 1], (n, "gathered"))


def test_build_reaches_the_global_top_kernel_behind_the_sort():
    n = 1_397_761
    types = abi.make_types(*B64, abi.BBOX, abi.F64)
    vols = mpc.random_volumes(np.random.default_rng(21), n, abi.BBOX, abi.F64, scale=100.0, size=0.6)
    holder = {}
    names = _kernels_of(lambda: holder.update(g=build(vols, types)))
    assert merge_launches(names) == [chk.FIRST, chk.TOP_GLOBAL]
    assert_bvh_equal(orc.build(vols, types), holder["g"])
