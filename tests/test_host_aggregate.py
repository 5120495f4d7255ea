"""The bottom-up merge on the host side: ibvh_aggregate's refusals (each returns before any HIP call), the checker of
tests/aggregate_checker.py against itself (the oracle at every built_level is a slice of its built_level = 1 run; the flat
min / max reduction accepts the oracle's BBox nodes and rejects two swapped neighbours), and the table of launches against
the constants as they stand in csrc/ibvh_aggregate.hip.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aggregate_checker as chk
import mixed_pair_checker as mpc
import oracle_lib as orc
from implicitbvh_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = mpc.LEAF_NODE_COMBOS
NODE_BYTES = (16, 24, 32, 48)  # BSphere{F32}, BBox{F32}, BSphere{F64}, BBox{F64}
F, M, TL, TG = chk.FIRST, chk.MIDDLE, chk.TOP_LDS, chk.TOP_GLOBAL


# ---------------------------------------------------------------------------------------------
# 1. what ibvh_aggregate refuses
# ---------------------------------------------------------------------------------------------
def _aggregate(types, tree, built_level, leaves, nodes):
    """ibvh_aggregate with host addresses: only for calls that return before anything is launched"""
    return lib.load().ibvh_aggregate(None if types is None else C.byref(types), None if tree is None else C.byref(tree), built_level,
                                     leaves, nodes, None)


def test_aggregate_refuses_bad_arguments_before_any_launch():
    types = abi.make_types()
    tree = orc.tree_shape(1000)
    dummy = np.zeros(64, np.uint8)  # never read: every call below returns first
    p = dummy.ctypes.data
    assert _aggregate(None, tree, 1, p, p) == abi.ERR_INVALID_ARG
    assert _aggregate(types, None, 1, p, p) == abi.ERR_INVALID_ARG
    assert _aggregate(types, tree, 1, None, p) == abi.ERR_INVALID_ARG
    assert _aggregate(types, tree, 0, p, p) == abi.ERR_INVALID_ARG
    assert _aggregate(types, tree, -3, p, p) == abi.ERR_INVALID_ARG
    assert _aggregate(types, tree, tree.levels + 1, p, p) == abi.ERR_INVALID_ARG
    for n in (2, 3, 1000):
        t = orc.tree_shape(n)
        assert t.real_nodes >= 2
        for b in (1, t.levels):
            assert _aggregate(types, t, b, p, None) == abi.ERR_INVALID_ARG
    assert dummy.tobytes() == bytes(64)


def test_aggregate_refuses_types_the_library_does_not_instantiate():
    tree = orc.tree_shape(1000)
    dummy = np.zeros(64, np.uint8)
    p = dummy.ctypes.data
    for lf in (abi.F32, abi.F64):
        for nf in (abi.F32, abi.F64):
            boxes_under_spheres = abi.make_types(abi.BBOX, lf, abi.BSPHERE, nf)
            assert not abi.combo_supported(boxes_under_spheres)
            assert _aggregate(boxes_under_spheres, tree, 1, p, p) == abi.ERR_UNSUPPORTED
    for field, _ in abi.Types._fields_:
        for bad in (-1, 2 if field != "morton_type" else 3, 7):
            types = abi.make_types()
            setattr(types, field, bad)
            assert _aggregate(types, tree, 1, p, p) == abi.ERR_UNSUPPORTED, (field, bad)
    assert dummy.tobytes() == bytes(64)


@pytest.mark.parametrize("combo", COMBOS, ids=str)
def test_aggregate_of_one_leaf_needs_no_nodes(combo):
    tree = orc.tree_shape(1)
    assert tree.astuple()[:3] == (1, 1, 1)
    for idx in (abi.I32, abi.I64):
        types = abi.make_types(*combo, idx, abi.U32)
        leaves = chk.make_leaves(types, 1, 5)
        before = leaves.tobytes()
        assert _aggregate(types, tree, 1, leaves.ctypes.data, None) == abi.OK
        guard = np.full(64, 0xA5, np.uint8)
        assert _aggregate(types, tree, 1, leaves.ctypes.data, guard.ctypes.data) == abi.OK
        assert leaves.tobytes() == before and (guard == 0xA5).all()


# ---------------------------------------------------------------------------------------------
# 2. the checker against itself
# ---------------------------------------------------------------------------------------------
def _self_check(types, n, seed, small=True):
    """every built_level; small=False: the flat reduction without the case's memo at built_level 1 only (it is 0.4 s there)"""
    case = chk.Case(types, n, seed)
    L = case.levels
    assert case.levels == case.tree.levels
    total = len(case.oracle)
    assert total == case.tree.real_nodes - n == chk.num_nodes(n)
    for b in range(1, L + 1):
        lo = case.first_built_node(b)
        assert lo == (chk.level_offset(n, min(b, L - 1)) if L > 1 else 0)
        at_b = orc.aggregate(types, case.tree, b, case.leaves)
        assert not at_b[:lo].view(np.uint8).any(), (n, b)  # the oracle writes nothing above built_level
        got = case.check(at_b, b)
        levels = L - min(b, L - 1) if L > 1 else 0
        assert got.levels == levels and got.nodes == total - lo == sum(chk.real_on(n, l) for l in range(L - levels, L)), (n, b)
        if case.boxes:
            stated = [l for l in range(L - levels, L) if l <= L - 2 or types.leaf_kind == abi.BBOX]
            assert got.flat_levels == len(stated) and got.flat_nodes == sum(chk.real_on(n, l) for l in stated), (n, b)
            if small or b == 1:  # and without the case's memo: the reduction made from these nodes' own leaf parents
                assert chk.flat_check(types, n, case.leaves, at_b, b) == (got.flat_levels, got.flat_nodes)
        else:
            assert (got.flat_levels, got.flat_nodes) == (0, 0)
    return case


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["I32", "I64"])
@pytest.mark.parametrize("combo", COMBOS, ids=str)
def test_oracle_at_every_built_level_is_a_slice_of_built_level_1(combo, idx):
    morton = (abi.U16, abi.U32, abi.U64)[(COMBOS.index(combo) + idx) % 3]
    for n in chk.SMALL_SIZES:
        _self_check(abi.make_types(*combo, idx, morton), n, 1000 * COMBOS.index(combo) + n)


def test_oracle_slices_and_flat_reduction_at_the_smallest_global_top_size():
    n = 1_397_761
    case = _self_check(abi.make_types(abi.BBOX, abi.F64, abi.BBOX, abi.F64, abi.I64, abi.U64), n, 7, small=False)
    assert chk.real_on(n, case.levels - 9) == 2731 and case.node_bytes == 48


def _swapped(case, level):
    """the oracle's nodes with the first two nodes of `level` that differ swapped"""
    off, have = chk.level_offset(case.n, level), chk.real_on(case.n, level)
    rows = case.oracle[off:off + have]
    i = int(np.nonzero(rows[:-1] != rows[1:])[0][0])
    bad = case.oracle.copy()
    bad[[off + i, off + i + 1]] = bad[[off + i + 1, off + i]]
    return bad


@pytest.mark.parametrize("leaf", [(abi.BBOX, abi.F64), (abi.BSPHERE, abi.F32), (abi.BBOX, abi.F32)], ids=str)
def test_flat_reduction_rejects_two_swapped_neighbours(leaf):
    for nf in (abi.F32, abi.F64):
        types = abi.make_types(*leaf, abi.BBOX, nf)
        for n in (3, 5, 257, 513, 1000, 4097):
            case = chk.Case(types, n, n)
            L = case.levels
            assert chk.flat_check(types, n, case.leaves, case.oracle, 1) == (
                L - 1 if leaf[0] == abi.BBOX else L - 2, chk.num_nodes(n) - (0 if leaf[0] == abi.BBOX else chk.real_on(n, L - 1)))
            # every level with two nodes that the reduction states: L-1 only from BBox leaves
            for level in range(2, L if leaf[0] == abi.BBOX else L - 1):
                bad = _swapped(case, level)
                with pytest.raises(AssertionError, match="flat reduction, level"):
                    chk.flat_check(types, n, case.leaves, bad, 1)
                with pytest.raises(AssertionError, match="oracle, level %d" % level):
                    case.check(bad, 1)
                if level <= L - 2:  # a build that stops below the swap does not look at it
                    stated = chk.flat_levels_stated(types, n, level + 1)
                    assert chk.flat_check(types, n, case.leaves, bad, level + 1) == (len(stated), sum(chk.real_on(n, l) for l in stated))


def test_inputs_are_unsorted_and_take_the_containment_branches():
    for combo in COMBOS:
        types = abi.make_types(*combo, abi.I64, abi.U64)
        for n in (8, 1000, 4097):
            leaves = chk.make_leaves(types, n, 3)
            assert sorted(leaves["index"].tolist()) == list(range(1, n + 1))
            assert (np.diff(leaves["morton"].astype(np.float64)) < 0).sum() > n // 4  # far from any sorted order
            v = leaves["volume"]
            if combo[0] == abi.BBOX:
                assert v[0] == v[1]
                continue
            dist = lambda a, b: float(np.sqrt(((v["x"][a].astype(np.float64) - v["x"][b]) ** 2).sum()))  # noqa: E731
            assert dist(0, 1) + v["r"][1] < v["r"][0] and dist(2, 3) + v["r"][2] < v["r"][3] and v[4] == v[5]
            # one level up: leaves 6, 7 lie inside leaf 4 = leaf 5 with room to spare, and so does any sphere that bounds them tightly
            assert max(dist(4, 6), dist(4, 7)) + 3 * max(v["r"][6], v["r"][7]) < v["r"][4]


# ---------------------------------------------------------------------------------------------
# 3. the table of launches
# ---------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_source():
    src = open(os.path.join(ROOT, "implicitbvh.jl_amd", "csrc", "ibvh_aggregate.hip")).read()
    found = {}
    for name in chk.CONSTANTS:
        m = re.findall(r"\b%s\s*=\s*([0-9][0-9 *]*)[,;]" % name, src)
        assert len(m) == 1, name
        value = 1
        for factor in m[0].split("*"):
            value *= int(factor)
        found[name] = value
    assert found == chk.CONSTANTS == {"AGG_TPB": 256, "CH_LEVELS": 9, "AGG_TOP_TPB": 1024, "AGG_TOP_MAX": 4096,
                                      "AGG_TOP_LDS_BYTES": 131072}
    # the first launch folds 2 * AGG_TPB inputs down to one node, and a thread of the top kernel owns at most two nodes
    assert 2 * found["AGG_TPB"] == 1 << found["CH_LEVELS"] and found["AGG_TOP_MAX"] // 2 == 2 * found["AGG_TOP_TPB"]
    # the labels the launch profile reports are the kernels as IBVH_LAUNCH names them
    for name in chk.MERGE_KERNELS:
        assert any(chk.label(m) == name for m in re.findall(r"IBVH_LAUNCH\((\(.*?\)),", src)), name


def test_levels_and_real_nodes_are_the_trees():
    for n in list(chk.SMALL_SIZES) + list(chk.LARGE_SIZES) + [6, 7, 8, 9, 1 << 20]:
        tree = orc.tree_shape(n)
        assert chk.levels_of(n) == tree.levels
        for level in range(1, tree.levels):
            first, last = orc.level_indices(tree, level)  # (memory indices of the level's real nodes)
            assert (first - 1, last - first + 1) == (chk.level_offset(n, level), chk.real_on(n, level)), (n, level)
            assert chk.level_offset(n, level) == orc.memory_index(tree, 2 ** (level - 1)) - 1


def test_route_table():
    """The table of the sizes and what each pins, row by row."""
    L = chk.levels_of
    R = chk.real_on
    assert [L(n) for n in chk.SMALL_SIZES] == [1, 2, 3, 3, 4, 9, 9, 10, 10, 10, 11, 11, 11, 12, 14]
    assert [L(n) for n in chk.LARGE_SIZES] == [22, 22, 22, 22, 23]
    for nb in NODE_BYTES:
        assert chk.expected_launches(1, nb, 1) == []
        for n in (2, 3, 4, 5, 255, 256, 257, 511, 512):  # the first launch alone
            for b in range(1, L(n) + 1):
                assert chk.expected_launches(n, nb, b) == [F], (n, b)
        for n, have in ((513, 2), (514, 2), (1000, 2), (1025, 3), (4097, 9)):  # the LDS top over 2 .. 9 nodes
            assert R(n, L(n) - 9) == have
            for b in range(1, L(n) + 1):
                assert chk.expected_launches(n, nb, b) == ([F, TL] if b <= L(n) - 10 else [F]), (n, b)
    n = (1 << 20) + 1  # the first thread that owns a second node
    assert (R(n, 13), R(n, 12)) == (2049, 1025)
    n = 1_397_760  # the largest 48-byte level that fits LDS
    assert R(n, 13) == 2730 and 2730 * 48 <= chk.AGG_TOP_LDS_BYTES < 2731 * 48
    for n in ((1 << 20) + 1, 1_397_760):
        for nb in NODE_BYTES:
            for b in chk.large_built_levels(n):
                assert chk.expected_launches(n, nb, b) == ([F, TL] if b <= 12 else [F]), (n, nb, b)
            assert chk.second_node_levels(n, nb, 1) == [12] and chk.second_node_levels(n, nb, 13) == []
    n = 1_397_761  # the smallest global-memory top
    assert R(n, 13) == 2731
    for nb in NODE_BYTES:
        for b in chk.large_built_levels(n):
            assert chk.expected_launches(n, nb, b) == ([F, TG if nb == 48 else TL] if b <= 12 else [F]), (nb, b)
        assert chk.second_node_levels(n, nb, 1) == ([] if nb == 48 else [12])
    n = 1 << 21  # both top kernels at their maximum; BSphere{F64} at exactly 128 KiB
    assert R(n, 13) == 4096 == chk.AGG_TOP_MAX and 4096 * 32 == chk.AGG_TOP_LDS_BYTES and R(n, 12) == 2048 == 2 * chk.AGG_TOP_TPB
    for nb in NODE_BYTES:
        for b in chk.large_built_levels(n):
            assert chk.expected_launches(n, nb, b) == ([F, TG if nb == 48 else TL] if b <= 12 else [F]), (nb, b)
    n = (1 << 21) + 1  # the smallest middle-launch size
    assert L(n) == 23 and R(n, 14) == 4097 and R(n, 5) == 9
    assert chk.large_built_levels(n) == [1, 2, 4, 5, 6, 13, 14, 15, 22, 23]
    for nb in NODE_BYTES:
        for b in chk.large_built_levels(n):
            exp = [F, M, TL] if b <= 4 else [F, M] if b <= 13 else [F]
            assert chk.expected_launches(n, nb, b) == exp, (nb, b)
        assert chk.second_node_levels(n, nb, 1) == []
    for n in chk.LARGE_SIZES[:4]:
        assert chk.large_built_levels(n) == [1, 2, 12, 13, 14, 21, 22]
    # no launch follows the first when built_level >= L - 9
    for n in chk.SMALL_SIZES + chk.LARGE_SIZES:
        for nb in NODE_BYTES:
            for b in range(max(1, L(n) - 9), L(n) + 1):
                assert chk.expected_launches(n, nb, b) == ([F] if n > 1 else [])
