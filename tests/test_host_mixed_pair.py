"""IBVH_PAIR_MIXED_TYPES on the host: the numpy checker of the mixed-type pair walk (tests/mixed_pair_checker.py) is pinned
to the oracle on every same-type pair, its leaf test to the oracle's iscontact on mixed kinds, and the Julia extension is
checked statically for binding the flag; the oracle's own mixed walk (IBVH_PAIR_MIXED_TYPES in oracle_traverse_pair_lvt_*) is
pinned to the checker on all 144 ordered pairs of two types.  No GPU."""
import itertools
import re

import numpy as np
import pytest

import mixed_pair_checker as mpc
import oracle_lib as orc
import implicitbvh_amd as ibvh  # noqa: F401  (registers the package under its import name)
from implicitbvh_amd import abi


def _oracle_list(o1, o2, sl1, sl2, narrow):
    c = orc.traverse_pair_lvt(o1, o2, sl1, sl2, narrow)[0]
    return np.stack([c["a"].astype(np.int64), c["b"].astype(np.int64)], axis=1) if len(c) else np.zeros((0, 2), np.int64)


@pytest.mark.parametrize("combo", mpc.LEAF_NODE_COMBOS, ids=lambda c: "%s%d_%s%d" % ("SB"[c[0]], 32 << c[1], "SB"[c[2]], 32 << c[3]))
def test_checker_equals_the_oracle_on_same_type_pairs(combo):
    """All 12 leaf / node combinations, several sizes (either BVH driving), every start level pair of a few, built_level > 1,
    both narrow codes: the checker's list equals the pinned oracle's, order included."""
    lk, lf, nk, nf = combo
    rng = np.random.default_rng(1000 + 7 * lk + 3 * lf + 5 * nk + nf)
    for idx, (n1, n2) in zip((abi.I32, abi.I64, abi.I32, abi.I64), ((1, 50), (50, 1), (190, 22), (700, 555))):
        types = abi.make_types(lk, lf, nk, nf, idx, (abi.U16, abi.U32, abi.U64)[n1 % 3])
        a = mpc.random_volumes(rng, n1, lk, lf, scale=5.0, size=0.4)
        b = mpc.random_volumes(rng, n2, lk, lf, scale=5.0, size=0.4, origin=1.0)
        for bl in (1, 2):
            o1, o2 = orc.build(a, types, built_level=min(bl, orc.tree_shape(n1).levels)), orc.build(b, types, built_level=min(bl, orc.tree_shape(n2).levels))
            for sl1 in sorted({o1.built_level, o1.tree.levels}):
                for sl2 in sorted({o2.built_level, (o2.tree.levels + 1) // 2 if o2.tree.levels >= o2.built_level * 2 else o2.built_level, o2.tree.levels}):
                    for narrow in (abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT):
                        exp = _oracle_list(o1, o2, sl1, sl2, narrow)
                        got = mpc.traverse_pair_lvt(o1, o2, sl1, sl2, narrow)
                        assert got.shape == exp.shape and (got == exp).all(), (combo, n1, n2, bl, sl1, sl2, narrow)


def test_checker_positions_and_smaller_drives():
    """positions=True gives 1-based leaf positions of the same pairs; smaller_drives gives the same SET in another order."""
    rng = np.random.default_rng(5)
    types = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32)
    o1, o2 = orc.build(mpc.random_volumes(rng, 300, abi.BSPHERE, abi.F32, 4, 0.3), types), \
        orc.build(mpc.random_volumes(rng, 120, abi.BSPHERE, abi.F32, 4, 0.3), types)
    by_idx = mpc.traverse_pair_lvt(o1, o2)
    pos = mpc.traverse_pair_lvt(o1, o2, positions=True)
    assert (o1.leaves["index"][pos[:, 0] - 1] == by_idx[:, 0]).all() and (o2.leaves["index"][pos[:, 1] - 1] == by_idx[:, 1]).all()
    small = mpc.traverse_pair_lvt(o1, o2, smaller_drives=True)
    assert sorted(map(tuple, small.tolist())) == sorted(map(tuple, by_idx.tolist()))
    assert len(by_idx) > 50


def _edge_volumes(kind, flt):
    f = abi.FLOAT_DTYPES[flt]
    inf, nan = np.inf, np.nan
    if kind == abi.BSPHERE:
        vols = [(0, 0, 0, 1), (2, 0, 0, 1), (0, 0, 0, 0), (1, 1, 1, inf), (nan, 0, 0, 1), (0, 0, 0, nan), (3, 0, 0, 0.5),
                (1e30, 1e30, 1e30, 1e30), (0.1, 0.2, 0.3, 0.1)]
    else:
        vols = [(-1, -1, -1, 1, 1, 1), (1, -1, -1, 3, 1, 1), (2, 2, 2, 2, 2, 2), (-inf, -inf, -inf, inf, inf, inf),
                (nan, 0, 0, 1, 1, 1), (0, 0, 0, nan, 1, 1), (3.5, -0.5, -0.5, 4, 0.5, 0.5), (0.1, 0.2, 0.3, 0.2, 0.3, 0.4)]
    return [np.asarray(v, f) for v in vols]


@pytest.mark.parametrize("kinds", list(itertools.product((abi.BSPHERE, abi.BBOX), repeat=2)), ids=lambda k: "%s%s" % ("SB"[k[0]], "SB"[k[1]]))
def test_checker_leaf_test_equals_the_oracle(kinds):
    """The checker's iscontact on the raw mixed types equals oracle_lib.iscontact for every kind and float pairing: random
    volumes, touching faces, zero and infinite radii, NaN anywhere, values near the Float32 range's end."""
    ka, kb = kinds
    rng = np.random.default_rng(17 + 2 * ka + kb)
    for fa, fb in itertools.product((abi.F32, abi.F64), repeat=2):
        vas = _edge_volumes(ka, fa) + [v for v in mpc.random_volumes(rng, 40, ka, fa, scale=3.0, size=0.7)]
        vbs = _edge_volumes(kb, fb) + [v for v in mpc.random_volumes(rng, 40, kb, fb, scale=3.0, size=0.7)]
        hits = 0
        for va in vas:
            for vb in vbs:
                want = orc.iscontact(ka, fa, va, kb, fb, vb)
                assert mpc.iscontact(ka, fa, va, kb, fb, vb) == want, (ka, fa, va, kb, fb, vb)
                hits += want
        assert 0 < hits < len(vas) * len(vbs)


def test_checker_refuses_a_box_query_against_sphere_nodes():
    """BSphere(::BBox) does not exist: the checker raises for it, and which BVH drives decides (the one with more leaves)."""
    rng = np.random.default_rng(3)
    ts = abi.make_types(abi.BSPHERE, abi.F32, abi.BSPHERE, abi.F32)
    tb = abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32)
    spheres = orc.build(mpc.random_volumes(rng, 40, abi.BSPHERE, abi.F32, 3, 0.3), ts)
    boxes = orc.build(mpc.random_volumes(rng, 90, abi.BBOX, abi.F32, 3, 0.3), tb)
    with pytest.raises(mpc.Refused):
        mpc.traverse_pair_lvt(boxes, spheres)          # boxes drive (more leaves): BSphere(::BBox) needed
    with pytest.raises(mpc.Refused):
        mpc.traverse_pair_lvt(spheres, boxes)
    assert len(mpc.traverse_pair_lvt(spheres, boxes, smaller_drives=True)) > 0   # spheres drive: BBox(::BSphere) exists


def test_checker_mixed_pair_is_the_contact_set_of_converted_queries():
    """A cross-check that does not go through the walk: on a mixed pair with BBox nodes, the checker's SET equals the
    brute-force set of iscontact(query, leaf) (box nodes are nested, so the node tests only prune)."""
    rng = np.random.default_rng(11)
    ts = abi.make_types(abi.BSPHERE, abi.F64, abi.BBOX, abi.F32, abi.I64, abi.U64)
    tb = abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F64, abi.I64, abi.U16)
    va, vb = mpc.random_volumes(rng, 400, abi.BSPHERE, abi.F64, 4, 0.3), mpc.random_volumes(rng, 250, abi.BBOX, abi.F32, 4, 0.3)
    o1, o2 = orc.build(va, ts), orc.build(vb, tb)
    got = mpc.traverse_pair_lvt(o1, o2)
    brute = {(i + 1, j + 1) for i in range(len(va)) for j in range(len(vb))
             if mpc.iscontact(abi.BSPHERE, abi.F64, va[i], abi.BBOX, abi.F32, vb[j])}
    assert set(map(tuple, got.tolist())) == brute and len(got) == len(brute) and len(brute) > 20


def _julia_ext():
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(here, "implicitbvh.jl_amd", "julia", "ImplicitBVHlibibvhExt.jl")).read()


def test_julia_ext_binds_the_mixed_flag():
    """The Julia extension's LVT pair method sends mixed pairs to the library with IBVH_PAIR_MIXED_TYPES (0x400, the header's
    value), refuses the pairs the library refuses through the generic method, sizes lvt_two_pass's scratch from BOTH
    descriptors, and the BFS pair method still hands every mixed pair to the generic method."""
    src = _julia_ext()
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))),
                                        "include", "ibvh.h")).read()
    assert re.search(r"IBVH_PAIR_MIXED_TYPES = 0x400\b", hdr)
    assert abi.PAIR_MIXED_TYPES == 0x400
    assert re.search(r"^const IBVH_PAIR_MIXED_TYPES = Int32\(0x400\)", src, re.M)
    m = re.search(r"#define IBVH_ABI_VERSION (\d+)", hdr)
    assert int(m.group(1)) == abi.ABI_VERSION == int(re.search(r"^const IBVH_ABI_VERSION = Int32\((\d+)\)", src, re.M).group(1))
    lvt = re.search(r"function ImplicitBVH\.traverse\(\s*bvh1::RocBVH\{I\}, bvh2::RocBVH, alg::LVTTraversal;(.*?)\nend\n", src, re.S).group(1)
    assert "d1.types != d2.types && !mixed_ok(d1, d2" in lvt
    assert "IBVH_PAIR_MIXED_TYPES" in lvt
    assert re.search(r"types2=mixed \? d2\.types : nothing", lvt)
    for entry in ("c_traverse_pair_lvt_count", "c_traverse_pair_lvt_write", "c_traverse_pair_lvt_enqueue"):
        call = re.search(entry + r"\(d1, d2, start_level1, start_level2, (\w+),", lvt)
        assert call and call.group(1) == "pcode", entry
    two = re.search(r"function lvt_two_pass\(.*?\n(.*?)\nend\n", src, re.S)
    assert "types2=nothing" in two.group(0)
    assert re.search(r"c_lvt_scratch_bytes\(types2, n_items, slots, need2\)", two.group(1))
    assert "max(need[], need2[])" in two.group(1)
    ok = re.search(r"function mixed_ok\(d1, d2, n1, n2\)\n(.*?)\nend\n", src, re.S).group(1)
    assert "index_type" in ok and "kind(BBox)" in ok and "kind(BSphere)" in ok and "n1 >= n2" in ok
    bfs = re.search(r"function ImplicitBVH\.traverse\(\s*bvh1::RocBVH\{I\}, bvh2::RocBVH, alg::BFSTraversal;(.*?)\nend\n", src, re.S).group(1)
    assert "d1.types != d2.types\n" in bfs and "mixed_ok" not in bfs


# ---- the oracle's own mixed walk (IBVH_PAIR_MIXED_TYPES in oracle_traverse_pair_lvt_*), pinned to the checker ----------
MORTONS = (abi.U16, abi.U32, abi.U64)
_COMBO_ID = lambda c: "%s%d%s%d" % ("SB"[c[0]], 32 << c[1], "SB"[c[2]], 32 << c[3])  # noqa: E731


def _mixed_types(i, j):
    """Types of the ordered combo pair (i, j) of LEAF_NODE_COMBOS: two different Morton widths, one index type."""
    idx = (abi.I32, abi.I64)[(i + j) % 2]
    m1 = i % 3
    return (abi.make_types(*mpc.LEAF_NODE_COMBOS[i], idx, MORTONS[m1]),
            abi.make_types(*mpc.LEAF_NODE_COMBOS[j], idx, MORTONS[(m1 + 1 + j % 2) % 3]))


def _pair_status(o1, o2, narrow, sl1=None, sl2=None):
    """The raw status of oracle_traverse_pair_lvt_count."""
    import ctypes as C
    sl1 = max(1, o1.built_level) if sl1 is None else sl1
    sl2 = max(1, o2.built_level) if sl2 is None else sl2
    s1, s2 = o1.struct(), o2.struct()
    counts = np.zeros(max(o1.tree.real_leaves, o2.tree.real_leaves), abi.INDEX_DTYPES[o1.types.index_type])
    total = C.c_int64()
    return orc.lib.oracle_traverse_pair_lvt_count(C.byref(s1), C.byref(s2), C.c_int64(sl1), C.c_int64(sl2), narrow,
                                                  C.c_void_p(counts.ctypes.data), C.byref(total))


def _check_against_checker(o1, o2, sl1, sl2, narrow, smaller):
    """-> number of pairs compared, or None when the combination is refused (by both)."""
    flags = abi.PAIR_MIXED_TYPES | (abi.PAIR_SMALLER_DRIVES if smaller else 0)
    try:
        exp = mpc.traverse_pair_lvt(o1, o2, sl1, sl2, narrow, smaller_drives=smaller)
    except mpc.Refused:
        assert _pair_status(o1, o2, narrow | flags, sl1, sl2) == abi.ERR_UNSUPPORTED
        return None
    got = _oracle_list(o1, o2, sl1, sl2, narrow | flags)
    assert got.shape == exp.shape and (got == exp).all(), (sl1, sl2, narrow, smaller)
    return len(exp)


@pytest.mark.parametrize("pair", list(itertools.product(range(len(mpc.LEAF_NODE_COMBOS)), repeat=2)),
                         ids=lambda p: _COMBO_ID(mpc.LEAF_NODE_COMBOS[p[0]]) + "_" + _COMBO_ID(mpc.LEAF_NODE_COMBOS[p[1]]))
def test_oracle_mixed_list_equals_the_checker(pair):
    """All 144 ordered pairs of leaf / node combinations, two Morton widths, either index type: sizes 1 and larger with
    either BVH driving, built_level 1 and 2, every start level of the walked tree, every pair narrow code, with and without
    IBVH_PAIR_SMALLER_DRIVES: the oracle's mixed list equals the checker's, order included; refused exactly where the
    checker has no NodeType(query)."""
    i, j = pair
    t1, t2 = _mixed_types(i, j)
    c1, c2 = mpc.LEAF_NODE_COMBOS[i], mpc.LEAF_NODE_COMBOS[j]
    rng = np.random.default_rng(7919 + 12 * i + j)
    compared = refused = 0
    for n1, n2 in ((1, 37), (37, 1), (150, 61), (61, 150)):
        a = mpc.random_volumes(rng, n1, c1[0], c1[1], scale=4.0, size=0.5)
        b = mpc.random_volumes(rng, n2, c2[0], c2[1], scale=4.0, size=0.5, origin=0.5)
        for bl in (1, 2):
            o1 = orc.build(a, t1, built_level=min(bl, orc.tree_shape(n1).levels))
            o2 = orc.build(b, t2, built_level=min(bl, orc.tree_shape(n2).levels))
            b1, b2 = o1.built_level, o2.built_level
            for narrow in (abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT):
                for smaller in (False, True):
                    r = _check_against_checker(o1, o2, b1, b2, narrow, smaller)
                    refused += r is None
                    compared += r or 0
            # every start level of either tree (only the walked tree's matters), narrow code and driver rotating
            sls = [(b1, s) for s in range(b2, o2.tree.levels + 1)] + [(s, b2) for s in range(b1 + 1, o1.tree.levels + 1)]
            for k, (sl1, sl2) in enumerate(sls):
                r = _check_against_checker(o1, o2, sl1, sl2, k % 3, (k // 3) % 2 == 1)
                refused += r is None
                compared += r or 0
    box_vs_spheres = (c1[0] == abi.BBOX and c2[2] == abi.BSPHERE) or (c2[0] == abi.BBOX and c1[2] == abi.BSPHERE)
    assert (refused > 0) == box_vs_spheres
    assert compared > 100


@pytest.mark.parametrize("idx", (abi.I32, abi.I64), ids=("i32", "i64"))
def test_oracle_mixed_list_with_nan_and_infinite_volumes(idx):
    """NaN and infinite radii and box bounds are data: on every ordered pair of combinations the oracle's mixed list equals
    the checker's."""
    rng = np.random.default_rng(23 + idx)
    for i, j in itertools.product(range(len(mpc.LEAF_NODE_COMBOS)), repeat=2):
        (lk1, lf1, nk1, nf1), (lk2, lf2, nk2, nf2) = mpc.LEAF_NODE_COMBOS[i], mpc.LEAF_NODE_COMBOS[j]
        t1 = abi.make_types(lk1, lf1, nk1, nf1, idx, MORTONS[i % 3])
        t2 = abi.make_types(lk2, lf2, nk2, nf2, idx, MORTONS[(i + 1) % 3])
        a = mpc.random_volumes(rng, 90, lk1, lf1, scale=3.0, size=0.5)
        b = mpc.random_volumes(rng, 70, lk2, lf2, scale=3.0, size=0.5)
        for v, k in ((a, lk1), (b, lk2)):
            rows = rng.choice(len(v), 12, replace=False)
            col = 3 if k == abi.BSPHERE else rng.integers(0, 6, 12)
            v[rows[:4], col if np.isscalar(col) else col[:4]] = np.inf
            v[rows[4:8], col if np.isscalar(col) else col[4:8]] = np.nan
            v[rows[8:], col if np.isscalar(col) else col[8:]] = -np.inf
        o1, o2 = orc.build(a, t1), orc.build(b, t2)
        for narrow in (abi.NARROW_NONE, abi.NARROW_MORTON_LT):
            for smaller in (False, True):
                _check_against_checker(o1, o2, o1.built_level, o2.built_level, narrow, smaller)


def test_oracle_refuses_what_the_library_refuses():
    """Two index types (with or without the flag), two types without the flag, and a BBox query against BSphere nodes
    (which BVH drives decides, IBVH_PAIR_SMALLER_DRIVES included): IBVH_ERR_UNSUPPORTED."""
    rng = np.random.default_rng(29)
    ts = abi.make_types(abi.BSPHERE, abi.F32, abi.BSPHERE, abi.F32, abi.I32, abi.U32)
    tb = abi.make_types(abi.BBOX, abi.F64, abi.BBOX, abi.F64, abi.I32, abi.U64)
    tb64 = abi.make_types(abi.BBOX, abi.F64, abi.BBOX, abi.F64, abi.I64, abi.U64)
    spheres = orc.build(mpc.random_volumes(rng, 40, abi.BSPHERE, abi.F32, 3, 0.3), ts)
    boxes = orc.build(mpc.random_volumes(rng, 90, abi.BBOX, abi.F64, 3, 0.3), tb)
    boxes64 = orc.build(mpc.random_volumes(rng, 20, abi.BBOX, abi.F64, 3, 0.3), tb64)
    M, S = abi.PAIR_MIXED_TYPES, abi.PAIR_SMALLER_DRIVES
    U = abi.ERR_UNSUPPORTED
    assert _pair_status(spheres, boxes, 0) == U and _pair_status(boxes, spheres, abi.NARROW_INDEX_LT) == U
    assert _pair_status(spheres, boxes64, M) == U and _pair_status(boxes64, spheres, M | S) == U
    assert _pair_status(boxes, spheres, M) == U and _pair_status(spheres, boxes, M) == U  # boxes drive
    assert _pair_status(spheres, boxes, M | S) == abi.OK and _pair_status(boxes, spheres, M | S) == abi.OK  # spheres drive
    assert _pair_status(boxes64, spheres, M) == U  # (index types differ)
    few = orc.build(mpc.random_volumes(rng, 10, abi.BBOX, abi.F64, 3, 0.3), tb)
    assert _pair_status(spheres, few, M) == abi.OK and _pair_status(spheres, few, M | S) == U  # now the spheres have more


@pytest.mark.parametrize("combo", mpc.LEAF_NODE_COMBOS, ids=_COMBO_ID)
def test_oracle_mixed_flag_changes_nothing_on_same_type_pairs(combo):
    """One type on both sides: the flag set gives the same contacts and the same counts, byte for byte, as the flag unset
    (every narrow code, either driver, IBVH_PAIR_SMALLER_DRIVES, both index types)."""
    rng = np.random.default_rng(31 + sum(combo))
    for idx, (n1, n2) in ((abi.I32, (120, 47)), (abi.I64, (33, 200)), (abi.I32, (1, 9))):
        t = abi.make_types(*combo, idx, MORTONS[n1 % 3])
        o1 = orc.build(mpc.random_volumes(rng, n1, combo[0], combo[1], 4, 0.5), t)
        o2 = orc.build(mpc.random_volumes(rng, n2, combo[0], combo[1], 4, 0.5, origin=0.5), t)
        for narrow in (abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT):
            for extra in (0, abi.PAIR_SMALLER_DRIVES):
                c0, k0 = orc.traverse_pair_lvt(o1, o2, narrow=narrow | extra)
                c1, k1 = orc.traverse_pair_lvt(o1, o2, narrow=narrow | extra | abi.PAIR_MIXED_TYPES)
                assert c0.tobytes() == c1.tobytes() and k0.tobytes() == k1.tobytes(), (idx, n1, n2, narrow, extra)
                exp = mpc.traverse_pair_lvt(o1, o2, narrow=narrow, smaller_drives=bool(extra))
                assert (_oracle_list(o1, o2, None, None, narrow | extra) == exp).all()
