"""The breadth-first traversal's host side, no GPU:
  * tests/bfs_levels_checker.py (the numpy restatement of the level-synchronous walk that tests/test_gpu_bfs_routes.py
    compares the level kernel's per-step counters and queues with) pinned to the oracle's BFS: same contact set, the sum
    of its per-step generated counts = the oracle's num_checks, as many steps as the library's plan;
  * the status the three BFS entry points, the three *_initial_capacity calls and ibvh_bfs_counters_bytes return for a bad
    argument, one at a time against an otherwise well-formed call — every case returns before the library makes a HIP
    call, so the buffers are host memory it never touches;
  * the level kernel's geometry constants, read from csrc/ibvh_bfs.hip, against the ones the route tests' preconditions
    are worked out from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bfs_levels_checker as chk
import mixed_pair_checker as mpc
import oracle_lib as orc
from dist_cross_checker import ALL_COMBOS, combo_name
from implicitbvh_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_COMBOS = [c for c in ALL_COMBOS if c[1] == c[3]]  # rays need one float type (ibvh_traverse_rays_bfs)
SIZES = (1, 2, 3, 5, 12, 100, 1001)
PAIR_NARROWS = (abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT)


def _sorted(p):
    return chk.sort_pairs(p)


def _oracle(c):
    return _sorted(np.stack([c["a"], c["b"]], axis=1)) if len(c) else np.zeros((0, 2), np.int64)


def _positions(leaves):
    idx = leaves["index"].astype(np.int64)
    pos = np.zeros(idx.max() + 1, np.int64)
    pos[idx] = np.arange(1, len(idx) + 1)
    return pos


def _start_levels(levels, n):
    return range(1, levels + 1) if n < 1001 else sorted({1, levels // 2, levels})


def _build(rng, n, combo, **kw):
    return orc.build(mpc.random_volumes(rng, n, combo[0], combo[1], **kw), abi.make_types(*combo))


# ---------------------------------------------------------------------------------------------
# the checker against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ALL_COMBOS, ids=combo_name)
def test_checker_self_is_the_oracles_bfs(combo):
    rng = np.random.default_rng(500 + ALL_COMBOS.index(combo))
    for n in SIZES:
        o = _build(rng, n, combo)
        tables, levels = {}, o.tree.levels
        for sl in _start_levels(levels, n):
            t = chk.trace_self(o, sl, tables=tables)
            exp, res = orc.traverse_bfs(o, sl)
            assert (_sorted(t.contacts) == _oracle(exp)).all() and t.num_contacts == res.num_contacts, (n, sl)
            assert t.num_checks == res.num_checks, (n, sl)
            assert len(t.steps) == 1 + levels - sl, (n, sl)
            assert [s.passed for s in t.steps[:-1]] == [len(s.source) for s in t.steps[1:]]
        sl = max(levels // 2, 1)
        pos = _positions(o.leaves)
        for narrow in PAIR_NARROWS:
            t = chk.trace_self(o, sl, narrow, tables=tables)
            exp, res = orc.traverse_bfs(o, sl, narrow)
            assert (_sorted(t.contacts) == _oracle(exp)).all() and t.num_checks == res.num_checks, (n, narrow)
            # positions: the left leaf first; the same contacts, named by where the leaves lie
            assert (t.positions[:, 0] < t.positions[:, 1]).all()
            e = _oracle(exp)
            pe = np.stack([pos[e[:, 0]], pos[e[:, 1]]], axis=1) if len(e) else e
            assert (_sorted(np.sort(pe, axis=1)) == _sorted(t.positions)).all(), (n, narrow)


def _pair_start_levels(l1, l2, n):
    if n < 100:
        return [(a, b) for a in range(1, l1 + 1) for b in range(1, l2 + 1)]
    if n == 100:
        return [(a, b) for a in range(1, l1 + 1) for b in sorted({1, l2 // 2, l2 - 1, l2})]
    return [(1, 1), (l1 // 2, l2 // 2), (l1, l2)]


@pytest.mark.parametrize("combo", ALL_COMBOS, ids=combo_name)
def test_checker_pair_is_the_oracles_bfs(combo):
    rng = np.random.default_rng(600 + ALL_COMBOS.index(combo))
    # (n1, n2): equal sizes, then levels1 != levels2 in both directions (a one-leaf tree, a ragged one, a full one)
    shapes = [(n, n) for n in SIZES] + [(1, 50), (50, 1), (3, 200), (200, 3), (64, 9), (9, 64), (22, 190), (190, 22)]
    for n1, n2 in shapes:
        o1, o2 = _build(rng, n1, combo), _build(rng, n2, combo, origin=0.5)
        tables, l1, l2 = {}, o1.tree.levels, o2.tree.levels
        for sl1, sl2 in _pair_start_levels(l1, l2, max(n1, n2)):
            t = chk.trace_pair(o1, o2, sl1, sl2, tables=tables)
            exp, res = orc.traverse_pair_bfs(o1, o2, sl1, sl2)
            assert (_sorted(t.contacts) == _oracle(exp)).all() and t.num_contacts == res.num_contacts, (n1, n2, sl1, sl2)
            assert t.num_checks == res.num_checks, (n1, n2, sl1, sl2)
            plan = chk.pair_plan(l1, l2, sl1, sl2)
            # the plan: one or both sides go down one level per step, from the start levels to the two leaf levels
            assert len(t.steps) == len(plan) and plan[0][:2] == (sl1, sl2) and plan[-1][:2] == (l1, l2)
            for (a1, a2, d1, d2), (b1, b2, _, _) in zip(plan[:-1], plan[1:]):
                assert (d1 or d2) and (b1, b2) == (a1 + d1, a2 + d2)
        sl1, sl2 = max(l1 // 2, 1), max(l2 // 2, 1)
        p1, p2 = _positions(o1.leaves), _positions(o2.leaves)
        for narrow in PAIR_NARROWS:
            t = chk.trace_pair(o1, o2, sl1, sl2, narrow, tables=tables)
            exp, res = orc.traverse_pair_bfs(o1, o2, sl1, sl2, narrow)
            e = _oracle(exp)
            assert (_sorted(t.contacts) == e).all() and t.num_checks == res.num_checks, (n1, n2, narrow)
            pe = np.stack([p1[e[:, 0]], p2[e[:, 1]]], axis=1) if len(e) else e
            assert (_sorted(pe) == _sorted(t.positions)).all(), (n1, n2, narrow)


def irregular_rays(rng, nr, extent, flt):
    """the rays of tests/test_gpu_rays_binned.py: zero, infinite, denormal and NaN components among ordinary ones"""
    p = (rng.random((nr, 3)) * (extent + 3) - 1).astype(np.float32)
    d = (rng.random((nr, 3)) - 0.5).astype(np.float32)
    d[::5, rng.integers(0, 3)] = 0
    d[7::41] = 0
    d[3::53, 1] = np.inf
    d[11::67, 2] = 1e-45
    p[13::71, 0] = np.nan
    p[17::73, 1] = np.inf
    d[19::79] *= 1e30
    f = abi.FLOAT_DTYPES[flt]
    return np.ascontiguousarray(p.astype(f)), np.ascontiguousarray(d.astype(f))


@pytest.mark.parametrize("combo", RAY_COMBOS, ids=combo_name)
def test_checker_rays_is_the_oracles_bfs(combo):
    rng = np.random.default_rng(700 + ALL_COMBOS.index(combo))
    for n in SIZES:
        o = _build(rng, n, combo)
        levels = o.tree.levels
        with np.errstate(all="ignore"):
            p, d = irregular_rays(rng, 150, 6, combo[1])
        p[::3] = mpc.random_volumes(rng, len(p[::3]), abi.BSPHERE, combo[1])[:, :3]  # some origins inside leaves
        tables = {}
        for sl in _start_levels(levels, n):
            t = chk.trace_rays(o, p, d, sl, tables=tables)
            exp, res = orc.traverse_rays_bfs(o, p, d, sl)
            assert (_sorted(t.contacts) == _oracle(exp)).all() and t.num_contacts == res.num_contacts, (n, sl)
            assert t.num_checks == res.num_checks, (n, sl)
            assert len(t.steps) == 1 + levels - sl, (n, sl)
        # the ray narrow is a filter on the hit list (raytrace_gpu.jl:159); positions name the same leaves
        t = chk.trace_rays(o, p, d, 1, tables=tables)
        tn = chk.trace_rays(o, p, d, 1, abi.NARROW_RAY_ORIGIN_OUTSIDE, tables=tables)
        assert [s.generated for s in tn.steps] == [s.generated for s in t.steps]
        vol = o.leaves["volume"]
        keep = []
        for pos, ray in t.positions.tolist():  # one hit at a time, in Python floats of the leaf type
            v, q = vol[pos - 1], p[ray - 1]
            if combo[0] == abi.BSPHERE:
                dd = q - v["x"]
                keep.append(bool(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] > v["r"] * v["r"]))
            else:
                keep.append(bool(((q < v["lo"]) | (q > v["up"])).any()))
        keep = np.asarray(keep, bool)
        assert (tn.positions == t.positions[keep]).all() and (tn.contacts == t.contacts[keep]).all()
        assert n < 100 or 0 < keep.sum() < len(keep)
        assert (_positions(o.leaves)[t.contacts[:, 0]] == t.positions[:, 0]).all()


def test_decode_counters_restates_the_layout():
    """flag, then the source count of every step, then GEN_SLOTS blocks of per-step check counts (the comment above
    level_kernel): a buffer written by that rule decodes to what was written."""
    total_levels = 11
    need = C.c_size_t()
    lib.call("ibvh_bfs_counters_bytes", total_levels, C.byref(need))
    chk_len = total_levels + 8
    w = np.zeros(need.value // 8, np.uint64)
    assert len(w) == chk_len * (1 + chk.GEN_SLOTS)
    w[0] = 4
    for s in range(6):
        w[1 + s] = 100 + s
        for k in range(chk.GEN_SLOTS):
            w[chk_len * (1 + k) + s] = (k + 1) * (s + 1)
    flag, source, generated = chk.decode_counters(w.view(np.uint8), total_levels)
    assert flag == 4 and source[:6].tolist() == [100, 101, 102, 103, 104, 105] and not source[6:].any()
    assert generated[:6].tolist() == [136 * (s + 1) for s in range(6)] and not generated[6:].any()


# ---------------------------------------------------------------------------------------------
# the level kernel's geometry
# ---------------------------------------------------------------------------------------------
def test_kernel_constants_are_the_ones_the_route_tests_assume():
    """tests/test_gpu_bfs_routes.py proves from the checker's trace that its inputs put several chunks and several flushes
    on one workgroup; that proof uses these numbers.  A change of the kernel's geometry must change them too."""
    src = open(os.path.join(ROOT, "implicitbvh.jl_amd", "csrc", "ibvh_bfs.hip")).read()
    assert int(re.search(r"constexpr int TPB = (\d+);", src).group(1)) == chk.TPB
    assert int(re.search(r"constexpr int GEN_SLOTS = (\d+);", src).group(1)) == chk.GEN_SLOTS
    m = re.search(r"constexpr int STAGE = \(sizeof\(I\) == 4 \? (\d+) : (\d+)\) \* 1024 / \(int\)sizeof\(IndexPair<I>\);", src)
    assert m, "the STAGE expression changed"
    assert int(m.group(1)) * 1024 // 8 == chk.STAGE and int(m.group(2)) * 1024 // 16 == chk.STAGE  # Int32 / Int64 pairs
    maxout = dict(re.findall(r"struct (\w+) \{[^{}]*?static constexpr int MAXOUT = (\d+);", src))
    assert {k: int(v) for k, v in maxout.items()} == {"Identity": chk.MAXOUT["initial"], "SelfStep": chk.MAXOUT["self"],
                                                      "PairStep": chk.MAXOUT["pair"], "RayStep": chk.MAXOUT["rays"]}
    assert "constexpr int MAXOUT = PolA::MAXOUT;" in src and "if (s_fill > STAGE - MAXOUT * TPB) flush();" in src
    assert "for (int64_t chunk = blockIdx.x; chunk * TPB < num_src; chunk += stride)" in src
    assert [chk.flush_threshold(k) for k in ("self", "pair", "rays", "initial")] == [2048, 2048, 2560, 2816]


# ---------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------
OK, INVALID, UNSUPPORTED, CAPACITY, OVERFLOW = abi.OK, abi.ERR_INVALID_ARG, abi.ERR_UNSUPPORTED, abi.ERR_CAPACITY, abi.ERR_OVERFLOW

PARAMS = {  # the parameters of each entry point, in order (include/ibvh.h)
    "bfs": "bvh sl narrow bvtt1 bvtt2 capacity counters result stream",
    "pair_bfs": "bvh1 bvh2 sl1 sl2 narrow bvtt1 bvtt2 capacity counters result stream",
    "rays_bfs": "bvh points dirs num_rays sl narrow bvtt1 bvtt2 capacity counters result stream",
}
ALL = tuple(PARAMS)
N1, N2, NR = 100, 60, 50  # leaves of bvh / bvh1, of bvh2; rays
BIG = 1 << 40             # a capacity no initial queue exceeds (never reached: every case fails a check first)
_buf = C.create_string_buffer(4096)  # stands in for every device buffer: never read or written by a call that fails its checks
BUF = C.cast(_buf, C.c_void_p)


def _bvh(n, types=None, built_level=1, levels=None):
    tree = abi.Tree()
    lib.call("ibvh_tree_shape", n, C.byref(tree))
    if levels is not None:
        tree.levels = levels  # (no tree_shape gives more than 61 levels)
    return abi.Bvh(types if types is not None else abi.make_types(), tree, built_level, BUF, BUF, BUF)


def _result(resume_step=0, resume_num=0):
    return abi.BfsResult(-1, -1, -1, -1, resume_step, resume_num)


def _call(entry, **bad):
    """entry(good arguments, with `bad` replacing some of them) -> (status, result)"""
    res = bad.pop("res", None) or _result()
    good = dict(bvh=_bvh(N1), bvh1=_bvh(N1), bvh2=_bvh(N2), sl=1, sl1=1, sl2=1, narrow=abi.NARROW_NONE, bvtt1=BUF, bvtt2=BUF,
                capacity=BIG, counters=BUF, result=C.byref(res), stream=None, points=BUF, dirs=BUF, num_rays=NR)
    good.update(bad)
    args = [good[p] for p in PARAMS[entry].split()]
    args = [C.byref(a) if isinstance(a, abi.Bvh) else a for a in args]
    return getattr(lib.load(), "ibvh_traverse_" + entry)(*args), res


def _first_bvh(entry, b):
    return {"bvh1" if entry == "pair_bfs" else "bvh": b}


def _first_sl(entry, sl):
    return {"sl1" if entry == "pair_bfs" else "sl": sl}


I64 = abi.make_types(index_type=abi.I64)
MIXED_FLOAT = abi.make_types(leaf_float=abi.F64)  # BSphere{Float64} leaves, BBox{Float32} nodes
LEVELS1 = _bvh(N1).tree.levels
LEVELS2 = _bvh(N2).tree.levels

CASES = [
    # ---- every entry point --------------------------------------------------------------------------------------------
    *[(e, _first_bvh(e, None), INVALID, "NULL bvh") for e in ALL],
    *[(e, dict(result=None), INVALID, "NULL result") for e in ALL],
    *[(e, dict(bvtt1=None), INVALID, "NULL bvtt1") for e in ALL],
    *[(e, dict(bvtt2=None), INVALID, "NULL bvtt2") for e in ALL],
    *[(e, dict(counters=None), INVALID, "NULL counters") for e in ALL],
    *[(e, dict(capacity=0), INVALID, "capacity < 1") for e in ALL],
    *[(e, dict(capacity=-5), INVALID, "capacity < 0") for e in ALL],
    *[(e, dict(narrow=0x1000), INVALID, "unknown narrow bit") for e in ALL],
    *[(e, dict(narrow=(abi.NARROW_MORTON_LT if e == "rays_bfs" else abi.NARROW_RAY_ORIGIN_OUTSIDE) | abi.OUTPUT_POSITIONS),
       INVALID, "the other menu's code with the positions flag") for e in ALL],
    *[(e, _first_sl(e, 0), INVALID, "start level 0") for e in ALL],
    *[(e, _first_sl(e, -1), INVALID, "start level < 0") for e in ALL],
    *[(e, _first_sl(e, LEVELS1 + 1), INVALID, "start level above levels") for e in ALL],
    *[(e, {**_first_bvh(e, _bvh(N1, built_level=3)), **_first_sl(e, 2)}, INVALID, "start level below built_level") for e in ALL],
    *[(e, {**_first_bvh(e, _bvh(N1, I64, levels=63)), **_first_sl(e, 63)}, INVALID, "levels > 62") for e in ALL],
    *[(e, {**_first_bvh(e, _bvh(1 << 33)), **_first_sl(e, 30)}, OVERFLOW, "Int32 indices, levels > 31") for e in ALL],
    *[(e, dict(res=_result(resume_step=-1)), INVALID, "resume_step < 0") for e in ALL],
    *[(e, dict(res=_result(resume_num=-1)), INVALID, "resume_num < 0") for e in ALL],
    ("bfs", dict(res=_result(resume_step=LEVELS1 + 5)), INVALID, "resume_step > total_levels + 4"),
    ("rays_bfs", dict(res=_result(resume_step=LEVELS1 + 5)), INVALID, "resume_step > total_levels + 4"),
    ("pair_bfs", dict(res=_result(resume_step=LEVELS1 + LEVELS2 + 5)), INVALID, "resume_step > total_levels + 4"),
    # ---- self and pair ------------------------------------------------------------------------------------------------
    *[(e, dict(narrow=abi.NARROW_RAY_ORIGIN_OUTSIDE), INVALID, "ray-menu code") for e in ("bfs", "pair_bfs")],
    ("pair_bfs", dict(bvh2=None), INVALID, "NULL bvh2"),
    ("pair_bfs", dict(sl2=0), INVALID, "start level 0 (bvh2)"),
    ("pair_bfs", dict(sl2=LEVELS2 + 1), INVALID, "start level above levels (bvh2)"),
    ("pair_bfs", dict(bvh2=_bvh(N2, built_level=2), sl2=1), INVALID, "start level below built_level (bvh2)"),
    ("pair_bfs", dict(bvh2=_bvh(1 << 33), sl2=30), OVERFLOW, "Int32 indices, levels > 31 (bvh2)"),
    ("pair_bfs", dict(bvh2=_bvh(N2, MIXED_FLOAT)), UNSUPPORTED, "two type sets"),
    ("pair_bfs", dict(bvh2=_bvh(N2, I64)), UNSUPPORTED, "two index types"),
    ("pair_bfs", dict(bvh2=_bvh(N2, MIXED_FLOAT), bvtt1=None), UNSUPPORTED, "types before NULL queues"),
    ("pair_bfs", dict(bvh2=_bvh(N2, MIXED_FLOAT), sl2=0), INVALID, "levels before types"),
    # ---- rays ---------------------------------------------------------------------------------------------------------
    ("rays_bfs", dict(num_rays=-1), INVALID, "num_rays < 0"),
    ("rays_bfs", dict(points=None), INVALID, "NULL points"),
    ("rays_bfs", dict(dirs=None), INVALID, "NULL dirs"),
    ("rays_bfs", dict(narrow=abi.NARROW_MORTON_LT), INVALID, "pair-menu code MORTON_LT"),
    ("rays_bfs", dict(narrow=abi.NARROW_INDEX_LT), INVALID, "pair-menu code INDEX_LT"),
    ("rays_bfs", dict(bvh=_bvh(N1, MIXED_FLOAT)), UNSUPPORTED, "leaf_float != node_float"),
    ("rays_bfs", dict(bvh=_bvh(N1, MIXED_FLOAT), points=None), UNSUPPORTED, "float types before NULL points"),
    ("rays_bfs", dict(num_rays=(1 << 31)), OVERFLOW, "Int32 indices, num_rays > INT32_MAX"),
    ("rays_bfs", dict(num_rays=(1 << 31), bvtt1=None), INVALID, "NULL queue before the ray count"),
]


@pytest.mark.parametrize("entry, bad, status, what", CASES,
                         ids=[f"{e}-{w.replace(' ', '_')}-{i}" for i, (e, _, _, w) in enumerate(CASES)])
def test_entry_point_status(entry, bad, status, what):
    got, _ = _call(entry, **dict(bad))
    assert got == status, f"ibvh_traverse_{entry} ({what}): status {got}, expected {status}"


def test_nothing_to_traverse_is_ok_without_buffers():
    """One leaf (bfs/traverse_single.jl:17-21) and no rays: IBVH_OK, an empty result, no buffer looked at."""
    for entry, bad in (("bfs", dict(bvh=_bvh(1))), ("rays_bfs", dict(num_rays=0, points=None, dirs=None))):
        st, res = _call(entry, bvtt1=None, bvtt2=None, counters=None, capacity=0, res=_result(3, 7), **bad)
        assert st == OK, entry
        assert (res.num_contacts, res.num_checks, res.contacts_in, res.required_capacity) == (0, 0, 1, 0), entry
        assert (res.resume_step, res.resume_num) == (3, 7)  # (left as they came)
    # the level checks come first
    assert _call("bfs", bvh=_bvh(1), sl=2)[0] == INVALID
    assert _call("rays_bfs", num_rays=0, sl=0)[0] == INVALID
    assert _call("rays_bfs", num_rays=0, bvh=_bvh(N1, MIXED_FLOAT))[0] == UNSUPPORTED


def _tree_only(n):
    """what the checker's initial queues need of a BVH: its tree"""
    class T:
        tree = _bvh(n).tree
    return T


@pytest.mark.parametrize("index_type", [abi.I32, abi.I64], ids=["i32", "i64"])
def test_fresh_call_below_the_initial_queue_reports_what_it_needs(index_type):
    types = abi.make_types(index_type=index_type)
    b1, b2 = _bvh(N1, types), _bvh(N2, types)
    t1, t2 = _tree_only(N1), _tree_only(N2)
    cases = []
    for sl in range(1, LEVELS1 + 1):
        cases.append(("bfs", dict(bvh=b1, sl=sl), len(chk.self_initial(t1, sl))))
        cases.append(("rays_bfs", dict(bvh=b1, sl=sl), chk.level_num_real(t1.tree, sl) * NR))
        for sl2 in (1, LEVELS2 // 2, LEVELS2):
            cases.append(("pair_bfs", dict(bvh1=b1, bvh2=b2, sl1=sl, sl2=sl2), len(chk.pair_initial(t1, t2, sl, sl2))))
    for entry, args, total0 in cases:
        if total0 < 2:
            continue
        st, res = _call(entry, capacity=total0 - 1, **args)
        assert st == CAPACITY, (entry, args)
        assert res.required_capacity == total0 + total0 // 4 + 1024, (entry, args)
        assert (res.resume_step, res.resume_num, res.contacts_in) == (0, 0, 1), (entry, args)
        assert (res.num_contacts, res.num_checks) == (0, 0)


@pytest.mark.parametrize("n", [5, 11, 1001])
def test_initial_capacity_is_the_checkers_step_zero(n):
    b, t = _bvh(n), _tree_only(n)
    out = C.c_int64(-1)
    L = lib.load()
    for sl in range(1, b.tree.levels + 1):
        assert L.ibvh_bfs_initial_capacity(C.byref(b), sl, C.byref(out)) == OK
        assert out.value == len(chk.self_initial(t, sl)), sl
        for nr in (0, 1, 777):
            assert L.ibvh_bfs_rays_initial_capacity(C.byref(b), nr, sl, C.byref(out)) == OK
            assert out.value == chk.level_num_real(t.tree, sl) * nr, (sl, nr)
        for n2 in (5, 11):
            b2, t2 = _bvh(n2), _tree_only(n2)
            for sl2 in range(1, b2.tree.levels + 1):
                assert L.ibvh_bfs_pair_initial_capacity(C.byref(b), C.byref(b2), sl, sl2, C.byref(out)) == OK
                assert out.value == len(chk.pair_initial(t, t2, sl, sl2)), (sl, n2, sl2)
                assert L.ibvh_bfs_pair_initial_capacity(C.byref(b2), C.byref(b), sl2, sl, C.byref(out)) == OK
                assert out.value == len(chk.pair_initial(t2, t, sl2, sl))


def test_initial_capacity_and_counters_bytes_refusals():
    L = lib.load()
    b, out, size = _bvh(N1), C.c_int64(-1), C.c_size_t(0)
    low = _bvh(N1, built_level=3)
    deep = _bvh(N1, levels=63)
    assert L.ibvh_bfs_initial_capacity(None, 1, C.byref(out)) == INVALID
    assert L.ibvh_bfs_initial_capacity(C.byref(b), 1, None) == INVALID
    assert L.ibvh_bfs_pair_initial_capacity(None, C.byref(b), 1, 1, C.byref(out)) == INVALID
    assert L.ibvh_bfs_pair_initial_capacity(C.byref(b), None, 1, 1, C.byref(out)) == INVALID
    assert L.ibvh_bfs_pair_initial_capacity(C.byref(b), C.byref(b), 1, 1, None) == INVALID
    assert L.ibvh_bfs_rays_initial_capacity(None, 5, 1, C.byref(out)) == INVALID
    assert L.ibvh_bfs_rays_initial_capacity(C.byref(b), 5, 1, None) == INVALID
    assert L.ibvh_bfs_rays_initial_capacity(C.byref(b), -1, 1, C.byref(out)) == INVALID
    for sl, bv in ((0, b), (-1, b), (LEVELS1 + 1, b), (2, low), (63, deep)):
        assert L.ibvh_bfs_initial_capacity(C.byref(bv), sl, C.byref(out)) == INVALID, sl
        assert L.ibvh_bfs_rays_initial_capacity(C.byref(bv), 5, sl, C.byref(out)) == INVALID, sl
        assert L.ibvh_bfs_pair_initial_capacity(C.byref(bv), C.byref(b), sl, 1, C.byref(out)) == INVALID, sl
        assert L.ibvh_bfs_pair_initial_capacity(C.byref(b), C.byref(bv), 1, sl, C.byref(out)) == INVALID, sl
    assert out.value == -1  # (a refused call writes nothing)
    assert L.ibvh_bfs_counters_bytes(-1, C.byref(size)) == INVALID
    assert L.ibvh_bfs_counters_bytes(5, None) == INVALID
    for total_levels in (0, 1, 17, 62, 124):
        assert L.ibvh_bfs_counters_bytes(total_levels, C.byref(size)) == OK
        assert size.value == (total_levels + 8) * 8 * (1 + chk.GEN_SLOTS)
