"""ibvh_triangle_contacts / triangle_contacts / self_intersections on the GPU: counts, offsets, index, mask, the two contact
points and the ORDER of every query's list are BIT-EQUAL to the brute force over all triangles of
tests/triangle_contacts_checker.py — the definition of the result — through the whole pipeline (volumes from triangles, build,
count, scan, write) for every accepted float / index combination, in the given order, through the Morton-sorted default path
and counting only; the self-intersection of two tori; hand-made meshes straight through the C entry point (tiny trees,
piercing, touching, coplanar and degenerate triangles, NaN and Inf vertices, output subsets, the index guard), offsets in a
permuted order and the capacity guard, skin margins and refit against the stored leaf boxes, the refusals, and one kernel per
pass."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import mesh_query_kit as kit  # noqa: E402
import triangle_contacts_checker as tcc  # noqa: E402
from mesh_query_kit import (FLOATS, MESHES, NP_F, NP_I, assert_one_kernel, bits as _bits, build as _build, leaf_order as _leaf_order,  # noqa: E402
                            stored_boxes as _stored_boxes, tf as _tf)
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_triangle_contacts"


@functools.lru_cache(maxsize=None)
def _reference(mesh, flt):
    """(triangles, queries, brute force in the order 1..n over tight boxes) of a mesh in a dtype: computed once, shared,
    never modified"""
    tris = torus_mesh(*MESHES[mesh]).astype(NP_F[flt])
    q = tcc.pipeline_queries(tris)
    bf = tcc.brute_force(tris, q, idt=np.int64)
    for a in (tris, bf.counts, bf.offsets, bf.query, bf.index, bf.mask, bf.points):
        a.setflags(write=False)   # (q goes through torch.from_numpy, which wants a writable array)
    return tris, q, bf


@functools.lru_cache(maxsize=None)
def _two_tori():
    """torus40 and its rigid transform as ONE mesh of 6,400 triangles, and its self-test in the order 1..n: all pairs with
    shared vertices skipped, and those with ids as well"""
    tris = torus_mesh(*MESHES["torus40"])
    both = np.concatenate([tris, tcc.other(tris)])
    twice = tcc.brute_force(both, both, skip_shared=True, idt=np.int64)
    once = tcc.brute_force(both, both, skip_shared=True, query_ids=np.arange(1, len(both) + 1), idt=np.int64)
    for a in (both, once.index, once.mask, once.points, once.query, twice.index, twice.mask, twice.points, twice.query):
        a.setflags(write=False)
    return both, once, twice


_assert_equal = functools.partial(kit.assert_equal, tcc.QUERY)
_same = functools.partial(kit.same, tcc.QUERY)
SENTINEL = {k: col.sentinel for k, col in tcc.QUERY.columns.items()}


def _call(bvh, tris, q, ids=None, skip=0, **kw):
    """count, scan on the host, write -> dict: counts, the outputs, both flag words and both statuses (kit.two_passes)"""
    ids = None if ids is None else np.asarray(ids).astype(NP_I[bvh.types.index_type])
    return kit.two_passes(tcc.QUERY, bvh, tris, (q, ids), (skip,), **kw)


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_whole_pipeline_is_bit_equal_to_the_brute_force(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, q, bf = _reference(mesh, leaf_flt)
    # the conditions that make the comparison mean something (tests/test_host_triangle_contacts.py pins them on the host too)
    nv = tcc.non_vacuity(bf)
    print(f"{mesh} {floats}: {nv}")
    tcc.assert_non_vacuous(nv)
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    order = _leaf_order(bvh)
    assert sorted(order.tolist()) == list(range(1, len(tris) + 1)) and (np.diff(order) < 0).any()
    exp = tcc.in_leaf_order(bf, order)
    assert (exp.index != bf.index).any()   # the leaf order is not the triangles' own: the order is being tested
    Q = cuda(q)
    got = ibvh.triangle_contacts(bvh, tdev, Q, presorted=True)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.points.dtype == _tf(leaf_flt)
    _assert_equal(got, exp, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.triangle_contacts(bvh, tdev, Q.reshape(-1, 3, 3)), exp, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.triangle_contacts(bvh, tdev.reshape(-1, 3, 3), Q, count_only=True), exp, (mesh, floats, idx, "count"), count_only=True)
    _assert_equal(ibvh.triangle_contacts(bvh, tdev, Q, count_only=True, presorted=True), exp, (mesh, floats, idx, "count, given"), count_only=True)


# ---- 2. one mesh against itself ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
def test_self_intersections_of_two_tori_in_one_mesh(idx):
    both, once, twice = _two_tori()
    n = len(both)
    assert len(once.index) == 384 and len(twice.index) == 768
    assert ((once.query < n // 2) & (once.index > n // 2)).all()   # every one across the two tori, under its lower index
    bvh, tdev = _build(both, idx=idx)
    order = _leaf_order(bvh)
    got = ibvh.self_intersections(bvh, tdev)
    _assert_equal(got, tcc.in_leaf_order(once, order), "self")
    assert (got.index > got.query.to(got.index.dtype)).all()
    _assert_equal(ibvh.self_intersections(bvh, tdev, count_only=True), once, "self, count", count_only=True)
    # without ids every pair appears in both directions, with bits 0-2 and 3-5 of the masks exchanged
    sym = ibvh.triangle_contacts(bvh, tdev, tdev, skip_shared_vertices=True)
    _assert_equal(sym, tcc.in_leaf_order(twice, order), "both directions")
    a, b, mask = sym.query.cpu().numpy(), sym.index.cpu().numpy().astype(np.int64), sym.mask.cpu().numpy()
    there = {(int(x), int(y)): int(m) for x, y, m in zip(a, b, mask)}
    assert len(there) == 768 and all(there[(y, x)] == int(tcc.swap_mask(m)) for (x, y), m in there.items())
    assert sorted((x, y) for (x, y) in there if x < y) == sorted(zip((once.query + 1).tolist(), once.index.tolist()))


# ---- 3. hand-made, straight through the C entry ------------------------------------------------------------------------
UNIT = [0, 0, 0, 1, 0, 0, 0, 1, 0]
HAND = [UNIT,
        [5, 5, 5, 6, 6, 6, 7, 7, 7],             # zero area: collinear
        [9, 9, 9, 9, 9, 9, 9, 9, 9],             # zero area: one point
        [3, 0, 0, 4, 0, 0, 3, 1, 0],
        [0, 0, 3, 1, 0, 3, 0, 1, 3]]
PIERCING = [0.25, 0.25, -1, 0.25, 0.25, 1, 2, 2, 1]          # its edge ab goes through UNIT, UNIT's edge p2p3 through it
TOUCHING = [0.25, 0.25, 0, 0.25, 0.25, 1, 1, 1, 1]           # its vertex a lies on UNIT's face
COPLANAR = [0.125, 0.125, 0, 0.75, 0.125, 0, 0.125, 0.75, 0]  # overlaps UNIT in its plane
COLLINEAR = [0.25, 0.25, -1, 0.25, 0.25, 0.5, 0.25, 0.25, 1]  # zero area, through UNIT: its edges ab and ca pierce it
A_POINT = [0.25, 0.25, 0] * 3                                 # zero area, on UNIT
SLAB = [-10, 0.25, -10, 20, 0.25, -10, 0, 0.25, 30]           # the plane y = 0.25 through triangles 1, 4 and 5
HAND_QUERIES = [PIERCING, TOUCHING, COPLANAR, COLLINEAR, A_POINT, SLAB,
                [np.nan, 0.25, -1, 0.25, 0.25, 1, 2, 2, 1], [0.25, 0.25, -1, 0.25, np.nan, 1, 2, 2, 1], [0.25, 0.25, -1, 0.25, 0.25, 1, 2, 2, np.nan],
                [0.25, 0.25, -1, 0.25, 0.25, np.inf, 2, 2, 1], [-np.inf, 0.25, -1, 0.25, 0.25, 1, 2, 2, 1],
                [3.25, 0.25, -1, 3.25, 0.25, 1, 9, 9, 9],      # through triangle 4, a vertex on triangle 3
                [0.25, 0.25, 2, 0.25, 0.25, 4, 5, 5, 5],       # through triangle 5, a vertex on triangle 2
                [50, 50, 50, 51, 50, 50, 50, 51, 50],           # far from everything
                UNIT]                                            # a mesh triangle itself: coplanar, every vertex shared


def _hand(n, dt):
    rng = np.random.default_rng(17)
    extra = (rng.random((40, 9)) * 6 - 1).astype(dt)
    return np.array(HAND[:n], dt), np.concatenate([np.array(HAND_QUERIES, dt), extra])


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (3, 1), (5, 1), (5, 2), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris, q = _hand(n, dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4}[n] and bvh.built_level == built_level
    order = _leaf_order(bvh)
    boxes = _stored_boxes(bvh, n)
    assert _bits(boxes) == _bits(tcc.tight_boxes(tris))
    exp = tcc.brute_force(tris, q, leaf_order=order, leaf_boxes=boxes, idt=NP_I[idx])
    got = _call(bvh, tris, q)
    _same(got, exp, (n, built_level))
    assert got["flag_count"] == 0 and got["flag"] == 0
    # what the checker itself says about these inputs
    of = lambda i: list(zip(exp.index[exp.query == i].tolist(), exp.mask[exp.query == i].tolist()))
    assert of(0) == [(1, 17)] and exp.points[exp.query == 0].tolist() == [[[0.25, 0.25, 0], [0.5, 0.5, 0]]]
    assert of(1) == [(1, 5)] and exp.points[exp.query == 1].tolist() == [[[0.25, 0.25, 0]] * 2]
    assert of(2) == [] and of(4) == [] and of(3) == [(1, 5)]
    assert exp.counts[6:9].tolist() == [0, 0, 0] and exp.counts[13] == 0 and exp.counts[14] == 0
    if n == 5:
        assert sorted(i for i, _ in of(5)) == [1, 4, 5] and [i for i, _ in of(5)] == [i for i in order if i in (1, 4, 5)]
        assert (np.diff(order) < 0).any() and 4 in [i for i, _ in of(11)] and 5 in [i for i, _ in of(12)]
        assert {0, 1, 3} <= set(exp.counts.tolist()) and exp.counts[9] == 0 and exp.counts[10] == 0
    # ids and the shared-vertex rule straight through the entry
    ids = np.arange(len(q)) % (n + 1)
    for skip in (0, abi.TRIS_SKIP_SHARED_VERTEX):
        e = tcc.brute_force(tris, q, leaf_order=order, leaf_boxes=boxes, query_ids=ids, skip_shared=bool(skip), idt=NP_I[idx])
        _same(_call(bvh, tris, q, ids=ids, skip=skip), e, ("ids", skip))
    # any subset of the outputs; what was not asked for is not written
    subsets = ["".join(x) for k in range(1, 4) for x in itertools.combinations("imp", k)]
    assert len(subsets) == 7
    for outs in subsets:
        _same(_call(bvh, tris, q, outs=outs), exp, outs, outs=outs)
    # num_queries = 0 with a pre-set flag: nothing is touched
    none = _call(bvh, tris, q, num=0, flag=4, rows=3)
    assert none["status_count"] == 0 and none["status"] == 0 and none["flag_count"] == 4 and none["flag"] == 4
    assert (none["counts"] == -7).all() and all((none[k] == SENTINEL[k]).all() for k in "imp")
    # num_triangles below the largest leaf index: those leaves are skipped in both passes, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        cut = _call(bvh, tris, q, num_triangles=n - 2, flag=4)
        assert cut["flag_count"] == 6 and cut["flag"] == 6
        cut_exp = tcc.brute_force(tris[:n - 2], q, leaf_order=order, leaf_boxes=boxes[:n - 2], idt=NP_I[idx])
        assert n < 5 or len(cut_exp.index) < len(exp.index)
        _same(cut, cut_exp, "guard")


def test_two_roots_one_over_a_virtual_sibling_and_a_batch_of_a_wave_and_one():
    """built_level = 2 over 3 leaves: the walk starts from two roots, and the second root's other child is virtual; 65
    queries are a full wave and one lane of a second workgroup"""
    tris = np.array([UNIT, HAND[3], HAND[4]], np.float32)
    rng = np.random.default_rng(65)
    q = np.concatenate([np.array(HAND_QUERIES[:6], np.float32), (rng.random((59, 9)) * 5 - 1).astype(np.float32)])
    q[64] = SLAB
    bvh, _ = _build(tris, built_level=2)
    assert len(q) == 65 and (bvh.tree.levels, bvh.built_level, bvh.tree.real_leaves, bvh.tree.virtual_leaves) == (3, 2, 3, 1)
    exp = tcc.brute_force(tris, q, leaf_order=_leaf_order(bvh), leaf_boxes=_stored_boxes(bvh, 3), idt=np.int32)
    assert set(exp.index.tolist()) == {1, 2, 3} and exp.counts[64] == 3 and {0, 1, 3} <= set(exp.counts.tolist())
    _same(_call(bvh, tris, q), exp)


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["nan_second", "nan_first"])
def test_a_triangle_with_a_nan_vertex_hides_none_and_reads_as_the_definition_says(order, flt):
    dt = NP_F[flt]
    both = np.array([UNIT, [np.nan, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5]], dt)[list(order)]
    q = np.array([PIERCING, TOUCHING, COLLINEAR, SLAB, [0.5, 0.5, 0.25, 0.5, 0.5, 0.75, 2, 2, 2]], dt)
    bvh, _ = _build(both, flt)
    exp = tcc.brute_force(both, q, leaf_order=_leaf_order(bvh), leaf_boxes=_stored_boxes(bvh, 2), idt=np.int32)
    good = order.index(0) + 1
    assert all(good in exp.index[exp.query == i].tolist() for i in range(4))
    got = _call(bvh, both, q)
    _same(got, exp, order)
    assert not np.isnan(got["p"][:got["total"]]).any()


# ---- 4. offsets and capacity -------------------------------------------------------------------------------------------
def test_offsets_in_a_permuted_order_and_the_capacity_guard():
    tris, q, bf = _reference("torus40", abi.F32)
    nq = len(q)
    bvh, _ = _build(tris)
    exp = tcc.in_leaf_order(bf, _leaf_order(bvh))
    total = len(exp.index)
    assert total > 800 and (exp.counts > 0).sum() > 150
    kit.check_offsets_and_capacity(tcc.QUERY, functools.partial(_call, bvh, tris, q), exp)


# ---- 5. skin and refit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_follow_the_stored_leaf_boxes(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, q, bf = _reference("torus40", leaf_flt)
    n = len(tris)
    Q = cuda(q)
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    boxes = _stored_boxes(bvh, n)
    assert (boxes[:, :3] < tcc.tight_boxes(tris)[:, :3]).all()
    exp = tcc.brute_force(tris, q, leaf_order=_leaf_order(bvh), leaf_boxes=boxes, idt=np.int64)
    assert len(exp.index) >= len(bf.index)
    _assert_equal(ibvh.triangle_contacts(bvh, tdev, Q), exp, (floats, "skin"))
    # refit the tight build to moved vertices: the moved triangles' brute force over the refitted boxes
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    moved = (tris + 0.01 * (rng.random(tris.shape) - 0.5)).astype(dt)
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    boxes = _stored_boxes(bvh, n)
    assert _bits(boxes) == _bits(tcc.tight_boxes(moved))
    exp = tcc.brute_force(moved, q, leaf_order=_leaf_order(bvh), leaf_boxes=boxes, idt=np.int64)
    assert (exp.counts != bf.counts).any() and len(exp.index) > 500
    for presorted in (True, False):
        _assert_equal(ibvh.triangle_contacts(bvh, mdev, Q, presorted=presorted), exp, (floats, "refit", presorted))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, q, bf = _reference("torus40", abi.F32)
    nq = len(q)
    Q = cuda(q)
    f = getattr(lib.load(), NAME)
    out = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        qd = cuda(q.astype(NP_F[bvh.types.leaf_float]))
        for mode, counts, offsets, index in ((abi.TRIS_COUNT, api._ptr(out), None, None), (abi.TRIS_WRITE, None, api._ptr(out), api._ptr(out))):
            st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(qd), None, nq, mode, 0, counts, offsets, nq, index,
                   None, None, None, api._stream())
            torch.cuda.synchronize()
            assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), (what, mode)
        with pytest.raises(ValueError):
            ibvh.triangle_contacts(bvh, tdev, qd)
        with pytest.raises(ValueError):
            ibvh.self_intersections(bvh, tdev)
    bvh, tdev = _build(tris)
    for mode in (abi.TRIS_COUNT, abi.TRIS_WRITE):   # a bit of `skip` other than bit 0: refused before anything is read
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(Q), None, nq, mode, 2, api._ptr(out), api._ptr(out), nq, api._ptr(out),
               None, None, None, api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_INVALID_ARG and (out == -7).all()
    with pytest.raises(ValueError):
        ibvh.triangle_contacts(bvh, tdev.double(), Q)          # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.triangle_contacts(bvh, tdev, Q.double())          # queries of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.triangle_contacts(bvh, bad, Q)
    for bad in (Q.cpu(), Q.t(), Q[:, :8], Q.reshape(-1), Q.reshape(-1, 3), q, None):
        with pytest.raises(ValueError):
            ibvh.triangle_contacts(bvh, tdev, bad)
    ids = torch.arange(1, nq + 1, dtype=torch.int32, device="cuda")
    for bad in (ids.cpu(), ids.long(), ids[:nq - 1], ids.reshape(-1, 1), ids.float(), list(range(nq)), 1):
        with pytest.raises(ValueError):
            ibvh.triangle_contacts(bvh, tdev, Q, query_ids=bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.triangle_contacts(bvh, tdev[:10], Q)              # flag bit 1
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.triangle_contacts(bvh, tdev[:10], Q, count_only=True)
    e = ibvh.triangle_contacts(bvh, tdev, Q[:0])
    assert e.offsets.tolist() == [0] and e.counts.shape == (0,) and e.index.shape == (0,) and e.index.dtype == torch.int32
    assert e.mask.shape == (0,) and e.mask.dtype == torch.uint8 and e.points.shape == (0, 2, 3) and e.query.shape == (0,)
    away = Q + 100
    far = ibvh.triangle_contacts(bvh, tdev, away)              # no contact at all: no write pass, empty outputs
    assert far.offsets.tolist() == [0] * (nq + 1) and far.index.shape == (0,) and far.points.shape == (0, 2, 3) and far.query.shape == (0,)
    assert_one_kernel(lambda: ibvh.triangle_contacts(bvh, tdev, away, presorted=True), "tritri_walk_kernel", "no write pass")


# ---- 7. one kernel per pass --------------------------------------------------------------------------------------------
def test_each_pass_is_one_kernel_of_the_new_translation_unit():
    tris, q, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    Q = cuda(q)
    # the write pass goes straight through the C entry, and writes index and mask alone
    kit.check_each_pass_is_one_kernel(tcc.QUERY, bvh, tdev, functools.partial(ibvh.triangle_contacts, bvh, tdev, Q, presorted=True),
                                      (Q, None), (0,), "im")
