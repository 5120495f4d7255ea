"""ibvh_triangle_distances / triangle_distances, mesh_distance, self_clearance on the GPU: index, kind and the bits of d2 and
of both points are EQUAL to the brute force over all pairs of tests/triangle_distance_checker.py — the definition of the
result — through the whole pipeline (volumes from triangles, build, one launch) for every accepted float combination and both
index types, in the given order and through the Morton-sorted default path; every output alone; a radius; the skip flag on a
mesh against itself; built levels, skin margins, a one-triangle mesh and a leaf count that is no power of two; a NaN query and
the index guard; the refusals, the empty batch and the one launch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import triangle_contacts_checker as tcc  # noqa: E402
import triangle_distance_checker as tdc  # noqa: E402
from mesh_query_kit import FLOATS, NP_F, assert_one_kernel, bits, build as _build, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_triangle_distances"
KERNEL = "tridist_walk_kernel"
QUERIES = {"torus40": 600, "torus64x63": 150}   # 3,200 triangles = 4,096 leaves' worth; 8,064: no power of two
FIELDS = ("index", "d2", "point_query", "point_mesh", "kind")


def _reference(mesh, flt):
    """(triangles, queries, the unbounded brute force): the checker's shared, read-only case"""
    return tdc.reference(mesh, NP_F[flt], QUERIES[mesh])


def _assert_equal(got, exp, what):
    """index and kind by value, d2 and both points BIT FOR BIT"""
    assert isinstance(got, ibvh.TriangleDistances), what
    for field in FIELDS:
        g, e = getattr(got, field).cpu().numpy(), getattr(exp, field)
        assert g.shape == e.shape, (what, field)
        if field == "index":
            assert (g == e).all(), (what, field, int((g != e).sum()))
        else:
            assert g.dtype == e.dtype and bits(g) == bits(e), (what, field, int((g != e).sum()))


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,floats,idx", [("torus40", "f32", abi.I32), ("torus40", "f32", abi.I64), ("torus40", "f64", abi.I32),
                                             ("torus40", "f32_under_f64", abi.I32), ("torus40", "f64", abi.I64),
                                             ("torus64x63", "f32", abi.I32), ("torus64x63", "f64", abi.I32)])
def test_whole_pipeline_is_equal_to_the_checker(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, q, bf = _reference(mesh, leaf_flt)
    n = len(q)
    # what makes the comparison mean something (tests/test_host_triangle_distances.py pins more of it on the host)
    assert (bf.kind == tdc.CUT).sum() >= n // 8 and ((bf.kind >= 3) & (bf.kind < tdc.CUT)).sum() >= n // 30 and (bf.index != 0).all()
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    Q = cuda(np.array(q))
    got = ibvh.triangle_distances(bvh, tdev, Q, presorted=True)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.d2.dtype == _tf(leaf_flt)
    assert got.index.shape == got.d2.shape == got.kind.shape == (n,) and got.point_query.shape == got.point_mesh.shape == (n, 3)
    assert got.kind.dtype == torch.uint8
    _assert_equal(got, bf, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.triangle_distances(bvh, tdev, Q), bf, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.triangle_distances(bvh, tdev.reshape(-1, 3, 3), Q.reshape(-1, 3, 3)), bf, (mesh, floats, idx, "(n, 3, 3)"))
    # the one closest pair of the two meshes: many queries cut the mesh, the tie goes to the lowest position
    d2, pos, index = tdc.global_minimum(bf)
    assert d2 == 0 and (bf.d2 == 0).sum() >= 2
    md = ibvh.mesh_distance(bvh, tdev, Q)
    assert isinstance(md, ibvh.MeshDistance) and (md.distance, md.query, md.index) == (0.0, pos, index)
    assert bits(md.point_query.cpu().numpy()) == bits(bf.point_query[pos - 1]) and bits(md.point_mesh.cpu().numpy()) == bits(bf.point_mesh[pos - 1])
    # ... and of the part that is clear of it: one smallest distance, then the same query twice
    clear = slice(n // 3, 2 * (n // 3))
    sub = tdc.limited(bf, np.inf)
    for field in FIELDS:
        setattr(sub, field, getattr(bf, field)[clear])
    d2, pos, index = tdc.global_minimum(sub)
    md = ibvh.mesh_distance(bvh, tdev, Q[clear])
    assert d2 > 0 and (md.distance, md.query, md.index) == (float(np.sqrt(float(d2))), pos, index)
    twice = torch.cat([Q[clear][pos - 1:pos].expand(3, 9), Q[clear]])
    md = ibvh.mesh_distance(bvh, tdev, twice)
    assert (md.distance, md.query, md.index) == (float(np.sqrt(float(d2))), 1, index)


# ---- 2. a radius -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_max_distance(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, q, bf = _reference("torus40", leaf_flt)
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    Q = cuda(np.array(q))
    radius = float(np.sqrt(np.median(bf.d2[200:400].astype(np.float64))))     # half of the queries that are clear of the mesh
    for what, r in (("the median gap", radius), ("exactly one query's distance", float(np.sqrt(dt(0.25)))), ("zero", 0.0), ("huge", 1e30)):
        with np.errstate(over="ignore"):
            r2 = dt(r) * dt(r)                                                # squared in the triangles' dtype, as the host does
        exp = tdc.limited(bf, r2)
        share = (exp.index != 0).mean()
        if what == "the median gap":
            assert share >= 0.2 and 1 - share >= 0.2, share                   # on the checker's result alone
        for presorted in (True, False):
            _assert_equal(ibvh.triangle_distances(bvh, tdev, Q, max_distance=r, presorted=presorted), exp, (floats, what, presorted))
    # the radius is inclusive: the squared distance of one query, handed to the C entry as it is
    k = 300
    got = _call(bvh, tris, q, max_d2=bf.d2[k])
    _same(got, tdc.limited(bf, bf.d2[k]), "d2 of query 300")
    assert got["i"][k] == bf.index[k] != 0
    below = np.nextafter(bf.d2[k], dt(0))
    assert _call(bvh, tris, q, max_d2=below)["i"][k] == 0


# ---- 3. straight through the C entry -----------------------------------------------------------------------------------
OUTS = "idqmk"
SENTINEL = dict(i=-7, d=-7, q=-7, m=-7, k=249)


def _call(bvh, tris, q, skip=0, max_d2=None, num_triangles=None, flag=0, outs=OUTS, num_queries=None):
    """-> dict of numpy outputs (prefilled with a sentinel so that 'not written' is visible), the flag word, the status"""
    n = len(q) if num_queries is None else num_queries
    rows = max(len(q), 1)
    T, Qd = cuda(np.array(tris)), cuda(np.array(q).reshape(-1, 9))       # (copies: the shared reference arrays are read-only)
    ft, idt = _tf(bvh.types.leaf_float), api._torch_index(bvh.types.index_type)
    o = {"i": torch.full((rows,), -7, dtype=idt, device="cuda"), "d": torch.full((rows,), -7, dtype=ft, device="cuda"),
         "q": torch.full((rows, 3), -7, dtype=ft, device="cuda"), "m": torch.full((rows, 3), -7, dtype=ft, device="cuda"),
         "k": torch.full((rows,), 249, dtype=torch.uint8, device="cuda")}
    fl = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    ptr = lambda k: api._ptr(o[k]) if k in outs else None
    r2 = None if max_d2 is None else C.byref((C.c_float if ft == torch.float32 else C.c_double)(max_d2))
    st = getattr(lib.load(), NAME)(C.byref(bvh.struct()), api._ptr(T), len(tris) if num_triangles is None else num_triangles,
                                   api._ptr(Qd), n, skip, r2, ptr("i"), ptr("d"), ptr("q"), ptr("m"), ptr("k"), api._ptr(fl), api._stream())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["flag"], out["status"] = int(fl.item()), st
    return out


def _same(got, exp, what=None, outs=OUTS):
    assert got["status"] == 0, what
    for k, e in zip(OUTS, (exp.index, exp.d2, exp.point_query, exp.point_mesh, exp.kind)):
        if k in outs:
            assert (got[k] == e).all() if k == "i" else (got[k].dtype == e.dtype and bits(got[k]) == bits(e)), (what, k)
        else:
            assert (got[k] == SENTINEL[k]).all(), (what, k, "not asked for, yet written")


def test_every_output_alone_and_all_together():
    tris, q, bf = _reference("torus40", abi.F32)
    bvh, _ = _build(tris)
    for outs in ("i", "d", "q", "m", "k", "ik", "dqm", OUTS):
        got = _call(bvh, tris, q, outs=outs)
        _same(got, bf, outs, outs=outs)
        assert got["flag"] == 0
    # fewer queries than rows: the rows behind them are untouched
    got = _call(bvh, tris, q, num_queries=77)
    assert got["status"] == 0 and (got["i"][:77] == bf.index[:77]).all() and (got["i"][77:] == -7).all() and (got["k"][77:] == 249).all()
    assert bits(got["d"][:77]) == bits(bf.d2[:77]) and (got["d"][77:] == -7).all() and (got["q"][77:] == -7).all() and (got["m"][77:] == -7).all()


# ---- 4. trees and meshes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", ["f32", "f64"])
@pytest.mark.parametrize("built_level", [2, 3])
def test_built_levels(built_level, floats):
    leaf_flt, node_flt = FLOATS[floats]
    tris, q, bf = _reference("torus40", leaf_flt)
    bvh, tdev = _build(tris, leaf_flt, node_flt, built_level=built_level)
    assert bvh.built_level == built_level
    _assert_equal(ibvh.triangle_distances(bvh, tdev, cuda(np.array(q))), bf, (built_level, floats))


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_leaf_boxes_with_a_skin_give_the_same_result(floats):
    leaf_flt, node_flt = FLOATS[floats]
    tris, q, bf = _reference("torus40", leaf_flt)
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)     # the definition reads the triangle's own box, not the stored one
    Q = cuda(np.array(q))
    for presorted in (True, False):
        _assert_equal(ibvh.triangle_distances(bvh, tdev, Q, presorted=presorted), bf, (floats, "skin", presorted))


HAND = [tcc.FLAT, [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5], tcc.PIERCING, [5, 5, 5, 6, 6, 6, 7, 7, 7], [0, -1, 1, 0, 1, 1, 0, 0, 6]]
nan = np.nan


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (2, 2), (3, 2), (5, 1), (5, 3)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt):
    dt = NP_F[flt]
    tris = np.array(HAND[:n], dt)
    q = np.array([tcc.FLAT, tcc.PIERCING, tcc.TOUCHING, tcc.COPLANAR, tcc.DISJOINT, tcc.FAR, [-1, 0, 0, 1, 0, 0, 0, 0, -5],
                  [1, 1, 1, 1, 1, 1, 1, 1, 1], [nan, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0, 0, 1, nan]], dt)
    bvh, _ = _build(tris, flt, built_level=built_level)
    exp = tdc.brute_force(tris, q)
    assert (exp.index[-2:] == 0).all() and (exp.index[:-2] != 0).all()        # a NaN query has no answer
    got = _call(bvh, tris, q)
    _same(got, exp, (n, built_level))
    assert got["flag"] == 0 and np.isinf(got["d"][-2:]).all() and (got["q"][-2:] == 0).all() and (got["m"][-2:] == 0).all() and (got["k"][-2:] == 0).all()
    _same(_call(bvh, tris, q, skip=abi.TRIS_SKIP_SHARED_VERTEX), tdc.brute_force(tris, q, skip_shared=True), (n, built_level, "skip"))
    _same(_call(bvh, tris, q, max_d2=0.25), tdc.brute_force(tris, q, max_d2=0.25), (n, built_level, "radius"))
    _same(_call(bvh, tris, q, max_d2=nan), tdc.brute_force(tris, q, max_d2=nan), (n, built_level, "a NaN radius"))


def test_duplicate_triangles_the_smaller_index_wins():
    tris, q, bf = _reference("torus40", abi.F32)
    winners = np.unique(bf.index[:240])
    twice = np.concatenate([tris[winners - 1], tris])          # every winner once more, under a smaller index: it wins the tie
    exp = tdc.brute_force(twice, q[:240])
    assert (exp.ties >= 2).all() and (exp.index <= len(winners)).all() and len(winners) >= 100
    bvh, _ = _build(twice)
    _same(_call(bvh, twice, q[:240]), exp, "duplicates")


# ---- 5. a mesh against itself --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(flt):
    tris = torus_mesh(12, 10).astype(NP_F[flt])
    return tris, tdc.brute_force(tris, tris), tdc.brute_force(tris, tris, skip_shared=True)


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skip_shared_vertices_with_the_mesh_as_its_own_queries(floats):
    leaf_flt, node_flt = FLOATS[floats]
    tris, plain, skip = _small(leaf_flt)
    n = len(tris)
    assert n == 240 and (plain.d2 == 0).all() and (skip.d2 > 0).all() and (skip.index != 0).all()
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    _assert_equal(ibvh.triangle_distances(bvh, tdev, tdev), plain, (floats, "itself or a neighbour"))
    got = ibvh.self_clearance(bvh, tdev)
    _assert_equal(got, skip, (floats, "self_clearance"))
    _assert_equal(ibvh.triangle_distances(bvh, tdev, tdev, skip_shared_vertices=True, presorted=True), skip, (floats, "flag"))
    # no triangle reports itself or a neighbour
    index = got.index.cpu().numpy().astype(np.int64)
    assert (index != np.arange(1, n + 1)).all() and not tcc.shares_vertex(tris, tris[index - 1]).any()
    r = float(np.sqrt(np.median(skip.d2.astype(np.float64))))
    lim = tdc.limited(skip, NP_F[leaf_flt](r) * NP_F[leaf_flt](r))
    assert 0.2 <= (lim.index != 0).mean() <= 0.8
    _assert_equal(ibvh.self_clearance(bvh, tdev, max_distance=r), lim, (floats, "self_clearance within a radius"))


# ---- 6. the index guard, refusals, the empty batch, one launch -----------------------------------------------------------
def test_a_leaf_index_outside_the_mesh_raises_flag_bit_1_and_is_skipped():
    tris, q, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    exp = tdc.brute_force(tris[:2000], q[:240])               # leaves 2001..3200 name no row of the 2,000 given
    assert (exp.index != bf.index[:240]).sum() >= 20
    got = _call(bvh, tris, q[:240], num_triangles=2000)
    _same(got, exp, "2,000 of 3,200 triangles")
    assert got["flag"] == 2
    assert _call(bvh, tris, q[:240], num_triangles=2000, flag=4)["flag"] == 6      # the flag word is never cleared
    none = _call(bvh, tris, q[:240], num_triangles=0)
    assert none["flag"] == 2 and (none["i"] == 0).all() and np.isinf(none["d"]).all() and (none["k"] == 0).all()
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.triangle_distances(bvh, tdev[:2000], cuda(np.array(q[:240])))


def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, q, bf = _reference("torus40", abi.F32)
    f = getattr(lib.load(), NAME)
    out = torch.full((600,), -7, dtype=torch.int32, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        Qd = cuda(q.astype(NP_F[bvh.types.leaf_float]))
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(Qd), 600, 0, None, api._ptr(out), None, None, None, None, None,
               api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), what
        for call in (ibvh.triangle_distances, ibvh.mesh_distance):
            with pytest.raises(ValueError):
                call(bvh, tdev, Qd)
        with pytest.raises(ValueError):
            ibvh.self_clearance(bvh, tdev)
    bvh, tdev = _build(tris)
    Q = cuda(np.array(q))
    assert f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(Q), 600, 2, None, api._ptr(out), None, None, None, None, None,
             api._stream()) == abi.ERR_INVALID_ARG and (out == -7).all()                 # a bad skip
    with pytest.raises(ValueError):
        ibvh.triangle_distances(bvh, tdev.double(), Q)          # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.triangle_distances(bvh, tdev, Q.double())          # queries of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.triangle_distances(bvh, bad, Q)
    for bad in (Q.cpu(), Q.to(torch.int32), Q[:, :8], Q.reshape(-1), Q.t(), q):
        with pytest.raises(ValueError):
            ibvh.triangle_distances(bvh, tdev, bad)
    e = ibvh.triangle_distances(bvh, tdev, Q[:0])
    assert e.index.shape == e.d2.shape == e.kind.shape == (0,) and e.point_query.shape == e.point_mesh.shape == (0, 3)
    assert e.index.dtype == torch.int32 and e.d2.dtype == e.point_query.dtype == torch.float32 and e.kind.dtype == torch.uint8
    md = ibvh.mesh_distance(bvh, tdev, Q[:0])
    assert (md.distance, md.query, md.index) == (float("inf"), 0, 0)
    md = ibvh.mesh_distance(bvh, tdev, Q[400:], max_distance=1.0)          # far away: none within the radius
    assert (md.distance, md.query, md.index) == (float("inf"), 0, 0) and (md.point_query == 0).all() and (md.point_mesh == 0).all()


def test_one_call_is_one_kernel_of_the_new_translation_unit():
    tris, q, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    Q = cuda(np.array(q))
    for kw in (dict(), dict(max_distance=0.5), dict(skip_shared_vertices=True)):
        assert_one_kernel(lambda: ibvh.triangle_distances(bvh, tdev, Q, presorted=True, **kw), KERNEL, kw)
