"""ibvh_closest_triangles / closest_points on the GPU: index, squared distance and closest point are BIT-EQUAL to the brute
force over all triangles of tests/closest_point_checker.py — the definition of the result — through the whole pipeline
(volumes from triangles, build, one launch) for every accepted float / index combination, in the given order and through
the Morton-sorted default path; bounded searches, the tie rule, hand-made meshes straight through the C entry point
(tiny trees, all seven regions, degenerate triangles, NaN, output subsets, the index guard), skin margins and refit, the
refusals, and the one launch.

The issue's case "the C entry returns IBVH_ERR_UNSUPPORTED for triangles of the other dtype" cannot be stated at the C
level: the entry point takes no triangle dtype (the triangles ARE of bvh->types.leaf_float); the Python mirror, which sees
the tensor's dtype, raises ValueError for it and that is checked here."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import closest_point_checker as cpc  # noqa: E402
from mesh_query_kit import FLOATS, MESHES, NP_F, NP_I, assert_one_kernel, build as _build, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402



@functools.lru_cache(maxsize=None)
def _reference(mesh, flt):
    """(triangles, points, brute force) of a mesh in a dtype: computed once, shared, never modified"""
    tris = torus_mesh(*MESHES[mesh]).astype(NP_F[flt])
    p = cpc.query_points(tris, NP_F[flt])
    bf = cpc.brute_force(tris, p, idt=np.int64)
    for a in (tris, bf.index, bf.d2, bf.point):  # (p goes through torch.from_numpy, which wants a writable array)
        a.setflags(write=False)
    return tris, p, bf


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_equal(got, exp, what, rows=slice(None)):
    gi = got.index.cpu().numpy()
    assert (gi == exp.index[rows]).all(), what
    assert _bits(got.distance2.cpu().numpy()) == _bits(exp.d2[rows]), what
    assert _bits(got.point.cpu().numpy()) == _bits(exp.point[rows]), what


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_whole_pipeline_is_bit_equal_to_the_brute_force(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, p, bf = _reference(mesh, leaf_flt)
    # the conditions that make the comparison mean something (tests/test_host_closest_points.py pins them on the host too)
    face, edges, vertices = cpc.region_counts(bf.region)
    tied, zero = int((bf.ties >= 2).sum()), int((bf.d2 == 0).sum())
    print(f"{mesh} {floats}: winners face {face} edges {edges} vertices {vertices}, {tied} tied points, {zero} zero distances")
    assert min(face, edges, vertices) >= 50 and tied >= 100 and zero >= 20
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    P = cuda(p).t()
    got = ibvh.closest_points(bvh, tdev, P, presorted=True)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.distance2.dtype == _tf(leaf_flt)
    assert got.point.shape == (800, 3)
    _assert_equal(got, bf, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.closest_points(bvh, tdev, P), bf, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.closest_points(bvh, tdev.reshape(-1, 3, 3), P), bf, (mesh, floats, idx, "(n, 3, 3)"))


def _radius_whose_square_is_a_distance(d2):
    """(r, r * r) with r * r — squared in the dtype — EQUAL to a brute-force d2: the median one, or, since not every float is
    the square of a float, the next larger d2 that is (the square root, nudged by one unit in the last place either way)"""
    dt = d2.dtype.type
    ordered = np.sort(d2)
    for target in ordered[len(ordered) // 2:]:
        root = np.sqrt(target)
        for r in (root, np.nextafter(root, dt(0)), np.nextafter(root, dt(np.inf))):
            if r * r == target:
                return r, target
    raise AssertionError("no brute-force d2 above the median is the square of a float")


# ---- 2. bounded search -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_bounded_search_keeps_exactly_the_points_within_the_radius(flt):
    dt = NP_F[flt]
    tris, p, bf = _reference("torus40", flt)
    bvh, tdev = _build(tris, flt)
    P = cuda(p).t()
    r, target = _radius_whose_square_is_a_distance(bf.d2)
    assert r.dtype == dt and r * r == target
    exp = cpc.brute_force(tris, p, max_d2=target, idt=np.int64)
    inside = bf.d2 <= target
    assert 300 < inside.sum() < 500 and (bf.d2 == target).any()
    assert ((exp.index > 0) == inside).all() and _bits(exp.d2[inside]) == _bits(bf.d2[inside])
    for presorted in (True, False):
        got = ibvh.closest_points(bvh, tdev, P, max_distance=float(r), presorted=presorted)
        _assert_equal(got, exp, (flt, presorted))
        gi, gd, gq = got.index.cpu().numpy(), got.distance2.cpu().numpy(), got.point.cpu().numpy()
        assert (gi[~inside] == 0).all() and np.isposinf(gd[~inside]).all() and (gq[~inside] == 0).all()
        assert (gi[inside] == bf.index[inside]).all() and _bits(gq[inside]) == _bits(bf.point[inside])
    zero = bf.d2 == 0
    got = ibvh.closest_points(bvh, tdev, P, max_distance=0)
    assert ((got.index.cpu().numpy() > 0) == zero).all() and zero.sum() >= 20
    _assert_equal(got, cpc.brute_force(tris, p, max_d2=dt(0), idt=np.int64), (flt, "radius 0"))


# ---- 3. tie rule -------------------------------------------------------------------------------------------------------
def test_a_duplicated_triangle_loses_to_the_smaller_index():
    base, _, _ = _reference("torus40", abi.F32)
    k = 1234
    tris = np.concatenate([base, base[k - 1:k]])
    n = len(base)
    rng = np.random.default_rng(3)
    w = rng.dirichlet((4.0, 4.0, 4.0), 64)            # well inside the triangle
    t64 = tris[k - 1].reshape(3, 3).astype(np.float64)
    target = (w[:, :, None] * t64[None]).sum(1)
    normal = np.cross(t64[1] - t64[0], t64[2] - t64[0])
    p = (target + 1e-3 * normal / np.linalg.norm(normal)).astype(np.float32)
    bf = cpc.brute_force(tris, p, idt=np.int64)
    assert (bf.index == k).all() and (bf.ties >= 2).all()
    bvh, tdev = _build(tris)
    for presorted in (True, False):
        got = ibvh.closest_points(bvh, tdev, cuda(p).t(), presorted=presorted)
        assert (got.index.cpu().numpy() == k).all() and not (got.index.cpu().numpy() == n + 1).any()
        _assert_equal(got, bf, presorted)


# ---- 4. hand-made, straight through the C entry ------------------------------------------------------------------------
def _call(bvh, tris, p, num_triangles=None, flag=0, outs="idq", num_points=None, max_d2=None):
    """-> dict of numpy outputs (prefilled with a sentinel so that 'not written' is visible), the flag word, the status"""
    ft = tris.dtype
    n = len(p) if num_points is None else num_points
    T, Pp = cuda(tris), cuda(p)
    idt = api._torch_index(bvh.types.index_type)
    o = {"i": torch.full((max(len(p), 1),), -7, dtype=idt, device="cuda"), "d": torch.full((max(len(p), 1),), -7.0, dtype=T.dtype, device="cuda"),
         "q": torch.full((max(len(p), 1), 3), -7.0, dtype=T.dtype, device="cuda")}
    fl = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    ptr = lambda k: api._ptr(o[k]) if k in outs else None
    r2 = None if max_d2 is None else C.byref((C.c_float if ft == np.float32 else C.c_double)(max_d2))
    st = getattr(lib.load(), "ibvh_closest_triangles")(C.byref(bvh.struct()), api._ptr(T), len(tris) if num_triangles is None else num_triangles,
                                                       api._ptr(Pp), n, r2, ptr("i"), ptr("d"), ptr("q"), api._ptr(fl), api._stream())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["flag"], out["status"] = int(fl.item()), st
    return out


def _same(got, exp, what=None):
    assert got["status"] == 0, what
    assert (got["i"] == exp.index).all() and _bits(got["d"]) == _bits(exp.d2) and _bits(got["q"]) == _bits(exp.point), what


UNIT = [0, 0, 0, 1, 0, 0, 0, 1, 0]
HAND = [UNIT,
        [5, 5, 5, 6, 6, 6, 7, 7, 7],             # zero area: collinear
        [9, 9, 9, 9, 9, 9, 9, 9, 9],             # zero area: one point
        [3, 0, 0, 4, 0, 0, 3, 1, 0],
        [0, 0, 3, 1, 0, 3, 0, 1, 3]]
REGION_POINTS = [[-1, -1, 1], [2, -0.5, 1], [0.5, -1, 1], [-0.5, 2, 1], [-1, 0.5, 1], [1, 1, 1], [0.25, 0.25, 1]]
HAND_POINTS = REGION_POINTS + [[5.5, 5.5, 5.5], [6.5, 6, 7], [9, 9, 10], [8, 8, 8], [np.nan, 0, 0], [0, np.inf, 0], [3.2, 0.2, -1], [0.2, 0.2, 2.9]]


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (3, 1), (5, 1), (5, 2), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris, p = np.array(HAND[:n], dt), np.array(HAND_POINTS, dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4}[n] and bvh.built_level == built_level
    exp = cpc.brute_force(tris, p, idt=NP_I[idx])
    got = _call(bvh, tris, p)
    _same(got, exp, (n, built_level))
    assert got["flag"] == 0 and not np.isnan(got["d"]).any() and not np.isnan(got["q"]).any()
    # what the checker itself says about these inputs: the seven regions of triangle 1, a NaN point is a miss
    assert exp.region[:7].tolist() == [0, 1, 2, 3, 4, 5, 6] and (exp.index[:7] == 1).all()
    assert exp.index[11] == 0 and np.isposinf(exp.d2[11]) and (exp.point[11] == 0).all()
    if n == 5:
        assert exp.index[7:11].tolist() == [2, 2, 3, 2] and exp.d2[7] == 0 and exp.ties[10] == 2 and exp.index[13:].tolist() == [4, 5]
    # any subset of the outputs; what was not asked for is not written
    for outs in ("i", "d", "q", "id", "dq"):
        sub = _call(bvh, tris, p, outs=outs)
        assert sub["status"] == 0
        for k, e in (("i", exp.index), ("d", exp.d2), ("q", exp.point)):
            assert _bits(sub[k]) == _bits(e.astype(sub[k].dtype)) if k in outs else (sub[k] == -7).all(), (outs, k)
    # a squared radius from the host pointer
    _same(_call(bvh, tris, p, max_d2=2.0), cpc.brute_force(tris, p, max_d2=dt(2.0), idt=NP_I[idx]), "radius")
    # num_points = 0 with a pre-set flag: nothing is touched
    none = _call(bvh, tris, p, num_points=0, flag=4)
    assert none["status"] == 0 and none["flag"] == 4 and all((none[k] == -7).all() for k in "idq")
    # num_triangles below the largest leaf index: those leaves are skipped, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        cut = _call(bvh, tris, p, num_triangles=n - 2, flag=4)
        assert cut["flag"] == 6
        _same(cut, cpc.brute_force(tris[:n - 2], p, idt=NP_I[idx]), "guard")


def test_two_roots_one_over_a_virtual_sibling_and_a_batch_of_a_wave_and_one():
    """built_level = 2 over 3 leaves: the walk starts from two roots, and the second root's other child is virtual; 65
    points are a full wave and one lane of a second workgroup"""
    tris = np.array(HAND[:3], np.float32)
    rng = np.random.default_rng(65)
    p = np.concatenate([np.array(HAND_POINTS[:11], np.float32), (rng.random((54, 3)) * 12 - 1).astype(np.float32)])
    bvh, _ = _build(tris, built_level=2)
    assert len(p) == 65 and (bvh.tree.levels, bvh.built_level, bvh.tree.real_leaves, bvh.tree.virtual_leaves) == (3, 2, 3, 1)
    exp = cpc.brute_force(tris, p, idt=np.int32)
    assert set(exp.index.tolist()) == {1, 2, 3}  # every leaf, hence either root, holds an answer
    _same(_call(bvh, tris, p), exp)


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["nan_second", "nan_first"])
def test_a_triangle_with_a_nan_vertex_never_wins(order, flt):
    dt = NP_F[flt]
    both = np.array([UNIT, [0, 0, 0.5, np.nan, 0, 0.5, 0, 1, 0.5]], dt)[list(order)]
    p = np.array(REGION_POINTS + [[0.2, 0.2, 0.5], [np.nan, np.nan, np.nan]], dt)
    bvh, _ = _build(both, flt)
    exp = cpc.brute_force(both, p, idt=np.int32)
    good = order.index(0) + 1
    assert (exp.index[:-1] == good).all() and exp.index[-1] == 0
    got = _call(bvh, both, p)
    _same(got, exp, order)
    assert not np.isnan(got["d"]).any() and not np.isnan(got["q"]).any()


# ---- 5. skin and refit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_keep_the_result_exact(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, p, bf = _reference("torus40", leaf_flt)
    P = cuda(p).t()
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    _assert_equal(ibvh.closest_points(bvh, tdev, P), bf, (floats, "skin"))
    # refit the tight build to moved vertices: the moved triangles' brute force
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    moved = (tris + 0.01 * (rng.random(tris.shape) - 0.5)).astype(dt)
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = cpc.brute_force(moved, p, idt=np.int64)
    assert (exp.index != bf.index).any() and _bits(exp.d2) != _bits(bf.d2)
    for presorted in (True, False):
        _assert_equal(ibvh.closest_points(bvh, mdev, P, presorted=presorted), exp, (floats, "refit", presorted))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, p, bf = _reference("torus40", abi.F32)
    P = cuda(p).t()
    f = getattr(lib.load(), "ibvh_closest_triangles")
    out = torch.full((800,), -7, dtype=torch.int32, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        pts = cuda(p.astype(NP_F[bvh.types.leaf_float]))
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(pts), 800, None, api._ptr(out), None, None, None, api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), what
        with pytest.raises(ValueError):
            ibvh.closest_points(bvh, tdev, pts.t())
    bvh, tdev = _build(tris)
    with pytest.raises(ValueError):
        ibvh.closest_points(bvh, tdev.double(), P)          # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.closest_points(bvh, tdev, P.double())          # points of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.closest_points(bvh, bad, P)
    for bad in (P.cpu(), P.t(), P[:2], P.reshape(-1), p):
        with pytest.raises(ValueError):
            ibvh.closest_points(bvh, tdev, bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.closest_points(bvh, tdev[:10], P)              # flag bit 1
    e = ibvh.closest_points(bvh, tdev, P[:, :0])
    assert e.index.shape == (0,) and e.distance2.shape == (0,) and e.point.shape == (0, 3) and e.index.dtype == torch.int32


# ---- 7. one launch -----------------------------------------------------------------------------------------------------
def test_one_call_is_one_kernel_of_the_new_translation_unit():
    tris, p, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    P = cuda(p).t()
    assert_one_kernel(lambda: ibvh.closest_points(bvh, tdev, P, presorted=True), "closest_walk_kernel")
