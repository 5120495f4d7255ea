"""ibvh_point_crossings / point_crossings / points_inside / signed_distance on the GPU: crossings and winding are EQUAL to the
brute force over all triangles of tests/point_crossings_checker.py — the definition of the result — through the whole
pipeline (volumes from triangles, build, one launch) for every accepted float / index combination and every axis, in the
given order and through the Morton-sorted default path; hand-made meshes straight through the C entry point (tiny trees,
every built level, rays along edges, through silhouette edges and in a face's plane, zero-area triangles, NaN, output
subsets, the index guard), skin margins and refit, the Python surface, the refusals, and the one launch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import point_crossings_checker as pcc  # noqa: E402
from mesh_query_kit import FLOATS, MESHES, NP_F, NP_I, assert_one_kernel, build as _build, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_point_crossings"


@functools.lru_cache(maxsize=None)
def _reference(mesh, flt, axis):
    """(triangles, points, brute force) of a mesh in a dtype for an axis: computed once, shared, never modified"""
    tris = torus_mesh(*MESHES[mesh]).astype(NP_F[flt])
    p = pcc.query_points(tris, NP_F[flt], axis)
    bf = pcc.brute_force(tris, p, axis, idt=np.int64)
    for a in (tris, bf.crossings, bf.winding):  # (p goes through torch.from_numpy, which wants a writable array)
        a.setflags(write=False)
    return tris, p, bf


def _assert_equal(got, exp, what):
    assert (got.crossings.cpu().numpy() == exp.crossings).all(), what
    assert (got.winding.cpu().numpy() == exp.winding).all(), what


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_whole_pipeline_is_equal_to_the_brute_force(mesh, floats, idx, axis):
    leaf_flt, node_flt = FLOATS[floats]
    tris, p, bf = _reference(mesh, leaf_flt, axis)
    # the conditions that make the comparison mean something (tests/test_host_point_crossings.py pins them on the host too)
    print(f"{mesh} {floats} axis {axis}: (odd, even above 0, none, vertex rays with a crossing, fewest of a centroid ray) = {pcc.non_vacuity(bf)}")
    pcc.assert_non_vacuous(bf)
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    P = cuda(p).t()
    got = ibvh.point_crossings(bvh, tdev, P, axis=axis, presorted=True)
    idt = torch.int32 if idx == abi.I32 else torch.int64
    assert got.crossings.dtype == idt and got.winding.dtype == idt and got.crossings.shape == got.winding.shape == (800,)
    _assert_equal(got, bf, (mesh, floats, idx, axis, "given order"))
    _assert_equal(ibvh.point_crossings(bvh, tdev, P, axis=axis), bf, (mesh, floats, idx, axis, "sorted"))
    _assert_equal(ibvh.point_crossings(bvh, tdev.reshape(-1, 3, 3), P, axis=axis), bf, (mesh, floats, idx, axis, "(n, 3, 3)"))


# ---- 2. hand-made, straight through the C entry ------------------------------------------------------------------------
def _call(bvh, tris, p, axis, num_triangles=None, flag=0, outs="cw", num_points=None):
    """-> dict of numpy outputs (prefilled with a sentinel so that 'not written' is visible), the flag word, the status"""
    n = len(p) if num_points is None else num_points
    T, Pp = cuda(tris), cuda(p)
    idt = api._torch_index(bvh.types.index_type)
    o = {k: torch.full((max(len(p), 1),), -7, dtype=idt, device="cuda") for k in "cw"}
    fl = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    ptr = lambda k: api._ptr(o[k]) if k in outs else None
    st = getattr(lib.load(), NAME)(C.byref(bvh.struct()), api._ptr(T), len(tris) if num_triangles is None else num_triangles,
                                   api._ptr(Pp), n, axis, ptr("c"), ptr("w"), api._ptr(fl), api._stream())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["flag"], out["status"] = int(fl.item()), st
    return out


def _same(got, exp, what=None):
    assert got["status"] == 0, what
    assert got["c"].dtype == exp.crossings.dtype and (got["c"] == exp.crossings).all() and (got["w"] == exp.winding).all(), what


O, X, Y, Z = [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]
TETRA = [O + Y + X, O + X + Z, O + Z + Y, X + Y + Z]                       # the unit tetrahedron, outward
HAND = TETRA + [[5, 5, 5, 6, 6, 6, 7, 7, 7], [9, 9, 9, 9, 9, 9, 9, 9, 9]]   # + zero area: collinear, one point
HAND_POINTS = [[0.1, 0.1, 0.1], [-1, .25, .25], [-1, 0, 0], [-1, .5, .5], [-1, 0, .5],   # inside; through; along an edge; silhouette; in a plane
               [.25, -1, .25], [.25, .25, -1], [0, 0, -1], [.5, .5, -1], [.5, -1, 0], [2, .1, .1], [.1, .1, 2], [-1, -1, -1],
               [np.nan, .1, .1], [.1, np.nan, .1], [.1, .1, np.nan], [np.inf, .1, .1], [.1, np.inf, .1], [.1, .1, np.inf],
               [5.5, 5.5, 5.5], [6, 6, 6], [4, 5.5, 5.5], [9, 9, 9], [8, 9, 9], [9, 8, 9], [9, 9, 8], [.2, .3, .1], [.3, .3, .3], [.4, .3, .3]]


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (5, 1), (5, 2), (5, 4), (6, 1), (6, 2), (6, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris, p = np.array(HAND[:n], dt), np.array(HAND_POINTS, dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4, 6: 4}[n] and bvh.built_level == built_level
    for axis in (0, 1, 2):
        exp = pcc.brute_force(tris, p, axis, idt=NP_I[idx])
        got = _call(bvh, tris, p, axis)
        _same(got, exp, (n, built_level, axis))
        assert got["flag"] == 0
        if n >= 4:
            # what the checker itself says about these inputs (the closed tetrahedron)
            assert (exp.crossings[0], exp.winding[0]) == (1, 1) and (exp.crossings[13:19] == 0).all()
            assert (exp.crossings % 2 == 0)[1:26].all() and (exp.winding[1:26] == 0).all()
            assert (exp.crossings[26:28] == 1).all() and (exp.winding[26:28] == 1).all() and exp.crossings[28] == 0
            if axis == 0:
                assert exp.crossings[1:5].tolist() == [2, 0, 0, 0]
        # either output alone; what was not asked for is not written
        for outs in ("c", "w"):
            sub = _call(bvh, tris, p, axis, outs=outs)
            assert sub["status"] == 0
            for k, e in (("c", exp.crossings), ("w", exp.winding)):
                assert (sub[k] == e).all() if k in outs else (sub[k] == -7).all(), (outs, k)
    # the faces reversed: winding -1 inside
    if n >= 4:
        rev = np.ascontiguousarray(tris.reshape(-1, 3, 3)[:, ::-1].reshape(-1, 9))
        got = _call(bvh, rev, p, 1)
        _same(got, pcc.brute_force(rev, p, 1, idt=NP_I[idx]), "reversed")
        assert got["w"][0] == -1 and got["c"][0] == 1
    # num_points = 0 with a pre-set flag: nothing is touched
    none = _call(bvh, tris, p, 0, num_points=0, flag=4)
    assert none["status"] == 0 and none["flag"] == 4 and all((none[k] == -7).all() for k in "cw")
    # num_triangles below the largest leaf index: those leaves are skipped, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        cut = _call(bvh, tris, p, 0, num_triangles=n - 2, flag=4)
        assert cut["flag"] == 6
        _same(cut, pcc.brute_force(tris[:n - 2], p, 0, idt=NP_I[idx]), "guard")


def test_two_roots_one_over_a_virtual_sibling_and_a_batch_of_a_wave_and_one():
    """built_level = 2 over 3 leaves: the walk starts from two roots, and the second root's other child is virtual; 65
    points are a full wave and one lane of a second workgroup"""
    tris = np.array(TETRA[:3], np.float32)
    rng = np.random.default_rng(65)
    p = np.concatenate([np.array(HAND_POINTS[:13], np.float32), (rng.random((52, 3)) * 1.5 - 0.75).astype(np.float32)])
    bvh, _ = _build(tris, built_level=2)
    assert len(p) == 65 and (bvh.tree.levels, bvh.built_level, bvh.tree.real_leaves, bvh.tree.virtual_leaves) == (3, 2, 3, 1)
    for axis in (0, 1, 2):
        hit, _ = pcc.evaluate(tris, p, axis)
        exp = pcc.brute_force(tris, p, axis)
        _same(_call(bvh, tris, p, axis), exp, axis)
        assert hit.any() and exp.crossings[64] == hit[64].sum()
    assert all(pcc.evaluate(tris, p, a)[0].any(axis=0)[k] for k, a in ((0, 2), (1, 1), (2, 0)))  # ... every leaf, hence either root


# ---- 3. skin and refit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_keep_the_result_exact(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    axis = 2
    tris, p, bf = _reference("torus40", leaf_flt, axis)
    P = cuda(p).t()
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    _assert_equal(ibvh.point_crossings(bvh, tdev, P, axis=axis), bf, (floats, "skin"))
    # refit the tight build to moved vertices: the moved triangles' brute force.  Vertices are moved, not corners of
    # triangles: shared vertices stay bit-identical, the mesh stays closed
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    verts, inverse = np.unique(tris.reshape(-1, 3), axis=0, return_inverse=True)
    shift = (0.01 * (rng.random(verts.shape) - 0.5)).astype(dt)
    moved = np.ascontiguousarray((verts + shift)[inverse.reshape(-1)].reshape(-1, 9).astype(dt))
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = pcc.brute_force(moved, p, axis, idt=np.int64)
    assert (exp.crossings != bf.crossings).any() and (exp.winding != bf.winding).any()
    assert set(np.unique(exp.winding[pcc.OFF_SURFACE]).tolist()) <= {0, 1}
    for presorted in (True, False):
        _assert_equal(ibvh.point_crossings(bvh, mdev, P, axis=axis, presorted=presorted), exp, (floats, "refit", presorted))


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_points_inside_and_signed_distance(flt):
    axis = 1
    tris, p, bf = _reference("torus40", flt, axis)
    bvh, tdev = _build(tris, flt)
    P = cuda(p).t()
    inside = {}
    for rule, exp in (("parity", bf.crossings % 2 == 1), ("winding", bf.winding != 0)):
        got = ibvh.points_inside(bvh, tdev, P, axis=axis, rule=rule)
        assert got.dtype == torch.bool and got.shape == (800,)
        assert (got.cpu().numpy() == exp).all(), rule
        assert 200 <= exp.sum() <= 600
        inside[rule] = got
    by_default = pcc.brute_force(tris, p, 0)                  # axis=0, rule="parity"
    assert (ibvh.points_inside(bvh, tdev, P).cpu().numpy() == (by_default.crossings % 2 == 1)).all()
    cp = ibvh.closest_points(bvh, tdev, P)
    mag = torch.sqrt(cp.distance2)
    for rule in ("parity", "winding"):
        dist, got = ibvh.signed_distance(bvh, tdev, P, axis=axis, rule=rule)
        assert dist.dtype == _tf(flt) and dist.shape == (800,)
        assert torch.equal(got.index, cp.index) and torch.equal(got.distance2, cp.distance2) and torch.equal(got.point, cp.point)
        assert torch.equal(dist.abs().view(torch.int64 if flt == abi.F64 else torch.int32), mag.view(torch.int64 if flt == abi.F64 else torch.int32))
        assert torch.equal(torch.signbit(dist), inside[rule])
    # bounded: +Inf where closest_points found nothing within the radius, inside or not
    r = 0.05
    cpr = ibvh.closest_points(bvh, tdev, P, max_distance=r)
    dist, got = ibvh.signed_distance(bvh, tdev, P, axis=axis, max_distance=r)
    none = cpr.index == 0
    assert torch.equal(got.index, cpr.index) and torch.equal(got.distance2, cpr.distance2)
    assert 100 <= int(none.sum()) <= 700 and int((none & inside["parity"]).sum()) >= 20
    assert torch.isposinf(dist[none]).all() and torch.isfinite(dist[~none]).all()
    assert torch.equal(torch.signbit(dist[~none]), inside["parity"][~none])
    assert torch.equal(dist[~none].abs(), torch.sqrt(cpr.distance2[~none]))
    with pytest.raises(ValueError):
        ibvh.points_inside(bvh, tdev, P, rule="odd")
    with pytest.raises(ValueError):
        ibvh.signed_distance(bvh, tdev, P, rule="odd")
    with pytest.raises(ValueError):
        ibvh.signed_distance(bvh, tdev, P, axis=3)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, p, bf = _reference("torus40", abi.F32, 0)
    P = cuda(p).t()
    f = getattr(lib.load(), NAME)
    out = torch.full((800,), -7, dtype=torch.int32, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        pts = cuda(p.astype(NP_F[bvh.types.leaf_float]))
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(pts), 800, 0, api._ptr(out), api._ptr(out), None, api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), what
        for fn in (ibvh.point_crossings, ibvh.points_inside, ibvh.signed_distance):
            with pytest.raises(ValueError):
                fn(bvh, tdev, pts.t())
    bvh, tdev = _build(tris)
    st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(cuda(p)), 800, 3, api._ptr(out), None, None, api._stream())
    torch.cuda.synchronize()
    assert st == abi.ERR_INVALID_ARG and (out == -7).all()
    for axis in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="axis"):
            ibvh.point_crossings(bvh, tdev, P, axis=axis)
    with pytest.raises(ValueError):
        ibvh.point_crossings(bvh, tdev.double(), P)          # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.point_crossings(bvh, tdev, P.double())          # points of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.point_crossings(bvh, bad, P)
    for bad in (P.cpu(), P.t(), P[:2], P.reshape(-1), p):
        with pytest.raises(ValueError):
            ibvh.point_crossings(bvh, tdev, bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.point_crossings(bvh, tdev[:10], P)              # flag bit 1
    e = ibvh.point_crossings(bvh, tdev, P[:, :0])
    assert e.crossings.shape == (0,) and e.winding.shape == (0,) and e.crossings.dtype == torch.int32 and e.winding.dtype == torch.int32
    assert ibvh.points_inside(bvh, tdev, P[:, :0]).shape == (0,)
    d, c = ibvh.signed_distance(bvh, tdev, P[:, :0])
    assert d.shape == (0,) and d.dtype == torch.float32 and c.index.shape == (0,) and c.point.shape == (0, 3)


# ---- 6. one launch -----------------------------------------------------------------------------------------------------
def test_one_call_is_one_kernel_of_the_new_translation_unit():
    tris, p, bf = _reference("torus40", abi.F32, 0)
    bvh, tdev = _build(tris)
    P = cuda(p).t()
    assert_one_kernel(lambda: ibvh.point_crossings(bvh, tdev, P, presorted=True), "crossings_walk_kernel")
