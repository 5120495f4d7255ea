"""ibvh_point_crossings on the host side: the header declares it (additive under ABI version 7) and carries its contract, the
ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its one
launch goes through the profiling wrapper and the shared walk, and the entry point validates its arguments — the axis and
the refused type combinations included — before any launch.  The numpy checker the GPU test pins the kernel to
(tests/point_crossings_checker.py) is watertight where the uncanonicalised rule is not, agrees with the analytic torus, its
guard on a triangle's box implies the guard on every enclosing box, and the GPU test's non-vacuity conditions hold for the
brute force alone.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib
from implicitbvh_amd.synthetic import torus_mesh

import mesh_query_kit as kit
import point_crossings_checker as pcc
from mesh_query_kit import MESHES

NAME = "ibvh_point_crossings"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *points", "int64_t num_points",
                    "int32_t axis", "void *crossings", "void *winding", "void *flag", "void *stream"]
    assert NAME in note and note.count("additive") >= 4
    # the doc comment carries the contract: the cyclic coordinates, the four rules, why it is watertight and lossless, the limits
    doc = raw[raw.index("inside / outside: the triangles an axis ray from a query point crosses"):raw.index("ibvh_status " + NAME)]
    for phrase in ("u = (axis + 1) % 3;  v = (axis + 2) % 3;  w = axis", "orientation is preserved", "false on NaN",
                   "max3(A.w, B.w, C.w) >= P.w", "CANONICAL", "lexicographically smaller than X on (u, v, w)",
                   "e = (Y.u - X.u)*(P.v - X.v) - (Y.v - X.v)*(P.u - X.u)", "left = (e >= 0)", "a tie goes LEFT", "side = left XOR flipped",
                   "ccw = all three sides true", "cw = all three false", "s = (N0*d.u + N1*d.v) + N2*d.w",
                   "(ccw && s < 0) || (cw && s > 0)", "s == 0", "WATERTIGHT", "same bits for e", "lossless WITHOUT an epsilon",
                   "comparisons hold on the box", "contains the boxes below it exactly", "ON the surface is ambiguous",
                   "bit-identical", "T-junctions or cracks", "orientation-independent", "unions of overlapping closed bodies",
                   "IBVH_ERR_UNSUPPORTED", "a sphere does not contain its triangle exactly", "skin margin", "ibvh_refit", "bit 1",
                   "not written", "num_points == 0", "No reference counterpart", "ALL triangles"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 4
    assert lib.SIGNATURES[NAME] == want == abi.POINT_CROSSINGS_ARGTYPES
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("point_crossings", "PointCrossings", "points_inside", "signed_distance"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    # the walk, its block size and grid, the prologue, the dispatch and the flag are the shared ones
    src = kit.query_unit("ibvh_crossings.hip", "crossings::crossings_walk_kernel", own_gather=True)
    assert "box_bound" not in src
    # three (T, TN) instantiations times two index types — the shared dispatch —, not times three axes
    assert "template <class T, class TN, class I>" in src and "int u, int v" in src


def test_julia_wrapper_binds_it_with_the_ctypes_signature_and_the_docs_name_it():
    src = kit.julia_ccall(NAME, "point_crossings")
    assert "point_crossings(" in src[src.index("function points_inside("):]
    assert "function ImplicitBVH.points_inside" not in src
    design = kit.read("DESIGN.md")
    section = design[design.index("Inside / outside of a closed mesh"):][:6000]
    for phrase in ("no reference counterpart", "lossless", "canonical", "watertight", "ambiguous", "T-junctions", "VGPRs", "scratch"):
        assert phrase in section, phrase
    assert kit.read("tools", "bench_inside.py")


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    ok = dict(bvh=_fake_bvh(), tris=p, nt=5, pts=p, np_=0, axis=0, cr=p, wi=None, flag=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["pts"], a["np_"], a["axis"], a["cr"], a["wi"], a["flag"], a["stream"])
    assert call() == abi.OK                                        # num_points = 0: nothing to do
    assert call(axis=1) == abi.OK and call(axis=2) == abi.OK
    assert call(cr=None) == abi.ERR_INVALID_ARG                    # both outputs NULL
    assert call(cr=None, wi=p) == abi.OK and call(wi=p) == abi.OK  # ... either one alone, or both
    for bad in (dict(bvh=None), dict(nt=-1), dict(np_=-1), dict(tris=None), dict(np_=5, pts=None), dict(axis=-1), dict(axis=3),
                dict(axis=-1, np_=5), dict(axis=3, np_=5), dict(bvh=_fake_bvh(leaves=None)), dict(bvh=_fake_bvh(nodes=None)),
                dict(bvh=_fake_bvh(built_level=0)), dict(bvh=_fake_bvh(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
    assert call(tris=None, nt=0) == abi.OK
    assert call(bvh=_fake_bvh(n=1, nodes=None)) == abi.OK          # a one-leaf tree has no nodes
    broken = _fake_bvh()
    broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # the accepted types: BBox leaves under BBox nodes of the same or a wider float type, any index type
    for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64)):
        assert call(bvh=_fake_bvh(**good)) == abi.OK, good
    for bad in (dict(leaf_kind=abi.BSPHERE), dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE), dict(node_kind=abi.BSPHERE),
                dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
        # (with points to process too: refused, never launched on the fake pointers)
        assert call(bvh=_fake_bvh(**bad)) == abi.ERR_UNSUPPORTED and call(bvh=_fake_bvh(**bad), np_=5) == abi.ERR_UNSUPPORTED, bad


# ---- the checker --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(mesh, dt, axis):
    tris = torus_mesh(*MESHES[mesh]).astype(dt)
    p = pcc.query_points(tris, dt, axis)
    assert p.shape == (800, 3) and p.dtype == dt
    return tris, p, pcc.brute_force(tris, p, axis)


CASES = [(m, dt, a) for m in sorted(MESHES) for dt in (np.float32, np.float64) for a in (0, 1, 2)]
IDS = [f"{m}-{np.dtype(dt).name}-axis{a}" for m, dt, a in CASES]


@pytest.mark.parametrize("mesh,dt,axis", CASES, ids=IDS)
def test_checker_is_watertight_and_agrees_with_the_analytic_torus(mesh, dt, axis):
    tris, p, bf = _case(mesh, dt, axis)
    assert bf.crossings.dtype == np.int32 and bf.winding.dtype == np.int32
    off = pcc.OFF_SURFACE
    assert len(off) == 700
    # a closed, outward-oriented 2-manifold: every off-surface point sees winding 0 or 1, and parity says the same
    assert set(np.unique(bf.winding[off]).tolist()) <= {0, 1}
    assert ((bf.crossings[off] % 2 == 1) == (bf.winding[off] == 1)).all()
    inside, margin = pcc.analytic_inside(p)
    far = margin > 0.03
    far[pcc.VERTICES] = False
    mismatches = int(((bf.winding == 1) != inside)[far].sum())
    print(f"{mesh} {np.dtype(dt).name} axis {axis}: compared {int(far.sum())} points, {mismatches} mismatches, "
          f"{int(inside[far].sum())} of them inside")
    assert far.sum() >= 600 and mismatches == 0
    assert inside[far].sum() >= 100 and (~inside[far]).sum() >= 100


@pytest.mark.parametrize("mesh,dt,axis", CASES, ids=IDS)
def test_point_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh, dt, axis):
    tris, p, bf = _case(mesh, dt, axis)
    odd, even, none, vray, cen = pcc.non_vacuity(bf)
    nv = pcc.naive(tris, p, axis)
    differs = int(((nv.crossings != bf.crossings) | (nv.winding != bf.winding)).sum())
    print(f"{mesh} {np.dtype(dt).name} axis {axis}: odd {odd}, even above 0 {even}, none {none}, vertex rays with a crossing {vray}, "
          f"fewest crossings of a centroid ray {cen}, naive differs on {differs} (its winding: {nv.winding.min()} .. {nv.winding.max()})")
    assert odd >= 200 and even >= 150 and none >= 200
    assert vray >= 100
    assert (bf.crossings[pcc.CENTROIDS] >= 2).all()
    assert differs >= 100
    pcc.assert_non_vacuous(bf)
    # the vertex rays keep a vertex's u and v bit for bit
    u, v, _ = pcc.cyclic(axis)
    verts = tris.reshape(-1, 3)
    keys = set(map(bytes, np.ascontiguousarray(verts[:, [u, v]])))
    assert all(bytes(np.ascontiguousarray(r)) in keys for r in p[pcc.VERTEX_RAYS][:, [u, v]])


@pytest.mark.parametrize("mesh,dt,axis", CASES, ids=IDS)
def test_guard_on_a_triangles_box_implies_the_guard_on_every_enclosing_box(mesh, dt, axis):
    tris, p, bf = _case(mesh, dt, axis)
    hit, _ = pcc.evaluate(tris, p, axis)
    lo, up = pcc.triangle_boxes(tris)
    own = pcc.box_guard(lo[None], up[None], p[:, None, :], axis)
    assert own.shape == hit.shape == (800, len(tris))
    assert (own | ~hit).all() and hit.sum() == bf.crossings.sum()     # a crossing passes the guard on its own box
    s = dt(0.01)                                                        # a skin margin
    assert (pcc.box_guard((lo - s)[None], (up + s)[None], p[:, None, :], axis) | ~own).all()
    lo2, up2 = np.minimum(lo[0::2], lo[1::2]), np.maximum(up[0::2], up[1::2])   # the union of neighbouring boxes = a node
    g2 = pcc.box_guard(lo2[None], up2[None], p[:, None, :], axis)
    assert (g2 | ~own[:, 0::2]).all() and (g2 | ~own[:, 1::2]).all()
    print(f"{mesh} {np.dtype(dt).name} axis {axis}: the guard admits {own.sum() / 800:.1f} of {len(tris)} triangles per point")
    assert own.sum() < 800 * 16                                         # ... and it prunes


O, X, Y, Z = [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]
TETRA = [O + Y + X, O + X + Z, O + Z + Y, X + Y + Z]                      # outward
HAND = TETRA + [[5, 5, 5, 6, 6, 6, 7, 7, 7], [9, 9, 9, 9, 9, 9, 9, 9, 9]]  # + zero area: collinear, one point


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_checker_on_the_unit_tetrahedron_and_degenerate_triangles(dt):
    tris = np.array(HAND, dt)
    rev = tris.reshape(-1, 3, 3)[:, ::-1].reshape(-1, 9).copy()
    one = lambda t, pt, axis: (lambda r: (int(r.crossings[0]), int(r.winding[0])))(pcc.brute_force(t, np.array([pt], dt), axis))
    for axis in (0, 1, 2):
        assert one(tris, [0.1, 0.1, 0.1], axis) == (1, 1)
        assert one(rev, [0.1, 0.1, 0.1], axis) == (1, -1)
    assert one(tris, [-1, .25, .25], 0) == (2, 0)
    assert one(tris, [-1, 0, 0], 0) == (0, 0)          # along an edge
    assert one(tris, [-1, .5, .5], 0) == (0, 0)        # through a silhouette edge
    assert one(tris, [-1, 0, .5], 0) == (0, 0)         # in a face's plane
    for bad in ([np.nan, .1, .1], [.1, np.nan, .1], [.1, .1, np.nan], [np.inf, .1, .1], [.1, np.inf, .1], [.1, .1, np.inf]):
        for axis in (0, 1, 2):
            assert one(tris, bad, axis) == (0, 0), (bad, axis)
    # every outside point: even crossings, winding 0; every inside point: one crossing; the zero-area triangles never count
    rng = np.random.default_rng(5)
    p = (rng.random((400, 3)) * 1.25 - 0.25).astype(dt)
    p = np.concatenate([p, np.array([[5.5, 5.5, 5.5], [6, 6, 6], [4, 5.5, 5.5], [9, 9, 9], [8, 9, 9], [9, 8, 9], [9, 9, 8]], dt)])
    margin = np.minimum(np.abs(p).min(axis=1), np.abs(p.sum(axis=1) - 1))
    inside = (p > 0).all(axis=1) & (p.sum(axis=1) < 1)
    keep = margin > 1e-3
    assert inside[keep].sum() >= 20 and (~inside[keep]).sum() >= 300
    for axis in (0, 1, 2):
        hit, _ = pcc.evaluate(tris, p, axis)
        assert not hit[:, 4:].any()
        bf = pcc.brute_force(tris, p, axis, idt=np.int64)
        assert bf.crossings.dtype == np.int64 and (bf.crossings == pcc.brute_force(tris[:4], p, axis).crossings).all()
        assert (bf.crossings[keep & ~inside] % 2 == 0).all() and (bf.winding[keep & ~inside] == 0).all()
        assert (bf.crossings[keep & inside] == 1).all() and (bf.winding[keep & inside] == 1).all()
        assert (pcc.brute_force(rev, p, axis).winding[keep & inside] == -1).all()
