"""ibvh_closest_triangles on the host side: the header declares it (additive under ABI version 7) and carries its contract, the
ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its one
launch goes through the profiling wrapper, and the entry point validates its arguments — the refused type combinations
included — before any launch.  The numpy checker the GPU test pins the kernel to (tests/closest_point_checker.py) agrees
with its own float64 run, its point-box bound never exceeds a distance, and the GPU test's non-vacuity conditions hold for
the brute force alone.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib
from implicitbvh_amd.synthetic import torus_mesh

import closest_point_checker as cpc
import mesh_query_kit as kit
from mesh_query_kit import MESHES

NAME = "ibvh_closest_triangles"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *points", "int64_t num_points",
                    "const void *max_distance2", "void *closest_index", "void *closest_d2", "void *closest_point", "void *flag",
                    "void *stream"]
    assert NAME in note and note.count("additive") >= 2
    # the doc comment carries the contract: arithmetic, tie rule, the clamp and why, accepted types, guards, miss values
    doc = raw[raw.index("closest point on the mesh for a batch of query points"):raw.index("ibvh_status " + NAME)]
    for phrase in ("(x0*y0 + x1*y1) + x2*y2", "vc = d1*d4 - d3*d2", "d3 >= 0 && d4 <= d3", "w = (d4-d3) / ((d4-d3) + (d5-d6))",
                   "den = 1 / ((va + vb) + vc)", "q = q < lo ? lo : (q > up ? up : q)", "LEXICOGRAPHIC MINIMUM", "SMALLER INDEX",
                   "false on NaN", "Why the clamp", "lb > best", "IBVH_ERR_UNSUPPORTED", "skin margin", "ibvh_refit", "bit 1",
                   "0 = no triangle", "+Inf = none", "HOST pointer", "num_points == 0"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    assert lib.SIGNATURES[NAME] == want
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("closest_points", "ClosestPoints"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    src = kit.query_unit("ibvh_closest.hip", "closest::closest_walk_kernel")
    assert "pointwalk::hopeless(p, max_d2)" in src and "pointwalk::radius_or_inf<T>(max_distance2)" in src
    assert src.count("if (pointwalk::wins(d2, index, best, best_index)) {") == 1 and "best_index == 0" not in src   # the shared tie rule
    # raise_flag is shared with the ray resolve, defined once
    assert "void raise_flag(" in kit.read("implicitbvh.jl_amd", "csrc", "ibvh_common.hpp")
    assert "void raise_flag(" not in kit.read("implicitbvh.jl_amd", "csrc", "ibvh_raytri.hip")


def test_julia_wrapper_binds_it_with_the_ctypes_signature():
    kit.julia_ccall(NAME, "closest_points")
    design = kit.read("DESIGN.md")
    assert "no reference counterpart" in design[design.index("Closest point on the mesh"):][:3000]


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    radius = C.byref(C.c_float(1.0))
    ok = dict(bvh=_fake_bvh(), tris=p, nt=5, pts=p, np_=0, r2=radius, ci=p, cd=None, cq=None, flag=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["pts"], a["np_"], a["r2"], a["ci"], a["cd"], a["cq"], a["flag"], a["stream"])
    assert call() == abi.OK                                        # num_points = 0: nothing to do
    assert call(r2=None) == abi.OK                                 # NULL radius = +Inf
    assert call(ci=None) == abi.ERR_INVALID_ARG                    # no output requested
    assert call(ci=None, cd=p) == abi.OK and call(ci=None, cq=p) == abi.OK   # ... any one output will do
    for bad in (dict(bvh=None), dict(nt=-1), dict(np_=-1), dict(tris=None), dict(np_=5, pts=None), dict(bvh=_fake_bvh(leaves=None)),
                dict(bvh=_fake_bvh(nodes=None)), dict(bvh=_fake_bvh(built_level=0)), dict(bvh=_fake_bvh(built_level=5))):
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
def test_checker_float32_distances_agree_with_its_float64_run():
    tris = torus_mesh(40, 40)
    p = cpc.query_points(tris, np.float32)
    b32 = cpc.brute_force(tris, p)
    b64 = cpc.brute_force(tris.astype(np.float64), p.astype(np.float64))
    dist32, dist64 = np.sqrt(b32.d2.astype(np.float64)), np.sqrt(b64.d2)
    eps32 = float(np.finfo(np.float32).eps)
    bound = 16 * eps32 * (np.abs(tris).max() + dist64)
    dev = np.abs(dist32 - dist64)
    print(f"largest |dist32 - dist64| = {dev.max():.3e}, smallest bound = {bound.min():.3e}")
    assert (dev <= bound).all()
    # and the closest point is a point of the winning triangle's plane patch: inside its box, at that distance
    lo, up = cpc.triangle_boxes(tris)
    k = b32.index - 1
    assert (b32.point >= lo[k]).all() and (b32.point <= up[k]).all()
    e = p - b32.point
    assert ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).tobytes() == b32.d2.tobytes()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_box_lower_bound_never_exceeds_a_distance_and_the_clamp_changes_nothing(dt):
    tris = torus_mesh(40, 40).astype(dt)
    p = cpc.query_points(tris, dt)
    q, d2, region = cpc.evaluate(tris, p)
    lo, up = cpc.triangle_boxes(tris)
    lb = cpc.box_lower_bound(lo[None], up[None], p[:, None, :])
    assert lb.shape == d2.shape == (800, 3200) and lb.dtype == dt
    assert (lb <= d2).all()
    # ... and of an enclosing box (a skin margin; the union of neighbouring boxes = a node)
    s = dt(0.01)
    assert (cpc.box_lower_bound((lo - s)[None], (up + s)[None], p[:, None, :]) <= d2).all()
    lo2, up2 = np.minimum(lo[0::2], lo[1::2]), np.maximum(up[0::2], up[1::2])
    lb2 = cpc.box_lower_bound(lo2[None], up2[None], p[:, None, :])
    assert (lb2 <= d2[:, 0::2]).all() and (lb2 <= d2[:, 1::2]).all()
    assert (q >= lo[None]).all() and (q <= up[None]).all()
    assert set(np.unique(region).tolist()) == set(range(7))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_point_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh, dt):
    tris = torus_mesh(*MESHES[mesh]).astype(dt)
    p = cpc.query_points(tris, dt)
    assert p.shape == (800, 3) and p.dtype == dt
    bf = cpc.brute_force(tris, p)
    face, edges, vertices = cpc.region_counts(bf.region)
    tied, zero = int((bf.ties >= 2).sum()), int((bf.d2 == 0).sum())
    print(f"{mesh} {np.dtype(dt).name}: winners face {face} edges {edges} vertices {vertices}, {tied} tied points, {zero} zero distances")
    assert (bf.index > 0).all() and face + edges + vertices == 800
    assert min(face, edges, vertices) >= 50 and tied >= 100 and zero >= 20


def test_checker_regions_degenerate_triangles_nan_and_the_tie_rule():
    f = np.float32
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f)
    pts = np.array([[-1, -1, 1], [2, -0.5, 1], [0.5, -1, 1], [-0.5, 2, 1], [-1, 0.5, 1], [1, 1, 1], [0.25, 0.25, 1]], f)
    q, d2, region = cpc.evaluate(tri, pts)
    assert region[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert q[:, 0].tolist() == [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]]
    assert d2[:, 0].tolist() == [3, 2.25, 2, 2.25, 2, 1.5, 1]
    # a duplicate loses to the smaller index; a NaN vertex never wins; zero-area triangles give finite answers
    tris = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0.5, np.nan, 0, 0.5, 0, 1, 0.5],
                     [5, 5, 5, 6, 6, 6, 7, 7, 7], [9, 9, 9, 9, 9, 9, 9, 9, 9]], f)
    pts = np.array([[0.25, 0.25, 1], [5.5, 5.5, 5.5], [9, 9, 10], [np.nan, 0, 0]], f)
    bf = cpc.brute_force(tris, pts, idt=np.int64)
    assert bf.index.tolist() == [1, 4, 5, 0] and bf.index.dtype == np.int64 and bf.ties.tolist() == [2, 1, 1, 0]
    assert bf.d2.tolist()[:3] == [1, 0, 1] and np.isposinf(bf.d2[3]) and (bf.point[3] == 0).all() and not np.isnan(bf.point).any()
    _, d2, _ = cpc.evaluate(tris, pts)
    assert np.isnan(d2[:, 2]).all() and np.isnan(d2[3]).all()
    # a bounded search keeps d2 <= max_d2, the bound itself included
    assert cpc.brute_force(tris, pts, max_d2=f(1)).index.tolist() == [1, 4, 5, 0]
    assert cpc.brute_force(tris, pts, max_d2=f(0.999)).index.tolist() == [0, 4, 0, 0]
    assert cpc.brute_force(tris, pts, max_d2=f(np.nan)).index.tolist() == [0, 0, 0, 0]
