"""ibvh_rays_resolve_triangles on the host side: the header declares it (additive under ABI version 7), the ctypes table and
the Julia extension bind it with the same argument kinds, the entry point validates its arguments before any launch, and the
numpy checker the GPU test pins the kernel to (tests/ray_triangle_checker.py) agrees with an independent float64 solve and
keeps the tie rule.  The GPU test's non-vacuity conditions on its ray sets are checked here by brute force.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib
from implicitbvh_amd.synthetic import random_rays, torus_mesh

import ray_triangle_checker as rtc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibvh_rays_resolve_triangles"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_point_under_abi_version_7():
    raw = _read("include", "ibvh.h")
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"ibvh_status\s+" + NAME + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/ibvh.h declares " + NAME
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["int32_t flt", "int32_t index_type", "const void *triangles", "int64_t num_triangles", "const void *points",
                    "const void *directions", "int64_t num_rays", "const void *counts", "const void *contacts", "int64_t capacity",
                    "void *closest_index", "void *closest_t", "void *closest_uv", "void *cand_t", "void *flag", "void *stream"]
    assert int(re.search(r"#define IBVH_ABI_VERSION (\d+)", hdr).group(1)) == 7 == abi.ABI_VERSION
    assert lib.load().ibvh_abi_version() == 7
    note = raw[raw.index("Bumped whenever"):raw.index("#define IBVH_ABI_VERSION")]
    assert NAME in note and "additive" in note
    # the doc comment carries the contract: arithmetic, tie rule, guards, conservativeness
    doc = raw[raw.index("Resolve the (leaf.index, iray) list"):raw.index("ibvh_status " + NAME)]
    for phrase in ("pv = d x e2", "inv = 1 / det", "(x0*y0 + x1*y1) + x2*y2", "EARLIER in the list", "-0 == +0", "bit 0", "bit 1",
                   "not watertight", "Exact ON THE LIST IT IS GIVEN", "BFS", "IBVH_OUTPUT_POSITIONS"):
        assert phrase in doc, phrase


def test_binding_table_and_python_surface():
    ct = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    want = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    assert lib.SIGNATURES[NAME] == want
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("resolve_triangles", "raycast", "RayHits"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    mk = _read("implicitbvh.jl_amd", "csrc", "Makefile")
    assert "ibvh_raytri.hip" in mk[mk.index("SRCS"):mk.index("OBJS")]
    src = _read("implicitbvh.jl_amd", "csrc", "ibvh_raytri.hip")
    assert re.search(r"IBVH_LAUNCH\(\(raytri::raytri_resolve_kernel<", src), "launched through the profiling wrapper"


def test_julia_wrapper_binds_it_with_the_ctypes_signature():
    src = _read("implicitbvh.jl_amd", "julia", "ImplicitBVHlibibvhExt.jl")
    m = re.search(r"\n(c_\w+)\([^)]*\) =\n\s*ccall\(\(:" + NAME + r", libibvh\), Cint,\s*\(([^)]*)\)", src)
    assert m, "one ccall wrapper binds " + NAME
    jl = {"Ptr{Cvoid}": C.c_void_p, "Int64": C.c_int64, "Int32": C.c_int32}  # only what the static signature test's map knows
    assert [jl[a.strip()] for a in m.group(2).split(",")] == lib.SIGNATURES[NAME]
    assert m.group(1) + "(" in src[src.index("function resolve_triangles("):]
    assert "function ImplicitBVH.resolve_triangles" not in src and "ImplicitBVH.raycast" not in src
    assert NAME in _read("INTEGRATION.md")


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    ok = dict(flt=abi.F32, idx=abi.I32, tris=p, nt=4, pts=p, dirs=p, nr=0, counts=p, contacts=p, cap=8, ci=p, ct=None, cuv=None,
              cand=None, flag=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["flt"], a["idx"], a["tris"], a["nt"], a["pts"], a["dirs"], a["nr"], a["counts"], a["contacts"], a["cap"], a["ci"],
                 a["ct"], a["cuv"], a["cand"], a["flag"], a["stream"])
    assert call() == abi.OK                                     # num_rays = 0: nothing to do
    assert call(ci=None) == abi.ERR_INVALID_ARG                 # no output requested
    assert call(ci=None, cand=p) == abi.OK                      # ... any one output will do
    for bad in (dict(nt=-1), dict(nr=-1), dict(cap=-1), dict(tris=None), dict(contacts=None),
                dict(nr=5, pts=None), dict(nr=5, dirs=None), dict(nr=5, counts=None)):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
    assert call(tris=None, nt=0) == abi.OK and call(contacts=None, cap=0) == abi.OK
    for bad in (dict(flt=2), dict(flt=-1), dict(idx=2), dict(idx=-1)):
        assert call(**bad) == abi.ERR_UNSUPPORTED, bad


# ---- the checker --------------------------------------------------------------------------------------------------------
MESHES = {"torus40": (40, 40), "torus64x63": (64, 63)}


def _ray_sets(tris, n):
    lo, hi = rtc.mesh_box(tris)
    return {"random": random_rays(n, lo, hi, seed=5), "aimed": rtc.aimed_rays(n, tris)}


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_ray_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh):
    """At least 50 % of the random and 99 % of the aimed rays have an exact hit (brute force over all triangles), no natural ties."""
    tris = torus_mesh(*MESHES[mesh])
    for name, (p, d) in _ray_sets(tris, 2000).items():
        hit, t, u, v = rtc.ray_triangle(tris[None], p[:400, None, :], d[:400, None, :])
        bf = rtc.brute_force(tris, p, d)
        share = float((bf.index > 0).mean())
        print(f"{mesh} {name}: {share:.3f} of 2000 rays hit")
        assert share >= (0.5 if name == "random" else 0.99), (mesh, name, share)
        # no two exact hits of one ray share their t (a tie would make the test depend on the list order alone)
        tt = np.where(hit, t, np.nan)
        tt.sort(axis=1)
        assert not (np.diff(tt, axis=1) == 0).any()
        assert bf.t.dtype == np.float32 and bf.uv.dtype == np.float32


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_checker_agrees_with_a_float64_solve_on_well_conditioned_pairs(dtype):
    tris = torus_mesh(24, 24)
    for name, (p, d) in _ray_sets(tris, 300).items():
        hit64, margin = rtc.solve_float64(tris, p, d)
        hit, t, u, v = rtc.ray_triangle(tris.astype(dtype)[None], p.astype(dtype)[:, None, :], d.astype(dtype)[:, None, :])
        clear = margin > 1e-3
        assert clear.mean() > 0.9 and hit64[clear].sum() > (100 if name == "aimed" else 30)
        assert (hit[clear] == hit64[clear]).all(), name
        # and t, u, v are the float64 solution to the precision of the dtype
        tri64 = tris.astype(np.float64)
        r, k = np.nonzero(hit & clear)
        x = p.astype(np.float64)[r] + t[r, k][:, None].astype(np.float64) * d.astype(np.float64)[r]
        a, b, c = tri64[k, 0:3], tri64[k, 3:6], tri64[k, 6:9]
        y = a + u[r, k][:, None] * (b - a) + v[r, k][:, None] * (c - a)
        assert np.abs(x - y).max() < (2e-3 if dtype == np.float32 else 1e-9)


def _one_list(tris, p, d, order):
    """every triangle a candidate of every ray, in `order`"""
    nr, n = len(p), len(order)
    contacts = np.stack([np.tile(np.asarray(order, np.int32), nr), np.repeat(np.arange(1, nr + 1, dtype=np.int32), n)], axis=1)
    counts = (np.arange(1, nr + 1) * n).astype(np.int32)
    return counts, contacts


def test_checker_edge_cases_and_the_tie_rule():
    f = np.float32
    t0 = [0, 0, 1, 1, 0, 1, 0, 1, 1]
    tris = np.array([t0,                                  # 1
                     [0, 0, 2, 1, 0, 2, 0, 1, 2],         # 2: behind triangle 1 as seen from z = 0
                     t0,                                  # 3: a duplicate of 1
                     [0, 0, 1, 1, 1, 1, 2, 2, 1],         # 4: zero area
                     [0, 0, -1, 1, 0, -1, 0, 1, -1]], f)  # 5: behind the origin
    p = np.array([[0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 1], [5, 5, 0], [np.nan, 0.25, 0], [0.25, 0.25, 0]], f)
    d = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, np.nan]], f)
    for order, first in (([1, 2, 3, 4, 5], 1), ([3, 2, 1, 4, 5], 3), ([5, 4, 2, 3, 1], 3)):
        counts, contacts = _one_list(tris, p, d, order)
        r = rtc.resolve(counts, contacts, tris, p, d)
        assert r.index.tolist() == [first, 5, 0, 0, 0, 0]   # equal t: the earlier list entry; backwards: only what lies ahead
        assert r.t[:2].tolist() == [1.0, 1.0] and np.isinf(r.t[2:]).all() and (r.uv[2:] == 0).all()
        assert r.uv[0].tolist() == [0.25, 0.25]
        acc = r.accepted.reshape(len(p), -1)
        assert acc[0].sum() == 3 and acc[2].sum() == 0            # ray 3 lies IN the plane of triangle 1: parallel, a miss
        assert not acc[:, list(order).index(4)].any()             # zero area: det == 0
        assert not acc[4].any() and not acc[5].any()              # NaN rays
        assert np.isinf(r.candidate_t[~r.accepted]).all() and (r.candidate_t[r.accepted] >= 0).all()
    # -0 == +0 is a tie: the earlier entry wins and its bits are kept
    tz = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 0, 1, 0, 0]], f)   # the same triangle, wound both ways
    pz, dz = np.array([[0.25, 0.25, 0]], f), np.array([[0, 0, 1]], f)               # a ray that starts ON it
    hit, t, u, v = rtc.ray_triangle(tz, pz, dz)
    assert hit.all() and (t == 0).all() and np.signbit(t[0]) != np.signbit(t[1])
    for order in ([1, 2], [2, 1]):
        counts, contacts = _one_list(tz, pz, dz, order)
        r = rtc.resolve(counts, contacts, tz, pz, dz)
        assert r.index[0] == order[0] and np.signbit(r.t[0]) == np.signbit(t[order[0] - 1])
    # an index outside 1..n is a miss and is reported; rays without candidates give 0 / +Inf
    counts = np.array([2, 2, 3], np.int64)
    contacts = np.array([[9, 1], [1, 1], [0, 3]], np.int64)
    r = rtc.resolve(counts, contacts, tris, p[:3], np.array([[0, 0, 1]] * 3, f))
    assert r.bad.tolist() == [True, False, True] and r.index.tolist() == [1, 0, 0] and np.isinf(r.t[1:]).all()
    assert r.index.dtype == np.int64
    # the brute force is the list of all triangles in index order
    bf = rtc.brute_force(tris, p, d, idt=np.int32)
    counts, contacts = _one_list(tris, p, d, [1, 2, 3, 4, 5])
    r = rtc.resolve(counts, contacts, tris, p, d)
    assert (bf.index == r.index).all() and bf.t.tobytes() == r.t.tobytes() and bf.uv.tobytes() == r.uv.tobytes()
