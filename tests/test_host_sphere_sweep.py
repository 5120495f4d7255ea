"""ibvh_sweep_spheres on the host side: the header declares it (additive under ABI version 7) and carries its contract, the
ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its one
launch goes through the profiling wrapper, the shared walk, the shared start-position and face tests and the slab test that
now exists once, and the entry point validates its arguments — the mode, the combination of outputs and the refused type
combinations included — before any launch.  The numpy checker the GPU test pins the kernel to (tests/sphere_sweep_checker.py):
at the time it reports the sphere is at distance r from the mesh and not before, the computed entry of a grown box never
exceeds that of a grown box it contains and an admitted one has admitted enclosing boxes (what makes pruning lossless), it is
exact on an analytic case, it agrees with the contact list about who touches at the start, and the GPU test's non-vacuity
conditions hold for the brute force alone.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib
from implicitbvh_amd.synthetic import torus_mesh

import closest_point_checker as cpc
import mesh_query_kit as kit
import ray_cast_checker as rcc
import sphere_contacts_checker as scc
import sphere_sweep_checker as ssc
from mesh_query_kit import MESHES

NAME = "ibvh_sweep_spheres"
UNIT = "ibvh_sweep.hip"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *centers",
                    "const void *displacements", "const void *radii", "int64_t num_spheres", "const void *t_max", "int32_t mode",
                    "void *hit_index", "void *hit_t", "void *hit_point", "void *hit_feature", "void *touched", "void *flag", "void *stream"]
    assert re.search(r"enum\s*\{\s*IBVH_SWEEP_CLOSEST = 0,\s*IBVH_SWEEP_ANY = 1\s*\};", hdr)
    assert (abi.SWEEP_CLOSEST, abi.SWEEP_ANY) == (0, 1)
    flat = " ".join(note.replace("*", " ").split())
    assert NAME + " and IBVH_SWEEP_CLOSEST / IBVH_SWEEP_ANY (additive under 7 likewise: one more entry point)" in flat
    assert flat.count("additive under 7 in the same way") == 4       # (what tests/test_host_ray_cast.py counts)
    # the doc comment carries the contract: the radius, the start, the seven candidates, the clamp, the limit, the results, why
    # seven suffice, why it is lossless, the limits
    doc = raw[raw.index("swept spheres: the first time of contact"):raw.index("ibvh_status " + NAME)]
    doc = re.sub(r"\n \*\s+", " ", doc)        # (the comment's lines joined: a phrase may run over a line end)
    for phrase in ("!(r >= 0)", "no flag bit is raised", "L = min(t_max[i], largest finite flt)", "A NaN or negative limit gives no hit",
                   "r2 = r * r", "dd = dot(d, d)", "the evaluation of ibvh_closest_triangles", "If d2 <= r2", "t_k = 0", "Otherwise, if d2 > r2 (false on NaN",
                   "the bits ibvh_sphere_contacts computes", "n = cross(b - a, c - a)", "len = sqrt(dot(n, n))", "s0 = dot(n, p - a)",
                   "side = s0 >= 0 ? 1 : -1", "o = p - ((side * r) / len) * n", "the exact test of ibvh_rays_resolve_triangles",
                   "det != 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= 0", "point = o + t * d", "(a, b), (b, c), (c, a)",
                   "e = y - x;  m = p - x;  ee = dot(e, e);  me = dot(m, e);  de = dot(d, e);  md = dot(m, d)",
                   "A = ee * dd - de * de;  B = ee * md - de * me;  C = ee * (dot(m, m) - r2) - me * me",
                   "disc = B * B - A * C;  t = (-B - sqrt(disc)) / A;  s = me + t * de",
                   "A > 0 && disc >= 0 && t >= 0 && s >= 0 && s <= ee", "point = x + (s / ee) * e",
                   "B = dot(m, d);  C = dot(m, m) - r2;  disc = B * B - dd * C;  t = (-B - sqrt(disc)) / dd",
                   "dd > 0 && disc >= 0 && t >= 0", "point = x", "AMONG EQUAL t THE FIRST CANDIDATE", "face, ab, bc, ca, a, b, c",
                   "strictly smaller", "0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 face",
                   "a prism", "three cylinders", "three spheres", "side walls lie", "inside the cylinders",
                   "[lo_j - r, up_j + r]", "t*_k = max(t_k, entry(grown leaf box of k))", "entry > t_k ? entry : t_k",
                   "the slab test of ibvh_cast_rays", "skin included", "t*_k <= L", "inclusive", "LEXICOGRAPHIC MINIMUM of (t*_k, k)",
                   "SMALLER INDEX", "1 iff a", "lossless WITHOUT an epsilon", "monotone", "contains the grown box of everything below it",
                   "word for word", "admitted box has admitted ancestors", "t*_k >= entry(grown leaf_k) >= entry(every grown ancestor)",
                   "entry > limit()", "strictly", "-Inf on the first hit", "d == 0", "is anything", "zero area", "no face candidate",
                   "hit_t == 0 names a triangle", "follows the candidate order", "not a geometric statement", "NaN leaf box",
                   "IBVH_ERR_UNSUPPORTED", "IBVH_ERR_INVALID_ARG", "skin margin", "ibvh_refit", "bit 1", "not written",
                   "num_spheres == 0", "No reference counterpart", "ONE launch", "no atomics, no LDS, no scratch buffer",
                   "correctly rounded divide and square root", "every comparison false on NaN"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    assert lib.SIGNATURES[NAME] == want == abi.SWEEP_SPHERES_ARGTYPES
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("sweep_spheres", "SphereSweep"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    # the walk (one call per mode), its block size and grid, the prologue, the gather and the flag are the shared ones
    src = kit.query_unit(UNIT, "sweep::sweep_walk_kernel", walks=2, any_mode=True)
    assert "box_bound" not in src and "__shared__" not in src and len(re.findall(r"__global__", src)) == 1
    # three (T, TN) instantiations times two index types times the two modes: the shared four-tag dispatch (query_unit), whose
    # bool the launch turns into the kernel's template parameter; the tie rule is the shared one
    assert "template <class T, class TN, class I, bool ANY>" in src and "constexpr bool ANY = decltype(mt)::value;" in src
    assert "const bool any = mode == " in src and "modes" not in src and "type_traits" not in src
    header = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    assert header.count("return flag ? f(ft, nt, it, std::true_type{}) : f(ft, nt, it, std::false_type{});") == 1
    assert "the any-hit mode of ibvh_cast.hip, ibvh_sweep.hip and ibvh_spherecast.hip" in " ".join(header[:header.index("#pragma once")].replace("//", " ").split())
    # ... applied where a candidate is offered to the answer (csrc/ibvh_firsthit.hpp, pinned by query_unit); the payload is q
    # and the feature
    assert src.count("firsthit::offer<ANY>(answer, ts, index, [&]() {\n                    best_feature = k.feature;") == 1 and "best_index == 0" not in src
    # the bound is the slab entry of the box grown by r, the ONE grown entry; nothing fused, the square root is the library's
    slab = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_slab.hpp")
    assert src.count("slab::grown_entry(lo, up, r, p, d, inv)") == 1 and "glo[" not in src and "slab_entry" not in src
    assert slab.count("const T glo[3] = {lo[0] - r, lo[1] - r, lo[2] - r}, gup[3] = {up[0] + r, up[1] + r, up[2] + r};\n    return slab_entry(glo, gup, p, d, inv);") == 1
    assert "ibvh_sqrt(" in src and "sqrtf" not in src and "fma" not in src
    assert "if ((r >= T(0)) & (L >= T(0))) firsthit::walk<ANY, " in src
    assert "firsthit::outputs_ok(mode, touched, hit_index || hit_t || hit_point || hit_feature)" in src


def test_the_start_the_face_and_the_slab_test_exist_once_and_the_unit_shares_them():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    text = {f: kit.read("implicitbvh.jl_amd", "csrc", f) for f in sources}
    for define, home in ((r"\bclosest_on_triangle\s*\([^)]*\)\s*\{", "ibvh_pointtri.hpp"), (r"\bbool ray_triangle\s*\([^)]*\)\s*\{", "ibvh_raytest.hpp"),
                         (r"\bT slab_entry\s*\([^)]*\)\s*\{", "ibvh_slab.hpp"), (r"\bvoid cross3\s*\(", "ibvh_raytest.hpp")):
        assert [f for f in sources if re.search(define, text[f])] == [home], define
        assert len(re.findall(define, text[home])) == 1
        assert re.search(r'^#include "' + home + '"$', text[UNIT], flags=re.M), home
    src = text[UNIT]
    assert "pointtri::closest_on_triangle(tr.v, p, k.q, region)" in src and "raytri::ray_triangle(tr, o, d, t, u, v)" in src
    assert "tmin" not in src and "1) / det" not in src and "region = " not in src
    # the ray cast took the slab test from the same header, and computes with it as before
    cast = text["ibvh_cast.hip"]
    assert re.search(r'^#include "ibvh_slab.hpp"$', cast, flags=re.M) and "using slab::slab_entry;" in cast and "tmin" not in cast
    assert cast.count("slab_entry(lo, up, p, d, inv)") == 1 and cast.count("slab_entry(b.lo, b.up, p, d, inv)") == 1
    slab = text["ibvh_slab.hpp"]
    for line in ("const bool still = d[k] == T(0);", "const T t1 = (lo[k] - p[k]) * inv[k], t2 = (up[k] - p[k]) * inv[k];",
                 "const T tnear = t2 < t1 ? t2 : t1, tfar = t2 > t1 ? t2 : t1;", "ok &= !still | ((lo[k] <= p[k]) & (p[k] <= up[k]));",
                 "return (ok & (tmin <= tmax) & (tmax >= T(0))) ? tmin : inf;"):
        assert line in slab, line
    import __graft_entry__ as entry
    assert {os.path.join(csrc, "ibvh_slab.hpp"), os.path.join(csrc, UNIT)} <= set(entry.kernel_sources(kit.ROOT))


def test_julia_wrapper_binds_it_with_the_ctypes_signature_and_the_docs_name_it():
    src = kit.julia_ccall(NAME, "sweep_spheres")
    body = src[src.index("function sweep_spheres("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_SWEEP_ANY : IBVH_SWEEP_CLOSEST" in body and "point_morton_order(centers)" in body
    design = kit.read("DESIGN.md")
    section = design[design.index("Swept spheres"):][:9000]
    for phrase in ("no reference counterpart", "lossless", "clamp", "seven candidates", "VGPRs", "scratch", "kernel_meta.py"):
        assert phrase in section, phrase
    assert len(re.findall(r"^\| `<(?:float|double), (?:float|double), (?:int|long), (?:false|true)>` \|", section, flags=re.M)) == 12
    assert kit.read("tools", "bench_sweep.py") and "bench_sweep.py" in kit.read("tools", "README.md")


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    ok = dict(bvh=_fake_bvh(), tris=p, nt=5, c=p, d=p, r=p, ns=0, tmax=None, mode=abi.SWEEP_CLOSEST, index=p, t=None, q=None, g=None,
              touched=None, flag=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["c"], a["d"], a["r"], a["ns"], a["tmax"], a["mode"], a["index"], a["t"], a["q"], a["g"],
                 a["touched"], a["flag"], a["stream"])
    # the two modes and which outputs each takes: closest any non-empty subset of the four, never `touched`; any that alone
    any_ = kit.check_mode_and_outputs(call, kit.SWEEP_SPHERES, p, "ns", ("index", "t", "q", "g"), "touched")
    assert call(tmax=p) == abi.OK and call(tmax=p, **any_) == abi.OK and call(flag=p) == abi.OK
    for bad in (dict(bvh=None), dict(nt=-1), dict(ns=-1), dict(tris=None), dict(ns=5, c=None), dict(ns=5, d=None), dict(ns=5, r=None),
                dict(bvh=_fake_bvh(leaves=None)), dict(bvh=_fake_bvh(nodes=None)), dict(bvh=_fake_bvh(built_level=0)),
                dict(bvh=_fake_bvh(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG and call(**dict(any_, **bad)) == abi.ERR_INVALID_ARG, bad
    assert call(tris=None, nt=0) == abi.OK and call(c=None, d=None, r=None) == abi.OK
    assert call(bvh=_fake_bvh(n=1, nodes=None)) == abi.OK          # a one-leaf tree has no nodes
    broken = _fake_bvh()
    broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # the accepted types: BBox leaves under BBox nodes of the same or a wider float type, any index type
    for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64)):
        assert call(bvh=_fake_bvh(**good)) == abi.OK and call(bvh=_fake_bvh(**good), **any_) == abi.OK, good
    for bad in (dict(leaf_kind=abi.BSPHERE), dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE), dict(node_kind=abi.BSPHERE),
                dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
        # (with spheres to process too: refused, never launched on the fake pointers)
        for mode in (dict(), any_):
            assert call(bvh=_fake_bvh(**bad), **mode) == abi.ERR_UNSUPPORTED, bad
            assert call(bvh=_fake_bvh(**bad), ns=5, **mode) == abi.ERR_UNSUPPORTED, bad
    # the order of ibvh_cast_rays: the entry's own checks first, the types next, the tree and the pointers last
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE), mode=9) == abi.ERR_INVALID_ARG
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE, leaves=None), tris=None) == abi.ERR_UNSUPPORTED


# ---- the checker --------------------------------------------------------------------------------------------------------
_case = ssc.reference


CASES = [(m, dt) for m in sorted(MESHES) for dt in (np.float32, np.float64)]
IDS = [f"{m}-{np.dtype(dt).name}" for m, dt in CASES]


def _assert_limited(bf, bounded, t_max, dt):
    """ssc.limited(), which the GPU test takes its bounded references from, is the brute force under that limit"""
    lim = ssc.limited(bf, t_max, dt)
    for name in ("index", "t", "point", "feature", "touched"):
        got, exp = getattr(lim, name), getattr(bounded, name)
        assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), name


@pytest.mark.parametrize("mesh,dt", CASES, ids=IDS)
def test_sphere_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh, dt):
    tris, p, d, r, bf = _case(mesh, dt)
    bf1 = ssc.brute_force(tris, p, d, r, t_max=np.ones(len(p), dt))
    nv = ssc.non_vacuity(bf, bf1, d)
    print(f"{mesh} {np.dtype(dt).name}: {nv}")
    ssc.assert_non_vacuous(nv)
    edge = scc.mean_edge(tris)
    assert (r >= dt(0.25 * edge) * dt(0.999)).all() and (r <= dt(3 * edge) * dt(1.001)).all()
    rows = np.arange(800)[ssc.ZERO]
    assert (d[rows, (rows // 10) % 3] == 0).all() and (d[list(ssc.STILL)] == 0).all() and ((d == 0).all(axis=1).sum() == len(ssc.STILL))
    # d == 0: "is anything touching now", both ways
    still = bf.index[list(ssc.STILL)] != 0
    assert still.any() and not still.all() and (bf.t[list(ssc.STILL)][still] == 0).all()
    # what the outputs say about each other
    hit = bf.index != 0
    assert (hit == np.isfinite(bf.t)).all() and (hit == (bf.touched == 1)).all() and (bf.t[hit] >= 0).all()
    assert (bf.point[~hit] == 0).all() and (bf.feature[~hit] == 0).all() and (bf.hits <= bf.found).all() and (bf.feature <= 6).all()
    # the limit only takes hits away, and leaves the ones within it as they were
    keep = bf.t <= 1
    assert (bf1.index[keep] == bf.index[keep]).all() and (bf1.index[~keep] == 0).all() and (bf1.t[keep] == bf.t[keep]).all()
    _assert_limited(bf, bf1, np.ones(len(p), dt), dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_at_the_reported_time_the_sphere_is_at_distance_r_from_the_mesh_and_not_before(dt):
    """On torus40, over the spheres that hit without starting in touch: the float64 distance from p + t d to the mesh is r, and
    at 0.25, 0.5, 0.9 and 0.999 of t nothing touches.  Measured here (x86-64, numpy): the largest |dist - r| is 1.284e-05
    in float32 and 9.909e-15 in float64 (MEASURED_F32, MEASURED_F64 below); asserted at 16 x that, which covers another platform's libm — nothing else varies."""
    tris, p, d, r, bf = _case("torus40", dt)
    moving = (bf.index != 0) & (bf.t > 0)
    assert moving.sum() >= 300
    t64, p64, d64, r64 = tris.astype(np.float64), p[moving].astype(np.float64), d[moving].astype(np.float64), r[moving].astype(np.float64)
    time = bf.t[moving].astype(np.float64)[:, None]
    dist = np.sqrt(cpc.brute_force(t64, p64 + time * d64).d2)
    worst = float(np.abs(dist - r64).max())
    print(f"torus40 {np.dtype(dt).name}: {int(moving.sum())} moving hits, the largest |dist - r| is {worst:.3e}")
    assert worst <= 16 * {np.float32: MEASURED_F32, np.float64: MEASURED_F64}[dt]
    # (limits of every kind, while the case is at hand: the bounded brute force is what ssc.limited() derives)
    mixed = bf.t.copy()
    mixed[0::5], mixed[1::5], mixed[2::5], mixed[3::5] = np.nan, -1, 0, mixed[3::5] * dt(0.5)
    _assert_limited(bf, ssc.brute_force(tris, p, d, r, t_max=mixed), mixed, dt)
    for fraction in (0.25, 0.5, 0.9, 0.999):
        before = np.sqrt(cpc.brute_force(t64, p64 + (fraction * time) * d64).d2)
        assert (before > r64).all(), fraction
    # the reported point lies on the reported triangle, at distance r from the centre, up to the same rounding
    centre = p64 + time * d64
    gap = np.linalg.norm(centre - bf.point[moving].astype(np.float64), axis=1)
    assert np.abs(gap - r64).max() <= 16 * {np.float32: MEASURED_F32, np.float64: MEASURED_F64}[dt] * 4
    q, d2, _ = cpc._evaluate(t64[bf.index[moving] - 1], bf.point[moving].astype(np.float64))
    assert np.sqrt(d2).max() <= 16 * {np.float32: MEASURED_F32, np.float64: MEASURED_F64}[dt] * 4


MEASURED_F32, MEASURED_F64 = 1.284e-05, 9.909e-15


def _nested(dt, n, rng):
    """n random boxes and, around each, a box that contains it (some faces shared: an equal corner is the edge of `contains`)"""
    c, h = rng.random((n, 3)) * 2 - 1, rng.random((n, 3)) * 0.2
    lo, up = (c - h).astype(dt), (c + h).astype(dt)
    grow_lo, grow_up = rng.random((n, 3)) * 0.3 * (rng.random((n, 3)) < 0.7), rng.random((n, 3)) * 0.3 * (rng.random((n, 3)) < 0.7)
    return lo, up, (lo - grow_lo.astype(dt)).astype(dt), (up + grow_up.astype(dt)).astype(dt)


@pytest.mark.parametrize("mesh,dt", CASES, ids=IDS)
def test_entry_of_a_grown_box_never_exceeds_the_entry_of_a_grown_box_it_contains(mesh, dt):
    """what the walk prunes with: entry(grown outer) <= entry(grown inner), admitted(grown inner) => admitted(grown outer) — on
    the merges of neighbouring leaf boxes (a node), on merges of merges, on a skin margin and on random nested boxes, for
    radii 0, small and large; zero direction components included.  And every triangle that steps 2 or 3 of the definition
    give a t_k has its grown leaf box admitted."""
    tris, p, d, r, bf = _case(mesh, dt)
    lo, up = rcc.triangle_boxes(tris)
    P, D = p[:200, None, :], d[:200, None, :]
    assert (D[..., 0] == 0).any() and (D[..., 1] == 0).any() and (D[..., 2] == 0).any() and (D == 0).all(axis=-1).any()
    rng = np.random.default_rng(43)
    ilo, iup, olo, oup = _nested(dt, 4000, rng)
    assert (olo <= ilo).all() and (oup >= iup).all() and (olo == ilo).any() and (olo < ilo).any()
    edge = scc.mean_edge(tris)
    for what, radii in (("r = 0", np.zeros(200, dt)), ("small", np.full(200, 1e-3 * edge, dt)), ("the spheres' own", r[:200]),
                        ("large", np.full(200, 40 * edge, dt))):
        R = lambda boxes: np.broadcast_to(radii[:, None], (200, boxes))

        def entry(blo, bup):
            return rcc.slab_entry(*ssc.grown(blo[None], bup[None], R(len(blo))), P, D)

        def check(outer, inner, inner_ok, why):
            e, ok = outer
            assert (ok | ~inner_ok).all(), (what, why)
            assert (e <= inner).all(), (what, why)        # (+Inf = not admitted: nothing to be below)
        own, own_ok = entry(lo, up)
        s = dt(0.01)
        check(entry(lo - s, up + s), own, own_ok, "skin")
        lo2, up2 = np.minimum(lo[0::2], lo[1::2]), np.maximum(up[0::2], up[1::2])
        e2, ok2 = entry(lo2, up2)
        check((e2, ok2), own[:, 0::2], own_ok[:, 0::2], "pair merge, first child")
        check((e2, ok2), own[:, 1::2], own_ok[:, 1::2], "pair merge, second child")
        lo4, up4 = np.minimum(lo2[0::2], lo2[1::2]), np.maximum(up2[0::2], up2[1::2])
        check(entry(lo4, up4), e2[:, 0::2], ok2[:, 0::2], "merge of merges, first child")
        check(entry(lo4, up4), e2[:, 1::2], ok2[:, 1::2], "merge of merges, second child")
        inner, inner_ok = entry(ilo, iup)
        assert inner_ok.sum() >= 1000
        check(entry(olo, oup), inner, inner_ok, "random nested boxes")
        if what == "the spheres' own":
            print(f"{mesh} {np.dtype(dt).name}: the slab test admits {own_ok.sum() / 200:.1f} of {len(tris)} grown leaf boxes per sphere")
            assert own_ok.sum() < 200 * len(tris) / 4               # ... and it prunes
            # steps 2 and 3 against step 4: whoever has a t_k is inside what the walk would have to enter
            tk, _, _, has = ssc.first_touch(tris[None], P, D, radii[:, None])
            assert has.sum() >= 2000 and (own_ok | ~has).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_checker_is_exact_on_an_analytic_case(dt):
    """spheres moving along an axis onto the face, an edge and a corner of an axis-aligned square, at distances that are powers
    of two (the sphere that passes the corner at (-3, ., .) with r = 5 touches it after 4: a 3-4-5 triangle): everything is
    exact in either dtype.  A sphere that lands exactly on the corner reports the first edge that ends there (the candidate
    order), the one that passes it obliquely the vertex; both are found in both triangles at the same time: the smaller index."""
    sq = ssc.square(dt)
    p, d, r = np.array(ssc.SQUARE_P, dt), np.array(ssc.SQUARE_D, dt), np.array(ssc.SQUARE_R, dt)
    bf = ssc.brute_force(sq, p, d, r, idt=np.int32)
    assert bf.index.tolist() == ssc.SQUARE_INDEX and bf.index.dtype == np.int32
    assert bf.t.tolist() == ssc.SQUARE_T and bf.feature.tolist() == ssc.SQUARE_FEATURE and bf.point.tolist() == ssc.SQUARE_POINT
    assert bf.tied.tolist() == ssc.SQUARE_TIED and not bf.clamped.any() and bf.touched.tolist() == [int(i != 0) for i in ssc.SQUARE_INDEX]
    assert bf.feature.dtype == np.uint8 and bf.touched.dtype == np.uint8
    # the limit: inclusive, per sphere; NaN, negative and zero limits (zero keeps who touches at the start)
    lim = np.array([2, 0.25, 0.5, 3, np.nan, -1, 9, 9, 0, -0.0, 0], dt)
    b2 = ssc.brute_force(sq, p, d, r, t_max=lim)
    assert b2.index.tolist() == [2, 0, 0, 1, 0, 0, 0, 0, 2, 1, 0] and b2.touched.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0]
    assert b2.t.tolist() == [2, np.inf, np.inf, 3, np.inf, np.inf, np.inf, np.inf, 0, 0, np.inf]
    just = ssc.brute_force(sq, p, d, r, t_max=np.nextafter(np.array(ssc.SQUARE_T, dt), dt(-np.inf)))
    assert just.index.tolist() == [0] * 11
    # a NaN radius, a negative radius: nothing; radius 0: the centre's own ray, and a centre ON the square touches it
    for bad in (np.nan, -1.0, -np.inf):
        assert ssc.brute_force(sq, p, d, np.full(11, bad, dt)).index.tolist() == [0] * 11, bad
    zero = ssc.brute_force(sq, p, d, np.zeros(11, dt))
    assert zero.index.tolist() == [2, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0] and zero.t.tolist()[:5] == [3, 0.75, 2, 4, 4]   # (in the plane: the edge, disc == 0)
    on = ssc.brute_force(sq, np.array([[1, 2, 2], [3, 1, 2]], dt), np.zeros((2, 3), dt), np.zeros(2, dt))
    assert on.index.tolist() == [2, 1] and on.t.tolist() == [0, 0] and on.feature.tolist() == [6, 6]
    # a zero-area triangle has no face candidate: its edges and vertices answer
    flat = np.array([[0, 0, 2, 4, 0, 2, 2, 0, 2]], dt)
    thin = ssc.brute_force(flat, np.array([[1, -4, 2], [1, 0, 6]], dt), np.array([[0, 1, 0], [0, 0, -1]], dt), np.ones(2, dt))
    assert thin.index.tolist() == [1, 1] and thin.t.tolist() == [3, 3] and thin.feature.tolist() == [2, 2] and thin.point.tolist() == [[1, 0, 2]] * 2
    # a NaN vertex: that triangle is never hit, the other one still is (at 3 - sqrt(1/2) = 2.29)
    broken = sq.copy()
    broken[1, 4] = np.nan
    rest = ssc.brute_force(broken, p, d, r, boxes=rcc.triangle_boxes(sq))
    assert (rest.index != 2).all() and rest.index[:6].tolist() == [1, 1, 1, 1, 1, 1] and rest.feature[:3].tolist() == [4, 4, 6]
    assert 2.25 < rest.t[0] < 2.5 and rest.t[2] == 1                                 # (later, on the diagonal edge of the other)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_clamp_is_active_on_an_axis_aligned_floor(dt):
    tris, p, d, r = ssc.floor_case(dt)
    bf = ssc.brute_force(tris, p, d, r)
    print(f"floor {np.dtype(dt).name}: {int((bf.index != 0).sum())} of {len(p)} spheres hit, the clamp is active on {int(bf.clamped.sum())}")
    assert (bf.index != 0).all() and bf.clamped.sum() >= 10 and (~bf.clamped).sum() >= 10
    # there t* is the grown box's entry, above the face candidate's t by rounding only
    tk, _, _, has = ssc.first_touch(tris[bf.index - 1], p, d, r)
    assert has.all() and (bf.t >= tk).all() and ((bf.t > tk) == bf.clamped).all() and (bf.t - tk <= 8 * np.finfo(dt).eps * tk).all()


@pytest.mark.parametrize("mesh,dt", CASES, ids=IDS)
def test_touching_at_the_start_agrees_with_the_contact_list(mesh, dt):
    """the spheres with t == 0 are the spheres with a non-empty ibvh_sphere_contacts list for the same radii, and the triangle
    named is the first of that list in index order"""
    tris, p, d, r, bf = _case(mesh, dt)
    contacts = scc.brute_force(tris, p, r, idt=np.int64)
    touching = contacts.counts > 0
    assert ((bf.t == 0) == touching).all() and 80 <= touching.sum() <= 720
    first = contacts.index[contacts.offsets[:-1][touching]]
    assert (bf.index[touching] == first).all()
    assert bf.point[touching].tobytes() == contacts.point[contacts.offsets[:-1][touching]].tobytes()
    assert (bf.feature[touching] == contacts.region[contacts.offsets[:-1][touching]]).all()
