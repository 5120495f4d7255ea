"""ibvh_cast_rays on the host side: the header declares it (additive under ABI version 7) and carries its contract, the ctypes
table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its one launch
goes through the profiling wrapper, the shared walk and the shared exact test, and the entry point validates its arguments —
the mode, the combination of outputs and the refused type combinations included — before any launch.  The numpy checker the
GPU test pins the kernel to (tests/ray_cast_checker.py): the computed entry of a box never exceeds that of a box it contains
and an admitted box has admitted enclosing boxes (what makes pruning lossless), it agrees with an analytic case, the clamp is
active on an axis-aligned floor, and the GPU test's non-vacuity conditions hold for the brute force alone.  No GPU."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib
from implicitbvh_amd.synthetic import torus_mesh

import mesh_query_kit as kit
import ray_cast_checker as rcc
from mesh_query_kit import MESHES

NAME = "ibvh_cast_rays"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *points", "const void *directions",
                    "int64_t num_rays", "const void *t_max", "int32_t mode", "void *hit_index", "void *hit_t", "void *hit_uv",
                    "void *occluded", "void *flag", "void *stream"]
    assert re.search(r"enum\s*\{\s*IBVH_CAST_CLOSEST = 0,\s*IBVH_CAST_ANY = 1\s*\};", hdr)
    assert (abi.CAST_CLOSEST, abi.CAST_ANY) == (0, 1)
    flat = " ".join(note.replace("*", " ").split())
    assert NAME + " and IBVH_CAST_CLOSEST / IBVH_CAST_ANY (additive under 7 in the same way)" in flat
    assert flat.count("additive under 7 in the same way") == 4 and note.count("additive") >= 5
    # the doc comment carries the contract: the slab test, the exact test, the clamp, the limit, the results, why it is lossless
    doc = raw[raw.index("ray cast: the closest hit, or any hit"):raw.index("ibvh_status " + NAME)]
    for phrase in ("inv_k = 1 / d_k, computed once per ray", "d_k == 0", "lo_k <= p_k && p_k <= up_k", "contributes nothing to tmin / tmax",
                   "0 * Inf is NaN on a box face", "t1 = (lo_k - p_k) * inv_k", "t2 = (up_k - p_k) * inv_k", "tnear = t2 < t1 ? t2 : t1",
                   "tmin = tnear > tmin ? tnear : tmin", "tmin <= tmax && tmax >= 0", "false on", "entry(box) = tmin if admitted, +Inf otherwise",
                   "det != 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= 0", "ibvh_rays_resolve_triangles", "t*_k = max(t_k, entry(leaf box of k))",
                   "skin included", "L = min(t_max[i], largest finite flt)", "never +Inf", "A NaN or negative t_max gives no hit",
                   "t*_k <= L", "inclusive", "LEXICOGRAPHIC MINIMUM of (t*_k, k)", "SMALLER INDEX", "1 iff a hit exists",
                   "lossless WITHOUT an epsilon", "monotone", "admitted box has admitted ancestors",
                   "t*_k >= entry(leaf_k) >= entry(every ancestor)", "entry > limit()", "strictly", "-Inf on the first hit",
                   "Traversal order", "axis-aligned floor", "not watertight along shared edges", "no t_min", "depends on the walk order",
                   "IBVH_ERR_UNSUPPORTED", "IBVH_ERR_INVALID_ARG", "skin margin", "ibvh_refit", "bit 1", "not written", "num_rays == 0",
                   "No reference counterpart", "ONE launch", "no atomics, no LDS, no scratch buffer", "NaN leaf box"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    assert lib.SIGNATURES[NAME] == want == abi.CAST_RAYS_ARGTYPES
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("cast_rays", "RayCast"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    # the walk (one call per mode), its block size and grid, the prologue, the gather and the flag are the shared ones
    src = kit.query_unit("ibvh_cast.hip", "cast::cast_walk_kernel", walks=2, any_mode=True)
    assert "box_bound" not in src
    # the exact test is the shared one: defined once, in the header both translation units include
    shared = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_raytest.hpp")
    resolve = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_raytri.hip")
    define = r"\bbool ray_triangle\s*\("
    assert len(re.findall(define, shared)) == 1 and not re.search(define, src) and not re.search(define, resolve)
    for unit in (src, resolve):
        assert re.search(r'^#include "ibvh_raytest.hpp"$', unit, flags=re.M) and "ray_triangle(tr, p, d, t, u, v)" in unit
        assert "void cross3(" not in unit and "1) / det" not in unit
    # three (T, TN) instantiations times two index types times the two modes: the shared four-tag dispatch (query_unit), whose
    # bool the launch turns into the kernel's template parameter; the tie rule is the shared one
    assert "template <class T, class TN, class I, bool ANY>" in src and "constexpr bool ANY = decltype(mt)::value;" in src
    assert "const bool any = mode == " in src and "modes" not in src and "type_traits" not in src
    header = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    assert header.count("return flag ? f(ft, nt, it, std::true_type{}) : f(ft, nt, it, std::false_type{});") == 1
    assert "the any-hit mode of ibvh_cast.hip, ibvh_sweep.hip and ibvh_spherecast.hip" in " ".join(header[:header.index("#pragma once")].replace("//", " ").split())
    # ... applied where a candidate is offered to the answer (csrc/ibvh_firsthit.hpp, pinned by query_unit); the payload is uv
    assert src.count("firsthit::offer<ANY>(answer, ts, index, [&]() { best_u = u, best_v = v; });") == 1 and "best_index == 0" not in src
    assert "if (L >= T(0)) firsthit::walk<ANY, " in src and "firsthit::outputs_ok(mode, occluded, hit_index || hit_t || hit_uv)" in src


def test_julia_wrapper_binds_it_with_the_ctypes_signature_and_the_docs_name_it():
    kit.julia_ccall(NAME, "cast_rays")
    design = kit.read("DESIGN.md")
    section = design[design.index("Ray cast"):][:8000]
    for phrase in ("no reference counterpart", "lossless", "clamp", "shared edge", "VGPRs", "scratch"):
        assert phrase in section, phrase
    assert kit.read("tools", "bench_cast.py")


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    ok = dict(bvh=_fake_bvh(), tris=p, nt=5, pts=p, dirs=p, nr=0, tmax=None, mode=abi.CAST_CLOSEST, index=p, t=None, uv=None, occ=None,
              flag=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["pts"], a["dirs"], a["nr"], a["tmax"], a["mode"], a["index"], a["t"], a["uv"], a["occ"],
                 a["flag"], a["stream"])
    # the two modes and which outputs each takes: closest any non-empty subset of the three, never `occluded`; any that alone
    any_ = kit.check_mode_and_outputs(call, kit.CAST_RAYS, p, "nr", ("index", "t", "uv"), "occ")
    assert call(tmax=p) == abi.OK and call(tmax=p, **any_) == abi.OK
    for bad in (dict(bvh=None), dict(nt=-1), dict(nr=-1), dict(tris=None), dict(nr=5, pts=None), dict(nr=5, dirs=None),
                dict(bvh=_fake_bvh(leaves=None)), dict(bvh=_fake_bvh(nodes=None)), dict(bvh=_fake_bvh(built_level=0)),
                dict(bvh=_fake_bvh(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG and call(**dict(any_, **bad)) == abi.ERR_INVALID_ARG, bad
    assert call(tris=None, nt=0) == abi.OK
    assert call(bvh=_fake_bvh(n=1, nodes=None)) == abi.OK          # a one-leaf tree has no nodes
    broken = _fake_bvh()
    broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # the accepted types: BBox leaves under BBox nodes of the same or a wider float type, any index type
    for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64)):
        assert call(bvh=_fake_bvh(**good)) == abi.OK and call(bvh=_fake_bvh(**good), **any_) == abi.OK, good
    for bad in (dict(leaf_kind=abi.BSPHERE), dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE), dict(node_kind=abi.BSPHERE),
                dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
        # (with rays to process too: refused, never launched on the fake pointers)
        for mode in (dict(), any_):
            assert call(bvh=_fake_bvh(**bad), **mode) == abi.ERR_UNSUPPORTED, bad
            assert call(bvh=_fake_bvh(**bad), nr=5, **mode) == abi.ERR_UNSUPPORTED, bad


# ---- the checker --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(mesh, dt):
    tris = torus_mesh(*MESHES[mesh]).astype(dt)
    p, d = rcc.rays(tris, dt)
    assert p.shape == d.shape == (800, 3) and p.dtype == d.dtype == dt
    return tris, p, d, rcc.brute_force(tris, p, d)


CASES = [(m, dt) for m in sorted(MESHES) for dt in (np.float32, np.float64)]
IDS = [f"{m}-{np.dtype(dt).name}" for m, dt in CASES]


@pytest.mark.parametrize("mesh,dt", CASES, ids=IDS)
def test_ray_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh, dt):
    tris, p, d, bf = _case(mesh, dt)
    hit, miss, multi, exact, zero, clamped, tied = rcc.non_vacuity(bf, d)
    print(f"{mesh} {np.dtype(dt).name}: {hit} rays hit, {miss} miss, {multi} hitting rays with two or more exact hits, {exact} exact "
          f"hits, {zero} hitting rays with a zero direction component, {clamped} clamped winners, {tied} ties")
    assert hit >= 400 and miss >= 40 and 4 * multi >= hit and zero >= 1
    assert clamped == 0 and tied == 0
    rcc.assert_non_vacuous(bf, d)
    nz = rcc.all_nonzero(d)
    assert nz.sum() == 640 and (d[rcc.ZERO_X, 0] == 0).all() and (d[rcc.ZERO_Y, 1] == 0).all()
    # the rays that start inside a leaf's box enter it at a negative parameter
    lo, up = rcc.triangle_boxes(tris)
    entry, admitted = rcc.slab_entry(lo[None], up[None], p[rcc.INSIDE, None, :], d[rcc.INSIDE, None, :])
    assert ((entry < 0) & admitted).any(axis=1).sum() >= 30
    # what the outputs say about each other
    assert ((bf.index != 0) == np.isfinite(bf.t)).all() and ((bf.index != 0) == (bf.occluded == 1)).all()
    assert (bf.uv[bf.index == 0] == 0).all() and (bf.t[bf.index != 0] >= 0).all() and (bf.hits <= bf.exact).all()


def _nested(dt, n, rng):
    """n random boxes and, around each, a box that contains it (some faces shared: an equal corner is the edge of `contains`)"""
    c, h = rng.random((n, 3)) * 2 - 1, rng.random((n, 3)) * 0.2
    lo, up = (c - h).astype(dt), (c + h).astype(dt)
    grow_lo, grow_up = rng.random((n, 3)) * 0.3 * (rng.random((n, 3)) < 0.7), rng.random((n, 3)) * 0.3 * (rng.random((n, 3)) < 0.7)
    return lo, up, (lo - grow_lo.astype(dt)).astype(dt), (up + grow_up.astype(dt)).astype(dt)


@pytest.mark.parametrize("mesh,dt", CASES, ids=IDS)
def test_entry_of_a_box_never_exceeds_the_entry_of_a_box_it_contains(mesh, dt):
    """what the walk prunes with: entry(outer) <= entry(inner), admitted(inner) => admitted(outer) — on the merges of
    neighbouring leaf boxes (a node), on a skin margin, and on random nested boxes; zero direction components included"""
    tris, p, d, bf = _case(mesh, dt)
    lo, up = rcc.triangle_boxes(tris)
    P, D = p[:200, None, :], d[:200, None, :]
    assert (D[..., 0] == 0).any() and (D[..., 1] == 0).any()
    own, own_ok = rcc.slab_entry(lo[None], up[None], P, D)

    def check(outer_lo, outer_up, inner, inner_ok, what):
        e, ok = rcc.slab_entry(outer_lo, outer_up, P, D)
        assert (ok | ~inner_ok).all(), what
        assert (e <= inner).all(), what          # (+Inf = not admitted: nothing to be below)
    s = dt(0.01)
    check((lo - s)[None], (up + s)[None], own, own_ok, "skin")
    lo2, up2 = np.minimum(lo[0::2], lo[1::2]), np.maximum(up[0::2], up[1::2])
    check(lo2[None], up2[None], own[:, 0::2], own_ok[:, 0::2], "pair merge, first child")
    check(lo2[None], up2[None], own[:, 1::2], own_ok[:, 1::2], "pair merge, second child")
    lo4, up4 = np.minimum(lo2[0::2], lo2[1::2]), np.maximum(up2[0::2], up2[1::2])
    e2, ok2 = rcc.slab_entry(lo2[None], up2[None], P, D)
    check(lo4[None], up4[None], e2[:, 0::2], ok2[:, 0::2], "merge of merges")
    print(f"{mesh} {np.dtype(dt).name}: the slab test admits {own_ok.sum() / 200:.1f} of {len(tris)} leaf boxes per ray")
    assert own_ok.sum() < 200 * 64               # ... and it prunes
    rng = np.random.default_rng(41)
    ilo, iup, olo, oup = _nested(dt, 4000, rng)
    assert (olo <= ilo).all() and (oup >= iup).all() and (olo == ilo).any() and (olo < ilo).any()
    inner, inner_ok = rcc.slab_entry(ilo[None], iup[None], P, D)
    assert inner_ok.sum() >= 1000
    check(olo[None], oup[None], inner, inner_ok, "random nested boxes")
    # origins ON a face of the inner box with a zero direction component along it: the comparison rule, no 0 * Inf
    Pf = P.repeat(4000, axis=1).copy()
    Pf[:, :, 0] = ilo[None, :, 0]
    Df = np.broadcast_to(D, Pf.shape).copy()
    Df[:, :, 0] = 0
    e_in, ok_in = rcc.slab_entry(ilo[None], iup[None], Pf, Df)
    e_out, ok_out = rcc.slab_entry(olo[None], oup[None], Pf, Df)
    assert not np.isnan(e_in).any() and ok_in.sum() >= 1000 and (ok_out | ~ok_in).all() and (e_out <= e_in).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_checker_agrees_with_an_analytic_case(dt):
    """rays along an axis onto an axis-aligned square at a known distance: everything is exact in either dtype"""
    sq = np.array([[0, 0, 2, 4, 0, 2, 4, 4, 2], [0, 0, 2, 4, 4, 2, 0, 4, 2]], dt)           # z = 2, [0, 4]^2
    p = np.array([[1, 2, 0], [3, 1, 0], [1, 2, 4], [1, 2, 2.5], [5, 1, 0], [3, 1, 0], [3, 1, 0], [2, 2, 0], [3, 1, 1], [3, 1, 0]], dt)
    d = np.array([[0, 0, 1], [0, 0, 2], [0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 1], [0, 0, 0.5], [0, 0, 0]], dt)
    bf = rcc.brute_force(sq, p, d, idt=np.int32)
    #                         below   faster  above   beyond  beside  away  parallel  diagonal: both, smaller index  slower  zero d
    assert bf.index.tolist() == [2, 1, 2, 0, 0, 0, 0, 1, 1, 0] and bf.index.dtype == np.int32
    assert bf.t.tolist() == [2, 1, 2, np.inf, np.inf, np.inf, np.inf, 2, 2, np.inf]
    assert bf.tied.tolist() == [False] * 7 + [True, False, False] and not bf.clamped.any()
    assert bf.uv[0].tolist() == [0.25, 0.25] and bf.uv[1].tolist() == [0.5, 0.25] and bf.uv[7].tolist() == [0, 0.5]
    assert bf.occluded.tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 0]
    # the limit: inclusive, per ray; NaN, negative and zero limits
    lim = np.array([2, 0.5, 1.5, 9, 9, 9, 9, np.nan, -1, 0], dt)
    b2 = rcc.brute_force(sq, p, d, t_max=lim)
    assert b2.index.tolist() == [2, 0, 0, 0, 0, 0, 0, 0, 0, 0] and b2.occluded.tolist() == [1] + [0] * 9
    assert rcc.limit(None, 3, dt).tolist() == [np.finfo(dt).max] * 3 and np.isnan(rcc.limit(np.array([np.nan], dt), 1, dt)).all()
    assert rcc.limit(np.array([np.inf, 1, -np.inf], dt), 3, dt).tolist() == [np.finfo(dt).max, 1, -np.inf]
    # an origin ON the square: t = 0 is a hit, also under a limit of 0 and of -0
    on = rcc.brute_force(sq, np.array([[1, 2, 2]] * 2, dt), np.array([[0, 0, 1]] * 2, dt), t_max=np.array([0.0, -0.0], dt))
    assert on.index.tolist() == [2, 2] and on.t.tolist() == [0, 0]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_clamp_is_active_on_an_axis_aligned_floor(dt):
    tris, p, d = rcc.floor_case(dt)
    lo, up = rcc.triangle_boxes(tris)
    assert (lo[:, 2] == up[:, 2]).all()                       # each triangle lies flat in a face of its own box
    bf = rcc.brute_force(tris, p, d)
    print(f"floor {np.dtype(dt).name}: {int((bf.index != 0).sum())} of {len(p)} rays hit, the clamp is active on {int(bf.clamped.sum())}")
    assert (bf.index != 0).all() and bf.clamped.sum() >= 10 and (~bf.clamped).sum() >= 10
    # there t* is the box's entry, above the exact test's t by rounding only
    from ray_triangle_checker import brute_force as exact_brute_force
    ex = exact_brute_force(tris, p, d)
    assert (ex.index == bf.index).all() and (bf.t >= ex.t).all() and ((bf.t > ex.t) == bf.clamped).all()
    assert (bf.t - ex.t <= 4 * np.finfo(dt).eps * ex.t).all() and (bf.uv == ex.uv).all()
