"""ibvh_cast_spheres on the host side: the header declares it (additive under ABI version 7) and carries its definition, the
hazard of sphere leaves and the loss-free argument; the ctypes table and the Julia extension bind it with the same argument
kinds; the Makefile builds its translation unit, whose one launch goes through the profiling wrapper and which takes the walk,
the tie rule, the slab test and the quadratic from their homes; the entry point validates its arguments — the mode, the
combination of outputs, the refused types and the order of refusal — before any launch.  The numpy checker the GPU test pins
the kernel to (tests/sphere_cast_checker.py): exact on hand-made cases, the grown entry of every box above a leaf's parent
never exceeds t* (what makes pruning lossless), and the GPU test's non-vacuity conditions — the nested pairs whose inner box
pokes out of the stored parent box among them — hold for the brute force alone.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib

import mesh_query_kit as kit
import sphere_cast_checker as scc

NAME = "ibvh_cast_spheres"
UNIT = "ibvh_spherecast.hip"
SHARED = "ibvh_raysphere.hpp"
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


def _flat(text):
    return " ".join(text.replace("//", " ").replace("*", " ").split())


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *points", "const void *displacements", "const void *radii", "int64_t num",
                    "const void *t_max", "const void *skip", "int32_t mode", "void *hit_index", "void *hit_t", "void *touched",
                    "void *stream"]
    assert re.search(r"enum\s*\{\s*IBVH_SPHERECAST_CLOSEST = 0,\s*IBVH_SPHERECAST_ANY = 1\s*\};", hdr)
    assert (abi.SPHERECAST_CLOSEST, abi.SPHERECAST_ANY) == (0, 1)
    assert NAME + " and IBVH_SPHERECAST_CLOSEST / IBVH_SPHERECAST_ANY (additive under 7 likewise: one more entry point)" in _flat(note)
    # the doc comment IS the specification: the eight steps, the hazard and the loss-free argument
    doc = raw[raw.index("rays and swept spheres against a sphere cloud"):raw.index("ibvh_status " + NAME)]
    doc = re.sub(r"\n \*\s+", " ", doc)
    for phrase in ("r = 0 is a ray", "t = 1 is the end of the displacement", "NULL = 0 for all", "0 names no leaf", "no flag argument",
                   "dot(x, y) = (x0 y0 + x1 y1) + x2 y2", "a > b ? a : b", "S = R + r;  m = p - c;  mm = dot(m, m)", "mm <= S * S",
                   "iscontact(BSphere, BSphere)", "t_k = 0", "provided mm > S * S", "B = dot(m, d);  dd = dot(d, d);  Cq = mm - S * S;  disc = B * B - dd * Cq",
                   "t_k = (-B - sqrt(disc)) / dd", "dd > 0 && disc >= 0 && t_k >= 0", "vertex candidate", "!(r >= 0)",
                   "(lo, up) = (c - R, c + R)", "own_k = entry(lo - r, up + r)", "the slab test of ibvh_cast_rays", "STORED box of the node directly above",
                   "tree.levels >= 2", "built_level <= tree.levels - 1", "otherwise -Inf", "t*_k = max(max(t_k, own_k), parent_k)",
                   "k != s and t*_k <= L", "inclusive", "A NaN or negative L admits nothing", "LEXICOGRAPHIC MINIMUM of (t*_k, k)", "SMALLER INDEX",
                   "1 iff a hit exists", "index 0, t +Inf", "FALSE at the lowest node level", "merge.jl:58-81", "length + a.r <= b.r", "3.3 %",
                   "pokes out", "admitted by the leaf's own box and refused by the parent's stored box", "without walking the tree",
                   "lossless WITHOUT an epsilon", "exact minimum / maximum", "monotone", "t*_k >= parent_k >= entry(every grown ancestor)",
                   "own_k <= t*_k", "entry > limit()", "strictly", "nothing that can still win or tie", "-Inf on the first hit",
                   "IBVH_ERR_UNSUPPORTED", "IBVH_ERR_INVALID_ARG", "num == 0", "ibvh_refit", "No reference counterpart", "ONE launch",
                   "no atomics, no LDS, no scratch buffer, no candidate list", "every comparison false on NaN"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    assert lib.SIGNATURES[NAME] == want == abi.CAST_SPHERES_ARGTYPES
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("cast_spheres", "SphereCast"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    for method in ("positions", "normals", "hit"):
        assert hasattr(ibvh.SphereCast, method)
    mk = kit.read("implicitbvh.jl_amd", "csrc", "Makefile")
    assert UNIT in mk[mk.index("SRCS"):mk.index("OBJS")]
    src = kit.read("implicitbvh.jl_amd", "csrc", UNIT)
    # ONE launch, through the profiling wrapper, of the one kernel, on the shared grid and block size
    assert re.findall(r"IBVH_LAUNCH\(\((\w+::\w+)<", src) == ["spherecast::cast_walk_kernel"] and src.count("IBVH_LAUNCH(") == 1
    assert src.count("IBVH_LAUNCH_CHECK()") == 1 and len(re.findall(r"__global__", src)) == 1
    assert "dim3(pre.blocks), dim3(pointwalk::kBlock)" in src and not re.search(r"\bkBlock\s*=", src)
    assert "template <class T, class TN, class I, bool ANY>" in src and "constexpr bool ANY = decltype(mt)::value;" in src
    # the shared walk, once per mode; the shared prologue, for sphere leaves; the shared four-tag dispatch; the shared tie rule
    # (csrc/ibvh_firsthit.hpp: the walk over sphere leaves under either mode's limit, the tie rule where a candidate is offered)
    kit.first_hit_unit(src, leaf="BSphere<T>")
    assert src.count("pointwalk::prepare(bvh, false, ") == src.count("pointwalk::prepare(") == 1
    assert src.index("leaf_kind != IBVH_BSPHERE) return IBVH_ERR_UNSUPPORTED;") < src.index("pointwalk::prepare(")
    assert "using pointwalk::dispatch_box_types_and_bool;" in src and src.count("dispatch_box_types_and_bool(bvh->types, any, launch)") == 1
    assert "using pointwalk::wins;" not in src and "best_index == 0" not in src
    assert src.count("if (index != ignored) firsthit::offer<ANY>(answer, ts, index, []() {});") == 1   # no payload
    for banned in kit.BANNED + kit.FRONT_END + ("fma", "sqrtf", "__builtin_clzll", "raise_flag", "box_bound"):
        assert banned not in src, banned
    # the bound is the slab entry of the box grown by r, the ONE grown entry; the limits; the skipped leaf; the parent from the
    # record pointer
    slab = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_slab.hpp")
    assert src.count("auto grown = [&](const T *lo, const T *up) { return slab::grown_entry(lo, up, r, p, d, inv); };") == 1 and "glo[" not in src
    assert slab.count("const T glo[3] = {lo[0] - r, lo[1] - r, lo[2] - r}, gup[3] = {up[0] + r, up[1] + r, up[2] + r};\n    return slab_entry(glo, gup, p, d, inv);") == 1
    assert "if (numbers & (r >= T(0)) & (L >= T(0))) firsthit::walk<ANY, " in src and "firsthit::outputs_ok(mode, touched, hit_index || hit_t)" in src
    assert "(rec - leaves)" in src and "(leaf_first + position) >> 1" in src and "level_skips(levels, tree.virtual_leaves, levels - 1) + 1" in src
    assert "levels >= 2 && built_level <= levels - 1" in src
    assert "const T tk = raysphere::first_touch(s.x, s.r, p, d, dd, r);" in src and "T ts = tk > entry ? tk : entry;" in src and "ts = ts > above ? ts : above;" in src
    head = _flat(src[:src.index("#include")])
    for phrase in ("FALSE at the lowest node level", "merge.jl:58-81", "length + a.r <= b.r", "poke out of it by an ulp",
                   "t >= entry(grown parent) >= entry(every grown ancestor)", "<= t .", "holds nothing that can still win or tie",
                   "(rec - leaves) / stride", "No reference counterpart"):
        assert phrase in head, phrase
    header = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    top = _flat(header[:header.index("#pragma once")])
    assert "the any-hit mode of ibvh_cast.hip, ibvh_sweep.hip and ibvh_spherecast.hip" in top and "is ibvh_firsthit.hpp's" in top


def test_the_slab_test_the_tie_rule_and_the_quadratic_exist_once_and_the_unit_shares_them():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    text = {f: kit.read("implicitbvh.jl_amd", "csrc", f) for f in sources}
    for define, home in ((r"\bT slab_entry\s*\([^)]*\)\s*\{", "ibvh_slab.hpp"), (r"\bT first_touch\s*\([^)]*\)\s*\{", SHARED)):
        assert [f for f in sources if re.search(define, text[f])] == [home], define
        assert len(re.findall(define, text[home])) == 1
        assert re.search(r'^#include "' + home + '"$', text[UNIT], flags=re.M), home
    src, shared = text[UNIT], text[SHARED]
    # the tie rule is the point walk's (the list resolve of ibvh_raytri.hip has one of its own, for another key)
    assert len(re.findall(r"IBVH_D bool wins\(", text["ibvh_pointwalk.hpp"])) == 1 and not re.search(r"\bwins\s*\([^)]*\)\s*\{", src)
    assert "slab::grown_entry(" in src and "slab_entry" not in src and "tmin" not in src and "ibvh_sqrt(" not in src and "disc" not in src
    # steps 1 to 3, operation for operation; nothing fused; the square root is the library's
    for line in ("const T S = R + r;", "const T m[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};", "const T mm = dot3(m, m);", "const T S2 = S * S;",
                 "const T B = dot3(m, d);", "const T Cq = mm - S2;", "const T disc = B * B - dd * Cq;", "const T t = (-B - ibvh_sqrt(disc)) / dd;",
                 "const bool valid = (mm > S2) & (dd > T(0)) & (disc >= T(0)) & (t >= T(0));", "return mm <= S2 ? T(0) : (valid ? t : inf);"):
        assert shared.count(line) == 1, line
    assert "using raytri::dot3;" in shared and "T dot3(" not in shared and "fma" not in shared and "sqrtf" not in shared
    assert "ibvh_sweep.hip keeps its own `vertex` for now" in _flat(shared) and "a later change" in _flat(shared)
    # the sweep's own candidate is untouched
    assert "const T disc = B * B - dd * Cq;" in text["ibvh_sweep.hip"] and "raysphere" not in text["ibvh_sweep.hip"]
    import __graft_entry__ as entry
    assert {os.path.join(csrc, SHARED), os.path.join(csrc, UNIT)} <= set(entry.kernel_sources(kit.ROOT))


def test_julia_wrapper_binds_it_with_the_ctypes_signature_and_the_docs_name_it():
    src = kit.julia_ccall(NAME, "cast_spheres")
    body = src[src.index("function cast_spheres("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_SPHERECAST_ANY : IBVH_SPHERECAST_CLOSEST" in body and "point_morton_order(points)" in body and "BSphere{T}" in body
    design = kit.read("DESIGN.md")
    section = design[design.index("Rays and swept spheres against a sphere cloud"):][:12000]
    for phrase in ("no reference counterpart", "lossless", "merge.jl:58-81", "pokes out", "3.3 %", "parent", "VGPRs", "scratch", "bench_cast_spheres.py"):
        assert phrase in section, phrase
    assert len(re.findall(r"^\| `<(?:float|double), (?:float|double), (?:int|long), (?:false|true)>` \|", section, flags=re.M)) == 12
    assert kit.read("tools", "bench_cast_spheres.py") and "bench_cast_spheres.py" in kit.read("tools", "README.md")
    assert "cast_spheres" in kit.read("README.md") and "cast_spheres" in kit.read("INTEGRATION.md")


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    fake = kit.fake_bvh
    ok = dict(bvh=fake(), p=p, d=p, r=None, n=0, tmax=None, skip=None, mode=abi.SPHERECAST_CLOSEST, index=p, t=None, touched=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["p"], a["d"], a["r"], a["n"], a["tmax"], a["skip"], a["mode"], a["index"], a["t"], a["touched"], a["stream"])
    # the two modes and which outputs each takes: closest any non-empty subset of the two, never `touched`; any that alone
    any_ = kit.check_mode_and_outputs(call, kit.CAST_SPHERES, p, "n", ("index", "t"), "touched")
    for optional in (dict(r=p), dict(tmax=p), dict(skip=p), dict(r=p, tmax=p, skip=p)):
        assert call(**optional) == abi.OK and call(**dict(any_, **optional)) == abi.OK, optional
    for bad in (dict(bvh=None), dict(n=-1), dict(n=5, p=None), dict(n=5, d=None), dict(bvh=fake(leaves=None)), dict(bvh=fake(nodes=None)),
                dict(bvh=fake(built_level=0)), dict(bvh=fake(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG and call(**dict(any_, **bad)) == abi.ERR_INVALID_ARG, bad
    assert call(p=None, d=None) == abi.OK                               # no items: no arrays needed
    assert call(bvh=fake(n=1, nodes=None)) == abi.OK                    # a one-leaf tree has no nodes
    assert call(bvh=fake(built_level=4, nodes=None)) == abi.OK          # ... nor does a tree built at its leaf level only
    broken = fake()
    broken.tree.virtual_leaves += 1                                     # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # the accepted types: BSphere leaves under BBox nodes of the same or a wider float type, any index type
    for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64), dict(morton=abi.U64)):
        assert call(bvh=fake(**good)) == abi.OK and call(bvh=fake(**good), **any_) == abi.OK, good
    for bad in (dict(leaf_kind=abi.BBOX), dict(node_kind=abi.BSPHERE), dict(leaf_kind=abi.BBOX, node_kind=abi.BSPHERE),
                dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
        # (with items to process too: refused, never launched on the fake pointers)
        for mode in (dict(), any_):
            assert call(bvh=fake(**bad), **mode) == abi.ERR_UNSUPPORTED, bad
            assert call(bvh=fake(**bad), n=5, **mode) == abi.ERR_UNSUPPORTED, bad
    # the order: the entry's own checks first, the types next, the tree and the pointers last
    assert call(bvh=fake(leaf_kind=abi.BBOX), mode=9) == abi.ERR_INVALID_ARG
    assert call(bvh=fake(leaf_kind=abi.BBOX), n=-1) == abi.ERR_INVALID_ARG
    assert call(bvh=fake(leaf_kind=abi.BBOX, leaves=None), n=5, p=None) == abi.ERR_UNSUPPORTED
    assert call(bvh=fake(node_kind=abi.BSPHERE, built_level=0)) == abi.ERR_UNSUPPORTED


# ---- the checker --------------------------------------------------------------------------------------------------------------
def _one(dt, spheres, p, d, r=0.0, **kw):
    """the brute force for hand-made spheres in one flat level (no parent boxes)"""
    s = np.array(spheres, dt).reshape(-1, 4)
    p, d = np.array(p, dt).reshape(-1, 3), np.array(d, dt).reshape(-1, 3)
    r = np.broadcast_to(np.array(r, dt), (len(p),)).copy()
    return scc.brute_force(s, np.arange(1, len(s) + 1), None, p, d, r, **kw)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_checker_is_exact_on_hand_made_cases(dt):
    ball = [[3, 0, 0, 1]]
    bf = _one(dt, ball, [[0, 0, 0]] * 2, [[1, 0, 0]] * 2, [0, 0.5], idt=np.int32)
    assert bf.index.tolist() == [1, 1] and bf.t.tolist() == [2, 1.5] and bf.touched.tolist() == [1, 1]
    assert bf.index.dtype == np.int32 and bf.t.dtype == dt and bf.touched.dtype == np.uint8 and not bf.start.any()
    # t is in units of d; a ray pointing away, a ray that passes beside it: a miss is index 0, t +Inf
    bf = _one(dt, ball, [[0, 0, 0]] * 3, [[2, 0, 0], [-1, 0, 0], [1, 1, 0]])
    assert bf.index.tolist() == [1, 0, 0] and bf.t.tolist() == [1, np.inf, np.inf] and bf.touched.tolist() == [1, 0, 0]
    # an origin inside, on the surface, and within r of it: t = 0
    bf = _one(dt, ball, [[3, 0.5, 0], [2, 0, 0], [1.5, 0, 0]], [[1, 0, 0], [-1, 0, 0], [0, 1, 0]], [0, 0, 0.5])
    assert bf.index.tolist() == [1, 1, 1] and bf.t.tolist() == [0, 0, 0] and bf.start.all()
    # d = 0: only touching hits
    bf = _one(dt, ball, [[3, 0, 0.5], [0, 0, 0], [1, 0, 0]], [[0, 0, 0]] * 3, [0, 0, 1])
    assert bf.index.tolist() == [1, 0, 1] and bf.t.tolist() == [0, np.inf, 0]
    # a duplicate sphere wins by the smaller index; skip hands the win to the twin; skip = 0 ignores nothing
    twins = [[3, 0, 0, 1], [7, 0, 0, 1], [3, 0, 0, 1]]
    bf = _one(dt, twins, [[0, 0, 0]] * 5, [[1, 0, 0]] * 5, skip=[0, 1, 3, 2, 9])
    assert bf.index.tolist() == [1, 3, 1, 1, 1] and bf.t.tolist() == [2] * 5 and bf.tied.tolist() == [True, False, False, True, True]
    assert bf.second_index.tolist() == [3, 2, 2, 3, 3] and bf.second_t.tolist() == [2, 6, 6, 2, 2] and bf.hits.tolist() == [3, 2, 2, 2, 3]
    both = _one(dt, [[3, 0, 0, 1]], [[0, 0, 0]], [[1, 0, 0]], skip=[1])
    assert both.index.tolist() == [0] and both.touched.tolist() == [0]
    # the limit: inclusive, per query; zero keeps who touches at the start; +Inf is none
    bf = _one(dt, twins, [[0, 0, 0]] * 6 + [[2.5, 0, 0]], [[1, 0, 0]] * 7, t_max=[2, np.nextafter(dt(2), dt(0)), 0, np.inf, 6, 1e30, 0])
    assert bf.index.tolist() == [1, 0, 0, 1, 1, 1, 1] and bf.t.tolist() == [2, np.inf, np.inf, 2, 2, 2, 0] and bf.hits.tolist() == [2, 0, 0, 3, 3, 3, 2]
    # NaN p, d, r or t_max, a negative r or t_max: a miss, even from inside
    nan = np.nan
    for kw in (dict(p=[nan, 0, 0]), dict(p=[3, 0, nan]), dict(d=[nan, 0, 0]), dict(d=[1, nan, 0]), dict(r=nan), dict(r=-1.0), dict(r=-np.inf),
               dict(t_max=[nan]), dict(t_max=[-1.0]), dict(t_max=[-np.inf])):
        for start in ([0, 0, 0], [3, 0, 0]):
            a = dict(dict(p=start, d=[1, 0, 0], r=0.0), **kw)
            bf = _one(dt, ball, [a.pop("p")], [a.pop("d")], a.pop("r"), **a)
            assert bf.index.tolist() == [0] and bf.t.tolist() == [np.inf] and bf.touched.tolist() == [0], (kw, start)
    # a NaN leaf is never hit, the other one still is; an infinite radius touches everything at once
    bf = _one(dt, [[3, 0, 0, nan], [nan, 0, 0, 1], [7, 0, 0, 1]], [[0, 0, 0]], [[1, 0, 0]])
    assert bf.index.tolist() == [3] and bf.t.tolist() == [6] and bf.hits.tolist() == [1]
    assert _one(dt, ball, [[50, 50, 50]], [[0, 0, 1]], np.inf).t.tolist() == [0]


def _merge_to_box(a, b):
    """merge_to(BSphere, BSphere, BBox) of merge.jl:58-81 for rows of spheres (n, 4), in their dtype -> (lo, up, shortcut)"""
    e = a[:, :3] - b[:, :3]
    length = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    alo, aup = scc.sphere_boxes(a)
    blo, bup = scc.sphere_boxes(b)
    only_b, only_a = (length + a[:, 3] <= b[:, 3])[:, None], (length + b[:, 3] <= a[:, 3])[:, None]
    lo = np.where(only_b, blo, np.where(only_a, alo, np.where(alo < blo, alo, blo)))
    up = np.where(only_b, bup, np.where(only_a, aup, np.where(aup > bup, aup, bup)))
    return lo, up, (only_b | only_a)[:, 0]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_grown_entry_of_every_box_above_the_parent_never_exceeds_t_star(dt):
    """What the walk prunes with.  2,000 leaf / query pairs — half of them random siblings, half the inner spheres of the nested
    pairs under the box of the outer one alone —: above the parent's stored box a chain of exact minimum / maximum boxes
    (kit.chain), each grown by r; its entry never exceeds the leaf's t*, nor does the leaf's own (the walk's bound of the leaf);
    and WITHOUT step 5 that fails on the nested pairs, which is why it is there."""
    rng = np.random.default_rng(5)
    pairs, axis, sign, _, _ = scc.nested_pairs(dt)
    k = 1000
    leaf = np.concatenate([rng.random((k, 3)) * 2 - 1, 0.05 + 0.2 * rng.random((k, 1))], axis=1).astype(dt)
    sibling = np.concatenate([leaf[:, :3] + 0.4 * (rng.random((k, 3)) - 0.5), 0.05 + 0.2 * rng.random((k, 1))], axis=1).astype(dt)
    rep = np.arange(k) % len(axis)
    leaf, sibling = np.concatenate([leaf, pairs[1::2][rep]]), np.concatenate([sibling, pairs[0::2][rep]])
    plo, pup, shortcut = _merge_to_box(leaf, sibling)
    assert shortcut[k:].all() and 0 < shortcut[:k].sum() < k // 2
    # queries: near the leaf, some from the poking tip, zero direction components, r = 0 and r > 0
    n = len(leaf)
    p = (leaf[:, :3] + (rng.random((n, 3)) - 0.5) * 1.5).astype(dt)
    d = ((leaf[:, :3] - p) * (0.5 + 1.5 * rng.random((n, 1))) + 0.2 * (rng.random((n, 3)) - 0.5)).astype(dt)   # roughly at the leaf
    tip = np.arange(k, n)
    p[tip] = leaf[tip, :3]
    p[tip, axis[rep]] = leaf[tip, axis[rep]] + sign[rep].astype(dt) * leaf[tip, 3]
    d[tip, axis[rep]] = 0
    d[np.arange(0, k, 7), rng.integers(0, 3, len(range(0, k, 7)))] = 0
    r = np.where(np.arange(n) % 2 == 0, 0, 0.1 * rng.random(n)).astype(dt)
    r[tip[: len(tip) // 2]] = 0
    tk = scc.first_touch(leaf[:, :3], leaf[:, 3], p, d, r)
    llo, lup = scc.sphere_boxes(leaf)
    own = scc.grown_entry(llo, lup, p, d, r)
    t4 = scc._max(tk, own)
    ts = scc._max(t4, scc.grown_entry(plo, pup, p, d, r))
    finite = np.isfinite(ts)
    assert finite[:k].sum() >= 200 and np.isfinite(t4[k:]).sum() >= 200
    assert (own <= ts).all()
    above = kit.chain(rng, plo, pup, dt)
    assert len(above) == 5 and (above[0][0] <= plo).all() and (above[-1][1] >= pup).all()
    for lo, up in above:
        assert lo.dtype == dt
        assert (scc.grown_entry(lo, up, p, d, r) <= ts).all()
    # without step 5 the parent's own entry exceeds the time on the nested pairs: the leaf would be a hit the walk cannot reach
    lost = scc.grown_entry(plo, pup, p, d, r) > t4
    assert lost[k:].sum() >= 100 and not lost[:k][~shortcut[:k]].any()


CLOUD_FLOORS = dict(hit=300, miss=80, start=100, later=150, second=200, tied_later=10, tied_start=30)


def cloud_facts(bf):
    hit = bf.index != 0
    return dict(hit=int(hit.sum()), miss=int((~hit).sum()), start=int(bf.start.sum()), later=int((hit & ~bf.start).sum()),
                second=int((bf.second_index != 0).sum()), tied_later=int((bf.tied & (bf.t > 0)).sum()), tied_start=int((bf.tied & (bf.t == 0)).sum()))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_cloud_and_lattice_meet_the_gpu_tests_non_vacuity_conditions(dt):
    """Measured here, equal in Float32 and Float64: of the cloud's 800 queries 416 hit (394 within t_max = 1), 144 start in touch,
    272 hit later, 366 have a runner-up, 26 winners are tied at t > 0 and 65 at 0; all 600 of the lattice hit, and the own-box
    clamp exceeds t for 43 (Float32) / 33 (Float64) winners.  Asserted at about half of each."""
    ref = scc.reference(dt)
    s, p, d, r, _ = ref["cloud"]
    assert s.dtype == dt and len(s) == 3300 and (s[3000:] == s[:300]).all() and (r[::4] == 0).all() and (r > 0).sum() >= 500
    order, boxes, bvh = scc.host_tree(s)
    assert sorted(order.tolist()) == list(range(1, 3301)) and boxes.shape == (1650, 6) and boxes.dtype == dt
    bf = scc.brute_force(s, order, boxes, p, d, r)
    facts = cloud_facts(bf)
    print(f"cloud {np.dtype(dt).name}: {facts}")
    for key, floor in CLOUD_FLOORS.items():
        assert facts[key] >= floor, (key, facts[key])
    hit = bf.index != 0
    assert (hit == np.isfinite(bf.t)).all() and (hit == (bf.touched == 1)).all() and (bf.t[hit] >= 0).all() and (bf.hits[hit] >= 1).all()
    # the limit only takes hits away and leaves those within it as they were
    one = scc.brute_force(s, order, boxes, p, d, r, t_max=np.ones(800, dt))
    keep = bf.t <= 1
    print(f"cloud {np.dtype(dt).name}: {int((one.index != 0).sum())} within t_max = 1")
    assert 150 <= keep.sum() < hit.sum() and (one.index[keep] == bf.index[keep]).all() and (one.index[~keep] == 0).all() and (one.t[keep] == bf.t[keep]).all()
    # skip = the winner: the runner-up
    again = scc.brute_force(s, order, boxes, p, d, r, skip=bf.index)
    assert (again.index == bf.second_index).all() and again.t.tobytes() == bf.second_t.tobytes()
    # the order of the leaves cannot matter where no parent box is read
    flat = scc.brute_force(s, np.arange(1, 3301), None, p, d, r)
    assert (flat.index == bf.index_no5).all() and flat.t.tobytes() == bf.t_no5.tobytes()
    s, p, d, r, _ = ref["lattice"]
    order, boxes, _ = scc.host_tree(s)
    bf = scc.brute_force(s, order, boxes, p, d, r)
    print(f"lattice {np.dtype(dt).name}: {int((bf.index != 0).sum())} of {len(p)} hit, the own-box clamp is active on {int(bf.clamp_own.sum())} winners")
    assert len(s) == 512 and len(p) == 600 and (bf.index != 0).all() and bf.clamp_own.sum() >= 20 and (r == 0).sum() == 400
    assert ((d != 0).sum(axis=1) == 1).all()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_nested_pairs_poke_out_of_their_parents_stored_box_and_step_5_decides(dt):
    """The hazard, on the CPU oracle's build.  Measured here: of 60,000 candidate pairs the shortcut fires for 54,040 (Float32) /
    55,197 (Float64) and 3,284 / 2,061 of those poke out; all 150 pairs kept are siblings under a parent box with the bits of
    the outer sphere's box; 78 / 118 tip queries are a miss under the definition and a t = 0 hit without step 5."""
    spheres, axis, sign, fires, pokes = scc.nested_pairs(dt)
    k = len(axis)
    print(f"nested {np.dtype(dt).name}: the shortcut fires for {fires} candidates, {pokes} of them poke out, {k} pairs kept")
    assert k >= 50 and pokes >= 50
    outer, inner = spheres[0::2], spheres[1::2]
    _, _, shortcut = _merge_to_box(inner, outer)
    (ilo, iup), (olo, oup) = scc.sphere_boxes(inner), scc.sphere_boxes(outer)
    rows = np.arange(k)
    out = np.where(sign > 0, iup[rows, axis] > oup[rows, axis], ilo[rows, axis] < olo[rows, axis])
    assert shortcut.all() and out.all()
    ulp = np.where(sign > 0, np.nextafter(oup[rows, axis], dt(np.inf)) == iup[rows, axis], np.nextafter(olo[rows, axis], dt(-np.inf)) == ilo[rows, axis])
    assert ulp.sum() >= k // 2                                            # ... by an ulp
    s, p, d, r, skip = scc.reference(dt)["nested"]
    assert s.tobytes() == spheres.tobytes() and len(p) == k + 200 and (d[rows, axis] == 0).all() and (skip[:k] == 2 * rows + 1).all()
    order, boxes, bvh = scc.host_tree(s)
    siblings = scc.sibling_pairs(s, order, boxes)
    bf = scc.brute_force(s, order, boxes, p, d, r, skip=skip)
    decided = (bf.index[:k] == 0) & (bf.index_no5[:k] == 2 * rows + 2) & (bf.t_no5[:k] == 0)
    print(f"nested {np.dtype(dt).name}: {int(siblings.sum())} sibling pairs, step 5 decides {int(decided.sum())} tip queries, "
          f"{int((bf.index[k:] != 0).sum())} of the 200 random queries hit")
    assert siblings.sum() >= 20 and decided.sum() >= 20 and (siblings | ~decided).all() and (bf.index[k:] != 0).sum() >= 5
    # nearest_leaves' premise holds on these pairs all the same: every centre lies in its parent's stored box
    position = np.empty(len(order), np.int64)
    position[order - 1] = np.arange(len(order))
    pb = boxes[position >> 1]
    assert ((pb[:, :3] <= s[:, :3]) & (s[:, :3] <= pb[:, 3:])).all()
