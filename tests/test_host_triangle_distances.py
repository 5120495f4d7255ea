"""ibvh_triangle_distances on the host side: the header declares it (additive under ABI version 7) and carries its contract,
the ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its
one launch goes through the profiling wrapper on the shared walk, the segment-segment routine lives once in a header of its
own, and the entry point validates its arguments — the skip flag, "any one output" and the refused type combinations
included — before any launch.  The numpy checker the GPU test pins the kernel to (tests/triangle_distance_checker.py): it
gives the known answers on hand-made pairs, every kind occurs, an independent float64 certificate holds on random pairs, the
computed bound of a box never exceeds a computed d2 under it (what makes pruning lossless), and the GPU test's conditions
hold for the brute force alone.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib

import mesh_query_kit as kit
import triangle_contacts_checker as tcc
import triangle_distance_checker as tdc

NAME = "ibvh_triangle_distances"
UNIT = "ibvh_tridist.hip"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)
DTYPES = [np.float32, np.float64]


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *queries",
                    "int64_t num_queries", "int32_t skip", "const void *max_distance2", "void *closest_index", "void *closest_d2",
                    "void *point_query", "void *point_mesh", "void *closest_kind", "void *flag", "void *stream"]
    flat = " ".join(note.replace("*", " ").split())
    assert NAME + " (additive under 7 likewise: one more entry point)" in flat
    doc = raw[raw.index("triangle-vs-mesh distance: the closest mesh triangle"):raw.index("ibvh_status " + NAME)]
    doc = re.sub(r"\n \*\s+", " ", doc)        # (the comment's lines joined: a phrase may run over a line end)
    for phrase in ("The CUT rule", "not apart", "six strict comparisons", "in its order", "t <= 1", "d2 = 0", "kind = 15", "FIRST test that hit",
                   "The CANDIDATE rule", "fifteen candidates", "strictly smaller", "kind 0, 1, 2", "kind 3, 4, 5", "kind 6 + 3 i + j",
                   "the evaluation of ibvh_closest_triangles", "Ericson", "5.1.9", "no epsilon", "A == 0", "E == 0", "den > 0",
                   "s = unit((B*F - C*E) / den)", "t = (B*s + F) / E", "s = unit(-C / A)", "s = unit((B - C) / A)",
                   "clamped into its own segment's box", "e = xQ - xK;  d2 = (e0*e0 + e1*e1) + e2*e2",
                   "LEXICOGRAPHIC MINIMUM of (d2, index)", "ALL mesh triangles", "d2 <= max_distance2", "names a row",
                   "tie rule of ibvh_closest_triangles", "NaN coordinate", "never wins", "lossless WITHOUT an epsilon",
                   "Every xQ lies in Q's exact box", "Every xK lies in K's exact box", "monotone",
                   "g_k = max(0, lo_k - qup_k, qlo_k - up_k)", "lb(B) = (g0*g0 + g1*g1) + g2*g2", "lb = 0", "strictly",
                   "OWN box, not the stored one", "skin", "coplanar and touching pairs are decided by rounding",
                   "IBVH_TRIS_SKIP_SHARED_VERTEX", "HOST pointer", "at least one non-NULL", "not written", "bit 1", "value 2",
                   "IBVH_ERR_UNSUPPORTED", "IBVH_ERR_INVALID_ARG", "num_queries == 0", "No reference counterpart", "ONE launch",
                   "no atomics, no LDS, no scratch buffer", "every comparison false on NaN", "Why the fifteen suffice"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 8
    assert lib.SIGNATURES[NAME] == want == abi.TRIANGLE_DISTANCES_ARGTYPES and abi.TRIDIST_CUT == tdc.CUT == 15
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("triangle_distances", "TriangleDistances", "mesh_distance", "MeshDistance", "self_clearance"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    # the walk, its block size and grid, the prologue, the gather, the dispatch and the flag are the shared ones
    src = kit.query_unit(UNIT, "tridist::tridist_walk_kernel", walks=2, pair=True)
    assert len(re.findall(r"__global__", src)) == 1 and "template <class T, class TN, class I>\n__global__" in src
    assert "fma" not in src
    # the first walk starts from Q's vertex a — the point candidate 0 is evaluated from, which the seed's argument rests on
    assert src.count("nodes, nan, Q.v, max_d2, box, gather, pair, best);") == 1
    assert src.index("if (c == 0) r.put(d2, xq, xk, 0);") < src.index("else r.offer(d2, xq, xk, c);")
    # the bound: both differences, the larger, not below zero; d2's order — the shared box_gap, with Q's box
    assert src.count("trigeom::box_gap(lo, up, qlo, qup)") == 1
    geom = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_trigeom.hpp")
    for line in ("const T below = lo[k] - qup[k], above = qlo[k] - up[k];", "const T m = below > above ? below : above;",
                 "g[k] = m > T(0) ? m : T(0);", "return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];"):
        assert geom.count(line) == 1 and line not in src, line
    # the candidates are loops, one at a time; the cut tests run only under the box clause
    assert src.count("#pragma unroll 1") == 3 and src.count("pointtri::closest_on_triangle(") == 1   # the candidates'; the seed's is the routine's
    assert src.count("segseg::closest_on_segments(") == 1 and src.count("trigeom::segment_cuts(tri, p0, p1, x)") == 1
    assert "ray_triangle(" not in src and geom.count("raytri::ray_triangle(tri, p0, d, t, u, v) & (t <= T(1))") == 1
    assert src.index("const bool apart = trigeom::apart(qlo, qup, klo, kup);") < src.index("if (!apart) {") < src.index("trigeom::segment_cuts(")
    assert src.index("trigeom::segment_cuts(") < src.index("pointtri::closest_on_triangle(tri.v, y, x, region)")


# what the mesh queries compute with in more than one unit: (what defines it, its one home); no other source defines it
SHARED_PIECES = (
    (r"\bclosest_on_triangle\s*\([^)]*\)\s*\{", "ibvh_pointtri.hpp"), (r"\bbool ray_triangle\s*\([^)]*\)\s*\{", "ibvh_raytest.hpp"),
    (r"\bclosest_on_segments\s*\([^)]*\)\s*\{", "ibvh_segseg.hpp"),
    (r"IBVH_D void triangle_box\(", "ibvh_trigeom.hpp"), (r"IBVH_D bool apart\(", "ibvh_trigeom.hpp"), (r"IBVH_D T box_gap\(", "ibvh_trigeom.hpp"),
    (r"IBVH_D bool same_vertex\(", "ibvh_trigeom.hpp"), (r"IBVH_D bool shares_vertex\(", "ibvh_trigeom.hpp"), (r"IBVH_D T sel\(", "ibvh_trigeom.hpp"),
    (r"IBVH_D void vertex_of\(", "ibvh_trigeom.hpp"), (r"IBVH_D void edge_of\(", "ibvh_trigeom.hpp"), (r"\bstruct Pair\b", "ibvh_trigeom.hpp"),
    (r"IBVH_D bool segment_cuts\(", "ibvh_trigeom.hpp"), (r"IBVH_D I closest_pair\(", "ibvh_pairwalk.hpp"),
    (r"IBVH_D void store_pair\(", "ibvh_pairwalk.hpp"), (r"IBVH_D bool wins\(T x, I index, T best, I best_index\)", "ibvh_pointwalk.hpp"),
    (r"int dispatch_box_types_and_bool\(", "ibvh_pointwalk.hpp"))
# ... and what the three first-hit queries and the grown-box queries share: (what defines it, its one home, the units that include it)
FIRST_HIT_UNITS = ("ibvh_cast.hip", "ibvh_sweep.hip", "ibvh_spherecast.hip")
FIRST_HIT_PIECES = (
    (r"IBVH_D T limit\(", "ibvh_firsthit.hpp", FIRST_HIT_UNITS), (r"\bstruct Answer\b", "ibvh_firsthit.hpp", FIRST_HIT_UNITS),
    (r"IBVH_D void offer\(Answer<T, I> &a, ", "ibvh_firsthit.hpp", FIRST_HIT_UNITS), (r"IBVH_D void store\(", "ibvh_firsthit.hpp", FIRST_HIT_UNITS),
    (r"inline bool outputs_ok\(", "ibvh_firsthit.hpp", FIRST_HIT_UNITS),
    (r"IBVH_D T grown_entry\(", "ibvh_slab.hpp", ("ibvh_sweep.hip", "ibvh_spherecast.hip", "ibvh_capsules.hip")))
# ... the operations behind them, which no other source spells: (the text, its one home)
SPELLED_ONCE = (
    ("l = v[3 + k] < l ? v[3 + k] : l;", "ibvh_trigeom.hpp"), ("u = v[6 + k] > u ? v[6 + k] : u;", "ibvh_trigeom.hpp"),
    ("(qup[0] < lo[0]) | (qlo[0] > up[0]) | (qup[1] < lo[1]) | (qlo[1] > up[1]) | (qup[2] < lo[2]) | (qlo[2] > up[2])", "ibvh_trigeom.hpp"),
    ("below > above ? below : above", "ibvh_trigeom.hpp"), ("(x[0] == y[0]) & (x[1] == y[1]) & (x[2] == y[2])", "ibvh_trigeom.hpp"),
    ("shared |= same_vertex(Q + 3 * i, K + 3 * j)", "ibvh_trigeom.hpp"), ("return c ? a : b;", "ibvh_trigeom.hpp"),
    ("sel(i == 1, v[3 + k], sel(i == 2, v[6 + k], v[k]))", "ibvh_trigeom.hpp"), ("sel(i == 0, v[3 + k], sel(i == 1, v[6 + k], v[k]))", "ibvh_trigeom.hpp"),
    ("if (d < d2) put(d, q, k, c);", "ibvh_trigeom.hpp"), ("& (t <= T(1))", "ibvh_trigeom.hpp"), ("x[k] = p0[k] + t * d[k];", "ibvh_trigeom.hpp"),
    ("(x < best) | ((x == best) & ((best_index == 0) | (index < best_index)))", "ibvh_pointwalk.hpp"),
    ("std::true_type{}", "ibvh_pointwalk.hpp"), ("seed = d2 < seed ? d2 : seed;", "ibvh_pairwalk.hpp"),
    ("hit ? best.d2 : std::numeric_limits<T>::infinity()", "ibvh_pairwalk.hpp"),
    # the first-hit protocol: the limit's two statements, the any-hit limit, the any-hit bit, the miss's t, the mode / outputs rule
    ("given = t_max ? t_max[item] : ", "ibvh_firsthit.hpp"), ("given > std::numeric_limits<T>::max() ? std::numeric_limits<T>::max() : given", "ibvh_firsthit.hpp"),
    ("? -inf : L", "ibvh_firsthit.hpp"), ("touched |= ts <= ", "ibvh_firsthit.hpp"), ("hit ? a.best : std::numeric_limits<T>::infinity()", "ibvh_firsthit.hpp"),
    ("any_output && !closest_outputs", "ibvh_firsthit.hpp"), ("IBVH_SPHERECAST_CLOSEST == 0 && IBVH_SPHERECAST_ANY == 1", "ibvh_firsthit.hpp"),
    ("lo[0] - r, lo[1] - r, lo[2] - r", "ibvh_slab.hpp"), ("up[0] + r, up[1] + r, up[2] + r", "ibvh_slab.hpp"))
# ... and how often each unit that used to spell one calls it now: as often as it spelled it
CALLS = {
    "trigeom::triangle_box(": {"ibvh_tritri.hip": 1, "ibvh_tridist.hip": 2, "ibvh_segtri.hpp": 1},
    "trigeom::apart(": {"ibvh_tritri.hip": 1, "ibvh_boxes.hip": 1, "ibvh_tridist.hip": 1, "ibvh_segtri.hpp": 1},
    "trigeom::box_gap(": {"ibvh_tridist.hip": 1, "ibvh_segdist.hip": 1, "ibvh_capsules.hip": 1},
    "trigeom::shares_vertex(Q.v, K.v)": {"ibvh_tritri.hip": 1, "ibvh_tridist.hip": 1},
    "trigeom::segment_cuts(": {"ibvh_tritri.hip": 1, "ibvh_tridist.hip": 1, "ibvh_segtri.hpp": 1},
    "trigeom::Pair<T>": {"ibvh_tridist.hip": 3, "ibvh_segtri.hpp": 1, "ibvh_segdist.hip": 2, "ibvh_capsules.hip": 1, "ibvh_pairwalk.hpp": 3},
    "pointwalk::wins(": {"ibvh_closest.hip": 1, "ibvh_firsthit.hpp": 1, "ibvh_pairwalk.hpp": 1},   # (no longer the three first-hit units)
    "firsthit::limit(": dict.fromkeys(FIRST_HIT_UNITS, 1), "firsthit::offer<ANY>(": dict.fromkeys(FIRST_HIT_UNITS, 1),
    "firsthit::walk<ANY, ": dict.fromkeys(FIRST_HIT_UNITS, 1), "firsthit::store<ANY>(": dict.fromkeys(FIRST_HIT_UNITS, 1),
    "firsthit::outputs_ok(": dict.fromkeys(FIRST_HIT_UNITS, 1), "pointwalk::walk<VL, TN>(tree, built_level, leaves, lay, nodes, bound, [&]() { return a.": {"ibvh_firsthit.hpp": 2},
    "slab::grown_entry(": {"ibvh_sweep.hip": 1, "ibvh_spherecast.hip": 1, "ibvh_capsules.hip": 1},
    "pairwalk::closest_pair<I>(": {"ibvh_tridist.hip": 1, "ibvh_segdist.hip": 1},
    "pairwalk::store_pair(": {"ibvh_tridist.hip": 1, "ibvh_segdist.hip": 1},
    "pointwalk::dispatch_box_types_and_bool(": {"ibvh_cast.hip": 1, "ibvh_sweep.hip": 1, "ibvh_spheres.hip": 1, "ibvh_tritri.hip": 1,
                                                "ibvh_capsules.hip": 1, "ibvh_boxes.hip": 1}}


def test_the_shared_routines_exist_once_and_the_unit_includes_them():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    text = {f: kit.read("implicitbvh.jl_amd", "csrc", f) for f in sources}
    for define, home in SHARED_PIECES:
        assert [f for f in sources if re.search(define, text[f])] == [home], define
        assert len(re.findall(define, text[home])) == 1
        assert re.search(r'^#include "' + home + '"$', text[UNIT], flags=re.M), home
    for define, home, units in FIRST_HIT_PIECES:
        assert [f for f in sources if re.search(define, text[f])] == [home] and len(re.findall(define, text[home])) == 1, define
        assert all(re.search(r'^#include "' + home + '"$', text[u], flags=re.M) for u in units), home
    assert all("wins(" not in text[u] for u in FIRST_HIT_UNITS)
    for spelled, home in SPELLED_ONCE:
        assert [f for f in sources if spelled in text[f]] == [home] and text[home].count(spelled) == 1, spelled
    assert [f for f in sources if "best_index == 0" in text[f]] == ["ibvh_pointwalk.hpp"]
    for call, users in CALLS.items():
        assert {f: text[f].count(call) for f in sources if call in text[f]} == users, call
    # the two shapes of the six edge tests stay two: named statically for the contacts, one rolled loop for the distances
    assert "#pragma unroll 1" not in text["ibvh_tritri.hip"] and "#pragma unroll 1" not in text["ibvh_trigeom.hpp"]
    seg = text["ibvh_segseg.hpp"]
    assert "using pointtri::dot3;" in seg and "T dot3(" not in seg       # dot3 associates as in ibvh_pointtri.hpp: it IS that one
    for line in ("if (a == T(0)) {", "if (e != T(0)) t = unit(f / e);", "if (e == T(0)) {", "const T den = a * e - b * b;",
                 "if (den > T(0)) s = unit((b * f - c * e) / den);", "t = (b * s + f) / e;", "s = unit(-c / a);", "s = unit((b - c) / a);",
                 "return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];"):
        assert line in seg, line
    assert "eps" not in seg.lower().replace("epsilon", "") and "1e-" not in seg
    import __graft_entry__ as entry
    assert {os.path.join(csrc, "ibvh_segseg.hpp"), os.path.join(csrc, UNIT)} <= set(entry.kernel_sources(kit.ROOT))


def test_julia_wrapper_binds_it_with_the_ctypes_signature_and_the_docs_name_it():
    src = kit.julia_ccall(NAME, "triangle_distances")
    reduce = src[src.index("function mesh_distance("):]
    assert "triangle_distances(bvh, triangles, queries;" in reduce[:reduce.index("\nend\n")] and "function ImplicitBVH.mesh_distance" not in src
    body = src[src.index("function triangle_distances("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_TRIS_SKIP_SHARED_VERTEX" in body and "point_morton_order(" in body
    design = kit.read("DESIGN.md")
    section = design[design.index("Triangle-vs-mesh distance"):][:12000]
    for phrase in ("no reference counterpart", "lossless", "Cut rule", "fifteen candidates", "VGPRs", "scratch", "certificate"):
        assert phrase in section, phrase
    assert len(re.findall(r"^\| `<(?:float|double), (?:float|double), (?:int|long)>` \|", section, flags=re.M)) == 6
    assert kit.read("tools", "bench_triangle_distances.py") and "bench_triangle_distances.py" in kit.read("tools", "README.md")


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    ok = dict(bvh=_fake_bvh(), tris=p, nt=5, q=p, nq=0, skip=0, r2=None, index=p, d2=None, xq=None, xk=None, kind=None, flag=None,
              stream=None)
    outputs = ("index", "d2", "xq", "xk", "kind")

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["q"], a["nq"], a["skip"], a["r2"], a["index"], a["d2"], a["xq"], a["xk"], a["kind"],
                 a["flag"], a["stream"])
    assert call() == abi.OK and call(flag=p) == abi.OK              # num_queries = 0: nothing to do
    assert call(skip=abi.TRIS_SKIP_SHARED_VERTEX) == abi.OK
    radius = C.c_float(1.0)
    assert call(r2=C.cast(C.byref(radius), C.c_void_p)) == abi.OK
    # any non-empty subset of the five outputs — any one will do —, never none
    for mask in range(1, 32):
        sub = {name: (p if mask >> j & 1 else None) for j, name in enumerate(outputs)}
        assert call(**sub) == abi.OK, sub
    for nq in (0, 5):
        assert call(index=None, nq=nq) == abi.ERR_INVALID_ARG          # no output at all
        for skip in (2, 3, -1, 8):                                     # only bit 0
            assert call(skip=skip, nq=nq) == abi.ERR_INVALID_ARG, skip
    for bad in (dict(bvh=None), dict(nt=-1), dict(nq=-1), dict(tris=None), dict(nq=5, q=None),
                dict(bvh=_fake_bvh(leaves=None)), dict(bvh=_fake_bvh(nodes=None)), dict(bvh=_fake_bvh(built_level=0)),
                dict(bvh=_fake_bvh(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
    assert call(tris=None, nt=0) == abi.OK and call(q=None) == abi.OK
    assert call(bvh=_fake_bvh(n=1, nodes=None)) == abi.OK          # a one-leaf tree has no nodes
    broken = _fake_bvh()
    broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # the accepted types, those of closest_points: BBox leaves under BBox nodes of the same or a wider float type, any index type
    for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64)):
        assert call(bvh=_fake_bvh(**good)) == abi.OK, good
    for bad in (dict(leaf_kind=abi.BSPHERE), dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE), dict(node_kind=abi.BSPHERE),
                dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
        # (with queries to process too: refused, never launched on the fake pointers)
        assert call(bvh=_fake_bvh(**bad)) == abi.ERR_UNSUPPORTED and call(bvh=_fake_bvh(**bad), nq=5) == abi.ERR_UNSUPPORTED, bad
    # the order of the other point-walk entries: the entry's own checks first, the types next, the tree and the pointers last
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE), skip=2) == abi.ERR_INVALID_ARG
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE), index=None) == abi.ERR_INVALID_ARG
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE, leaves=None), tris=None) == abi.ERR_UNSUPPORTED


# ---- the checker: hand-made pairs with known answers ---------------------------------------------------------------------
FLAT = tcc.FLAT                                            # (0,0,0) (1,0,0) (0,1,0)
ABOVE = [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5]                  # FLAT moved up by h = 0.5
OVER_FACE = [0.25, 0.25, 0.5, 0.25, 0.25, 2, 2, 2, 2]      # its vertex a hangs 0.5 over FLAT's face
EDGE_X = [-1, 0, 0, 1, 0, 0, 0, 0, -5]                     # edge ab along x; the rest of it below
EDGE_Y = [0, -1, 1, 0, 1, 1, 0, 0, 6]                      # edge p1p2 along y, 1 above EDGE_X's ab; the rest of it above
AT_ORIGIN = [0, 0, 0, -1, 0, 1, 0, -1, 1]                  # shares the vertex (0,0,0) with FLAT
LINE = [5, 5, 5, 6, 6, 6, 7, 7, 7]                         # zero area: collinear
POINT = [1, 1, 1, 1, 1, 1, 1, 1, 1]                        # zero area: one point
HAND = {   # name: (Q, K, d2, xQ, xK, kind); None = not pinned
    "parallel, offset by h": (FLAT, ABOVE, 0.25, (0, 0, 0), (0, 0, 0.5), 0),
    "a vertex of Q over K's face": (OVER_FACE, FLAT, 0.25, (0.25, 0.25, 0.5), (0.25, 0.25, 0), 0),
    "a vertex of K over Q's face": (FLAT, OVER_FACE, 0.25, (0.25, 0.25, 0), (0.25, 0.25, 0.5), 3),
    "crossed edges, gap 1": (EDGE_X, EDGE_Y, 1.0, (0, 0, 0), (0, 0, 1), 6),
    "crossed edges the other way round": (EDGE_Y, EDGE_X, 1.0, (0, 0, 1), (0, 0, 0), 6),
    "an edge pierces a face": (tcc.PIERCING, FLAT, 0.0, (0.25, 0.25, 0), (0.25, 0.25, 0), 15),
    "a face is pierced by an edge": (FLAT, tcc.PIERCING, 0.0, None, None, 15),
    "boxes overlap, nothing meets": (tcc.DISJOINT, FLAT, 0.25, (0.25, 0.25, 0.5), (0.25, 0.25, 0), 0),
    "a collinear K": (FLAT, LINE, 65.5, (0.5, 0.5, 0), (5, 5, 5), 3),
    "a one-point Q": (POINT, FLAT, 1.5, (1, 1, 1), (0.5, 0.5, 0), 0),
    "a one-point Q against a collinear K": (POINT, LINE, 48.0, (1, 1, 1), (5, 5, 5), 0),
}


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_hand_made_pairs_have_their_known_answers(dt):
    for what, (q, k, d2, xq, xk, kind) in HAND.items():
        g2, gq, gk, gkind = (x[0] for x in tdc.pairs(np.array([q], dt), np.array([k], dt)))
        assert g2 == d2 and gkind == kind, (what, g2, gkind)
        assert xq is None or (gq == np.array(xq, dt)).all(), (what, gq)
        assert xk is None or (gk == np.array(xk, dt)).all(), (what, gk)
        assert g2 > 0 or (gq == gk).all(), what                    # a cut pair's two points are one
    # the segment routine on its degenerate branches: two points, a point against a segment either way, parallel segments
    z, e = np.zeros(3, dt), np.array([2, 0, 0], dt)
    up = np.array([0, 0, 3], dt)
    for (p1, q1, p2, q2), want in (((z, z, up, up), 9), ((z, z, up - e, up + e), 9), ((up - e, up + e, z, z), 9), ((z, e, up, up + e), 9),
                                   ((z, e, up + 2 * e, up + 3 * e), 13)):
        x1, x2, d2 = tdc.closest_on_segments(p1, q1, p2, q2)
        assert d2 == want and ((x1 - x2) ** 2).sum() == want, (p1, q1, p2, q2, d2)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_per_query_rules_shared_vertex_duplicates_radius_and_nan(dt):
    far = [9, 9, 9, 10, 9, 9, 9, 10, 9]
    mesh = np.array([FLAT, far, ABOVE, ABOVE], dt)
    q = np.array([AT_ORIGIN, [0, 0, 1, 1, 0, 1, 0, 1, 1], [np.nan, 0, 0, 1, 0, 0, 0, 1, 0]], dt)
    bf = tdc.brute_force(mesh, q)
    # a shared vertex is distance 0; a query 0.5 above the two copies of ABOVE takes the smaller index; a NaN query has no answer
    assert bf.index.tolist() == [1, 3, 0] and bf.d2.tolist() == [0, 0.25, np.inf] and bf.ties.tolist() == [1, 2, 0]
    assert (bf.point_query[2] == 0).all() and (bf.point_mesh[2] == 0).all() and bf.kind[2] == 0
    # ... with the skip flag the triangle that shares a vertex is no answer: the next one is
    skip = tdc.brute_force(mesh, q, skip_shared=True)
    assert skip.index.tolist() == [3, 3, 0] and 0 < skip.d2[0] < 0.25 and skip.d2[1] == 0.25
    # a radius: d2 <= max_d2, inclusive; limited() is the brute force under a radius
    for r2 in (0.25, 0.2, 0.0, np.inf, -1.0, np.nan):
        lim, cut = tdc.brute_force(mesh, q, max_d2=r2), tdc.limited(bf, r2)
        for field in ("index", "d2", "point_query", "point_mesh", "kind"):
            assert kit.bits(getattr(lim, field)) == kit.bits(getattr(cut, field)), (r2, field)
    assert tdc.brute_force(mesh, q, max_d2=0.25).index.tolist() == [1, 3, 0] and tdc.brute_force(mesh, q, max_d2=0.2).index.tolist() == [1, 0, 0]
    assert tdc.global_minimum(bf) == (0, 1, 1) and tdc.global_minimum(tdc.brute_force(mesh, q[1:])) == (0.25, 1, 3)
    assert tdc.global_minimum(tdc.brute_force(mesh, q[2:])) == (np.inf, 0, 0)
    # a mesh triangle with a NaN vertex has a NaN d2 and never wins
    broken = mesh.copy()
    broken[2, 8] = np.nan
    assert tdc.brute_force(broken, q).index.tolist() == [1, 4, 0]


def test_every_kind_occurs():
    kinds = set()
    for dt in DTYPES:
        kinds |= {int(tdc.pairs(np.array([q], dt), np.array([k], dt))[3][0]) for q, k, *_ in HAND.values()}
        q, k = tdc.random_pairs(dt)
        kinds |= set(tdc.pairs(q, k)[3].tolist())
    assert kinds == set(range(16)), sorted(kinds)


# ---- the checker against an independent float64 certificate ---------------------------------------------------------------
# Measured on these very inputs: the largest deviation of xQ / xK from their triangles, and of the separating gap from |n|, both
# relative to the pair's extent.  The assertions allow four times that: the margin covers other seeds, not other arithmetic.
ON = {np.float32: 1.67e-6, np.float64: 8.15e-15}
GAP = {np.float32: 5.86e-4, np.float64: 9.30e-14}


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_the_points_lie_on_their_triangles_and_their_direction_separates_them_by_the_distance(dt):
    q, k = tdc.random_pairs(dt)
    d2, xq, xk, kind = tdc.pairs(q, k)
    assert not np.isnan(d2).any() and (d2 == 0).sum() >= 200 and ((d2 == 0) == (kind == tdc.CUT)).all()
    pos = d2 > 0
    assert pos.sum() >= 3000
    on, gap = tdc.certificate(q[pos], k[pos], xq[pos], xk[pos])
    print(f"{dt.__name__}: on {on.max():.3e} gap {gap.max():.3e}")
    assert on.max() <= 4 * ON[dt] and gap.max() <= 4 * GAP[dt], (on.max(), gap.max())
    # d2 is the squared length of xQ - xK, in the checker's own arithmetic
    e = xq - xk
    assert ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] == d2).all()
    # and symmetric in value: (K, Q) finds the same distance up to the order of the candidates
    back = tdc.pairs(k, q)[0]
    assert np.allclose(back, d2, rtol=0, atol=4 * GAP[dt] * 4)


# ---- what makes pruning lossless -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_the_bound_of_a_box_never_exceeds_a_distance_under_it(dt):
    rng = np.random.default_rng(47)
    q, k = tdc.random_pairs(dt, n=6000, seed=53)
    # ... and pairs that touch or nearly do: K moved so that its box meets Q's box face to face
    qlo, qup = tcc.fold_box(q)
    klo, kup = tcc.fold_box(k)
    shift = np.zeros((len(q), 3), dt)
    axis = rng.integers(0, 3, len(q))
    rows = np.arange(len(q))
    shift[rows, axis] = (qup - klo)[rows, axis]
    touching = (k[:2000].reshape(-1, 3, 3) + shift[:2000, None, :]).reshape(-1, 9).astype(dt)
    q, k = np.concatenate([q, q[:2000]]), np.concatenate([k, touching])
    d2, _, _, kind = tdc.pairs(q, k)
    assert (kind == tdc.CUT).sum() >= 300 and (d2 > 0).sum() >= 5000
    qlo, qup = tcc.fold_box(q)
    klo, kup = tcc.fold_box(k)
    assert ((klo == qup).any(axis=1)).sum() >= 500                  # boxes that touch exactly
    grow = lambda scale: (klo - (scale * rng.random(klo.shape)).astype(dt), kup + (scale * rng.random(kup.shape)).astype(dt))
    other_lo, other_up = tcc.fold_box(rng.random((len(q), 9)).astype(dt) * 3 - 1)
    boxes = {"K's own box": (klo, kup), "a skin": grow(1e-3), "a leaf's parent": grow(0.3), "near the root": grow(3.0),
             "merged with another box": (np.where(other_lo < klo, other_lo, klo), np.where(other_up > kup, other_up, kup)),
             "grown as far as Q's box": (np.where(qup < klo, qup, klo), np.where(qlo > kup, qlo, kup))}
    for what, (lo, up) in boxes.items():
        assert (lo <= klo).all() and (up >= kup).all()
        lb = tdc.box_bound(lo, up, qlo, qup)
        assert (lb <= d2).all(), (what, int((lb > d2).sum()))        # exact: no tolerance
        assert (lb[kind == tdc.CUT] == 0).all(), what                # a cut pair's boxes are not apart
    own = tdc.box_bound(klo, kup, qlo, qup)
    assert (own > 0).sum() >= 2000 and (own == d2).sum() >= 1        # the bound bites, and is attained


# ---- the GPU test's conditions, on the brute force alone ------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_mesh_queries_meet_the_gpu_tests_conditions(dt):
    tris, queries, bf = tdc.reference("torus40", dt)
    assert tris.shape == (3200, 9) and queries.shape == (600, 9) and (bf.index != 0).all()
    third = slice(0, 200), slice(200, 400), slice(400, 600)
    assert (bf.d2[third[0]] == 0).sum() >= 100 and (bf.kind[third[0]] == tdc.CUT).sum() >= 100      # cutting
    assert (bf.d2[third[1]] > 0).all() and bf.d2[third[1]].max() < 2                                # clear of it, near
    assert bf.d2[third[2]].min() > 1000                                                              # far away
    assert len(set(bf.kind.tolist())) >= 10 and bf.ties.max() >= 2
    # closest_points on the queries' vertices is not this query: it misses the cuts and the edge pairs
    assert ((bf.kind >= 3) & (bf.kind != tdc.CUT)).sum() >= 30
