"""ibvh_triangle_contacts on the host side: the header declares it (additive under ABI version 7) and carries its contract, the
ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its one
launch goes through the profiling wrapper, the edge-against-triangle test it shares with the ray queries exists once, and
the entry point validates its arguments — the refused type combinations included — before any launch, in the documented
order.  The numpy checker the GPU test pins the kernel to (tests/triangle_contacts_checker.py) does what its definition says
on hand-made pairs, and the GPU test's non-vacuity conditions hold for the brute force alone.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib
from implicitbvh_amd.synthetic import torus_mesh

import mesh_query_kit as kit
import triangle_contacts_checker as tcc
from mesh_query_kit import MESHES, bits as _bits

NAME = "ibvh_triangle_contacts"
UNIT = "ibvh_tritri.hip"
SHARED = "ibvh_raytest.hpp"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)


# ---- 1. the header -----------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *queries", "const void *query_ids",
                    "int64_t num_queries", "int32_t mode", "int32_t skip", "void *counts", "const void *offsets", "int64_t capacity",
                    "void *contact_index", "void *contact_mask", "void *contact_points", "void *flag", "void *stream"]
    assert "ibvh_triangle_contacts and IBVH_TRIS_COUNT / IBVH_TRIS_WRITE (additive under 7 likewise: one more entry point)" in note
    assert re.search(r"enum \{ IBVH_TRIS_COUNT = 0, IBVH_TRIS_WRITE = 1 \};", hdr)
    assert re.search(r"enum \{ IBVH_TRIS_SKIP_SHARED_VERTEX = 1 \};", hdr)
    assert (abi.TRIS_COUNT, abi.TRIS_WRITE, abi.TRIS_SKIP_SHARED_VERTEX) == (0, 1, 1)
    # the doc comment carries the contract: the six tests and their bits, the box clause, NaN, the order, rows, the guards
    doc = raw[raw.index("triangle-vs-mesh contacts: every mesh triangle each query triangle cuts"):raw.index("ibvh_status " + NAME)]
    doc = " ".join(doc.replace("\n *", "\n").split())
    for phrase in ("bit 0 a -> b against K bit 3 p1 -> p2 against Q", "bit 1 b -> c against K bit 4 p2 -> p3 against Q",
                   "bit 2 c -> a against K bit 5 p3 -> p1 against Q", "d = P1 - P0", "AND t <= 1", "`x < m ? x : m` / `x > m ? x : m`",
                   "qup_k < lo_k || qlo_k > up_k", "six strict comparisons, each false on NaN", "A NaN box is entered",
                   "!apart(K's stored leaf box)", "mask != 0", "index > query_ids[i]", "== on all three coordinates, over the nine vertex pairs",
                   "P0 + t * d of the LOWEST set bit", "that of the HIGHEST set bit", "one rounded product and one rounded sum",
                   "exactly two bits are set", "A query with a NaN coordinate has NO contacts", "LEAF ORDER", "ascending position",
                   "bvh->leaves", "row offsets[i] + j", "need NOT be monotone", "A row >= capacity or < 0 is never written",
                   "bit 2 of `flag` (value 4)", "bit 1 of `flag` (value 2)", "BOTH passes alike", "ANY exclusive prefix sum",
                   "The scan is the caller's", "counts[i] = the number of contacts", "x int64", "uint8", "capacity x 2 x 3 x flt",
                   "at least one non-NULL", "any bit of `skip` other than bit 0", "IBVH_ERR_INVALID_ARG", "IBVH_ERR_UNSUPPORTED",
                   "num_queries == 0", "skin margin", "ibvh_refit", "No reference counterpart", "Coplanar pairs have det == 0 in all six tests",
                   "never contacts", "rounding noise", "depend on rounding", "The decision is symmetric", "bits 0-2 and 3-5 exchanged",
                   "only removes ghosts of rounding", "has only leaves that are apart from Q", "nothing fused"):
        assert phrase in doc, phrase
    # the refusals come in the documented order: the entry's own, the types, the tree and the arrays
    order = [doc.index(x) for x in ("The entry's own checks", "Then the type combination", "Then a tree shape")]
    assert order == sorted(order)


# ---- 2. bindings and source --------------------------------------------------------------------------------------------
def test_binding_table_makefile_launch_and_python_surface():
    want = ([C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
             C.c_int64] + [C.c_void_p] * 5)
    assert lib.SIGNATURES[NAME] == want
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("triangle_contacts", "TriangleContacts", "self_intersections"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    src = kit.query_unit(UNIT, "tritri::tritri_walk_kernel", lists=True)
    # one kernel template for both passes, the pass a template parameter reached through the two bool types — which the shared
    # header spells, once, with the rest of the two-pass protocol (kit.PROTOCOL, checked by query_unit)
    assert len(re.findall(r"__global__", src)) == 1 and "template <class T, class TN, class I, bool WRITE>" in src
    # the crossings query's way of keeping leaf order: a 0 / 1 bound under a constant limit of 0
    assert src.count("return trigeom::apart(qlo, qup, lo, up) ? T(1) : T(0);") == 1 and "[]() { return T(0); }" in src
    assert src.count("trigeom::triangle_box(Q.v, qlo, qup);") == 1
    assert src.count("if ((skip & IBVH_TRIS_SKIP_SHARED_VERTEX) && trigeom::shares_vertex(Q.v, K.v)) return;") == 1
    assert "raise_flag(flag, 4u)" in src and "skip & ~IBVH_TRIS_SKIP_SHARED_VERTEX" in src
    # the six tests name their vertices statically, in the documented order
    calls = re.findall(r"^\s*seg\(([^;]*)\);", src, flags=re.M)
    assert calls == ["Q.v, Q.v + 3, K, 1u", "Q.v + 3, Q.v + 6, K, 2u", "Q.v + 6, Q.v, K, 4u", "K.v, K.v + 3, Q, 8u", "K.v + 3, K.v + 6, Q, 16u",
                     "K.v + 6, K.v, Q, 32u"]
    # each is the shared cut test — the ray test with d = p1 - p0, t <= 1, the point p0 + t d — and the count pass's early-out
    # stays around the call
    seg = src[src.index("auto seg = [&]"):src.index("seg(Q.v, Q.v + 3, K, 1u);")]
    assert seg.index("if (!WRITE && mask != 0) return;") < seg.index("if (trigeom::segment_cuts(tri, p0, p1, x)) {") and src.count("trigeom::segment_cuts(") == 1
    geom = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_trigeom.hpp")
    cut = geom[geom.index("IBVH_D bool segment_cuts("):]
    for line in ("const T d[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};", "& (t <= T(1))", "x[k] = p0[k] + t * d[k];", "WRITE"):
        assert (line in cut) == (line != "WRITE"), line


def test_the_edge_test_exists_once_and_the_unit_includes_it():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    for define in (r"\bbool ray_triangle\s*\([^)]*\)\s*\{", r"\bvoid cross3\s*\([^)]*\)\s*\{"):
        assert [f for f in sources if re.search(define, kit.read("implicitbvh.jl_amd", "csrc", f))] == [SHARED], define
    text = kit.read("implicitbvh.jl_amd", "csrc", UNIT)
    assert re.search(r'^#include "' + SHARED + '"$', text, flags=re.M) and "ray_triangle(" not in text
    geom = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_trigeom.hpp")
    assert re.search(r'^#include "ibvh_trigeom.hpp"$', text, flags=re.M) and re.search(r'^#include "' + SHARED + '"$', geom, flags=re.M)
    assert geom.count("raytri::ray_triangle(tri, p0, d, t, u, v)") == 1
    assert "cross3" not in text and "dot3" not in text
    import __graft_entry__ as entry
    assert {os.path.join(csrc, SHARED), os.path.join(csrc, UNIT)} <= set(entry.kernel_sources(kit.ROOT))


# ---- 3. Julia and the documents ----------------------------------------------------------------------------------------
def test_julia_wrapper_binds_it_and_the_documents_describe_it():
    src = kit.julia_ccall(NAME, "triangle_contacts")
    body = src[src.index("function triangle_contacts("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_TRIS_COUNT" in body and "IBVH_TRIS_WRITE" in body and ("cumsum" in body or "accumulate" in body)
    assert "function self_intersections(" in src and "function ImplicitBVH.self_intersections" not in src
    assert len(re.findall(r"function ImplicitBVH\.", src)) == 7
    design = kit.read("DESIGN.md")
    title = "Triangle-vs-mesh contacts (`ibvh_tritri.hip`) — no reference counterpart"
    assert design.count(title) == 1
    assert design.index("### Sphere-vs-mesh contacts") < design.index("### " + title) < design.index("### BFS traversal")
    section = design[design.index(title):design.index("### BFS traversal")]
    for phrase in ("lossless", "leaf order", "six", "t <= 1", "VGPR", "scratch", "tools/kernel_meta.py", "tools/bench_triangle_contacts.py",
                   "ms", "coplanar"):
        assert phrase in section, phrase
    assert "ibvh_triangle_contacts" in kit.read("README.md") and "triangle_contacts" in kit.read("INTEGRATION.md")
    tool = kit.read("tools", "bench_triangle_contacts.py")
    assert "same_pairs_as_library" in tool and "self_intersections" in tool and "traverse(" in tool
    assert "bench_triangle_contacts.py" in kit.read("tools", "README.md")


# ---- 4. argument validation --------------------------------------------------------------------------------------------
def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    count = dict(bvh=_fake_bvh(), tris=p, nt=5, q=p, ids=None, nq=0, mode=abi.TRIS_COUNT, skip=0, counts=p, offsets=None, cap=0, ci=None,
                 cm=None, cp=None, flag=None, stream=None)
    write = dict(count, mode=abi.TRIS_WRITE, counts=None, offsets=p, cap=7, ci=p)

    def call(base, **kw):
        a = dict(base, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["q"], a["ids"], a["nq"], a["mode"], a["skip"], a["counts"], a["offsets"], a["cap"], a["ci"],
                 a["cm"], a["cp"], a["flag"], a["stream"])
    kit.check_two_pass_arguments(call, count, write, p, "nq", ("ci", "cm", "cp"), needs=("q",), absent=dict(q=None), fake=_fake_bvh)
    # what is this query's own: the optional ids, and `skip`, any bit of which other than bit 0 is refused
    assert call(count, ids=p) == abi.OK and call(write, ids=p) == abi.OK
    assert call(count, skip=1) == abi.OK and call(write, skip=abi.TRIS_SKIP_SHARED_VERTEX) == abi.OK
    for skip in (2, 3, 4, -1, 1 << 30):
        assert call(count, skip=skip) == abi.ERR_INVALID_ARG and call(write, skip=skip) == abi.ERR_INVALID_ARG, skip
    for base in (count, write):   # ... among the entry's own checks, which come before the types
        assert call(base, bvh=_fake_bvh(leaf_kind=abi.BSPHERE), skip=2, nq=5) == abi.ERR_INVALID_ARG
        assert call(base, bvh=_fake_bvh(leaf_kind=abi.BSPHERE), cap=-1, nq=5) == abi.ERR_INVALID_ARG
        assert call(base, bvh=_fake_bvh(leaf_float=abi.F64, node_float=abi.F32, built_level=0), q=None, nq=5) == abi.ERR_UNSUPPORTED


# ---- 5. the checker on hand-made pairs ---------------------------------------------------------------------------------
from triangle_contacts_checker import COPLANAR, DISJOINT, FAR, FLAT, PIERCING, TOUCHING  # noqa: E402  (the hand-made triangles)


def _pair(q, k, dt, **kw):
    """the contacts of the one query q with the one-triangle mesh k -> (mask or None, points or None)"""
    bf = tcc.brute_force(np.array([k], dt), np.array([q], dt), **kw)
    assert bf.counts.tolist() == [len(bf.index)] and len(bf.index) <= 1 and (bf.index == 1).all()
    return (int(bf.mask[0]), bf.points[0].tolist()) if len(bf.index) else (None, None)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_checker_follows_its_definition_on_hand_made_pairs(dt):
    # a piercing pair: exact mask and points, and the other order with bits 0-2 and 3-5 exchanged
    assert _pair(PIERCING, FLAT, dt) == (1 | 16, [[0.25, 0.25, 0], [0.5, 0.5, 0]])
    assert _pair(FLAT, PIERCING, dt) == (2 | 8, [[0.5, 0.5, 0], [0.25, 0.25, 0]])
    assert tcc.swap_mask(1 | 16) == 2 | 8 and tcc.swap_mask(tcc.swap_mask(np.arange(64))).tolist() == list(range(64))
    # touching at a vertex: both of the query's edges at that vertex find it (t = 0 and t = 1), at the same point
    assert _pair(TOUCHING, FLAT, dt) == (1 | 4, [[0.25, 0.25, 0]] * 2)
    assert _pair(FLAT, TOUCHING, dt) == (8 | 32, [[0.25, 0.25, 0]] * 2)
    # coplanar and overlapping: det == 0 in all six tests; disjoint; boxes apart
    for q in (COPLANAR, FLAT, DISJOINT, FAR):
        assert _pair(q, FLAT, dt) == (None, None) and _pair(FLAT, q, dt) == (None, None), q
    # a NaN coordinate in the query: nothing; in the mesh triangle: only through the edge between its two other vertices
    for k in range(9):
        q = list(PIERCING)
        q[k] = np.nan
        assert _pair(q, FLAT, dt) == (None, None), k
    assert _pair(PIERCING, [np.nan, 0, 0, 1, 0, 0, 0, 1, 0], dt) == (16, [[0.5, 0.5, 0]] * 2)
    assert _pair(PIERCING, [0, 0, 0, 1, np.nan, 0, 0, 1, 0], dt) == (None, None)
    # the box clause is part of the definition: a stored box that is apart from the query's hides the triangle
    away = np.array([[0, 0, 1.5, 1, 1, 2]], dt)
    assert _pair(PIERCING, FLAT, dt, leaf_boxes=away) == (None, None)
    assert _pair(PIERCING, FLAT, dt, leaf_boxes=np.array([[-1, -1, -1, 2, 2, 1]], dt))[0] == 17
    assert _pair(PIERCING, FLAT, dt, leaf_boxes=np.array([[np.nan] * 6], dt))[0] == 17   # a NaN box is entered
    # shared-vertex neighbours: two triangles hinged on an edge touch along it, unless skipped
    hinge = [0, 0, 0, 1, 0, 0, 0.5, 0.5, 1]
    mask, _ = _pair(hinge, FLAT, dt)
    assert mask is not None and _pair(hinge, FLAT, dt, skip_shared=True) == (None, None)
    assert _pair(FLAT, hinge, dt)[0] == int(tcc.swap_mask(mask)) and _pair(FLAT, hinge, dt, skip_shared=True) == (None, None)
    assert _pair(PIERCING, FLAT, dt, skip_shared=True)[0] == 17
    one_corner = [0, 1, 0, -1, 2, 1, -1, 2, -1]
    assert _pair(one_corner, FLAT, dt, skip_shared=True) == (None, None)
    # query_ids: only triangles whose index exceeds the query's id; lists in leaf order
    tris = np.array([FLAT, [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5], FAR, [0, 0, -0.5, 1, 0, -0.5, 0, 1, -0.5]], dt)
    q = np.array([PIERCING] * 5, dt)
    bf = tcc.brute_force(tris, q, query_ids=np.array([0, 1, 2, 4, 9]), idt=np.int32)
    assert bf.index.tolist() == [1, 2, 4, 2, 4, 4] and bf.counts.tolist() == [3, 2, 1, 0, 0] and bf.index.dtype == np.int32
    assert bf.query.tolist() == [0, 0, 0, 1, 1, 2] and bf.offsets.tolist() == [0, 3, 5, 6, 6, 6] and bf.mask.dtype == np.uint8
    back = tcc.brute_force(tris, q[:1], leaf_order=[4, 9, 2, 3, 1, 0])
    assert back.index.tolist() == [4, 2, 1] and back.points[:, 0, 2].tolist() == [-0.5, 0.5, 0]
    assert tcc.in_leaf_order(tcc.brute_force(tris, q[:1]), [4, 2, 3, 1]).index.tolist() == [4, 2, 1]
    assert tcc.brute_force(tris[:0], q).counts.tolist() == [0] * 5 and tcc.brute_force(tris, q[:0]).offsets.tolist() == [0]
    assert tcc.brute_force(tris, q.reshape(-1, 3, 3)).index.tolist() == [1, 2, 4] * 5


# ---- 6. non-vacuity ----------------------------------------------------------------------------------------------------
EXPECTED = {"torus40": dict(pairs=384, split=(3016, 67, 117), longest=6, per_bit=[152, 124, 108, 152, 120, 112], slicers=[153, 160, 172]),
            "torus64x63": dict(pairs=610, split=(7767, 104, 193), longest=7, per_bit=[240, 192, 176, 246, 192, 174], slicers=[261, 252, 276])}


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_query_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh, dt):
    tris = torus_mesh(*MESHES[mesh]).astype(dt)
    q = tcc.pipeline_queries(tris)
    assert q.shape == (len(tris) + 3, 9) and q.dtype == dt and _bits(q[3:]) == _bits(tcc.other(tris))
    bf = tcc.brute_force(tris, q)
    nv = tcc.non_vacuity(bf)
    print(f"{mesh} {np.dtype(dt).name}: {nv}")
    tcc.assert_non_vacuous(nv)
    # the figures of the other mesh against this one, and of the three slicing triangles
    e = EXPECTED[mesh]
    rest = bf.query >= 3
    counts = bf.counts[3:]
    assert int(rest.sum()) == e["pairs"] and bf.counts[:3].tolist() == e["slicers"]
    assert (int((counts == 0).sum()), int((counts == 1).sum()), int((counts >= 2).sum())) == e["split"] and int(counts.max()) == e["longest"]
    assert [int(((bf.mask[rest] >> b) & 1).sum()) for b in range(6)] == e["per_bit"]
    assert nv["two_bits"] == nv["pairs"]   # general position: always exactly two set bits
    # a permuted leaf order permutes each list and nothing else
    perm = np.random.default_rng(5).permutation(len(tris)) + 1
    moved = tcc.brute_force(tris, q, leaf_order=perm)
    assert (moved.counts == bf.counts).all() and (moved.index != bf.index).any()
    rank = np.empty(len(tris) + 1, np.int64)
    rank[perm] = np.arange(len(tris))
    resort = np.lexsort((moved.index, moved.query))
    assert (moved.index[resort] == bf.index).all() and _bits(moved.points[resort]) == _bits(bf.points) and (moved.mask[resort] == bf.mask).all()
    assert (np.diff(rank[moved.index])[np.diff(moved.query) == 0] > 0).all()
    again = tcc.in_leaf_order(bf, perm)
    assert (again.index == moved.index).all() and _bits(again.points) == _bits(moved.points)


def test_self_test_of_two_tori_in_one_mesh():
    tris = torus_mesh(*MESHES["torus40"])
    both = np.concatenate([tris, tcc.other(tris)])
    n = len(both)
    every = tcc.brute_force(both, both)
    skipped = tcc.brute_force(both, both, skip_shared=True)
    once = tcc.brute_force(both, both, skip_shared=True, query_ids=np.arange(1, n + 1))
    assert (len(every.index), len(skipped.index), len(once.index)) == (82899, 768, 384)
    assert ((once.query < n // 2) & (once.index > n // 2)).all()        # every one across the two tori
    # a triangle is coplanar with itself, but its computed det is rounding noise, not 0: the arithmetic alone does not keep it
    # from meeting itself (or its neighbours) — the shared-vertex rule and the ids do
    assert (every.query + 1 == every.index).any() and not (skipped.query + 1 == skipped.index).any()
    # the decision is symmetric: both directions, bits 0-2 and 3-5 exchanged
    there = {(int(a) + 1, int(b)): int(m) for a, b, m in zip(skipped.query, skipped.index, skipped.mask)}
    assert len(there) == 768 and all(there[(b, a)] == int(tcc.swap_mask(m)) for (a, b), m in there.items())
    assert sorted(k for k in there if k[0] < k[1]) == sorted(zip((once.query + 1).tolist(), once.index.tolist()))
