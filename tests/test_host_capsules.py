"""ibvh_capsule_contacts and ibvh_segment_distances on the host side: the header declares both (additive under ABI version 7)
and carries their contract, the ctypes table and the Julia extension bind them with the same argument kinds, the Makefile
builds their translation units, each unit's one launch goes through the profiling wrapper on the shared walk, the
segment-triangle evaluation lives once in a header of its own, and the entry points validate their arguments before any
launch.  The numpy checker the GPU tests pin the kernels to (tests/capsule_checker.py): it gives the known answers on hand-made
pairs of every kind, follows the per-capsule rules, agrees with its own Float64 evaluation within a measured deviation, the
computed gap of a box never exceeds a computed d2 under it and the slab clause is monotone up a chain of boxes (what makes
pruning lossless), and the GPU tests' conditions hold for the brute force alone.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib

import capsule_checker as cc
import mesh_query_kit as kit
import triangle_contacts_checker as tcc
import triangle_distance_checker as tdc

CONTACTS, DISTANCES = "ibvh_capsule_contacts", "ibvh_segment_distances"
UNITS = {CONTACTS: "ibvh_capsules.hip", DISTANCES: "ibvh_segdist.hip"}
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_both_entry_points_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(CONTACTS)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *starts", "const void *ends",
                    "const void *radii", "int64_t num_capsules", "int32_t mode", "void *counts", "const void *offsets", "int64_t capacity",
                    "void *contact_index", "void *contact_d2", "void *contact_point_segment", "void *contact_point_mesh",
                    "void *contact_kind", "void *flag", "void *stream"]
    assert kit.header_prototype(DISTANCES)[2] == [
        "const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *starts", "const void *ends",
        "int64_t num_segments", "const void *max_distance2", "void *closest_index", "void *closest_d2", "void *point_segment",
        "void *point_mesh", "void *closest_kind", "void *flag", "void *stream"]
    flat = " ".join(note.replace("*", " ").split())
    assert "ibvh_capsule_contacts and IBVH_CAPSULES_COUNT / IBVH_CAPSULES_WRITE, ibvh_segment_distances (additive under 7" in flat
    assert re.search(r"enum \{ IBVH_CAPSULES_COUNT = 0, IBVH_CAPSULES_WRITE = 1 \};", hdr)
    join = lambda text: re.sub(r"\n \*\s+", " ", text)        # (the comment's lines joined: a phrase may run over a line end)
    doc = join(raw[raw.index("capsule-vs-mesh contacts: every triangle within r"):raw.index("ibvh_status " + CONTACTS)])
    for phrase in ("The CUT rule", "not apart", "six strict comparisons", "p = a, d = b - a", "t <= 1", "d2 = 0", "kind = 5",
                   "The CANDIDATE rule", "five candidates", "strictly smaller", "kind 0, 1", "kind 2, 3, 4", "p1->p2, p2->p3, p3->p1",
                   "the evaluation of ibvh_closest_triangles", "clamped into S's box", "NOT reported", "the SLAB clause", "entry <= 1",
                   "STORED box grown by r", "lo_k - r, up_k + r", "the DISTANCE clause", "d2 <= r2", "(ii) implies (i)",
                   "prune on it without loss", "!(r >= 0)", "NaN", "length zero is valid", "LEAF ORDER", "lossless WITHOUT an epsilon",
                   "S's box in place of Q's", "monotone", "ancestors that pass", "IBVH_CAPSULES_COUNT or IBVH_CAPSULES_WRITE",
                   "bit 2", "value 4", "bit 1", "value 2", "IBVH_ERR_UNSUPPORTED", "IBVH_ERR_INVALID_ARG", "num_capsules == 0",
                   "No reference counterpart", "ONE launch each", "every comparison false on NaN", "skin margin", "ibvh_refit"):
        assert phrase in doc, phrase
    doc = join(raw[raw.index("segment-to-mesh distance: the closest mesh triangle"):raw.index("ibvh_status " + DISTANCES)])
    for phrase in ("LEXICOGRAPHIC MINIMUM of (d2, index)", "ALL mesh triangles", "d2 <= max_distance2", "inclusive", "NO slab clause",
                   "segment-triangle evaluation of ibvh_capsule_contacts", "tie rule of ibvh_closest_triangles", "HOST pointer",
                   "at least one non-NULL", "0 = none", "+Inf = none", "candidate 0 of the pair (S, F)", "strictly",
                   "OWN box, not the stored one", "ONE launch", "num_segments == 0", "NaN coordinate", "never wins"):
        assert phrase in doc, phrase


def test_binding_tables_makefile_launches_and_python_surface():
    vp = C.c_void_p
    assert lib.SIGNATURES[CONTACTS] == abi.CAPSULE_CONTACTS_ARGTYPES == (
        [C.POINTER(abi.Bvh), vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, C.c_int64] + [vp] * 7)
    assert lib.SIGNATURES[DISTANCES] == abi.SEGMENT_DISTANCES_ARGTYPES == [C.POINTER(abi.Bvh), vp, C.c_int64, vp, vp, C.c_int64] + [vp] * 8
    assert (abi.CAPSULES_COUNT, abi.CAPSULES_WRITE) == (0, 1) and abi.SEGTRI_CUT == cc.CUT == 5
    for name in (CONTACTS, DISTANCES):
        assert hasattr(lib.load(), name), "libibvh.so exports " + name
    for name in ("capsule_contacts", "CapsuleContacts", "segment_distances", "SegmentDistances"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    assert issubclass(ibvh.CapsuleContacts, ibvh.api._ContactLists) and ibvh.CapsuleContacts.ENTRY == (CONTACTS, 0, 1)
    # the contacts: the shared walk once, the shared count / write protocol, the pass as a template parameter
    src = kit.query_unit(UNITS[CONTACTS], "capsules::capsules_walk_kernel", lists=True)
    assert len(re.findall(r"__global__", src)) == 1 and "template <class T, class TN, class I, bool WRITE>\n__global__" in src
    assert "fma" not in src and "[]() { return T(0); }" in src and "mode == IBVH_CAPSULES_WRITE" in src
    slab = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_slab.hpp")   # (the box grown by r: the ONE grown entry, the sweep's too)
    assert slab.count("const T glo[3] = {lo[0] - r, lo[1] - r, lo[2] - r}, gup[3] = {up[0] + r, up[1] + r, up[2] + r};\n    return slab_entry(glo, gup, p, d, inv);") == 1
    for line in ("trigeom::box_gap(lo, up, slo, sup)", "slab::grown_entry(lo, up, r, a, d, inv)", "(gap > r2) | (entry > T(1))",
                 "if (p.d2 <= r2) {", "const T inv[3] = {T(1) / d[0], T(1) / d[1], T(1) / d[2]};",
                 "(r >= T(0)) && !pointwalk::hopeless(a, r2) && !pointwalk::hopeless(b, r2)"):
        assert line in src, line
    # the distances: two walks, the first from the end a on the shared point-box bound, which seeds the limit of the second
    src = kit.query_unit(UNITS[DISTANCES], "segdist::segdist_walk_kernel", walks=2, pair=True)
    assert len(re.findall(r"__global__", src)) == 1 and "template <class T, class TN, class I>\n__global__" in src
    assert "fma" not in src and "slab" not in src.replace("no slab", "")
    # (the shared lane routine, kit.pair_routine: checked by query_unit) from the end a — the point candidate 0 is evaluated from
    assert src.count("nodes, nan, a, max_d2, box, gather, pair, best);") == 1 and src.count("trigeom::box_gap(lo, up, slo, sup)") == 1
    assert src.count("const bool nan = pointwalk::hopeless(a, max_d2) || pointwalk::hopeless(b, max_d2);") == 1
    seg = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_segtri.hpp")
    assert seg.index("if (c == 0) r.put(d2, p, x, 0);") < seg.index("else r.offer(d2, p, x, 1);") and "sel(c == 0, a[0], b[0])" in seg
    header = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    assert len(re.findall(r"static_assert\(IBVH_CAPSULES_COUNT == 0 && IBVH_CAPSULES_WRITE == 1,", header)) == 1
    assert "ibvh_capsules.hip" in header[:header.index("#pragma once")] and "ibvh_segdist.hip" in header[:header.index("#pragma once")]


def test_the_segment_triangle_evaluation_exists_once_and_both_units_include_it():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    text = {f: kit.read("implicitbvh.jl_amd", "csrc", f) for f in sources}
    assert [f for f in sources if "namespace segtri" in text[f]] == ["ibvh_segtri.hpp"]
    seg = text["ibvh_segtri.hpp"]
    geom = text["ibvh_trigeom.hpp"]
    assert len(re.findall(r"IBVH_D void evaluate\(", seg)) == 1 and len(re.findall(r"IBVH_D T box_gap\(", geom)) == 1 and "box_gap" not in seg
    for unit in UNITS.values():
        assert re.search(r'^#include "ibvh_segtri.hpp"$', text[unit], flags=re.M), unit
        assert text[unit].count("segtri::evaluate(a, b, slo, sup, K, ") == 1 and text[unit].count("segtri::segment_box(a, b, slo, sup)") == 1
        assert "closest_on_segments" not in text[unit] and "ray_triangle" not in text[unit]
    # it is built from the one copy of each piece, the cut rule under the box clause first, the candidates rolled
    for home in ("ibvh_pointtri.hpp", "ibvh_raytest.hpp", "ibvh_segseg.hpp", "ibvh_trigeom.hpp"):
        assert re.search(r'^#include "' + home + '"$', seg, flags=re.M), home
    assert seg.count("pointtri::closest_on_triangle(") == seg.count("segseg::closest_on_segments(") == seg.count("trigeom::segment_cuts(K, a, b, ") == 1
    assert "ray_triangle(" not in seg and geom.count("raytri::ray_triangle(tri, p0, d, t, u, v) & (t <= T(1))") == 1
    assert seg.index("const bool apart = trigeom::apart(slo, sup, klo, kup);") < seg.index("if (!apart) {") < seg.index("trigeom::segment_cuts(")
    assert seg.index("trigeom::segment_cuts(") < seg.index("pointtri::closest_on_triangle(")
    assert seg.index("pointtri::closest_on_triangle(") < seg.index("segseg::closest_on_segments(a, b, p2, q2, x, y)")
    assert seg.count("#pragma unroll 1") == 2 and "fma" not in seg and "1e-" not in seg
    for line in ("lo[k] = a[k] < b[k] ? a[k] : b[k];", "up[k] = a[k] > b[k] ? a[k] : b[k];", "constexpr int kCut = 5;",
                 "trigeom::edge_of(K.v, c, p2, q2);"):
        assert line in seg, line
    # ... the pair and the gap, with the query's box where S's stood: the one copy, ibvh_trigeom.hpp's
    for line in ("if (d < d2) put(d, q, k, c);", "const T below = lo[k] - qup[k], above = qlo[k] - up[k];", "const T m = below > above ? below : above;",
                 "g[k] = m > T(0) ? m : T(0);", "return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];"):
        assert geom.count(line) == 1 and line not in seg, line
    assert "NOT reported" in seg and "does not classify" in seg
    import __graft_entry__ as entry
    assert {os.path.join(csrc, f) for f in ("ibvh_segtri.hpp",) + tuple(UNITS.values())} <= set(entry.kernel_sources(kit.ROOT))


def test_julia_wrappers_bind_them_with_the_ctypes_signatures_and_the_docs_name_them():
    src = kit.julia_ccall(CONTACTS, "capsule_contacts")
    assert kit.julia_ccall(DISTANCES, "segment_distances") == src
    body = src[src.index("function capsule_contacts("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_CAPSULES_COUNT" in body and "IBVH_CAPSULES_WRITE" in body and "cumsum" in body and "point_morton_order(" in body
    body = src[src.index("function segment_distances("):]
    assert "point_morton_order((starts .+ ends) ./ T(2))" in body[:body.index("\nend\n")]
    design = kit.read("DESIGN.md")
    for title in ("Capsule-vs-mesh contacts", "Segment-to-mesh distance"):
        section = design[design.index(title):][:9000]
        for phrase in ("no reference counterpart", "lossless", "VGPRs", "scratch"):
            assert phrase in section, (title, phrase)
    section = design[design.index("Capsule-vs-mesh contacts"):][:9000]
    assert "leaf order" in section and "slab clause" in section and "certificate" in section
    assert len(re.findall(r"^\| `<(?:float|double), (?:float|double), (?:int|long)(?:, (?:count|write))?>` \|", design[design.index("Capsule-vs-mesh contacts"):], flags=re.M)) >= 18
    assert kit.read("tools", "bench_capsules.py") and "bench_capsules.py" in kit.read("tools", "README.md")


def test_contacts_entry_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), CONTACTS)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    count = dict(bvh=_fake_bvh(), tris=p, nt=5, a=p, b=p, r=p, nc=0, mode=abi.CAPSULES_COUNT, counts=p, offsets=None, cap=0, ci=None,
                 cd=None, cs=None, cm=None, ck=None, flag=None, stream=None)
    write = dict(count, mode=abi.CAPSULES_WRITE, counts=None, offsets=p, cap=7, ci=p)

    def call(base, **kw):
        x = dict(base, **kw)
        bvh = C.byref(x["bvh"]) if x["bvh"] is not None else None
        return f(bvh, x["tris"], x["nt"], x["a"], x["b"], x["r"], x["nc"], x["mode"], x["counts"], x["offsets"], x["cap"], x["ci"], x["cd"],
                 x["cs"], x["cm"], x["ck"], x["flag"], x["stream"])
    kit.check_two_pass_arguments(call, count, write, p, "nc", ("ci", "cd", "cs", "cm", "ck"), needs=("a", "b", "r"),
                                 absent=dict(a=None, b=None, r=None), fake=_fake_bvh)


def test_distances_entry_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), DISTANCES)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    ok = dict(bvh=_fake_bvh(), tris=p, nt=5, a=p, b=p, ns=0, r2=None, index=p, d2=None, xs=None, xk=None, kind=None, flag=None, stream=None)
    outputs = ("index", "d2", "xs", "xk", "kind")

    def call(**kw):
        x = dict(ok, **kw)
        bvh = C.byref(x["bvh"]) if x["bvh"] is not None else None
        return f(bvh, x["tris"], x["nt"], x["a"], x["b"], x["ns"], x["r2"], x["index"], x["d2"], x["xs"], x["xk"], x["kind"], x["flag"],
                 x["stream"])
    assert call() == abi.OK and call(flag=p) == abi.OK              # num_segments = 0: nothing to do
    radius = C.c_float(1.0)
    assert call(r2=C.cast(C.byref(radius), C.c_void_p)) == abi.OK
    # any non-empty subset of the five outputs — any one will do —, never none
    for mask in range(1, 32):
        sub = {name: (p if mask >> j & 1 else None) for j, name in enumerate(outputs)}
        assert call(**sub) == abi.OK, sub
    for ns in (0, 5):
        assert call(index=None, ns=ns) == abi.ERR_INVALID_ARG          # no output at all
    for bad in (dict(bvh=None), dict(nt=-1), dict(ns=-1), dict(tris=None), dict(ns=5, a=None), dict(ns=5, b=None),
                dict(bvh=_fake_bvh(leaves=None)), dict(bvh=_fake_bvh(nodes=None)), dict(bvh=_fake_bvh(built_level=0)),
                dict(bvh=_fake_bvh(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
    assert call(tris=None, nt=0) == abi.OK and call(a=None, b=None) == abi.OK
    assert call(bvh=_fake_bvh(n=1, nodes=None)) == abi.OK          # a one-leaf tree has no nodes
    broken = _fake_bvh()
    broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # the accepted types, those of closest_points: BBox leaves under BBox nodes of the same or a wider float type, any index type
    for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64)):
        assert call(bvh=_fake_bvh(**good)) == abi.OK, good
    for bad in (dict(leaf_kind=abi.BSPHERE), dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE), dict(node_kind=abi.BSPHERE),
                dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
        # (with segments to process too: refused, never launched on the fake pointers)
        assert call(bvh=_fake_bvh(**bad)) == abi.ERR_UNSUPPORTED and call(bvh=_fake_bvh(**bad), ns=5) == abi.ERR_UNSUPPORTED, bad
    # the order of the other point-walk entries: the entry's own checks first, the types next, the tree and the pointers last
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE), index=None) == abi.ERR_INVALID_ARG
    assert call(bvh=_fake_bvh(leaf_kind=abi.BSPHERE, leaves=None), tris=None) == abi.ERR_UNSUPPORTED


# ---- the checker: hand-made pairs with known answers ---------------------------------------------------------------------
FLAT = tcc.FLAT                                            # (0,0,0) (1,0,0) (0,1,0)
TURNED = FLAT[6:9] + FLAT[0:6]                             # the same triangle as p3 p1 p2: its edge p2p3 is FLAT's p1p2
FAR = tcc.FAR
HAND = {   # name: (a, b, K, d2, xs, xk, kind)
    "through a face": ((0.25, 0.25, -1), (0.25, 0.25, 1), FLAT, 0.0, (0.25, 0.25, 0), (0.25, 0.25, 0), 5),
    "parallel above a face at height 0.5": ((0.25, 0.25, 0.5), (0.5, 0.25, 0.5), FLAT, 0.25, (0.25, 0.25, 0.5), (0.25, 0.25, 0), 0),
    "end-on above a vertex": ((0, 0, 3), (0, 0, 1), FLAT, 1.0, (0, 0, 1), (0, 0, 0), 1),
    "crossing edge p1p2 at a skew": ((0.25, -1, -1), (0.75, -1, 1), FLAT, 1.0, (0.5, -1, 0), (0.5, 0, 0), 2),
    "crossing edge p2p3 at a skew": ((0.25, -1, -1), (0.75, -1, 1), TURNED, 1.0, (0.5, -1, 0), (0.5, 0, 0), 3),
    "crossing edge p3p1 at a skew": ((-1, 0.25, -1), (-1, 0.75, 1), FLAT, 1.0, (-1, 0.5, 0), (0, 0.5, 0), 4),
    "zero length": ((0.25, 0.25, 0.5), (0.25, 0.25, 0.5), FLAT, 0.25, (0.25, 0.25, 0.5), (0.25, 0.25, 0), 0),
    "zero length on the face": ((0.25, 0.25, 0), (0.25, 0.25, 0), FLAT, 0.0, (0.25, 0.25, 0), (0.25, 0.25, 0), 0),
    "boxes apart": ((0, 0, 0), (1, 1, 1), FAR, 48.0, (1, 1, 1), (5, 5, 5), 1),
}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_hand_made_pairs_have_their_known_answers(dt):
    for what, (a, b, k, d2, xs, xk, kind) in HAND.items():
        g2, gs, gk, gkind = (x[0] for x in cc.pairs(np.array([a], dt), np.array([b], dt), np.array([k], dt)))
        assert g2 == d2 and gkind == kind, (what, g2, gkind)
        assert (gs == np.array(xs, dt)).all() and (gk == np.array(xk, dt)).all(), (what, gs, gk)
    assert {v[-1] for v in HAND.values()} == set(range(6))       # each of the six kinds


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_per_capsule_rules_radius_nan_and_the_rim(dt):
    mesh = np.array([FLAT, FAR], dt)
    half = dt(0.5)
    below = np.nextafter(half, dt(0))
    rows = [("parallel above a face at height 0.5", r) for r in (half, below, dt(-1), dt(np.nan), dt(0), dt(np.inf))]
    rows += [("through a face", dt(0)), ("zero length", half), ("zero length", below), ("zero length on the face", dt(0))]
    a = np.array([HAND[w][0] for w, _ in rows], dt)
    b = np.array([HAND[w][1] for w, _ in rows], dt)
    r = np.array([x for _, x in rows], dt)
    bf = cc.brute_force_contacts(mesh, a, b, r)
    # d2 == r * r is a contact, one unit below is none; negative and NaN touch nothing; 0 keeps what the segment lies on or cuts;
    # +Inf admits every triangle; a point capsule is a sphere
    assert bf.counts.tolist() == [1, 0, 0, 0, 0, 2, 1, 1, 0, 1] and bf.slab_dropped == 0
    assert bf.index.tolist() == [1, 1, 2, 1, 1, 1] and bf.d2.tolist() == [0.25, 0.25, 63.0625, 0, 0.25, 0]
    assert bf.kind.tolist() == [0, 0, 1, 5, 0, 0] and bf.capsule.tolist() == [0, 5, 5, 6, 7, 9]
    # the leaf order orders a capsule's rows; an entry that names no triangle is skipped
    back = cc.brute_force_contacts(mesh, a, b, r, leaf_order=[2, 7, 1, 0])
    assert back.counts.tolist() == bf.counts.tolist() and back.index.tolist() == [1, 2, 1, 1, 1, 1]
    again = cc.in_leaf_order(bf, [2, 1])
    assert all(kit.bits(getattr(again, f)) == kit.bits(getattr(back, f)) for f in ("capsule", "index", "d2", "point_segment", "point_mesh", "kind"))
    # a NaN in a or in b touches nothing, and has no closest triangle
    for end in (a, b):
        broken = end.copy()
        broken[5, 1] = np.nan
        pair = (broken, b) if end is a else (a, broken)
        assert cc.brute_force_contacts(mesh, *pair, r).counts.tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 1]
        assert cc.brute_force_distances(mesh, *pair).index.tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    # the stored box decides the slab clause: a leaf box moved away from its triangle drops the contact the distance admits
    moved = tcc.tight_boxes(mesh) + dt(9)
    lost = cc.brute_force_contacts(mesh, a, b, r, leaf_boxes=moved)
    assert lost.counts.tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0, 0] and lost.slab_dropped == 4
    # the distances: the smaller index among equal d2; a radius is inclusive; limited() is the brute force under a radius
    twice = np.array([FAR, FLAT, FLAT], dt)
    dist = cc.brute_force_distances(twice, a, b)
    assert dist.index.tolist() == [2] * 10 and dist.ties.tolist() == [2] * 10 and dist.d2[:2].tolist() == [0.25, 0.25]
    for r2 in (0.25, 0.2, 0.0, np.inf, -1.0, np.nan):
        lim, cut = cc.brute_force_distances(twice, a, b, max_d2=r2), cc.limited(dist, r2)
        for field in cc.FIELDS:
            assert kit.bits(getattr(lim, field)) == kit.bits(getattr(cut, field)), (r2, field)
    assert cc.brute_force_distances(twice, a, b, max_d2=0.2).index.tolist() == [0, 0, 0, 0, 0, 0, 2, 0, 0, 2]
    # a mesh triangle with a NaN vertex has a NaN d2: never a contact, never the closest
    twice[1, 8] = np.nan
    assert cc.brute_force_distances(twice, a, b).index.tolist() == [3] * 10


# ---- the checker against its own Float64 evaluation ----------------------------------------------------------------------
def random_pairs(dt, n=4000, seed=67):
    """n pairs of a random segment and a random triangle in the unit cube, the triangle shifted by up to 0.9 along a random
    direction: apart, close and crossing"""
    rng = np.random.default_rng(seed)
    a, b = rng.random((n, 3)), rng.random((n, 3))
    k = rng.random((n, 9)) + np.repeat(rng.normal(size=(n, 3)) * rng.random((n, 1)) * 0.9, 3, axis=0).reshape(n, 9)
    return a.astype(dt), b.astype(dt), k.astype(dt)


# Measured on these very inputs, relative to the pair's extent (the diagonal of the box around segment and triangle): the largest
# deviation of the Float32 distance from the Float64 distance of the same inputs, and how far the Float32 points lie — in
# Float64 — from their segment / triangle.  The assertions allow four times that: the margin covers other seeds.
DISTANCE_DEVIATION = 8.79e-8
POINT_DEVIATION = 8.79e-8


def test_float32_agrees_with_the_same_evaluation_in_float64():
    a, b, k = random_pairs(np.float32)
    d2, xs, xk, kind = cc.pairs(a, b, k)
    assert not np.isnan(d2).any() and ((d2 == 0) == (kind == cc.CUT)).all() and (kind == cc.CUT).sum() >= 100
    assert np.bincount(kind, minlength=6).min() >= 100              # every kind decides
    a64, b64, k64 = (x.astype(np.float64) for x in (a, b, k))
    e2 = cc.pairs(a64, b64, k64)[0]
    corners = np.concatenate([a64[:, None], b64[:, None], k64.reshape(-1, 3, 3)], axis=1)
    extent = np.linalg.norm(corners.max(axis=1) - corners.min(axis=1), axis=1)
    distance = np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(e2)) / extent
    # the points: xs against the segment (a point-like "segment" against S), xk against K, both in Float64
    xs64, xk64 = xs.astype(np.float64), xk.astype(np.float64)
    off_s = np.sqrt(tdc.closest_on_segments(xs64, xs64, a64, b64)[2]) / extent
    off_k = np.sqrt(cc.cpc._evaluate(k64, xk64)[1]) / extent
    points = np.maximum(off_s, off_k)
    print(f"distance {distance.max():.3e} points {points.max():.3e}")
    assert distance.max() <= 4 * DISTANCE_DEVIATION and points.max() <= 4 * POINT_DEVIATION, (distance.max(), points.max())
    # d2 is the squared length of xs - xk, in the checker's own arithmetic
    e = xs - xk
    assert ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] == d2).all()


# ---- what makes pruning lossless -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_gap_of_a_box_never_exceeds_a_distance_under_it_and_the_slab_clause_is_monotone(dt):
    rng = np.random.default_rng(71)
    tris, a, b, r, bf, _ = cc.reference("torus40", dt)
    pick = slice(0, None, 4)                                         # 100 capsules x 3,200 triangles
    A, B, R = a[pick, None], b[pick, None], r[pick, None]
    d2, _, _, kind = cc.pairs(A, B, tris[None])
    slo, sup = cc.segment_box(A, B)
    klo, kup = cc.triangle_box(tris)
    skin = (klo - dt(1e-3), kup + dt(1e-3))
    boxes = [(klo, kup), skin] + kit.chain(rng, klo, kup, dt)
    entries = []
    for lo, up in boxes:
        assert (lo <= klo).all() and (up >= kup).all()
        lb = tdc.box_bound(lo[None], up[None], slo, sup)
        assert (lb <= d2).all(), int((lb > d2).sum())                  # exact: no tolerance
        assert (lb[kind == cc.CUT] == 0).all()                         # a cut pair's boxes are not apart
        entries.append(cc.grown_entry(lo[None], up[None], R, A, B))
    own = tdc.box_bound(klo[None], kup[None], slo, sup)
    assert (own > 0).mean() > 0.9 and (own == d2).sum() >= 1           # the bound bites, and is attained
    # the slab clause up the chain: a box contains the one before it, so its grown entry is no larger, and a leaf that passes
    # has ancestors that pass
    tight, chained = entries[0], entries[2:]
    for lower, upper in zip([tight] + chained[:-1], chained):
        assert (upper <= lower).all()
    assert (entries[1] <= tight).all()                                 # a skin likewise
    # on the tight boxes the slab clause drops no pair the distance admits, and refuses leaves the gap alone would visit
    with np.errstate(invalid="ignore"):
        near = d2 <= (R * R)
        by_gap, by_slab = cc.refused(klo[None], kup[None], R, A, B)
    assert not (near & (by_gap | by_slab)).any() and bf.slab_dropped == 0
    print(f"the slab clause refuses {(by_slab & ~by_gap).sum() / (~by_gap).sum():.1%} of the leaf pairs the gap admits")
    assert (by_slab & ~by_gap).any() and (by_gap & ~by_slab).any()     # neither bound makes the other idle


# ---- the GPU tests' conditions, on the brute force alone -------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_shared_case_meets_the_gpu_tests_conditions(dt):
    tris, a, b, r, bf, dist = cc.reference("torus40", dt)
    assert tris.shape == (3200, 9) and a.shape == b.shape == (400, 3) and r.shape == (400,)
    from sphere_contacts_checker import mean_edge
    e = mean_edge(tris)
    d = (b - a).astype(np.float64)
    length = np.linalg.norm(d, axis=1)
    assert (length[cc.ZERO_LENGTH] == 0).all() and (length[20:] > 0).all() and length.max() <= 12.001 * e
    assert ((d[cc.ONE_AXIS_STILL] == 0).sum(axis=1) == 1).all() and (r >= 0.49 * e).all() and (r <= 3.01 * e).all()
    total = len(bf.index)
    per_kind = np.bincount(bf.kind, minlength=6)
    print(f"{total} contacts, {total / len(a):.1f} per capsule, kinds {per_kind.tolist()}, {int((bf.counts == 0).sum())} capsules without")
    assert (per_kind[:5] >= 0.05 * total).all(), per_kind                # each of kinds 0 - 4 is at least 5 % of the contacts
    assert per_kind[5] >= 100                                            # at least 100 cuts
    assert total >= 50 * len(a)                                          # at least 50 contacts per capsule on average
    assert (bf.counts == 0).sum() >= 3                                   # at least three capsules with no contact
    assert bf.slab_dropped == 0 and bf.counts.max() >= 64 and (bf.counts[cc.ZERO_LENGTH] > 0).sum() >= 5
    # the distances: every segment has an answer, every kind answers, some answers are tied
    assert (dist.index != 0).all() and len(set(dist.kind.tolist())) == 6 and dist.ties.max() >= 2
    assert (dist.d2 == 0).sum() >= 50 and (dist.d2 > 0).sum() >= 150
