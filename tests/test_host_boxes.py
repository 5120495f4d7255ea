"""ibvh_box_contacts on the host side: the header declares it (additive under ABI version 7) and carries its contract, the
ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, the unit's
one launch goes through the profiling wrapper on the shared walk and the shared count / write protocol, the triangle-box test
lives once in a header of its own, and the entry point validates its arguments before any launch.  The numpy checker the GPU
tests pin the kernel to (tests/box_contacts_checker.py): it gives the known answers on hand-made pairs, each under the identity
and under a rotation, follows the per-box rules, never misses a pair that shares a sampled point, gives an identity matrix the
bits of no matrix, being apart from the hull is monotone up a chain of boxes (what makes pruning lossless), and the GPU tests'
conditions hold for the brute force alone.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib

import box_contacts_checker as bc
import mesh_query_kit as kit
from triangle_distance_checker import boxes_apart

NAME = "ibvh_box_contacts"
UNIT, SAT = "ibvh_boxes.hip", "ibvh_tribox.hpp"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *centers",
                    "const void *half_extents", "const void *rotations", "int64_t num_boxes", "int32_t mode", "void *counts",
                    "const void *offsets", "int64_t capacity", "void *contact_index", "void *contact_inside", "void *flag", "void *stream"]
    flat = " ".join(note.replace("*", " ").split())
    assert "ibvh_box_contacts and IBVH_BOXES_COUNT / IBVH_BOXES_WRITE (additive under 7" in flat
    assert "ibvh_capsule_contacts and IBVH_CAPSULES_COUNT / IBVH_CAPSULES_WRITE, ibvh_segment_distances (additive under 7" in flat
    assert re.search(r"enum \{ IBVH_BOXES_COUNT = 0, IBVH_BOXES_WRITE = 1 \};", hdr)
    join = lambda text: re.sub(r"\n \*\s+", " ", text)        # (the comment's lines joined: a phrase may run over a line end)
    doc = join(raw[raw.index("box-vs-mesh contacts: every triangle an oriented box overlaps"):raw.index("ibvh_status " + NAME)])
    for phrase in ("The HULL Q", "e_k = ((|R_0k| * h_0 + |R_1k| * h_1) + |R_2k| * h_2)", "v[k] = ((u_k0 * w_0 + u_k1 * w_1) + u_k2 * w_2)",
                   "w = x - c", "row k", "ASSUMED orthonormal", "NULL = the identity", "SAME arithmetic", "no second code path",
                   "the BOX clause", "not apart", "six strict comparisons", "the SAT clause", "13 axes", "Akenine-Möller 2001",
                   "min <= rad and max >= -rad", "`P_2 < m ? P_2 : m`", "Touching counts as overlapping",
                   "e_0 = v_2 - v_1, e_1 = v_3 - v_2, e_2 = v_1 - v_3", "n = e_0 x e_1", "d = ((n_0 * v_1[0] + n_1 * v_1[1]) + n_2 * v_1[2])",
                   "rad = ((|n_0| * h_0 + |n_1| * h_1) + |n_2| * h_2)", "d <= rad and d >= -rad", "a = axis_k x e_j",
                   "two non-zero components", "P_i = e[1] * v_i[2] - e[2] * v_i[1], rad = |e[2]| * h_1 + |e[1]| * h_2",
                   "P_i = e[2] * v_i[0] - e[0] * v_i[2], rad = |e[2]| * h_0 + |e[0]| * h_2",
                   "P_i = e[0] * v_i[1] - e[1] * v_i[0], rad = |e[1]| * h_0 + |e[0]| * h_1", "ZERO-AREA", "CONSERVATIVE", "never loses one",
                   "OUTSIDE the contract", "does NOT check", "(ii) implies (i)", "prune on it without loss", "STORED box",
                   "The INSIDE mask", "|v_i[k]| <= h_k", "wholly inside", "without holding a vertex", "INVALID boxes", "not >= 0",
                   "NaN or infinite", "A half extent of zero is valid", "LEAF ORDER", "contact j of the count pass is row j of the write pass",
                   "lossless WITHOUT an epsilon", "contains the boxes below it exactly", "constant limit of 0",
                   "IBVH_BOXES_COUNT or IBVH_BOXES_WRITE", "bit 2", "value 4", "bit 1", "value 2", "IBVH_ERR_UNSUPPORTED",
                   "IBVH_ERR_INVALID_ARG", "num_boxes == 0", "No reference counterpart", "ONE launch each", "every comparison false on NaN",
                   "skin margin", "ibvh_refit", "exactly those of ibvh_capsule_contacts"):
        assert phrase in doc, phrase


def test_binding_tables_makefile_launch_and_python_surface():
    vp = C.c_void_p
    assert lib.SIGNATURES[NAME] == abi.BOX_CONTACTS_ARGTYPES == (
        [C.POINTER(abi.Bvh), vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, C.c_int64] + [vp] * 4)
    assert (abi.BOXES_COUNT, abi.BOXES_WRITE) == (0, 1)
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("box_contacts", "BoxContacts", "voxelize"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    assert issubclass(ibvh.BoxContacts, ibvh.api._ContactLists) and ibvh.BoxContacts.ENTRY == (NAME, 0, 1)
    counted = ibvh.BoxContacts(np.array([0, 2, 5]))                  # what count_only returns: no per-contact column at all
    assert counted.counts.tolist() == [2, 3] and counted.index is None and counted.inside is None and counted.box is None
    # the shared walk once, the shared count / write protocol, the pass as a template parameter
    src = kit.query_unit(UNIT, "boxes::boxes_walk_kernel", lists=True)
    assert len(re.findall(r"__global__", src)) == 1 and "template <class T, class TN, class I, bool WRITE>\n__global__" in src
    assert "fma" not in src and "1e-" not in src and "[]() { return T(0); }" in src and "mode == IBVH_BOXES_WRITE" in src
    geom = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_trigeom.hpp")
    assert geom.count("return (qup[0] < lo[0]) | (qlo[0] > up[0]) | (qup[1] < lo[1]) | (qlo[1] > up[1]) | (qup[2] < lo[2]) | (qlo[2] > up[2]);") == 1
    assert "qup[0] < lo[0]" not in src and re.search(r'^#include "ibvh_trigeom.hpp"$', src, flags=re.M)
    for line in ("return trigeom::apart(qlo, qup, lo, up) ? T(1) : T(0);",
                 "tribox::hull(q, qlo, qup);", "tribox::to_local(q, K + 3 * i, v + 3 * i);", "if (tribox::overlaps(q.h, v)) {",
                 "tribox::inside_mask(q.h, v)", "finite = finite + (q.c[k] - q.c[k]);", "finite = finite + (q.u[k] - q.u[k]);",
                 "if (rotations) q.u[k] = rotations[9 * item + k];", "!pointwalk::hopeless(q.c, finite)",
                 "(q.h[0] >= T(0)) & (q.h[1] >= T(0)) & (q.h[2] >= T(0))"):
        assert line in src, line
    # the local vertices are computed in the visit, after the gather: only for a leaf that passed (i)
    assert src.index("pointwalk::leaf_triangle(") < src.index("tribox::to_local(") < src.index("tribox::overlaps(")
    header = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    assert len(re.findall(r"static_assert\(IBVH_BOXES_COUNT == 0 && IBVH_BOXES_WRITE == 1,", header)) == 1
    assert len(re.findall(r"static_assert\(IBVH_CAPSULES_COUNT == 0 && IBVH_CAPSULES_WRITE == 1,", header)) == 1
    assert UNIT in header[:header.index("#pragma once")]


def test_the_triangle_box_test_exists_once_and_the_unit_includes_it():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    text = {f: kit.read("implicitbvh.jl_amd", "csrc", f) for f in sources}
    assert [f for f in sources if "namespace tribox" in text[f]] == [SAT]
    sat, unit = text[SAT], text[UNIT]
    assert re.search(r'^#include "' + SAT + '"$', unit, flags=re.M)
    for define in (r"IBVH_D void hull\(", r"IBVH_D void to_local\(", r"IBVH_D bool axis_overlaps\(", r"IBVH_D bool overlaps\(",
                   r"IBVH_D unsigned inside_mask\("):
        assert len(re.findall(define, sat)) == 1, define
    for body in (sat, unit):
        assert "fma" not in body and "1e-" not in body and "__shared__" not in body and "/ " not in re.sub(r"//.*", "", body)
    # the operation order of the contract, statement for statement
    for line in ("const T e = (mag(b.u[k]) * b.h[0] + mag(b.u[3 + k]) * b.h[1]) + mag(b.u[6 + k]) * b.h[2];", "lo[k] = b.c[k] - e;",
                 "up[k] = b.c[k] + e;", "const T w[3] = {p[0] - b.c[0], p[1] - b.c[1], p[2] - b.c[2]};",
                 "v[k] = (b.u[3 * k] * w[0] + b.u[3 * k + 1] * w[1]) + b.u[3 * k + 2] * w[2];", "mn = p2 < mn ? p2 : mn;",
                 "mx = p3 > mx ? p3 : mx;", "return (mn <= rad) & (mx >= -rad);",
                 "const T n[3] = {e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]};",
                 "const T d = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2];",
                 "const T rad = (mag(n[0]) * h[0] + mag(n[1]) * h[1]) + mag(n[2]) * h[2];", "if (!((d <= rad) & (d >= -rad))) return false;",
                 "ey * v[2] - ez * v[1], ey * v[5] - ez * v[4], ey * v[8] - ez * v[7], mag(ez) * h[1] + mag(ey) * h[2]",
                 "ez * v[0] - ex * v[2], ez * v[3] - ex * v[5], ez * v[6] - ex * v[8], mag(ez) * h[0] + mag(ex) * h[2]",
                 "ex * v[1] - ey * v[0], ex * v[4] - ey * v[3], ex * v[7] - ey * v[6], mag(ey) * h[0] + mag(ex) * h[1]",
                 "if ((x <= h[0]) & (y <= h[1]) & (z <= h[2])) mask |= 1u << i;"):
        assert line in sat, line
    assert sat.count("axis_overlaps(") == 1 + 1 + 3 and "Akenine-Möller" in sat and "conservative" in sat
    import __graft_entry__ as entry
    assert {os.path.join(csrc, f) for f in (SAT, UNIT)} <= set(entry.kernel_sources(kit.ROOT))


def test_julia_wrapper_binds_it_with_the_ctypes_signature_and_the_docs_name_it():
    src = kit.julia_ccall(NAME, "box_contacts")
    body = src[src.index("function box_contacts("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_BOXES_COUNT" in body and "IBVH_BOXES_WRITE" in body and "cumsum" in body and "point_morton_order(centers)" in body
    design = kit.read("DESIGN.md")
    section = design[design.index("Box-vs-mesh contacts"):][:9000]
    for phrase in ("no reference counterpart", "lossless", "leaf order", "VGPRs", "scratch", "Float32", "Float64"):
        assert phrase in section, phrase
    assert len(re.findall(r"^\| `<(?:float|double), (?:float|double), (?:int|long), (?:count|write)>` \|", section, flags=re.M)) == 12
    assert kit.read("tools", "bench_boxes.py") and "bench_boxes.py" in kit.read("tools", "README.md")
    assert "box_contacts" in kit.read("README.md") and "voxelize" in kit.read("README.md")


def test_entry_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    count = dict(bvh=_fake_bvh(), tris=p, nt=5, c=p, h=p, r=p, nb=0, mode=abi.BOXES_COUNT, counts=p, offsets=None, cap=0, ci=None,
                 cm=None, flag=None, stream=None)
    write = dict(count, mode=abi.BOXES_WRITE, counts=None, offsets=p, cap=7, ci=p)

    def call(base, **kw):
        x = dict(base, **kw)
        bvh = C.byref(x["bvh"]) if x["bvh"] is not None else None
        return f(bvh, x["tris"], x["nt"], x["c"], x["h"], x["r"], x["nb"], x["mode"], x["counts"], x["offsets"], x["cap"], x["ci"], x["cm"],
                 x["flag"], x["stream"])
    kit.check_two_pass_arguments(call, count, write, p, "nb", ("ci", "cm"), needs=("c", "h"), absent=dict(c=None, h=None, r=None), fake=_fake_bvh)
    # the rotations are optional whatever else is there: NULL is never what a call is refused for
    for base in (count, write):
        assert call(base, r=None) == abi.OK
        assert call(base, r=None, bvh=_fake_bvh(leaf_kind=abi.BSPHERE), nb=5) == abi.ERR_UNSUPPORTED


# ---- the checker: hand-made pairs with known answers ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_hand_made_pairs_have_their_known_answers(dt):
    seen = set()
    for what, (tri, variants, near, families, inside) in bc.HAND.items():
        assert any(R is None for _, _, R in variants) and any(R is not None and R != bc.EYE for _, _, R in variants) or "rotation" in what or "hulls" in what, what
        for c, h, R in variants:
            k, C3, H3 = np.array([tri], dt), np.array([c], dt), np.array([h], dt)
            R33 = None if R is None else np.array([R], dt)
            box_ok, normal_ok, edge_ok, mask = (x[0] for x in bc.pairs(k, C3, H3, R33))
            assert (box_ok, normal_ok, edge_ok) == families, (what, R, box_ok, normal_ok, edge_ok)
            bf = bc.brute_force_contacts(k, C3, H3, R33)
            assert bf.counts.tolist() == [int(near and all(families))], (what, R)
            # whether clause (i) passed, and which family refused first, as the brute force records them
            refused = [int(near and not families[0]), int(near and families[0] and not families[1]), int(near and all(families[:2]) and not families[2])]
            assert bf.refused_first.tolist() == refused, (what, R, bf.refused_first)
            if inside is not None:
                assert mask == inside and bf.inside.tolist() == [inside] and bf.index.tolist() == [1], (what, R, mask)
            seen.add((near,) + families)
    # a contact, each family alone, and the box clause deciding
    assert seen == {(True, True, True, True), (True, True, True, False), (True, True, False, True), (True, False, True, True), (False, False, True, True)}
    assert {case[4] for case in bc.HAND.values()} >= {0, 7}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_per_box_rules_touching_invalid_boxes_and_the_leaf_order(dt):
    mesh = np.array([bc.FLAT, bc.ON_FACE, bc.tcc.FAR], dt)
    one, beyond = dt(1), np.nextafter(dt(1), dt(2))
    # touching is a contact, one unit in the last place beyond is none — under the identity and under a rotation
    for R in (None, np.array([bc.RZ90] * 2, dt)):
        k = np.array([bc.ON_FACE, bc.ON_FACE], dt)
        k[1, 0::3] = beyond
        c, h = np.zeros((2, 3), dt), np.ones((2, 3), dt)
        b, n, e, m = bc.pairs(k, c, h, R)
        assert (b & n & e).tolist() == [True, False] and m.tolist() == [7, 0] and b.tolist() == [True, False]
    # invalid boxes touch nothing, around a triangle they would hold; -0.0 is a valid half extent, but -Inf beside it is not
    for c, h, R in bc.INVALID:
        args = np.array([c], dt), np.array([h], dt), None if R is None else np.array([R], dt)
        assert bc.brute_force_contacts(mesh, *args).counts.tolist() == [0], (c, h, R)
        sound = np.array([[2, 2, 1]], dt), None
        assert bc.brute_force_contacts(mesh, np.array([[0.25, 0.25, 0]], dt), *sound).index.tolist() == [1, 2]
    # an infinite half extent is not refused: the result is what the arithmetic gives
    huge = bc.brute_force_contacts(mesh, np.zeros((1, 3), dt), np.full((1, 3), np.inf, dt), None)
    assert huge.counts.tolist() == [int(len(huge.index))]
    # the leaf order orders a box's rows; an entry that names no triangle is skipped
    c, h = np.array([[0, 0, 0], [5, 5, 5], [9, 9, 9]], dt), np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1]], dt)
    bf = bc.brute_force_contacts(mesh, c, h, None)
    assert bf.counts.tolist() == [2, 1, 0] and bf.index.tolist() == [1, 2, 3] and bf.box.tolist() == [0, 0, 1] and bf.inside.tolist() == [7, 7, 7]
    back = bc.brute_force_contacts(mesh, c, h, None, leaf_order=[3, 7, 2, 0, 1])
    assert back.counts.tolist() == [2, 1, 0] and back.index.tolist() == [2, 1, 3]
    again = bc.in_leaf_order(bf, [3, 2, 1])
    assert all(kit.bits(getattr(again, f)) == kit.bits(getattr(back, f)) for f in ("box", "index", "inside"))
    # the stored box decides clause (i): a leaf box moved away from its triangle drops the contact the 13 axes admit
    # (and a stored box that reaches the hull admits nothing by itself: the 13 axes still read the triangle)
    moved = bc.tcc.tight_boxes(mesh) + dt(9)
    lost = bc.brute_force_contacts(mesh, c, h, None, leaf_boxes=moved)
    assert lost.counts.tolist() == [0, 0, 0] and lost.refused_first.sum() == 2 and bf.refused_first.sum() == 0
    # a NaN vertex fails a comparison: no contact, whichever vertex carries it
    for j in range(9):
        broken = mesh.copy()
        broken[0, j] = np.nan
        assert bc.brute_force_contacts(broken, c[:1], np.full((1, 3), 4, dt), None).index.tolist() == [2], j


# ---- properties ------------------------------------------------------------------------------------------------------------
def _turned_cube(rng, n, dt=np.float64):
    """n cubes turned by 45 degrees about z, and as many random triangles around them"""
    c = (rng.random((n, 3)) - 0.5).astype(dt)
    h = np.full((n, 3), 0.5, dt)
    R = np.broadcast_to(np.array(bc.RZ45, dt), (n, 3, 3)).copy()
    k = ((rng.random((n, 9)) - 0.5) * 3).astype(dt)
    return k, c, h, R


def test_a_contact_is_never_missed_interior_point_sampling_against_a_turned_cube():
    """Float64; a pair is certainly in contact if some sampled point of the triangle lies strictly inside the cube: the 13 axes
    must then all overlap.  The converse bounds what they admit: a pair they admit lies within the cube grown a little."""
    rng = np.random.default_rng(73)
    k, c, h, R = _turned_cube(rng, 4000)
    box_ok, normal_ok, edge_ok, inside = bc.pairs(k, c, h, R)
    sat = box_ok & normal_ok & edge_ok
    bary = rng.dirichlet(np.ones(3), size=(len(k), 256))                                    # (n, 256, 3)
    points = np.einsum("nsi,nij->nsj", bary, k.reshape(-1, 3, 3))
    loc = np.einsum("nkj,nsj->nsk", R, points - c[:, None])
    certainly = (np.abs(loc) < h[:, None] - 1e-9).all(axis=2).any(axis=1)
    assert certainly.sum() >= 500 and (~sat).sum() >= 500
    assert sat[certainly].all(), int((certainly & ~sat).sum())
    assert ((inside != 0) <= sat).all()                                                      # a vertex inside is a contact
    # every family refuses some pair the others pass, so none is idle
    assert (~box_ok & normal_ok & edge_ok).any() and (box_ok & ~normal_ok & edge_ok).any() and (box_ok & normal_ok & ~edge_ok).any()
    # the hull of the turned cube is sqrt(2) wide in x and y, and a contact's triangle box is never apart from it: (ii) implies (i)
    qlo, qup = bc.hull(c, h, R)
    assert np.allclose(qup - qlo, [2 ** 0.5, 2 ** 0.5, 1])
    klo, kup = bc.tcc.fold_box(k)
    assert not boxes_apart(qlo, qup, klo, kup)[sat].any()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_an_identity_matrix_gives_the_bits_of_no_matrix(dt):
    tris, c, h, R, bf = bc.reference("torus40", dt)
    quarter = len(c) // 4
    assert (R[:quarter] == np.eye(3, dtype=dt)).all() and not (R[quarter:] == np.eye(3, dtype=dt)).all(axis=(1, 2)).any()
    none = bc.brute_force_contacts(tris, c[:quarter], h[:quarter], None)
    part = bc.first(bf, quarter)
    assert len(none.index) > 1000 and all(kit.bits(getattr(none, f)) == kit.bits(getattr(part, f)) for f in ("counts", "box", "index", "inside"))
    # ... and under the identity the hull is the box itself and the local coordinates are p - c
    qlo, qup = bc.hull(c[:quarter], h[:quarter], R[:quarter])
    assert kit.bits(qlo) == kit.bits(c[:quarter] - h[:quarter]) and kit.bits(qup) == kit.bits(c[:quarter] + h[:quarter])
    v = bc.local(c[:quarter, None], R[:quarter, None], tris[None, :50, 0:3])
    assert kit.bits(np.stack(v, axis=-1)) == kit.bits(tris[None, :50, 0:3] - c[:quarter, None])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_being_apart_from_the_hull_is_monotone_up_a_chain_of_boxes(dt):
    """what the pruning rests on: a box that is apart from Q lies over boxes that are apart from Q — so a leaf that passes (i)
    has ancestors that pass, and a refused node hides no contact"""
    rng = np.random.default_rng(71)
    tris, c, h, R, bf = bc.reference("torus40", dt)
    pick = slice(0, None, 3)                                         # 100 boxes x 3,200 triangles
    qlo, qup = bc.hull(c[pick], h[pick], R[pick])
    klo, kup = bc.tcc.fold_box(tris)
    skin = (klo - dt(1e-3), kup + dt(1e-3))
    levels = [(klo, kup), skin] + kit.chain(rng, klo, kup, dt)
    apart = [boxes_apart(qlo[:, None], qup[:, None], lo[None], up[None]) for lo, up in levels]
    for lo, up in levels:
        assert (lo <= klo).all() and (up >= kup).all()
    tight, chained = apart[0], apart[2:]
    for lower, upper in zip([tight] + chained[:-1], chained):
        assert (upper <= lower).all()                                # apart above implies apart below
    assert (apart[1] <= tight).all()                                 # a skin likewise
    assert chained[-1].any() and (tight & ~chained[-1]).any()        # the chain still prunes, and less than the leaves do
    # no contact of the brute force lies under a box that is apart
    rows = np.flatnonzero(np.isin(bf.box, np.arange(len(c))[pick]))
    at = (bf.box[rows] // 3, bf.index[rows] - 1)
    assert len(rows) > 5000 and not any(a[at].any() for a in apart)
    # a NaN in the hull refuses nothing
    assert not boxes_apart(np.full(3, np.nan, dt), np.full(3, np.nan, dt), klo, kup).any()


# ---- the GPU tests' conditions, on the brute force alone -------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_shared_case_meets_the_gpu_tests_conditions(dt):
    tris, c, h, R, bf = bc.reference("torus40", dt)
    assert tris.shape == (3200, 9) and c.shape == h.shape == (300, 3) and R.shape == (300, 3, 3)
    from sphere_contacts_checker import mean_edge
    e = mean_edge(tris)
    assert (h >= 0.249 * e).all() and (h <= 3.001 * e).all()
    R64 = R.astype(np.float64)
    assert np.abs(R64 @ R64.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R64), 1, atol=1e-6)
    total = len(bf.index)
    classes = [int((bf.inside == 0).sum()), int(((bf.inside > 0) & (bf.inside < 7)).sum()), int((bf.inside == 7).sum())]
    print(f"{total} contacts, {total / len(c):.1f} per box, inside 0 / partial / 7 {classes}, refused first {bf.refused_first.tolist()}, "
          f"{int((bf.counts == 0).sum())} boxes without")
    assert min(classes) >= 50, classes                                   # at least 50 contacts in each inside class
    assert bf.refused_first.min() >= 50, bf.refused_first                # at least 50 pairs refused first by each family
    assert (bf.counts == 0).sum() >= 3                                   # at least three boxes without a contact
    assert total >= 50 * len(c)                                          # at least 50 contacts a box on average
    assert set(np.unique(bf.inside).tolist()) == set(range(8))           # every mask occurs
    # the smaller case of the GPU tests: every class and family still occurs
    _, c2, _, _, bf2 = bc.reference("torus64x63", dt, 100)
    assert len(bf2.index) >= 50 * len(c2) and bf2.refused_first.min() >= 20 and (bf2.counts == 0).sum() >= 3
