"""ibvh_sphere_contacts on the host side: the header declares it (additive under ABI version 7) and carries its contract, the
ctypes table and the Julia extension bind it with the same argument kinds, the Makefile builds its translation unit, its one
launch goes through the profiling wrapper, the point-triangle routine it shares with the closest-point query exists once, and
the entry point validates its arguments — the refused type combinations included — before any launch.  The numpy checker the
GPU test pins the kernel to (tests/sphere_contacts_checker.py) does what its definition says on hand-made inputs, and the GPU
test's non-vacuity conditions hold for the brute force alone.  No GPU."""
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
import sphere_contacts_checker as scc
from mesh_query_kit import MESHES

NAME = "ibvh_sphere_contacts"
UNIT = "ibvh_spheres.hip"
SHARED = "ibvh_pointtri.hpp"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BBOX)


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *triangles", "int64_t num_triangles", "const void *centers", "const void *radii",
                    "int64_t num_spheres", "int32_t mode", "void *counts", "const void *offsets", "int64_t capacity",
                    "void *contact_index", "void *contact_d2", "void *contact_point", "void *contact_region", "void *flag",
                    "void *stream"]
    assert NAME in note and "IBVH_SPHERES_COUNT / IBVH_SPHERES_WRITE" in note and note.count("additive") >= 2
    assert re.search(r"enum \{ IBVH_SPHERES_COUNT = 0, IBVH_SPHERES_WRITE = 1 \};", hdr)
    assert (abi.SPHERES_COUNT, abi.SPHERES_WRITE) == (0, 1)
    # the doc comment carries the contract: the region codes, the radius, NaN, the order, the two passes, capacity, the guards
    doc = raw[raw.index("sphere-vs-mesh contacts: every triangle within each sphere's radius"):raw.index("ibvh_status " + NAME)]
    for phrase in ("0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 face", "r2 = r * r, rounded once",
                   "d2(k, c) <= r2", "false on NaN", "!(r >= 0)", "r = +Inf", "LEAF ORDER", "ascending position", "bvh->leaves",
                   "row offsets[s] + j", "need NOT be monotone", "A row >= capacity or < 0 is never written", "bit 2 of `flag` (value 4)",
                   "bit 1 of `flag` (value 2)", "BOTH passes alike", "ANY exclusive prefix sum", "The scan is the caller's",
                   "counts[s] = the number of contacts", "x int64", "uint8", "at least one non-NULL", "IBVH_ERR_INVALID_ARG",
                   "IBVH_ERR_UNSUPPORTED", "num_spheres == 0", "skin margin", "ibvh_refit", "No reference counterpart", "lb(B) > r2",
                   "the same clamp of q into the triangle's box", "nothing fused"):
        assert phrase in doc, phrase


def test_binding_table_makefile_launch_and_python_surface():
    want = ([C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
            + [C.c_void_p] * 6)
    assert lib.SIGNATURES[NAME] == want
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    for name in ("sphere_contacts", "SphereContacts"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    src = kit.query_unit(UNIT, "spheres::spheres_walk_kernel", lists=True)
    # one kernel template for both passes, the pass a template parameter reached through the two bool types — which the shared
    # header spells, once, with the rest of the two-pass protocol (kit.PROTOCOL, checked by query_unit)
    assert len(re.findall(r"__global__", src)) == 1 and "template <class T, class TN, class I, bool WRITE>" in src
    # the crossings query's way of keeping leaf order: a 0 / 1 bound under a constant limit of 0
    assert "pointwalk::box_bound(lo, up, p) > r2 ? T(1) : T(0)" in src and "[]() { return T(0); }" in src
    assert "raise_flag(flag, 4u)" in src and "hopeless(p, r2)" in src and "r >= T(0)" in src


def test_the_point_triangle_routine_exists_once_and_both_queries_share_it():
    csrc = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))]
    define = r"\bclosest_on_triangle\s*\([^)]*\)\s*\{"
    assert [f for f in sources if re.search(define, kit.read("implicitbvh.jl_amd", "csrc", f))] == [SHARED]
    shared = kit.read("implicitbvh.jl_amd", "csrc", SHARED)
    assert len(re.findall(define, shared)) == 1 and [int(x) for x in re.findall(r"region = (\d);", shared)] == list(range(7))
    for unit in ("ibvh_closest.hip", UNIT):
        text = kit.read("implicitbvh.jl_amd", "csrc", unit)
        assert re.search(r'^#include "' + SHARED + '"$', text, flags=re.M) and "closest_on_triangle(tr, p, q, region)" in text, unit
    # ... and not in the walk's header, whose contents other tests pin; the bound stays there alone
    walk = kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    assert "closest_on_triangle" not in walk and "box_bound" not in shared
    import __graft_entry__ as entry
    assert {os.path.join(csrc, SHARED), os.path.join(csrc, UNIT)} <= set(entry.kernel_sources(kit.ROOT))


def test_julia_wrapper_binds_it_with_the_ctypes_signature():
    src = kit.julia_ccall(NAME, "sphere_contacts")
    body = src[src.index("function sphere_contacts("):]
    body = body[:body.index("\nend\n")]
    assert "IBVH_SPHERES_COUNT" in body and "IBVH_SPHERES_WRITE" in body and ("cumsum" in body or "accumulate" in body)
    design = kit.read("DESIGN.md")
    section = design[design.index("Sphere-vs-mesh contacts"):][:6000]
    assert "no reference counterpart" in section and "lossless" in section and "leaf order" in section


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    count = dict(bvh=_fake_bvh(), tris=p, nt=5, c=p, r=p, ns=0, mode=abi.SPHERES_COUNT, counts=p, offsets=None, cap=0, ci=None, cd=None,
                 cq=None, cr=None, flag=None, stream=None)
    write = dict(count, mode=abi.SPHERES_WRITE, counts=None, offsets=p, cap=7, ci=p)

    def call(base, **kw):
        a = dict(base, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["tris"], a["nt"], a["c"], a["r"], a["ns"], a["mode"], a["counts"], a["offsets"], a["cap"], a["ci"], a["cd"],
                 a["cq"], a["cr"], a["flag"], a["stream"])
    kit.check_two_pass_arguments(call, count, write, p, "ns", ("ci", "cd", "cq", "cr"), needs=("c", "r"), absent=dict(c=None, r=None),
                                 fake=_fake_bvh)


# ---- the checker --------------------------------------------------------------------------------------------------------
def test_checker_follows_its_definition_on_hand_made_inputs():
    f = np.float32
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f)
    pts = np.array([[-1, -1, 1], [2, -0.5, 1], [0.5, -1, 1], [-0.5, 2, 1], [-1, 0.5, 1], [1, 1, 1], [0.25, 0.25, 1]], f)
    d2 = np.array([3, 2.25, 2, 2.25, 2, 1.5, 1], f)
    bf = scc.brute_force(tri, pts, np.nextafter(np.sqrt(d2), f(np.inf)))
    assert bf.counts.tolist() == [1] * 7 and bf.region.tolist() == list(range(7)) and bf.d2.tolist() == d2.tolist()
    assert bf.region.dtype == np.uint8 and bf.offsets.tolist() == list(range(8)) and bf.index.tolist() == [1] * 7
    assert scc.brute_force(tri, pts, np.sqrt(d2) * f(0.999)).counts.tolist() == [0] * 7
    # several triangles, a leaf order, a duplicate, a NaN vertex, leaves that name no triangle
    tris = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0.5, np.nan, 0, 0.5, 0, 1, 0.5],
                     [0, 0, 2, 1, 0, 2, 0, 1, 2]], f)
    c = np.array([[0.25, 0.25, 1]] * 6 + [[np.nan, 0.25, 1]], f)
    r = np.array([1, 0.5, -1, np.nan, np.inf, 0, 1], f)
    bf = scc.brute_force(tris, c, r, leaf_order=[4, 9, 2, 3, 1, 0], idt=np.int64)
    assert bf.counts.tolist() == [3, 0, 0, 0, 3, 0, 0] and bf.index.tolist() == [4, 2, 1, 4, 2, 1] and bf.index.dtype == np.int64
    assert bf.sphere.tolist() == [0, 0, 0, 4, 4, 4] and bf.offsets.tolist() == [0, 3, 3, 3, 3, 6, 6, 6]
    assert (bf.d2 == 1).all() and (bf.region == 6).all() and bf.point.tolist() == [[0.25, 0.25, 2]] + [[0.25, 0.25, 0]] * 2 + [[0.25, 0.25, 2]] + [[0.25, 0.25, 0]] * 2
    assert scc.brute_force(tris, c, r).index.tolist() == [1, 2, 4, 1, 2, 4]
    assert scc.brute_force(tris[:0], c, r).counts.tolist() == [0] * 7
    on = scc.brute_force(tris, np.array([[0.25, 0.25, 0], [0.25, 0.25, 0.001]], f), np.zeros(2, f))
    assert on.counts.tolist() == [2, 0] and (on.d2 == 0).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_sphere_sets_meet_the_gpu_tests_non_vacuity_conditions(mesh, dt):
    tris = torus_mesh(*MESHES[mesh]).astype(dt)
    c, radii = scc.pipeline_spheres(tris, dt)
    assert c.shape == (800, 3) and radii.shape == (800,) and c.dtype == radii.dtype == dt
    assert (radii[600::2] == 0).all() and (radii[601::2] > 0).all()
    bf = scc.brute_force(tris, c, radii, idt=np.int64)
    nv = scc.non_vacuity(bf, radii)
    print(f"{mesh} {np.dtype(dt).name}: {nv}")
    scc.assert_non_vacuous(nv)
    # every exact-square radius keeps the contact whose d2 it was made from, and the lists agree with the evaluation
    rows = np.arange(0, 600, 16)
    rim = np.zeros(800, bool)
    rim[bf.sphere[bf.d2 == bf.r2[bf.sphere]]] = True
    assert rim[rows].all() and (bf.counts[rows] >= 5).all()
    q, d2, region = cpc.evaluate(tris, c[:64])
    with np.errstate(invalid="ignore"):
        assert ((d2 <= bf.r2[:64, None]).sum(axis=1) == bf.counts[:64]).all()
    # a permuted leaf order permutes each list and nothing else
    perm = np.random.default_rng(5).permutation(len(tris)) + 1
    other = scc.brute_force(tris, c, radii, leaf_order=perm, idt=np.int64)
    assert (other.counts == bf.counts).all() and (other.index != bf.index).any()
    rank = np.empty(len(tris) + 1, np.int64)
    rank[perm] = np.arange(len(tris))
    resort = np.lexsort((other.index, other.sphere))
    assert (other.index[resort] == bf.index).all() and other.d2[resort].tobytes() == bf.d2.tobytes()
    assert (np.diff(rank[other.index])[np.diff(other.sphere) == 0] > 0).all()
