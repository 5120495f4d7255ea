"""ibvh_rays_resolve_triangles on the GPU: index, t, uv and candidate_t are BIT-EQUAL to the numpy checker
(tests/ray_triangle_checker.py) run on the library's own candidate list — every float / index type, both leaf kinds, small
meshes, a mesh on the binned ray path, with and without the ray narrow, random and aimed rays — plus the guards, the tie
rule, the degenerate inputs and the errors of the Python mirror.  On the small meshes the result is also held against a
brute force over all triangles: the list can only lose hits (the broad phase is the reference's rounded test), never invent
or move one; the share of rays where it lost the brute-force winner is printed, not bounded (DESIGN.md quotes it)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import random_rays, torus_mesh  # noqa: E402

import ray_triangle_checker as rtc  # noqa: E402
from test_gpu_parity import _rays_positions, cuda, make_options  # noqa: E402
from test_gpu_rays_binned import _kernels_of  # noqa: E402

NP_F = {abi.F32: np.float32, abi.F64: np.float64}
NP_I = {abi.I32: np.int32, abi.I64: np.int64}
TOKEN = {abi.BSPHERE: ibvh.BSphere, abi.BBOX: ibvh.BBox}
# (u, v) of torus_mesh and the rays per set; "binned": 72,200 triangles = 18 levels under 5,000 rays, which the shipped rule
# sends down the binned ray path (tests/test_gpu_rays_binned.py::test_the_shipped_rule_really_takes_the_path_it_names)
MESHES = {"torus40": (40, 40, 2000), "torus64x63": (64, 63, 2000), "binned": (190, 190, 5000)}


def _mesh(name, flt):
    u, v, nr = MESHES[name]
    return torus_mesh(u, v).astype(NP_F[flt]), nr


def _build(tris, kind, flt, idx):
    types = abi.make_types(kind, flt, abi.BBOX, flt, index_type=idx)
    tdev = cuda(tris)
    ft = torch.float32 if flt == abi.F32 else torch.float64
    vols = ibvh.bounding_volumes_from_triangles(tdev, TOKEN[kind](ft))
    return ibvh.BVH(vols, ibvh.BBox(ft), options=make_options(types)), tdev


def _ray_sets(tris, nr, dt):
    lo, hi = rtc.mesh_box(tris)
    p, d = random_rays(nr, lo, hi, seed=5)
    pa, da = rtc.aimed_rays(nr, tris, dt)
    return {"random": (p.astype(dt), d.astype(dt)), "aimed": (pa, da)}


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_equal(got, exp, trav, what):
    """RayHits against the checker, bit for bit"""
    assert (got.index.cpu().numpy() == exp.index).all(), what
    assert got.index.cpu().numpy().dtype == exp.index.dtype, what
    assert _bits(got.t.cpu().numpy()) == _bits(exp.t), what
    assert _bits(got.uv.cpu().numpy()) == _bits(exp.uv), what
    if got.candidate_t is not None:
        assert got.candidate_t.shape[0] == trav.num_contacts == len(exp.candidate_t), what
        assert _bits(got.candidate_t.cpu().numpy()) == _bits(exp.candidate_t), what


def _check_on_own_list(trav, got, tris, p, d, what):
    counts = trav.cache2.cpu().numpy()[: len(p)]
    contacts = trav.contacts.cpu().numpy()
    exp = rtc.resolve(counts, contacts, tris, p, d)
    assert not exp.bad.any()
    _assert_equal(got, exp, trav, what)
    return exp


@pytest.mark.parametrize("narrow", [None, ibvh.NARROW_RAY_ORIGIN_OUTSIDE], ids=["none", "origin_outside"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("kind", [abi.BSPHERE, abi.BBOX], ids=["bsphere", "bbox"])
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_resolve_is_bit_equal_to_the_checker_on_the_librarys_own_list(flt, idx, kind, mesh, narrow):
    tris, nr = _mesh(mesh, flt)
    bvh, tdev = _build(tris, kind, flt, idx)
    for name, (p, d) in _ray_sets(tris, nr, NP_F[flt]).items():
        P, D = cuda(p).t(), cuda(d).t()
        what = (mesh, name)
        got, trav = ibvh.raycast(bvh, tdev, P, D, narrow=narrow, all_hits=True)
        assert trav.contacts.dtype == (torch.int32 if idx == abi.I32 else torch.int64)
        exp = _check_on_own_list(trav, got, tris, p, d, what)
        # the conditions that make the comparison mean something
        share = float((exp.index > 0).mean())
        print(f"{mesh} {name} flt={flt} idx={idx} kind={kind} narrow={narrow}: {trav.num_contacts / nr:.2f} candidates per ray, "
              f"{share:.3f} of the rays hit, {int(exp.accepted.sum())} accepted / {int((~exp.accepted).sum())} rejected candidates")
        assert share >= (0.5 if name == "random" else 0.99), (what, share)
        assert exp.accepted.any() and (~exp.accepted).any(), what
        # closest only (no cand_t) and through the cached, enqueued traversal: the same bits
        got2 = ibvh.resolve_triangles(ibvh.traverse_rays(bvh, P, D, narrow=narrow, cache=trav), tdev, P, D)
        assert got2.candidate_t is None
        _assert_equal(got2, exp, trav, what)


def test_the_big_mesh_takes_the_binned_ray_path_and_the_profiler_sees_the_resolve_kernel():
    tris, nr = _mesh("binned", abi.F32)
    bvh, tdev = _build(tris, abi.BSPHERE, abi.F32, abi.I32)
    p, d = _ray_sets(tris, nr, np.float32)["random"]
    P, D = cuda(p).t(), cuda(d).t()
    names = _kernels_of(lambda: ibvh.raycast(bvh, tdev, P, D))
    assert {"rays_top_kernel", "rays_subtree_kernel", "raytri_resolve_kernel"} <= names, names


@pytest.mark.parametrize("mesh", ["torus40", "torus64x63"])
@pytest.mark.parametrize("kind", [abi.BSPHERE, abi.BBOX], ids=["bsphere", "bbox"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_the_list_only_loses_hits_against_a_brute_force_over_all_triangles(flt, kind, mesh):
    tris, nr = _mesh(mesh, flt)
    bvh, tdev = _build(tris, kind, flt, abi.I32)
    for name, (p, d) in _ray_sets(tris, nr, NP_F[flt]).items():
        got, _ = ibvh.raycast(bvh, tdev, cuda(p).t(), cuda(d).t())
        bf = rtc.brute_force(tris, p, d, idt=np.int32)
        gi, gt, guv = got.index.cpu().numpy(), got.t.cpu().numpy(), got.uv.cpu().numpy()
        assert (gt >= bf.t).all(), (mesh, name)          # (a miss is +Inf; nothing nearer than the true nearest hit)
        assert (bf.index[gi > 0] > 0).all()               # a hit of the list is a hit of the mesh
        same = (gi == bf.index) & (gi > 0)
        assert _bits(gt[same]) == _bits(bf.t[same]) and _bits(guv[same]) == _bits(bf.uv[same])
        lost = (bf.index > 0) & (gi != bf.index)
        print(f"broad-phase loss {mesh} {name} flt={flt} kind={kind}: {int(lost.sum())} of {int((bf.index > 0).sum())} rays with a "
              f"brute-force hit lost the brute-force winner ({lost.sum() / max(1, (bf.index > 0).sum()):.5f})")


# ---- hand-made lists straight through the C entry point ------------------------------------------------------------------
def _call(tris, p, d, counts, contacts, capacity=None, num_triangles=None, flag=0, outs="itub", num_rays=None):
    """-> dict of numpy outputs (prefilled with sentinels so that 'not written' is visible) + the flag word"""
    ft, it = tris.dtype, contacts.dtype
    nr = len(p) if num_rays is None else num_rays
    cap = len(contacts) if capacity is None else capacity
    T, Pp, Dd, Cn, Ct = cuda(tris), cuda(p), cuda(d), cuda(counts), cuda(contacts)
    o = {"i": torch.full((max(nr, 1),), -7, dtype=Cn.dtype, device="cuda"), "t": torch.full((max(nr, 1),), -7.0, dtype=T.dtype, device="cuda"),
         "u": torch.full((max(nr, 1), 2), -7.0, dtype=T.dtype, device="cuda"), "b": torch.full((max(len(contacts), 1),), -7.0, dtype=T.dtype, device="cuda")}
    fl = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    ptr = lambda k: api._ptr(o[k]) if k in outs else None
    st = getattr(lib.load(), "ibvh_rays_resolve_triangles")(
        abi.F32 if ft == np.float32 else abi.F64, abi.I32 if it == np.int32 else abi.I64, api._ptr(T),
        len(tris) if num_triangles is None else num_triangles, api._ptr(Pp), api._ptr(Dd), nr, api._ptr(Cn), api._ptr(Ct), cap,
        ptr("i"), ptr("t"), ptr("u"), ptr("b"), api._ptr(fl), api._stream())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["flag"], out["status"] = int(fl.item()), st
    return out


EDGE_TRIS = [[0, 0, 1, 1, 0, 1, 0, 1, 1],         # 1
             [0, 0, 2, 1, 0, 2, 0, 1, 2],         # 2: behind 1 as seen from z = 0
             [0, 0, 1, 1, 0, 1, 0, 1, 1],         # 3: a duplicate of 1
             [0, 0, 1, 1, 1, 1, 2, 2, 1],         # 4: zero area
             [0, 0, -1, 1, 0, -1, 0, 1, -1]]      # 5: below z = 0
EDGE_P = [[0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 1], [5, 5, 0], [np.nan, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 0]]
EDGE_D = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, np.nan], [0, 0, 1]]


@pytest.mark.parametrize("it", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("ft", [np.float32, np.float64], ids=["f32", "f64"])
def test_duplicates_degenerate_triangles_and_rays_without_candidates(ft, it):
    tris, p, d = np.array(EDGE_TRIS, ft), np.array(EDGE_P, ft), np.array(EDGE_D, ft)
    for order, first in (([1, 2, 3, 4, 5], 1), ([3, 2, 1, 4, 5], 3), ([5, 4, 2, 3, 1], 3)):
        # rays 1 - 6 see every triangle in `order`; ray 7 has no candidates
        n = len(order)
        contacts = np.stack([np.tile(np.asarray(order, it), 6), np.repeat(np.arange(1, 7, dtype=it), n)], axis=1)
        counts = np.array([n, 2 * n, 3 * n, 4 * n, 5 * n, 6 * n, 6 * n], it)
        exp = rtc.resolve(counts, contacts, tris, p, d)
        got = _call(tris, p, d, counts, contacts)
        assert got["status"] == 0 and got["flag"] == 0
        assert (got["i"] == exp.index).all() and _bits(got["t"]) == _bits(exp.t) and _bits(got["u"]) == _bits(exp.uv)
        assert _bits(got["b"]) == _bits(exp.candidate_t)
        # what the checker itself says about these inputs (tests/test_host_ray_triangles.py pins it on the host too)
        assert got["i"].tolist() == [first, 5, 0, 0, 0, 0, 0]       # duplicate: equal t, the earlier entry; parallel, far, NaN, empty: misses
        assert got["t"][:2].tolist() == [1.0, 1.0] and np.isposinf(got["t"][2:]).all() and (got["u"][2:] == 0).all()
        acc = np.isfinite(got["b"]).reshape(6, n)
        assert acc[0].sum() == 3 and not acc[2:].any() and not acc[:, order.index(4)].any()
    # -0 == +0: the same triangle wound both ways under a ray that starts on it; the earlier entry wins, its sign is kept
    tz = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 0, 1, 0, 0]], ft)
    pz, dz = np.array([[0.25, 0.25, 0]], ft), np.array([[0, 0, 1]], ft)
    for order in ([1, 2], [2, 1]):
        contacts = np.array([[order[0], 1], [order[1], 1]], it)
        counts = np.array([2], it)
        exp = rtc.resolve(counts, contacts, tz, pz, dz)
        got = _call(tz, pz, dz, counts, contacts)
        assert got["i"][0] == order[0] == exp.index[0] and _bits(got["t"]) == _bits(exp.t) and _bits(got["b"]) == _bits(exp.candidate_t)
        assert got["t"][0] == 0 and np.signbit(got["b"][0]) != np.signbit(got["b"][1])
    # any subset of the outputs
    contacts = np.stack([np.tile(np.arange(1, 6, dtype=it), 7), np.repeat(np.arange(1, 8, dtype=it), 5)], axis=1)
    counts = (np.arange(1, 8) * 5).astype(it)
    exp = rtc.resolve(counts, contacts, tris, p, d)
    for outs in ("i", "t", "u", "b", "it", "ub"):
        got = _call(tris, p, d, counts, contacts, outs=outs)
        assert got["status"] == 0
        for k, e in (("i", exp.index), ("t", exp.t), ("u", exp.uv), ("b", exp.candidate_t)):
            assert _bits(got[k]) == _bits(e) if k in outs else (got[k] == -7).all(), (outs, k)


def test_guards_capacity_and_index_range():
    ft, it = np.float32, np.int32
    tris, p, d = np.array(EDGE_TRIS, ft), np.array(EDGE_P, ft), np.array(EDGE_D, ft)
    contacts = np.stack([np.tile(np.arange(1, 6, dtype=it), 7), np.repeat(np.arange(1, 8, dtype=it), 5)], axis=1)
    counts = (np.arange(1, 8) * 5).astype(it)
    # capacity below the device total: the list was never written — nothing is written except flag bit 0 (never cleared: 4 stays)
    got = _call(tris, p, d, counts, contacts, capacity=34, flag=4)
    assert got["status"] == 0 and got["flag"] == 5
    for k in "itub":
        assert (got[k] == -7).all(), k
    assert _call(tris, p, d, counts, contacts, capacity=35, flag=0)["flag"] == 0   # exactly enough is enough
    # num_triangles below the largest index: those candidates are misses, bit 1 is raised, the rest stays exact
    got = _call(tris, p, d, counts, contacts, num_triangles=3, flag=4)
    keep = contacts.copy()
    exp = rtc.resolve(counts, keep, tris[:3], p, d)
    assert exp.bad.sum() == 14 and got["status"] == 0 and got["flag"] == 6
    assert (got["i"] == exp.index).all() and _bits(got["t"]) == _bits(exp.t) and _bits(got["u"]) == _bits(exp.uv)
    assert _bits(got["b"]) == _bits(exp.candidate_t) and got["i"].tolist() == [1, 0, 0, 0, 0, 0, 1]
    # ... also indices below 1
    c0 = contacts.copy()
    c0[::5, 0] = 0
    c0[1::5, 0] = -3
    exp = rtc.resolve(counts, c0, tris, p, d)
    got = _call(tris, p, d, counts, c0)
    assert got["flag"] == 2 and (got["i"] == exp.index).all() and _bits(got["b"]) == _bits(exp.candidate_t)
    # num_rays = 0: nothing to do, nothing touched
    got = _call(tris, p[:0], d[:0], counts[:0], contacts[:0], flag=4)
    assert got["status"] == 0 and got["flag"] == 4 and (got["i"] == -7).all()


def test_a_duplicated_triangle_through_the_whole_pipeline():
    """torus_mesh(40, 40) with triangle 1234 appended again as number n + 1: rays aimed at it find both copies at equal t, and
    whichever copy comes first in the library's list wins."""
    tris = torus_mesh(40, 40)
    k = 1234
    tris = np.concatenate([tris, tris[k - 1:k]])
    n = len(tris)
    rng = np.random.default_rng(3)
    w = rng.dirichlet((1.0, 1.0, 1.0), 64)
    target = (w[:, :, None] * tris[k - 1].reshape(1, 3, 3).astype(np.float64)).sum(1)
    normal = np.cross(tris[k - 1, 3:6] - tris[k - 1, 0:3], tris[k - 1, 6:9] - tris[k - 1, 0:3]).astype(np.float64)
    origin = target + 0.05 * normal / np.linalg.norm(normal)
    p, d = origin.astype(np.float32), (target - origin).astype(np.float32)
    for kind in (abi.BSPHERE, abi.BBOX):
        bvh, tdev = _build(tris, kind, abi.F32, abi.I32)
        got, trav = ibvh.raycast(bvh, tdev, cuda(p).t(), cuda(d).t(), all_hits=True)
        exp = _check_on_own_list(trav, got, tris, p, d, kind)
        contacts, cand = trav.contacts.cpu().numpy(), got.candidate_t.cpu().numpy()
        both = 0
        for r in range(len(p)):
            seg = np.nonzero(contacts[:, 1] == r + 1)[0]
            ia, ib = seg[contacts[seg, 0] == k], seg[contacts[seg, 0] == n]
            if len(ia) and len(ib) and np.isfinite(cand[ia[0]]) and got.index[r].item() in (k, n):
                both += 1
                assert cand[ia[0]] == cand[ib[0]] == got.t[r].item()
                assert got.index[r].item() == (k if ia[0] < ib[0] else n)
        assert both >= 32, both


def test_python_mirror_refuses_what_the_pass_cannot_resolve():
    tris, nr = _mesh("torus40", abi.F32)
    bvh, tdev = _build(tris, abi.BSPHERE, abi.F32, abi.I32)
    p, d = _ray_sets(tris, 500, np.float32)["random"]
    P, D = cuda(p).t(), cuda(d).t()
    with pytest.raises(ValueError, match="BFS"):
        ibvh.resolve_triangles(ibvh.traverse_rays(bvh, P, D, ibvh.BFSTraversal()), tdev, P, D)
    with pytest.raises(ValueError, match="positions"):
        ibvh.resolve_triangles(_rays_positions(bvh, P, D), tdev, P, D)
    with pytest.raises(ValueError):  # a list a callable filtered has no counts
        ibvh.resolve_triangles(ibvh.traverse_rays(bvh, P, D, narrow=lambda bv, pp, dd: bv.index > 0), tdev, P, D)
    with pytest.raises(ValueError):
        ibvh.resolve_triangles(ibvh.traverse(bvh), tdev, P, D)
    with pytest.raises(ValueError):
        ibvh.raycast(bvh, tdev, P, D, alg=ibvh.BFSTraversal())
    good = ibvh.traverse_rays(bvh, P, D)
    for bad in (tdev.to(torch.int32), tdev.to(torch.float16), tdev.cpu(), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.resolve_triangles(good, bad, P, D)
    with pytest.raises(ValueError):
        ibvh.resolve_triangles(good, tdev, P[:2], D[:2])
    with pytest.raises(ValueError):
        ibvh.resolve_triangles(good, tdev, P, D[:, :10])
    with pytest.raises(ValueError):
        ibvh.resolve_triangles(good, tdev, torch.cat([P, P], dim=1), torch.cat([D, D], dim=1))  # more rays than counts
    with pytest.raises(ValueError):
        ibvh.raycast(bvh, tdev.double(), P, D)      # not the BVH's leaf float type
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.resolve_triangles(good, tdev[:10], P, D)   # flag bit 1
    # (n, 3, 3) triangles and an empty batch are fine
    a = ibvh.resolve_triangles(good, tdev.reshape(-1, 3, 3), P, D)
    b = ibvh.resolve_triangles(good, tdev, P, D)
    assert torch.equal(a.index, b.index) and torch.equal(a.t, b.t)
    e, et = ibvh.raycast(bvh, tdev, P[:, :0], D[:, :0], all_hits=True)
    assert e.index.shape == (0,) and e.t.shape == (0,) and e.uv.shape == (0, 2) and e.candidate_t.shape == (0,) and et.num_contacts == 0
