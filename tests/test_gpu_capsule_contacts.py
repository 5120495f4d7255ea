"""ibvh_capsule_contacts / capsule_contacts on the GPU: counts, offsets, index, kind and the ORDER of every capsule's list are
equal, and d2 and both points BIT-EQUAL, to the brute force over all triangles of tests/capsule_checker.py — the definition of
the result — through the whole pipeline (volumes from triangles, build, count, scan, write) for every accepted float / index
combination, in the given order, through the Morton-sorted default path and counting only; tiny trees and built levels
straight through the C entry point with every output alone, NaN segments, negative and NaN radii, zero-length capsules and a
capsule inside a triangle's plane; offsets in a permuted order and the capacity guard; skin margins — the slab clause reads
the stored box — and refit; the index guard, the refusals, the empty batch, and one kernel per pass."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

import capsule_checker as cc  # noqa: E402
from capsule_checker import CAPSULES_PER_MESH as CAPSULES, HAND, HAND_CAPSULES  # noqa: E402
import mesh_query_kit as kit  # noqa: E402
from mesh_query_kit import FLOATS, NP_F, NP_I, build as _build, leaf_order as _leaf_order, stored_boxes as _stored_boxes, tf as _tf  # noqa: E402
from sphere_contacts_checker import mean_edge  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_capsule_contacts"
_assert_equal = functools.partial(kit.assert_equal, cc.QUERY)
_same = functools.partial(kit.same, cc.QUERY)
SENTINEL = {k: col.sentinel for k, col in cc.QUERY.columns.items()}


def _reference(mesh, flt):
    """(triangles, a, b, radii, the contacts in the order 1..n, the distances): the checker's shared, read-only case"""
    return cc.reference(mesh, NP_F[flt], CAPSULES[mesh])


def _call(bvh, tris, a, b, r, **kw):
    """count, scan on the host, write -> dict: counts, the outputs, both flag words and both statuses (kit.two_passes)"""
    return kit.two_passes(cc.QUERY, bvh, tris, (a, b, r), **kw)


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,floats,idx", [("torus40", "f32", abi.I32), ("torus40", "f32", abi.I64), ("torus40", "f64", abi.I32),
                                             ("torus40", "f64", abi.I64), ("torus40", "f32_under_f64", abi.I32),
                                             ("torus40", "f32_under_f64", abi.I64), ("torus64x63", "f32", abi.I32),
                                             ("torus64x63", "f64", abi.I32)])
def test_whole_pipeline_is_equal_to_the_brute_force(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, a, b, radii, bf, _ = _reference(mesh, leaf_flt)
    # what makes the comparison mean something (tests/test_host_capsules.py pins more of it on the host)
    per_kind = np.bincount(bf.kind, minlength=6)
    print(f"{mesh} {floats}: {len(bf.index)} contacts, kinds {per_kind.tolist()}, {int((bf.counts == 0).sum())} capsules without")
    assert per_kind.min() >= 20 and len(bf.index) >= 50 * len(a) and (bf.counts == 0).sum() >= 3
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    order = _leaf_order(bvh)
    assert sorted(order.tolist()) == list(range(1, len(tris) + 1)) and (np.diff(order) < 0).any()
    exp = cc.in_leaf_order(bf, order)
    assert (exp.index != bf.index).any()   # the leaf order is not the triangles' own: the order is being tested
    A, B, R = cuda(a).t(), cuda(b).t(), cuda(radii)
    got = ibvh.capsule_contacts(bvh, tdev, A, B, R, presorted=True)
    assert isinstance(got, ibvh.CapsuleContacts) and got.kind.dtype == torch.uint8
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.distance2.dtype == _tf(leaf_flt)
    _assert_equal(got, exp, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.capsule_contacts(bvh, tdev, A, B, R), exp, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.capsule_contacts(bvh, tdev.reshape(-1, 3, 3), A, B, R), exp, (mesh, floats, idx, "(n, 3, 3)"))
    _assert_equal(ibvh.capsule_contacts(bvh, tdev, A, B, R, count_only=True), exp, (mesh, floats, idx, "count"), count_only=True)
    _assert_equal(ibvh.capsule_contacts(bvh, tdev, A, B, R, count_only=True, presorted=True), exp, (mesh, floats, idx, "count, given"), count_only=True)


def test_one_radius_for_all():
    tris, a, b, _, _, _ = _reference("torus64x63", abi.F32)
    r = np.float32(1.5 * mean_edge(tris))
    bvh, tdev = _build(tris)
    exp = cc.brute_force_contacts(tris, a, b, np.full(len(a), r, np.float32), leaf_order=_leaf_order(bvh))
    assert (exp.counts == 0).sum() >= 3 and (exp.counts >= 2).sum() >= 50
    for radius in (float(r), r):
        _assert_equal(ibvh.capsule_contacts(bvh, tdev, cuda(a).t(), cuda(b).t(), radius), exp, "scalar")


# ---- 2. hand-made, straight through the C entry ------------------------------------------------------------------------
def _hand(n, dt):
    a, b, r = (np.array([c[j] for c in HAND_CAPSULES], dt) for j in range(3))
    return np.array(HAND[:n], dt), a, b, r


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (3, 2), (5, 1), (5, 2), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris, a, b, r = _hand(n, dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4}[n] and bvh.built_level == built_level
    order = _leaf_order(bvh)
    exp = cc.brute_force_contacts(tris, a, b, r, leaf_order=order, idt=NP_I[idx])
    got = _call(bvh, tris, a, b, r)
    _same(got, exp, (n, built_level))
    assert got["flag_count"] == 0 and got["flag"] == 0
    # what the checker itself says about these inputs
    first = exp.index == 1
    assert exp.kind[first & (exp.capsule == 0)] == 5 and exp.d2[first & (exp.capsule == 0)] == 0          # through the face, r = 0
    assert exp.d2[first & (exp.capsule == 1)] == exp.r2[1] and exp.counts[1] == min(n, 2) and exp.counts[2] == 0   # d2 == r * r; below
    assert exp.counts[5] >= 1 and exp.counts[6] == 1 and exp.counts[7] >= 1 and exp.counts[8] == (n >= 4)  # zero length; in the plane
    assert exp.counts[[10, 11, 14, 15, 16]].tolist() == [0] * 5 and exp.counts[12] == 1                   # -1, NaN, -Inf; NaN ends; -0.0
    assert exp.counts[13] == n                                                                            # +Inf admits every triangle
    if n == 5:
        assert exp.counts[9] >= 3 and (exp.index[exp.capsule == 13] == order).all() and (np.diff(order) < 0).any()
        assert {0, 1, 2, 5} <= set(exp.kind.tolist())
    # every output alone, some together; what was not asked for is not written
    for outs in ("i", "d", "s", "m", "k", "ik", "dsm"):
        _same(_call(bvh, tris, a, b, r, outs=outs), exp, outs, outs=outs)
    # num_capsules = 0 with a pre-set flag: nothing is touched
    none = _call(bvh, tris, a, b, r, num=0, flag=4, rows=3)
    assert none["status_count"] == 0 and none["status"] == 0 and none["flag_count"] == 4 and none["flag"] == 4
    assert (none["counts"] == -7).all() and all((none[k] == SENTINEL[k]).all() for k in "idsmk")
    # num_triangles below the largest leaf index: those leaves are skipped in both passes, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        cut = _call(bvh, tris, a, b, r, num_triangles=n - 2, flag=4)
        assert cut["flag_count"] == 6 and cut["flag"] == 6
        cut_exp = cc.brute_force_contacts(tris[:n - 2], a, b, r, leaf_order=order, leaf_boxes=None, idt=NP_I[idx])
        assert len(cut_exp.index) < len(exp.index)
        _same(cut, cut_exp, "guard")


def test_zero_length_capsules_are_spheres():
    """b == a: every axis is still, the cut rule cannot hit (det == 0) and the point on the segment is a.  Candidate 0 is
    sphere_contacts' evaluation; an edge candidate replaces it only where its own rounding makes its d2 strictly smaller, so
    where kind == 0 the row carries sphere_contacts' d2 and point bit for bit"""
    tris, a, _, radii, _, _ = _reference("torus40", abi.F32)
    a, radii = a[:150], radii[:150]
    bvh, tdev = _build(tris)
    A, R = cuda(a).t(), cuda(radii)
    got = ibvh.capsule_contacts(bvh, tdev, A, A.clone(), R)
    exp = cc.brute_force_contacts(tris, a, a.copy(), radii, leaf_order=_leaf_order(bvh))
    assert len(exp.index) > 5000 and (exp.kind != 1).all() and (exp.kind != cc.CUT).all() and (exp.kind == 0).mean() > 0.5
    assert kit.bits(exp.point_segment) == kit.bits(a[exp.capsule])
    _assert_equal(got, exp, "zero length")
    spheres = ibvh.sphere_contacts(bvh, tdev, A, R)
    mine = {(int(s), int(i)): (d, tuple(p)) for s, i, d, p, k in zip(got.capsule.cpu().numpy(), got.index.cpu().numpy(), got.distance2.cpu().numpy(),
                                                                      got.point_mesh.cpu().numpy(), exp.kind) if k == 0}
    theirs = {(int(s), int(i)): (d, tuple(p)) for s, i, d, p in zip(spheres.sphere.cpu().numpy(), spheres.index.cpu().numpy(),
                                                                    spheres.distance2.cpu().numpy(), spheres.point.cpu().numpy())}
    assert len(mine) > 2500 and all(theirs[key] == value for key, value in mine.items())


# ---- 3. offsets and capacity -------------------------------------------------------------------------------------------
def test_offsets_in_a_permuted_order_and_the_capacity_guard():
    tris, a, b, radii, bf, _ = _reference("torus40", abi.F32)
    keep = slice(0, 100)
    bvh, _ = _build(tris)
    part = cc.Contacts()
    rows = bf.capsule < 100
    for field in ("capsule", "index", "d2", "point_segment", "point_mesh", "kind"):
        setattr(part, field, getattr(bf, field)[rows])
    part.counts = bf.counts[keep]
    part.offsets = bf.offsets[:101]
    exp = cc.in_leaf_order(part, _leaf_order(bvh))
    assert len(exp.index) > 1000 and (exp.counts > 0).sum() > 50 and (exp.counts >= 3).any()
    kit.check_offsets_and_capacity(cc.QUERY, functools.partial(_call, bvh, tris, a[keep], b[keep], radii[keep]), exp)


# ---- 4. skin, refit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_follow_the_stored_boxes(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, a, b, radii, bf, _ = _reference("torus40", leaf_flt)
    a, b, radii = a[:120], b[:120], radii[:120]
    A, B, R = cuda(a).t(), cuda(b).t(), cuda(radii)
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    boxes = _stored_boxes(bvh, len(tris))
    tight = cc.tcc.tight_boxes(tris)
    assert (boxes[:, :3] < tight[:, :3]).all() and (boxes[:, 3:] > tight[:, 3:]).all()
    exp = cc.brute_force_contacts(tris, a, b, radii, leaf_order=_leaf_order(bvh), leaf_boxes=boxes)
    assert exp.slab_dropped == 0 and len(exp.index) > 5000
    for presorted in (True, False):
        _assert_equal(ibvh.capsule_contacts(bvh, tdev, A, B, R, presorted=presorted), exp, (floats, "skin", presorted))
    # refit the tight build to moved vertices: the moved triangles' brute force on their stored boxes
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    moved = (tris + 0.01 * (rng.random(tris.shape) - 0.5)).astype(dt)
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = cc.brute_force_contacts(moved, a, b, radii, leaf_order=_leaf_order(bvh), leaf_boxes=_stored_boxes(bvh, len(tris)))
    assert (exp.counts != bf.counts[:120]).any() and len(exp.index) > 5000
    for presorted in (True, False):
        _assert_equal(ibvh.capsule_contacts(bvh, mdev, A, B, R, presorted=presorted), exp, (floats, "refit", presorted))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, a, b, radii, bf, _ = _reference("torus40", abi.F32)
    n = len(a)
    A, B, R = cuda(a).t(), cuda(b).t(), cuda(radii)
    f = getattr(lib.load(), NAME)
    out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        dt = NP_F[bvh.types.leaf_float]
        ad, bd, rd = cuda(a.astype(dt)), cuda(b.astype(dt)), cuda(radii.astype(dt))
        for mode, counts, offsets, index in ((abi.CAPSULES_COUNT, api._ptr(out), None, None), (abi.CAPSULES_WRITE, None, api._ptr(out), api._ptr(out))):
            st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(ad), api._ptr(bd), api._ptr(rd), n, mode, counts, offsets, n,
                   index, None, None, None, None, None, api._stream())
            torch.cuda.synchronize()
            assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), (what, mode)
        with pytest.raises(ValueError):
            ibvh.capsule_contacts(bvh, tdev, ad.t(), bd.t(), rd)
    bvh, tdev = _build(tris)
    with pytest.raises(ValueError):
        ibvh.capsule_contacts(bvh, tdev.double(), A, B, R)          # triangles of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.capsule_contacts(bvh, bad, A, B, R)
    for bad in (A.cpu(), A.double(), A.t(), A[:2], A[:, :n - 1], A.reshape(-1), a):
        with pytest.raises(ValueError):
            ibvh.capsule_contacts(bvh, tdev, bad, B, R)
        with pytest.raises(ValueError):
            ibvh.capsule_contacts(bvh, tdev, A, bad, R)
    for bad in (R.cpu(), R.double(), R[:n - 1], R.reshape(-1, 1), radii, None, "1", True, [0.1] * n):
        with pytest.raises(ValueError):
            ibvh.capsule_contacts(bvh, tdev, A, B, bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.capsule_contacts(bvh, tdev[:10], A, B, R)              # flag bit 1
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.capsule_contacts(bvh, tdev[:10], A, B, R, count_only=True)
    e = ibvh.capsule_contacts(bvh, tdev, A[:, :0], B[:, :0], R[:0])
    assert e.offsets.tolist() == [0] and e.counts.shape == (0,) and e.index.shape == (0,) and e.index.dtype == torch.int32
    assert e.distance2.shape == (0,) and e.point_segment.shape == e.point_mesh.shape == (0, 3) and e.kind.shape == e.capsule.shape == (0,)
    far = ibvh.capsule_contacts(bvh, tdev, A + 100, B + 100, R)     # no contact at all: no write pass, empty outputs
    assert far.offsets.tolist() == [0] * (n + 1) and far.index.shape == (0,) and far.point_mesh.shape == (0, 3) and far.capsule.shape == (0,)


# ---- 6. one kernel per pass --------------------------------------------------------------------------------------------
def test_each_pass_is_one_kernel_of_the_new_translation_unit():
    tris, a, b, radii, bf, _ = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    A, B, R = cuda(a).t(), cuda(b).t(), cuda(radii)
    # the write pass goes straight through the C entry, and writes index and kind alone
    kit.check_each_pass_is_one_kernel(cc.QUERY, bvh, tdev, functools.partial(ibvh.capsule_contacts, bvh, tdev, A, B, R, presorted=True),
                                      (A.t().contiguous(), B.t().contiguous(), R), (), "ik")
