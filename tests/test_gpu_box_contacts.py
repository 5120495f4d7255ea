"""ibvh_box_contacts / box_contacts / voxelize on the GPU: counts, offsets, index, the inside mask and the ORDER of every box's
list are equal, bit for bit, to the brute force over all triangles of tests/box_contacts_checker.py — the definition of the
result — through the whole pipeline (volumes from triangles, build, count, scan, write) for every accepted float / index
combination, in the given order, through the Morton-sorted default path, counting only, and with no rotations on the boxes
that carry the identity; tiny trees and built levels straight through the C entry point with every output alone, oriented and
axis-aligned hand-made boxes, plates, points, negative and NaN half extents, NaN and infinite centres and rotations; offsets
in a permuted order and the capacity guard; skin margins — the box clause reads the stored box — and refit; the index guard,
the refusals, the empty batch, one kernel per pass, and the voxel grid."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

import box_contacts_checker as bc  # noqa: E402
from capsule_checker import HAND  # noqa: E402
import mesh_query_kit as kit  # noqa: E402
from mesh_query_kit import FLOATS, NP_F, NP_I, build as _build, leaf_order as _leaf_order, stored_boxes as _stored_boxes, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_box_contacts"
BOXES = {"torus40": bc.N_BOXES, "torus64x63": 100}   # 3,200 triangles; 8,064: a leaf count that is no power of two
_assert_equal = functools.partial(kit.assert_equal, bc.QUERY)
_same = functools.partial(kit.same, bc.QUERY)
SENTINEL = {k: col.sentinel for k, col in bc.QUERY.columns.items()}


def _reference(mesh, flt):
    """(triangles, c, h, R, the contacts in the order 1..n): the checker's shared, read-only case"""
    return bc.reference(mesh, NP_F[flt], BOXES[mesh])


def _call(bvh, tris, c, h, R, **kw):
    """count, scan on the host, write -> dict: counts, the outputs, both flag words and both statuses (kit.two_passes)"""
    return kit.two_passes(bc.QUERY, bvh, tris, (c, h, R), **kw)


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,floats,idx", [("torus40", "f32", abi.I32), ("torus40", "f32", abi.I64), ("torus40", "f64", abi.I32),
                                             ("torus40", "f64", abi.I64), ("torus40", "f32_under_f64", abi.I32),
                                             ("torus40", "f32_under_f64", abi.I64), ("torus64x63", "f32", abi.I32),
                                             ("torus64x63", "f64", abi.I32)])
def test_whole_pipeline_is_equal_to_the_brute_force(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, c, h, R, bf = _reference(mesh, leaf_flt)
    # what makes the comparison mean something (tests/test_host_boxes.py pins more of it on the host)
    classes = [int((bf.inside == 0).sum()), int(((bf.inside > 0) & (bf.inside < 7)).sum()), int((bf.inside == 7).sum())]
    print(f"{mesh} {floats}: {len(bf.index)} contacts, inside 0 / partial / 7 {classes}, refused first {bf.refused_first.tolist()}, "
          f"{int((bf.counts == 0).sum())} boxes without")
    assert min(classes) >= 50 and bf.refused_first.min() >= 20 and len(bf.index) >= 50 * len(c) and (bf.counts == 0).sum() >= 3
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    order = _leaf_order(bvh)
    assert sorted(order.tolist()) == list(range(1, len(tris) + 1)) and (np.diff(order) < 0).any()
    exp = bc.in_leaf_order(bf, order)
    assert (exp.index != bf.index).any()   # the leaf order is not the triangles' own: the order is being tested
    Cd, Hd, Rd = cuda(c).t(), cuda(h).t(), cuda(R)
    got = ibvh.box_contacts(bvh, tdev, Cd, Hd, Rd, presorted=True)
    assert isinstance(got, ibvh.BoxContacts) and got.inside.dtype == torch.uint8
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64)
    _assert_equal(got, exp, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.box_contacts(bvh, tdev, Cd, Hd, Rd), exp, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.box_contacts(bvh, tdev.reshape(-1, 3, 3), Cd, Hd, Rd), exp, (mesh, floats, idx, "(n, 3, 3)"))
    _assert_equal(ibvh.box_contacts(bvh, tdev, Cd, Hd, Rd, count_only=True), exp, (mesh, floats, idx, "count"), count_only=True)
    _assert_equal(ibvh.box_contacts(bvh, tdev, Cd, Hd, Rd, count_only=True, presorted=True), exp, (mesh, floats, idx, "count, given"), count_only=True)
    # the quarter that carries the identity, with no rotations at all: the same bits
    quarter = len(c) // 4
    part = bc.first(exp, quarter)
    assert len(part.index) >= 50 * quarter // 2
    for presorted in (True, False):
        _assert_equal(ibvh.box_contacts(bvh, tdev, Cd[:, :quarter], Hd[:, :quarter], None, presorted=presorted), part, (mesh, floats, idx, "no rotations", presorted))


def test_half_extents_for_all_boxes():
    tris, c, _, R, _ = _reference("torus64x63", abi.F32)
    bvh, tdev = _build(tris)
    e = np.float32(0.2)
    for value, h in ((float(e), np.full((len(c), 3), e, np.float32)), (e, np.full((len(c), 3), e, np.float32)),
                     ((0.1, 0.25, 0.5), np.tile(np.array([0.1, 0.25, 0.5], np.float32), (len(c), 1)))):
        exp = bc.brute_force_contacts(tris, c, h, R, leaf_order=_leaf_order(bvh))
        assert (exp.counts == 0).sum() >= 3 and (exp.counts >= 2).sum() >= 50
        _assert_equal(ibvh.box_contacts(bvh, tdev, cuda(c).t(), value, cuda(R)), exp, ("for all", value))


# ---- 2. hand-made, straight through the C entry ------------------------------------------------------------------------
def _hand(n, dt):
    return (np.array(HAND[:n], dt),) + bc.hand_boxes(dt)


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (3, 2), (5, 1), (5, 2), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris, c, h, R = _hand(n, dt)
    # one more box around everything: its list is the leaf order
    c, h, R = np.concatenate([c, [[3, 3, 3]]]).astype(dt), np.concatenate([h, [[8, 8, 8]]]).astype(dt), np.concatenate([R, [bc.RZ45]]).astype(dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4}[n] and bvh.built_level == built_level
    order = _leaf_order(bvh)
    exp = bc.brute_force_contacts(tris, c, h, R, leaf_order=order, idt=NP_I[idx])
    got = _call(bvh, tris, c, h, R)
    _same(got, exp, (n, built_level))
    assert got["flag_count"] == 0 and got["flag"] == 0
    # what the checker itself says about these inputs
    assert (exp.index[exp.box == len(c) - 1] == order).all() and exp.counts[-1] == n and (exp.inside[exp.box == len(c) - 1] == 7).all()
    assert (exp.counts > 0).sum() >= 10 and (exp.counts == 0).sum() >= len(bc.INVALID) and {0, 7} <= set(exp.inside.tolist())
    if n == 5:
        assert (np.diff(order) < 0).any() and exp.counts.max() == 5
    # no rotations at all, on the boxes that carry the identity
    k = bc.IDENTITY
    assert (R[:k] == np.eye(3, dtype=dt)).all() and not (R[k:] == np.eye(3, dtype=dt)).all(axis=(1, 2)).any()
    plain = bc.brute_force_contacts(tris, c[:k], h[:k], None, leaf_order=order, idt=NP_I[idx])
    assert kit.bits(plain.index) == kit.bits(bc.first(exp, k).index) and kit.bits(plain.inside) == kit.bits(bc.first(exp, k).inside)
    _same(_call(bvh, tris, c[:k], h[:k], None), plain, "no rotations")
    # every output alone and both together; what was not asked for is not written
    for outs in ("i", "m", "im"):
        _same(_call(bvh, tris, c, h, R, outs=outs), exp, outs, outs=outs)
    # num_boxes = 0 with a pre-set flag: nothing is touched
    none = _call(bvh, tris, c, h, R, num=0, flag=4, rows=3)
    assert none["status_count"] == 0 and none["status"] == 0 and none["flag_count"] == 4 and none["flag"] == 4
    assert (none["counts"] == -7).all() and all((none[k] == SENTINEL[k]).all() for k in "im")
    # num_triangles below the largest leaf index: those leaves are skipped in both passes, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        cut = _call(bvh, tris, c, h, R, num_triangles=n - 2, flag=4)
        assert cut["flag_count"] == 6 and cut["flag"] == 6
        cut_exp = bc.brute_force_contacts(tris[:n - 2], c, h, R, leaf_order=order, leaf_boxes=None, idt=NP_I[idx])
        assert len(cut_exp.index) < len(exp.index)
        _same(cut, cut_exp, "guard")


# ---- 3. offsets and capacity -------------------------------------------------------------------------------------------
def test_offsets_in_a_permuted_order_and_the_capacity_guard():
    tris, c, h, R, bf = _reference("torus40", abi.F32)
    keep = slice(0, 100)
    bvh, _ = _build(tris)
    exp = bc.in_leaf_order(bc.first(bf, 100), _leaf_order(bvh))
    assert len(exp.index) > 1000 and (exp.counts > 0).sum() > 50 and (exp.counts >= 3).any()
    kit.check_offsets_and_capacity(bc.QUERY, functools.partial(_call, bvh, tris, c[keep], h[keep], R[keep]), exp)


# ---- 4. skin, refit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_follow_the_stored_boxes(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, c, h, R, bf = _reference("torus40", leaf_flt)
    c, h, R = c[:120], h[:120], R[:120]
    Cd, Hd, Rd = cuda(c).t(), cuda(h).t(), cuda(R)
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    boxes = _stored_boxes(bvh, len(tris))
    tight = bc.tcc.tight_boxes(tris)
    assert (boxes[:, :3] < tight[:, :3]).all() and (boxes[:, 3:] > tight[:, 3:]).all()
    exp = bc.brute_force_contacts(tris, c, h, R, leaf_order=_leaf_order(bvh), leaf_boxes=boxes)
    assert len(exp.index) > 5000 and exp.refused_first.sum() > bc.brute_force_contacts(tris, c, h, R).refused_first.sum()   # the skin admits more pairs to (ii)
    for presorted in (True, False):
        _assert_equal(ibvh.box_contacts(bvh, tdev, Cd, Hd, Rd, presorted=presorted), exp, (floats, "skin", presorted))
    # refit the tight build to moved vertices: the moved triangles' brute force on their stored boxes
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    moved = (tris + 0.01 * (rng.random(tris.shape) - 0.5)).astype(dt)
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = bc.brute_force_contacts(moved, c, h, R, leaf_order=_leaf_order(bvh), leaf_boxes=_stored_boxes(bvh, len(tris)))
    assert (exp.counts != bf.counts[:120]).any() and len(exp.index) > 5000
    for presorted in (True, False):
        _assert_equal(ibvh.box_contacts(bvh, mdev, Cd, Hd, Rd, presorted=presorted), exp, (floats, "refit", presorted))


def test_a_stored_box_moved_off_its_triangle_drops_the_contact():
    """clause (i) reads the STORED box, not the triangle's own: leaves refitted to boxes far from their triangles give no contact
    although the 13 axes admit thousands"""
    tris, c, h, R, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    vols = ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32))
    ibvh.refit(bvh, vols + 100)
    got = ibvh.box_contacts(bvh, tdev, cuda(c).t(), cuda(h).t(), cuda(R))
    assert len(bf.index) > 5000 and got.index.shape == (0,) and int(got.counts.sum()) == 0


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, c, h, R, bf = _reference("torus40", abi.F32)
    n = len(c)
    Cd, Hd, Rd = cuda(c).t(), cuda(h).t(), cuda(R)
    f = getattr(lib.load(), NAME)
    out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        dt = NP_F[bvh.types.leaf_float]
        cd, hd, rd = cuda(c.astype(dt)), cuda(h.astype(dt)), cuda(R.astype(dt))
        for mode, counts, offsets, index in ((abi.BOXES_COUNT, api._ptr(out), None, None), (abi.BOXES_WRITE, None, api._ptr(out), api._ptr(out))):
            st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(cd), api._ptr(hd), api._ptr(rd), n, mode, counts, offsets, n,
                   index, None, None, api._stream())
            torch.cuda.synchronize()
            assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), (what, mode)
        with pytest.raises(ValueError):
            ibvh.box_contacts(bvh, tdev, cd.t(), hd.t(), rd)
    bvh, tdev = _build(tris)
    with pytest.raises(ValueError):
        ibvh.box_contacts(bvh, tdev.double(), Cd, Hd, Rd)           # triangles of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.box_contacts(bvh, bad, Cd, Hd, Rd)
    for bad in (Cd.cpu(), Cd.double(), Cd.t(), Cd[:2], Cd.reshape(-1), c):
        with pytest.raises(ValueError):
            ibvh.box_contacts(bvh, tdev, bad, Hd, Rd)
    for bad in (Hd.cpu(), Hd.double(), Hd.t(), Hd[:2], Hd[:, :n - 1], Hd.reshape(-1), h, None, "1", True, (1, 2), (1, 2, "3"), [0.1] * 4):
        with pytest.raises(ValueError):
            ibvh.box_contacts(bvh, tdev, Cd, bad, Rd)
    for bad in (Rd.cpu(), Rd.double(), Rd[:n - 1], Rd.reshape(n, 9), Rd[:, :2], R, 1.0):
        with pytest.raises(ValueError):
            ibvh.box_contacts(bvh, tdev, Cd, Hd, bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.box_contacts(bvh, tdev[:10], Cd, Hd, Rd)               # flag bit 1
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.box_contacts(bvh, tdev[:10], Cd, Hd, Rd, count_only=True)
    e = ibvh.box_contacts(bvh, tdev, Cd[:, :0], Hd[:, :0], Rd[:0])
    assert e.offsets.tolist() == [0] and e.counts.shape == (0,) and e.index.shape == (0,) and e.index.dtype == torch.int32
    assert e.inside.shape == e.box.shape == (0,) and e.inside.dtype == torch.uint8
    far = ibvh.box_contacts(bvh, tdev, Cd + 100, Hd, Rd)            # no contact at all: no write pass, empty outputs
    assert far.offsets.tolist() == [0] * (n + 1) and far.index.shape == (0,) and far.inside.shape == (0,) and far.box.shape == (0,)
    for bad in (dict(origin=(0, 0)), dict(spacing=(1, 2)), dict(shape=(2, 2)), dict(shape=(2, 2, -1)), dict(spacing="1"), dict(shape=(2.0, 2, 2))):
        with pytest.raises(ValueError):
            ibvh.voxelize(bvh, tdev, **dict(dict(origin=(0, 0, 0), spacing=1.0, shape=(2, 2, 2)), **bad))


# ---- 6. one kernel per pass --------------------------------------------------------------------------------------------
def test_each_pass_is_one_kernel_of_the_new_translation_unit():
    tris, c, h, R, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    Cd, Hd, Rd = cuda(c).t(), cuda(h).t(), cuda(R)
    # the write pass goes straight through the C entry, and writes both columns
    kit.check_each_pass_is_one_kernel(bc.QUERY, bvh, tdev, functools.partial(ibvh.box_contacts, bvh, tdev, Cd, Hd, Rd, presorted=True),
                                      (Cd.t().contiguous(), Hd.t().contiguous(), Rd), (), "im")


# ---- 7. the voxel grid -------------------------------------------------------------------------------------------------
def _cells(shape, dt):
    """(nx * ny * nz, 3): i + 0.5, j + 0.5, k + 0.5 of every cell, k fastest"""
    return np.stack(np.meshgrid(*[np.arange(s, dtype=dt) + dt(0.5) for s in shape], indexing="ij"), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("floats", ["f32", "f64"])
def test_voxelize_is_the_count_pass_over_the_grids_cells(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris = _reference("torus40", leaf_flt)[0]
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    pts = tris.reshape(-1, 3).astype(np.float64)
    lo, up = pts.min(axis=0), pts.max(axis=0)
    lo, up = lo - 0.05 * (up - lo), up + 0.05 * (up - lo)              # the bounding box, inflated
    shape = (24, 24, 24)
    origin, spacing = lo.astype(dt), ((up - lo) / 24).astype(dt)
    got = ibvh.voxelize(bvh, tdev, tuple(float(x) for x in origin), tuple(float(x) for x in spacing), shape)
    assert got.dtype == torch.bool and tuple(got.shape) == shape and got.is_cuda
    # the cells as the contract states them: centre origin + (i + 0.5) * spacing, half extent spacing / 2, in the BVH's float type
    ijk = _cells(shape, dt)
    centers = origin + ijk * spacing
    half = np.broadcast_to(spacing / dt(2), centers.shape).copy()
    assert centers.dtype == dt and half.dtype == dt
    exp = bc.brute_force_contacts(tris, centers, half, None, chunk=256)
    filled = (exp.counts > 0).reshape(shape)
    print(f"{int(filled.sum())} of {filled.size} cells hold a triangle")
    assert filled.sum() >= 200 and (~filled).sum() >= filled.size // 2
    assert (got.cpu().numpy() == filled).all()
    # one number for all three spacings, and an empty grid
    one = ibvh.voxelize(bvh, tdev, tuple(float(x) for x in origin), float(spacing[0]), (4, 3, 2))
    cube = bc.brute_force_contacts(tris, (origin + _cells((4, 3, 2), dt) * spacing[0]).astype(dt), np.full((24, 3), spacing[0] / dt(2), dt), None)
    assert (one.cpu().numpy() == (cube.counts > 0).reshape(4, 3, 2)).all()
    assert tuple(ibvh.voxelize(bvh, tdev, (0, 0, 0), 1.0, (0, 3, 2)).shape) == (0, 3, 2)

