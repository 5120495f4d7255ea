"""ibvh_segment_distances / segment_distances on the GPU: index and kind are equal, and the bits of d2 and of both points, to the
brute force over all triangles of tests/capsule_checker.py — the definition of the result — through the whole pipeline
(volumes from triangles, build, one launch) for every accepted float combination and both index types, in the given order and
through the Morton-sorted default path; every output alone; a radius, inclusive at exactly one query's d2, zero and huge;
built levels, skin margins, refit, a one-triangle mesh and a leaf count that is no power of two; NaN segments and a NaN
radius; the index guard; the refusals, the empty batch and the one launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

import capsule_checker as cc  # noqa: E402
from capsule_checker import CAPSULES_PER_MESH as CAPSULES, HAND, HAND_CAPSULES  # noqa: E402
from mesh_query_kit import FLOATS, NP_F, assert_one_kernel, bits, build as _build, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_segment_distances"
KERNEL = "segdist_walk_kernel"
nan = np.nan


def _reference(mesh, flt):
    """(triangles, a, b, the unbounded brute force): the checker's shared, read-only case"""
    tris, a, b, _, _, dist = cc.reference(mesh, NP_F[flt], CAPSULES[mesh])
    return tris, a, b, dist


def _assert_equal(got, exp, what):
    """index and kind by value, d2 and both points BIT FOR BIT"""
    assert isinstance(got, ibvh.SegmentDistances), what
    for field in cc.FIELDS:
        g, e = getattr(got, field).cpu().numpy(), getattr(exp, field)
        assert g.shape == e.shape, (what, field)
        if field == "index":
            assert (g == e).all(), (what, field, int((g != e).sum()))
        else:
            assert g.dtype == e.dtype and bits(g) == bits(e), (what, field, int((g != e).sum()))


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,floats,idx", [("torus40", "f32", abi.I32), ("torus40", "f32", abi.I64), ("torus40", "f64", abi.I32),
                                             ("torus40", "f64", abi.I64), ("torus40", "f32_under_f64", abi.I32),
                                             ("torus40", "f32_under_f64", abi.I64), ("torus64x63", "f32", abi.I32),
                                             ("torus64x63", "f64", abi.I32)])
def test_whole_pipeline_is_equal_to_the_checker(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, a, b, bf = _reference(mesh, leaf_flt)
    n = len(a)
    # what makes the comparison mean something (tests/test_host_capsules.py pins more of it on the host)
    assert (bf.index != 0).all() and (bf.kind == cc.CUT).sum() >= n // 8 and len(set(bf.kind.tolist())) == 6 and bf.ties.max() >= 2
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    A, B = cuda(a).t(), cuda(b).t()
    got = ibvh.segment_distances(bvh, tdev, A, B, presorted=True)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.d2.dtype == _tf(leaf_flt)
    assert got.index.shape == got.d2.shape == got.kind.shape == (n,) and got.point_segment.shape == got.point_mesh.shape == (n, 3)
    assert got.kind.dtype == torch.uint8
    _assert_equal(got, bf, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.segment_distances(bvh, tdev, A, B), bf, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.segment_distances(bvh, tdev.reshape(-1, 3, 3), A, B), bf, (mesh, floats, idx, "(n, 3, 3)"))


# ---- 2. straight through the C entry -----------------------------------------------------------------------------------
OUTS = "idsmk"
SENTINEL = dict(i=-7, d=-7, s=-7, m=-7, k=249)


def _call(bvh, tris, a, b, max_d2=None, num_triangles=None, flag=0, outs=OUTS, num_segments=None):
    """-> dict of numpy outputs (prefilled with a sentinel so that 'not written' is visible), the flag word, the status"""
    n = len(a) if num_segments is None else num_segments
    rows = max(len(a), 1)
    T, Ad, Bd = cuda(np.array(tris)), cuda(np.array(a)), cuda(np.array(b))   # (copies: the shared reference arrays are read-only)
    ft, idt = _tf(bvh.types.leaf_float), api._torch_index(bvh.types.index_type)
    o = {"i": torch.full((rows,), -7, dtype=idt, device="cuda"), "d": torch.full((rows,), -7, dtype=ft, device="cuda"),
         "s": torch.full((rows, 3), -7, dtype=ft, device="cuda"), "m": torch.full((rows, 3), -7, dtype=ft, device="cuda"),
         "k": torch.full((rows,), 249, dtype=torch.uint8, device="cuda")}
    fl = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    ptr = lambda k: api._ptr(o[k]) if k in outs else None
    r2 = None if max_d2 is None else C.byref((C.c_float if ft == torch.float32 else C.c_double)(max_d2))
    st = getattr(lib.load(), NAME)(C.byref(bvh.struct()), api._ptr(T), len(tris) if num_triangles is None else num_triangles,
                                   api._ptr(Ad), api._ptr(Bd), n, r2, ptr("i"), ptr("d"), ptr("s"), ptr("m"), ptr("k"), api._ptr(fl),
                                   api._stream())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["flag"], out["status"] = int(fl.item()), st
    return out


def _same(got, exp, what=None, outs=OUTS):
    assert got["status"] == 0, what
    for k, e in zip(OUTS, (exp.index, exp.d2, exp.point_segment, exp.point_mesh, exp.kind)):
        if k in outs:
            assert (got[k] == e).all() if k == "i" else (got[k].dtype == e.dtype and bits(got[k]) == bits(e)), (what, k)
        else:
            assert (got[k] == SENTINEL[k]).all(), (what, k, "not asked for, yet written")


def test_every_output_alone_and_all_together():
    tris, a, b, bf = _reference("torus40", abi.F32)
    bvh, _ = _build(tris)
    for outs in ("i", "d", "s", "m", "k", "ik", "dsm", OUTS):
        got = _call(bvh, tris, a, b, outs=outs)
        _same(got, bf, outs, outs=outs)
        assert got["flag"] == 0
    # fewer segments than rows: the rows behind them are untouched
    got = _call(bvh, tris, a, b, num_segments=77)
    assert got["status"] == 0 and (got["i"][:77] == bf.index[:77]).all() and (got["i"][77:] == -7).all() and (got["k"][77:] == 249).all()
    assert bits(got["d"][:77]) == bits(bf.d2[:77]) and (got["d"][77:] == -7).all() and (got["s"][77:] == -7).all() and (got["m"][77:] == -7).all()


# ---- 3. a radius -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_max_distance(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, a, b, bf = _reference("torus40", leaf_flt)
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    A, B = cuda(a).t(), cuda(b).t()
    radius = float(np.sqrt(np.median(bf.d2[bf.d2 > 0].astype(np.float64))))     # half of the segments that are clear of the mesh
    for what, r in (("the median gap", radius), ("zero", 0.0), ("huge", 1e30)):
        with np.errstate(over="ignore"):
            r2 = dt(r) * dt(r)                                                # squared in the triangles' dtype, as the host does
        exp = cc.limited(bf, r2)
        share = (exp.index != 0).mean()
        if what == "the median gap":
            assert share >= 0.2 and 1 - share >= 0.2, share                   # on the checker's result alone
        if what == "zero":
            assert ((exp.index != 0) == (bf.d2 == 0)).all() and (exp.index != 0).sum() >= 50
        for presorted in (True, False):
            _assert_equal(ibvh.segment_distances(bvh, tdev, A, B, max_distance=r, presorted=presorted), exp, (floats, what, presorted))
    # the radius is inclusive: the squared distance of one segment, handed to the C entry as it is, and one unit below it
    k = int(np.flatnonzero(bf.d2 > 0)[7])
    got = _call(bvh, tris, a, b, max_d2=bf.d2[k])
    _same(got, cc.limited(bf, bf.d2[k]), "d2 of one segment")
    assert got["i"][k] == bf.index[k] != 0
    below = np.nextafter(bf.d2[k], dt(0))
    got = _call(bvh, tris, a, b, max_d2=below)
    _same(got, cc.limited(bf, below), "one unit below")
    assert got["i"][k] == 0


# ---- 4. trees and meshes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", ["f32", "f64"])
@pytest.mark.parametrize("built_level", [2, 4])
def test_built_levels(built_level, floats):
    leaf_flt, node_flt = FLOATS[floats]
    tris, a, b, bf = _reference("torus40", leaf_flt)
    bvh, tdev = _build(tris, leaf_flt, node_flt, built_level=built_level)
    assert bvh.built_level == built_level
    _assert_equal(ibvh.segment_distances(bvh, tdev, cuda(a).t(), cuda(b).t()), bf, (built_level, floats))


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_leaf_boxes_with_a_skin_give_the_same_result_and_refit_follows_the_moved_mesh(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, a, b, bf = _reference("torus40", leaf_flt)
    A, B = cuda(a).t(), cuda(b).t()
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)     # the definition reads the triangle's own box, not the stored one
    for presorted in (True, False):
        _assert_equal(ibvh.segment_distances(bvh, tdev, A, B, presorted=presorted), bf, (floats, "skin", presorted))
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    moved = (tris + 0.01 * (rng.random(tris.shape) - 0.5)).astype(dt)
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = cc.brute_force_distances(moved, a[:120], b[:120])
    assert (exp.d2 != bf.d2[:120]).any()
    _assert_equal(ibvh.segment_distances(bvh, mdev, A[:, :120], B[:, :120]), exp, (floats, "refit"))


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (2, 2), (3, 2), (5, 1), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt):
    dt = NP_F[flt]
    tris = np.array(HAND[:n], dt)
    a, b = (np.array([c[j] for c in HAND_CAPSULES], dt) for j in range(2))
    bvh, _ = _build(tris, flt, built_level=built_level)
    exp = cc.brute_force_distances(tris, a, b)
    assert (exp.index[[15, 16]] == 0).all() and (exp.index[:14] != 0).all()        # a NaN segment has no answer
    assert exp.kind[0] == cc.CUT and exp.d2[0] == 0 and exp.d2[[6, 7, 12]].tolist() == [0, 0, 0]   # through, on and inside the plane
    got = _call(bvh, tris, a, b)
    _same(got, exp, (n, built_level))
    assert got["flag"] == 0 and np.isinf(got["d"][[15, 16]]).all() and (got["s"][[15, 16]] == 0).all() and (got["m"][[15, 16]] == 0).all()
    assert (got["k"][[15, 16]] == 0).all()
    _same(_call(bvh, tris, a, b, max_d2=0.0625), cc.brute_force_distances(tris, a, b, max_d2=0.0625), (n, built_level, "radius"))
    _same(_call(bvh, tris, a, b, max_d2=0.0), cc.brute_force_distances(tris, a, b, max_d2=0.0), (n, built_level, "the zero radius"))
    for r2 in (nan, -1.0):
        none = _call(bvh, tris, a, b, max_d2=r2)
        _same(none, cc.brute_force_distances(tris, a, b, max_d2=r2), (n, built_level, r2))
        assert (none["i"] == 0).all() and np.isinf(none["d"]).all()


def test_duplicate_triangles_the_smaller_index_wins():
    tris, a, b, bf = _reference("torus40", abi.F32)
    winners = np.unique(bf.index[:150])
    twice = np.concatenate([tris[winners - 1], tris])          # every winner once more, under a smaller index: it wins the tie
    exp = cc.brute_force_distances(twice, a[:150], b[:150])
    assert (exp.ties >= 2).all() and (exp.index <= len(winners)).all() and len(winners) >= 50
    bvh, _ = _build(twice)
    _same(_call(bvh, twice, a[:150], b[:150]), exp, "duplicates")


# ---- 5. the index guard, refusals, the empty batch, one launch -----------------------------------------------------------
def test_a_leaf_index_outside_the_mesh_raises_flag_bit_1_and_is_skipped():
    tris, a, b, bf = _reference("torus40", abi.F32)
    a, b = a[:150], b[:150]
    bvh, tdev = _build(tris)
    exp = cc.brute_force_distances(tris[:2000], a, b)           # leaves 2001..3200 name no row of the 2,000 given
    assert (exp.index != bf.index[:150]).sum() >= 20
    got = _call(bvh, tris, a, b, num_triangles=2000)
    _same(got, exp, "2,000 of 3,200 triangles")
    assert got["flag"] == 2
    assert _call(bvh, tris, a, b, num_triangles=2000, flag=4)["flag"] == 6      # the flag word is never cleared
    none = _call(bvh, tris, a, b, num_triangles=0)
    assert none["flag"] == 2 and (none["i"] == 0).all() and np.isinf(none["d"]).all() and (none["k"] == 0).all()
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.segment_distances(bvh, tdev[:2000], cuda(a).t(), cuda(b).t())


def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, a, b, bf = _reference("torus40", abi.F32)
    n = len(a)
    f = getattr(lib.load(), NAME)
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        dt = NP_F[bvh.types.leaf_float]
        ad, bd = cuda(a.astype(dt)), cuda(b.astype(dt))
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(ad), api._ptr(bd), n, None, api._ptr(out), None, None, None, None,
               None, api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), what
        with pytest.raises(ValueError):
            ibvh.segment_distances(bvh, tdev, ad.t(), bd.t())
    bvh, tdev = _build(tris)
    A, B = cuda(a).t(), cuda(b).t()
    with pytest.raises(ValueError):
        ibvh.segment_distances(bvh, tdev.double(), A, B)          # triangles of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.segment_distances(bvh, bad, A, B)
    for bad in (A.cpu(), A.double(), A.t(), A[:2], A[:, :n - 1], A.reshape(-1), a):
        with pytest.raises(ValueError):
            ibvh.segment_distances(bvh, tdev, bad, B)
        with pytest.raises(ValueError):
            ibvh.segment_distances(bvh, tdev, A, bad)
    e = ibvh.segment_distances(bvh, tdev, A[:, :0], B[:, :0])
    assert e.index.shape == e.d2.shape == e.kind.shape == (0,) and e.point_segment.shape == e.point_mesh.shape == (0, 3)
    assert e.index.dtype == torch.int32 and e.d2.dtype == e.point_segment.dtype == torch.float32 and e.kind.dtype == torch.uint8
    far = ibvh.segment_distances(bvh, tdev, A + 100, B + 100, max_distance=1.0)          # far away: none within the radius
    assert (far.index == 0).all() and torch.isinf(far.d2).all() and (far.point_segment == 0).all() and (far.kind == 0).all()


def test_one_call_is_one_kernel_of_the_new_translation_unit():
    tris, a, b, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    A, B = cuda(a).t(), cuda(b).t()
    for kw in (dict(), dict(max_distance=0.5)):
        assert_one_kernel(lambda: ibvh.segment_distances(bvh, tdev, A, B, presorted=True, **kw), KERNEL, kw)
