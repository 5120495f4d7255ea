"""ibvh_sphere_contacts / sphere_contacts on the GPU: counts, offsets, index, squared distance, closest point, region and the
ORDER of every sphere's list are BIT-EQUAL to the brute force over all triangles of tests/sphere_contacts_checker.py — the
definition of the result — through the whole pipeline (volumes from triangles, build, count, scan, write) for every accepted
float / index combination, in the given order, through the Morton-sorted default path and counting only; hand-made meshes
straight through the C entry point (tiny trees, all seven regions, degenerate triangles, NaN and Inf centres and radii, output
subsets, the index guard), offsets in a permuted order and the capacity guard, skin margins and refit, a duplicated triangle,
the refusals, and one kernel per pass."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import mesh_query_kit as kit  # noqa: E402
import sphere_contacts_checker as scc  # noqa: E402
from mesh_query_kit import FLOATS, MESHES, NP_F, NP_I, bits as _bits, build as _build, leaf_order as _leaf_order, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

NAME = "ibvh_sphere_contacts"


@functools.lru_cache(maxsize=None)
def _reference(mesh, flt):
    """(triangles, centres, radii, brute force in the order 1..n) of a mesh in a dtype: computed once, shared, never modified"""
    tris = torus_mesh(*MESHES[mesh]).astype(NP_F[flt])
    c, radii = scc.pipeline_spheres(tris, NP_F[flt])
    bf = scc.brute_force(tris, c, radii, idt=np.int64)
    for a in (tris, bf.counts, bf.offsets, bf.sphere, bf.index, bf.d2, bf.point, bf.region):
        a.setflags(write=False)   # (c and radii go through torch.from_numpy, which wants a writable array)
    return tris, c, radii, bf


_assert_equal = functools.partial(kit.assert_equal, scc.QUERY)
_same = functools.partial(kit.same, scc.QUERY)
SENTINEL = {k: col.sentinel for k, col in scc.QUERY.columns.items()}


def _call(bvh, tris, c, r, **kw):
    """count, scan on the host, write -> dict: counts, the outputs, both flag words and both statuses (kit.two_passes)"""
    return kit.two_passes(scc.QUERY, bvh, tris, (c, r), **kw)


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_whole_pipeline_is_bit_equal_to_the_brute_force(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, c, radii, bf = _reference(mesh, leaf_flt)
    # the conditions that make the comparison mean something (tests/test_host_sphere_contacts.py pins them on the host too)
    nv = scc.non_vacuity(bf, radii)
    print(f"{mesh} {floats}: {nv}")
    scc.assert_non_vacuous(nv)
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    order = _leaf_order(bvh)
    assert sorted(order.tolist()) == list(range(1, len(tris) + 1)) and (np.diff(order) < 0).any()
    exp = scc.in_leaf_order(bf, order)
    assert (exp.index != bf.index).any()   # the leaf order is not the triangles' own: the order is being tested
    P, R = cuda(c).t(), cuda(radii)
    got = ibvh.sphere_contacts(bvh, tdev, P, R, presorted=True)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.distance2.dtype == _tf(leaf_flt)
    _assert_equal(got, exp, (mesh, floats, idx, "given order"))
    _assert_equal(ibvh.sphere_contacts(bvh, tdev, P, R), exp, (mesh, floats, idx, "sorted"))
    _assert_equal(ibvh.sphere_contacts(bvh, tdev.reshape(-1, 3, 3), P, R, count_only=True), exp, (mesh, floats, idx, "count"), count_only=True)
    _assert_equal(ibvh.sphere_contacts(bvh, tdev, P, R, count_only=True, presorted=True), exp, (mesh, floats, idx, "count, given"), count_only=True)


def test_a_scalar_radius_is_a_radius_search_around_points():
    tris, c, radii, _ = _reference("torus40", abi.F32)
    r = np.float32(2.5 * scc.mean_edge(tris))
    bvh, tdev = _build(tris)
    exp = scc.brute_force(tris, c, np.full(len(c), r, np.float32), leaf_order=_leaf_order(bvh), idt=np.int64)
    assert (exp.counts == 0).sum() >= 100 and (exp.counts >= 2).sum() >= 100
    for radius in (float(r), r):
        _assert_equal(ibvh.sphere_contacts(bvh, tdev, cuda(c).t(), radius), exp, "scalar")


# ---- 2. hand-made, straight through the C entry ------------------------------------------------------------------------
UNIT = [0, 0, 0, 1, 0, 0, 0, 1, 0]
HAND = [UNIT,
        [5, 5, 5, 6, 6, 6, 7, 7, 7],             # zero area: collinear
        [9, 9, 9, 9, 9, 9, 9, 9, 9],             # zero area: one point
        [3, 0, 0, 4, 0, 0, 3, 1, 0],
        [0, 0, 3, 1, 0, 3, 0, 1, 3]]
REGION_POINTS = [[-1, -1, 1], [2, -0.5, 1], [0.5, -1, 1], [-0.5, 2, 1], [-1, 0.5, 1], [1, 1, 1], [0.25, 0.25, 1]]
HAND_POINTS = REGION_POINTS + [[5.5, 5.5, 5.5], [6.5, 6, 7], [9, 9, 10], [8, 8, 8], [np.nan, 0, 0], [0, np.inf, 0], [3.2, 0.2, -1], [0.2, 0.2, 2.9]]
# the unit triangle's d2 to the seven region points is 3, 2.25, 2, 2.25, 2, 1.5, 1: each radius reaches it, the last exactly
HAND_RADII = [1.8, 1.6, 1.5, 1.6, 1.5, 1.3, 1.0, 0, 1.2, 1, 7, 1, 1, 1.1, 0.05]
# ... and the centres and radii that touch nothing, or everything
EXTRA_POINTS = [[0.25, 0.25, 1]] * 5 + [[np.nan, 0.25, 1], [0.25, np.nan, 1], [0.25, 0.25, np.nan], [0, np.inf, 0], [0.25, 0.25, 0], [0.25, 0.25, 1], [2, 2, 2]]
EXTRA_RADII = [-1, np.nan, np.inf, -0.0, -np.inf, np.inf, 1, 1, np.inf, 0, 2.3, 20]


def _hand(n, dt):
    return np.array(HAND[:n], dt), np.array(HAND_POINTS + EXTRA_POINTS, dt), np.array(HAND_RADII + EXTRA_RADII, dt)


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (3, 1), (5, 1), (5, 2), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris, c, r = _hand(n, dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4}[n] and bvh.built_level == built_level
    order = _leaf_order(bvh)
    exp = scc.brute_force(tris, c, r, leaf_order=order, idt=NP_I[idx])
    got = _call(bvh, tris, c, r)
    _same(got, exp, (n, built_level))
    assert got["flag_count"] == 0 and got["flag"] == 0
    # what the checker itself says about these inputs: the seven regions of triangle 1; NaN centres, negative and NaN radii
    # touch nothing; -0.0 is a radius of zero; +Inf reaches every triangle, and a d2 of +Inf is within it (a NaN d2 is not)
    first = exp.index == 1
    assert exp.region[first & (exp.sphere < 7)].tolist() == [0, 1, 2, 3, 4, 5, 6] and exp.sphere[first & (exp.sphere < 7)].tolist() == list(range(7))
    assert exp.d2[first & (exp.sphere == 6)] == exp.r2[6] == 1
    e0 = len(HAND_POINTS)
    assert exp.counts[11] == 0 and exp.counts[[e0, e0 + 1, e0 + 3, e0 + 4, e0 + 5, e0 + 6, e0 + 7]].tolist() == [0] * 7
    assert exp.counts[e0 + 2] == n and exp.counts[e0 + 8] == (n >= 2) and np.isposinf(exp.d2[exp.sphere == e0 + 8]).all()
    assert exp.counts[e0 + 9] == 1 and exp.d2[exp.sphere == e0 + 9] == 0 and exp.counts[e0 + 11] == n
    if n == 5:
        assert {0, 1, 2, 5} <= set(exp.counts.tolist()) and exp.counts[10] == 2 and exp.counts[7] == 1
        assert (exp.index[exp.sphere == e0 + 11] == order).all() and (np.diff(order) < 0).any()
    # any subset of the outputs; what was not asked for is not written
    subsets = ["".join(x) for k in range(1, 5) for x in itertools.combinations("idqg", k)]
    assert len(subsets) == 15
    for outs in subsets:
        _same(_call(bvh, tris, c, r, outs=outs), exp, outs, outs=outs)
    # num_spheres = 0 with a pre-set flag: nothing is touched
    none = _call(bvh, tris, c, r, num=0, flag=4, rows=3)
    assert none["status_count"] == 0 and none["status"] == 0 and none["flag_count"] == 4 and none["flag"] == 4
    assert (none["counts"] == -7).all() and all((none[k] == SENTINEL[k]).all() for k in "idqg")
    # num_triangles below the largest leaf index: those leaves are skipped in both passes, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        cut = _call(bvh, tris, c, r, num_triangles=n - 2, flag=4)
        assert cut["flag_count"] == 6 and cut["flag"] == 6
        cut_exp = scc.brute_force(tris[:n - 2], c, r, leaf_order=order, idt=NP_I[idx])
        assert len(cut_exp.index) < len(exp.index)
        _same(cut, cut_exp, "guard")


def test_two_roots_one_over_a_virtual_sibling_and_a_batch_of_a_wave_and_one():
    """built_level = 2 over 3 leaves: the walk starts from two roots, and the second root's other child is virtual; 65
    spheres are a full wave and one lane of a second workgroup"""
    tris = np.array(HAND[:3], np.float32)
    rng = np.random.default_rng(65)
    c = np.concatenate([np.array(HAND_POINTS[:11], np.float32), (rng.random((54, 3)) * 12 - 1).astype(np.float32)])
    r = np.concatenate([np.array(HAND_RADII[:11], np.float32), (rng.random(54) * 16).astype(np.float32)])
    bvh, _ = _build(tris, built_level=2)
    assert len(c) == 65 and (bvh.tree.levels, bvh.built_level, bvh.tree.real_leaves, bvh.tree.virtual_leaves) == (3, 2, 3, 1)
    exp = scc.brute_force(tris, c, r, leaf_order=_leaf_order(bvh), idt=np.int32)
    assert set(exp.index.tolist()) == {1, 2, 3} and exp.counts[64] > 0 and {0, 1, 2, 3} == set(exp.counts.tolist())
    _same(_call(bvh, tris, c, r), exp)


# ---- 3. offsets and capacity -------------------------------------------------------------------------------------------
def test_offsets_in_a_permuted_order_and_the_capacity_guard():
    tris, c, radii, bf = _reference("torus40", abi.F32)
    c, radii = c[:200], radii[:200]
    bvh, _ = _build(tris)
    exp = scc.brute_force(tris, c, radii, leaf_order=_leaf_order(bvh), idt=np.int32)
    total = len(exp.index)
    assert total > 1000 and (exp.counts > 0).sum() > 50
    kit.check_offsets_and_capacity(scc.QUERY, functools.partial(_call, bvh, tris, c, radii), exp)


# ---- 4. NaN, skin, refit, duplicates -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["nan_second", "nan_first"])
def test_a_triangle_with_a_nan_vertex_is_never_a_contact_and_hides_none(order, flt):
    dt = NP_F[flt]
    both = np.array([UNIT, [0, 0, 0.5, np.nan, 0, 0.5, 0, 1, 0.5]], dt)[list(order)]
    c = np.array(REGION_POINTS + [[0.2, 0.2, 0.5], [np.nan, np.nan, np.nan], [0.2, 0.2, 0.5]], dt)
    r = np.array(HAND_RADII[:7] + [1, 1, np.inf], dt)
    bvh, _ = _build(both, flt)
    exp = scc.brute_force(both, c, r, leaf_order=_leaf_order(bvh), idt=np.int32)
    good = order.index(0) + 1
    assert (exp.index == good).all() and exp.counts.tolist() == [1] * 8 + [0, 1]
    got = _call(bvh, both, c, r)
    _same(got, exp, order)
    assert not np.isnan(got["d"]).any() and not np.isnan(got["q"]).any()


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_keep_the_result_exact(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, c, radii, bf = _reference("torus40", leaf_flt)
    P, R = cuda(c).t(), cuda(radii)
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    _assert_equal(ibvh.sphere_contacts(bvh, tdev, P, R), scc.in_leaf_order(bf, _leaf_order(bvh)), (floats, "skin"))
    # refit the tight build to moved vertices: the moved triangles' brute force
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    moved = (tris + 0.01 * (rng.random(tris.shape) - 0.5)).astype(dt)
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = scc.brute_force(moved, c, radii, leaf_order=_leaf_order(bvh), idt=np.int64)
    assert (exp.counts != bf.counts).any() and len(exp.index) > 10000
    for presorted in (True, False):
        _assert_equal(ibvh.sphere_contacts(bvh, mdev, P, R, presorted=presorted), exp, (floats, "refit", presorted))


def test_a_duplicated_triangle_appears_twice_at_both_leaf_positions():
    base, _, _, _ = _reference("torus40", abi.F32)
    k = 1234
    tris = np.concatenate([base, base[k - 1:k]])
    n = len(base)
    rng = np.random.default_rng(3)
    w = rng.dirichlet((4.0, 4.0, 4.0), 64)            # well inside the triangle
    t64 = tris[k - 1].reshape(3, 3).astype(np.float64)
    normal = np.cross(t64[1] - t64[0], t64[2] - t64[0])
    c = ((w[:, :, None] * t64[None]).sum(1) + 1e-3 * normal / np.linalg.norm(normal)).astype(np.float32)
    r = np.full(64, 2 * scc.mean_edge(base), np.float32)
    bvh, tdev = _build(tris)
    order = _leaf_order(bvh)
    exp = scc.brute_force(tris, c, r, leaf_order=order, idt=np.int32)
    pos = {int(i): int(np.flatnonzero(order == i)[0]) for i in (k, n + 1)}
    for s in range(64):
        mine = exp.index[exp.offsets[s]:exp.offsets[s + 1]].tolist()
        assert mine.count(k) == 1 and mine.count(n + 1) == 1 and (mine.index(k) < mine.index(n + 1)) == (pos[k] < pos[n + 1])
    a, b = exp.index == k, exp.index == n + 1
    assert _bits(exp.d2[a]) == _bits(exp.d2[b]) and (exp.region[a] == 6).all()
    for presorted in (True, False):
        _assert_equal(ibvh.sphere_contacts(bvh, tdev, cuda(c).t(), cuda(r), presorted=presorted), exp, presorted)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, c, radii, bf = _reference("torus40", abi.F32)
    P, R = cuda(c).t(), cuda(radii)
    f = getattr(lib.load(), NAME)
    out = torch.full((800,), -7, dtype=torch.int64, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        dt = NP_F[bvh.types.leaf_float]
        cd, rd = cuda(c.astype(dt)), cuda(radii.astype(dt))
        for mode, counts, offsets, index in ((abi.SPHERES_COUNT, api._ptr(out), None, None), (abi.SPHERES_WRITE, None, api._ptr(out), api._ptr(out))):
            st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(cd), api._ptr(rd), 800, mode, counts, offsets, 800, index,
                   None, None, None, None, api._stream())
            torch.cuda.synchronize()
            assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), (what, mode)
        with pytest.raises(ValueError):
            ibvh.sphere_contacts(bvh, tdev, cd.t(), rd)
    bvh, tdev = _build(tris)
    with pytest.raises(ValueError):
        ibvh.sphere_contacts(bvh, tdev.double(), P, R)          # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.sphere_contacts(bvh, tdev, P.double(), R)          # centres of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.sphere_contacts(bvh, bad, P, R)
    for bad in (P.cpu(), P.t(), P[:2], P.reshape(-1), c):
        with pytest.raises(ValueError):
            ibvh.sphere_contacts(bvh, tdev, bad, R)
    for bad in (R.cpu(), R.double(), R[:799], R.reshape(-1, 1), R.reshape(1, -1), radii, None, "1", True, [0.1] * 800):
        with pytest.raises(ValueError):
            ibvh.sphere_contacts(bvh, tdev, P, bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.sphere_contacts(bvh, tdev[:10], P, R)              # flag bit 1
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.sphere_contacts(bvh, tdev[:10], P, R, count_only=True)
    e = ibvh.sphere_contacts(bvh, tdev, P[:, :0], R[:0])
    assert e.offsets.tolist() == [0] and e.counts.shape == (0,) and e.index.shape == (0,) and e.index.dtype == torch.int32
    assert e.distance2.shape == (0,) and e.point.shape == (0, 3) and e.region.shape == (0,) and e.sphere.shape == (0,)
    far = ibvh.sphere_contacts(bvh, tdev, P + 100, R)           # no contact at all: no write pass, empty outputs
    assert far.offsets.tolist() == [0] * 801 and far.index.shape == (0,) and far.point.shape == (0, 3) and far.sphere.shape == (0,)


# ---- 6. one kernel per pass --------------------------------------------------------------------------------------------
def test_each_pass_is_one_kernel_of_the_new_translation_unit():
    tris, c, radii, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    P, R = cuda(c).t(), cuda(radii)
    # the write pass goes straight through the C entry, and writes index and region alone
    kit.check_each_pass_is_one_kernel(scc.QUERY, bvh, tdev, functools.partial(ibvh.sphere_contacts, bvh, tdev, P, R, presorted=True),
                                      (P.t().contiguous(), R), (), "ig")
