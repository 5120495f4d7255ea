"""ibvh_sweep_spheres / sweep_spheres on the GPU: the first contact (index, the bits of t and of the point, the feature) and
the any mask are EQUAL to the brute force over all triangles of tests/sphere_sweep_checker.py — the definition of the result —
through the whole pipeline (volumes from triangles, build, one launch) for every accepted float / index combination, in the
given order and through the Morton-sorted default path, with scalar and tensor radii; per-sphere limits; hand-made meshes
straight through the C entry point (tiny trees, every built level, every output subset, the analytic square, d == 0, a
zero-area triangle, a NaN vertex, bad radii, the index guard); the axis-aligned floor on which the clamp is active; skin
margins and refit; the cross-check against sphere_contacts; the refusals, the empty batch and the one launch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

import ray_cast_checker as rcc  # noqa: E402
import sphere_sweep_checker as ssc  # noqa: E402
import mesh_query_kit as kit  # noqa: E402
from mesh_query_kit import FLOATS, MESHES, NP_F, NP_I, assert_one_kernel, build as _build, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

BITS = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}
NAME = "ibvh_sweep_spheres"


def _reference(mesh, flt):
    """(triangles, centres, displacements, radii, brute force of the unbounded spheres): the checker's shared, read-only case"""
    return ssc.reference(mesh, NP_F[flt])


def _dev(*arrays):
    return [cuda(np.array(a)) for a in arrays]       # (copies: the shared reference arrays are read-only)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype])


_assert_closest = functools.partial(kit.assert_closest, kit.SWEEP_SPHERES)   # index and feature, and t and the point BIT FOR BIT
_assert_any = functools.partial(kit.assert_any, kit.SWEEP_SPHERES)
_same = functools.partial(kit.first_hit_same, kit.SWEEP_SPHERES)


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_whole_pipeline_is_equal_to_the_checker(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, p, d, r, bf = _reference(mesh, leaf_flt)
    # the conditions that make the comparison mean something (tests/test_host_sphere_sweep.py pins them on the host too)
    nv = ssc.non_vacuity(bf, ssc.limited(bf, np.ones(800, dt), dt), d)
    print(f"{mesh} {floats}: {nv}")
    ssc.assert_non_vacuous(nv)
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    P, D, R = _dev(p, d, r)
    P, D = P.t(), D.t()
    got = ibvh.sweep_spheres(bvh, tdev, P, D, R, presorted=True)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.t.dtype == _tf(leaf_flt)
    assert got.index.shape == got.t.shape == got.hit.shape == got.feature.shape == (800,) and got.point.shape == (800, 3)
    assert got.hit.dtype == torch.bool and got.feature.dtype == torch.uint8
    _assert_closest(got, bf, (mesh, floats, idx, "given order"))
    _assert_closest(ibvh.sweep_spheres(bvh, tdev, P, D, R), bf, (mesh, floats, idx, "sorted"))
    _assert_closest(ibvh.sweep_spheres(bvh, tdev.reshape(-1, 3, 3), P, D, R), bf, (mesh, floats, idx, "(n, 3, 3)"))
    _assert_any(ibvh.sweep_spheres(bvh, tdev, P, D, R, any_hit=True, presorted=True), bf, (mesh, floats, idx, "any, given order"))
    _assert_any(ibvh.sweep_spheres(bvh, tdev, P, D, R, any_hit=True), bf, (mesh, floats, idx, "any, sorted"))


@functools.lru_cache(maxsize=None)
def _one_radius(flt):
    tris, p, d, r, _ = _reference("torus40", flt)
    radius = float(np.median(r))
    bf = ssc.brute_force(tris, p, d, np.full(800, radius, NP_F[flt]))
    for a in vars(bf).values():
        a.setflags(write=False)
    return radius, bf


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_one_number_is_every_spheres_radius(floats):
    leaf_flt, node_flt = FLOATS[floats]
    tris, p, d, r, _ = _reference("torus40", leaf_flt)
    radius, exp = _one_radius(leaf_flt)
    assert 200 <= (exp.index != 0).sum() <= 780 and ((exp.index != 0) & (exp.t > 0)).sum() >= 100
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    P, D = (x.t() for x in _dev(p, d))
    for presorted in (True, False):
        _assert_closest(ibvh.sweep_spheres(bvh, tdev, P, D, radius, presorted=presorted), exp, (floats, "a number", presorted))
        _assert_any(ibvh.sweep_spheres(bvh, tdev, P, D, radius, any_hit=True, presorted=presorted), exp, (floats, "a number, any"))
    _assert_closest(ibvh.sweep_spheres(bvh, tdev, P, D, torch.full((800,), radius, dtype=_tf(leaf_flt), device="cuda")), exp, (floats, "tensor"))


# ---- 2. the limit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_t_max_per_sphere(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, p, d, r, bf = _reference("torus40", leaf_flt)
    hit = bf.index != 0
    t1, t2 = bf.t, bf.second
    with np.errstate(invalid="ignore"):
        middle = ((t1.astype(np.float64) + t2.astype(np.float64)) / 2).astype(dt)
    later = np.isfinite(t2) & (middle < t2)          # (a second hit one step above the first leaves no room between them)
    assert later.sum() >= 200 and (hit & (t1 > 0)).sum() >= 300
    between = np.where(later, middle, t1)
    assert (between[later] < t2[later]).all() and (between >= t1)[hit].all()
    mixed = bf.t.copy()
    mixed[0::4], mixed[1::4], mixed[2::4] = np.nan, -1, 0
    limits = {"half": (bf.t * dt(0.5)).astype(dt), "exactly": bf.t.copy(), "between": between, "nan, negative, zero": mixed,
              "+Inf": np.full(800, np.inf, dt), "largest finite": np.full(800, np.finfo(dt).max, dt)}
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    P, D, R = _dev(p, d, r)
    P, D = P.t(), D.t()
    for what, lim in limits.items():
        exp = ssc.limited(bf, lim, dt)       # (tests/test_host_sphere_sweep.py pins limited() to the brute force under a limit)
        # what the checker itself says about these limits
        start = hit & (bf.t == 0)
        if what == "half":
            assert ((exp.index != 0) == start).all()                         # a hit at t1 > 0 lies beyond t1 / 2
        elif what in ("exactly", "between", "+Inf", "largest finite"):
            assert (exp.index == bf.index).all() and (_bits(exp.t) == _bits(bf.t)).all()   # inclusive; the first of two
        else:
            k = np.arange(800) % 4
            assert (exp.index[k < 2] == 0).all() and ((exp.index[k == 2] != 0) == start[k == 2]).all()
            assert (exp.index[k == 3] == bf.index[k == 3]).all() and hit[k < 2].sum() >= 250 and start[k == 2].sum() >= 20
        L = cuda(lim)
        for presorted in (True, False):
            got = ibvh.sweep_spheres(bvh, tdev, P, D, R, t_max=L, presorted=presorted)
            _assert_closest(got, exp, (floats, what, presorted))
            touched = ibvh.sweep_spheres(bvh, tdev, P, D, R, t_max=L, any_hit=True, presorted=presorted)
            _assert_any(touched, exp, (floats, what, presorted))
            assert torch.equal(touched, got.hit)                             # the two modes' masks agree under every limit
    # a number is every sphere's limit: 1 = the whole displacement
    exp = ssc.limited(bf, np.ones(800, dt), dt)
    assert 40 <= (exp.index == 0).sum() <= 750
    _assert_closest(ibvh.sweep_spheres(bvh, tdev, P, D, R, t_max=1), exp, (floats, "a number"))
    _assert_any(ibvh.sweep_spheres(bvh, tdev, P, D, R, t_max=1.0, any_hit=True), exp, (floats, "a number, any"))


# ---- 3. hand-made, straight through the C entry ------------------------------------------------------------------------
OUTS = "itqg"


def _call(bvh, tris, p, d, r, t_max=None, num_spheres=None, **kw):
    return kit.first_hit_call(kit.SWEEP_SPHERES, bvh, tris, (p, d, r), (t_max,), num=num_spheres, **kw)


Z = 0.3
SQUARE = [[0, 0, 2, 4, 0, 2, 4, 4, 2], [0, 0, 2, 4, 4, 2, 0, 4, 2]]                                # ssc.square's
FLOOR = [[-1.3, -1.1, Z, 1.7, -0.9, Z, 1.2, 1.4, Z], [-1.3, -1.1, Z, 1.2, 1.4, Z, -0.8, 1.3, Z]]   # ssc.floor_case's
HAND = SQUARE + FLOOR + [[5, 5, 5, 6, 6, 6, 7, 7, 7]]                                              # + zero area: collinear
nan, inf = np.nan, np.inf
HAND_SPHERES = [  # centre, displacement, radius
    ([2, 2, 5], [0, 0, -1], 1), ([1, 1, 5], [0, 0, -2], 0.5), ([3, 3, 0], [0, 0, 1], 0.25),       # onto the shared diagonal: equal t*
    ([1, 0.5, 4], [0, 0, -1], 0.5), ([0.5, 1, 4], [0, 0, -1], 0.5), ([1, 0.5, 1.5], [0, 0, -1], 0.25),   # either triangle, then the floor
    ([6, 2, 3], [-1, 0, -0.5], 0.5), ([-2, -3, 3], [1, 1, -0.5], 0.75), ([2, 6, 2], [0, -1, 0], 1),      # onto edges and corners, obliquely
    ([5, -1, 4], [-0.5, 0.5, -1], 0.3), ([-1, 5, 1], [0.7, -0.6, 0.4], 0.6), ([0.2, 0.1, 9], [0.01, 0.02, -1], 0.1),
    ([4, 8, 9], [1, -1, -1.5], 0.5), ([9, 9, 9], [-1, -1, -1], 0.75), ([5, 5, 9], [0.2, 0.2, -1], 1),   # the zero-area one: edges, ends
    ([1, 0.5, 2.2], [0, 0, 1], 0.25), ([1, 0.5, 2], [0.3, 0.1, 1], 0), ([1, 0.5, 3], [0, 0, -1], 0),     # touching at the start; radius 0
    ([1, 0.5, 3], [0, 0, -1], nan), ([1, 0.5, 3], [0, 0, -1], -1), ([1, 0.5, 3], [0, 0, -1], -inf), ([1, 0.5, 3], [0, 0, -1], inf),
    ([nan, 0.5, 3], [0, 0, -1], 0.5), ([1, nan, 3], [0, 0, -1], 0.5), ([1, 0.5, 3], [nan, 0, -1], 0.5), ([1, 0.5, 3], [0, 0, nan], 0.5),
    ([inf, 0.5, 3], [0, 0, -1], 0.5), ([1, 0.5, 3], [0, 0, -inf], 0.5), ([1, 0.5, 3], [1e-42, 0, -1], 0.5),
]
BAD_RADII = slice(18, 21)


def _hand(dt):
    """the analytic square's spheres (ssc.SQUARE_*), the hand-made ones and 16 of the floor's"""
    _, fp, fd, fr = ssc.floor_case(dt)
    p = np.concatenate([np.array(ssc.SQUARE_P, dt), np.array([s[0] for s in HAND_SPHERES], dt), fp[:16]])
    d = np.concatenate([np.array(ssc.SQUARE_D, dt), np.array([s[1] for s in HAND_SPHERES], dt), fd[:16]])
    with np.errstate(over="ignore"):
        r = np.concatenate([np.array(ssc.SQUARE_R, dt), np.array([s[2] for s in HAND_SPHERES], dt), fr[:16]])
    return np.ascontiguousarray(p), np.ascontiguousarray(d), np.ascontiguousarray(r)


SUBSETS = ["".join(k for j, k in enumerate(OUTS) if mask >> j & 1) for mask in range(1, 16)]


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (5, 1), (5, 2), (5, 3), (5, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris = np.array(HAND[:n], dt)
    p, d, r = _hand(dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4}[n] and bvh.built_level == built_level
    exp = ssc.brute_force(tris, p, d, r, idt=NP_I[idx])
    got = _call(bvh, tris, p, d, r)
    _same(got, exp, (n, built_level))
    assert got["flag"] == 0                                                       # a bad radius raises no bit, as in ibvh_sphere_contacts
    _same(_call(bvh, tris, p, d, r, mode=abi.SWEEP_ANY), exp, (n, built_level, "any"), outs="o")
    # what the checker itself says about these inputs
    a, h = len(ssc.SQUARE_P), len(ssc.SQUARE_P) + len(HAND_SPHERES)
    hand = exp.index[a:h]
    assert (hand[BAD_RADII] == 0).all() and (hand[22:28] == 0).all() and (exp.index[h:] != 0).sum() >= (16 if n >= 4 else 0)
    if n == 2:   # the analytic square: exact, d == 0 touching and not, the corner's tie
        assert exp.index[:a].tolist() == ssc.SQUARE_INDEX and exp.t[:a].tolist() == ssc.SQUARE_T and exp.feature[:a].tolist() == ssc.SQUARE_FEATURE
        assert exp.point[:a].tolist() == ssc.SQUARE_POINT and exp.tied[:a].tolist() == ssc.SQUARE_TIED
    if n >= 2:
        assert hand[:3].tolist() == [1, 1, 1] and exp.tied[a:a + 3].all()        # the shared diagonal: equal t*, the smaller index
        assert hand[15] == 1 and exp.t[a + 15] == 0 and hand[16] == 1 and exp.t[a + 16] == 0 and hand[17] == 1 and exp.t[a + 17] == 1
    if n == 5:
        assert (hand[12:15] == 5).all() and (exp.feature[a + 12:a + 15] != 6).all()   # zero area: no face, its edges and ends answer
        assert set(exp.feature[exp.index != 0].tolist()) >= {0, 2, 6} and len(set(exp.index.tolist())) == 6
    # every subset of the closest outputs; what was not asked for is not written
    for outs in SUBSETS:
        _same(_call(bvh, tris, p, d, r, outs=outs), exp, (n, built_level, outs), outs=outs)
    # a limit per sphere: the spheres' own t (inclusive), every third one halved
    lim = np.where(np.isfinite(exp.t), exp.t, dt(1)).astype(dt)
    lim[::3] *= dt(0.5)
    bounded = ssc.brute_force(tris, p, d, r, t_max=lim, idt=NP_I[idx])
    _same(_call(bvh, tris, p, d, r, t_max=lim), bounded, (n, built_level, "t_max"))
    _same(_call(bvh, tris, p, d, r, t_max=lim, mode=abi.SWEEP_ANY), bounded, (n, built_level, "t_max, any"), outs="o")
    assert (bounded.index != 0).sum() >= 8 and ((exp.index != 0) & (bounded.index == 0)).sum() >= 3
    # num_spheres = 0 with a pre-set flag: nothing is touched
    for mode in (abi.SWEEP_CLOSEST, abi.SWEEP_ANY):
        none = _call(bvh, tris, p, d, r, mode=mode, num_spheres=0, flag=4)
        assert none["status"] == 0 and none["flag"] == 4
        _same(none, exp, "empty", outs="")
    # a wrong combination of outputs: refused, nothing written
    for mode, outs in ((abi.SWEEP_CLOSEST, ""), (abi.SWEEP_CLOSEST, "ito"), (abi.SWEEP_CLOSEST, "o"), (abi.SWEEP_ANY, ""), (abi.SWEEP_ANY, "io"),
                       (abi.SWEEP_ANY, "go"), (abi.SWEEP_ANY, OUTS), (2, OUTS), (-1, "o")):
        bad = _call(bvh, tris, p, d, r, mode=mode, outs=outs)
        assert bad["status"] == abi.ERR_INVALID_ARG and bad["flag"] == 0, (mode, outs)
        _same(dict(bad, status=0), exp, (mode, outs), outs="")
    # num_triangles below the largest leaf index: those leaves are skipped, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        for mode, outs in ((abi.SWEEP_CLOSEST, OUTS), (abi.SWEEP_ANY, "o")):
            cut = _call(bvh, tris, p, d, r, mode=mode, num_triangles=n - 2, flag=4)
            assert cut["flag"] == 6
            _same(cut, ssc.brute_force(tris[:n - 2], p, d, r, idt=NP_I[idx]), "guard", outs=outs)


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (2, 2)])
def test_a_nan_vertex_in_a_tree_of_at_most_two_leaves(n, built_level, flt):
    """the triangle with the NaN vertex is never hit; the other one answers as if it were alone (a NaN leaf box may hide more
    in deeper trees: the header's caveat)"""
    dt = NP_F[flt]
    tris = np.array(SQUARE[:n], dt)
    tris[n - 1, 4] = nan
    p, d, r = _hand(dt)
    bvh, _ = _build(tris, flt, built_level=built_level)
    exp = ssc.brute_force(tris, p, d, r, idt=np.int32)
    assert (exp.index != n).all() and ((exp.index != 0).sum() >= 10 if n == 2 else (exp.index == 0).all())
    _same(_call(bvh, tris, p, d, r), exp, (n, built_level))
    _same(_call(bvh, tris, p, d, r, mode=abi.SWEEP_ANY), exp, (n, built_level, "any"), outs="o")


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("built_level", [1, 2])
def test_the_clamp_is_active_on_an_axis_aligned_floor(built_level, flt):
    """spheres coming straight down on a floor that lies flat in its boxes: the face candidate's t and the grown box's entry are
    two roundings of one time; the checker says on how many spheres the entry is the larger"""
    dt = NP_F[flt]
    tris, p, d, r = ssc.floor_case(dt)
    bvh, _ = _build(tris, flt, built_level=built_level)
    exp = ssc.brute_force(tris, p, d, r, idt=np.int32)
    print(f"floor {np.dtype(dt).name}: the clamp is active on {int(exp.clamped.sum())} of {len(p)} spheres")
    assert (exp.index != 0).all() and exp.clamped.sum() >= 10 and (~exp.clamped).sum() >= 10
    _same(_call(bvh, tris, p, d, r), exp, built_level)
    _same(_call(bvh, tris, p, d, r, mode=abi.SWEEP_ANY), exp, (built_level, "any"), outs="o")
    _same(_call(bvh, tris, p, d, r, t_max=exp.t), exp, (built_level, "t_max = t*"))
    # ... and a limit one step below t* loses exactly those hits
    below = np.nextafter(exp.t, dt(-np.inf))
    assert (_call(bvh, tris, p, d, r, t_max=below)["i"] == 0).all()


def test_two_roots_one_over_a_virtual_sibling_and_a_batch_of_a_wave_and_one():
    """built_level = 2 over 3 leaves: the walk starts from two roots, and the second root's other child is virtual; 65
    spheres are a full wave and one lane of a second workgroup"""
    tris = np.array(HAND[1:4], np.float32)
    p, d, r = _hand(np.float32)
    p, d, r = np.concatenate([p, p[:9]])[:65], np.concatenate([d, d[:9]])[:65], np.concatenate([r, r[:9]])[:65]
    bvh, _ = _build(tris, built_level=2)
    assert len(p) == 65 and (bvh.tree.levels, bvh.built_level, bvh.tree.real_leaves, bvh.tree.virtual_leaves) == (3, 2, 3, 1)
    exp = ssc.brute_force(tris, p, d, r, idt=np.int32)
    _same(_call(bvh, tris, p, d, r), exp)
    _same(_call(bvh, tris, p, d, r, mode=abi.SWEEP_ANY), exp, outs="o")
    assert set(exp.index.tolist()) == {0, 1, 2, 3} and exp.index[64] != 0      # ... every leaf, hence either root


# ---- 4. skin and refit -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _skin_and_refit(flt):
    dt = NP_F[flt]
    tris, p, d, r, bf = _reference("torus40", flt)
    lo, up = rcc.triangle_boxes(tris)
    s = dt(0.02)
    skin = ssc.brute_force(tris, p, d, r, boxes=((lo - s).astype(dt), (up + s).astype(dt)))
    rng = np.random.default_rng(11)
    verts, inverse = np.unique(tris.reshape(-1, 3), axis=0, return_inverse=True)
    shift = (0.01 * (rng.random(verts.shape) - 0.5)).astype(dt)
    moved = np.ascontiguousarray((verts + shift)[inverse.reshape(-1)].reshape(-1, 9).astype(dt))
    refit = ssc.brute_force(moved, p, d, r)
    for a in (moved,) + tuple(vars(skin).values()) + tuple(vars(refit).values()):
        a.setflags(write=False)
    return skin, moved, refit


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_keep_the_result_exact(floats):
    leaf_flt, node_flt = FLOATS[floats]
    tris, p, d, r, bf = _reference("torus40", leaf_flt)
    skin, moved, refit = _skin_and_refit(leaf_flt)
    P, D, R = _dev(p, d, r)
    P, D = P.t(), D.t()
    # the leaf box is the STORED volume, skin included: the definition is evaluated on it (a wider box can only lower a clamp)
    assert (skin.index == bf.index).all() and (skin.t <= bf.t).all() and (_bits(skin.t) != _bits(bf.t)).sum() <= bf.clamped.sum()
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    for presorted in (True, False):
        _assert_closest(ibvh.sweep_spheres(bvh, tdev, P, D, R, presorted=presorted), skin, (floats, "skin", presorted))
        _assert_any(ibvh.sweep_spheres(bvh, tdev, P, D, R, any_hit=True, presorted=presorted), skin, (floats, "skin, any", presorted))
    # refit the tight build to moved vertices: the moved triangles' brute force
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    mdev = cuda(np.array(moved))
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    assert (_bits(refit.t) != _bits(bf.t)).sum() >= 300 and (refit.index != 0).sum() >= 400
    for presorted in (True, False):
        _assert_closest(ibvh.sweep_spheres(bvh, mdev, P, D, R, presorted=presorted), refit, (floats, "refit", presorted))
        _assert_any(ibvh.sweep_spheres(bvh, mdev, P, D, R, any_hit=True, presorted=presorted), refit, (floats, "refit, any", presorted))


# ---- 5. the contact list -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_touching_at_the_start_agrees_with_sphere_contacts(mesh, flt):
    """hit_t == 0 iff the sphere's contact list is not empty, and the triangle named is the list's smallest index, with the
    list's point and feature for it"""
    tris, p, d, r, bf = _reference(mesh, flt)
    bvh, tdev = _build(tris, flt)
    P, D, R = _dev(p, d, r)
    got = ibvh.sweep_spheres(bvh, tdev, P.t(), D.t(), R)
    contacts = ibvh.sphere_contacts(bvh, tdev, P.t(), R)
    touching = contacts.counts > 0
    assert torch.equal(got.t == 0, touching) and 80 <= int(touching.sum()) <= 720
    owner, index = (contacts.sphere - 1).cpu().numpy(), contacts.index.cpu().numpy().astype(np.int64)
    first = np.full(800, np.iinfo(np.int64).max)
    np.minimum.at(first, owner, index)
    t = touching.cpu().numpy()
    assert (got.index.cpu().numpy()[t] == first[t]).all()
    row = np.flatnonzero(index == first[owner])
    assert len(row) == t.sum() and (owner[row] == np.flatnonzero(t)).all()
    assert torch.equal(got.point[touching], contacts.point[torch.from_numpy(row).cuda()])
    assert torch.equal(got.feature[touching], contacts.region[torch.from_numpy(row).cuda()])


# ---- 6. refusals, the empty batch, one launch --------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, p, d, r, bf = _reference("torus40", abi.F32)
    P, D, R = _dev(p, d, r)
    P, D = P.t(), D.t()
    f = getattr(lib.load(), NAME)
    out = torch.full((800,), -7, dtype=torch.int32, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        ft = NP_F[bvh.types.leaf_float]
        c, dis, rad = _dev(p.astype(ft), d.astype(ft), r.astype(ft))
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(c), api._ptr(dis), api._ptr(rad), 800, None, abi.SWEEP_CLOSEST,
               api._ptr(out), None, None, None, None, None, api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), what
        for any_hit in (False, True):
            with pytest.raises(ValueError):
                ibvh.sweep_spheres(bvh, tdev, c.t(), dis.t(), rad, any_hit=any_hit)
    bvh, tdev = _build(tris)
    with pytest.raises(ValueError):
        ibvh.sweep_spheres(bvh, tdev.double(), P, D, R)          # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.sweep_spheres(bvh, tdev, P.double(), D, R)          # centres of the other dtype
    with pytest.raises(ValueError):
        ibvh.sweep_spheres(bvh, tdev, P, D.double(), R)          # displacements of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.sweep_spheres(bvh, bad, P, D, R)
    for bad in (P.cpu(), P.t(), P[:2], P.reshape(-1), p):
        with pytest.raises(ValueError):
            ibvh.sweep_spheres(bvh, tdev, bad, D, R)
    for bad in (D.cpu(), D.t(), D[:2], D[:, :799], D.reshape(-1), d):
        with pytest.raises(ValueError):
            ibvh.sweep_spheres(bvh, tdev, P, bad, R)
    L = torch.ones(800, device="cuda")
    for bad in (L.cpu(), L.double(), L[:799], L.reshape(1, 800), "far", True, [1.0] * 800):
        with pytest.raises(ValueError, match="t_max"):
            ibvh.sweep_spheres(bvh, tdev, P, D, R, t_max=bad)
        with pytest.raises(ValueError, match="radii"):
            ibvh.sweep_spheres(bvh, tdev, P, D, bad)
    with pytest.raises(ValueError, match="radii"):
        ibvh.sweep_spheres(bvh, tdev, P, D, None)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.sweep_spheres(bvh, tdev[:10], P, D, R)              # flag bit 1
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.sweep_spheres(bvh, tdev[:10], P, D, R, any_hit=True)
    e = ibvh.sweep_spheres(bvh, tdev, P[:, :0], D[:, :0], R[:0])
    assert e.index.shape == e.t.shape == e.hit.shape == e.feature.shape == (0,) and e.point.shape == (0, 3)
    assert e.index.dtype == torch.int32 and e.t.dtype == e.point.dtype == torch.float32 and e.hit.dtype == torch.bool and e.feature.dtype == torch.uint8
    o = ibvh.sweep_spheres(bvh, tdev, P[:, :0], D[:, :0], 0.5, any_hit=True, t_max=L[:0])
    assert o.shape == (0,) and o.dtype == torch.bool


def test_one_call_is_one_kernel_of_the_new_translation_unit():
    tris, p, d, r, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    P, D, R = _dev(p, d, r)
    P, D = P.t(), D.t()
    L = torch.ones(800, device="cuda")
    for kw in (dict(), dict(any_hit=True), dict(t_max=L)):
        assert_one_kernel(lambda: ibvh.sweep_spheres(bvh, tdev, P, D, R, presorted=True, **kw), "sweep_walk_kernel", kw)
