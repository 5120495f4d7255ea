"""ibvh_cast_rays / cast_rays on the GPU: the closest hit (index, the bits of t, the bits of u and v) and the any-hit mask are
EQUAL to the brute force over all triangles of tests/ray_cast_checker.py — the definition of the result — through the whole
pipeline (volumes from triangles, build, one launch) for every accepted float / index combination, in the given order and
through the Morton-sorted default path; per-ray limits; hand-made meshes straight through the C entry point (tiny trees, every
built level, the axis-aligned floor on which the clamp is active, a shared edge with equal t*, rays in a triangle's plane,
zero-area triangles, NaN and Inf, the zero direction, an origin on a box face, output subsets, the index guard); skin margins
and refit; the existing raycast() path on the rays it is comparable on; the refusals, the empty batch and the one launch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import ray_cast_checker as rcc  # noqa: E402
import mesh_query_kit as kit  # noqa: E402
from mesh_query_kit import FLOATS, MESHES, NP_F, NP_I, assert_one_kernel, build as _build, tf as _tf  # noqa: E402
from test_gpu_parity import cuda  # noqa: E402

BITS = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}
NAME = "ibvh_cast_rays"


@functools.lru_cache(maxsize=None)
def _reference(mesh, flt):
    """(triangles, origins, directions, brute force of the unbounded rays) of a mesh in a dtype: computed once, shared, never
    modified"""
    tris = torus_mesh(*MESHES[mesh]).astype(NP_F[flt])
    p, d = rcc.rays(tris, NP_F[flt])
    bf = rcc.brute_force(tris, p, d)
    for a in (tris, bf.index, bf.t, bf.uv, bf.occluded, bf.clamped, bf.tied):  # (p, d go through torch.from_numpy: writable)
        a.setflags(write=False)
    return tris, p, d, bf


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype])


_assert_closest = functools.partial(kit.assert_closest, kit.CAST_RAYS)   # index, and t, u, v BIT FOR BIT
_assert_any = functools.partial(kit.assert_any, kit.CAST_RAYS)
_same = functools.partial(kit.first_hit_same, kit.CAST_RAYS)


# ---- 1. brute force, whole pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_whole_pipeline_is_equal_to_the_checker(mesh, floats, idx):
    leaf_flt, node_flt = FLOATS[floats]
    tris, p, d, bf = _reference(mesh, leaf_flt)
    # the conditions that make the comparison mean something (tests/test_host_ray_cast.py pins them on the host too)
    print(f"{mesh} {floats}: (hit, miss, two or more exact hits, exact hits, zero-component hits, clamped, tied) = {rcc.non_vacuity(bf, d)}")
    rcc.assert_non_vacuous(bf, d)
    bvh, tdev = _build(tris, leaf_flt, node_flt, idx)
    assert bvh.tree.virtual_leaves > 0
    P, D = cuda(p).t(), cuda(d).t()
    got = ibvh.cast_rays(bvh, tdev, P, D, presorted=True)
    assert isinstance(got, ibvh.RayCast)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.t.dtype == _tf(leaf_flt)
    assert got.index.shape == got.t.shape == got.hit.shape == (800,) and got.uv.shape == (800, 2) and got.hit.dtype == torch.bool
    _assert_closest(got, bf, (mesh, floats, idx, "given order"))
    _assert_closest(ibvh.cast_rays(bvh, tdev, P, D), bf, (mesh, floats, idx, "sorted"))
    _assert_closest(ibvh.cast_rays(bvh, tdev.reshape(-1, 3, 3), P, D), bf, (mesh, floats, idx, "(n, 3, 3)"))
    _assert_any(ibvh.cast_rays(bvh, tdev, P, D, any_hit=True, presorted=True), bf, (mesh, floats, idx, "any, given order"))
    _assert_any(ibvh.cast_rays(bvh, tdev, P, D, any_hit=True), bf, (mesh, floats, idx, "any, sorted"))


# ---- 2. the limit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_t_max_per_ray(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, p, d, bf = _reference("torus40", leaf_flt)
    t1, t2 = rcc.second_hit(tris, p, d)
    hit = bf.index != 0
    assert (_bits(t1) == _bits(bf.t)).all() and (t1[hit] > 0).all() and (np.isfinite(t2) & (t2 > t1)).sum() >= 400
    two = np.isfinite(t2)
    between = np.where(two, (t1.astype(np.float64) + t2.astype(np.float64)) / 2, t1).astype(dt)
    assert (between[two & (t2 > t1)] < t2[two & (t2 > t1)]).all() and (between >= t1)[hit].all()
    mixed = bf.t.copy()
    mixed[0::4], mixed[1::4], mixed[2::4] = np.nan, -1, 0
    limits = {"half": (bf.t * dt(0.5)).astype(dt), "exactly": bf.t.copy(), "between": between, "nan, negative, zero": mixed,
              "+Inf": np.full(800, np.inf, dt), "largest finite": np.full(800, np.finfo(dt).max, dt)}
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    P, D = cuda(p).t(), cuda(d).t()
    for what, lim in limits.items():
        exp = rcc.brute_force(tris, p, d, t_max=lim)
        # what the checker itself says about these limits
        if what == "half":
            assert (exp.index == 0).all()                                   # a hit at t1 > 0 lies beyond t1 / 2
        elif what in ("exactly", "between", "+Inf", "largest finite"):
            assert (exp.index == bf.index).all() and (_bits(exp.t) == _bits(bf.t)).all()   # inclusive; the first of two
        else:
            k = np.arange(800) % 4
            assert (exp.index[k < 3] == 0).all() and (exp.index[k == 3] == bf.index[k == 3]).all() and hit[k < 3].sum() >= 500
        L = cuda(lim)
        for presorted in (True, False):
            got = ibvh.cast_rays(bvh, tdev, P, D, t_max=L, presorted=presorted)
            _assert_closest(got, exp, (floats, what, presorted))
            occ = ibvh.cast_rays(bvh, tdev, P, D, t_max=L, any_hit=True, presorted=presorted)
            _assert_any(occ, exp, (floats, what, presorted))
            assert torch.equal(occ, got.hit)                                # the two modes' masks agree under every limit
    # a number is every ray's limit
    exp = rcc.brute_force(tris, p, d, t_max=np.full(800, 0.75, dt))
    assert 50 <= (exp.index != 0).sum() <= 750
    _assert_closest(ibvh.cast_rays(bvh, tdev, P, D, t_max=0.75), exp, (floats, "a number"))
    _assert_any(ibvh.cast_rays(bvh, tdev, P, D, t_max=0.75, any_hit=True), exp, (floats, "a number, any"))


# ---- 3. hand-made, straight through the C entry ------------------------------------------------------------------------
def _call(bvh, tris, p, d, t_max=None, num_rays=None, **kw):
    return kit.first_hit_call(kit.CAST_RAYS, bvh, tris, (p, d), (t_max,), num=num_rays, **kw)


Z = 0.3
FLOOR = [[-1.3, -1.1, Z, 1.7, -0.9, Z, 1.2, 1.4, Z], [-1.3, -1.1, Z, 1.2, 1.4, Z, -0.8, 1.3, Z]]   # rcc.floor_case's
SQUARE = [[0, 0, 2, 4, 0, 2, 4, 4, 2], [0, 0, 2, 4, 4, 2, 0, 4, 2]]                                # z = 2: coplanar, the diagonal shared
HAND = FLOOR + SQUARE + [[5, 5, 5, 6, 6, 6, 7, 7, 7], [9, 9, 9, 9, 9, 9, 9, 9, 9]]                 # + zero area: collinear, one point
nan, inf = np.nan, np.inf
HAND_RAYS = [  # origin, direction
    ([2, 2, 3], [0, 0, -1]), ([1, 1, 5], [0, 0, -2]), ([3, 3, 0], [0, 0, 1]),        # the shared diagonal: equal t*, the smaller index
    ([1, 0.5, 3], [0, 0, -1]), ([0.5, 1, 3], [0, 0, -1]),                            # either triangle of the square, then the floor
    ([1, 0.5, 1], [0, 0, -1]), ([1, 0.5, 1], [0, 0, 1]), ([1, 0.5, 0], [0, 0, -1]),  # between the two; below both, looking away
    ([-1, 1, 2], [1, 0, 0]), ([-1, 1, 2], [1, 0.5, 0]), ([-1, 0, Z], [1, 0.1, 0]),   # in a triangle's plane
    ([0, 1, 0], [0, 0, 1]), ([4, 1, 5], [0, 0, -1]), ([1, 0, 0], [0, 0, 1]),         # an origin on a box face, a zero component along it
    ([1, 4, 9], [0, 0, -1]), ([0, 0, 0], [0, 0, 1]), ([4, 4, 0], [0, 0, 1]),         # ... and on box edges and corners
    ([1, 0.5, 3], [0, 0, 0]), ([1, 0.5, 2], [0, 0, 0]),                              # the zero direction, off and on a triangle
    ([nan, 0.5, 3], [0, 0, -1]), ([1, nan, 3], [0, 0, -1]), ([1, 0.5, nan], [0, 0, -1]),
    ([1, 0.5, 3], [nan, 0, -1]), ([1, 0.5, 3], [0, nan, -1]), ([1, 0.5, 3], [0, 0, nan]),
    ([inf, 0.5, 3], [0, 0, -1]), ([1, 0.5, inf], [0, 0, -1]), ([1, 0.5, -inf], [0, 0, 1]), ([-inf, 0.5, 2], [1, 0, 0]),
    ([1, 0.5, 3], [0, 0, -inf]), ([1, 0.5, 3], [inf, 0, -1]), ([1, 0.5, 3], [1e-42, 0, -1]), ([0, 0.5, 3], [1e-42, 0, -1]),
    ([5.5, 5.5, 0], [0, 0, 1]), ([6, 6, 0], [0, 0, 1]), ([4, 5, 6], [1, 1, 0]), ([9, 9, 0], [0, 0, 1]), ([8, 8, 8], [1, 1, 1]),   # zero area
    ([1, 0.5, 2], [0, 0, -1]), ([1, 0.5, 2], [0.1, 0.2, 1]), ([1, 0.5, Z], [0.3, 0.1, -1]),                                        # cast from a surface
    ([-2, -2, 4], [1.1, 0.9, -1.3]), ([5, 5, 4], [-1.4, -1.6, -1.2]), ([3, -3, -2], [-0.9, 1.2, 0.8]), ([0.2, 0.1, 9], [0.01, 0.02, -1]),
]


def _hand(dt):
    """the hand-made rays and 24 of the floor's (the clamp is active on some of them)"""
    _, fp, fd = rcc.floor_case(dt)
    p = np.concatenate([np.array([r[0] for r in HAND_RAYS], dt), fp[:24]])
    d = np.concatenate([np.array([r[1] for r in HAND_RAYS], dt), fd[:24]])
    return np.ascontiguousarray(p), np.ascontiguousarray(d)


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,built_level", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (5, 1), (5, 2), (5, 3), (5, 4), (6, 1), (6, 2), (6, 3),
                                           (6, 4)])
def test_hand_made_meshes_through_the_c_entry(n, built_level, flt, idx):
    dt = NP_F[flt]
    tris = np.array(HAND[:n], dt)
    p, d = _hand(dt)
    bvh, _ = _build(tris, flt, idx=idx, built_level=built_level)
    assert bvh.tree.levels == {1: 1, 2: 2, 3: 3, 5: 4, 6: 4}[n] and bvh.built_level == built_level
    exp = rcc.brute_force(tris, p, d, idt=NP_I[idx])
    got = _call(bvh, tris, p, d)
    _same(got, exp, (n, built_level))
    assert got["flag"] == 0
    _same(_call(bvh, tris, p, d, mode=abi.CAST_ANY), exp, (n, built_level, "any"), outs="o")
    # what the checker itself says about these inputs
    h = len(HAND_RAYS)
    assert (exp.index[h:] != 0).sum() >= (24 if n >= 2 else 8)                   # the floor (one triangle is half of it) ...
    assert exp.clamped[h:].sum() >= 3 and (exp.index[h:] != 0).sum() - exp.clamped[h:].sum() >= 3   # ... the clamp is active on some rays
    assert (exp.index[17:31] == 0).all() and (exp.index[8:11] == 0).all()       # zero direction, NaN, Inf, in-plane: no hit
    assert exp.index[31] != 0 and (n == 1 or exp.index[32] != 0)                 # a direction component so small that its inverse overflows
    if n >= 4:
        assert exp.index[:3].tolist() == [3, 3, 3] and exp.tied[:3].all()        # the shared edge: equal t*, the smaller index wins
        assert exp.index[3:7].tolist() == [3, 4, 1, 3] and exp.t[[3, 4, 6]].tolist() == [1, 1, 1] and abs(float(exp.t[5]) - 0.7) < 1e-6
        assert exp.index[11:17].tolist() == [2, 3, 1, 4, 1, 3]                   # on faces, edges and corners: by comparison, no NaN
        assert (exp.index[33:38] == 0).all() and exp.index[38] == 3 and exp.t[38] == 0
    # every subset of the closest-hit outputs; what was not asked for is not written
    for outs in ("i", "t", "u", "it", "tu"):
        _same(_call(bvh, tris, p, d, outs=outs), exp, (n, built_level, outs), outs=outs)
    # a limit per ray: the rays' own t (inclusive), every third one halved
    lim = np.where(np.isfinite(exp.t), exp.t, dt(1)).astype(dt)
    lim[::3] *= dt(0.5)
    bounded = rcc.brute_force(tris, p, d, t_max=lim, idt=NP_I[idx])
    _same(_call(bvh, tris, p, d, t_max=lim), bounded, (n, built_level, "t_max"))
    _same(_call(bvh, tris, p, d, t_max=lim, mode=abi.CAST_ANY), bounded, (n, built_level, "t_max, any"), outs="o")
    assert (bounded.index != 0).sum() >= 10 and ((exp.index != 0) & (bounded.index == 0)).sum() >= 5
    # num_rays = 0 with a pre-set flag: nothing is touched
    for mode in (abi.CAST_CLOSEST, abi.CAST_ANY):
        none = _call(bvh, tris, p, d, mode=mode, num_rays=0, flag=4)
        assert none["status"] == 0 and none["flag"] == 4
        _same(none, exp, "empty", outs="")
    # a wrong combination of outputs: refused, nothing written
    for mode, outs in ((abi.CAST_CLOSEST, ""), (abi.CAST_CLOSEST, "ito"), (abi.CAST_CLOSEST, "o"), (abi.CAST_ANY, ""), (abi.CAST_ANY, "io"),
                       (abi.CAST_ANY, "itu"), (2, "itu"), (-1, "o")):
        bad = _call(bvh, tris, p, d, mode=mode, outs=outs)
        assert bad["status"] == abi.ERR_INVALID_ARG and bad["flag"] == 0, (mode, outs)
        _same(dict(bad, status=0), exp, (mode, outs), outs="")
    # num_triangles below the largest leaf index: those leaves are skipped, bit 1 is raised (never cleared: 4 stays)
    if n >= 3:
        for mode, outs in ((abi.CAST_CLOSEST, "itu"), (abi.CAST_ANY, "o")):
            cut = _call(bvh, tris, p, d, mode=mode, num_triangles=n - 2, flag=4)
            assert cut["flag"] == 6
            _same(cut, rcc.brute_force(tris[:n - 2], p, d, idt=NP_I[idx]), "guard", outs=outs)


def test_two_roots_one_over_a_virtual_sibling_and_a_batch_of_a_wave_and_one():
    """built_level = 2 over 3 leaves: the walk starts from two roots, and the second root's other child is virtual; 65
    rays are a full wave and one lane of a second workgroup"""
    tris = np.array(HAND[1:4], np.float32)
    p, d = _hand(np.float32)
    p, d = np.concatenate([p[:64], p[3:4]]), np.concatenate([d[:64], d[3:4]])   # (the 65th ray hits)
    bvh, _ = _build(tris, built_level=2)
    assert len(p) == 65 and (bvh.tree.levels, bvh.built_level, bvh.tree.real_leaves, bvh.tree.virtual_leaves) == (3, 2, 3, 1)
    exp = rcc.brute_force(tris, p, d, idt=np.int32)
    _same(_call(bvh, tris, p, d), exp)
    _same(_call(bvh, tris, p, d, mode=abi.CAST_ANY), exp, outs="o")
    assert set(exp.index.tolist()) == {0, 1, 2, 3} and exp.index[64] != 0      # ... every leaf, hence either root


# ---- 4. skin and refit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_skin_margins_and_refit_keep_the_result_exact(floats):
    leaf_flt, node_flt = FLOATS[floats]
    dt = NP_F[leaf_flt]
    tris, p, d, bf = _reference("torus40", leaf_flt)
    P, D = cuda(p).t(), cuda(d).t()
    # the leaf box is the STORED volume, skin included: the definition is evaluated on it
    lo, up = rcc.triangle_boxes(tris)
    s = dt(0.02)
    exp = rcc.brute_force(tris, p, d, boxes=((lo - s).astype(dt), (up + s).astype(dt)))
    assert (exp.index == bf.index).all() and (_bits(exp.t) == _bits(bf.t)).all() and not exp.clamped.any()
    bvh, tdev = _build(tris, leaf_flt, node_flt, skin=0.02)
    for presorted in (True, False):
        _assert_closest(ibvh.cast_rays(bvh, tdev, P, D, presorted=presorted), exp, (floats, "skin", presorted))
        _assert_any(ibvh.cast_rays(bvh, tdev, P, D, any_hit=True, presorted=presorted), exp, (floats, "skin, any", presorted))
    # refit the tight build to moved vertices: the moved triangles' brute force
    bvh, tdev = _build(tris, leaf_flt, node_flt)
    rng = np.random.default_rng(11)
    verts, inverse = np.unique(tris.reshape(-1, 3), axis=0, return_inverse=True)
    shift = (0.01 * (rng.random(verts.shape) - 0.5)).astype(dt)
    moved = np.ascontiguousarray((verts + shift)[inverse.reshape(-1)].reshape(-1, 9).astype(dt))
    mdev = cuda(moved)
    ibvh.refit(bvh, ibvh.bounding_volumes_from_triangles(mdev, ibvh.BBox(_tf(leaf_flt))))
    exp = rcc.brute_force(moved, p, d)
    assert (_bits(exp.t) != _bits(bf.t)).sum() >= 400 and (exp.index != 0).sum() >= 400
    for presorted in (True, False):
        _assert_closest(ibvh.cast_rays(bvh, mdev, P, D, presorted=presorted), exp, (floats, "refit", presorted))
        _assert_any(ibvh.cast_rays(bvh, mdev, P, D, any_hit=True, presorted=presorted), exp, (floats, "refit, any", presorted))


# ---- 5. the existing path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_agrees_with_raycast_on_the_rays_whose_direction_components_are_all_non_zero(mesh, flt):
    """raycast() is the reference's leaf-vs-tree ray traversal plus the resolve; its slab test has no rule for a zero direction
    component, so the comparison runs on the rays without one — a selection on the INPUT (80 % of the batch), never on a
    result.  There no winner is clamped or tied (asserted), so t* is the resolve's t and both tie rules are idle."""
    tris, p, d, bf = _reference(mesh, flt)
    nz = rcc.all_nonzero(d)
    assert nz.sum() == 640 and not bf.clamped[nz].any() and not bf.tied[nz].any() and (bf.index[nz] != 0).sum() >= 500
    bvh, tdev = _build(tris, flt)
    P, D = cuda(np.ascontiguousarray(p[nz])).t(), cuda(np.ascontiguousarray(d[nz])).t()
    hits, _ = ibvh.raycast(bvh, tdev, P, D)
    got = ibvh.cast_rays(bvh, tdev, P, D)
    assert torch.equal(got.index, hits.index.to(got.index.dtype))
    assert torch.equal(got.t.view(torch.int32 if flt == abi.F32 else torch.int64), hits.t.view(torch.int32 if flt == abi.F32 else torch.int64))
    assert torch.equal(got.uv, hits.uv)
    assert (got.index.cpu().numpy() == bf.index[nz]).all()


# ---- 6. refusals, the empty batch, one launch --------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    tris, p, d, bf = _reference("torus40", abi.F32)
    P, D = cuda(p).t(), cuda(d).t()
    f = getattr(lib.load(), NAME)
    out = torch.full((800,), -7, dtype=torch.int32, device="cuda")
    for what, kw in (("sphere leaves", dict(leaf_kind=abi.BSPHERE)), ("sphere nodes", dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE)),
                     ("f64 leaves under f32 nodes", dict(leaf_flt=abi.F64, node_flt=abi.F32))):
        bvh, tdev = _build(tris, **kw)
        ft = NP_F[bvh.types.leaf_float]
        pts, dirs = cuda(p.astype(ft)), cuda(d.astype(ft))
        st = f(C.byref(bvh.struct()), api._ptr(tdev), len(tris), api._ptr(pts), api._ptr(dirs), 800, None, abi.CAST_CLOSEST, api._ptr(out),
               None, None, None, None, api._stream())
        torch.cuda.synchronize()
        assert st == abi.ERR_UNSUPPORTED and (out == -7).all(), what
        for any_hit in (False, True):
            with pytest.raises(ValueError):
                ibvh.cast_rays(bvh, tdev, pts.t(), dirs.t(), any_hit=any_hit)
    bvh, tdev = _build(tris)
    with pytest.raises(ValueError):
        ibvh.cast_rays(bvh, tdev.double(), P, D)             # triangles of the other dtype
    with pytest.raises(ValueError):
        ibvh.cast_rays(bvh, tdev, P.double(), D)             # origins of the other dtype
    with pytest.raises(ValueError):
        ibvh.cast_rays(bvh, tdev, P, D.double())             # directions of the other dtype
    for bad in (tdev.cpu(), tdev.to(torch.int32), tdev[:, :8], tdev.reshape(-1), tris):
        with pytest.raises(ValueError):
            ibvh.cast_rays(bvh, bad, P, D)
    for bad in (P.cpu(), P.t(), P[:2], P.reshape(-1), p):
        with pytest.raises(ValueError):
            ibvh.cast_rays(bvh, tdev, bad, D)
    for bad in (D.cpu(), D.t(), D[:2], D[:, :799], D.reshape(-1), d):
        with pytest.raises(ValueError):
            ibvh.cast_rays(bvh, tdev, P, bad)
    L = torch.ones(800, device="cuda")
    for bad in (L.cpu(), L.double(), L[:799], L.reshape(1, 800), "far", True, [1.0] * 800):
        with pytest.raises(ValueError, match="t_max"):
            ibvh.cast_rays(bvh, tdev, P, D, t_max=bad)
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.cast_rays(bvh, tdev[:10], P, D)                 # flag bit 1
    with pytest.raises(ValueError, match="outside 1"):
        ibvh.cast_rays(bvh, tdev[:10], P, D, any_hit=True)
    e = ibvh.cast_rays(bvh, tdev, P[:, :0], D[:, :0])
    assert e.index.shape == e.t.shape == e.hit.shape == (0,) and e.uv.shape == (0, 2)
    assert e.index.dtype == torch.int32 and e.t.dtype == torch.float32 and e.uv.dtype == torch.float32 and e.hit.dtype == torch.bool
    o = ibvh.cast_rays(bvh, tdev, P[:, :0], D[:, :0], any_hit=True, t_max=L[:0])
    assert o.shape == (0,) and o.dtype == torch.bool


def test_one_call_is_one_kernel_of_the_new_translation_unit():
    tris, p, d, bf = _reference("torus40", abi.F32)
    bvh, tdev = _build(tris)
    P, D = cuda(p).t(), cuda(d).t()
    L = torch.ones(800, device="cuda")
    for kw in (dict(), dict(any_hit=True), dict(t_max=L)):
        assert_one_kernel(lambda: ibvh.cast_rays(bvh, tdev, P, D, presorted=True, **kw), "cast_walk_kernel", kw)
