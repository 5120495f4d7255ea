"""ibvh_cast_spheres / cast_spheres on the GPU: the first leaf hit, its time and the any-hit mask are the brute force over ALL
leaves of tests/sphere_cast_checker.py — the definition of the result: the index by value, t BIT FOR BIT — through the Python
mirror and straight through the C entry point: the three float combinations and both index types on the cloud with its
duplicated leaves, in the given order and through the Morton-sorted default; the lattice and the nested pairs, whose inner
boxes poke out of their parents' stored boxes (the hazard step 5 of the definition answers); radii as None, a number, a
tensor; per-query limits and skipped leaves; a cloud swept against itself; trees from one leaf to one level more than a power
of two at every built level, every output subset, batches around a wave; agreement with the pair traversal about who
overlaps; refit; the refusals; the empty batch; and the one launch."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api  # noqa: E402

import mesh_query_kit as kit  # noqa: E402
import sphere_cast_checker as scc  # noqa: E402
from mesh_query_kit import FLOATS, NP_F, NP_I, tf as _tf  # noqa: E402
from test_gpu_parity import cuda, make_options  # noqa: E402


def _build(spheres, node_flt=None, idx=abi.I32, node_kind=abi.BBOX, built_level=1):
    flt = abi.F32 if spheres.dtype == np.float32 else abi.F64
    node_flt = flt if node_flt is None else node_flt
    kind = abi.BSPHERE if spheres.shape[1] == 4 else abi.BBOX
    types = abi.make_types(kind, flt, node_kind, node_flt, idx)
    node_type = (ibvh.BBox if node_kind == abi.BBOX else ibvh.BSphere)(_tf(node_flt))
    bvh = ibvh.BVH(cuda(np.array(spheres)), node_type, built_level=built_level, options=make_options(types))
    assert bvh.types.key() == types.key()
    return bvh


def _inputs(bvh):
    """the checker's view of a built BVH: the leaf order and the stored boxes directly above the leaves"""
    return scc.tree_inputs(bvh.leaves.index.cpu().numpy(), bvh.nodes.cpu().numpy(), bvh.tree.levels, bvh.tree.virtual_leaves, bvh.built_level)


_memo = {}


def _expected(spheres, bvh, p, d, r, t_max=None, skip=None, key=None):
    """the brute force for this BVH's leaf order and parent boxes; with a key, computed once per distinct tree"""
    order, boxes = _inputs(bvh)
    if key is not None:
        key = (key, spheres.dtype.str, order.tobytes(), None if boxes is None else boxes.tobytes())
        if key not in _memo:
            _memo[key] = scc.brute_force(spheres, order, boxes, p, d, r, t_max=t_max, skip=skip)
        return _memo[key]
    return scc.brute_force(spheres, order, boxes, p, d, r, t_max=t_max, skip=skip)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _dev(x, dtype=None):
    return None if x is None else cuda(np.array(x, dtype=dtype))


def _run(bvh, p, d, r=None, t_max=None, skip=None, **kw):
    """the Python mirror on numpy inputs ((m, 3) points and displacements)"""
    sk = None if skip is None else cuda(np.asarray(skip).astype(NP_I[bvh.types.index_type]))
    return ibvh.cast_spheres(bvh, cuda(np.array(p)).t(), cuda(np.array(d)).t(), radii=r if r is None or np.isscalar(r) else _dev(r),
                             t_max=t_max if t_max is None or np.isscalar(t_max) else _dev(t_max), skip=sk, **kw)


_same = functools.partial(kit.assert_closest, kit.CAST_SPHERES)       # the index by value, t BIT FOR BIT, .hit
_same_any = functools.partial(kit.assert_any, kit.CAST_SPHERES)
_same_c = functools.partial(kit.first_hit_same, kit.CAST_SPHERES)     # ... straight through the C entry


def _check(bvh, spheres, p, d, r, t_max=None, skip=None, key=None, what=None, orders=(True, False)):
    exp = _expected(spheres, bvh, p, d, r, t_max=np.asarray(t_max, spheres.dtype) if t_max is not None else None, skip=skip, key=key)
    for presorted in orders:
        _same(_run(bvh, p, d, r, t_max, skip, presorted=presorted), exp, (what, presorted))
        _same_any(_run(bvh, p, d, r, t_max, skip, any_hit=True, presorted=presorted), exp, (what, presorted, "any"))
    return exp


# ---- 1. the whole pipeline ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_cloud_is_the_brute_force_in_the_given_order_and_through_the_sorted_default(floats, idx):
    flt, node_flt = FLOATS[floats]
    spheres, p, d, r, _ = scc.reference(NP_F[flt])["cloud"]
    bvh = _build(spheres, node_flt, idx)
    assert bvh.tree.levels == 13 and bvh.nodes.dtype == _tf(node_flt)
    exp = _check(bvh, spheres, p, d, r, key="cloud", what=(floats, idx))
    got = _run(bvh, p, d, r)
    assert got.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64) and got.t.dtype == _tf(flt)
    # the comparison means something (the host test pins the same floors on the CPU oracle's build)
    hit = exp.index != 0
    assert hit.sum() >= 300 and (~hit).sum() >= 80 and exp.start.sum() >= 100 and (exp.tied & (exp.t > 0)).sum() >= 10 and (exp.tied & (exp.t == 0)).sum() >= 30
    order = api._morton_order(cuda(p))
    assert not torch.equal(order, torch.arange(len(p), device="cuda"))


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_lattice_and_nested_pairs(floats):
    flt, node_flt = FLOATS[floats]
    dt = NP_F[flt]
    spheres, p, d, r, _ = scc.reference(dt)["lattice"]
    exp = _check(_build(spheres, node_flt), spheres, p, d, r, what=(floats, "lattice"))
    assert (exp.index != 0).all() and exp.clamp_own.sum() >= 20
    # the hazard: siblings under a stored parent box with the bits of the outer sphere's box, out of which the inner box pokes
    spheres, p, d, r, skip = scc.reference(dt)["nested"]
    bvh = _build(spheres, node_flt)
    order, boxes = _inputs(bvh)
    siblings = scc.sibling_pairs(spheres, order, boxes)
    exp = _check(bvh, spheres, p, d, r, skip=skip, what=(floats, "nested"))
    k = len(spheres) // 2
    decided = (exp.index[:k] == 0) & (exp.index_no5[:k] != 0) & (exp.t_no5[:k] == 0)
    assert k >= 50 and siblings.sum() >= 20 and decided.sum() >= 20 and (siblings | ~decided).all()


# ---- 2. radii, limits, skipped leaves ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_radii_none_is_zeros_and_a_number_is_a_tensor(flt):
    dt = NP_F[flt]
    spheres, p, d, _, _ = scc.reference(dt)["cloud"]
    bvh = _build(spheres)
    zeros = _check(bvh, spheres, p, d, np.zeros(len(p), dt), key="rays", what="zeros", orders=(False,))
    none = _run(bvh, p, d, None)
    _same(none, zeros, "None")
    _same(_run(bvh, p, d, 0.0), zeros, "0.0")
    _same_any(_run(bvh, p, d, None, any_hit=True), zeros, "None, any")
    fat = _check(bvh, spheres, p, d, np.full(len(p), 0.0125, dt), what="tensor", orders=(False,))
    _same(_run(bvh, p, d, 0.0125), fat, "number")
    assert (fat.index != zeros.index).any()
    # a negative and a NaN radius touch nothing
    for bad in (-1.0, float("nan")):
        got = _run(bvh, p, d, bad)
        assert (got.index == 0).all() and torch.isposinf(got.t).all() and not _run(bvh, p, d, bad, any_hit=True).any()


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_per_query_limits(flt):
    dt = NP_F[flt]
    spheres, p, d, r, _ = scc.reference(dt)["cloud"]
    bvh = _build(spheres)
    free = _expected(spheres, bvh, p, d, r, key="cloud")
    m = len(p)
    hit, two = free.index != 0, (free.second_index != 0) & (free.second_t > free.t)
    assert two.sum() >= 150
    # between the first and the runner-up: the first; exactly the first's t: inclusive; below it: a miss
    between = np.where(two, (free.t + free.second_t) / dt(2), free.t).astype(dt)
    got = _run(bvh, p, d, r, between)
    assert (got.index.cpu().numpy() == free.index).all() and _bits(got.t.cpu().numpy()) == _bits(free.t)
    _same(_run(bvh, p, d, r, free.t.copy()), free, "t_max = t")
    moving = hit & (free.t > 0)
    below = np.where(moving, np.nextafter(free.t, dt(0)), dt(-1)).astype(dt)
    got = _run(bvh, p, d, r, below)
    assert (got.index == 0).all() and torch.isposinf(got.t).all() and not _run(bvh, p, d, r, below, any_hit=True).any()
    # 0: only who touches at the start; +Inf equals none; NaN or negative: a miss; a mixture, against the checker
    zero = _check(bvh, spheres, p, d, r, t_max=np.zeros(m, dt), what="0", orders=(False,))
    assert ((zero.index != 0) == (free.t == 0)).all() and (zero.index != 0).sum() >= 100
    _same(_run(bvh, p, d, r, float("inf")), free, "+Inf")
    _same(_run(bvh, p, d, r, np.full(m, np.inf, dt)), free, "+Inf tensor")
    for bad in (float("nan"), -1.0, -0.5):
        got = _run(bvh, p, d, r, bad)
        assert (got.index == 0).all() and torch.isposinf(got.t).all() and not _run(bvh, p, d, r, bad, any_hit=True).any()
    mixed = free.t.copy()
    mixed[0::5], mixed[1::5], mixed[2::5], mixed[3::5] = np.nan, -1, 0, 1
    some = _check(bvh, spheres, p, d, r, t_max=mixed, what="mixed")
    assert 100 <= (some.index != 0).sum() < hit.sum()


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
def test_skipped_leaves(idx):
    spheres, p, d, r, _ = scc.reference(np.float32)["cloud"]
    bvh = _build(spheres, idx=idx)
    free = _expected(spheres, bvh, p, d, r, key="cloud")
    # skip = the winner: the runner-up; skip = 0: nothing is ignored
    got = _run(bvh, p, d, r, skip=free.index)
    assert (got.index.cpu().numpy() == free.second_index).all() and _bits(got.t.cpu().numpy()) == _bits(free.second_t)
    assert (free.second_index != 0).sum() >= 200
    _same(_run(bvh, p, d, r, skip=np.zeros(len(p), np.int64)), free, "skip = 0")
    _check(bvh, spheres, p, d, r, skip=free.index, what="skip = winner")
    # any mode: skipping the only hit gives 0
    only = free.hits == 1
    mask = _run(bvh, p, d, r, skip=free.index, any_hit=True).cpu().numpy()
    assert only.sum() >= 20 and not mask[only].any() and mask[free.hits >= 2].all()


def test_a_cloud_swept_against_itself():
    dt = np.float32
    spheres, _, _, _, _ = scc.reference(dt)["cloud"]
    rng = np.random.default_rng(21)
    who = rng.choice(3000, 500, replace=False)
    p, r = spheres[who, :3].copy(), spheres[who, 3].copy()
    u = rng.normal(size=(500, 3))
    d = (u / np.linalg.norm(u, axis=1, keepdims=True) * (0.02 + 0.2 * rng.random((500, 1)))).astype(dt)
    bvh = _build(spheres)
    exp = _check(bvh, spheres, p, d, r, skip=who + 1, what="self")
    assert (exp.index != 0).sum() >= 50 and (exp.index != who + 1).all()
    # without the skip every particle finds itself (or its duplicate) at t = 0
    own = _run(bvh, p, d, r)
    assert (own.t == 0).all()


# ---- 3. straight through the C entry ---------------------------------------------------------------------------------------------
def _call(bvh, p, d, r=None, t_max=None, skip=None, **kw):
    return kit.first_hit_call(kit.CAST_SPHERES, bvh, None, (p, d, r), (t_max, skip), **kw)


@functools.lru_cache(maxsize=None)
def _small(n, m=65):
    """n spheres in the unit cube and m queries that mostly hit (computed once, shared)"""
    rng = np.random.default_rng(100 + n)
    spheres = np.concatenate([rng.random((n, 3)), 0.05 + 0.15 * rng.random((n, 1))], axis=1).astype(np.float32)
    p = (rng.random((m, 3)) * 1.6 - 0.3).astype(np.float32)
    d = ((rng.random((m, 3)) - 0.5) * 2).astype(np.float32)
    aimed = np.arange(0, m, 2)                                    # every other one at a leaf, a little off its centre
    d[aimed] = ((spheres[rng.integers(0, n, len(aimed)), :3] - p[aimed]) * 1.5 + 0.05 * (rng.random((len(aimed), 3)) - 0.5)).astype(np.float32)
    r = (0.05 * rng.random(m)).astype(np.float32)
    r[::3] = 0
    for x in (spheres, p, d, r):
        x.setflags(write=False)
    return spheres, p, d, r


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 129])
def test_every_tree_shape_built_level_and_output_subset(n):
    spheres, p, d, r = _small(n)
    levels = {1: 1, 2: 2, 3: 3, 5: 4, 64: 7, 65: 8, 129: 9}[n]
    hits = 0
    for built_level in range(1, levels + 1):
        bvh = _build(spheres, built_level=built_level)
        assert bvh.tree.levels == levels and bvh.built_level == built_level
        order, boxes = _inputs(bvh)
        assert (boxes is None) == (levels < 2 or built_level == levels)
        exp = scc.brute_force(spheres, order, boxes, p, d, r, idt=np.int32)
        hits += int((exp.index != 0).sum())
        for outs in ("it", "i", "t"):   # what is asked for is the checker's, the rest keeps its sentinel
            _same_c(_call(bvh, p, d, r, outs=outs), exp, (n, built_level, outs), outs=outs)
        _same_c(_call(bvh, p, d, r, mode=abi.SPHERECAST_ANY), exp, (n, built_level), outs="a")
    assert hits >= 10 * levels


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_query_batches_around_a_wave(m):
    spheres, p, d, r = _small(129, m)
    bvh = _build(spheres)
    order, boxes = _inputs(bvh)
    exp = scc.brute_force(spheres, order, boxes, p, d, r, idt=np.int32)
    _same_c(_call(bvh, p, d, r), exp, m)
    _same_c(_call(bvh, p, d, r, mode=abi.SPHERECAST_ANY), exp, m, outs="a")
    # fewer queries than rows: the rest is not written
    if m > 1:
        part = _call(bvh, p, d, r, num=m - 1)
        assert (part["i"][:m - 1] == exp.index[:m - 1]).all() and part["i"][m - 1] == -7 and part["t"][m - 1] == -7


# ---- 4. agreement with the pair traversal, refit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_standing_queries_agree_with_the_pair_traversal_about_who_overlaps(flt):
    dt = NP_F[flt]
    spheres, p, _, r, _ = scc.reference(dt)["cloud"]
    bvh = _build(spheres)
    queries = np.concatenate([p, r[:, None]], axis=1).astype(dt)
    contacts = ibvh.traverse(_build(queries), bvh).contacts.cpu().numpy()
    listed = np.zeros(len(p), bool)
    listed[contacts[:, 0] - 1] = True
    mask = _run(bvh, p, np.zeros_like(p), r, any_hit=True).cpu().numpy()
    assert 100 <= listed.sum() < len(p) and (mask == listed).all()
    first = _run(bvh, p, np.zeros_like(p), r)
    assert ((first.index != 0).cpu().numpy() == listed).all() and (first.t[first.index != 0] == 0).all()
    # ... and the leaf named is the smallest index of the query's contacts
    smallest = np.full(len(p), np.iinfo(np.int64).max)
    np.minimum.at(smallest, contacts[:, 0] - 1, contacts[:, 1])
    assert (first.index.cpu().numpy()[listed] == smallest[listed]).all()


@pytest.mark.parametrize("floats", sorted(FLOATS))
def test_refit_to_a_moved_cloud_needs_no_skin(floats):
    flt, node_flt = FLOATS[floats]
    dt = NP_F[flt]
    spheres, p, d, r, _ = scc.reference(dt)["cloud"]
    bvh = _build(spheres, node_flt)
    before = _expected(spheres, bvh, p, d, r, key="cloud")
    rng = np.random.default_rng(12)
    moved = np.array(spheres)
    moved[:, :3] += (0.05 * (rng.random((len(moved), 3)) - 0.5)).astype(dt)
    ibvh.refit(bvh, cuda(moved))
    exp = _check(bvh, moved, p, d, r, what=(floats, "refit"))
    assert (exp.index != before.index).any() and _bits(exp.t) != _bits(before.t) and (exp.index != 0).sum() >= 300


# ---- 5. one launch, the empty batch, the refusals --------------------------------------------------------------------------------
def test_one_call_is_one_kernel_and_the_empty_batch_launches_nothing():
    spheres, p, d, r, _ = scc.reference(np.float32)["cloud"]
    bvh = _build(spheres)
    P, D, R = cuda(np.array(p)).t(), cuda(np.array(d)).t(), cuda(np.array(r))
    for any_hit in (False, True):
        kit.assert_one_kernel(lambda: ibvh.cast_spheres(bvh, P, D, R, any_hit=any_hit, presorted=True), "cast_walk_kernel", any_hit)
    from test_gpu_rays_binned import _kernels_of
    assert _kernels_of(lambda: ibvh.cast_spheres(bvh, P[:, :0], D[:, :0])) == set()
    none = _call(bvh, p, d, r, num=0)
    assert none["status"] == abi.OK and (none["i"] == -7).all() and (none["t"] == -7).all()
    e = ibvh.cast_spheres(bvh, P[:, :0], D[:, :0])
    assert e.index.shape == e.t.shape == (0,) and e.index.dtype == torch.int32 and e.t.dtype == torch.float32
    assert ibvh.cast_spheres(bvh, P[:, :0], D[:, :0], any_hit=True).shape == (0,)


def test_positions_and_normals():
    spheres, p, d, r, _ = scc.reference(np.float64)["cloud"]
    bvh = _build(spheres)
    P, D, R, S = cuda(np.array(p)).t(), cuda(np.array(d)).t(), cuda(np.array(r)), cuda(np.array(spheres))
    res = ibvh.cast_spheres(bvh, P, D, R)
    x, nrm = res.positions(P, D), res.normals(S, P, D)
    hit = res.hit
    assert x.shape == nrm.shape == (3, len(p)) and hit.sum() >= 300
    assert torch.isnan(x[:, ~hit]).all() and torch.isnan(nrm[:, ~hit]).all()
    assert torch.equal(x[:, hit], (P + res.t.clamp(max=1e300)[None] * D)[:, hit])
    # at contact the centres are R + r apart (the moving hits: Float64, a few ulps of the quadratic), the normal has length 1
    moving = hit & (res.t > 0)
    leaf = S[(res.index[moving] - 1).long()]
    gap = torch.linalg.vector_norm(x[:, moving] - leaf[:, :3].t(), dim=0)
    assert moving.sum() >= 150 and ((gap - (leaf[:, 3] + R[moving])).abs() <= 1e-9).all()
    assert ((torch.linalg.vector_norm(nrm[:, hit], dim=0) - 1).abs() <= 1e-12).all()


def test_refusals_of_the_c_entry_and_the_python_mirror():
    spheres, p, d, r = _small(65)
    boxes = np.concatenate([spheres[:, :3] - spheres[:, 3:], spheres[:, :3] + spheres[:, 3:]], axis=1)
    for what, bvh in (("box leaves", _build(boxes)), ("sphere nodes", _build(spheres, node_kind=abi.BSPHERE)),
                      ("f64 leaves under f32 nodes", _build(spheres.astype(np.float64), abi.F32))):
        dt = NP_F[bvh.types.leaf_float]
        for mode, outs in ((abi.SPHERECAST_CLOSEST, "it"), (abi.SPHERECAST_ANY, "a")):
            got = _call(bvh, p, d, r, mode=mode, outs=outs)
            assert got["status"] == abi.ERR_UNSUPPORTED and (got["i"] == -7).all() and (got["t"] == -7).all() and (got["a"] == 9).all(), what
        with pytest.raises(ValueError):
            _run(bvh, p.astype(dt), d.astype(dt), r.astype(dt))
    bvh = _build(spheres)
    for mode, outs in ((abi.SPHERECAST_CLOSEST, ""), (abi.SPHERECAST_CLOSEST, "ia"), (abi.SPHERECAST_CLOSEST, "a"), (abi.SPHERECAST_ANY, "i"),
                       (abi.SPHERECAST_ANY, "ta"), (abi.SPHERECAST_ANY, ""), (2, "it"), (-1, "a")):
        got = _call(bvh, p, d, r, mode=mode, outs=outs)
        assert got["status"] == abi.ERR_INVALID_ARG and (got["i"] == -7).all() and (got["t"] == -7).all() and (got["a"] == 9).all(), (mode, outs)
    assert _call(bvh, p, d, r, num=-1)["status"] == abi.ERR_INVALID_ARG
    P, D, R = cuda(np.array(p)).t(), cuda(np.array(d)).t(), cuda(np.array(r))
    for bad in (dict(points=P.cpu()), dict(points=P.t()), dict(points=P.double()), dict(displacements=D[:, :5]), dict(displacements=D.double()),
                dict(radii=R[:5]), dict(radii=R.double()), dict(radii="1"), dict(t_max=R[:5]), dict(skip=R), dict(skip=torch.zeros(5, dtype=torch.int32, device="cuda")),
                dict(skip=torch.zeros(len(p), dtype=torch.int32))):
        with pytest.raises(ValueError):
            ibvh.cast_spheres(**dict(dict(bvh=bvh, points=P, displacements=D, radii=R), **bad))
