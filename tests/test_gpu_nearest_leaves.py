"""ibvh_nearest_leaves / nearest_leaves on the GPU: indices and squared distances are BIT-EQUAL to the brute force over all
leaves of tests/nearest_leaves_checker.py — the definition of the result — through the C entry point and through the Python
mirror: every accepted leaf / node type, both index types, a 16-bit and a 64-bit Morton type, trees from one leaf to one
level more than a power of two, partial builds, query batches around a wave, k below and above the number of leaves, ties
on a lattice, duplicates, caller-supplied indices, bounded searches, NaN / infinite / degenerate inputs, refit, the
Morton-sorted default path against the given order, the refusals, and the one launch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

import nearest_leaves_checker as nlc  # noqa: E402
from mesh_query_kit import NP_F, NP_I, assert_one_kernel, tf as _tf  # noqa: E402
from test_gpu_parity import cuda, make_options  # noqa: E402

# (leaf kind, leaf float, node float)
COMBOS = {"sphere32_box32": (abi.BSPHERE, abi.F32, abi.F32), "sphere32_box64": (abi.BSPHERE, abi.F32, abi.F64),
          "sphere64_box64": (abi.BSPHERE, abi.F64, abi.F64), "box32_box32": (abi.BBOX, abi.F32, abi.F32),
          "box64_box64": (abi.BBOX, abi.F64, abi.F64)}
KS = (1, 2, 3, 8, 16)


@functools.lru_cache(maxsize=None)
def _cloud(kind, flt, n, seed=1):
    """n volumes in the unit cube (computed once, shared, never modified): spheres of radius < 0.03 / boxes of half width < 0.03"""
    rng = np.random.default_rng(seed + 7 * n)
    c = rng.random((n, 3))
    if kind == abi.BSPHERE:
        v = np.concatenate([c, 0.03 * rng.random((n, 1))], axis=1)
    else:
        h = 0.03 * rng.random((n, 3))
        v = np.concatenate([c - h, c + h], axis=1)
    v = v.astype(NP_F[flt])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _points(flt, m, seed=2):
    """m query points: in the cube inflated by a quarter each way"""
    rng = np.random.default_rng(seed + 11 * m)
    return (rng.random((m, 3)) * 1.5 - 0.25).astype(NP_F[flt])


def _build(vols, node_flt=None, idx=abi.I32, morton=abi.U32, node_kind=abi.BBOX, built_level=1, indices=None):
    kind = abi.BSPHERE if vols.shape[1] == 4 else abi.BBOX
    flt = abi.F32 if vols.dtype == np.float32 else abi.F64
    node_flt = flt if node_flt is None else node_flt
    types = abi.make_types(kind, flt, node_kind, node_flt, idx, morton)
    opts = make_options(types)
    node_type = (ibvh.BBox if node_kind == abi.BBOX else ibvh.BSphere)(_tf(node_flt))
    src = cuda(vols) if indices is None else ibvh.BoundingVolumes.wrap(cuda(vols), np.asarray(indices), opts)
    bvh = ibvh.BVH(src, node_type, built_level=built_level, options=opts)
    assert bvh.types.key() == types.key()
    return bvh


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _call(bvh, p, k, max_d2=None, outs="id", num_points=None):
    """straight through the C entry -> dict of numpy outputs (prefilled with a sentinel: 'not written' is visible), the status"""
    ft = NP_F[bvh.types.leaf_float]
    p = np.ascontiguousarray(p, dtype=ft)
    n = len(p) if num_points is None else num_points
    P = cuda(p) if len(p) else torch.empty((0, 3), dtype=_tf(bvh.types.leaf_float), device="cuda")
    rows = max(len(p), 1) * max(k, 1)
    o = {"i": torch.full((rows,), -7, dtype=api._torch_index(bvh.types.index_type), device="cuda"),
         "d": torch.full((rows,), -7.0, dtype=_tf(bvh.types.leaf_float), device="cuda")}
    ptr = lambda key: api._ptr(o[key]) if key in outs else None
    r2 = None if max_d2 is None else C.byref((C.c_float if ft == np.float32 else C.c_double)(max_d2))
    st = getattr(lib.load(), "ibvh_nearest_leaves")(C.byref(bvh.struct()), api._ptr(P), n, k, r2, ptr("i"), ptr("d"), api._stream())
    torch.cuda.synchronize()
    out = {key: v.cpu().numpy().reshape(max(len(p), 1), max(k, 1)) for key, v in o.items()}
    out["status"] = st
    return out


def _same(got, exp, what=None):
    assert got["status"] == abi.OK, what
    assert (got["i"] == exp.index).all(), what
    assert _bits(got["d"]) == _bits(exp.d2), what


def _same_api(got, exp, what=None):
    assert (got.index.cpu().numpy() == exp.index).all(), what
    assert _bits(got.d2.cpu().numpy()) == _bits(exp.d2), what


# ---- 1. leaf counts x types x k ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 1000, 4097])
def test_every_tree_shape_type_and_k_is_bit_equal_to_the_brute_force(n, combo):
    kind, flt, node_flt = COMBOS[combo]
    vols, p = _cloud(kind, flt, n), _points(flt, 65)
    bvh = _build(vols, node_flt)
    assert bvh.tree.real_leaves == n and (bvh.tree.virtual_leaves > 0) == (n & (n - 1) != 0)
    index = np.arange(1, n + 1)
    for k in KS:
        exp = nlc.brute_force(vols, index, p, k)
        assert (exp.count == min(k, n)).all()
        got = _call(bvh, p, k)
        _same(got, exp, (n, combo, k))
        if k > n:  # more slots than leaves: the tail is 0 / +Inf
            assert (got["i"][:, n:] == 0).all() and np.isposinf(got["d"][:, n:]).all() and (got["i"][:, :n] > 0).all()
        assert (got["d"][:, 1:] >= got["d"][:, :-1]).all()
    res = ibvh.nearest_leaves(bvh, cuda(p).t(), k=3)
    assert res.index.shape == res.d2.shape == (65, 3) and res.index.dtype == torch.int32 and res.d2.dtype == _tf(flt)
    _same_api(res, nlc.brute_force(vols, index, p, 3), (n, combo, "mirror"))


# ---- 2. query counts, index types --------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_query_batches_around_a_wave_and_both_index_types(m, idx):
    for kind, flt in ((abi.BSPHERE, abi.F32), (abi.BBOX, abi.F64)):
        vols, p = _cloud(kind, flt, 1000), _points(flt, m)
        bvh = _build(vols, idx=idx)
        for k in (1, 8, 16):
            exp = nlc.brute_force(vols, np.arange(1, 1001), p, k, idt=NP_I[idx])
            got = _call(bvh, p, k)
            assert got["i"].dtype == NP_I[idx]
            _same(got, exp, (m, idx, kind, k))
            # either output alone; what was not asked for is not written
            for outs in ("i", "d"):
                sub = _call(bvh, p, k, outs=outs)
                assert sub["status"] == abi.OK
                assert _bits(sub["i"]) == (_bits(exp.index) if outs == "i" else _bits(np.full_like(exp.index, -7)))
                assert _bits(sub["d"]) == (_bits(exp.d2) if outs == "d" else _bits(np.full_like(exp.d2, -7)))
        res = ibvh.nearest_leaves(bvh, cuda(p).t(), k=8)
        assert res.index.dtype == (torch.int32 if idx == abi.I32 else torch.int64)
        _same_api(res, nlc.brute_force(vols, np.arange(1, 1001), p, 8), (m, idx, kind, "mirror"))


# ---- 3. Morton types, partial builds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
@pytest.mark.parametrize("morton", [abi.U16, abi.U64], ids=["u16", "u64"])
def test_a_16_bit_and_a_64_bit_morton_type(morton, idx):
    for combo in ("sphere32_box32", "box64_box64"):
        kind, flt, node_flt = COMBOS[combo]
        vols, p = _cloud(kind, flt, 1000), _points(flt, 65)
        bvh = _build(vols, node_flt, idx=idx, morton=morton)
        assert bvh.types.morton_type == morton
        for k in (1, 3, 16):
            _same(_call(bvh, p, k), nlc.brute_force(vols, np.arange(1, 1001), p, k, idt=NP_I[idx]), (morton, idx, combo, k))


@pytest.mark.parametrize("n,built_level", [(1, 1), (5, 1), (5, 2), (5, 4), (1000, 3), (1000, 8), (1000, 11), (4097, 6)])
def test_partial_builds_read_nothing_above_the_built_level(n, built_level):
    for combo in ("sphere32_box32", "box32_box32"):
        kind, flt, node_flt = COMBOS[combo]
        vols, p = _cloud(kind, flt, n), _points(flt, 65)
        bvh = _build(vols, node_flt, built_level=built_level)
        assert bvh.built_level == built_level and bvh.tree.levels == {1: 1, 5: 4, 1000: 11, 4097: 14}[n]
        for k in (1, 8):
            _same(_call(bvh, p, k), nlc.brute_force(vols, np.arange(1, n + 1), p, k), (n, built_level, combo, k))


# ---- 4. ties -----------------------------------------------------------------------------------------------------------
def _lattice(kind, flt, side=5):
    dt = NP_F[flt]
    c = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(dt)
    if kind == abi.BSPHERE:
        return np.concatenate([c, np.full((len(c), 1), 0.25, dt)], axis=1), c
    return np.concatenate([c - dt(0.25), c + dt(0.25)], axis=1), c


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_equal_distances_resolve_by_the_smaller_index(combo):
    kind, flt, node_flt = COMBOS[combo]
    vols, c = _lattice(kind, flt)
    assert _bits(nlc.centers(vols)) == _bits(c)                       # the centres ARE the lattice points, exactly
    p = np.concatenate([c[::3], c[:60] + NP_F[flt](0.5)])             # lattice points and cell centres
    n = len(vols)
    rng = np.random.default_rng(4)
    shuffled = rng.permutation(np.arange(1, n + 1)) * 7 - 300          # caller-supplied: non-monotone, some negative, none 0
    assert (shuffled != 0).all()
    for what, v, index in (("built", vols, None), ("wrapped", vols, shuffled),
                           ("duplicated", np.concatenate([vols, vols[10:40]]), None)):
        bvh = _build(v, node_flt, indices=index)
        ids = np.arange(1, len(v) + 1) if index is None else index
        for k in KS:
            exp = nlc.brute_force(v, ids, p, k)
            assert (exp.ties > 0).sum() >= len(p) // 2, (what, k)      # the comparison means something
            _same(_call(bvh, p, k), exp, (combo, what, k))
        _same_api(ibvh.nearest_leaves(bvh, cuda(p).t(), k=16), nlc.brute_force(v, ids, p, 16), (combo, what, "mirror"))
    # a duplicate's copy (index > n) never comes before its original
    exp = nlc.brute_force(np.concatenate([vols, vols[10:40]]), np.arange(1, n + 31), c[10:40], 2)
    assert (exp.index[:, 0] == np.arange(11, 41)).all() and (exp.index[:, 1] == np.arange(n + 1, n + 31)).all() and (exp.d2 == 0).all()


# ---- 5. radius ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["sphere32_box32", "sphere64_box64", "box32_box32"])
def test_bounded_searches(combo):
    kind, flt, node_flt = COMBOS[combo]
    dt = NP_F[flt]
    vols = _cloud(kind, flt, 1000)
    centres = nlc.centers(vols)
    p = np.concatenate([_points(flt, 100), centres[:20]])              # the last 20 queries sit exactly on a centre
    index = np.arange(1, 1001)
    bvh = _build(vols, node_flt)
    unbounded = nlc.brute_force(vols, index, p, 8)
    # a radius whose square is EXACTLY the 4th distance of the first query: d2 == max_d2 qualifies
    edge = unbounded.d2[0, 3]
    for max_d2 in (edge, np.nextafter(edge, dt(0)), dt(0.01), dt(0), dt(-1), dt(np.nan), dt(np.inf)):
        for k in (1, 8, 16):
            exp = nlc.brute_force(vols, index, p, k, max_d2)
            _same(_call(bvh, p, k, max_d2=max_d2), exp, (combo, max_d2, k))
    assert nlc.brute_force(vols, index, p, 8, edge).count[0] == 4 and nlc.brute_force(vols, index, p, 8, np.nextafter(edge, dt(0))).count[0] == 3
    few = nlc.brute_force(vols, index, p, 8, dt(0.01))
    assert ((few.count > 0) & (few.count < 8)).sum() >= 50 and (few.count == 0).any()   # fewer than k, and none at all
    zero = nlc.brute_force(vols, index, p, 8, dt(0))
    assert (zero.count[:100] == 0).all() and (zero.count[100:] == 1).all() and (zero.index[100:, 0] == np.arange(1, 21)).all()
    # the mirror squares the radius in the leaves' dtype on the host
    r = dt(0.1)
    for presorted in (True, False):
        _same_api(ibvh.nearest_leaves(bvh, cuda(p).t(), k=8, max_distance=float(r), presorted=presorted),
                  nlc.brute_force(vols, index, p, 8, r * r), (combo, presorted))
    _same_api(ibvh.nearest_leaves(bvh, cuda(p).t(), k=2, max_distance=0), nlc.brute_force(vols, index, p, 2, dt(0)), combo)


# ---- 6. special inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_nan_queries_infinite_and_zero_radii(flt):
    dt = NP_F[flt]
    base = _cloud(abi.BSPHERE, flt, 65)
    p = np.concatenate([_points(flt, 30), [[np.nan, 0.5, 0.5], [0.5, 0.5, np.nan], [np.nan] * 3, [np.inf, 0.5, 0.5], [0.5, -np.inf, np.inf]]]).astype(dt)
    index = np.arange(1, 66)
    cases = {"plain": base}
    v = base.copy()
    v[17, 3] = np.inf                                                  # one leaf's box is all of space
    cases["infinite radius"] = v
    v = base.copy()
    v[:, 3] = 0                                                        # every box is a point
    cases["zero radii"] = v
    for what, vols in cases.items():
        bvh = _build(vols)
        for k in (1, 3, 16):
            exp = nlc.brute_force(vols, index, p, k)
            got = _call(bvh, p, k)
            _same(got, exp, (what, k))
            # a NaN coordinate: every slot is empty; an infinite one: every d2 is +Inf and the smallest indices win
            assert (got["i"][30:33] == 0).all() and np.isposinf(got["d"][30:33]).all()
            assert (got["i"][33:] == np.arange(1, k + 1)).all() and np.isposinf(got["d"][33:]).all()
            assert not np.isnan(got["d"]).any()
    boxes = _cloud(abi.BBOX, flt, 65).copy()
    boxes[:8, 3:] = boxes[:8, :3]                                      # degenerate boxes: lo == up
    bvh = _build(boxes)
    for k in (1, 16):
        _same(_call(bvh, p, k), nlc.brute_force(boxes, index, p, k), ("degenerate boxes", k))


# ---- 7. refit, input order ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_refit_to_moved_volumes(combo):
    kind, flt, node_flt = COMBOS[combo]
    vols, p = _cloud(kind, flt, 1000), _points(flt, 200)
    index = np.arange(1, 1001)
    bvh = _build(vols, node_flt)
    before = nlc.brute_force(vols, index, p, 8)
    rng = np.random.default_rng(12)
    moved = vols.copy()
    shift = (0.05 * (rng.random((1000, 3)) - 0.5)).astype(vols.dtype)
    moved[:, :3] += shift
    if kind == abi.BBOX:
        moved[:, 3:] += shift
    ibvh.refit(bvh, cuda(moved))
    exp = nlc.brute_force(moved, index, p, 8)
    assert (exp.index != before.index).any() and _bits(exp.d2) != _bits(before.d2)
    _same(_call(bvh, p, 8), exp, (combo, "refit"))
    for presorted in (True, False):
        _same_api(ibvh.nearest_leaves(bvh, cuda(p).t(), k=8, presorted=presorted), exp, (combo, "refit", presorted))


def test_unsorted_points_give_the_rows_of_the_presorted_batch():
    vols = _cloud(abi.BSPHERE, abi.F32, 4097)
    p = _points(abi.F32, 1000)
    bvh = _build(vols)
    P = cuda(p)
    order = api._morton_order(P)
    assert not torch.equal(order, torch.arange(1000, device="cuda"))
    for k, radius in ((1, None), (16, None), (8, 0.05)):
        given = ibvh.nearest_leaves(bvh, P.t(), k=k, max_distance=radius)
        srt = ibvh.nearest_leaves(bvh, P[order].t(), k=k, max_distance=radius, presorted=True)
        assert torch.equal(given.index[order], srt.index) and _bits(given.d2[order].cpu().numpy()) == _bits(srt.d2.cpu().numpy())
        max_d2 = None if radius is None else np.float32(radius) * np.float32(radius)
        _same_api(given, nlc.brute_force(vols, np.arange(1, 4098), p, k, max_d2), (k, radius))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_and_the_python_mirror():
    spheres, p = _cloud(abi.BSPHERE, abi.F32, 65), _points(abi.F32, 65)
    for what, bvh in (("sphere nodes", _build(spheres, node_kind=abi.BSPHERE)),
                      ("f64 spheres under f32 nodes", _build(_cloud(abi.BSPHERE, abi.F64, 65), abi.F32)),
                      ("f64 boxes under f32 nodes", _build(_cloud(abi.BBOX, abi.F64, 65), abi.F32))):
        got = _call(bvh, p, 3)
        assert got["status"] == abi.ERR_UNSUPPORTED and (got["i"] == -7).all() and (got["d"] == -7).all(), what
        with pytest.raises(ValueError):
            ibvh.nearest_leaves(bvh, cuda(p.astype(NP_F[bvh.types.leaf_float])).t(), k=3)
    bvh = _build(spheres)
    for k in (0, 17, -1):
        got = _call(bvh, p, k)
        assert got["status"] == abi.ERR_INVALID_ARG and (got["i"] == -7).all() and (got["d"] == -7).all(), k
        with pytest.raises(ValueError):
            ibvh.nearest_leaves(bvh, cuda(p).t(), k=k)
    got = _call(bvh, p, 3, outs="")
    assert got["status"] == abi.ERR_INVALID_ARG                        # no output pointer
    none = _call(bvh, p, 3, num_points=0)
    assert none["status"] == abi.OK and (none["i"] == -7).all() and (none["d"] == -7).all()   # nothing is touched
    P = cuda(p).t()
    for bad in (P.cpu(), P.t(), P[:2], P.reshape(-1), P.double(), p):
        with pytest.raises(ValueError):
            ibvh.nearest_leaves(bvh, bad)
    with pytest.raises(ValueError):
        ibvh.nearest_leaves(bvh, P, k=2.0)
    e = ibvh.nearest_leaves(bvh, P[:, :0], k=4)
    assert e.index.shape == e.d2.shape == (0, 4) and e.index.dtype == torch.int32 and e.d2.dtype == torch.float32


# ---- 9. one launch -----------------------------------------------------------------------------------------------------
def test_one_call_is_one_kernel_of_the_new_translation_unit():
    bvh = _build(_cloud(abi.BSPHERE, abi.F32, 1000))
    P = cuda(_points(abi.F32, 65)).t()
    assert_one_kernel(lambda: ibvh.nearest_leaves(bvh, P, k=8, presorted=True), "nearest_walk_kernel")
