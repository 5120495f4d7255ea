"""ibvh_nearest_leaves on the host side: the header declares it (additive under ABI version 7) and carries its contract; the
header, the ctypes mirror and the Julia extension agree on the prototype and on IBVH_NEAREST_MAX_K; the Makefile builds its
translation unit and its one launch goes through the profiling wrapper; the entry point validates its arguments — the
refused type combinations included — before any launch.  The numpy checker the GPU test pins the kernel to
(tests/nearest_leaves_checker.py) agrees with a naive per-point loop, and its point-box bound never exceeds the distance of
a centre inside the box.  No GPU."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib

import mesh_query_kit as kit
import nearest_leaves_checker as nlc

NAME = "ibvh_nearest_leaves"
_fake_bvh = functools.partial(kit.fake_bvh, leaf_kind=abi.BSPHERE)


def test_header_declares_the_entry_point_under_abi_version_7():
    raw, hdr, args, note = kit.header_prototype(NAME)
    assert args == ["const ibvh_bvh *bvh", "const void *points", "int64_t num_points", "int32_t k", "const void *max_distance2",
                    "void *nearest_index", "void *nearest_d2", "void *stream"]
    assert NAME in note and "IBVH_NEAREST_MAX_K" in note and note.count("additive") >= 3
    # the doc comment carries the contract: arithmetic, tie rule, the bound and why, what makes it exact, accepted types
    doc = raw[raw.index("k nearest leaves for a batch of query points"):raw.index("ibvh_status " + NAME)]
    for phrase in ("(e0*e0 + e1*e1) + e2*e2", "0.5 * (lo + up)", "LEXICOGRAPHICALLY SMALLEST", "SMALLER INDEX", "false on NaN",
                   "lb > the k-th best", "EVERY LEAF CENTRE MUST LIE IN THE BOXES ABOVE IT", "r >= 0", "ibvh_refit",
                   "IBVH_ERR_UNSUPPORTED", "0 / +Inf", "HOST pointer", "num_points == 0", "ASCENDING", "x -/+ r", "built_level"):
        assert phrase in doc, phrase


def test_header_mirror_and_julia_agree_on_the_prototype_and_the_largest_k():
    hdr = kit.read("include", "ibvh.h")
    max_k = int(re.search(r"#define IBVH_NEAREST_MAX_K (\d+)", hdr).group(1))
    assert max_k == abi.NEAREST_MAX_K == 16
    want = [C.POINTER(abi.Bvh), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert abi.NEAREST_LEAVES_ARGTYPES == want and lib.SIGNATURES[NAME] == want
    assert hasattr(lib.load(), NAME), "libibvh.so exports " + NAME
    src = kit.julia_ccall(NAME, "nearest_leaves")
    assert int(re.search(r"const IBVH_NEAREST_MAX_K = (\d+)", src).group(1)) == max_k


def test_makefile_launch_and_python_surface():
    for name in ("nearest_leaves", "NearestLeaves"):
        assert name in ibvh.__all__ and callable(getattr(ibvh, name))
    # the walk, its block size and grid and the prologue are the shared ones; no mesh: no gather, no flag, its own dispatch
    src = kit.query_unit("ibvh_nearest.hip", "nearest::nearest_walk_kernel", mesh=False)
    assert "pointwalk::hopeless(p, max_d2)" in src and "pointwalk::radius_or_inf<T>(max_distance2)" in src
    assert "-ffp-contract=off" in kit.read("implicitbvh.jl_amd", "csrc", "Makefile")
    for text in (src, kit.read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")):
        assert "fp-contract" not in text and "fma(" not in text   # the Makefile's -ffp-contract=off holds for this file


def test_entry_point_validates_its_arguments_before_any_launch():
    f = getattr(lib.load(), NAME)
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    radius = C.byref(C.c_float(1.0))
    ok = dict(bvh=_fake_bvh(), pts=p, np_=0, k=1, r2=radius, ni=p, nd=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        bvh = C.byref(a["bvh"]) if a["bvh"] is not None else None
        return f(bvh, a["pts"], a["np_"], a["k"], a["r2"], a["ni"], a["nd"], a["stream"])
    assert call() == abi.OK                                        # num_points = 0: nothing to do
    assert call(r2=None) == abi.OK                                 # NULL radius = +Inf
    assert call(pts=None) == abi.OK                                # ... and no points are needed for none
    assert call(ni=None) == abi.ERR_INVALID_ARG                    # no output requested
    assert call(ni=None, nd=p) == abi.OK                           # ... either output will do
    for k in (1, 2, 3, 8, 16):
        assert call(k=k) == abi.OK
    for k in (0, 17, -1, 1 << 20):
        assert call(k=k) == abi.ERR_INVALID_ARG and call(k=k, np_=5) == abi.ERR_INVALID_ARG, k
    for bad in (dict(bvh=None), dict(np_=-1), dict(np_=5, pts=None), dict(bvh=_fake_bvh(leaves=None)),
                dict(bvh=_fake_bvh(nodes=None)), dict(bvh=_fake_bvh(built_level=0)), dict(bvh=_fake_bvh(built_level=5))):
        assert call(**bad) == abi.ERR_INVALID_ARG, bad
    assert call(bvh=_fake_bvh(n=1, nodes=None)) == abi.OK          # a one-leaf tree has no nodes
    broken = _fake_bvh()
    broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
    assert call(bvh=broken) == abi.ERR_INVALID_ARG
    # accepted: sphere or box leaves under BBox nodes of the same or a wider float type, any index and Morton type
    for good in (dict(), dict(leaf_kind=abi.BBOX), dict(node_float=abi.F64), dict(leaf_float=abi.F64, node_float=abi.F64),
                 dict(leaf_kind=abi.BBOX, leaf_float=abi.F64, node_float=abi.F64), dict(idx=abi.I64), dict(morton=abi.U16),
                 dict(morton=abi.U64)):
        assert call(bvh=_fake_bvh(**good)) == abi.OK, good
    for bad in (dict(node_kind=abi.BSPHERE), dict(leaf_kind=abi.BBOX, node_kind=abi.BSPHERE), dict(leaf_float=abi.F64, node_float=abi.F32),
                dict(leaf_kind=abi.BBOX, leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2), dict(morton=3)):
        # (with points to process too: refused, never launched on the fake pointers)
        assert call(bvh=_fake_bvh(**bad)) == abi.ERR_UNSUPPORTED and call(bvh=_fake_bvh(**bad), np_=5) == abi.ERR_UNSUPPORTED, bad


# ---- the checker --------------------------------------------------------------------------------------------------------
def _naive(volumes, indices, points, k, max_d2=None, idt=np.int32):
    """the definition of include/ibvh.h as a per-point, per-leaf Python loop over numpy scalars: a second, independent
    statement of it (slow: a few dozen leaves)"""
    v = np.asarray(volumes)
    dt = v.dtype.type
    max_d2 = dt(np.inf) if max_d2 is None else dt(max_d2)
    half = dt(0.5)
    index = np.zeros((len(points), k), idt)
    out = np.full((len(points), k), np.inf, v.dtype)
    with np.errstate(all="ignore"):
        for i, p in enumerate(np.asarray(points, dtype=v.dtype)):
            found = []
            for vol, j in zip(v, indices):
                c = vol[:3] if len(vol) == 4 else [half * (vol[a] + vol[a + 3]) for a in range(3)]
                e = [p[a] - c[a] for a in range(3)]
                d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                assert type(d2) is dt
                if d2 <= max_d2:
                    found.append((d2, int(j)))
            for s, (d2, j) in enumerate(sorted(found)[:k]):
                index[i, s], out[i, s] = j, d2
    return index, out


def _volumes(rng, n, width, dt):
    c = rng.random((n, 3))
    if width == 4:
        return np.concatenate([c, 0.05 * rng.random((n, 1))], axis=1).astype(dt)
    h = 0.05 * rng.random((n, 3))
    return np.concatenate([c - h, c + h], axis=1).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("width", [4, 6], ids=["spheres", "boxes"])
def test_checker_agrees_with_a_naive_per_point_loop(width, dt):
    rng = np.random.default_rng(5)
    v = _volumes(rng, 40, width, dt)
    v[7] = v[3]                                                  # a duplicate: equal d2, the smaller index first
    # centres partly on a lattice, queries on lattice points and cell centres: many exactly equal d2
    lattice = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(dt)
    v[10:37, :3] = lattice if width == 4 else lattice - dt(0.25)
    if width == 6:
        v[10:37, 3:] = lattice + dt(0.25)
    idx = rng.permutation(np.arange(1, 41)) * 3 - 50             # caller-supplied, non-monotone, some negative
    p = np.concatenate([rng.random((20, 3)) * 2, lattice[:10], lattice[:8] + 0.5, [[np.nan, 0, 0], [0.5, np.inf, 0.5]]]).astype(dt)
    some_d2 = np.sort(nlc.distances2(nlc.centers(v), p)[0])[4]
    for k, max_d2 in ((1, None), (3, None), (16, None), (5, dt(0.3)), (4, dt(0)), (2, dt(-1)), (3, dt(np.nan)), (8, some_d2)):
        bf = nlc.brute_force(v, idx, p, k, max_d2, idt=np.int64)
        ni, nd = _naive(v, idx, p, k, max_d2, idt=np.int64)
        assert (bf.index == ni).all() and bf.d2.tobytes() == nd.tobytes(), (k, max_d2)
        assert bf.index.shape == bf.d2.shape == (len(p), k) and bf.d2.dtype == dt
        if max_d2 is not None:
            assert (bf.count == np.isfinite(nd).sum(axis=1)).all()
    bf = nlc.brute_force(v, idx, p, 16)
    assert (bf.ties[20:38] > 0).sum() >= 10 and (bf.count[:38] == 16).all() and bf.count[38] == 0
    # more slots than leaves: the tail is 0 / +Inf
    bf = nlc.brute_force(v[:3], idx[:3], p[:5], 5)
    assert (bf.index[:, 3:] == 0).all() and np.isposinf(bf.d2[:, 3:]).all() and (bf.count == 3).all()
    assert (np.sort(bf.index[:, :3], axis=1) == np.sort(idx[:3])).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("width", [4, 6], ids=["spheres", "boxes"])
def test_box_lower_bound_never_exceeds_the_distance_of_a_centre_inside(width, dt):
    rng = np.random.default_rng(6)
    v = _volumes(rng, 512, width, dt)
    v[:8, 3:] = v[:8, :3] if width == 6 else 0                  # degenerate boxes, zero-radius spheres
    p = (rng.random((300, 3)) * 1.5 - 0.25).astype(dt)
    p[:8] = nlc.centers(v)[:8]
    d2 = nlc.distances2(nlc.centers(v), p)
    lo, up = nlc.leaf_boxes(v)
    assert (lo <= nlc.centers(v)).all() and (nlc.centers(v) <= up).all()
    lb = nlc.box_lower_bound(lo[None], up[None], p[:, None, :])
    assert lb.shape == d2.shape and lb.dtype == dt and (lb <= d2).all() and (lb[np.arange(8), np.arange(8)] == 0).all()
    # ... and of the minima / maxima of neighbouring boxes, level by level (the nodes above the leaves)
    group = 1
    while len(lo) > 1:
        lo, up = np.minimum(lo[0::2], lo[1::2]), np.maximum(up[0::2], up[1::2])
        group *= 2
        lb = nlc.box_lower_bound(lo[None], up[None], p[:, None, :])
        assert (np.repeat(lb, group, axis=1) <= d2).all(), group
