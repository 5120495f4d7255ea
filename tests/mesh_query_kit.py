"""What the tests of the twelve point-walk queries share — closest_points, nearest_leaves, point_crossings, points_inside,
cast_rays, sweep_spheres, triangle_distances, segment_distances and the four list queries sphere_contacts, triangle_contacts,
capsule_contacts, box_contacts —: the type tables and meshes, the mesh-BVH builder, the leaves' stored boxes and the one-kernel
check of the GPU tests; the fake ibvh_bvh, the header / Julia matchers, the chain of boxes above a box and the source-text
facts about the shared front end (csrc/ibvh_pointwalk.hpp) of the host tests.  For the four list queries also everything
about their count / write protocol, which is one protocol: the description of a list query (ListQuery), the checkers'
re-sorting into a leaf order, the two passes through the C entry point, the two comparators, the offsets-and-capacity
scenario, the one-kernel-per-pass check and the entry points' common argument matrix.  For the three first-hit queries
cast_rays, sweep_spheres and cast_spheres (a cloud's, the one query here that is not a mesh's) likewise their closest / any-hit
protocol: the description of a first-hit query (FirstHit), the one call straight through the C entry point, the bit-for-bit
comparator, the closest / any comparators for Python results, the source-text facts about csrc/ibvh_firsthit.hpp and the mode /
outputs part of the entry points' argument matrix.  Each query's checker, hand-made meshes
and reference builders stay with its own tests.  Importing this needs no GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np

from implicitbvh_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_F = {abi.F32: np.float32, abi.F64: np.float64}
NP_I = {abi.I32: np.int32, abi.I64: np.int64}
MESHES = {"torus40": (40, 40), "torus64x63": (64, 63)}   # torus_mesh arguments: 3,200 and 8,064 triangles
FLOATS = {"f32": (abi.F32, abi.F32), "f64": (abi.F64, abi.F64), "f32_under_f64": (abi.F32, abi.F64)}   # (leaves, nodes)


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- GPU tests --------------------------------------------------------------------------------------------------------------
def tf(flt):
    import torch
    return torch.float32 if flt == abi.F32 else torch.float64


def build(tris, leaf_flt=abi.F32, node_flt=None, idx=abi.I32, leaf_kind=abi.BBOX, node_kind=abi.BBOX, skin=None, built_level=1):
    """-> (the BVH over the triangles' volumes, the triangles on the device)"""
    import implicitbvh_amd as ibvh
    from test_gpu_parity import cuda, make_options
    node_flt = leaf_flt if node_flt is None else node_flt
    types = abi.make_types(leaf_kind, leaf_flt, node_kind, node_flt, index_type=idx)
    tdev = cuda(tris.astype(NP_F[leaf_flt]))
    token = ibvh.BBox if leaf_kind == abi.BBOX else ibvh.BSphere
    vols = ibvh.bounding_volumes_from_triangles(tdev, token(tf(leaf_flt)))
    if skin is not None:
        vols[:, :3] -= skin
        vols[:, 3:] += skin
    ntoken = ibvh.BBox if node_kind == abi.BBOX else ibvh.BSphere
    return ibvh.BVH(vols, ntoken(tf(node_flt)), built_level=built_level, options=make_options(types)), tdev


def assert_one_kernel(call, kernel, what=None):
    """one call() is exactly this one kernel of the library, and its launch profiler counted 1"""
    import torch
    from test_gpu_rays_binned import _kernels_of
    torch.cuda.synchronize()
    count = C.c_int64(-1)

    def run():
        call()
        torch.cuda.synchronize()
        lib.call("ibvh_profile_count", C.byref(count))
    names = _kernels_of(run)
    assert names == {kernel} and count.value == 1, (what, names, count.value)


# ---- the list queries: numpy only -----------------------------------------------------------------------------------------------
# An output column: the checker's field, the Python result's, "index" / "float" (the BVH's types) or "uint8", the shape of a row,
# and what the tests prefill it with so that 'not written' is visible.  A list query: its C entry point, its one kernel, the
# name — in the checker (0-based) and the Python result (1-based) — of the column that says whose list a row is in, its two
# modes, and letter -> Column in the entry point's order of outputs (the index first).
Column = collections.namedtuple("Column", "checker result dtype shape sentinel")
ListQuery = collections.namedtuple("ListQuery", "entry kernel owner count write columns")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def in_leaf_order(bf, leaf_order, owner, fields):
    """`bf` with every owner's list put in another leaf order, for a leaf_order that names every triangle at most once: the
    same contacts, re-sorted (what brute_force(..., leaf_order) gives, without evaluating again).  fields: the per-contact
    fields besides `owner` and index; whatever else `bf` holds is per item and stays."""
    order = np.asarray(leaf_order).astype(np.int64)
    assert len(np.unique(order)) == len(order)
    rank = np.full(max(int(order.max(initial=0)), int(bf.index.max(initial=0))) + 1, -1, np.int64)
    rank[order[order >= 0]] = np.flatnonzero(order >= 0)
    assert (rank[bf.index] >= 0).all()
    perm = np.lexsort((rank[bf.index], getattr(bf, owner)))
    out = type(bf)()
    vars(out).update(vars(bf))
    for name in (owner, "index") + tuple(fields):
        setattr(out, name, getattr(bf, name)[perm])
    return out


def same(query, got, exp, what=None, outs=None):
    """what two_passes() returned is the checker's `exp`: both statuses, the counts, the total, every column asked for bit
    for bit, and every other column untouched"""
    outs = "".join(query.columns) if outs is None else outs
    assert got["status_count"] == 0 and got["status"] == 0, what
    n, m = len(exp.counts), len(exp.index)
    assert (got["counts"][:n] == exp.counts).all() and got["total"] == m, what
    for k, col in query.columns.items():
        if k in outs:
            assert bits(got[k][:m]) == bits(getattr(exp, col.checker).astype(got[k].dtype)), (what, k)
        else:
            assert (got[k] == col.sentinel).all(), (what, k)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def assert_equal(query, got, exp, what, count_only=False):
    """a Python result `got` is the checker's `exp`: int64 offsets and counts; after count_only no column at all; otherwise
    every column's shape, the index by value, the other columns by dtype and bit for bit, and the 1-based owner column"""
    offsets, counts = _host(got.offsets), _host(got.counts)
    assert offsets.dtype == counts.dtype == np.int64, what
    assert (counts == exp.counts).all() and (offsets == exp.offsets).all(), what
    if count_only:
        assert all(getattr(got, col.result) is None for col in query.columns.values()) and getattr(got, query.owner) is None, what
        return
    m = len(exp.index)
    for k, col in query.columns.items():
        g, e = _host(getattr(got, col.result)), getattr(exp, col.checker)
        assert g.shape == (m,) + col.shape, (what, k)
        if col.dtype == "index":
            assert (g == e).all(), (what, k)
        else:
            assert g.dtype == e.dtype and bits(g) == bits(e), (what, k)
    assert (_host(getattr(got, query.owner)) == getattr(exp, query.owner) + 1).all(), what


# ---- the list queries: GPU tests ----------------------------------------------------------------------------------------------
def leaf_order(bvh):
    return bvh.leaves.index.cpu().numpy().astype(np.int64)


def stored_boxes(bvh, n):
    """(n, 6): the box stored in each triangle's leaf, by triangle — what a clause on the STORED box reads; a triangle no leaf
    names keeps zeros, a leaf that names none is left out"""
    vol = bvh.leaves.volume.cpu().numpy()
    boxes = np.zeros((n, 6), vol.dtype)
    order = leaf_order(bvh)
    ok = (order >= 1) & (order <= n)
    boxes[order[ok] - 1] = vol[ok]
    return boxes


def two_passes(query, bvh, tris, head, tail=(), num=None, num_triangles=None, flag=0, outs=None, offsets=None, capacity=None, rows=None):
    """count, scan on the host, write, straight through the C entry point -> dict: counts, the outputs (prefilled with their
    sentinel; `rows` of them, default the total), both flag words and both statuses.  head: the item arrays between
    num_triangles and the number of items (None = a NULL pointer), tail: the arguments between mode and counts."""
    import torch
    from implicitbvh_amd import api
    from test_gpu_parity import cuda
    outs = "".join(query.columns) if outs is None else outs
    items = len(head[0])
    n = items if num is None else num
    nt = len(tris) if num_triangles is None else num_triangles
    T = cuda(np.array(tris))   # (copies: the shared reference arrays are read-only)
    H = [None if h is None else cuda(np.array(h)) for h in head]
    f = getattr(lib.load(), query.entry)
    front = [C.byref(bvh.struct()), api._ptr(T), nt] + [api._ptr(h) for h in H] + [n]
    counts = torch.full((max(items, 1),), -7, dtype=torch.int64, device="cuda")
    fl = torch.full((2,), flag, dtype=torch.int32, device="cuda")
    out = {}
    out["status_count"] = f(*front, query.count, *tail, api._ptr(counts), None, 0, *[None] * len(query.columns),
                            C.c_void_p(fl.data_ptr()), api._stream())
    torch.cuda.synchronize()
    out["counts"] = counts.cpu().numpy()
    cn = out["counts"][:n] if out["status_count"] == 0 else np.zeros(0, np.int64)
    total = int(cn.sum())
    scan = (np.cumsum(cn) - cn).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
    out["offsets"], out["total"] = scan, total
    m = total if rows is None else rows
    dtypes = {"index": api._torch_index(bvh.types.index_type), "float": T.dtype, "uint8": torch.uint8}
    o = {k: torch.full((max(m, 1),) + col.shape, col.sentinel, dtype=dtypes[col.dtype], device="cuda") for k, col in query.columns.items()}
    Od = cuda(scan if len(scan) else np.zeros(1, np.int64))
    out["status"] = f(*front, query.write, *tail, None, C.c_void_p(Od.data_ptr()), m if capacity is None else capacity,
                      *[C.c_void_p(o[k].data_ptr()) if k in outs else None for k in query.columns], C.c_void_p(fl.data_ptr() + 4), api._stream())
    torch.cuda.synchronize()
    out.update({k: v.cpu().numpy() for k, v in o.items()})
    out["flag_count"], out["flag"] = (int(x) for x in fl.cpu().numpy())
    return out


def check_offsets_and_capacity(query, call, exp):
    """Offsets in a permuted order and the capacity guard.  call(**kw): two_passes() on the inputs `exp` is the checker's
    result of, in the BVH's leaf order; the caller has made sure that there are contacts enough."""
    n, total = len(exp.counts), len(exp.index)
    owner = getattr(exp, query.owner)
    cols = [(k, getattr(exp, col.checker), col.sentinel) for k, col in query.columns.items()]
    untouched = lambda got, where=slice(None): all((got[k][where] == sentinel).all() for k, _, sentinel in cols)
    # the lists laid out in another order of the items: each item's rows land where its offset says
    perm = np.random.default_rng(9).permutation(n)
    offs = np.empty(n, np.int64)
    offs[perm] = np.cumsum(exp.counts[perm]) - exp.counts[perm]
    assert (np.diff(offs) < 0).any()
    row = np.repeat(offs, exp.counts) + (np.arange(total) - np.repeat(exp.offsets[:-1], exp.counts))
    assert sorted(row.tolist()) == list(range(total))
    got = call(offsets=offs)
    assert got["status"] == 0 and got["flag"] == 0 and got["total"] == total
    for k, e, _ in cols:
        assert bits(got[k][row]) == bits(e.astype(got[k].dtype)), k
    # capacity one short of the total (the buffers hold the total): exactly the last row keeps its sentinel, bit 2 is raised
    short = call(capacity=total - 1, rows=total)
    assert short["status"] == 0 and short["flag"] == 4 and short["flag_count"] == 0
    for k, e, sentinel in cols:
        assert bits(short[k][:total - 1]) == bits(e[:total - 1].astype(short[k].dtype)) and (short[k][total - 1] == sentinel).all(), k
    # ... the same through permuted offsets: the rows >= capacity, wherever their items are
    cap = total - 37
    short = call(offsets=offs, capacity=cap, rows=total)
    keep = row < cap
    assert short["flag"] == 4 and (~keep).sum() == 37
    for k, e, _ in cols:
        assert bits(short[k][row[keep]]) == bits(e[keep].astype(short[k].dtype)), k
    assert untouched(short, slice(cap, None))
    # negative rows and rows far beyond are refused alike, never written
    busy = np.flatnonzero(exp.counts > 0)[:2]
    wild = offs.copy()
    wild[busy[0]], wild[busy[1]] = -10 ** 6, 2 ** 62
    bad = call(offsets=wild, rows=total)
    ok = ~np.isin(owner, busy)
    assert bad["status"] == 0 and bad["flag"] == 4 and (~ok).sum() >= 2
    assert (bad["i"][row[ok]] == exp.index[ok]).all() and (bad["i"][row[~ok]] == query.columns["i"].sentinel).all()
    # the guard is per ROW, not per item: with an offset of -1 an item's first contact (row -1) is refused and its later
    # ones land in rows 0, 1, ...; the other items are laid out behind them, so no row is written twice
    b = int(np.flatnonzero(exp.counts >= 3)[0])
    cb = int(exp.counts[b])
    edge = np.empty(n, np.int64)
    others = np.delete(np.arange(n), b)
    edge[others] = (cb - 1) + np.cumsum(exp.counts[others]) - exp.counts[others]
    edge[b] = -1
    erow = np.repeat(edge, exp.counts) + (np.arange(total) - np.repeat(exp.offsets[:-1], exp.counts))
    lost = erow < 0
    assert lost.sum() == 1 and owner[lost] == b and sorted(erow[~lost].tolist()) == list(range(total - 1))
    got = call(offsets=edge, capacity=total - 1, rows=total)
    assert got["status"] == 0 and got["flag"] == 4
    for k, e, sentinel in cols:
        assert bits(got[k][erow[~lost]]) == bits(e[~lost].astype(got[k].dtype)) and (got[k][total - 1] == sentinel).all(), k
    # capacity 0: nothing is written
    zero = call(capacity=0, rows=total)
    assert zero["status"] == 0 and zero["flag"] == 4 and untouched(zero)


def check_each_pass_is_one_kernel(query, bvh, tdev, python_call, head, tail, written):
    """python_call(count_only=...): the Python query in the given order; its count pass is ONE launch of the query's kernel, and
    so is the write pass straight through the C entry point — head, tail as for two_passes(), but device tensors —, which
    writes the `written` columns (letters) as the Python query did"""
    import torch
    from implicitbvh_amd import api
    assert_one_kernel(lambda: python_call(count_only=True), query.kernel)
    got = python_call(count_only=False)
    first = got.offsets[:-1].contiguous()
    mine = {k: torch.zeros_like(getattr(got, query.columns[k].result)) for k in written}
    call = lambda: lib.call(query.entry, C.byref(bvh.struct()), api._ptr(tdev), tdev.shape[0], *[api._ptr(h) for h in head],
                            got.counts.shape[0], query.write, *tail, None, api._ptr(first), got.index.shape[0],
                            *[api._ptr(mine.get(k)) for k in query.columns], None, api._stream())
    assert_one_kernel(call, query.kernel, "write")
    assert len(mine) >= 2 and all((mine[k] == getattr(got, query.columns[k].result)).all() for k in mine)


# ---- the first-hit queries ------------------------------------------------------------------------------------------------------
# A first-hit query: its C entry point (mesh: it takes the triangles and a flag word), its one kernel, the Python result's
# class, its two modes, and letter -> Column in the entry point's order of outputs: the closest outputs, the index first, then
# the any-hit byte (its `result` is None: the Python query returns the mask itself).
FirstHit = collections.namedtuple("FirstHit", "entry mesh kernel result closest any columns")
_hit = lambda checker, dtype="float", shape=(), sentinel=-7: Column(checker, checker, dtype, shape, sentinel)
CAST_RAYS = FirstHit("ibvh_cast_rays", True, "cast_walk_kernel", "RayCast", abi.CAST_CLOSEST, abi.CAST_ANY,
                     dict(i=_hit("index", "index"), t=_hit("t"), u=_hit("uv", shape=(2,)), o=Column("occluded", None, "uint8", (), 7)))
SWEEP_SPHERES = FirstHit("ibvh_sweep_spheres", True, "sweep_walk_kernel", "SphereSweep", abi.SWEEP_CLOSEST, abi.SWEEP_ANY,
                         dict(i=_hit("index", "index"), t=_hit("t"), q=_hit("point", shape=(3,)), g=_hit("feature", "uint8", sentinel=249),
                              o=Column("touched", None, "uint8", (), 7)))
CAST_SPHERES = FirstHit("ibvh_cast_spheres", False, "cast_walk_kernel", "SphereCast", abi.SPHERECAST_CLOSEST, abi.SPHERECAST_ANY,
                        dict(i=_hit("index", "index"), t=_hit("t"), a=Column("touched", None, "uint8", (), 9)))


def closest_letters(query):
    return "".join(query.columns)[:-1]


def first_hit_call(query, bvh, tris, head, tail=(), mode=None, outs=None, num=None, num_triangles=None, flag=0):
    """one launch straight through the C entry point -> dict: the outputs as numpy arrays (prefilled with their sentinel so
    that 'not written' is visible), the status and, a mesh query, the flag word.  head: the item arrays before the number of
    items, tail: those between it and the mode (None = a NULL pointer); floats go in the leaves' type, integers in the index
    type.  outs: the letters of the outputs handed over (default: the mode's own)."""
    import torch
    from implicitbvh_amd import api
    from test_gpu_parity import cuda
    mode = query.closest if mode is None else mode
    outs = (closest_letters(query) if mode == query.closest else list(query.columns)[-1]) if outs is None else outs
    n = len(head[0]) if num is None else num
    rows = max(len(head[0]), 1)
    np_t = {"f": NP_F[bvh.types.leaf_float], "i": NP_I[bvh.types.index_type], "u": NP_I[bvh.types.index_type]}
    dev = lambda x: None if x is None else cuda(np.ascontiguousarray(np.array(x)).astype(np_t[np.asarray(x).dtype.kind]))
    H, L = [dev(x) for x in head], [dev(x) for x in tail]
    dtypes = {"index": api._torch_index(bvh.types.index_type), "float": tf(bvh.types.leaf_float), "uint8": torch.uint8}
    o = {k: torch.full((rows,) + col.shape, col.sentinel, dtype=dtypes[col.dtype], device="cuda") for k, col in query.columns.items()}
    fl = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    front, back = [C.byref(bvh.struct())], [api._stream()]
    if query.mesh:
        T = cuda(np.array(tris))   # (copies: the shared reference arrays are read-only)
        front, back = front + [api._ptr(T), len(tris) if num_triangles is None else num_triangles], [api._ptr(fl)] + back
    st = getattr(lib.load(), query.entry)(*front, *[api._ptr(x) for x in H], n, *[api._ptr(x) for x in L], mode,
                                          *[api._ptr(o[k]) if k in outs else None for k in query.columns], *back)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["status"] = st
    if query.mesh:
        out["flag"] = int(fl.item())
    return out


def first_hit_same(query, got, exp, what=None, outs=None):
    """what first_hit_call() returned is the checker's `exp`: the status, every output asked for of the checker's dtype —
    index, feature and byte by value, the floats BIT FOR BIT — and every other output untouched"""
    outs = closest_letters(query) if outs is None else outs
    assert got["status"] == 0, what
    for k, col in query.columns.items():
        if k in outs:
            e = getattr(exp, col.checker)
            assert got[k].dtype == e.dtype, (what, k)
            same = bits(got[k]) == bits(e) if col.dtype == "float" else (got[k] == e).all()
            assert same, (what, k, got[k], e)
        else:
            assert (got[k] == col.sentinel).all(), (what, k, "not asked for, yet written")


def assert_closest(query, got, exp, what=None):
    """a Python result `got` is the checker's `exp`: the query's result class; the index by value; the floats by dtype, shape
    and BIT FOR BIT; a uint8 column by dtype and value; and .hit"""
    assert type(got).__name__ == query.result, what
    for k in closest_letters(query):
        col = query.columns[k]
        g, e = _host(getattr(got, col.result)), getattr(exp, col.checker)
        if col.dtype == "float":
            assert g.dtype == e.dtype and g.shape == e.shape and bits(g) == bits(e), (what, k, int((g != e).sum()))
        else:
            assert (col.dtype == "index" or g.dtype == np.uint8) and (g == e).all(), (what, k, int((g != e).sum()))
    assert (_host(got.hit) == (exp.index != 0)).all(), what


def assert_any(query, got, exp, what=None):
    """the Python query's any-hit result is a bool mask: the checker's byte"""
    import torch
    byte = getattr(exp, list(query.columns.values())[-1].checker)
    assert got.dtype == torch.bool and ((byte == 0) | (byte == 1)).all() and (_host(got) == (byte == 1)).all(), what


# ---- host tests -------------------------------------------------------------------------------------------------------------
def fake_bvh(leaf_kind=abi.BSPHERE, leaf_float=abi.F32, node_kind=abi.BBOX, node_float=abi.F32, idx=abi.I32, morton=abi.U32, n=5,
             built_level=1, leaves=64, nodes=64):
    """a hand-filled ibvh_bvh over fake non-NULL pointers: never dereferenced"""
    b = abi.Bvh()
    b.types = abi.make_types(leaf_kind, leaf_float, node_kind, node_float, idx, morton)
    lib.call("ibvh_tree_shape", n, C.byref(b.tree))
    b.built_level, b.leaves, b.nodes, b.skips = built_level, leaves, nodes, 64
    return b


def header_prototype(name):
    """include/ibvh.h declares `name` under ABI version 7, which the mirror and the library report too -> (the header's text,
    the same without comments, the declared arguments, the note on what bumped the version)"""
    raw = read("include", "ibvh.h")
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"ibvh_status\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/ibvh.h declares " + name
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert int(re.search(r"#define IBVH_ABI_VERSION (\d+)", hdr).group(1)) == 7 == abi.ABI_VERSION
    assert lib.load().ibvh_abi_version() == 7
    return raw, hdr, args, raw[raw.index("Bumped whenever"):raw.index("#define IBVH_ABI_VERSION")]


def julia_ccall(name, function):
    """ONE ccall wrapper of the Julia extension binds `name`, with the ctypes table's argument kinds; the extension's own
    `function` calls it and does not extend ImplicitBVH's namespace; the documents name the entry point -> the extension's text"""
    src = read("implicitbvh.jl_amd", "julia", "ImplicitBVHlibibvhExt.jl")
    m = re.search(r"\n(c_\w+)\([^)]*\) =\n\s*ccall\(\(:" + name + r", libibvh\), Cint,\s*\(([^)]*)\)", src)
    assert m, "one ccall wrapper binds " + name
    assert src.count(":" + name + ",") == 1
    jl = {"Ptr{Cvoid}": C.c_void_p, "Int64": C.c_int64, "Int32": C.c_int32, "Ref{IbvhBvh}": C.POINTER(abi.Bvh)}
    assert [jl[a.strip()] for a in m.group(2).split(",")] == lib.SIGNATURES[name]
    assert m.group(1) + "(" in src[src.index("function " + function + "("):]
    assert "function ImplicitBVH." + function not in src
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert name in read(doc), doc
    return src


def chain(rng, lo, up, dt, levels=5):
    """boxes above (lo, up) as a tree builds them: each the exact minimum / maximum with another random box"""
    out = []
    for _ in range(levels):
        centre, size = rng.random(lo.shape) * 4 - 2, rng.random(lo.shape) * 0.5
        other_lo, other_up = (centre - size).astype(dt), (centre + size).astype(dt)
        lo, up = np.where(other_lo < lo, other_lo, lo), np.where(other_up > up, other_up, up)
        out.append((lo, up))
    return out


BANNED = ("hipLaunchKernelGGL", "<<<", "atomic", "hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize",
          "__shared__", "hipMalloc")
# what only the shared front end spells: the rules, the layout, the grid and the triangle gather
FRONT_END = ("combo_ok", "box_nodes_hold_leaves", "tree_ok", "layout_of", "tree_dev", "grid_blocks", "__builtin_memcpy")


def _body(text, start):
    text = text[text.index(start):]
    return text[:text.index("\n}\n")]


# the list queries' protocol, which only the shared header spells: the pass as a type, the row's capacity guard and why it
# is safe, the two-pass argument rule
PROTOCOL = ("std::true_type{}", "std::false_type{}", "row < (uint64_t)capacity", "a negative row is a huge one",
            "wraps, never overflows", "mode == IBVH_SPHERES_WRITE ? offsets && any_output : mode == IBVH_SPHERES_COUNT && counts")
# ... and the unit's use of it, once each
PROTOCOL_USES = ("pointwalk::first_row<WRITE>(offsets, item)", "pointwalk::contact<WRITE>(next, capacity, over, [&](uint64_t row) {",
                 "pointwalk::store_count<WRITE>(counts, item, next)", "pointwalk::passes_ok(mode, counts, offsets, ",
                 "pointwalk::dispatch_box_types_and_bool(bvh->types, mode == ", "raise_flag(flag, 4u)")


# the first-hit queries' protocol, which only csrc/ibvh_firsthit.hpp spells: the limit's two statements and why a NaN stays one,
# how a candidate enters the answer, the two limits of the walk, the common stores, the mode / outputs rule, the one pair
FIRST_HIT = ("const T given = t_max ? t_max[item] : std::numeric_limits<T>::infinity();",
             "return given > std::numeric_limits<T>::max() ? std::numeric_limits<T>::max() : given;", "a NaN limit stays NaN and admits nothing",
             "a.touched |= ts <= a.L;", "} else if (pointwalk::wins(ts, index, a.best, a.best_index)) {", "keep();",
             "[&]() { return a.touched ? -inf : L; }", "[&]() { return a.best; }", "out_any[item] = a.touched ? 1 : 0;",
             "const bool hit = a.best_index != 0;", "if (out_index) out_index[item] = a.best_index;",
             "if (out_t) out_t[item] = hit ? a.best : std::numeric_limits<T>::infinity();",
             "return mode == IBVH_CAST_ANY ? any_output && !closest_outputs : mode == IBVH_CAST_CLOSEST && !any_output && closest_outputs;",
             "static_assert(IBVH_CAST_CLOSEST == 0 && IBVH_CAST_ANY == 1 && IBVH_SWEEP_CLOSEST == 0 && IBVH_SWEEP_ANY == 1,",
             "static_assert(IBVH_SPHERECAST_CLOSEST == 0 && IBVH_SPHERECAST_ANY == 1,")
# ... and the unit's use of it, once each
FIRST_HIT_USES = ("const T L = firsthit::limit(t_max, item);", "firsthit::Answer<T, I> answer(L);", "firsthit::offer<ANY>(answer, ts, index, ",
                  "firsthit::store<ANY>(answer, item, out_index, out_t, out_", "if (!firsthit::outputs_ok(mode, ")


def first_hit_unit(src, leaf="BBox<T>"):
    """The unit `src` answers with the closest or any hit through csrc/ibvh_firsthit.hpp: it includes it (and through it the
    shared walk), uses each piece once — the limit, the answer, the offer, the ONE walk call for both modes over `leaf`
    leaves, the common stores, the mode / outputs rule ahead of everything but the entry's own counts — and spells none of
    the protocol, the tie rule's call included -> the header's text"""
    fh = read("implicitbvh.jl_amd", "csrc", "ibvh_firsthit.hpp")
    assert re.search(r'^#include "ibvh_firsthit.hpp"$', src, flags=re.M) and re.search(r'^#include "ibvh_pointwalk.hpp"$', fh, flags=re.M)
    for use in FIRST_HIT_USES + ("firsthit::walk<ANY, " + leaf + ", TN>(tree, built_level, leaves, lay, nodes, answer, ",):
        assert src.count(use) == 1, use
    for text in FIRST_HIT:
        assert text not in src and fh.count(text) == 1, text
    for text in ("pointwalk::walk<", "wins(", "given", "-inf", "hit ?", "_CLOSEST"):
        assert text not in src, text
    assert fh.count("pointwalk::walk<VL, TN>(tree, built_level, leaves, lay, nodes, bound, ") == fh.count("pointwalk::walk<") == 2
    assert src.index("return IBVH_ERR_INVALID_ARG;") < src.index("firsthit::outputs_ok(") < src.index("const bool any = mode == ") < src.index("pointwalk::prepare(")
    for banned in BANNED + ("fma",):
        assert banned not in fh, banned
    return fh


def pair_routine(src):
    """The unit `src` answers with the closest pair through csrc/ibvh_pairwalk.hpp, once: the routine walks twice — first from
    the seed point on the shared point-box bound, which seeds the limit of the second —, applies the shared tie rule once and
    stores the five outputs; its comment states what the loss-free seed asks of the caller -> the header's text"""
    pw = read("implicitbvh.jl_amd", "csrc", "ibvh_pairwalk.hpp")
    assert re.search(r'^#include "ibvh_pairwalk.hpp"$', src, flags=re.M)
    assert src.count("pairwalk::closest_pair<I>(tree, built_level, leaves, lay, nodes, nan, ") == src.count("pairwalk::closest_pair") == 1
    assert src.count("max_d2, box, gather, pair, best);") == 1
    assert src.count("pairwalk::store_pair(item, best_index, best, out_index, out_d2, ") == src.count("pairwalk::store_pair") == 1
    for text in ("seed", "best.d2", "closest_on_triangle(K.v", "box_bound", "wins(", "infinity()", "hit ?"):
        assert text not in src, text
    assert pw.count("pointwalk::walk<") == 2 and pw.count("pointwalk::wins(r.d2, index, best.d2, best_index)") == 1
    assert pw.count("pointwalk::box_bound(lo, up, seed_point)") == 1 and pw.count("pointtri::closest_on_triangle(K.v, seed_point, x, region)") == 1
    assert pw.index("[&]() { return seed; }") < pw.index("best.d2 = seed;") < pw.index("[&]() { return best.d2; }")
    assert pw.count("seed = d2 < seed ? d2 : seed;") == 1 and pw.count("best.put(max_d2, zero, zero, 0);") == 1
    assert pw.count("if (hopeless) return best_index;") == 1 and pw.index("if (hopeless)") < pw.index("pointwalk::walk<")
    for line in ("if (out_index) out_index[item] = best_index;", "if (out_d2) out_d2[item] = hit ? best.d2 : std::numeric_limits<T>::infinity();",
                 "if (out_xq) out_xq[3 * item + k] = hit ? best.xq[k] : T(0);", "if (out_xk) out_xk[3 * item + k] = hit ? best.xk[k] : T(0);",
                 "if (out_kind) out_kind[item] = hit ? (uint8_t)best.kind : (uint8_t)0;", "const bool hit = best_index != 0;"):
        assert pw.count(line) == 1, line
    flat = " ".join(pw.replace("//", " ").split())
    for phrase in ("THE CALLER'S OBLIGATION: seed_point is the first point candidate 0 of evaluate() is evaluated from",
                   "IS candidate 0 of the pair (item, F), bit for bit", "nothing beyond it can win or tie", "F itself is still reached"):
        assert phrase in flat, phrase
    for banned in BANNED + ("fma", "__shared__"):
        assert banned not in pw, banned
    return pw


def query_unit(unit, kernel, walks=1, mesh=True, own_gather=False, lists=False, any_mode=False, pair=False):
    """The source-text facts about a query's translation unit and the header it shares with the other ten -> the unit's
    text.  The Makefile builds it; its ONE launch — of `kernel`, on the shared grid and block size — goes through the profiling
    wrapper and is checked; it calls the shared walk (`walks` times), the shared prologue once and, a mesh query, the shared
    gather (own_gather: spells its statements out once, with the reason), dispatch and raise_flag; it spells none of BANNED and
    none of FRONT_END itself.  A query with an any-hit mode (any_mode) dispatches on it through the shared four-tag dispatch and
    takes the closest / any-hit protocol, its two walks included, from csrc/ibvh_firsthit.hpp (first_hit_unit).  A
    list query (lists) dispatches on the pass through the same and uses each piece of the shared count / write
    protocol once, which the header defines once and the unit does not spell.  The header defines each shared piece once, refuses in the documented order and dispatches three
    (T, TN) pairs per index type."""
    mk = read("implicitbvh.jl_amd", "csrc", "Makefile")
    assert unit in mk[mk.index("SRCS"):mk.index("OBJS")]
    src = read("implicitbvh.jl_amd", "csrc", unit)
    header = read("implicitbvh.jl_amd", "csrc", "ibvh_pointwalk.hpp")
    assert re.findall(r"IBVH_LAUNCH\(\((\w+::\w+)<", src) == [kernel] and src.count("IBVH_LAUNCH(") == 1, "ONE launch, through the profiling wrapper"
    assert src.count("IBVH_LAUNCH_CHECK()") == 1
    assert "dim3(pre.blocks), dim3(pointwalk::kBlock)" in src and not re.search(r"\bkBlock\s*=", src)
    for text in (src, header):
        for banned in BANNED:
            assert banned not in text, banned
    if any_mode:  # a first-hit query: its walk under either mode's limit is the shared protocol's, and so is the include
        assert walks == 2 and first_hit_unit(src)
    else:
        assert re.search(r'^#include "ibvh_pointwalk.hpp"$', src, flags=re.M) and src.count("pointwalk::walk<") == (0 if pair else walks)
    if pair:  # a closest-pair query: its two walks, its tie rule and its five stores are the shared lane routine's
        assert walks == 2 and pair_routine(src)
    assert "__builtin_clzll" not in src and "void raise_flag(" not in src
    assert src.count("pointwalk::prepare(bvh, " + ("true" if mesh else "false") + ", ") == src.count("pointwalk::prepare(") == 1
    for piece in FRONT_END[:-1]:
        assert piece not in src, piece
    assert src.count("__builtin_memcpy") == int(own_gather) and src.count("pointwalk::leaf_triangle(") == int(mesh and not own_gather)
    if own_gather:  # the one exception says where the statements come from and why it keeps them
        why = src[src.index("only a leaf that passes gathers its triangle"):src.index("__builtin_memcpy")]
        assert "statements of pointwalk::leaf_triangle" in why and "(DESIGN.md)" in why
        assert "index >= 1 && (int64_t)index <= num_triangles" in why and "index >= 1 && (int64_t)index <= num_triangles" in header
    assert src.count("pointwalk::dispatch_box_types(") + src.count("pointwalk::dispatch_box_types_and_bool(") == src.count("raise_flag(flag, 2u)") == int(mesh)
    # a bool as a fourth tag: a list query's pass, the any-hit mode (any_mode) of the ray cast and the sweep; only the header
    # turns the bool into the two types
    assert src.count("pointwalk::dispatch_box_types_and_bool(") == int(lists or any_mode) and not (lists and any_mode)
    assert src.count("pointwalk::dispatch_box_types_and_bool(bvh->types, any, launch)") == int(any_mode)
    for text in PROTOCOL[:2]:
        assert text not in src and header.count(text) == 1, text
    if lists:
        for use in PROTOCOL_USES:
            assert src.count(use) == 1, use
        for text in PROTOCOL + ("over = true", "++row"):
            assert text not in src and header.count(text) == 1, text
        assert "if constexpr" not in src and "++next" not in src
        assert len(re.findall(r"if \(over && flag\) raise_flag\(flag, 4u\);\n\}", src)) == 1   # ... when the lane is done
    assert ("dispatch_index" in src) == (not mesh)
    # the header: each piece once
    for define in (r"inline bool box_nodes_hold_leaves\(", r"inline bool tree_ok\(", r"inline unsigned grid_blocks\(",
                   r"inline ibvh_status prepare\(", r"IBVH_D bool leaf_triangle\(", r"IBVH_D bool hopeless\(",
                   r"int dispatch_box_types\(", r"T radius_or_inf\(", r"__builtin_memcpy\(", r"IBVH_D uint64_t first_row\(",
                   r"IBVH_D void contact\(", r"IBVH_D void store_count\(", r"inline bool passes_ok\(",
                   r"int dispatch_box_types_and_bool\(", r"IBVH_D bool wins\(", r"static_assert\(IBVH_SPHERES_COUNT == 0 && IBVH_SPHERES_WRITE == 1 && IBVH_TRIS_COUNT == 0 && IBVH_TRIS_WRITE == 1,"):
        assert len(re.findall(define, header)) == 1, define
    prepare = _body(header, "inline ibvh_status prepare(")
    for call in FRONT_END[:-1]:
        assert prepare.count(call + "(") == 1, call
    # ... the order a call with several faults is refused in
    steps = [("!combo_ok(t)", "IBVH_ERR_UNSUPPORTED"), ("t.leaf_kind != IBVH_BBOX) || !box_nodes_hold_leaves(t)", "IBVH_ERR_UNSUPPORTED"),
             ("!tree_ok(bvh) || !pointers_ok", "IBVH_ERR_INVALID_ARG"), ("num == 0", "IBVH_OK"), ("!layout_of(", "IBVH_ERR_UNSUPPORTED")]
    found = re.findall(r"if \((.*)\) return (\w+);", prepare)
    assert len(found) == len(steps) and all(cond in f[0] and f[1] == status for f, (cond, status) in zip(found, steps)), found
    assert prepare.index("!layout_of(") < prepare.index("tree_dev(") < prepare.index("grid_blocks(")
    # ... three (T, TN) pairs under dispatch_index
    dispatch = _body(header, "int dispatch_box_types(")
    assert dispatch.count("dispatch_index(t.index_type") == 1
    assert re.findall(r"f\(Tag<(\w+)>\{\}, Tag<(\w+)>\{\}, it\)", dispatch) == [("double", "double"), ("float", "double"), ("float", "float")]
    return src


def check_mode_and_outputs(call, query, p, num, outputs, any_output):
    """The part of a first-hit query's argument matrix that is the closest / any-hit protocol's.  call(**changes) -> status,
    from a base that is the closest mode with the first of the closest outputs set and no items; p: a fake non-NULL pointer;
    num: the name of the number of items; outputs: the names of the closest outputs, any_output: that of the any-hit byte.
    Every refusal is asserted without items and with some: it comes before anything is read -> the any-hit base's changes."""
    any_ = {"mode": query.any, outputs[0]: None, any_output: p}
    assert call() == abi.OK and call(**any_) == abi.OK                     # no items: nothing to do
    for mask in range(1, 1 << len(outputs)):
        sub = {name: (p if mask >> j & 1 else None) for j, name in enumerate(outputs)}
        assert call(**sub) == abi.OK, sub                                  # closest: any non-empty subset of its outputs ...
        for n in (0, 5):
            assert call(**{any_output: p, num: n}, **sub) == abi.ERR_INVALID_ARG, sub      # ... never the byte
            assert call(**dict(any_, **{num: n}, **sub)) == abi.ERR_INVALID_ARG, sub       # any: the byte and nothing else
    for n in (0, 5):
        none = {outputs[0]: None, num: n}
        assert call(**none) == abi.ERR_INVALID_ARG                         # no output at all
        assert call(**{any_output: p}, **none) == abi.ERR_INVALID_ARG and call(mode=query.any, **none) == abi.ERR_INVALID_ARG
        for mode in (-1, 2, 7):
            assert call(mode=mode, **{num: n}) == abi.ERR_INVALID_ARG and call(mode=mode, **{any_output: p}, **none) == abi.ERR_INVALID_ARG
    return any_


def check_two_pass_arguments(call, count, write, p, num, outputs, needs, absent, fake):
    """The part of a list query's argument matrix that is the two-pass protocol's and the shared front end's.  call(base,
    **changes) -> status, for the bases `count` and `write` — dicts of the entry's arguments under the names bvh, tris, nt,
    mode, counts, offsets, cap and the query's own; no items, so every accepted call returns before a launch — p: a fake
    non-NULL pointer; num: the name of the number of items; outputs: the names of the output pointers (`write` sets the
    first); needs: the names of the item arrays a call with items cannot do without, absent: all of them, as NULL; fake: the
    query's fake_bvh."""
    ci = outputs[0]
    assert call(count) == abi.OK and call(write) == abi.OK             # no items: nothing to do
    assert call(count, offsets=p, cap=3, **{ci: p}) == abi.OK          # the count pass ignores the write pass's arguments
    assert call(count, counts=None) == abi.ERR_INVALID_ARG             # no counts in the count pass
    assert call(write, offsets=None) == abi.ERR_INVALID_ARG            # no offsets in the write pass
    assert call(write, **{ci: None}) == abi.ERR_INVALID_ARG            # no output in the write pass
    for one in outputs:                                                # ... any one output will do
        assert call(write, **{ci: None, one: p}) == abi.OK, one
    assert call(write, counts=p) == abi.OK and call(write, cap=0) == abi.OK
    for mode in (-1, 2, 7):
        assert call(count, mode=mode) == abi.ERR_INVALID_ARG and call(write, mode=mode) == abi.ERR_INVALID_ARG, mode
    for base in (count, write):
        for bad in ([dict(bvh=None), dict(nt=-1), {num: -1}, dict(cap=-1), dict(tris=None)] + [{num: 5, name: None} for name in needs]
                    + [dict(bvh=fake(leaves=None)), dict(bvh=fake(nodes=None)), dict(bvh=fake(built_level=0)), dict(bvh=fake(built_level=5))]):
            assert call(base, **bad) == abi.ERR_INVALID_ARG, bad
        assert call(base, tris=None, nt=0) == abi.OK and call(base, **absent) == abi.OK
        assert call(base, bvh=fake(n=1, nodes=None)) == abi.OK         # a one-leaf tree has no nodes
        broken = fake()
        broken.tree.virtual_leaves += 1                                # not an ImplicitTree's shape
        assert call(base, bvh=broken) == abi.ERR_INVALID_ARG
        # the accepted types: BBox leaves under BBox nodes of the same or a wider float type, any index type
        for good in (dict(), dict(leaf_float=abi.F64, node_float=abi.F64), dict(node_float=abi.F64), dict(idx=abi.I64)):
            assert call(base, bvh=fake(**good)) == abi.OK, good
        for bad in (dict(leaf_kind=abi.BSPHERE), dict(leaf_kind=abi.BSPHERE, node_kind=abi.BSPHERE), dict(node_kind=abi.BSPHERE),
                    dict(leaf_float=abi.F64, node_float=abi.F32), dict(leaf_float=2), dict(idx=2)):
            # (with items to process too: refused, never launched on the fake pointers)
            assert call(base, bvh=fake(**bad)) == abi.ERR_UNSUPPORTED and call(base, bvh=fake(**bad), **{num: 5}) == abi.ERR_UNSUPPORTED, bad
        # the entry's own checks come first, the types next, the tree and the pointers last
        assert call(base, bvh=fake(leaf_kind=abi.BSPHERE), mode=9) == abi.ERR_INVALID_ARG
        assert call(base, bvh=fake(leaf_kind=abi.BSPHERE, leaves=None), tris=None) == abi.ERR_UNSUPPORTED
