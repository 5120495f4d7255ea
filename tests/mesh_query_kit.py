"""What the tests of the four point-walk queries — closest_points, point_crossings, cast_rays, nearest_leaves — share: the type
tables and meshes, the mesh-BVH builder and the one-kernel check of the GPU tests; the fake ibvh_bvh, the header / Julia
matchers and the source-text facts about the shared front end (csrc/ibvh_pointwalk.hpp) of the host tests.  Each query's
checker, hand-made meshes and reference builders stay with its own tests.  Importing this needs no GPU."""
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


BANNED = ("hipLaunchKernelGGL", "<<<", "atomic", "hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize",
          "__shared__", "hipMalloc")
# what only the shared front end spells: the rules, the layout, the grid and the triangle gather
FRONT_END = ("combo_ok", "box_nodes_hold_leaves", "tree_ok", "layout_of", "tree_dev", "grid_blocks", "__builtin_memcpy")


def _body(text, start):
    text = text[text.index(start):]
    return text[:text.index("\n}\n")]


def query_unit(unit, kernel, walks=1, mesh=True, own_gather=False):
    """The source-text facts about a query's translation unit and the header it shares with the other three -> the unit's
    text.  The Makefile builds it; its ONE launch — of `kernel`, on the shared grid and block size — goes through the profiling
    wrapper and is checked; it calls the shared walk (`walks` times), the shared prologue once and, a mesh query, the shared
    gather (own_gather: spells its statements out once, with the reason), dispatch and raise_flag; it spells none of BANNED and
    none of FRONT_END itself.  The header defines each shared piece once, refuses in the documented order and dispatches three
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
    assert re.search(r'^#include "ibvh_pointwalk.hpp"$', src, flags=re.M) and src.count("pointwalk::walk<") == walks
    assert "__builtin_clzll" not in src and "void raise_flag(" not in src
    assert src.count("pointwalk::prepare(bvh, " + ("true" if mesh else "false") + ", ") == src.count("pointwalk::prepare(") == 1
    for piece in FRONT_END[:-1]:
        assert piece not in src, piece
    assert src.count("__builtin_memcpy") == int(own_gather) and src.count("pointwalk::leaf_triangle(") == int(mesh and not own_gather)
    if own_gather:  # the one exception says where the statements come from and why it keeps them
        why = src[src.index("only a leaf that passes gathers its triangle"):src.index("__builtin_memcpy")]
        assert "statements of pointwalk::leaf_triangle" in why and "(DESIGN.md)" in why
        assert "index >= 1 && (int64_t)index <= num_triangles" in why and "index >= 1 && (int64_t)index <= num_triangles" in header
    assert src.count("pointwalk::dispatch_box_types(") == src.count("raise_flag(flag, 2u)") == int(mesh)
    assert ("dispatch_index" in src) == (not mesh)
    # the header: each piece once
    for define in (r"inline bool box_nodes_hold_leaves\(", r"inline bool tree_ok\(", r"inline unsigned grid_blocks\(",
                   r"inline ibvh_status prepare\(", r"IBVH_D bool leaf_triangle\(", r"IBVH_D bool hopeless\(",
                   r"int dispatch_box_types\(", r"T radius_or_inf\(", r"__builtin_memcpy\("):
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
