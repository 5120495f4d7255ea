"""Stream order, the part that needs no GPU: source-text pins over the kernels' host code and the Python mirror — every launch,
memset and copy names a stream variable, nothing copies synchronously, every entry point that takes a stream is handed torch's
current one — and the condition that keeps tests/test_gpu_streams.py from passing vacuously: for every case of its table
the CPU references of the real and the decoy inputs differ, evaluated here with the real checkers and the oracle."""
import ast
import glob
import os
import re

import pytest

import mesh_query_kit as kit
import stream_kit
from implicitbvh_amd import lib

CSRC = os.path.join(kit.ROOT, "implicitbvh.jl_amd", "csrc")
FORBIDDEN_STREAMS = ("0", "nullptr", "NULL", "hipStreamDefault", "hipStreamLegacy", "hipStreamPerThread", "")
# a variable, a member of one, or a cast of either to hipStream_t
STREAM_EXPRESSION = re.compile(r"^(\(hipStream_t\)\s*)?[A-Za-z_]\w*((\.|->)[A-Za-z_]\w*)*$")


def _sources():
    files = sorted(p for ext in ("*.hip", "*.hpp", "*.inc") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(files) > 30
    for path in files:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
        yield os.path.basename(path), re.sub(r"//[^\n]*", "", text)


def _arguments(text, start, close=")"):
    """the top-level arguments of the call whose opening bracket ends at `start`"""
    depth, args, cur, i = 0, [], [], start
    while True:
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            if depth == 0:
                assert c == close, text[start:i]
                return args + ["".join(cur).strip()]
            depth -= 1
        if c == "," and depth == 0:
            args.append("".join(cur).strip())
            cur = []
        else:
            cur.append(c)
        i += 1


def _stream_arguments():
    """(file, what, the stream expression) of every launch, asynchronous memset and asynchronous copy in csrc"""
    found = []
    for name, text in _sources():
        for m in re.finditer(r"\bIBVH_LAUNCH\(", text):
            if text[:m.start()].endswith("#define "):
                assert name == "ibvh_common.hpp"
                continue
            args = _arguments(text, m.end())
            assert len(args) >= 6, (name, args)
            found.append((name, "IBVH_LAUNCH", args[4]))
        for m in re.finditer(r"\bhipLaunchKernelGGL\(", text):
            args = _arguments(text, m.end())
            found.append((name, "hipLaunchKernelGGL", args[4]))
        for m in re.finditer(r"<<<", text):
            args = _arguments(text[:text.index(">>>", m.end())] + ")", m.end())   # grid, block, shared memory, stream
            assert len(args) == 4, (name, args)
            found.append((name, "<<< >>>", args[3]))
        for m in re.finditer(r"\bhipMem(cpy|set)Async\(", text):
            found.append((name, m.group(0)[:-1], _arguments(text, m.end())[-1]))
    return found


def test_every_launch_memset_and_copy_names_a_stream_variable():
    found = _stream_arguments()
    kinds = {what: sum(1 for f in found if f[1] == what) for what in ("IBVH_LAUNCH", "hipLaunchKernelGGL", "<<< >>>", "hipMemcpyAsync", "hipMemsetAsync")}
    print(kinds)
    # (the wrapper's own hipLaunchKernelGGL in ibvh_common.hpp forwards the macro's `st`; two raw launches and one <<< >>> in the
    # distributed driver)
    assert kinds["IBVH_LAUNCH"] >= 80 and kinds["hipMemcpyAsync"] >= 10 and kinds["hipMemsetAsync"] >= 15, kinds
    for name, what, stream in found:
        assert stream not in FORBIDDEN_STREAMS and STREAM_EXPRESSION.match(stream), (name, what, stream)
    # the names those expressions end in: a stream parameter or a field that was filled from one
    last = {re.split(r"\.|->|\)", s)[-1].strip() for _, _, s in found}
    assert last <= {"st", "stream"}, last


def test_no_synchronous_copy_and_symbol_copies_only_in_the_debug_counter_readers():
    symbol = []
    for name, text in _sources():
        assert not re.search(r"\bhipMemcpy\s*\(", text) and not re.search(r"\bhipMemset\s*\(", text), name
        assert not re.search(r"\bhipMemcpy(2D|3D|DtoH|HtoD|DtoD)\w*\s*\(", text), name
        assert "hipDeviceSynchronize" not in text, name
        symbol += [(name, m.group(1)) for m in re.finditer(r"\bhipMemcpy(ToSymbol|FromSymbol)\w*\s*\(", text)]
    assert sorted(symbol) == [("ibvh_lvt_queue_self.hip", "FromSymbol"), ("ibvh_lvt_queue_self.hip", "ToSymbol"), ("ibvh_msd.hip", "FromSymbol")]
    # ... each inside a reader of development counters, not a product entry point of include/ibvh.h
    header = kit.read("include", "ibvh.h")
    for unit, symbol_name in (("ibvh_lvt_queue_self.hip", "g_lvt_ticks"), ("ibvh_msd.hip", "g_stamps")):
        text = kit.read("implicitbvh.jl_amd", "csrc", unit)
        for m in re.finditer(r"hipMemcpy(To|From)Symbol\(", text):
            head = text[:m.start()]
            function = re.findall(r"\n(?:extern \"C\" )?\w[\w \*]*?\b(\w+)\s*\([^;{}]*\)\s*\{", head)[-1]
            assert symbol_name in text[m.start():m.start() + 200] and function not in header and function not in lib.SIGNATURES, (unit, function)


def _header_prototypes():
    raw = kit.read("include", "ibvh.h")
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    protos = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
              for m in re.finditer(r"\b(ibvh_\w+)\s*\(([^()]*)\)\s*;", hdr)}
    assert set(protos) == set(lib.SIGNATURES)
    for name, args in protos.items():
        assert len(args) == len(lib.SIGNATURES[name]) or args == ["void"], name
    return protos


def _takes_stream(protos):
    """the entry points whose prototype ends in a stream (and none that takes one anywhere else)"""
    takes = {name for name, args in protos.items() if args[-1] == "void *stream"}
    for name, args in protos.items():
        assert not any("stream" in a for a in args[:-1]), name
        assert (name in takes) == ("stream" in args[-1]), (name, args[-1])
        if name in takes:
            import ctypes
            assert lib.SIGNATURES[name][-1] is ctypes.c_void_p, name
    return takes


def _is_stream_call(node):
    return isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_stream" and not node.args


def test_the_mirror_hands_every_entry_point_that_takes_a_stream_the_current_one():
    protos = _header_prototypes()
    takes = _takes_stream(protos)
    assert len(takes) == 47 and "ibvh_build" in takes and "ibvh_tree_shape" not in takes
    tree = ast.parse(kit.read("implicitbvh.jl_amd", "api.py"))
    suffixes = ("_count", "_write", "_enqueue")
    # the names that reach an entry call through a variable: every "ibvh_..." string constant that is not itself the first
    # argument of lib.call — a family's prefix (ibvh_traverse_lvt + _count / _write / _enqueue), a result class's ENTRY, the
    # name a query hands to _mesh_query_call or _bfs_run.  All of them take a stream, so every call through a variable must
    # pass one.
    direct, sites = set(), []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        is_call = isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name) and f.value.id == "lib"
        # getattr(lib.load(), entry)(...)
        is_getattr = (isinstance(f, ast.Call) and isinstance(f.func, ast.Name) and f.func.id == "getattr" and len(f.args) == 2
                      and "lib.load()" in ast.unparse(f.args[0]))
        if is_call:
            name, args = node.args[0], node.args[1:]
        elif is_getattr:
            name, args = f.args[1], node.args
        else:
            continue
        if isinstance(name, ast.Constant):
            direct.add(id(name))
            assert name.value in lib.SIGNATURES, name.value
            if name.value not in takes:
                assert not any(_is_stream_call(a) for a in args), name.value
                continue
            what = name.value
        else:
            what = ast.unparse(name)   # a variable, or a prefix + a suffix
            if isinstance(name, ast.BinOp):
                assert isinstance(name.right, ast.Constant) and name.right.value in suffixes, what
        assert args and _is_stream_call(args[-1]) and not any(_is_stream_call(a) for a in args[:-1]), (what, node.lineno)
        if isinstance(name, ast.Constant):
            assert len(args) == len(protos[what]), (what, node.lineno)
        sites.append((node.lineno, what))
    indirect = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"ibvh_\w+", node.value) and id(node) not in direct:
            indirect.add(node.value)
    assert len(indirect) >= 15, indirect
    for name in sorted(indirect):
        family = [name + s for s in suffixes if name + s in lib.SIGNATURES]
        names = family if family else [name]
        assert (len(family) == 3 or name in lib.SIGNATURES) and all(n in takes for n in names), name
    print(len(sites), "entry calls pass _stream()")
    # (18 entry calls; the file mentions _stream() in 27 lines: its definition, the launch stream a pending total remembers and
    # compares, and comments make up the rest)
    assert len(sites) == 18, sites
    # _stream() itself is torch's current stream, by its raw handle where this torch has the accessor
    src = kit.read("implicitbvh.jl_amd", "api.py")
    body = src[src.index("def _stream():"):src.index("def _ptr(")]
    assert "_cuda_getCurrentRawStream" in body and "torch.cuda.current_stream().cuda_stream" in body


# ---- the cases of tests/test_gpu_streams.py are not vacuous -----------------------------------------------------------------------
def _cases():
    import test_gpu_streams
    return test_gpu_streams


def test_the_case_table_names_every_public_device_call():
    t = _cases()
    names = " ".join(t.CASE_NAMES)
    for call in ("BVH cold 1500", "BVH cold 3000", "BVH cold 20000", "BBox", "Float64", "Int64", "UInt64", "cache=", "wrapped in place",
                 "wrapped out of place", "refit(bvh, v)", "refit(bvh)", "bounding_volumes_from_triangles", "generate_spheres",
                 "traverse self LVT", "traverse self BFS", "traverse pair LVT", "traverse pair BFS", "traverse rays LVT", "traverse rays BFS",
                 "binned", "resolve_triangles", "closest_points", "nearest_leaves", "point_crossings", "cast_rays closest", "cast_rays any-hit",
                 "sweep_spheres", "cast_spheres", "triangle_distances", "segment_distances", "sphere_contacts", "triangle_contacts",
                 "capsule_contacts", "box_contacts", "cast_rays, triangles late", "sphere_contacts, triangles late"):
        assert call in names, call
    # the non-blocking table: every entry the issue lists, each used by a case or by the chains of part B
    used = {c.nonblocking for c in t.CASES if c.nonblocking}
    assert used | {"traverse / traverse_rays (LVT, cache= with a contact buffer)"} == set(t.NONBLOCKING)
    # every other case reads a flag word, a count or counters
    for c in t.CASES:
        if c.nonblocking is None:
            assert c.name.startswith(("traverse", "resolve", "closest", "point_cr", "cast_rays", "sweep", "triangle_", "segment_", "sphere_c",
                                      "capsule_", "box_")), c.name


@pytest.mark.parametrize("name", _cases().CASE_NAMES)
def test_real_and_decoy_references_differ(name):
    t = _cases()
    case = t.CASES[t.CASE_NAMES.index(name)]
    real, decoy = case.inputs("real"), case.inputs("decoy")
    assert len(real) == len(decoy) and all(r.shape == d.shape and r.dtype == d.dtype for r, d in zip(real, decoy))
    if not real:
        assert name == "generate_spheres"   # no input: judged by its gate and its oracle alone
        return
    assert any(r.tobytes() != d.tobytes() for r, d in zip(real, decoy))
    assert stream_kit.answers_differ(case.expected("real"), case.expected("decoy")), name


def test_the_sizing_rule_and_the_digest():
    import numpy as np
    assert stream_kit.delay_ms_for(0.0) == 40.0 and stream_kit.delay_ms_for(0.004) == 80.0 and stream_kit.delay_ms_for(3.0) == 1000.0
    a = np.arange(6, dtype=np.float32)
    assert not stream_kit.answers_differ((a, {"k": a}), (a.copy(), {"k": a.copy()}))
    assert stream_kit.answers_differ(a, a.reshape(2, 3)) and stream_kit.answers_differ(a, a.astype(np.float64)[:6] * 2)

    class Answer:
        def __init__(self, x):
            self.x = x
    assert stream_kit.answers_differ(Answer(a), Answer(a + 1)) and not stream_kit.answers_differ(Answer(a), Answer(a.copy()))
