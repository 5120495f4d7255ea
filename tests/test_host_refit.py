"""ibvh_refit on the host side: the header declares it under ABI version 7, and the Julia extension's `refit!` binds it with the
ctypes signature and refuses, before any ccall, the BVHs the library does not instantiate (there is no generic refit to fall
back to: the reference has none).  No GPU."""
import os
import re

import implicitbvh_amd as ibvh
from implicitbvh_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _julia_refit():
    """The body of `function refit!(...)` in the Julia extension."""
    src = _read("implicitbvh.jl_amd", "julia", "ImplicitBVHlibibvhExt.jl")
    m = re.search(r"\nfunction refit!\((.*?)\) where \{[^}]*\}\n(.*?)\nend\n", src, re.S)
    assert m, "the Julia extension defines refit!"
    return src, m.group(1), m.group(2)


def test_header_declares_refit_at_abi_version_7():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "ibvh.h"), flags=re.S)
    assert re.search(r"ibvh_status\s+ibvh_refit\s*\(\s*const ibvh_bvh \*bvh,\s*const void \*volumes,\s*int64_t num_volumes,"
                     r"\s*void \*flag,\s*void \*stream\s*\)\s*;", hdr)
    assert int(re.search(r"#define IBVH_ABI_VERSION (\d+)", hdr).group(1)) == 7 == abi.ABI_VERSION
    assert hasattr(lib.load(), "ibvh_refit")
    assert lib.load().ibvh_abi_version() == 7
    assert "refit" in ibvh.__all__ and callable(ibvh.refit)


def test_julia_refit_calls_ibvh_refit_with_the_ctypes_signature():
    import ctypes as C
    src, _, body = _julia_refit()
    wrapper = re.search(r"\n(c_\w+)\([^)]*\) =\n\s*ccall\(\(:ibvh_refit, libibvh\), Cint,\s*\(([^)]*)\)", src)
    assert wrapper, "one ccall wrapper binds ibvh_refit"
    jl = {"Ptr{Cvoid}": C.c_void_p, "Int64": C.c_int64, "Ref{IbvhBvh}": C.POINTER(abi.Bvh)}
    assert [jl[a.strip()] for a in wrapper.group(2).split(",")] == lib.SIGNATURES["ibvh_refit"]
    assert wrapper.group(1) + "(" in body, "refit! goes through that wrapper"
    # not a method of ImplicitBVH: the count of ImplicitBVH.-qualified methods stays what the generic-fallback test pins
    assert "function ImplicitBVH.refit" not in src


def test_julia_refit_guards_unsupported_types_before_the_ccall():
    src, sig, body = _julia_refit()
    assert "bvh::RocBVH" in sig and "volumes::Union{Nothing, ROCVector}=nothing" in sig
    code = "\n".join(line.split("#")[0] for line in body.splitlines())
    desc = code.index("bvh_desc(bvh)")
    guard = re.search(r"isnothing\((\w+)\) && throw\(ArgumentError\(", code)
    assert guard and guard.start() > desc and re.search(r"(\w+) = bvh_desc\(bvh\)", code).group(1) == guard.group(1)
    assert guard.start() < code.index("c_refit(")
    # the volumes' element type and the index range are checked before the ccall as well
    assert code.index("ArgumentError(\"refit!: volumes") < code.index("c_refit(")
    assert code.index("outside 1:$m") < code.index("c_refit(")
