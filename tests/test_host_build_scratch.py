"""The scratch a build and a pair sort ask for, pinned byte for byte: ibvh_build_scratch_bytes carves the build's buffers
plus max(pair sort, record sort) for the sort region, and both sorts size theirs from their planners — so a change to the
host planning (csrc/ibvh_build.hip carve / choose_route, ibvh_sort.hip plan_pairs, ibvh_msd.hip make_plan) that moves a
tile count, a digit width or a threshold shows up here.  Host arithmetic only: no GPU.

tests/golden/build_scratch_sizes.json was recorded ONCE, with measure() below, from the library of the commit before the
build's planning was gathered into one route choice (the one that still had the `msd` knob and the gather kernel);
nothing regenerates it."""
import ctypes as C
import json
import os

import pytest

import implicitbvh_amd as ibvh  # noqa: F401  (registers the package under its import name)
from implicitbvh_amd import abi, lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_scratch_sizes.json")

# 1, 2: the smallest trees; 2047 | 2048: LSD passes | pair hybrid; 4095 | 4096: pair sort | record sort; 1e6: the benchmark;
# 2^22 - 1 | 2^22: the sorts' small | large tiles; 1e7, 2e7: the 8,192- and 16,384-record finish geometries
SIZES = [1, 2, 2047, 2048, 4095, 4096, 4097, 10**6, 2**22 - 1, 2**22, 10**7, 2 * 10**7]
MORTONS = {"U16": abi.U16, "U32": abi.U32, "U64": abi.U64}
LEAVES = {"BSphere{F32}": (abi.BSPHERE, abi.F32), "BBox{F32}": (abi.BBOX, abi.F32), "BBox{F64}": (abi.BBOX, abi.F64)}
INDICES = {"I32": abi.I32, "I64": abi.I64}


def measure():
    """{"sizes": SIZES, "build": {"<morton>/<leaf>/<index>": [bytes per size]}, "sort": {"<key bytes>": [bytes per size]}}"""
    need = C.c_size_t()
    build = {}
    for mname, morton in MORTONS.items():
        for lname, (kind, flt) in LEAVES.items():
            for iname, index in INDICES.items():
                types = abi.make_types(kind, flt, abi.BBOX, flt, index, morton)
                row = []
                for n in SIZES:
                    lib.call("ibvh_build_scratch_bytes", C.byref(types), n, C.byref(need))
                    row.append(need.value)
                build[f"{mname}/{lname}/{iname}"] = row
    sort = {}
    for key_bytes in (4, 8):
        row = []
        for n in SIZES:
            lib.call("ibvh_sort_scratch_bytes", key_bytes, n, C.byref(need))
            row.append(need.value)
        sort[str(key_bytes)] = row
    return {"sizes": SIZES, "build": build, "sort": sort}


def test_scratch_sizes_are_the_recorded_ones():
    want = json.load(open(GOLDEN))
    got = measure()
    assert want["sizes"] == SIZES
    assert sorted(want["build"]) == sorted(got["build"]) and len(got["build"]) == 18
    for name, row in got["build"].items():
        assert row == want["build"][name], name
    assert got["sort"] == want["sort"]


def test_the_msd_knob_is_gone_and_the_other_sort_knobs_are_not():
    """With `msd` gone the record sort takes every build of 4,096 leaves or more; the knobs tests and ibvh_sort_pairs use stay."""
    L = lib.load()
    v = C.c_int32()
    assert L.ibvh_get_tuning(b"msd", C.byref(v)) != 0
    assert L.ibvh_set_tuning(b"msd", 0) != 0
    for name, default in (("msd_avg", 1024), ("msd_equalize", 0), ("msd_rescue", 1), ("sort_lsd", 0), ("sort_msd_avg", 1536)):
        assert L.ibvh_get_tuning(name.encode(), C.byref(v)) == 0, name
        assert v.value == default, name
