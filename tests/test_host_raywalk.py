"""The pieces of the per-lane ray walk exist ONCE: csrc/ibvh_raywalk.hpp holds the ray load with its reciprocals, the cursor
with its pending-sibling pop, the child addressing at a global level and the two-children load; walker 3 (ibvh_lvt_rays.hip)
and the binned path (ibvh_lvt_raybins.hip) include it and carry no copy of their own; origin_outside lives in
ibvh_common.hpp alone; an edit to the header rebuilds the library.  No GPU."""
import os
import re

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicitbvh.jl_amd", "csrc")
HEADER = "ibvh_raywalk.hpp"
WALKERS = ("ibvh_lvt_rays.hip", "ibvh_lvt_raybins.hip")
SOURCES = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))]

# what the walk is made of, as it is written in C++ (whitespace aside)
PIECES = {
    "the reciprocal load": r"T\s*\(\s*1\s*\)\s*/\s*\w*d\s*\[",
    "the pending-sibling pop": r">>\s*\(\s*\w+\s*-\s*pl\s*\)\s*\)\s*\|\s*1u",
    "the inline level_skips": r"\(\s*2\s*\*\s*v\s*\)\s*-\s*\(uint32_t\)\s*__popcll\s*\(\s*v\s*\)",
    "the Two load": r"__builtin_memcpy\s*\(\s*&\w+\s*,\s*__builtin_assume_aligned\s*\(\s*np\s*,\s*8\s*\)\s*,\s*sizeof\s*\(\s*Two\b",
}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_both_ray_units_include_the_header():
    assert HEADER in SOURCES and all(w in SOURCES for w in WALKERS)
    for name in WALKERS:
        assert re.search(r'^#include "' + re.escape(HEADER) + '"$', _read(name), flags=re.M), name
    assert "namespace raywalk" in _read(HEADER)


def test_each_piece_of_the_walk_is_defined_once_in_the_header():
    for what, pattern in PIECES.items():
        assert len(re.findall(pattern, _read(HEADER))) == 1, what
        for name in WALKERS:
            assert not re.search(pattern, _read(name)), (what, name)


def test_the_pop_is_the_only_highest_bit_scan_of_the_walkers():
    """31 - clz(pend) belongs to the pop; the one other use is the tail's splitter of a parked walk's pending siblings into units"""
    clz = r"31\s*-\s*__builtin_clz\s*\(\s*(\w+)\s*\)"
    assert re.findall(clz, _read(HEADER)) == ["pend"]
    assert re.findall(clz, _read("ibvh_lvt_rays.hip")) == []
    assert sorted(re.findall(clz, _read("ibvh_lvt_raybins.hip"))) == ["h", "up_pend"]  # (h: the depth of a heap index while staging)


def test_the_struct_of_two_children_is_declared_once():
    assert [f for f in SOURCES if re.search(r"struct\s+Two\s*\{", _read(f))] == [HEADER]


def test_origin_outside_is_defined_only_in_the_common_header():
    definition = r"\borigin_outside\s*\([^)]*\)\s*\{"
    assert [f for f in SOURCES if re.search(definition, _read(f))] == ["ibvh_common.hpp"]
    assert len(re.findall(definition, _read("ibvh_common.hpp"))) == 2  # (sphere, box)


def test_an_edit_to_the_header_rebuilds_the_library():
    assert os.path.join(CSRC, HEADER) in entry.kernel_sources(ROOT)
