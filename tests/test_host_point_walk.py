"""The bounded walk of the point queries exists ONCE: csrc/ibvh_pointwalk.hpp holds the point-box bound, the descent, the
trail word and its pop, and the block size; ibvh_closest.hip and ibvh_nearest.hip include it and carry no copy of their own;
an edit to the header rebuilds the library.  No GPU."""
import os
import re

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicitbvh.jl_amd", "csrc")
HEADER = "ibvh_pointwalk.hpp"
QUERIES = ("ibvh_closest.hip", "ibvh_nearest.hip")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_both_queries_include_the_header():
    for name in QUERIES:
        assert re.search(r'^#include "' + re.escape(HEADER) + '"$', _read(name), flags=re.M), name
    assert "namespace pointwalk" in _read(HEADER)


def test_the_bound_and_the_trail_pop_are_defined_once_in_the_header():
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))]
    assert HEADER in sources and all(q in sources for q in QUERIES)
    assert [f for f in sources if re.search(r"\bbox_bound\s*\([^)]*\)\s*\{", _read(f))] == [HEADER]
    assert len(re.findall(r"\bbox_bound\s*\([^)]*\)\s*\{", _read(HEADER))) == 1
    assert "__builtin_clzll" in _read(HEADER)
    for name in QUERIES:
        assert "__builtin_clzll" not in _read(name), name


def test_neither_query_defines_its_own_block_size():
    assert len(re.findall(r"\bkBlock\s*=", _read(HEADER))) == 1
    for name in QUERIES:
        assert not re.search(r"\bkBlock\s*=", _read(name)), name


def test_an_edit_to_the_header_rebuilds_the_library():
    assert os.path.join(CSRC, HEADER) in entry.kernel_sources(ROOT)
