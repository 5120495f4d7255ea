"""The steps of the build that must agree bit for bit are each written ONCE: the epsilon expansion of the extrema
(expand_bound, csrc/ibvh_common.hpp), the fold of the six running extrema through a workgroup (fold_extrema,
csrc/ibvh_build.hip) and the parent step of the bottom-up merge (parent_of, csrc/ibvh_aggregate.hip); the merge is a unit of
its own that the Makefile compiles and whose header rebuilds the library; what the refactor deleted stays deleted.  No GPU."""
import os
import re
import shutil
import time

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicitbvh.jl_amd", "csrc")
SOURCES = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))]
MERGE_UNIT = "ibvh_aggregate.hip"


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _bodies(text):
    """{function name: [its bodies]} of every function or kernel DEFINED in `text`: name(args) {...} at namespace scope, the
    body taken by counting braces (the sources have no brace inside a string or a comment); the arguments may hold one level of
    parentheses, as in `T (*s)[6]`, and the name the arguments of a specialisation"""
    out = {}
    for m in re.finditer(r"\b(\w+)(?:<\w+>)?\s*\((?:[^;{}()]|\([^;{}()]*\))*\)\s*\{", text):
        name = m.group(1)
        if name in ("if", "for", "while", "switch", "return", "sizeof") or text[:m.start()].count("{") - text[:m.start()].count("}") > 2:
            continue
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        out.setdefault(name, []).append(text[m.end():i - 1])
    return out


def _callers(pattern, skip=()):
    """[(file, function)] of every function body that holds `pattern`, the functions named in `skip` aside"""
    found = []
    for f in SOURCES:
        for name, bodies in _bodies(_read(f)).items():
            found += [(f, name) for b in bodies if name not in skip and re.search(pattern, b)]
    return found


def test_the_body_finder_sees_the_functions_it_is_asked_about():
    build, common, merge = _bodies(_read("ibvh_build.hip")), _bodies(_read("ibvh_common.hpp")), _bodies(_read(MERGE_UNIT))
    assert {"wave_min", "wave_max", "fold_extrema", "take_partials", "extrema_partial_kernel", "extrema_final_kernel",
            "encode_hist_kernel", "ibvh_build"} <= set(build)
    assert {"expand_bound", "key_bits", "key_bytes", "index_bytes", "tree_dev", "layout_of"} <= set(common)
    assert len(common["relative_precision"]) == 2  # (the two specialisations; the primary template is only declared)
    assert {"parent_of", "fold_up", "aggregate_kernel", "refit_kernel", "aggregate_top_kernel", "aggregate", "aggregate_tree",
            "ibvh_aggregate", "ibvh_refit"} <= set(merge)
    # nothing of a file lies outside the bodies and still holds the calls counted below
    for f in SOURCES:
        text, bodies = _read(f), _bodies(_read(f))
        for call in (r"relative_precision<\w+>\(\)(?!\s*\{)", r"\bwave_m(?:in|ax)\(\w+\[", r"\bmerge_to\((?!const\b)"):
            assert len(re.findall(call, text)) == sum(len(re.findall(call, b)) for bs in bodies.values() for b in bs), (f, call)


def test_the_epsilon_expansion_is_written_once():
    assert _callers(r"relative_precision<", skip=("relative_precision",)) == [("ibvh_common.hpp", "expand_bound")]
    users = {f for f in SOURCES if re.search(r"\bexpand_bound\(", _read(f))}
    assert users == {"ibvh_common.hpp", "ibvh_build.hip", "ibvh_dist.hip"}
    # extrema_final_kernel, encode_hist_kernel; expand_kernel, unpack_extrema_kernel
    assert sorted(n for f, n in _callers(r"\bexpand_bound\(")) == ["encode_hist_kernel", "expand_kernel", "extrema_final_kernel",
                                                                  "unpack_extrema_kernel"]


def test_the_workgroup_fold_of_the_extrema_is_written_once():
    assert _callers(r"\bwave_min\(", skip=("wave_min",)) == [("ibvh_build.hip", "fold_extrema")]
    assert _callers(r"\bwave_max\(", skip=("wave_max",)) == [("ibvh_build.hip", "fold_extrema")]
    assert sorted(n for f, n in _callers(r"\bfold_extrema\(")) == ["encode_hist_kernel", "extrema_final_kernel", "extrema_partial_kernel"]
    assert sorted(n for f, n in _callers(r"\btake_partials\(")) == ["encode_hist_kernel", "extrema_final_kernel"]
    assert len(re.findall(r"partials\[i \* 6", _read("ibvh_build.hip"))) == 2  # (a minimum and a maximum, in take_partials)
    # the encoder's rows are its own, sized for a 1024-thread block
    assert re.search(r"__shared__ T s_fold\[16\]\[6\];", _bodies(_read("ibvh_build.hip"))["encode_hist_kernel"][0])


def test_the_parent_step_of_the_merge_is_written_once():
    text = _read(MERGE_UNIT)
    assert len(re.findall(r"\bmerge_to\(", text)) == 1
    assert _callers(r"\bmerge_to\(", skip=("merge_to", "parent_of")) == [] and "merge_to(" in _bodies(text)["parent_of"][0]
    assert len(re.findall(r"\bconvert_to\(", text)) == 1 and "convert_to(" in _bodies(text)["parent_of"][0]
    # every kernel of the merge reaches it
    reach = {n for f, n in _callers(r"\bparent_of<") if f == MERGE_UNIT}
    assert reach == {"fold_up", "aggregate_kernel", "refit_kernel", "aggregate_top_kernel"}
    # ... and the build unit holds none of it any more
    build = _read("ibvh_build.hip")
    for gone in ("merge_to(", "aggregate_kernel", "refit_kernel", "aggregate_top_kernel", "fold_up", "RefitGather", "AGG_TPB"):
        assert gone not in build, gone
    assert re.search(r'^#include "ibvh_aggregate.hpp"$', build, flags=re.M) and "aggregate_tree(" in build


def test_what_was_deleted_stays_deleted():
    for f in SOURCES:
        text = _read(f)
        for gone in ("skips_kernel", "key_bits_of", "key_bytes_of", "morton_key_bits"):
            assert gone not in text, (f, gone)
        # the sizes of a key and of an index, and the device view of a tree, come from ibvh_common.hpp
        if f != "ibvh_common.hpp":
            assert not re.search(r"IBVH_U64 \? 8 : 4|IBVH_I32 \? 4 : 8", text), f
        if f not in ("ibvh_common.hpp", "ibvh_lvt.hip"):
            assert not re.search(r"TreeDev\s*\w*\{[^}]*\blevels\b", text), f


def test_the_makefile_compiles_the_merge_unit():
    mk = _read("Makefile")
    srcs = " ".join(l for l in mk.replace("\\\n", " ").splitlines() if l.startswith("SRCS"))
    assert MERGE_UNIT in srcs.split() and "ibvh_build.hip" in srcs.split()
    assert os.path.join(CSRC, MERGE_UNIT) in entry.kernel_sources(ROOT)


def test_an_edit_to_the_merge_header_makes_the_library_stale(tmp_path):
    root = tmp_path / "copy"
    (root / "implicitbvh.jl_amd" / "csrc").mkdir(parents=True)
    (root / "include").mkdir()
    for f in entry.kernel_sources():
        shutil.copy2(f, root / os.path.relpath(f, ROOT))
    so = root / "implicitbvh.jl_amd" / "libibvh.so"
    so.write_bytes(b"built")
    now = time.time()
    os.utime(so, (now, now))
    for f in entry.kernel_sources(str(root)):
        os.utime(f, (now - 100, now - 100))
    assert not entry.library_is_stale(str(root))
    header = root / "implicitbvh.jl_amd" / "csrc" / "ibvh_aggregate.hpp"
    header.write_bytes(header.read_bytes() + b"\n// edited\n")
    os.utime(header, (now + 100, now + 100))
    assert entry.library_is_stale(str(root))
