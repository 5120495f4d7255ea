"""The leaf-vs-tree scratch as a data format (csrc/ibvh_lvt_scratch.hpp), checked on the CPU: the two public size queries
against a recorded table, and the placement of every resident for arbitrary sizes against a restatement of the arithmetic
the launch code used before the layout had one description.  Host arithmetic only: no GPU."""
import ctypes as C
import itertools
import json
import os
import subprocess

import pytest

from implicitbvh_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "lvt_scratch_sizes.json")

N_ITEMS = [0, 1, 63, 64, 511, 512, 513, 2047, 2048, 50_000, 10**6, 7_201_012, 10**8]
CACHE_SLOTS = [0, 1, 8, 32, 64, 65, 1000]
KINDS = {abi.BSPHERE: "BSphere", abi.BBOX: "BBox"}
FLOATS = {abi.F32: "F32", abi.F64: "F64"}
INDICES = {abi.I32: "I32", abi.I64: "I64"}
# tests/test_host_cpu.py::test_ray_scratch_follows_the_binned_path_rule: its (leaves, rays), types and knob settings
RAY_CASES = [(7_201_012, 1_000_000), (7_201_012, 30_000), (7_201_012, 64), (7_201_012, 10_000_000), (30_000, 1_000_000),
             (3_200, 1_000), (3_200, 100_000), (250_000, 100_000), (250_000, 1_000_000), (2_000, 500), (1000, 5000)]
RAY_TYPES = {"f32": (abi.BSPHERE, abi.F32, abi.BBOX, abi.F32), "f64": (abi.BSPHERE, abi.F64, abi.BBOX, abi.F64),
             "two_floats": (abi.BSPHERE, abi.F64, abi.BBOX, abi.F32)}
RAY_KNOBS = [(binned, per_ray) for binned in (0, 1, 2) for per_ray in (0, 4)]
RAY_SLOTS = [0, 8]


def lvt_sizes():
    """{"BSphere/F32/BBox/F32/I32": [[bytes per cache_slots] per n_items]} over every leaf / node combination the library has"""
    out = {}
    for lk, lf, nk, nf, it in itertools.product(KINDS, FLOATS, KINDS, FLOATS, INDICES):
        t = abi.make_types(lk, lf, nk, nf, it)
        if not abi.combo_supported(t):
            continue
        need = C.c_size_t()
        rows = []
        for n in N_ITEMS:
            rows.append([])
            for slots in CACHE_SLOTS:
                lib.call("ibvh_lvt_scratch_bytes", C.byref(t), n, slots, C.byref(need))
                rows[-1].append(need.value)
        out["/".join((KINDS[lk], FLOATS[lf], KINDS[nk], FLOATS[nf], INDICES[it]))] = rows
    return out


def ray_sizes():
    """{"f32/I32/binned1/per_ray0": [[bytes per RAY_SLOTS] per RAY_CASES]}"""
    out = {}
    try:
        for (binned, per_ray), (tname, tt), it in itertools.product(RAY_KNOBS, RAY_TYPES.items(), INDICES):
            lib.set_tuning("rays_binned", binned)
            lib.set_tuning("rays_items_per_ray", per_ray)
            b = abi.Bvh()
            b.types = abi.make_types(*tt, it)
            b.built_level = 1
            need = C.c_size_t()
            rows = []
            for leaves, rays in RAY_CASES:
                lib.call("ibvh_tree_shape", leaves, C.byref(b.tree))
                rows.append([])
                for slots in RAY_SLOTS:
                    lib.call("ibvh_rays_scratch_bytes", C.byref(b), rays, slots, C.byref(need))
                    rows[-1].append(need.value)
            out[f"{tname}/{INDICES[it]}/binned{binned}/per_ray{per_ray}"] = rows
    finally:
        lib.set_tuning("rays_binned", 1)
        lib.set_tuning("rays_items_per_ray", 0)
    return out


def test_scratch_sizes_equal_the_recorded_table():
    """Callers memoise ibvh_lvt_scratch_bytes / ibvh_rays_scratch_bytes and pass one buffer to both calls of a pair, so the sizes
    are part of the contract: every value equals the table recorded from the library at commit 61e69ae (the last one that
    added the terms up by hand).  A change of the layout has to change the table on purpose."""
    table = json.load(open(TABLE))
    assert table["n_items"] == N_ITEMS and table["cache_slots"] == CACHE_SLOTS
    assert table["ray_cases"] == [list(c) for c in RAY_CASES] and table["ray_slots"] == RAY_SLOTS
    got = lvt_sizes()
    assert len(got) == 24 and sorted(got) == sorted(table["lvt"])
    for name, rows in got.items():
        assert rows == table["lvt"][name], name
    got = ray_sizes()
    assert len(got) == 36 and sorted(got) == sorted(table["rays"])
    for name, rows in got.items():
        assert rows == table["rays"][name], name
    # (the table is not trivial: the binned path's tables are in it, and leave when the knob says so)
    assert table["rays"]["f32/I32/binned1/per_ray0"][0][1] > 16 * 40 * 10**6 > table["rays"]["f32/I32/binned0/per_ray0"][0][1]


# ---- placements ------------------------------------------------------------------------------------------------------------
NONE, ROWS, BINS = 0, 1, 2


def _plan_lib():
    so = os.path.join(ROOT, "oracle", "liblvt_scratch_plan.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liblvt_scratch_plan.so"])
    l = C.CDLL(so)
    l.lvt_scratch_plan.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64)]
    l.lvt_scratch_size.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_uint64]
    l.lvt_scratch_size.restype = C.c_uint64
    return l


def _up(v, a):
    return -(-v // a) * a


def _scan_bytes(n):
    return _up((-(-max(n, 1) // 4096) + 9) * 8, 256)


def launch_arithmetic_61e69ae(n, pair_bytes, tail, bins_bytes, scratch_bytes):
    """run<MODE>() of csrc/ibvh_lvt.hip at commit 61e69ae, lines 53 - 82, 114 - 126, transcribed: (K, offsets of the contact cache,
    the index array, the rows, the ray bins; -1: absent), or None where it answered IBVH_ERR_SCRATCH.  `tail`: what the call
    was entitled to there (rows: SELF / PAIR, BBox nodes of one kind; bins: a ray batch whose cut lies at or below the start)."""
    scan = _scan_bytes(n)
    if scratch_bytes < scan:
        return None
    bins = bins_bytes if tail == BINS else 0
    if scratch_bytes < scan + bins + 256:
        bins = 0
    rows = qidx = 0
    if tail == ROWS:
        rows = -(-max(n, 1) // 512) * 512 * 4
        qidx = _up(n * (pair_bytes // 2), 256)
        if scratch_bytes < scan + rows + qidx + 256:
            qidx = 0
        if scratch_bytes < scan + rows + 256:
            rows = 0
        if not rows:
            qidx = 0
        rows += qidx
    tail_bytes = bins if bins else rows
    cache_room = scratch_bytes - (tail_bytes + 256 if tail_bytes else 0)
    tail_off = (scratch_bytes - tail_bytes) & ~255
    k = 0 if cache_room <= scan or n <= 0 else min(64, (cache_room - scan) // (n * pair_bytes))
    return (k, scan if k else -1, tail_off if qidx else -1, tail_off + qidx if rows else -1, tail_off if bins else -1)


def test_placements_equal_the_launch_arithmetic_they_replace():
    """For the documented sizes and for sizes a little and a lot below them (the steps at which the index array, the rows and the
    bins must disappear, and one byte either side of the alignment), scratch_plan() gives the K, the presence / absence and
    the offsets the launch code computed by hand; at a documented size everything asked for is there and nothing overlaps."""
    l = _plan_lib()
    out = (C.c_int64 * 5)()
    checked = 0
    for n, pair_bytes, slots in itertools.product(N_ITEMS[1:], (8, 16), (0, 1, 8, 64)):
        rows_bytes, qidx_bytes = -(-n // 512) * 2048, _up(n * (pair_bytes // 2), 256)
        for tail, bins_bytes in ((NONE, 0), (ROWS, 0), (BINS, 2048 + 256 * 7), (BINS, 40 * 16 * 10**6 + 2048)):
            for sized_rows in (False, True):  # (a ray scratch under BBox nodes has the rows' room too)
                if tail == ROWS and not sized_rows:
                    continue
                full = l.lvt_scratch_size(n, pair_bytes, slots, sized_rows, bins_bytes)
                if tail != BINS:  # the library's own query is this size
                    t = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX if sized_rows else abi.BSPHERE, abi.F32,
                                       abi.I32 if pair_bytes == 8 else abi.I64)
                    need = C.c_size_t()
                    lib.call("ibvh_lvt_scratch_bytes", C.byref(t), n, slots, C.byref(need))
                    assert need.value == full
                for less in (0, 1, 255, 256, 257, 511, 512, qidx_bytes, qidx_bytes + rows_bytes, qidx_bytes + rows_bytes + 512,
                             bins_bytes, bins_bytes + 512):
                    size = full - less
                    if size < 0:
                        continue
                    want = launch_arithmetic_61e69ae(n, pair_bytes, tail, bins_bytes, size)
                    ok = l.lvt_scratch_plan(n, pair_bytes, tail, bins_bytes, size, out)
                    assert (tuple(out) if ok else None) == want, (n, pair_bytes, slots, tail, bins_bytes, sized_rows, less)
                    checked += 1
                    if less == 0:
                        k, cache, index, rows, bins = want
                        assert k >= slots and (cache == _scan_bytes(n)) == (k > 0)
                        assert (index >= 0 and rows == index + qidx_bytes) == (tail == ROWS) and (bins >= 0) == (tail == BINS)
                        back = [o for o in (index, rows, bins) if o >= 0]
                        if back:
                            assert _scan_bytes(n) + k * n * pair_bytes <= min(back) and min(back) % 256 == 0
                            assert max(back) + (rows_bytes if tail == ROWS else bins_bytes) <= size
    assert checked > 5000
