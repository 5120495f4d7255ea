"""The record sort's host plan (csrc/ibvh_msd_plan.hpp: digit, partition tile, finish workgroup, table counts, LDS budget, table
layout), checked on the CPU through its host-compiled view (oracle/msd_plan.cpp): every plan against a recorded table, the
accepted plans against the LDS, and the build's scratch size against the msd_rescue knob.  Host arithmetic only: no GPU.

tests/golden/msd_plans.json was recorded ONCE from make_plan / scratch_bytes of commit 95f00f0, the last one that planned inside
ibvh_msd.hip (a shim linked against that commit's library, outside the repository); nothing regenerates it."""
import ctypes as C
import itertools
import json
import os

import implicitbvh_amd as ibvh  # noqa: F401  (registers the package under its import name)
from implicitbvh_amd import abi, lib

import msd_plan_view as mv

TABLE = os.path.join(mv.ROOT, "tests", "golden", "msd_plans.json")

# 4,096: the smallest record sort; 2^21: the encoder's fold; 2^22: the large tile; 1e6, 1e7, 2e7: the benchmark sizes and the 8,192- /
# 16,384-record finish; both sides of the two finish rules' steps at 11 and 12 bits (average cell 5,120 = 5/8 of 8,192; 6,553 = 8/10
# of it), read literally and as the rule rounds (n >> bits); 2^32 - 65536: the first size the record sort refuses
SIZES = [4095, 4096, 4097, 2**21, 2**21 + 1, 2**22 - 1, 2**22, 10**6, 10**7]
for _x, _s in itertools.product((5120, 6553), (11, 12)):
    SIZES += [(_x << _s) - 1, _x << _s, ((_x + 1) << _s) - 1, (_x + 1) << _s]
SIZES += [2 * 10**7, 10**8, 2**32 - 65537, 2**32 - 65536]
MSD_AVG = [1, 1024, 2**20]
MORTONS = {"U16": (abi.U16, 15, 4), "U32": (abi.U32, 30, 4), "U64": (abi.U64, 63, 8)}  # type, key bits, key bytes


def leaf_sizes(morton):
    """every leaf_bytes ibvh_layout_of gives for the supported leaf kind / float / index combinations of one Morton type"""
    sizes = set()
    for kind, flt, idx in itertools.product((abi.BSPHERE, abi.BBOX), (abi.F32, abi.F64), (abi.I32, abi.I64)):
        t = abi.make_types(kind, flt, abi.BBOX, flt, idx, morton)
        lay = abi.Layout()
        if lib.load().ibvh_layout_of(C.byref(t), C.byref(lay)) == 0:
            sizes.add(int(lay.leaf_bytes))
    return sorted(sizes)


def rows():
    """(morton name, msd_avg, n, leaf_bytes, the recorded row or 0) over the whole table"""
    table = json.load(open(TABLE))
    for name, per_avg in table["plans"].items():
        for avg, per_n in zip(table["msd_avg"], per_avg):
            for n, groups in zip(table["n"], per_n):
                for leaf_bytes, row in ((lb, g[1]) for g in groups for lb in g[0]):
                    yield name, avg, n, leaf_bytes, row


def test_plans_equal_the_recorded_table():
    table = json.load(open(TABLE))
    assert table["n"] == SIZES and table["msd_avg"] == MSD_AVG and table["fields"] == mv.FIELDS + ["scratch_bytes"]
    assert sorted(table["mortons"]) == sorted(MORTONS) == sorted(table["plans"])
    for name, (morton, key_bits, key_bytes) in MORTONS.items():
        assert table["mortons"][name] == {"key_bits": key_bits, "key_bytes": key_bytes, "leaf_bytes": leaf_sizes(morton)}, name
        assert len(table["plans"][name]) == len(MSD_AVG) and all(len(per_n) == len(SIZES) for per_n in table["plans"][name])
        for per_n in table["plans"][name]:  # every leaf size has exactly one row per (msd_avg, n)
            assert all(sorted(lb for g in groups for lb in g[0]) == table["mortons"][name]["leaf_bytes"] for groups in per_n)
    checked = applies = 0
    for name, avg, n, leaf_bytes, want in rows():
        _, key_bits, key_bytes = MORTONS[name]
        p, total = mv.plan(n, key_bits, key_bytes, leaf_bytes, avg)
        got = 0 if p is None else [p[f] for f in mv.FIELDS] + [total + 4096]
        assert got == want, (name, avg, n, leaf_bytes)
        checked += 1
        applies += p is not None
    assert checked == (6 + 6 + 4) * len(MSD_AVG) * len(SIZES) and applies > checked * 3 // 4
    # (the table is not trivial: every row of both geometry tables is in it)
    seen_part = {(r[2], r[3]) for *_, r in rows() if r}
    seen_fin = {(MORTONS[name][2], r[4] * r[5], r[4], r[6]) for name, *_, r in rows() if r}
    assert seen_part == set(mv.partition_rows()) and seen_fin == set(mv.finish_rows())


def test_accepted_plans_fit_the_lds_and_their_tables_do_not_overlap():
    """What make_plan accepts, the launches can run: the geometries are rows of the tables the dispatchers expand, the partition's
    dynamic LDS — level 1 plain, level 1 equalised where sort_records would choose that, the extra levels' 8-bit digit — stays
    within the 160 KiB of a CU, and the tables lie one after the other, 256-byte aligned, inside the size the query reports."""
    part_rows, fin_rows = mv.partition_rows(), mv.finish_rows()
    assert part_rows == [(256, 4), (256, 8), (512, 8)] and len(fin_rows) == 8
    equalised = 0
    for name, avg, n, leaf_bytes, want in rows():
        _, key_bits, key_bytes = MORTONS[name]
        p, total = mv.plan(n, key_bits, key_bytes, leaf_bytes, avg)
        if p is None:
            continue
        geometry = (p["part_tpb"], p["part_ipt"])
        assert geometry in part_rows and mv.finish_row(p, key_bytes) in fin_rows, (name, avg, n, leaf_bytes)
        assert 6 <= p["bits"] <= 12 and p["shift"] == key_bits - p["bits"]
        lds = {eq: mv.view().msd_partition_lds(*geometry, leaf_bytes, p["bits"], eq) for eq in (0, 1)}
        # sort_records: equalised cells only where that stage fits; plain otherwise
        for eq in (0, 1) if lds[1] <= mv.MAX_LDS else (0,):
            assert lds[eq] <= mv.MAX_LDS, (name, avg, n, leaf_bytes, eq, lds)
        equalised += lds[1] <= mv.MAX_LDS
        assert lds[1] >= lds[0] >= geometry[0] * geometry[1] * leaf_bytes
        assert mv.view().msd_partition_lds(*geometry, leaf_bytes, 8, 0) <= mv.MAX_LDS
        offsets, total2 = mv.table_offsets(n, key_bits, key_bytes, leaf_bytes, avg)
        assert total2 == total and offsets[0] == 0 and offsets == sorted(offsets) and all(o % 256 == 0 for o in offsets)
        assert len(set(offsets)) == len(offsets) and offsets[-1] < total  # (no table is empty: at least one rescue slot)
        assert n * 2 <= offsets[11] - offsets[10] < n * 2 + 256  # the 2-byte cell of every leaf
    assert equalised > 500


def test_build_scratch_does_not_depend_on_the_rescue_knob():
    """Callers memoise ibvh_build_scratch_bytes per (types, n); tests flip msd_rescue between builds that share such a buffer.  The
    rescue workgroups' slots are carved either way: the knob only decides how many the finish launch asks for."""
    need = C.c_size_t()
    sizes = {}
    try:
        for rescue in (1, 0):
            lib.set_tuning("msd_rescue", rescue)
            for (morton, _, _), kind, idx, n in itertools.product(MORTONS.values(), (abi.BSPHERE, abi.BBOX), (abi.I32, abi.I64),
                                                                 (4096, 50_001, 10**6, 10**7, 2 * 10**7)):
                t = abi.make_types(kind, abi.F32, abi.BBOX, abi.F32, idx, morton)
                lib.call("ibvh_build_scratch_bytes", C.byref(t), n, C.byref(need))
                sizes.setdefault((morton, kind, idx, n), []).append(need.value)
    finally:
        lib.set_tuning("msd_rescue", 1)
    assert len(sizes) == 60 and all(a == b and a > 0 for a, b in sizes.values()), sizes
