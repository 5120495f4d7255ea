"""The record sort's host plan (csrc/ibvh_msd_plan.hpp) as tests see it: oracle/libmsd_plan.so, the header compiled for the host."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["bits", "shift", "part_tpb", "part_ipt", "fin_tpb", "fin_ipt", "resident", "num_tiles", "max_seg", "max_tiles2", "rescue_slots"]
MAX_LDS = 160 * 1024

_lib = None


def view():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "oracle", "libmsd_plan.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libmsd_plan.so"])
        l = C.CDLL(so)
        l.msd_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        l.msd_plan.restype = C.c_uint64
        l.msd_table_offsets.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        l.msd_table_offsets.restype = C.c_uint64
        l.msd_partition_lds.argtypes = [C.c_int] * 5
        l.msd_partition_lds.restype = C.c_uint64
        _lib = l
    return _lib


def plan(n, key_bits, key_bytes, leaf_bytes, msd_avg=1024):
    """(the plan's fields as a dict, or None where the record sort does not apply; the bytes of its tables)"""
    out = (C.c_int64 * len(FIELDS))()
    total = view().msd_plan(n, key_bits, key_bytes, leaf_bytes, msd_avg, out)
    if out[0] == 0:
        assert total == 0 and not any(out)
        return None, 0
    return dict(zip(FIELDS, out)), total


def table_offsets(n, key_bits, key_bytes, leaf_bytes, msd_avg=1024):
    out = (C.c_uint64 * view().msd_table_count())()
    total = view().msd_table_offsets(n, key_bits, key_bytes, leaf_bytes, msd_avg, out)
    return list(out), total


def partition_rows():
    out = (C.c_int * 64)()
    return [tuple(out[2 * i:2 * i + 2]) for i in range(view().msd_partition_rows(out))]


def finish_rows():
    """(key bytes, capacity, threads, resident)"""
    out = (C.c_int * 128)()
    return [tuple(out[4 * i:4 * i + 4]) for i in range(view().msd_finish_rows(out))]


def finish_row(p, key_bytes):
    return (key_bytes, p["fin_tpb"] * p["fin_ipt"], p["fin_tpb"], p["resident"])
