"""The status each stand-alone device piece of the multi-GPU build (ibvh_key_histogram, ibvh_dist_partition[_scratch_bytes],
ibvh_pack_records, ibvh_expand_extrema, ibvh_dist_pack_extrema, ibvh_dist_unpack_extrema) returns for a bad argument, one at a
time against an otherwise well-formed call, plus a few pairs that pin which check comes first.  Every case returns before the
library makes any HIP call, so the buffers are host memory the library never touches (what the calls compute is the GPU
suite's business: tests/test_gpu_dist_pieces.py).  No GPU."""
import ctypes as C

import pytest

import implicitbvh_amd as ibvh  # noqa: F401  (registers the package under its import name)
from implicitbvh_amd import abi, lib

OK, INVALID, UNSUPPORTED, OVERFLOW, SCRATCH = abi.OK, abi.ERR_INVALID_ARG, abi.ERR_UNSUPPORTED, abi.ERR_OVERFLOW, abi.ERR_SCRATCH
INT32_MAX = 2**31 - 1

# the parameters of each entry point, in order (include/ibvh.h)
PARAMS = {
    "key_histogram": "key_bytes keys n shift bits prefix_shift prefixes nprefix out stream",
    "dist_partition": "key_bytes keys n splitters nranks perm_out counts_out scratch scratch_bytes stream",
    "pack_records": "types volumes keys perm index_base n records_out stream",
    "expand_extrema": "flt extrema stream",
    "dist_pack_extrema": "flt extrema has_data rank nranks n_local vec_out stream",
    "dist_unpack_extrema": "flt vec extrema_out stream",
}
N = 1000
BIG = 1 << 40                        # a scratch_bytes no size check refuses
_buf = C.create_string_buffer(4096)  # stands in for every device buffer: never read or written by a call that fails its checks
BUF = C.cast(_buf, C.c_void_p)
PREFIXES = (C.c_uint64 * 16)(*range(16))
SPLITTERS = (C.c_uint64 * 256)(*range(1, 257))
TYPES = abi.make_types()                                                   # BSphere{Float32} leaves, Int32, UInt32
TYPES_I64 = abi.make_types(index_type=abi.I64, morton_type=abi.U64)
NO_COMBO = abi.make_types(leaf_kind=abi.BBOX, node_kind=abi.BSPHERE)       # no BSphere(::BBox): ibvh_layout_of refuses it
NO_INDEX = abi.Types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32, 7, abi.U32)  # an index type that does not exist


def partition_scratch(n):
    need = C.c_size_t()
    lib.call("ibvh_dist_partition_scratch_bytes", n, C.byref(need))
    return need.value


def _call(entry, **bad):
    """entry(good arguments, with `bad` replacing some of them) -> status"""
    good = {
        "key_histogram": dict(key_bytes=8, keys=BUF, n=N, shift=51, bits=12, prefix_shift=63, prefixes=PREFIXES, nprefix=2, out=BUF),
        "dist_partition": dict(key_bytes=8, keys=BUF, n=N, splitters=SPLITTERS, nranks=4, perm_out=BUF, counts_out=BUF, scratch=BUF,
                               scratch_bytes=BIG),
        "pack_records": dict(types=TYPES, volumes=BUF, keys=BUF, perm=None, index_base=0, n=N, records_out=BUF),
        "expand_extrema": dict(flt=abi.F32, extrema=BUF),
        "dist_pack_extrema": dict(flt=abi.F32, extrema=BUF, has_data=1, rank=0, nranks=4, n_local=N, vec_out=BUF),
        "dist_unpack_extrema": dict(flt=abi.F32, vec=BUF, extrema_out=BUF),
    }[entry]
    good["stream"] = None
    assert set(bad) <= set(good), (entry, bad)
    good.update(bad)
    args = [good[p] for p in PARAMS[entry].split()]
    args = [C.byref(a) if isinstance(a, abi.Types) else a for a in args]
    return getattr(lib.load(), "ibvh_" + entry)(*args)


# rows x 2^bits x 4 bytes must fit the 160 KB the kernel stages in LDS, and rows <= 15: the first refused row count per digit width
FIRST_REFUSED_ROWS = {1: 16, 6: 16, 11: 16, 12: 11}

CASES = [
    # ---- ibvh_key_histogram ------------------------------------------------------------------------------------------------
    ("key_histogram", dict(out=None), INVALID, "NULL out"),
    ("key_histogram", dict(keys=None), INVALID, "NULL keys, n > 0"),
    ("key_histogram", dict(n=-1), INVALID, "n < 0"),
    *[("key_histogram", dict(key_bytes=b), INVALID, f"key_bytes {b}") for b in (0, 2, 3, 16)],
    ("key_histogram", dict(bits=0), INVALID, "bits 0"),
    ("key_histogram", dict(bits=13), INVALID, "bits 13"),
    ("key_histogram", dict(bits=-1), INVALID, "bits -1"),
    ("key_histogram", dict(nprefix=-1), INVALID, "nprefix < 0"),
    ("key_histogram", dict(nprefix=16, bits=6), INVALID, "nprefix 16"),
    ("key_histogram", dict(nprefix=2, prefixes=None), INVALID, "NULL prefixes, nprefix > 0"),
    *[("key_histogram", dict(nprefix=r, bits=b, shift=0, prefix_shift=b), INVALID, f"{r} rows at {b} bits: beyond the LDS limit")
      for b, r in FIRST_REFUSED_ROWS.items()],
    ("key_histogram", dict(nprefix=15, bits=12), INVALID, "15 rows at 12 bits: beyond the LDS limit"),
    ("key_histogram", dict(shift=-1), INVALID, "shift < 0"),
    ("key_histogram", dict(shift=64), INVALID, "shift 64"),
    ("key_histogram", dict(shift=2**31 - 1), INVALID, "shift INT32_MAX"),
    ("key_histogram", dict(prefix_shift=-1), INVALID, "prefix_shift < 0, nprefix > 0"),
    ("key_histogram", dict(prefix_shift=-2**31), INVALID, "prefix_shift INT32_MIN, nprefix > 0"),
    # which check comes first: a bad argument is refused before n == 0 returns
    ("key_histogram", dict(n=0, shift=64), INVALID, "shift 64 before the empty return"),
    ("key_histogram", dict(n=0, nprefix=11), INVALID, "11 rows at 12 bits before the empty return"),
    # ---- ibvh_dist_partition -----------------------------------------------------------------------------------------------
    ("dist_partition", dict(n=-1), INVALID, "n < 0"),
    *[("dist_partition", dict(key_bytes=b), INVALID, f"key_bytes {b}") for b in (0, 2, 16)],
    ("dist_partition", dict(nranks=0), INVALID, "nranks 0"),
    ("dist_partition", dict(nranks=-1), INVALID, "nranks -1"),
    ("dist_partition", dict(nranks=257), UNSUPPORTED, "nranks 257"),
    ("dist_partition", dict(keys=None), INVALID, "NULL keys"),
    ("dist_partition", dict(perm_out=None), INVALID, "NULL perm_out"),
    ("dist_partition", dict(scratch=None), INVALID, "NULL scratch"),
    ("dist_partition", dict(splitters=None), INVALID, "NULL splitters, nranks > 1"),
    ("dist_partition", dict(scratch_bytes=partition_scratch(N) - 1), SCRATCH, "scratch one byte short"),
    ("dist_partition", dict(scratch_bytes=0), SCRATCH, "no scratch bytes"),
    # all of it with a counts_out: refused before counts_out is zeroed (a host buffer here: the memset would fail or crash)
    ("dist_partition", dict(nranks=257, keys=None), UNSUPPORTED, "nranks before NULL keys"),
    ("dist_partition", dict(keys=None, scratch_bytes=0), INVALID, "NULL keys before the scratch size"),
    ("dist_partition", dict(n=0, nranks=257, counts_out=None), UNSUPPORTED, "nranks 257 before the empty return"),
    ("dist_partition", dict(n=0, counts_out=None, keys=None, perm_out=None, scratch=None, scratch_bytes=0, splitters=None), OK,
     "n == 0 without counts_out: nothing needed"),
    # ---- ibvh_pack_records -------------------------------------------------------------------------------------------------
    ("pack_records", dict(types=None), INVALID, "NULL types"),
    ("pack_records", dict(n=-1), INVALID, "n < 0"),
    ("pack_records", dict(volumes=None), INVALID, "NULL volumes"),
    ("pack_records", dict(keys=None), INVALID, "NULL keys"),
    ("pack_records", dict(records_out=None), INVALID, "NULL records_out"),
    ("pack_records", dict(types=NO_COMBO), UNSUPPORTED, "BBox leaves, BSphere nodes"),
    ("pack_records", dict(types=NO_INDEX), UNSUPPORTED, "unknown index type"),
    ("pack_records", dict(index_base=INT32_MAX - N + 1), OVERFLOW, "I32: index_base + n == INT32_MAX + 1"),
    ("pack_records", dict(index_base=INT32_MAX), OVERFLOW, "I32: index_base == INT32_MAX"),
    ("pack_records", dict(index_base=2**40), OVERFLOW, "I32: index_base 2^40"),
    ("pack_records", dict(index_base=0, n=2**31), OVERFLOW, "I32: n == 2^31"),
    ("pack_records", dict(index_base=-1), INVALID, "I32: index_base < 0"),
    ("pack_records", dict(types=TYPES_I64, index_base=-1), INVALID, "I64: index_base < 0"),
    ("pack_records", dict(n=0, volumes=None, keys=None, records_out=None), OK, "n == 0: nothing needed"),
    ("pack_records", dict(n=0, index_base=-1), INVALID, "index_base < 0 before the empty return"),
    ("pack_records", dict(index_base=INT32_MAX, volumes=None), INVALID, "NULL volumes before the overflow"),
    ("pack_records", dict(index_base=INT32_MAX, types=NO_COMBO), UNSUPPORTED, "types before the overflow"),
    # ---- extrema -----------------------------------------------------------------------------------------------------------
    ("expand_extrema", dict(extrema=None), INVALID, "NULL extrema"),
    *[("expand_extrema", dict(flt=f), INVALID, f"flt {f}") for f in (-1, 2)],
    ("dist_pack_extrema", dict(vec_out=None), INVALID, "NULL vec_out"),
    ("dist_pack_extrema", dict(extrema=None), INVALID, "NULL extrema, has_data"),
    ("dist_pack_extrema", dict(nranks=0), INVALID, "nranks 0"),
    ("dist_pack_extrema", dict(nranks=1019, rank=0), INVALID, "nranks 1019"),
    ("dist_pack_extrema", dict(rank=-1), INVALID, "rank -1"),
    ("dist_pack_extrema", dict(rank=4), INVALID, "rank == nranks"),
    ("dist_pack_extrema", dict(n_local=-1), INVALID, "n_local < 0"),
    *[("dist_pack_extrema", dict(flt=f), INVALID, f"flt {f}") for f in (-1, 2)],
    ("dist_unpack_extrema", dict(vec=None), INVALID, "NULL vec"),
    ("dist_unpack_extrema", dict(extrema_out=None), INVALID, "NULL extrema_out"),
    *[("dist_unpack_extrema", dict(flt=f), INVALID, f"flt {f}") for f in (-1, 2)],
]


@pytest.mark.parametrize("entry, bad, status, what", CASES,
                         ids=[f"{e}-{w.replace(' ', '_')}-{i}" for i, (e, _, _, w) in enumerate(CASES)])
def test_entry_point_status(entry, bad, status, what):
    got = _call(entry, **bad)
    assert got == status, f"ibvh_{entry} ({what}): status {got}, expected {status}"


def test_partition_scratch_bytes_arguments():
    need = C.c_size_t(7)
    f = lib.load().ibvh_dist_partition_scratch_bytes
    assert f(-1, C.byref(need)) == INVALID and need.value == 7
    assert f(N, None) == INVALID
    assert f(0, C.byref(need)) == OK
    small = need.value
    assert f(1 << 22, C.byref(need)) == OK and need.value > small + 3 * 4 * (1 << 22)  # three n x uint32 slabs + the sort's own


def test_refused_calls_leave_the_plan_loop_a_batch_size():
    """What ibvh_dist_plan's batch loop relies on: at every digit width the splitter search uses (12 bits, and the narrower
    last level of 15-, 30- and 63-bit keys: 3 and 6 bits) one more row than the documented limit is refused, so the limit
    the header states — 10 rows at 12 bits, 15 below — is the one the check applies."""
    for bits, limit in ((12, 10), (11, 15), (6, 15), (3, 15), (1, 15)):
        assert _call("key_histogram", bits=bits, shift=0, prefix_shift=bits, nprefix=limit + 1) == INVALID, bits
        # (the accepted side launches a kernel: tests/test_gpu_dist_pieces.py)
