"""The six stand-alone device pieces of the multi-GPU build — ibvh_key_histogram, ibvh_dist_partition, ibvh_pack_records,
ibvh_expand_extrema, ibvh_dist_pack_extrema, ibvh_dist_unpack_extrema — each against a numpy reference of its own operation,
at the shapes include/ibvh.h allows and the driver's virtual-rank tests never reach (256 ranks, 15 prefixes, 12-bit digits,
either key width, every leaf layout), and the driver itself (ibvh_dist_plan / ibvh_dist_exchange) at world sizes whose
splitter refinement needs more histogram rows than one call takes.

Every expected value is integer arithmetic in numpy, or float arithmetic in the leaf float type; every comparison is exact.
Every output buffer carries guard words behind its end, which must survive the call."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, lib  # noqa: E402

U64_MAX = 2**64 - 1
INT32_MAX = 2**31 - 1
GUARD = 0x5A            # byte every output buffer is pre-filled with
KEY_NP = {4: np.uint32, 8: np.uint64}


def cuda(a):
    """numpy array -> device tensor of the same bytes (unsigned types travel as their signed twins)."""
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(twin) if twin else a).cuda()


def guarded(nbytes, extra=64):
    """A device byte buffer of nbytes + extra, all GUARD."""
    return torch.full((nbytes + extra,), GUARD, dtype=torch.uint8, device="cuda")


def host(t, dtype, count):
    """The first `count` elements of `dtype` of a device byte buffer, and whether everything behind them is still GUARD."""
    raw = t.cpu().numpy()
    nbytes = count * np.dtype(dtype).itemsize
    return raw[:nbytes].view(dtype).copy(), bool((raw[nbytes:] == GUARD).all())


def u64s(values):
    return (C.c_uint64 * max(len(values), 1))(*[int(v) for v in values])


# ---------------------------------------------------------------------------------------------
# ibvh_key_histogram
# ---------------------------------------------------------------------------------------------
def max_rows(bits):
    """Rows one call takes (include/ibvh.h): what fits 160 KB of LDS, at most 15."""
    return min(15, (160 * 1024) // (4 << bits))


def histogram_reference(keys, shift, bits, prefix_shift, prefixes):
    k = keys.astype(np.uint64)
    d = ((k >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    if len(prefixes) == 0:
        return np.bincount(d, minlength=1 << bits)[None, :]
    p = (k >> np.uint64(prefix_shift)) if prefix_shift < 64 else np.zeros(len(k), np.uint64)
    return np.stack([np.bincount(d[p == np.uint64(pre)], minlength=1 << bits) for pre in prefixes])


def histogram(keys_dev, key_bytes, n, shift, bits, prefix_shift, prefixes):
    """-> (status, rows x 2^bits counts, guard rows behind them intact)"""
    rows = max(len(prefixes), 1)
    out = guarded(rows * (4 << bits), extra=2 * (4 << bits))  # sentinel everywhere, two sentinel rows behind
    st = lib.load().ibvh_key_histogram(key_bytes, keys_dev.data_ptr() if keys_dev is not None else None, n, shift, bits, prefix_shift,
                                       u64s(prefixes) if len(prefixes) else None, len(prefixes), out.data_ptr(), None)
    torch.cuda.synchronize()
    got, intact = host(out, np.uint32, rows << bits)
    return st, got.reshape(rows, 1 << bits).astype(np.int64), intact


def check_histogram(keys, keys_dev, shift, bits, prefix_shift, prefixes, what=""):
    kb = keys.dtype.itemsize
    st, got, intact = histogram(keys_dev, kb, len(keys), shift, bits, prefix_shift, prefixes)
    where = f"{what} key_bytes={kb} n={len(keys)} shift={shift} bits={bits} prefix_shift={prefix_shift} nprefix={len(prefixes)}"
    assert st == abi.OK, where
    assert intact, "rows behind the histogram were written: " + where
    want = histogram_reference(keys, shift, bits, prefix_shift, prefixes)
    assert np.array_equal(got, want), where
    return got


def some_prefixes(rng, keys, prefix_shift, count):
    """`count` prefixes: ones that occur among the keys, one that matches no key, one listed twice (when there is room)."""
    if count == 0:
        return []
    k = keys.astype(np.uint64)
    present = np.unique(k >> np.uint64(prefix_shift)) if prefix_shift < 64 and len(k) else np.zeros(1, np.uint64)
    pick = [int(p) for p in rng.permutation(present)[:count]]
    absent = next(p for p in itertools.count(int(present.max()) + 1 if int(present.max()) < U64_MAX else 1) if p not in set(present.tolist()))
    if count >= 2:
        pick = pick[:count - 1] + [absent]
    if count >= 3:
        pick = pick[:count - 1]
        pick.insert(1, pick[0])  # a prefix listed twice
    while len(pick) < count:
        pick.append(absent + len(pick))
    return pick[:count]


HIST_SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 1024 * 4096 + 333]


@pytest.mark.parametrize("n", HIST_SIZES)
@pytest.mark.parametrize("key_bytes", [4, 8])
def test_key_histogram_sizes(key_bytes, n):
    """Every size class of the launch: nothing, one thread, one block (256) and its neighbours, one block's 16 passes (4096) and
    its neighbours, and 1,024 x 4,096 + 333 — past the 1,024-block cap, so the grid-stride loop runs — at every digit width
    with no prefix, one, two, and as many as one call takes (15; 10 at 12 bits), in the driver's arrangement
    (prefix_shift = shift + bits)."""
    rng = np.random.default_rng(1000 * key_bytes + n % 997)
    key_bits = 30 if key_bytes == 4 else 63
    keys = rng.integers(0, 2**key_bits, n, dtype=np.uint64).astype(KEY_NP[key_bytes])
    dev = cuda(keys) if n else None
    big = n > 100000
    for bits in (1, 3, 6, 12):
        shift = key_bits - 12 - bits  # a second-level digit: 4,096 possible prefixes above it
        counts = (0, max_rows(bits)) if big else (0, 1, 2, 10, max_rows(bits))
        for nprefix in counts:
            check_histogram(keys, dev, shift, bits, shift + bits, some_prefixes(rng, keys, shift + bits, nprefix))


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_key_histogram_shifts(key_bytes):
    """Every digit position the header allows: the bottom of the key, the driver's first level for 15-, 30- and 63-bit keys
    (key_bits - bits), bit 52, and 63 — the last amount a 64-bit shift takes.  Keys fill their whole word, so every shift sees
    set bits; 4-byte keys are widened, so a shift of 32 or more sees zeros.  prefix_shift = 64 means "every key has prefix 0"."""
    rng = np.random.default_rng(7 + key_bytes)
    n = 4097
    keys = rng.integers(0, 2**(8 * key_bytes), n, dtype=np.uint64, endpoint=False).astype(KEY_NP[key_bytes])
    dev = cuda(keys)
    for bits in (1, 3, 6, 12):
        for shift in sorted({0, 15 - bits, 30 - bits, 63 - bits, 31, 32, 52, 63}):
            ps = min(shift + bits, 64)
            for nprefix in (0, 1, 2, 10, max_rows(bits)):
                pre = some_prefixes(rng, keys, ps, nprefix)
                if ps == 64 and nprefix:
                    pre[0] = 0  # the one prefix every key has
                got = check_histogram(keys, dev, shift, bits, ps, pre)
                if ps == 64 and nprefix:
                    assert got[0].sum() == n and got[1:][np.array(pre[1:], dtype=np.uint64) != 0].sum() == 0
            # a prefix position unrelated to the digit's, and one past the key
            check_histogram(keys, dev, shift, bits, 8 * key_bytes - 4, list(range(max_rows(bits))))
            check_histogram(keys, dev, shift, bits, 100, [0, 1, 0])


def test_key_histogram_key_sets():
    """All keys equal (one counter takes every increment, 2^20 + 1 of them); 8-byte keys that differ only above bit 32; the
    maximum key of either width; prefixes that match no key (rows of zeros); a prefix listed twice — BOTH rows get the count
    (the kernel tests every row for every key), which is what include/ibvh.h documents."""
    rng = np.random.default_rng(11)
    n = (1 << 20) + 1
    for kb, value in ((4, 0x2AAAAAAA), (8, 0x5555555555555555), (4, 2**32 - 1), (8, U64_MAX), (4, 0), (8, 0)):
        keys = np.full(n, value, dtype=KEY_NP[kb])
        dev = cuda(keys)
        for bits, shift in ((12, 0), (12, 8 * kb - 12), (6, 13), (1, 8 * kb - 1)):
            got = check_histogram(keys, dev, shift, bits, 64, [])
            assert got[0, (value >> shift) & ((1 << bits) - 1)] == n
            pre = value >> (shift + bits) if shift + bits < 64 else 0
            got = check_histogram(keys, dev, shift, bits, min(shift + bits, 64), [pre, pre + 1, pre])
            assert got[0].sum() == n and got[1].sum() == 0 and got[2].sum() == n  # a duplicate prefix: both rows
    # 8-byte keys whose low words are all the same
    n = 70001
    keys = (rng.integers(0, 2**31, n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xDEADBEEF)
    dev = cuda(keys)
    for bits, shift in ((12, 51), (12, 39), (12, 32), (6, 30), (12, 20), (3, 0)):
        ps = shift + bits
        check_histogram(keys, dev, shift, bits, 64, [])
        check_histogram(keys, dev, shift, bits, ps, some_prefixes(rng, keys, ps, max_rows(bits)))
    # no prefix matches: every row zero
    got = check_histogram(keys, dev, 20, 12, 63, [1, 1, 1])
    assert got.sum() == 0


def test_key_histogram_largest_lds_configuration():
    """10 rows x 12 bits x 4 bytes = exactly 160 KB of dynamic LDS, the most include/ibvh.h allows one call: the launch must be
    accepted and count right, with 64-bit keys, at a size that fills every block's 16 passes and more than one block."""
    rng = np.random.default_rng(12)
    n = 300007
    keys = rng.integers(0, 2**63, n, dtype=np.uint64)
    dev = cuda(keys)
    assert max_rows(12) == 10
    pre = [int(p) for p in np.unique(keys >> np.uint64(60))[:8]] + [9, 3]  # eight that occur, one that cannot (> 7), one twice
    got = check_histogram(keys, dev, 48, 12, 60, pre, "full LDS")
    assert got[:8].sum() == n and got[8].sum() == 0 and np.array_equal(got[9], got[pre.index(3)])
    # the level the driver refines a 63-bit key at, with ten of its prefixes
    check_histogram(keys, dev, 39, 12, 51, some_prefixes(rng, keys, 51, 10), "full LDS, driver level")


def test_key_histogram_rows_beyond_one_call_are_refused_and_covered_in_batches():
    """11 rows at 12 bits (176 KB) do not fit one call: IBVH_ERR_INVALID_ARG, `out` untouched — and the same 11 prefixes
    counted the way ibvh_dist_plan does it, max_rows(bits) rows a call, give numpy's histogram.  Likewise 16 rows at 6 bits."""
    rng = np.random.default_rng(13)
    n = 50021
    keys = rng.integers(0, 2**63, n, dtype=np.uint64)
    dev = cuda(keys)
    for bits, rows in ((12, 11), (12, 15), (6, 16)):
        shift, ps = 63 - 12 - bits, 63 - 12
        pre = some_prefixes(rng, keys, ps, rows)
        out = guarded(rows * (4 << bits))
        st = lib.load().ibvh_key_histogram(8, dev.data_ptr(), n, shift, bits, ps, u64s(pre), rows, out.data_ptr(), None)
        torch.cuda.synchronize()
        assert st == abi.ERR_INVALID_ARG, (bits, rows)
        assert host(out, np.uint8, 0)[1], "a refused call wrote to out"
        step = max_rows(bits)
        got = np.concatenate([check_histogram(keys, dev, shift, bits, ps, pre[r0:r0 + step]) for r0 in range(0, rows, step)])
        assert np.array_equal(got, histogram_reference(keys, shift, bits, ps, pre))


def test_key_histogram_refuses_shifts_a_64_bit_key_cannot_take():
    keys = np.arange(100, dtype=np.uint64)
    dev = cuda(keys)
    for shift, ps, pre in ((64, 64, []), (-1, 64, []), (0, -1, [0]), (200, 64, [])):
        out = guarded(4 << 6)
        st = lib.load().ibvh_key_histogram(8, dev.data_ptr(), 100, shift, 6, ps, u64s(pre) if pre else None, len(pre), out.data_ptr(), None)
        torch.cuda.synchronize()
        assert st == abi.ERR_INVALID_ARG and host(out, np.uint8, 0)[1], (shift, ps)
    # a negative prefix_shift is not looked at without prefixes (the driver's first level passes 64; any value must do)
    check_histogram(keys, dev, 0, 6, -1, [])


# ---------------------------------------------------------------------------------------------
# ibvh_dist_partition
# ---------------------------------------------------------------------------------------------
def partition(keys, keys_dev, splitters, nranks, with_counts, scratch_short=0):
    """-> (status, perm, counts or None, guards intact)"""
    n, kb = len(keys), keys.dtype.itemsize
    need = C.c_size_t()
    lib.call("ibvh_dist_partition_scratch_bytes", n, C.byref(need))
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    perm = guarded(4 * n)
    counts = guarded(8 * nranks) if with_counts else None
    st = lib.load().ibvh_dist_partition(kb, keys_dev.data_ptr() if n else None, n, u64s(splitters) if nranks > 1 else None, nranks,
                                        perm.data_ptr(), counts.data_ptr() if with_counts else None, scratch.data_ptr(),
                                        need.value - scratch_short, None)
    torch.cuda.synchronize()
    p, ok = host(perm, np.uint32, n)
    c = None
    if with_counts:
        c, ok2 = host(counts, np.uint64, nranks)
        ok = ok and ok2
    return st, p, c, ok


def check_partition(keys, keys_dev, splitters, with_counts, what=""):
    nranks = len(splitters) + 1
    where = f"{what} key_bytes={keys.dtype.itemsize} n={len(keys)} nranks={nranks} counts={with_counts}"
    st, perm, counts, intact = partition(keys, keys_dev, splitters, nranks, with_counts)
    assert st == abi.OK, where
    assert intact, "words behind perm_out / counts_out were written: " + where
    dest = np.searchsorted(np.array(splitters, dtype=np.uint64), keys.astype(np.uint64), side="right")
    assert np.array_equal(perm, np.argsort(dest, kind="stable").astype(np.uint32)), where
    if with_counts:
        assert np.array_equal(counts, np.bincount(dest, minlength=nranks).astype(np.uint64)), where
    return dest


def quantile_splitters(keys, nranks):
    """nranks - 1 ascending splitters taken FROM the keys: every splitter has keys equal to it (they go to the rank on its
    right).  Fewer distinct keys than ranks: the splitters repeat (empty ranks)."""
    s = np.sort(keys.astype(np.uint64))
    return [int(s[len(s) * r // nranks]) for r in range(1, nranks)]


PARTITION_RANKS = [1, 2, 3, 5, 255, 256]


@pytest.mark.parametrize("n", [1, 256, 257, 4096 * 256 + 77])
@pytest.mark.parametrize("key_bytes", [4, 8])
def test_dist_partition_sizes_and_ranks(key_bytes, n):
    """One key, one block, one more, and 4,096 x 256 + 77 — past the 4,096-block cap of the destination kernel — for 1 to 256
    ranks, with and without counts_out; the splitters are keys of the input, so keys equal to a splitter are always present."""
    rng = np.random.default_rng(2000 * key_bytes + n % 991)
    keys = rng.integers(0, 2**(30 if key_bytes == 4 else 63), n, dtype=np.uint64).astype(KEY_NP[key_bytes])
    dev = cuda(keys)
    for nranks in PARTITION_RANKS:
        sp = quantile_splitters(keys, nranks)
        for with_counts in (False, True):
            dest = check_partition(keys, dev, sp, with_counts)
        if n > 1000 and nranks > 1:
            assert (keys.astype(np.uint64) == np.uint64(sp[0])).any() and dest[keys.astype(np.uint64) == np.uint64(sp[0])].min() == 1


@pytest.mark.parametrize("n", [(1 << 22) - 1, 1 << 22])
def test_dist_partition_on_both_sides_of_the_sort_route_change(n):
    """The partition sorts a key of <= 8 bits with implicit values through rsort::sort_pairs.  For such a key the planner in
    ibvh_sort.hip never takes the MSD hybrid (choose_msd: key_bits <= 8 -> plain LSD, one pass), so the one size at which the
    route changes is choose_geometry's n = 2^22 = 4,194,304: below it 256 x 8 tiles, from it on 512 x 16 tiles.  2^22 - 1 and
    2^22, with 256 ranks (8 key bits) and with 3 (2 key bits)."""
    rng = np.random.default_rng(n % 1009)
    keys = rng.integers(0, 2**30, n, dtype=np.uint64).astype(np.uint32)
    dev = cuda(keys)
    check_partition(keys, dev, quantile_splitters(keys, 256), True, "route")
    check_partition(keys, dev, [2**28, 2**29 + 12345], False, "route")


def test_dist_partition_splitter_shapes():
    """Distinct splitters; runs of equal ones (empty ranks in the middle); first splitter 0 (rank 0 empty); last splitter
    2^64 - 1 (only the maximum key reaches the last rank); splitters >= 2^32 under 4-byte keys (no key reaches them); 8-byte
    keys that differ only in the high word; keys equal to a splitter."""
    rng = np.random.default_rng(21)
    n = 5003
    k8 = rng.integers(0, 2**63, n, dtype=np.uint64)
    k8[:7] = U64_MAX
    k8[7:11] = 0
    d8 = cuda(k8)
    q = quantile_splitters(k8, 5)
    for sp in (q, [q[0], q[0], q[0], q[3]], [0] + q[1:], [0, 0, q[2], q[3]], q[:3] + [U64_MAX], [U64_MAX] * 4, [0] * 4,
               [q[1]] * 255, sorted(rng.integers(0, 2**63, 255, dtype=np.uint64).tolist())):
        for with_counts in (False, True):
            dest = check_partition(k8, d8, sp, with_counts, f"splitters {sp[:4]}")
        if sp[0] == 0:
            assert (dest > 0).all()                      # rank 0 empty, zero keys included
        if sp[-1] == U64_MAX:
            assert (dest == len(sp)).sum() == 7          # only the maximum key sits right of 2^64 - 1
    k4 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    k4[:5] = 2**32 - 1
    d4 = cuda(k4)
    q = quantile_splitters(k4, 4)
    for sp in (q, q[:2] + [2**32], q[:1] + [2**32, 2**40], [2**32 - 1, 2**32, 2**63], [2**32] * 3, [q[0], q[0], q[2]]):
        for with_counts in (False, True):
            dest = check_partition(k4, d4, sp, with_counts, f"4-byte keys, splitters {sp}")
        assert (dest <= sum(s < 2**32 for s in sp)).all()  # no 4-byte key reaches a splitter of 2^32 or more
    hi = (rng.integers(0, 2**31, n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x12345678)
    dh = cuda(hi)
    for nranks in (2, 5, 256):
        check_partition(hi, dh, quantile_splitters(hi, nranks), True, "high words")
    # splitters that differ from the keys only in the LOW word: just left and just right of a key
    mid = int(np.sort(hi)[n // 2])
    check_partition(hi, dh, [mid - 1, mid, mid + 1], True, "around a key")


def test_dist_partition_refusals_and_empty_input():
    rng = np.random.default_rng(22)
    keys = rng.integers(0, 2**63, 1000, dtype=np.uint64)
    dev = cuda(keys)
    sp256 = quantile_splitters(keys, 256)
    # 257 ranks: IBVH_ERR_UNSUPPORTED; a scratch one byte short: IBVH_ERR_SCRATCH — and neither has touched perm_out or counts_out
    st, perm, counts, intact = partition(keys, dev, sp256 + [U64_MAX], 257, True)
    assert st == abi.ERR_UNSUPPORTED and intact and (perm.view(np.uint8) == GUARD).all() and (counts.view(np.uint8) == GUARD).all()
    st, perm, counts, intact = partition(keys, dev, sp256, 256, True, scratch_short=1)
    assert st == abi.ERR_SCRATCH and intact and (perm.view(np.uint8) == GUARD).all() and (counts.view(np.uint8) == GUARD).all()
    # n == 0 with counts_out: zeros, nothing else is touched (no keys, no perm_out, no scratch needed)
    counts = guarded(8 * 5)
    perm = guarded(64)
    st = lib.load().ibvh_dist_partition(8, None, 0, u64s([1, 2, 3, 4]), 5, perm.data_ptr(), counts.data_ptr(), None, 0, None)
    torch.cuda.synchronize()
    c, intact = host(counts, np.uint64, 5)
    assert st == abi.OK and (c == 0).all() and intact and host(perm, np.uint8, 0)[1]
    assert lib.load().ibvh_dist_partition(8, None, 0, None, 1, None, None, None, 0, None) == abi.OK


# ---------------------------------------------------------------------------------------------
# ibvh_pack_records
# ---------------------------------------------------------------------------------------------
LEAF_COMBOS = list(itertools.product((abi.BSPHERE, abi.BBOX), (abi.F32, abi.F64), (abi.I32, abi.I64), (abi.U16, abi.U32, abi.U64)))


def pack(types, vols_dev, keys_dev, perm_dev, index_base, n, lay):
    out = guarded(n * lay.leaf_bytes, extra=2 * lay.leaf_bytes)  # two guard records behind n
    st = lib.load().ibvh_pack_records(C.byref(types), vols_dev.data_ptr(), keys_dev.data_ptr(), perm_dev.data_ptr() if perm_dev is not None else None,
                                      index_base, n, out.data_ptr(), None)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    return st, raw[:n * lay.leaf_bytes], bool((raw[n * lay.leaf_bytes:] == GUARD).all())


@pytest.mark.parametrize("combo", LEAF_COMBOS, ids=str)
def test_pack_records_every_leaf_layout(combo):
    """Every (leaf kind, float, index, Morton) combination ibvh_layout_of accepts, read back field by field through
    ibvh_layout's offsets: the volume's bits, .index == index_base + p + 1 in the index type, .morton == keys[p] (UInt16 codes
    are stored from a 4-byte key) with p = perm[i]: no perm, the identity, a random permutation, one with repeats; bases 0,
    12345, 2^40 (Int64), and the last base Int32 takes; 1, 256, 257 records and 4,096 x 256 + 5 (past the 4,096-block cap)."""
    kind, flt, idx, mor = combo
    types = abi.make_types(kind, flt, abi.BBOX, abi.F32, idx, mor)
    lay = abi.Layout()
    lib.call("ibvh_layout_of", C.byref(types), C.byref(lay))
    rec_dt = abi.leaf_dtype(types)
    assert rec_dt.itemsize == lay.leaf_bytes and rec_dt.fields["index"][1] == lay.index_off and rec_dt.fields["morton"][1] == lay.morton_off
    rng = np.random.default_rng(hash(combo) % 2**32)
    width, fdt = abi.volume_width(kind), abi.FLOAT_DTYPES[flt]
    key_dt, key_bits = abi.key_dtype(types), abi.MORTON_BITS[mor]
    bases = [0, 12345] + ([2**40] if idx == abi.I64 else [])
    for n in (1, 256, 257, 4096 * 256 + 5):
        vols = rng.standard_normal((n, width)).astype(fdt)
        vols[0, 0] = -0.0
        keys = rng.integers(0, 2**key_bits, n, dtype=np.uint64).astype(key_dt)
        keys[-1] = 2**key_bits - 1
        vd, kd = cuda(vols), cuda(keys)
        perms = {"none": None, "identity": np.arange(n, dtype=np.uint32), "random": rng.permutation(n).astype(np.uint32),
                 "repeats": rng.integers(0, n, n, dtype=np.uint64).astype(np.uint32)}
        cases = list(itertools.product(perms, bases)) if n < 1000 else [("random", bases[-1]), ("none", 0)]
        if idx == abi.I32:
            cases.append(("repeats", INT32_MAX - n))  # the largest index any record can get is exactly INT32_MAX
        for which, base in cases:
            perm = perms[which]
            st, raw, intact = pack(types, vd, kd, cuda(perm) if perm is not None else None, base, n, lay)
            where = f"n={n} perm={which} base={base}"
            assert st == abi.OK, where
            assert intact, "records behind n were written: " + where
            rec = raw.view(rec_dt)
            p = perm.astype(np.int64) if perm is not None else np.arange(n, dtype=np.int64)
            assert rec["volume"].tobytes() == vols[p].tobytes(), where
            assert np.array_equal(rec["index"].astype(np.int64), base + p + 1), where
            assert np.array_equal(rec["morton"].astype(np.uint64), keys[p].astype(np.uint64)), where


def test_pack_records_refuses_indices_past_int32():
    types = abi.make_types()
    lay = abi.Layout()
    lib.call("ibvh_layout_of", C.byref(types), C.byref(lay))
    n = 300
    vd, kd = cuda(np.ones((n, 4), np.float32)), cuda(np.arange(n, dtype=np.uint32))
    for base, status in ((INT32_MAX - n + 1, abi.ERR_OVERFLOW), (2**40, abi.ERR_OVERFLOW), (-1, abi.ERR_INVALID_ARG)):
        st, raw, intact = pack(types, vd, kd, None, base, n, lay)
        assert st == status and intact and (raw == GUARD).all(), base
    t64 = abi.make_types(index_type=abi.I64)
    lib.call("ibvh_layout_of", C.byref(t64), C.byref(lay))
    st, raw, intact = pack(t64, vd, kd, None, INT32_MAX, n, lay)
    assert st == abi.OK and intact and np.array_equal(raw.view(abi.leaf_dtype(t64))["index"], INT32_MAX + 1 + np.arange(n, dtype=np.int64))


# ---------------------------------------------------------------------------------------------
# extrema: expand, pack, unpack
# ---------------------------------------------------------------------------------------------
def device_extrema(types, vols, expand):
    """ibvh_extrema over raw volumes -> 6 values of the leaf float type (host)"""
    fdt = abi.FLOAT_DTYPES[types.leaf_float]
    dv = cuda(vols)
    ext = guarded(6 * np.dtype(fdt).itemsize)
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    lib.call("ibvh_extrema", C.byref(types), dv.data_ptr(), 0, len(vols), expand, ext.data_ptr(), scratch.data_ptr(), scratch.numel(), None)
    torch.cuda.synchronize()
    got, intact = host(ext, fdt, 6)
    assert intact
    return got, ext


def special_spheres(rng, flt, n):
    """Sphere centres whose extrema are the values an expansion can go wrong on: axis 0 spans -floatmax .. +floatmax (+-Inf after
    the expansion), axis 1 -Inf .. +Inf, axis 2 holds 0, -0, a subnormal and negative values only (its maximum is the
    reference's neutral element, floatmin)."""
    fdt = abi.FLOAT_DTYPES[flt]
    fi = np.finfo(fdt)
    v = rng.standard_normal((n, 4)).astype(fdt)
    v[:, 3] = np.abs(v[:, 3])
    v[:, 2] = -np.abs(v[:, 2])
    v[0, 2], v[1, 2], v[2 % n, 2] = 0.0, -0.0, fi.smallest_subnormal
    if n >= 4:
        v[n // 2, 0], v[n - 1, 0] = fi.max, -fi.max
        v[n // 3, 1], v[n - 2, 1] = np.inf, -np.inf
    return v


EXTREMA_INPUTS = ["random", "special", "zeros", "tiny"]


def extrema_input(which, rng, kind, flt, n):
    fdt = abi.FLOAT_DTYPES[flt]
    if which == "special":
        return special_spheres(rng, flt, n)
    if which == "zeros":     # every centre +-0: the expansion gives -+floatmin
        v = np.zeros((n, 4), fdt)
        v[::2, :3] = -0.0
        return v
    if which == "tiny":      # subnormal centres only
        v = (rng.integers(-50, 50, (n, 4)) * np.finfo(fdt).smallest_subnormal).astype(fdt)
        v[:, 3] = 0
        return v
    c = (6 * rng.standard_normal((n, 3))).astype(fdt)
    if kind == abi.BSPHERE:
        return np.concatenate([c, np.abs(rng.standard_normal((n, 1))).astype(fdt)], axis=1)
    h = np.abs(rng.standard_normal((n, 3))).astype(fdt)
    return np.concatenate([c - h, c + h], axis=1)


def expand_reference(ext, flt):
    """morton/utils.jl:63-69 in the leaf float type, two roundings a side: mins - rp |mins| - floatmin, maxs + rp |maxs| + floatmin"""
    fdt = abi.FLOAT_DTYPES[flt]
    rp, fm = fdt(1e-5 if flt == abi.F32 else 1e-14), np.finfo(fdt).tiny
    e = np.asarray(ext, dtype=fdt)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (rp * np.abs(e)).astype(fdt)
        return np.concatenate([((e[:3] - a[:3]).astype(fdt) - fm).astype(fdt), ((e[3:] + a[3:]).astype(fdt) + fm).astype(fdt)])


@pytest.mark.parametrize("which", EXTREMA_INPUTS)
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_expand_extrema_equals_the_expanding_reduce_and_the_oracle(flt, which):
    """ibvh_expand_extrema(ibvh_extrema(expand = 0)) is bit-equal to ibvh_extrema(expand = 1), to the oracle's extrema and to
    the expansion done in numpy in the leaf float type; the 7th value behind the six is not touched."""
    rng = np.random.default_rng(31 + flt)
    for kind in ((abi.BSPHERE,) if which != "random" else (abi.BSPHERE, abi.BBOX)):
        types = abi.make_types(kind, flt)
        vols = extrema_input(which, rng, kind, flt, 3001)
        raw, raw_dev = device_extrema(types, vols, 0)
        want, _ = device_extrema(types, vols, 1)
        assert lib.load().ibvh_expand_extrema(flt, raw_dev.data_ptr(), None) == abi.OK
        torch.cuda.synchronize()
        got, intact = host(raw_dev, abi.FLOAT_DTYPES[flt], 6)
        assert intact
        assert got.tobytes() == want.tobytes(), (got, want)
        recs = orc.as_volumes(vols, kind, flt)
        assert got.tobytes() == orc.extrema(types, recs, 0, expand=True).tobytes()
        want_raw = orc.extrema(types, recs, 0, expand=False)
        assert np.array_equal(raw, want_raw) if which == "zeros" else raw.tobytes() == want_raw.tobytes()  # (min(0, -0): either zero)
        assert got.tobytes() == expand_reference(raw, flt).tobytes()
        if which == "special":
            assert got[0] == -np.inf and got[3] == np.inf and got[1] == -np.inf and got[4] == np.inf


def pack_vec(flt, ext_dev, has_data, rank, nranks, n_local):
    vec = guarded(8 * (6 + nranks))
    st = lib.load().ibvh_dist_pack_extrema(flt, ext_dev.data_ptr() if ext_dev is not None else None, has_data, rank, nranks, n_local,
                                           vec.data_ptr(), None)
    torch.cuda.synchronize()
    got, intact = host(vec, np.float64, 6 + nranks)
    return st, got, intact, vec


@pytest.mark.parametrize("which", EXTREMA_INPUTS)
@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_extrema_round_trip_over_ranks(flt, world, which):
    """Every rank packs its share's unexpanded extrema (one rank has no leaves: has_data = 0, a NULL extrema pointer), the
    vectors are reduced with np.maximum on the host, the result is unpacked: bit-equal to ibvh_extrema(expand = 1) over the
    union.  Each packed vector is [-mins, maxs, one-hot count] computed in numpy, bit for bit; the reduced tail is exactly
    the per-rank counts, 2^53 among them."""
    rng = np.random.default_rng(100 * world + flt)
    fdt = abi.FLOAT_DTYPES[flt]
    fi = np.finfo(fdt)
    types = abi.make_types(abi.BSPHERE, flt)
    n = 2000 + world
    vols = extrema_input(which, rng, abi.BSPHERE, flt, n)
    empty = world // 2 if world > 1 else None  # the rank without leaves
    cuts = np.sort(rng.integers(1, n, world - 1)) if world > 1 else np.zeros(0, np.int64)
    bounds = [0] + cuts.tolist() + [n]
    if empty is not None:
        bounds[empty + 1] = bounds[empty]
    told = [2**53 if r == 0 else bounds[r + 1] - bounds[r] for r in range(world)]  # (the count is the caller's word: rank 0 claims 2^53)
    reduced = np.full(6 + world, -np.inf)
    for r in range(world):
        share = vols[bounds[r]:bounds[r + 1]]
        if len(share):
            ext, ext_dev = device_extrema(types, share, 0)
            want6 = np.concatenate([-ext[:3].astype(np.float64), ext[3:].astype(np.float64)])
        else:
            ext_dev = None
            want6 = np.array([-float(fi.max)] * 3 + [float(fi.tiny)] * 3)
        st, vec, intact, _ = pack_vec(flt, ext_dev, 1 if len(share) else 0, r, world, told[r])
        assert st == abi.OK and intact
        want = np.concatenate([want6, [float(told[q]) if q == r else 0.0 for q in range(world)]])
        assert vec.tobytes() == want.tobytes(), (r, vec, want)
        reduced = np.maximum(reduced, vec)
    assert [int(c) for c in reduced[6:]] == told and reduced[6] == 2.0**53
    vec_dev = cuda(reduced)
    out = guarded(6 * fi.bits // 8)
    assert lib.load().ibvh_dist_unpack_extrema(flt, vec_dev.data_ptr(), out.data_ptr(), None) == abi.OK
    torch.cuda.synchronize()
    got, intact = host(out, fdt, 6)
    assert intact
    want, _ = device_extrema(types, vols, 1)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert got.tobytes() == orc.extrema(types, orc.as_volumes(vols, abi.BSPHERE, flt), 0, expand=True).tobytes()


@pytest.mark.parametrize("flt", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_pack_and_unpack_extrema_on_given_values(flt):
    """pack and unpack on extrema handed in directly: 0, -0, a subnormal, +-floatmax, +-Inf keep their bits through
    float -> -double -> float, and the expansion in unpack equals numpy's in the leaf float type."""
    fdt = abi.FLOAT_DTYPES[flt]
    fi = np.finfo(fdt)
    for ext in ([0.0, -0.0, fi.smallest_subnormal, -0.0, 0.0, -fi.smallest_subnormal], [-fi.max, -np.inf, fi.max, fi.max, np.inf, -fi.max],
                [fi.tiny, -fi.tiny, 1.0, fi.tiny, -fi.tiny, 1.0], [-3.5, 2.25, 1e-30, 7.0, 2.25, 1e30]):
        e = np.array(ext, dtype=fdt)
        st, vec, intact, vec_dev = pack_vec(flt, cuda(e), 1, 2, 5, 77)
        want = np.concatenate([-e[:3].astype(np.float64), e[3:].astype(np.float64), [0, 0, 77, 0, 0]])
        assert st == abi.OK and intact and vec.tobytes() == want.tobytes(), ext
        out = guarded(6 * fi.bits // 8)
        assert lib.load().ibvh_dist_unpack_extrema(flt, vec_dev.data_ptr(), out.data_ptr(), None) == abi.OK
        torch.cuda.synchronize()
        got, intact = host(out, fdt, 6)
        assert intact and got.tobytes() == expand_reference(e, flt).tobytes(), (ext, got)


def test_pack_extrema_rank_limits():
    """1,018 ranks (6 + 1,018 = the 1,024 threads of the one block) are accepted and every element is written; 1,019 are not."""
    e = cuda(np.arange(6, dtype=np.float32))
    st, vec, intact, _ = pack_vec(abi.F32, e, 1, 1017, 1018, 5)
    want = np.concatenate([[-0.0, -1.0, -2.0, 3.0, 4.0, 5.0], np.zeros(1017), [5.0]])
    assert st == abi.OK and intact and vec.tobytes() == want.tobytes()
    st, vec, intact, _ = pack_vec(abi.F32, e, 1, 0, 1019, 5)
    assert st == abi.ERR_INVALID_ARG and intact and (vec.view(np.uint8) == GUARD).all()


# ---------------------------------------------------------------------------------------------
# the driver where the virtual-rank tests of test_gpu_parity.py never took it
# ---------------------------------------------------------------------------------------------
def _virtual_ranks():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import virtual_ranks
    return virtual_ranks


def _distributed(world, n, seed, tolerance, types):
    """-> (the oracle's single-device build, [(leaves, builder.last) per rank])"""
    from implicitbvh_amd import dist as ibd
    r0 = 0.5 * (3 * 8 / (4 * np.pi * n)) ** (1 / 3)
    single = orc.build(orc.generate_spheres_f32(n, seed, r0=r0), types)
    bounds = [n * r // world for r in range(world + 1)]
    options = ibvh.BVHOptions(index=abi.INDEX_DTYPES[types.index_type], morton=ibvh.DefaultMortonAlgorithm(abi.MORTON_DTYPES[types.morton_type]))

    def fn(comm):
        vols = ibvh.generate_spheres(bounds[comm.rank + 1] - bounds[comm.rank], seed, first_index=bounds[comm.rank], r0=r0)
        builder = ibd.DistributedBuilder(comm, tolerance=tolerance)
        bvh = builder.build(vols, options=options)
        torch.cuda.synchronize()
        return bvh.leaves.to_numpy(), builder.last
    return single, _virtual_ranks().run_virtual_ranks(world, fn)


@pytest.mark.parametrize("im", [(abi.I32, abi.U32), (abi.I64, abi.U64)], ids=["u32", "u64"])
def test_distributed_build_sixteen_ranks_exact_splitters(im):
    """World 16, tolerance 0: all 15 splitters stay undecided down to the last key bit, so every refinement level asks for 15
    histogram rows — more than one ibvh_key_histogram call takes at 12 bits.  About 3,000 leaves a rank, none empty.  The
    slices, concatenated, are the single-device build byte for byte; the extrema are equal; the splitters are the keys at the
    balanced positions of the sorted sequence and the slice sizes follow from them (numpy), within 1 of each other."""
    world, n = 16, 16 * 3000 + 7
    types = abi.make_types(index_type=im[0], morton_type=im[1])
    single, out = _distributed(world, n, 52, 0.0, types)
    cat = np.concatenate([o[0] for o in out])
    assert cat.tobytes() == single.leaves.tobytes()
    keys = single.leaves["morton"].astype(np.uint64)  # sorted
    splitters = [int(keys[(k + 1) * n // world]) for k in range(world - 1)]
    sizes = np.bincount(np.searchsorted(np.array(splitters, dtype=np.uint64), keys, side="right"), minlength=world).tolist()
    for leaves, last in out:
        assert last["extrema"].tobytes() == single.extrema.tobytes()
        assert last["levels_used"] == abi.MORTON_BITS[im[1]] and last["n_global"] == n
        assert last["splitters"] == splitters
    assert [len(o[0]) for o in out] == sizes
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1


def test_distributed_build_thirty_two_ranks_default_tolerance():
    """World 32, default tolerance 0.005, a uniform cloud: a first-level bucket holds N / 4096 keys, more than the 0.005 N / 32
    a splitter may leave undecided, so (nearly) all 31 splitters go to a second level — several batches of histogram rows."""
    world, n = 32, 32 * 3000 + 11
    types = abi.make_types()
    single, out = _distributed(world, n, 53, 0.005, types)
    cat = np.concatenate([o[0] for o in out])
    assert cat.tobytes() == single.leaves.tobytes()
    for leaves, last in out:
        assert last["extrema"].tobytes() == single.extrema.tobytes()
        assert last["levels_used"] > 12
    sizes = [len(o[0]) for o in out]
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 2 * int(0.005 * n / world) + 1  # each end of a slice is off by at most tolerance x N / P
