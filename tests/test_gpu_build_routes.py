"""ibvh_build against the oracle, bit for bit (leaves: volume, index, Morton; nodes; skips; extrema), at the sizes where the
build's sort changes its route or its kernel geometry (csrc/ibvh_build.hip choose_route, ibvh_sort.hip plan_pairs,
ibvh_msd_plan.hpp make_plan):
    n < 2,048            the pair sort's LSD passes, the last scatter writing the records
    2,048 <= n < 4,096   the pair sort's hybrid: one MSD partition of the pairs, the bucket sort writing the records
    n >= 4,096           the record sort: partition of whole records + in-LDS finish
for every Morton type, for fresh volumes, for already wrapped records in place (volumes == NULL: the caller's records are
input and output, user indices kept) and out of place (the source records stay untouched), on a uniform cloud and on a
lattice of at most 64 distinct centres — nearly every key ties there, so the order of the leaves is the sort's stability.
Each build names the kernels it launched through the library's launch profile: a planner that silently took another route,
or whose key encoder and sort disagreed about the first histogram (the sort would launch one of its own for its first pass),
fails here."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_parity import TOKENS, assert_bvh_equal, cuda, make_options, random_volumes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi  # noqa: E402
from test_gpu_lvt_blocks import _kernels_of  # noqa: E402

SIZES = [1, 2, 3, 2047, 2048, 2049, 4095, 4096, 4097]
# (Morton type, index type): Int32 and Int64 once each
TYPES = {"u16-i32": (abi.U16, abi.I32), "u32-i32": (abi.U32, abi.I32), "u64-i64": (abi.U64, abi.I64)}
CLOUDS = ("uniform", "lattice")
MODES = ("fresh", "in_place", "out_of_place")

LSD = {"scan_kernel", "scatter_kernel"}  # (+ hist_kernel for every 8-bit pass after the first, whose histogram the encoder made)
KEY_BITS = {abi.U16: 15, abi.U32: 30, abi.U64: 63}
HYBRID = {"scan_kernel", "scatter_wide_kernel", "bucket_sort_kernel"}
RECORDS = {"scan_tiles_kernel", "partition_kernel", "finish_kernel"}  # (+ the extra levels' kernels, which find nothing to do)
SORT_KERNELS = LSD | HYBRID | RECORDS | {"hist_kernel", "hist_wide_kernel", "finish_resident_kernel"}


def expected_sort(n, morton):
    if n < 2048:
        return LSD | ({"hist_kernel"} if KEY_BITS[morton] > 8 else set())
    return HYBRID if n < 4096 else RECORDS


def base_name(label):
    """'(ibvh::rsort::scatter_kernel<K, TPB, IPT, true>)' -> 'scatter_kernel'"""
    return label.strip("() ").split("<")[0].split("::")[-1].strip()


@functools.lru_cache(maxsize=None)
def volumes(n, cloud):
    """n BSphere{F32}; lattice: centres on a 4 x 4 x 4 grid (<= 64 distinct), radii all different"""
    rng = np.random.default_rng(7 * n + len(cloud))
    vols = random_volumes(rng, n, abi.BSPHERE, abi.F32)
    if cloud == "lattice":
        vols[:, :3] = rng.integers(0, 4, (n, 3)).astype(np.float32) * np.float32(1.5)
        assert len(np.unique(vols[:, :3], axis=0)) <= 64
    vols.setflags(write=False)
    return vols


@functools.lru_cache(maxsize=None)
def user_indices(n):
    return np.random.default_rng(n).permutation(n) + 100


@functools.lru_cache(maxsize=None)
def oracle(n, cloud, tname, wrapped):
    morton, index = TYPES[tname]
    types = abi.make_types(index_type=index, morton_type=morton)
    return orc.build(volumes(n, cloud), types, indices=user_indices(n) if wrapped else None)


def build(n, cloud, tname, mode):
    """(device BVH, the kernels its build launched, the source records of a wrapped build before the build)"""
    morton, index = TYPES[tname]
    types = abi.make_types(index_type=index, morton_type=morton)
    opts = make_options(types)
    node_type = TOKENS[abi.BBOX](torch.float32)
    dev = cuda(volumes(n, cloud).copy())
    holder = {}
    if mode == "fresh":
        names = _kernels_of(lambda: holder.update(g=ibvh.BVH(dev, node_type, options=opts)))
        return holder["g"], names, None, None
    bv = ibvh.BoundingVolumes.wrap(dev, user_indices(n), opts)
    before = bv.buf.clone()
    names = _kernels_of(lambda: holder.update(g=ibvh.BVH(bv, node_type, options=opts, _out_of_place=(mode == "out_of_place"))))
    return holder["g"], names, bv, before


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("n", SIZES)
def test_build_matches_the_oracle_on_the_expected_route(n, tname):
    for cloud in CLOUDS:
        for mode in MODES:
            what = (n, tname, cloud, mode)
            o = oracle(n, cloud, tname, mode != "fresh")
            g, names, src, before = build(n, cloud, tname, mode)
            assert_bvh_equal(o, g)
            if mode == "in_place":
                assert g.leaves.buf.data_ptr() == src.buf.data_ptr(), what
            if mode == "out_of_place":
                assert g.leaves.buf.data_ptr() != src.buf.data_ptr() and torch.equal(src.buf, before), what
            ran = {base_name(s) for s in names}
            assert "encode_hist_kernel" in ran, (what, names)
            # the sort's kernels: exactly the route's family, and no histogram launch of the sort's own for its FIRST pass
            # (the key encoder's fused one is the one the sort planned for): the sort starts with a scan, and the LSD passes
            # launch hist_kernel once per later pass only
            assert ran & SORT_KERNELS == expected_sort(n, TYPES[tname][0]), (what, names)
            sort_launches = [base_name(s) for s in names if base_name(s) in SORT_KERNELS]
            assert sort_launches[0] in ("scan_kernel", "scan_tiles_kernel"), (what, names)
            if n < 2048:
                passes = -(-KEY_BITS[TYPES[tname][0]] // 8)
                assert sort_launches == ["scan_kernel", "scatter_kernel"] + ["hist_kernel", "scan_kernel", "scatter_kernel"] * (passes - 1), (what, names)
            # the pair sort writes the records in its last launch (RECORDS = true), and only there
            flat = [s.replace(" ", "") for s in names]
            writers = [s for s in flat if base_name(s) in ("scatter_kernel", "bucket_sort_kernel") and s.endswith("true>)")]
            if n < 4096:
                last = [s for s in flat if base_name(s) in ("scatter_kernel", "bucket_sort_kernel")][-1]
                assert writers == [last], (what, names)
            else:
                assert not writers, (what, names)
