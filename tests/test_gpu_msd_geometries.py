"""Every geometry the record sort's planner can choose (csrc/ibvh_msd_plan.hpp: the rows of the partition and finish tables),
built and compared with the oracle bit for bit at sizes that take seconds.  Only full-size builds reach anything but the
smallest finish workgroup under the shipped settings; here the development knob msd_avg = 2^20 keeps the first digit at 6 bits,
so the average cell is n / 64 and the planner's own rule picks the larger workgroups at small n.  Each case asserts the geometry
it expects through the host-compiled view of the plan before it builds — a wrong expectation fails on the CPU first — and that
the library's size query under the knob is the one of that plan.  The (512, 8) partition tile needs 2^22 leaves and stays with the
full-size tests.  Each case: a cold build of fresh volumes and one of wrapped records in place, on a uniform cloud and on the
64-centre lattice of test_gpu_build_routes.py (every cell one run of equal keys: the leaves' order is the sort's stability)."""
import ctypes as C
import functools

import numpy as np
import pytest

import msd_plan_view as mv
import oracle_lib as orc
from test_gpu_parity import TOKENS, assert_bvh_equal, cuda, make_options, random_volumes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

MSD_AVG = 2**20
KEYS = {abi.U32: (30, 4), abi.U64: (63, 8)}  # Morton type -> key bits, key bytes
# name: (leaves — odd counts no other test builds: the Python mirror memoises scratch sizes per (types, n), and the knob moves them —
#        leaf kind, Morton type, finish row (key bytes, capacity, threads, resident), partition row, crowded cells)
CASES = {
    "2048": (64 * 1000 + 1, abi.BSPHERE, abi.U32, (4, 2048, 256, 0), (256, 4), False),
    "4096": (64 * 2400 + 1, abi.BSPHERE, abi.U32, (4, 4096, 256, 0), (256, 8), False),
    "8192-resident": (64 * 4500 + 1, abi.BSPHERE, abi.U32, (4, 8192, 1024, 1), (256, 8), False),  # 24-byte records
    "8192-bbox": (64 * 4500 + 3, abi.BBOX, abi.U32, (4, 8192, 512, 0), (256, 8), False),            # 32-byte records: not resident
    "16384": (64 * 9000 + 1, abi.BSPHERE, abi.U32, (4, 16384, 512, 0), (256, 8), False),
    "u64-2048": (64 * 1000 + 3, abi.BSPHERE, abi.U64, (8, 2048, 256, 0), (256, 4), False),
    "u64-4096": (64 * 2400 + 3, abi.BSPHERE, abi.U64, (8, 4096, 256, 0), (256, 8), False),
    "u64-8192": (64 * 4500 + 5, abi.BSPHERE, abi.U64, (8, 8192, 512, 0), (256, 8), False),
    # the last row for 64-bit keys whatever the cell: ~9,000 records per cell of 8,192 go through the extra levels a cold build launches
    "u64-8192-crowded": (64 * 9000 + 3, abi.BSPHERE, abi.U64, (8, 8192, 512, 0), (256, 8), True),
}


def test_the_cases_reach_every_row_of_both_tables_but_the_large_tile():
    assert {c[3] for c in CASES.values()} == set(mv.finish_rows())
    assert {c[4] for c in CASES.values()} | {(512, 8)} == set(mv.partition_rows())


def types_of(kind, morton):
    return abi.make_types(kind, abi.F32, abi.BBOX, abi.F32, abi.I32, morton)


@functools.lru_cache(maxsize=None)
def volumes(n, kind, cloud):
    rng = np.random.default_rng(11 * n + len(cloud))
    vols = random_volumes(rng, n, kind, abi.F32)
    if cloud == "lattice":  # centres on a 4 x 4 x 4 grid, sizes all different
        centre = rng.integers(0, 4, (n, 3)).astype(np.float32) * np.float32(1.5)
        if kind == abi.BSPHERE:
            vols[:, :3] = centre
        else:
            half = (vols[:, 3:] - vols[:, :3]) * np.float32(0.5)
            vols[:, :3], vols[:, 3:] = centre - half, centre + half
    vols.setflags(write=False)
    return vols


def scratch_bytes(types, n):
    need = C.c_size_t()
    lib.call("ibvh_build_scratch_bytes", C.byref(types), n, C.byref(need))
    return need.value


@pytest.fixture
def knob():
    """msd_avg = 2^20 for the test, and none of its scratch sizes left in (or taken from) the mirror's memo"""
    def forget():
        for key in [k for k in api._shape_memo if isinstance(k, tuple) and k[0] == "build_scratch"]:
            del api._shape_memo[key]
    forget()
    try:
        lib.set_tuning("msd_avg", MSD_AVG)
        yield
    finally:
        lib.set_tuning("msd_avg", 1024)
        forget()


@pytest.mark.parametrize("name", list(CASES))
def test_build_matches_the_oracle_on_the_expected_geometry(name, knob):
    n, kind, morton, finish, partition, crowded = CASES[name]
    key_bits, key_bytes = KEYS[morton]
    types = types_of(kind, morton)
    lay = abi.Layout()
    lib.call("ibvh_layout_of", C.byref(types), C.byref(lay))
    # the plan, on the CPU: the expected rows, a 6-bit digit, cells that fit the finish workgroup (or do not)
    p, tables = mv.plan(n, key_bits, key_bytes, int(lay.leaf_bytes), MSD_AVG)
    assert p is not None and p["bits"] == 6, p
    assert mv.finish_row(p, key_bytes) == finish and (p["part_tpb"], p["part_ipt"]) == partition, p
    assert (n // 64 > finish[1]) == crowded
    # ... and it is the plan the library follows under the knob: its size query moves by exactly these tables
    sort = C.c_size_t()
    lib.call("ibvh_sort_scratch_bytes", key_bytes, n, C.byref(sort))
    lib.set_tuning("msd_avg", 1024)
    p0, tables0 = mv.plan(n, key_bits, key_bytes, int(lay.leaf_bytes), 1024)
    size0 = scratch_bytes(types, n)
    lib.set_tuning("msd_avg", MSD_AVG)
    region = [-(-max(sort.value, t + 4096) // 256) * 256 for t in (tables, tables0)]
    assert (p0 == p) == (n >> 6 <= 1024) and (region[0] == region[1]) == (p0 == p)  # (the smallest workgroup: the shipped plan too)
    assert scratch_bytes(types, n) - size0 == region[0] - region[1]

    opts = make_options(types)
    node_type = TOKENS[abi.BBOX](torch.float32)
    indices = np.random.default_rng(n).permutation(n) + 100
    for cloud in ("uniform", "lattice"):
        vols = volumes(n, kind, cloud)
        # fresh volumes, cold: COLD_SORT_LEVELS extra partition levels are launched, and find work only in the crowded case
        g = ibvh.BVH(cuda(vols.copy()), node_type, options=opts)
        assert_bvh_equal(orc.build(vols, types), g)
        torch.cuda.synchronize()
        if cloud == "uniform":
            assert (int(g._skew[0]) & 0xFF != 0) == crowded, (name, hex(int(g._skew[0])))
        # wrapped records, in place: the caller's buffer is source and destination, user indices kept
        bv = ibvh.BoundingVolumes.wrap(cuda(vols.copy()), indices, opts)
        g = ibvh.BVH(bv, node_type, options=opts)
        assert g.leaves.buf.data_ptr() == bv.buf.data_ptr()
        assert_bvh_equal(orc.build(vols, types, indices=indices), g)
