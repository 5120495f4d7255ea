"""The inclusive scan of the LVT per-item counts (csrc/ibvh_lvt_scan.hip, scan_counts) on every one of its routes, at sizes the
oracle walks in a fraction of a second.  The knob lvt_scan_fused picks the route behind a walker that zeroed the scan's tile
aggregates (walker 2's counting pass, the binned ray path): 0 = scan_reduce_kernel + scan_apply_kernel, 1 = scan_fused_kernel,
N > 1 = at most N workgroups, i.e. scan_fused_grouped_kernel as soon as there are more than N tiles of 4,096 items — a route the
shipped rule takes only beyond millions of items.  Behind a walker that does not zero them (the exact joint walk) the scan is
reduce + apply whatever the knob says.  Each case names the route it took with the library's launch profile and compares the
result with the oracle, in order: the tile edge, a guarded tail, clipped last groups, both index types (16 / 8 items per 16-byte
access), a counts pointer off 16-byte alignment (the guarded loads and stores), and the device-side length of the binned ray path.
The 32-bit overflow return (IBVH_ERR_OVERFLOW) needs more than 2^31 contacts: it stays with the full-size test
(tests/test_gpu_parity.py::test_more_contacts_than_int32_is_an_overflow_error)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_parity import build_both, contacts_np, cuda, oracle_pairs, random_volumes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, lib  # noqa: E402
from test_gpu_lvt_blocks import _kernels_of  # noqa: E402
from test_gpu_rays_binned import _rays  # noqa: E402

TILE = 4096
ROUTES = [0, 1, 2, 3]  # values of lvt_scan_fused
SIZES = [1, 2, 4095, 4096, 4097, 12_293, 20_000, 28_669]
TWO_LAUNCH = {"scan_reduce_kernel", "scan_apply_kernel"}
SCAN_KERNELS = TWO_LAUNCH | {"scan_fused_kernel", "scan_fused_grouped_kernel"}
INDEX_TYPES = {"i32": abi.I32, "i64": abi.I64}


@pytest.fixture
def knob():
    """set_tuning; lvt_scan_fused and rays_binned go back to what they were afterwards"""
    saved = {}
    for k in ("lvt_scan_fused", "rays_binned"):
        v = C.c_int32()
        lib.call("ibvh_get_tuning", k.encode(), C.byref(v))
        saved[k] = v.value
    yield lib.set_tuning
    for k, v in saved.items():
        lib.set_tuning(k, v)


def expected_scan(route, n, zeroed=True):
    """the scan kernels scan_counts launches for n items (zeroed: the walker in front of it zeroed the tile aggregates)"""
    tiles = -(-n // TILE)
    if route == 0 or not zeroed:
        return TWO_LAUNCH
    return {"scan_fused_grouped_kernel"} if route > 1 and tiles > route else {"scan_fused_kernel"}


def scans_in(names):
    return {k for k in SCAN_KERNELS if any(k in name for name in names)}  # (no name is part of another)


@functools.lru_cache(maxsize=None)
def cloud(n, index="i32", seed=0):
    """(oracle BVH, device BVH, the oracle's self list, its scanned counts) of n BSphere{F32} leaves under BBox{F32} nodes"""
    rng = np.random.default_rng(1000 * seed + n)
    vols = random_volumes(rng, n, abi.BSPHERE, abi.F32, scale=0.9 * max(n, 8) ** (1 / 3))
    o, g = build_both(vols, abi.make_types(index_type=INDEX_TYPES[index]))
    contacts, scanned = orc.traverse_lvt(o)
    return o, g, oracle_pairs(contacts), scanned


def check_self(route, n, index="i32"):
    o, g, exp, _ = cloud(n, index)
    if n > 2:
        assert len(exp) > n // 2, "a cloud this sparse checks nothing"
    # (a single leaf: nothing to walk, nothing is launched at all — self_common in csrc/ibvh_lvt.hip; two leaves are the
    # smallest tree walker 2 serves: the one-tile kernels on two items)
    want = expected_scan(route, n) if n > 1 else set()
    names = _kernels_of(lambda: ibvh.traverse(g))
    assert scans_in(names) == want, (route, n, names)
    t = ibvh.traverse(g)
    assert t.num_contacts == len(exp), (route, n)
    assert (contacts_np(t) == exp).all(), (route, n)
    holder = {}
    names = _kernels_of(lambda: holder.update(t2=ibvh.traverse(g, cache=t)))  # the enqueue path: device total + pinned host total
    assert scans_in(names) == want, (route, n, names)
    assert holder["t2"].num_contacts == len(exp), (route, n)
    assert (contacts_np(holder["t2"]) == exp).all(), (route, n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("route", ROUTES)
def test_self_lists_in_order_on_every_route(knob, route, n):
    knob("lvt_scan_fused", route)
    check_self(route, n)


def test_the_sizes_reach_both_one_kernel_routes():
    """what the table above is for: groups of 3 + 2 tiles under knob 2, of 3 + 3 + 1 under knob 3, one tile kernel at <= 4,096"""
    assert expected_scan(2, 20_000) == expected_scan(3, 28_669) == expected_scan(3, 12_293) == {"scan_fused_grouped_kernel"}
    assert all(expected_scan(r, n) == {"scan_fused_kernel"} for r in (1, 2, 3) for n in (1, 4095, 4096))
    assert expected_scan(2, 4097) == expected_scan(3, 12_288) == {"scan_fused_kernel"}
    assert -(-20_000 // TILE) == 5 and -(-28_669 // TILE) == 7 and -(-12_293 // TILE) == 4


@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("n", [12_293, 28_669])
@pytest.mark.parametrize("route", ROUTES)
def test_both_index_types(knob, route, n, index):
    knob("lvt_scan_fused", route)
    o, g, exp, _ = cloud(n, index)
    assert g.struct().types.index_type == INDEX_TYPES[index]
    check_self(route, n, index)
    assert ibvh.traverse(g).contacts.dtype == (torch.int64 if index == "i64" else torch.int32)


@functools.lru_cache(maxsize=None)
def pair_case():
    o1, g1, _, _ = cloud(12_293)
    rng = np.random.default_rng(77)
    o2, g2 = build_both(random_volumes(rng, 4102, abi.BSPHERE, abi.F32, scale=0.9 * 12_293 ** (1 / 3)), abi.make_types())
    return g1, g2, oracle_pairs(orc.traverse_pair_lvt(o1, o2)[0]), oracle_pairs(orc.traverse_pair_lvt(o2, o1)[0])


@pytest.mark.parametrize("route", ROUTES)
def test_a_pair_walk(knob, route):
    knob("lvt_scan_fused", route)
    g1, g2, exp12, exp21 = pair_case()
    assert len(exp12) > 4102
    for ga, gb, exp in ((g1, g2, exp12), (g2, g1, exp21)):  # (the 12,293 leaves drive both times: one scan item each)
        names = _kernels_of(lambda: ibvh.traverse(ga, gb))
        assert scans_in(names) == expected_scan(route, 12_293), (route, names)
        t = ibvh.traverse(ga, gb)
        assert t.num_contacts == len(exp)
        assert (contacts_np(t) == exp).all()
        assert (contacts_np(ibvh.traverse(ga, gb, cache=t)) == exp).all()


@pytest.mark.parametrize("route", ROUTES)
def test_a_walker_that_zeroes_no_aggregates_gets_the_two_launch_scan(knob, route):
    """Two single-leaf trees: the pair walk starts at the leaf level, the exact joint walk serves it and the scan of its ONE count
    is reduce + apply on every setting of the knob."""
    knob("lvt_scan_fused", route)
    types = abi.make_types()
    o1, g1 = build_both(np.array([[0.0, 0.0, 0.0, 1.0]], np.float32), types)
    o2, g2 = build_both(np.array([[0.5, 0.0, 0.0, 1.0]], np.float32), types)
    exp = oracle_pairs(orc.traverse_pair_lvt(o1, o2)[0])
    assert len(exp) == 1
    names = _kernels_of(lambda: ibvh.traverse(g1, g2))
    assert scans_in(names) == expected_scan(route, 1, zeroed=False), names
    t = ibvh.traverse(g1, g2)
    assert t.num_contacts == 1 and (contacts_np(t) == exp).all()
    assert (contacts_np(ibvh.traverse(g1, g2, cache=t)) == exp).all()


@pytest.mark.parametrize("route", ROUTES)
def test_a_counts_pointer_off_16_byte_alignment(knob, route):
    """counts one element into an Int32 tensor: every thread takes the guarded loads and stores; the elements on either side of
    the n counts stay as they were."""
    knob("lvt_scan_fused", route)
    n = 12_293
    o, g, exp, scanned = cloud(n)
    s = g.struct()
    nbytes = C.c_size_t()
    lib.call("ibvh_lvt_scratch_bytes", C.byref(g.types), n, 8, C.byref(nbytes))
    buf = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    buf[0], buf[n + 1] = 123_456_789, -987_654_321
    counts = buf[1:n + 1]
    assert counts.data_ptr() % 16 == 4
    scratch = torch.zeros(nbytes.value, dtype=torch.uint8, device="cuda")
    total = C.c_int64()
    names = _kernels_of(lambda: lib.call("ibvh_traverse_lvt_count", C.byref(s), 1, 0, counts.data_ptr(), C.byref(total),
                                         scratch.data_ptr(), nbytes.value, None))
    assert scans_in(names) == expected_scan(route, n), (route, names)
    assert total.value == len(exp) == int(scanned[-1])
    assert (counts.cpu().numpy() == scanned).all()
    out = torch.zeros((total.value, 2), dtype=torch.int32, device="cuda")
    lib.call("ibvh_traverse_lvt_write", C.byref(s), 1, 0, counts.data_ptr(), out.data_ptr(), scratch.data_ptr(), nbytes.value, None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().astype(np.int64) == exp).all()
    assert int(buf[0]) == 123_456_789 and int(buf[n + 1]) == -987_654_321
    assert (counts.cpu().numpy() == scanned).all()  # (the writing pass reads them only)


@functools.lru_cache(maxsize=None)
def ray_case(index):
    """4,097 leaves under 2,500 rays (tests/test_gpu_rays_binned.py's small size): 2,500 per-ray item counts (one tile) and
    a 40,000-slot item list (ten tiles) whose length in use is known only on the device"""
    rng = np.random.default_rng(41)
    vols = random_volumes(rng, 4097, abi.BSPHERE, abi.F32, scale=20.0)
    o, g = build_both(vols, abi.make_types(index_type=INDEX_TYPES[index]))
    p, d = _rays(rng, 2500, 20)
    with np.errstate(all="ignore"):
        exp = oracle_pairs(orc.traverse_rays_lvt(o, p, d)[0]).reshape(-1, 2)
    return g, cuda(p).t(), cuda(d).t(), exp


@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("route", ROUTES)
def test_the_device_side_length_of_the_binned_ray_path(knob, route, index):
    knob("rays_binned", 2)
    knob("lvt_scan_fused", route)
    g, P, D, exp = ray_case(index)
    assert len(exp) > 1000
    names = _kernels_of(lambda: ibvh.traverse_rays(g, P, D))
    assert any("rays_top_kernel" in k for k in names) and any("rays_subtree_kernel" in k for k in names), names  # the binned path ran
    # the scan over the rays' item counts, then the one over the items' hits with limit = the items in use (the binned path zeroes
    # the aggregates of both), then the per-ray hit counts' own scan behind rays_counts_kernel, which zeroes nothing
    want = expected_scan(route, 2500) | expected_scan(route, 2500 * 16) | expected_scan(route, 2500, zeroed=False)
    assert scans_in(names) == want, (route, names)
    scans = [k for name in names for k in SCAN_KERNELS if k in name]
    assert len(scans) == (6 if route == 0 else 4), scans  # three scans: 2 + 2 + 2 launches, or 1 + 1 + 2
    t = ibvh.traverse_rays(g, P, D)
    assert t.num_contacts == len(exp)
    assert (contacts_np(t).reshape(-1, 2) == exp).all()
    t2 = ibvh.traverse_rays(g, P, D, cache=t)
    assert (contacts_np(t2).reshape(-1, 2) == exp).all()
