"""The cross-shard contact completion (ibvh_dist_cross_plan / _exchange / _count / _write, csrc/ibvh_distdrv.hip) on the
device, on every leaf / node / index / code type and on shard shapes the product's Morton slices of a smooth cloud never
have: what the plan says (the boxes a slice is described by, who touches whom, who sends how much), what travels (the
export and import buffers, record by record), and the contacts, ORIENTED (own slice, other slice) and GROUPED by imported
set, before anything is folded.

Ranks are in-process virtual ranks (tools/virtual_ranks.py).  Their BVHs come from (A) the product's distributed build, or
(B) an ordinary BVH per rank over volumes wrapped with global indices — any shard geometry.  Expected values never come
from the library: descriptions and export bounds from tests/dist_cross_checker.py on the oracle's trees, contacts from the
oracle (tests/test_host_dist_cross.py proves on the same inputs that they are unambiguous and not vacuous).  Every
comparison is exact; every device buffer is exactly as large as the plan says, with 64 guard bytes behind it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import dist_cross_checker as chk
import oracle_lib as orc
from dist_cross_oracle import brute_pairs, oracle_tree, pair_codes, types_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd import dist as ibd  # noqa: E402
from test_gpu_parity import TOKENS, cuda, make_options  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from virtual_ranks import run_virtual_ranks  # noqa: E402

GUARD = 0x5A
GUARD_BYTES = 64


def guarded(nbytes):
    return torch.full((int(nbytes) + GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")


def intact(buf, nbytes):
    return bool((buf[int(nbytes):] == GUARD).all().item())


def same_records(a, b):
    """Two leaf record arrays hold the same volumes, indices and codes (padding bytes are not data)."""
    return a.dtype == b.dtype and len(a) == len(b) and all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)


def by_index(raw, ldt):
    """The records in a byte buffer as rows of bytes, ordered by their index field (the indices are distinct)."""
    return raw.reshape(-1, ldt.itemsize)[np.argsort(raw.view(ldt)["index"], kind="stable")]


def node_type_of(types):
    return TOKENS[types.node_kind](torch.float32 if types.node_float == abi.F32 else torch.float64)


def plan_to_host(plan):
    P = plan.size
    out = {f: int(getattr(plan, f)) for f in ("size", "rank", "n_recv", "cache_slots", "import_bytes", "scratch_bytes", "export_bytes",
                                               "build_offset")}
    for f in ("recv_rank", "recv_leaves", "recv_offset", "scratch_offset"):
        out[f] = np.array(getattr(plan, f)[:plan.n_recv], dtype=np.int64)
    for f in ("slice_leaves", "touches", "send_leaves", "send_offset", "n_boxes"):
        out[f] = np.array(getattr(plan, f)[:P], dtype=np.int64)
    out["boxes"] = np.ctypeslib.as_array(plan.boxes)[:P].copy()  # (P, 16, 6) float64
    return out


def cross_by_hand(vt, bvh, cache_slots, stop_after_exchange=False):
    """The four C calls in the order DistributedBuilder.cross_contacts makes them, same vt.begin() / vt.check() protocol,
    every device buffer exactly the size the plan names + guard bytes.  -> dict: plan (host copy), export (the export
    buffer's bytes after _exchange), imported (the imported leaf records after _exchange, before _count rebuilds them in
    place), totals, contacts, guards (all intact?)."""
    L = lib.load()
    P = vt.comm.size
    s = bvh.struct()
    lay = abi.Layout()
    lib.call("ibvh_layout_of", C.byref(bvh.types), C.byref(lay))
    small_bytes = abi.dist_cross_scratch(P)
    small = guarded(small_bytes)
    plan = abi.DistCrossPlan()
    vt.begin()
    vt.check("ibvh_dist_cross_plan", L.ibvh_dist_cross_plan(C.byref(vt.struct), C.byref(s), cache_slots, api._ptr(small), small_bytes, C.byref(plan),
                                                            api._stream()))
    exp, imp = guarded(plan.export_bytes), guarded(plan.import_bytes)
    vt.check("ibvh_dist_cross_exchange", L.ibvh_dist_cross_exchange(C.byref(vt.struct), C.byref(s), C.byref(plan), api._ptr(exp), api._ptr(imp),
                                                                    api._ptr(small), small_bytes, api._stream()))
    torch.cuda.synchronize()
    out = {"plan": plan_to_host(plan), "export": exp[:plan.export_bytes].cpu().numpy().copy()}
    received = int(sum(plan.recv_leaves[k] for k in range(plan.n_recv)) * lay.leaf_bytes)
    out["imported"] = imp[:received].cpu().numpy().copy()
    out["guards"] = intact(small, small_bytes) and intact(exp, plan.export_bytes)
    if stop_after_exchange:
        out["guards"] = out["guards"] and intact(imp, plan.import_bytes)
        return out
    totals = (C.c_int64 * abi.DIST_MAX_RANKS)()
    total = C.c_int64(-1)
    idt = api._torch_index(bvh.types.index_type)
    if plan.n_recv == 0:  # nothing imported: no buffer is needed, and none is given
        abi.check(L.ibvh_dist_cross_count(C.byref(s), C.byref(plan), None, None, 0, totals, C.byref(total), api._stream()), "count (NULL)")
        assert total.value == 0 and plan.import_bytes == 0
        abi.check(L.ibvh_dist_cross_write(C.byref(s), C.byref(plan), None, None, 0, totals, None, api._stream()), "write (NULL)")
        torch.cuda.synchronize()
        out["totals"], out["contacts"] = np.zeros(0, np.int64), np.zeros((0, 2), abi.INDEX_DTYPES[bvh.types.index_type])
        out["guards"] = out["guards"] and intact(imp, 0)
        return out
    scratch = guarded(plan.scratch_bytes)
    abi.check(L.ibvh_dist_cross_count(C.byref(s), C.byref(plan), api._ptr(imp), api._ptr(scratch), int(plan.scratch_bytes), totals, C.byref(total),
                                      api._stream()), "ibvh_dist_cross_count")
    out["totals"] = np.array(totals[:plan.n_recv], dtype=np.int64)
    assert total.value == out["totals"].sum()
    esz = 8 if bvh.types.index_type == abi.I64 else 4
    assert lay.pair_bytes == 2 * esz
    contacts = guarded(total.value * lay.pair_bytes)
    # (imported leaves without a single contact among them: _write has nothing to write and takes a NULL contacts_out)
    abi.check(L.ibvh_dist_cross_write(C.byref(s), C.byref(plan), api._ptr(imp), api._ptr(scratch), int(plan.scratch_bytes), totals,
                                      api._ptr(contacts) if total.value > 0 else None, api._stream()), "ibvh_dist_cross_write")
    torch.cuda.synchronize()
    out["contacts"] = contacts[:total.value * lay.pair_bytes].view(idt).reshape(-1, 2).cpu().numpy().copy()
    out["guards"] = (out["guards"] and intact(imp, plan.import_bytes) and intact(scratch, plan.scratch_bytes)
                     and intact(contacts, total.value * lay.pair_bytes))
    return out


# ---------------------------------------------------------------------------------------------
# the ranks
# ---------------------------------------------------------------------------------------------
def run_case(case, cache_slots=api.LVT_CACHE_SLOTS, stop_after_exchange=False, also_binding=False):
    """-> per rank: the dict of cross_by_hand + leaves (the rank's sorted leaf records), nodes, last (path A: builder.last),
    binding (also_binding: what DistributedBuilder.cross_contacts returns on the same BVH)."""
    types = types_of(case)
    opts, node_type = make_options(types), node_type_of(types)
    dev = [cuda(s) for s in case.shards]

    def fn(comm):
        r = comm.rank
        if case.path == "A":
            builder = ibd.DistributedBuilder(comm)
            bvh = builder.build(dev[r], node_type, options=opts)
            vt = builder.vtable
        else:
            builder = None
            idx = case.base[r] + 1 + np.arange(len(case.shards[r]))
            bvh = ibvh.BVH(ibvh.BoundingVolumes.wrap(dev[r], idx, opts), node_type, options=opts)
            vt = ibd.CommVtable(comm)
        torch.cuda.synchronize()
        raw, nodes = bvh.leaves.buf.cpu().numpy(), bvh.nodes.cpu().numpy()  # (bytes: copying a structured array drops its padding)
        leaves = raw.view(abi.leaf_dtype(types))
        out = cross_by_hand(vt, bvh, cache_slots, stop_after_exchange)
        out.update(leaves=leaves, nodes=nodes, last=builder.last if builder else None)
        assert bvh.leaves.buf.cpu().numpy().tobytes() == raw.tobytes() and bvh.nodes.cpu().numpy().tobytes() == nodes.tobytes()  # (the own tree stays)
        if also_binding:
            got = (builder or ibd.DistributedBuilder(comm)).cross_contacts(bvh, cache_slots=cache_slots)
            torch.cuda.synchronize()
            out["binding"] = got.cpu().numpy()
            out["binding_dtype"] = got.dtype
        return out
    return run_virtual_ranks(case.world, fn)


def oracle_trees_and_expected(case, out):
    """-> (the oracle's tree of every rank's slice, {(r, s): sorted codes of the expected (index in r, index in s) pairs}, r < s).
    Path A first checks the criterion of test_distributed_build_virtual_ranks_gpu: the concatenated slices are the
    single-device sorted leaves, byte for byte, and every rank built with the single-device extrema."""
    W, types = case.world, types_of(case)
    if case.path == "B":
        trees = [oracle_tree(case, r) for r in range(W)]
        return trees, {(r, s): brute_pairs(case, r, s) for r in range(W) for s in range(r + 1, W)}
    cloud = np.concatenate(case.shards)
    single = orc.build(cloud, types)
    assert same_records(np.concatenate([o["leaves"] for o in out]), single.leaves)
    trees, owner = [], np.full(len(cloud) + 1, -1)
    for r, o in enumerate(out):
        assert o["last"]["extrema"].tobytes() == single.extrema.tobytes()
        v = o["leaves"]["volume"]
        flat = np.ascontiguousarray(v).view(v.dtype[0].base).reshape(len(v), -1)
        trees.append(orc.build(flat, types, indices=o["leaves"]["index"], compute_extrema=False, mins=single.extrema[:3], maxs=single.extrema[3:]))
        owner[o["leaves"]["index"]] = r
    whole = orc.traverse_lvt(single)[0]  # (== all pairs tried: test_host_dist_cross.py)
    a, b = whole["a"].astype(np.int64), whole["b"].astype(np.int64)
    swap = owner[a] > owner[b]
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    expected = {(r, s): pair_codes(a[(owner[a] == r) & (owner[b] == s)], b[(owner[a] == r) & (owner[b] == s)])
                for r in range(W) for s in range(r + 1, W)}
    assert sum(len(e) for e in expected.values()) > 0
    return trees, expected


def standard_checks(case, out, trees, expected=None):
    W, types = case.world, types_of(case)
    ldt = abi.leaf_dtype(types)
    lb = ldt.itemsize
    n_global = sum(len(o["leaves"]) for o in out)
    plans = [o["plan"] for o in out]
    rel = chk.export_cap(case.combo[1], case.combo[3])
    assert all(o["guards"] for o in out), "guard bytes behind a buffer were written"
    # the library's trees are the oracle's (pinned elsewhere; everything below leans on it)
    for r in range(W):
        assert same_records(out[r]["leaves"], trees[r].leaves) and out[r]["nodes"].tobytes() == trees[r].nodes.tobytes(), r
    # ---- the plan: the same on every rank, the checker's description of every slice, who touches whom
    desc = []
    for r in range(W):
        report = {}
        desc.append(chk.describe(trees[r].nodes, trees[r].leaves, trees[r].tree, types, report))
        assert report["ties"] == 0, r
    for me, p in enumerate(plans):
        assert (p["size"], p["rank"]) == (W, me)
        assert p["slice_leaves"].tolist() == [len(o["leaves"]) for o in out]
        assert p["n_boxes"].tolist() == [len(d) for d in desc], me
        assert p["boxes"].tobytes() == plans[0]["boxes"].tobytes(), me
        for r in range(W):
            assert p["boxes"][r, :len(desc[r])].tobytes() == desc[r].tobytes(), (me, r)
            assert p["touches"][r] == (1 if r != me and chk.touches(desc[me], desc[r]) else 0), (me, r)
            assert p["touches"][r] == plans[r]["touches"][me], (me, r)
    # ---- export: per lower rank distinct records of the own leaf array, between the two bounds; nothing for the others
    own_boxes = [chk.volume_boxes(o["leaves"]["volume"], case.combo[0]) for o in out]
    for me, (o, p) in enumerate(zip(out, plans)):
        where = np.full(n_global + 1, -1)
        where[o["leaves"]["index"]] = np.arange(len(o["leaves"]))
        at = 0
        for r in range(W):
            k = int(p["send_leaves"][r])
            assert p["send_offset"][r] == at, (me, r)
            if r >= me or not p["touches"][r]:
                assert k == 0, (me, r)
                continue
            seg = o["export"][at:at + k * lb]
            pos = where[seg.view(ldt)["index"]]
            assert (pos >= 0).all() and len(np.unique(pos)) == k, (me, r)
            assert np.array_equal(o["leaves"].view(np.uint8).reshape(-1, lb)[pos], seg.reshape(k, lb)), (me, r)
            sent = np.zeros(len(o["leaves"]), bool)
            sent[pos] = True
            must, may = chk.must_export(own_boxes[me], desc[r]), chk.may_export(own_boxes[me], desc[r], rel)
            assert not (must & ~sent).any(), f"rank {me} keeps back {int((must & ~sent).sum())} leaves rank {r} needs"
            assert not (sent & ~may).any(), f"rank {me} sends rank {r} {int((sent & ~may).sum())} leaves beyond the cap"
            at += k * lb
        assert p["export_bytes"] == at == len(o["export"]), me
    # ---- import: the higher ranks that sent something, ascending; each set is the sender's segment, as a multiset
    for me, (o, p) in enumerate(zip(out, plans)):
        senders = [s for s in range(me + 1, W) if plans[s]["send_leaves"][me] > 0]
        assert p["recv_rank"].tolist() == senders and p["n_recv"] == len(senders), me
        assert p["recv_leaves"].tolist() == [int(plans[s]["send_leaves"][me]) for s in senders], me
        assert p["recv_offset"].tolist() == [int(v) for v in np.concatenate([[0], np.cumsum(p["recv_leaves"] * lb)[:-1]])][:len(senders)], me
        assert (p["import_bytes"] == 0) == (len(senders) == 0) and p["import_bytes"] >= p["recv_leaves"].sum() * lb, me
        for k, s in enumerate(senders):
            got = o["imported"][p["recv_offset"][k]:p["recv_offset"][k] + p["recv_leaves"][k] * lb]
            ps = plans[s]
            sent = out[s]["export"][ps["send_offset"][me]:ps["send_offset"][me] + ps["send_leaves"][me] * lb]
            assert np.array_equal(by_index(got, ldt), by_index(sent, ldt)), (me, s)
    if expected is None:
        return desc
    # ---- contacts: grouped by imported set, (own, other), the expected set, nothing twice
    for me, (o, p) in enumerate(zip(out, plans)):
        assert o["contacts"].dtype == abi.INDEX_DTYPES[types.index_type] and o["contacts"].shape == (o["totals"].sum(), 2), me
        assert len(o["totals"]) == p["n_recv"]
        at = 0
        for k, s in enumerate(p["recv_rank"].tolist()):
            rows = o["contacts"][at:at + o["totals"][k]]
            assert np.isin(rows[:, 0], out[me]["leaves"]["index"]).all(), (me, s)
            assert np.isin(rows[:, 1], out[s]["leaves"]["index"]).all(), (me, s)
            assert np.array_equal(pair_codes(rows[:, 0], rows[:, 1]), expected[me, s]), (me, s)
            at += o["totals"][k]
        for s in range(me + 1, W):
            if s not in p["recv_rank"].tolist():
                assert len(expected[me, s]) == 0, (me, s)
    for r, s in case.cross:
        assert len(expected[r, s]) > 0
    return desc


def run_and_check(case, **kw):
    out = run_case(case, **kw)
    trees, expected = oracle_trees_and_expected(case, out)
    standard_checks(case, out, trees, expected)
    return out


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", chk.case_names(prefix="types-"))
def test_every_type_combination_on_overlapping_slabs(name):
    """12 leaf / node combinations, three of them also with (Int64, UInt64) and (Int32, UInt16): three slabs of one cloud,
    each exports a shell to the slab below it and nothing to the one after that."""
    case = chk.case(name)
    out = run_and_check(case)
    assert out[1]["plan"]["touches"].tolist() == [1, 0, 1]
    if case.combo[2] == chk.BBOX:  # (the boxes of sphere nodes are fat: slabs 0 and 2 touch, and no leaf travels between them)
        assert out[2]["plan"]["touches"].tolist() == [0, 1, 0]
    assert out[2]["plan"]["send_leaves"][0] == 0 and out[0]["plan"]["recv_rank"].tolist() == [1]
    for s, r in ((1, 0), (2, 1)):
        assert 0 < out[s]["plan"]["send_leaves"][r] < (len(out[s]["leaves"]) // 2 if case.combo[2] == chk.BBOX else len(out[s]["leaves"]))


@pytest.mark.parametrize("name", chk.case_names(path="A"))
def test_product_path_on_types_it_has_never_seen(name):
    """DistributedBuilder.build (ibvh_dist_plan / _exchange) on box leaves, Float64 leaves with UInt64 codes and Int64
    indices, Float64 spheres under Float32 boxes and UInt16 codes: Morton slices of a clustered cloud."""
    out = run_and_check(chk.case(name))
    assert sum(len(o["contacts"]) for o in out) > 0


def test_everything_overlaps_so_every_leaf_travels_and_rank_0_imports_three_sets():
    out = run_and_check(chk.case("everything-overlaps"))
    for me, o in enumerate(out):
        assert o["plan"]["send_leaves"].tolist() == [800 if r < me else 0 for r in range(4)]
    assert out[0]["plan"]["recv_rank"].tolist() == [1, 2, 3] and (out[0]["totals"] > 0).all()
    assert len(set(out[0]["plan"]["scratch_offset"].tolist())) == 3


def test_nothing_touches_so_nothing_travels_and_null_buffers_are_fine():
    out = run_and_check(chk.case("nothing-touches"), also_binding=True)
    for o in out:
        p = o["plan"]
        assert not p["touches"].any() and p["export_bytes"] == p["import_bytes"] == p["n_recv"] == 0
        assert o["contacts"].shape == (0, 2)
        assert tuple(o["binding"].shape) == (0, 2) and o["binding_dtype"] == torch.int32


@pytest.mark.parametrize("m", [1, 2, 3])
def test_bridge_of_one_two_three_leaves_is_a_tree_built_inside_the_import_buffer(m):
    out = run_and_check(chk.case(f"bridge-{m}"))
    assert out[0]["plan"]["recv_leaves"].tolist() == [m] and out[0]["totals"][0] > 0


@pytest.mark.parametrize("name", ["sizes-1-2-3-5-33", "sizes-40-3000", "sizes-3000-40"])
def test_tiny_and_uneven_shards_keep_the_orientation(name):
    """One-leaf slices, virtual children, refinement that ends at the last node level; then an imported set larger, and
    smaller, than the own slice: the smaller side drives the traversal, the pairs stay (own, other)."""
    out = run_and_check(chk.case(name))
    if name == "sizes-1-2-3-5-33":
        assert out[0]["plan"]["n_boxes"].tolist() == [1, 1, 2, 3, 16]
    else:
        own, got = len(out[0]["leaves"]), int(out[0]["plan"]["recv_leaves"][0])
        assert (got > own) == (name == "sizes-40-3000") and got != own and out[0]["totals"][0] > 0


@pytest.mark.parametrize("name,zero", [("zero-contact-set-last", [False, True]), ("zero-contact-set-first", [True, False]),
                                       ("zero-contact-sets-only", [True, True])])
def test_imported_sets_without_a_contact(name, zero):
    """Leaves inside rank 0's boxes that touch none of its leaves: a total of 0 after, before, and instead of a set with
    contacts (the last: _write has nothing to do and takes a NULL contacts_out)."""
    out = run_and_check(chk.case(name))
    assert out[0]["plan"]["recv_rank"].tolist() == [1, 2] and (out[0]["plan"]["recv_leaves"] > 0).all()
    assert (out[0]["totals"] == 0).tolist() == zero
    if all(zero):
        assert out[1]["plan"]["n_recv"] == 1 and out[1]["totals"].tolist() == [0]


@pytest.mark.parametrize("name", ["flat-shard", "abutting-unit-boxes", "translated-B32-B32-i32-u32", "translated-S64-B32-i32-u32",
                                  "infinite-radius-in-shard-0", "infinite-radius-in-shard-1"])
def test_degenerate_geometry(name):
    out = run_and_check(chk.case(name))
    if name == "flat-shard":
        assert out[0]["plan"]["n_boxes"].tolist() == [1, 16]
    if name == "abutting-unit-boxes":  # the leaves that travel are exactly the layer behind the cut
        assert 0 < out[1]["plan"]["send_leaves"][0] <= 16
    if name.startswith("infinite"):
        which = int(name[-1])
        assert np.isinf(out[0]["plan"]["boxes"][which]).any() and out[0]["totals"][0] >= len(out[1 - which]["leaves"])


@pytest.mark.parametrize("name", ["sizes-40-3000", "types-B32-B32-i32-u32"])
def test_cache_slots_zero_and_the_binding_give_the_same_set(name):
    """cache_slots = 0 (another scratch carving; the default runs everywhere else), and DistributedBuilder.cross_contacts on
    the same BVHs: the same pairs."""
    case = chk.case(name)
    out = run_and_check(case, cache_slots=0, also_binding=True)
    assert all(o["plan"]["cache_slots"] == 0 for o in out)
    for o in out:
        assert o["binding"].shape == o["contacts"].shape
        assert np.array_equal(pair_codes(o["binding"][:, 0], o["binding"][:, 1]), pair_codes(o["contacts"][:, 0], o["contacts"][:, 1]))


def test_second_grid_stride_trip_of_the_filter():
    """2,200,000 leaves: more than the filter's 8192 workgroups of 256 cover in one trip.  _plan and _exchange only."""
    case = chk.stride_case()
    out = run_case(case, stop_after_exchange=True)
    trees = [oracle_tree(case, r) for r in range(2)]
    standard_checks(case, out, trees)
    ldt = abi.leaf_dtype(types_of(case))
    sent = out[1]["export"].view(ldt)["index"]
    where = np.full(case.base[1] + len(case.shards[1]) + 1, -1)
    where[out[1]["leaves"]["index"]] = np.arange(len(out[1]["leaves"]))
    pos = where[sent]
    assert (pos < 8192 * 256).any() and (pos >= 8192 * 256).any()
