"""IBVH_PAIR_MIXED_TYPES on the device: pair LVT traversals of two BVHs of different leaf / node / Morton types.  Every list
equals, order included, the numpy restatement of the reference's walk (tests/mixed_pair_checker.py, pinned to the oracle by
tests/test_host_mixed_pair.py) evaluated on the BVHs the device built; the one combination the reference has no conversion for
(a BBox query against BSphere nodes) is refused, never answered with a list."""
import ctypes as C

import numpy as np
import pytest

import mixed_pair_checker as mpc
import oracle_lib as orc

torch = pytest.importorskip("torch")

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

pytestmark = pytest.mark.gpu

TOKENS = {abi.BSPHERE: ibvh.BSphere, abi.BBOX: ibvh.BBox}
TORCH_F = {abi.F32: torch.float32, abi.F64: torch.float64}
MORTONS = (abi.U16, abi.U32, abi.U64)
COMBOS = mpc.LEAF_NODE_COMBOS
# size pairs (n1, n2), dealt round robin to the ordered type pairs (the checker's time grows with n1 * n2)
SIZES = ((1, 50), (50, 1), (190, 22), (1000, 777), (22, 190), (777, 1000), (3000, 2500), (50, 1), (190, 22), (1000, 777),
         (1, 50), (2500, 3000))


def combo_id(c):
    return "%s%d%s%d" % ("SB"[c[0]], 32 << c[1], "SB"[c[2]], 32 << c[3])


class Built:
    """A BVH built on the device and the same BVH as host records for the checker (the device's own leaves and nodes)."""

    def __init__(self, vols, types, built_level):
        lk, lf, nk, nf = types.leaf_kind, types.leaf_float, types.node_kind, types.node_float
        opts = ibvh.BVHOptions(index=abi.INDEX_DTYPES[types.index_type], morton=ibvh.DefaultMortonAlgorithm(abi.MORTON_DTYPES[types.morton_type]))
        self.g = ibvh.BVH(torch.from_numpy(vols).cuda(), TOKENS[nk](TORCH_F[nf]), built_level=built_level, options=opts)
        assert self.g.types.key() == types.key()
        n = len(vols)
        nodes = np.ascontiguousarray(self.g.nodes.cpu().numpy()).view(abi.node_dtype(types)).reshape(-1)
        self.h = orc.HostBVH(types, orc.tree_shape(n), self.g.built_level, self.g.leaves.to_numpy(), nodes, None, None)


def host_of(g):
    """A device-built BVH as oracle_lib.HostBVH records (its own leaves and nodes; skips computed): the oracle walks it."""
    t, tree = g.types, orc.tree_shape(len(g.leaves))
    nodes = np.ascontiguousarray(g.nodes.cpu().numpy()).view(abi.node_dtype(t)).reshape(-1)
    skips = orc.compute_skips(tree).astype(abi.INDEX_DTYPES[t.index_type])
    return orc.HostBVH(t, tree, g.built_level, np.ascontiguousarray(g.leaves.to_numpy()), nodes, skips, None)


def oracle_list(h1, h2, code=0):
    """The oracle's mixed list (IBVH_PAIR_MIXED_TYPES) of two HostBVHs as an (m, 2) int64 array."""
    c = orc.traverse_pair_lvt(h1, h2, narrow=code | abi.PAIR_MIXED_TYPES)[0]
    return np.stack([c["a"], c["b"]], axis=1).astype(np.int64) if len(c) else np.zeros((0, 2), np.int64)


_built = {}


def built(k, n, idx, morton, seed_shift=0):
    """BVH number k of COMBOS with n leaves: clouds of every type fill the same box, so any two of them overlap."""
    key = (k, n, idx, morton, seed_shift)
    if key not in _built:
        lk, lf, nk, nf = COMBOS[k]
        rng = np.random.default_rng(1 + 97 * k + n + 13 * idx + 7 * morton + seed_shift)
        vols = mpc.random_volumes(rng, n, lk, lf, scale=10.0, size=0.45 * (1000.0 / max(n, 1000)) ** (1 / 3))
        levels = orc.tree_shape(n).levels
        bl = 2 if (k % 3 == 0 and levels >= 4) else 1  # (built_level > 1: the nodes above it do not exist)
        _built[key] = Built(vols, abi.make_types(lk, lf, nk, nf, idx, morton), bl)
    return _built[key]


def contacts_np(t):
    return t.contacts.cpu().numpy().astype(np.int64).reshape(-1, 2)


def refused(b1, b2, smaller):
    flip = mpc.driver_of(b1.h, b2.h, smaller)
    drv, oth = (b2, b1) if flip else (b1, b2)
    return drv.h.types.leaf_kind == abi.BBOX and oth.h.types.node_kind == abi.BSPHERE


@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["i32", "i64"])
def test_every_ordered_type_pair_equals_the_checker(idx):
    """All 144 ordered pairs of the 12 instantiated (leaf, node) types, the second BVH always with another Morton width (so
    every pair is a pair of two types, also where leaf and node types agree); sizes dealt from (1, 50), (50, 1), (190, 22),
    (1000, 777), (3000, 2500) in both orientations; start levels drawn between built_level and levels; built_level 2 for a
    third of the types; every narrow code; positions output, smaller-drives and the cache= / enqueue path in rotation.
    Lists equal the checker's, order included; the refused combination raises the reference's MethodError."""
    rng = np.random.default_rng(40 + idx)
    case = 0
    ran = refusals = 0
    for k1 in range(len(COMBOS)):
        for k2 in range(len(COMBOS)):
            n1, n2 = SIZES[(k1 * len(COMBOS) + k2 + 5 * idx) % len(SIZES)]
            m1 = MORTONS[(k1 + k2) % 3]
            m2 = MORTONS[(k1 + k2 + 1) % 3]
            b1, b2 = built(k1, n1, idx, m1), built(k2, n2, idx, m2)
            case += 1
            narrow = (abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT)[case % 3]
            positions = case % 4 == 1
            smaller = case % 5 == 2
            use_cache = case % 6 == 3
            sl1 = int(rng.integers(b1.h.built_level, b1.h.tree.levels + 1))
            sl2 = int(rng.integers(b2.h.built_level, b2.h.tree.levels + 1))
            code = narrow | (abi.OUTPUT_POSITIONS if positions else 0) | (abi.PAIR_SMALLER_DRIVES if smaller else 0)
            what = (combo_id(COMBOS[k1]), combo_id(COMBOS[k2]), n1, n2, sl1, sl2, narrow, positions, smaller, use_cache)
            if refused(b1, b2, smaller):
                with pytest.raises(abi.MethodError):
                    api._traverse_lvt_pair(b1.g, b2.g, sl1, sl2, code, None)
                refusals += 1
                continue
            exp = mpc.traverse_pair_lvt(b1.h, b2.h, sl1, sl2, narrow, positions=positions, smaller_drives=smaller)
            t = api._traverse_lvt_pair(b1.g, b2.g, sl1, sl2, code, None)
            got = contacts_np(t)
            assert got.shape == exp.shape and (got == exp).all(), what  # (smaller-drives: the checker's order for it too)
            if use_cache:  # enqueued against the previous traversal's buffers
                t2 = api._traverse_lvt_pair(b1.g, b2.g, sl1, sl2, code, t)
                again = contacts_np(t2)
                assert again.shape == exp.shape and (again == exp).all(), ("cache", what)
            ran += 1
    assert ran > 100 and refusals > 0


def test_public_traverse_mixed_types_and_its_refusals():
    """ibvh.traverse(bvh1, bvh2) with LVT (the default) accepts two types: a particle cloud in BSphere{Float32} against boxes
    in BBox{Float32}, both argument orders, with cache=; the refused combination raises abi.MethodError whichever argument
    order; BFS pairs of two types and two index types keep raising."""
    rng = np.random.default_rng(8)
    ts = abi.make_types(abi.BSPHERE, abi.F32, abi.BSPHERE, abi.F32)
    tb = abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32)
    spheres = Built(mpc.random_volumes(rng, 1500, abi.BSPHERE, abi.F32, 10.0, 0.5), abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32), 1)
    boxes = Built(mpc.random_volumes(rng, 900, abi.BBOX, abi.F32, 10.0, 0.5), tb, 1)
    for a, b in ((spheres, boxes), (boxes, spheres)):
        exp = mpc.traverse_pair_lvt(a.h, b.h)
        t = ibvh.traverse(a.g, b.g)
        assert (contacts_np(t) == exp).all() and len(exp) > 100
        t2 = ibvh.traverse(a.g, b.g, cache=t)
        assert (contacts_np(t2) == exp).all()
        assert t2.num_contacts == len(exp)
    with pytest.raises(ValueError):
        ibvh.traverse(spheres.g, boxes.g, ibvh.BFSTraversal())
    # BSphere nodes walked by a BBox query: no BSphere(::BBox) — refused whichever argument order when the boxes drive
    sph_nodes = Built(mpc.random_volumes(rng, 400, abi.BSPHERE, abi.F32, 10.0, 0.5), ts, 1)
    for a, b in ((boxes, sph_nodes), (sph_nodes, boxes)):
        with pytest.raises(abi.MethodError):
            ibvh.traverse(a.g, b.g)
    # ... but the same two types with the SPHERES driving (more leaves) are a pair the reference accepts
    many = Built(mpc.random_volumes(rng, 2000, abi.BSPHERE, abi.F32, 10.0, 0.5), ts, 1)
    exp = mpc.traverse_pair_lvt(boxes.h, many.h)
    assert (contacts_np(ibvh.traverse(boxes.g, many.g)) == exp).all() and len(exp) > 0
    # one index type (traverse_pair.jl:50-52)
    b64 = Built(mpc.random_volumes(rng, 300, abi.BBOX, abi.F32, 10.0, 0.5), abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32, abi.I64), 1)
    with pytest.raises(ValueError):
        ibvh.traverse(spheres.g, b64.g)


def test_abi_contract_of_the_flag():
    """Through the C ABI: without IBVH_PAIR_MIXED_TYPES two types return IBVH_ERR_UNSUPPORTED (as before); with it the count
    is the checker's; a BBox query against BSphere nodes and two index types return IBVH_ERR_UNSUPPORTED; scratch sized as
    the larger of ibvh_lvt_scratch_bytes over the two types."""
    rng = np.random.default_rng(9)
    sph = Built(mpc.random_volumes(rng, 1200, abi.BSPHERE, abi.F64, 10.0, 0.5), abi.make_types(abi.BSPHERE, abi.F64, abi.BSPHERE, abi.F32), 1)
    box = Built(mpc.random_volumes(rng, 700, abi.BBOX, abi.F32, 10.0, 0.5), abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F64, abi.I32, abi.U64), 1)
    box_big = Built(mpc.random_volumes(rng, 1500, abi.BBOX, abi.F32, 10.0, 0.5), abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32), 1)
    box_i64 = Built(mpc.random_volumes(rng, 100, abi.BBOX, abi.F32, 10.0, 0.5), abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32, abi.I64), 1)
    L = lib.load()

    def count(a, b, narrow):
        n = max(len(a.g.leaves), len(b.g.leaves))
        need = 0
        for t in (a.g.types, b.g.types):
            sz = C.c_size_t()
            lib.call("ibvh_lvt_scratch_bytes", C.byref(t), n, 8, C.byref(sz))
            need = max(need, sz.value)
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")  # (Int32 indices throughout)
        scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
        total = C.c_int64(-1)
        s1, s2 = a.g.struct(), b.g.struct()
        rc = L.ibvh_traverse_pair_lvt_count(C.byref(s1), C.byref(s2), a.h.built_level, b.h.built_level, narrow, counts.data_ptr(),
                                            C.byref(total), scratch.data_ptr(), scratch.numel(), None)
        torch.cuda.synchronize()
        return rc, total.value

    assert count(sph, box, 0)[0] == abi.ERR_UNSUPPORTED
    rc, total = count(sph, box, abi.PAIR_MIXED_TYPES)
    assert rc == abi.OK and total == len(mpc.traverse_pair_lvt(sph.h, box.h)) and total > 0
    rc, total = count(box, sph, abi.PAIR_MIXED_TYPES | abi.NARROW_MORTON_LT)
    assert rc == abi.OK and total == len(mpc.traverse_pair_lvt(box.h, sph.h, narrow=abi.NARROW_MORTON_LT))
    assert count(box_big, sph, abi.PAIR_MIXED_TYPES)[0] == abi.ERR_UNSUPPORTED   # the boxes drive: no BSphere(::BBox)
    assert count(sph, box_big, abi.PAIR_MIXED_TYPES)[0] == abi.ERR_UNSUPPORTED
    assert count(sph, box_i64, abi.PAIR_MIXED_TYPES)[0] == abi.ERR_UNSUPPORTED   # two index types
    assert count(sph, box_big, abi.PAIR_MIXED_TYPES | abi.PAIR_SMALLER_DRIVES)[0] == abi.OK  # the spheres drive


def test_particles_against_the_published_surface():
    """2e5 BSphere{Float32} particles against the 249,882-triangle torus as BBox{Float32} leaves (a checker at this size would
    be slow): the contact set equals the same-type run with the particles given as their BBox{Float32} boxes (the box
    iscontact(::BSphere, ::BBox) forms), every contact passes the exact leaf test, and the two argument orders agree; and the
    lists equal the oracle's mixed walk in order, with the default knobs' shared descent."""
    from implicitbvh_amd.synthetic import sphere_radius_law, torus_mesh
    tris = torch.from_numpy(torus_mesh(354, 353)[:249_882].copy()).cuda()
    surf_vols = ibvh.bounding_volumes_from_triangles(tris, ibvh.BBox(torch.float32))
    surf = ibvh.BVH(surf_vols, ibvh.BBox(torch.float32))
    lo, hi = surf_vols[:, :3].min(0).values.cpu().numpy(), surf_vols[:, 3:].max(0).values.cpu().numpy()
    n = 200_000
    rng = np.random.default_rng(2)
    c = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    r = (sphere_radius_law(n) * float((hi - lo).max()) * (0.5 + 0.5 * rng.random((n, 1)))).astype(np.float32)
    sph_host = np.concatenate([c, r], axis=1)
    sph = ibvh.BVH(torch.from_numpy(sph_host).cuda(), ibvh.BBox(torch.float32))
    boxes_host = np.concatenate([c - r, c + r], axis=1)  # (Float32 arithmetic: the box iscontact forms)
    as_boxes = ibvh.BVH(torch.from_numpy(boxes_host).cuda(), ibvh.BBox(torch.float32))
    got = contacts_np(ibvh.traverse(sph, surf))
    want = contacts_np(ibvh.traverse(as_boxes, surf))
    assert len(got) > 10_000
    key = lambda a: np.sort(a[:, 0] * (1 << 32) + a[:, 1])  # noqa: E731
    assert len(got) == len(want) and (key(got) == key(want)).all()
    rev = contacts_np(ibvh.traverse(surf, sph))
    assert (key(rev[:, ::-1].copy()) == key(got)).all()
    sv = surf_vols.cpu().numpy()
    s, t = sph_host[got[:, 0] - 1], sv[got[:, 1] - 1]
    hit = np.ones(len(got), bool)
    for k in range(3):
        hit &= (s[:, k] + s[:, 3] >= t[:, k]) & (s[:, k] - s[:, 3] <= t[:, 3 + k])
    assert hit.all()
    # the full lists, in order, against the oracle's mixed walk: both argument orders and the particles driving
    # (IBVH_PAIR_SMALLER_DRIVES); more than 2^17 driving leaves and one node type, so the default knobs take the shared
    # descent (the profile shows lvt_block_frontier_kernel), the one-kernel scan and the dense .index copy
    from test_gpu_lvt_blocks import _kernels_of
    hs, ht = host_of(sph), host_of(surf)
    for (a, ha), (b, hb) in (((sph, hs), (surf, ht)), ((surf, ht), (sph, hs))):
        for code in (0, abi.PAIR_SMALLER_DRIVES):
            exp = oracle_list(ha, hb, code)
            names = _kernels_of(lambda: api._traverse_lvt_pair(a, b, 1, 1, code, None))
            assert any("lvt_block_frontier_kernel" in k for k in names), (code, names)
            t = api._traverse_lvt_pair(a, b, 1, 1, code, None)
            assert contacts_np(t).shape == exp.shape and (contacts_np(t) == exp).all(), code
            assert (contacts_np(api._traverse_lvt_pair(a, b, 1, 1, code, t)) == exp).all(), ("enqueue", code)
