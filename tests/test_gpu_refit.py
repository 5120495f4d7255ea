"""ibvh.refit / ibvh_refit on the device: new leaf volumes into a built BVH's EXISTING leaf order, nodes merged again.

The checker is the oracle, never the library: oracle_lib.aggregate merges any given leaf order, and an oracle HostBVH assembled
from the refitted leaves and those nodes runs every oracle traversal.  A refit must leave
  - leaf volumes = the new volumes of the leaves' user indices, byte for byte; .index / .morton and skips untouched;
  - nodes byte-identical to aggregate_oibvh! (build.jl:366-523) over the updated leaves;
and every traversal of the refitted tree must equal the oracle's on the same tree (LVT order included, BFS as sets) — also on
trees whose leaves are far from Morton order, which no build ever produces."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import mixed_pair_checker as mpc
import oracle_lib as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

TOKENS = {abi.BSPHERE: ibvh.BSphere, abi.BBOX: ibvh.BBox}
TORCH_F = {abi.F32: torch.float32, abi.F64: torch.float64}
COMBOS = mpc.LEAF_NODE_COMBOS
# (2^21 + 5 leaves: the first launch ends 9 levels up with more than AGG_TOP_MAX = 4096 nodes, so the middle
# aggregate_kernel launches run before the top one)
SIZES = (1, 2, 3, 5, 64, 1000, 4097, (1 << 16) + 3)
BIG = (1 << 21) + 5


def combo_id(c):
    return "%s%d%s%d" % ("SB"[c[0]], 32 << c[1], "SB"[c[2]], 32 << c[3])


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def options(types):
    return ibvh.BVHOptions(index=abi.INDEX_DTYPES[types.index_type], morton=ibvh.DefaultMortonAlgorithm(abi.MORTON_DTYPES[types.morton_type]))


def build(vols, types, built_level=1, indices=None):
    node = TOKENS[types.node_kind](TORCH_F[types.node_float])
    opts = options(types)
    if indices is None:
        g = ibvh.BVH(cuda(vols), node, built_level=built_level, options=opts)
    else:
        g = ibvh.BVH(ibvh.BoundingVolumes.wrap(cuda(vols), np.asarray(indices), opts), node, built_level=built_level, options=opts)
    assert g.types.key() == types.key()
    return g


def jitter(rng, vols, amount):
    out = vols.copy()
    out[:, :3] += (amount * (rng.random((len(vols), 3)) * 2 - 1)).astype(vols.dtype)
    if vols.shape[1] == 6:
        out[:, 3:] = np.maximum(out[:, 3:] + (out[:, :3] - vols[:, :3]), out[:, :3])
    return out


def new_volumes(rng, a, how):
    """B for a refit of a BVH built from A: A jittered, a random permutation of A (a maximally incoherent tree), or fresh."""
    kind, flt = (abi.BSPHERE if a.shape[1] == 4 else abi.BBOX), (abi.F32 if a.dtype == np.float32 else abi.F64)
    if how == "jitter":
        return jitter(rng, a, 0.05)
    if how == "permute":
        return a[rng.permutation(len(a))]
    return mpc.random_volumes(rng, len(a), kind, flt, scale=10.0, size=0.45)


def with_volumes(leaves, vols_of_leaf):
    """The records `leaves` with their volumes replaced by vols_of_leaf (one row per leaf, in leaf order)."""
    out = leaves.copy()
    vdt = leaves.dtype["volume"]
    out["volume"] = np.ascontiguousarray(vols_of_leaf).view(vdt).reshape(-1)
    return out


def host_bvh(g):
    """The device BVH as oracle host records: its leaves, its nodes, its skips."""
    nodes = np.ascontiguousarray(g.nodes.cpu().numpy()).view(abi.node_dtype(g.types)).reshape(-1)
    return orc.HostBVH(g.types, orc.tree_shape(len(g.leaves)), g.built_level, g.leaves.to_numpy(), nodes, g.skips.cpu().numpy(), None)


def first_built_node(tree, built_level):
    """0-based position in the node array of the first node a build writes (the nodes above built_level do not exist)."""
    return orc.memory_index(tree, 2 ** (min(built_level, tree.levels - 1) - 1)) - 1 if tree.levels > 1 else 0


def assert_oracle_nodes(h):
    """The host twin's nodes (the device's) down from built_level are the oracle's merge of its leaves."""
    lo = first_built_node(h.tree, h.built_level)
    assert h.nodes[lo:].tobytes() == orc.aggregate(h.types, h.tree, h.built_level, h.leaves)[lo:].tobytes()


def snapshot(g):
    """What a refit must keep or start from: the leaf records, the skips and the nodes, as host copies."""
    return g.leaves.to_numpy().copy(), g.skips.cpu().numpy().tobytes(), g.nodes.cpu().numpy().copy()


def assert_refit(g, snap, vols_of_leaf, what):
    """g's leaves hold vols_of_leaf (leaf order) with index / morton untouched, its nodes down from built_level are the oracle's
    merge, and the nodes above built_level (which no build writes) are untouched."""
    before, skips_before, nodes_before = snap
    got = g.leaves.to_numpy()
    exp = with_volumes(before, vols_of_leaf)
    assert got["index"].tobytes() == before["index"].tobytes(), what
    assert got["morton"].tobytes() == before["morton"].tobytes(), what
    assert got["volume"].tobytes() == exp["volume"].tobytes(), what
    assert g.skips.cpu().numpy().tobytes() == skips_before, what
    tree = orc.tree_shape(len(exp))
    lo = first_built_node(tree, g.built_level)
    gn = g.nodes.cpu().numpy()
    on = orc.aggregate(g.types, tree, g.built_level, exp).view(gn.dtype).reshape(gn.shape)
    assert gn[lo:].tobytes() == on[lo:].tobytes(), what
    assert gn[:lo].tobytes() == nodes_before[:lo].tobytes(), what


def built_levels(levels):
    return sorted({1, max(1, (levels + 1) // 2), levels})


# ---------------------------------------------------------------------------------------------
# 1. bit-exact refits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [abi.I32, abi.I64], ids=["I32", "I64"])
@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_refit_is_the_oracle_merge_over_the_new_leaves(combo, idx):
    """Every leaf / node combination x index type x Morton width, sizes 1 .. 2^16 + 3, built_level 1 / mid / levels; B = A
    jittered, permuted or fresh; both forms (gathered from user order, and moved in place)."""
    lk, lf, nk, nf = combo
    rng = np.random.default_rng(7 + 31 * COMBOS.index(combo) + idx)
    case = 0
    for morton in (abi.U16, abi.U32, abi.U64):
        types = abi.make_types(lk, lf, nk, nf, idx, morton)
        for n in SIZES:
            a = mpc.random_volumes(rng, n, lk, lf, scale=10.0, size=0.45)
            levels = orc.tree_shape(n).levels
            for how in ("jitter", "permute", "fresh"):
                bl = built_levels(levels)[case % len(built_levels(levels))]
                in_place = case % 2 == 1
                case += 1
                g = build(a, types, built_level=bl)
                snap = snapshot(g)
                before = snap[0]
                b = new_volumes(rng, a, how)
                of_leaf = b[before["index"].astype(np.int64) - 1]
                if in_place:
                    g.leaves.volume.copy_(cuda(of_leaf))
                    assert ibvh.refit(g) is g
                else:
                    assert ibvh.refit(g, cuda(b)) is g
                assert_refit(g, snap, of_leaf, (morton, n, how, bl, in_place))


def test_refit_runs_the_middle_merge_launches():
    """2^21 + 5 leaves: the first launch leaves more than AGG_TOP_MAX nodes, so aggregate_kernel<..., false> runs in between."""
    rng = np.random.default_rng(3)
    for types in (abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32), abi.make_types(abi.BBOX, abi.F64, abi.BBOX, abi.F32, abi.I64, abi.U64)):
        a = mpc.random_volumes(rng, BIG, types.leaf_kind, types.leaf_float, scale=100.0, size=0.2)
        g = build(a, types)
        snap = snapshot(g)
        before = snap[0]
        b = jitter(rng, a, 0.1)
        ibvh.refit(g, cuda(b))
        assert_refit(g, snap, b[before["index"].astype(np.int64) - 1], "gathered")
        snap = snapshot(g)
        before = snap[0]
        c = jitter(rng, b, 0.1)[before["index"].astype(np.int64) - 1]
        g.leaves.volume.copy_(cuda(c))
        ibvh.refit(g)
        assert_refit(g, snap, c, "in place")


def test_refit_of_user_indexed_leaves():
    """BVHs built from BoundingVolumes: the bench's reversed numbering, and sparse indices into a larger array (m > n).
    The leaf with index k takes volumes[k - 1]."""
    rng = np.random.default_rng(11)
    for types in (abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32), abi.make_types(abi.BBOX, abi.F64, abi.BBOX, abi.F64, abi.I64, abi.U16)):
        n = 20_000
        a = mpc.random_volumes(rng, n, types.leaf_kind, types.leaf_float, scale=10.0, size=0.2)
        for indices, m in ((np.arange(n, 0, -1), n), (3 * rng.permutation(n) + 2, 3 * n + 5)):
            g = build(a, types, built_level=2, indices=indices)
            snap = snapshot(g)
            before = snap[0]
            big = mpc.random_volumes(rng, m, types.leaf_kind, types.leaf_float, scale=10.0, size=0.2)
            ibvh.refit(g, cuda(big))
            assert_refit(g, snap, big[before["index"].astype(np.int64) - 1], (m, "first"))
            big2 = jitter(rng, big, 0.02)  # a second refit of the same object: the memoised index check
            snap = snapshot(g)
            ibvh.refit(g, cuda(big2))
            assert_refit(g, snap, big2[before["index"].astype(np.int64) - 1], (m, "second"))


# ---------------------------------------------------------------------------------------------
# 2. traversals on refitted trees
# ---------------------------------------------------------------------------------------------
def contacts_np(t):
    return t.contacts.cpu().numpy().astype(np.int64).reshape(-1, 2)


def oracle_pairs(c):
    return np.stack([c["a"], c["b"]], axis=1).astype(np.int64) if len(c) else np.zeros((0, 2), np.int64)


def as_set(a):
    return sorted(map(tuple, a.tolist()))


@contextlib.contextmanager
def rays_binned(mode):
    lib.set_tuning("rays_binned", mode)
    try:
        yield
    finally:
        lib.set_tuning("rays_binned", 1)


def refitted(rng, n, types, how, built_level=1, steps=1):
    """A device BVH built from A, then refitted `steps` times (how = "permute": one random permutation of A; "drift": moves of
    at most a Morton cell per step), and its oracle host twin."""
    a = mpc.random_volumes(rng, n, types.leaf_kind, types.leaf_float, scale=10.0, size=0.45 * (1000.0 / max(n, 1000)) ** (1 / 3))
    g = build(a, types, built_level=built_level)
    b = a
    for _ in range(steps):
        b = b[rng.permutation(n)] if how == "permute" else jitter(rng, b, 10.0 / 1024)
        ibvh.refit(g, cuda(b))
    h = host_bvh(g)
    assert_oracle_nodes(h)
    return g, h


@pytest.mark.parametrize("how", ["permute", "drift"])
@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[3], COMBOS[6], COMBOS[11]], ids=combo_id)
def test_lvt_self_on_refitted_trees(combo, how):
    """LVT self at several start levels, every narrow of the menu and IBVH_OUTPUT_POSITIONS: the oracle's list, in order."""
    rng = np.random.default_rng(100 + COMBOS.index(combo))
    for n, idx in ((700, abi.I32), (3000, abi.I64)):
        types = abi.make_types(*combo, idx, abi.U32)
        g, h = refitted(rng, n, types, how, built_level=2, steps=1 if how == "permute" else 5)
        pos = np.zeros(n + 1, np.int64)
        pos[h.leaves["index"].astype(np.int64)] = np.arange(1, n + 1)
        cache = None
        for sl in sorted({2, h.tree.levels // 2, h.tree.levels - 1, h.tree.levels}):
            for narrow in (abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT):
                exp = oracle_pairs(orc.traverse_lvt(h, sl, narrow)[0])
                t = ibvh.traverse(g, start_level=sl, narrow=narrow or None)
                assert (contacts_np(t) == exp).all() and t.num_contacts == len(exp), (n, sl, narrow)
                cache = ibvh.traverse(g, start_level=sl, narrow=narrow or None, cache=cache)
                assert (contacts_np(cache) == exp).all(), (n, sl, narrow, "cache")
            exp = oracle_pairs(orc.traverse_lvt(h, sl)[0])
            want = np.stack([np.minimum(pos[exp[:, 0]], pos[exp[:, 1]]), np.maximum(pos[exp[:, 0]], pos[exp[:, 1]])], 1)
            assert (contacts_np(api._traverse_lvt_single(g, sl, abi.OUTPUT_POSITIONS, None)) == want).all(), (n, sl, "positions")
        assert len(exp) > 0


@pytest.mark.parametrize("how", ["permute", "drift"])
def test_lvt_pairs_on_refitted_trees(how):
    """Same-type pairs against the oracle (order included, with and without cache=), and a sphere / box pair of two
    refitted BVHs against the mixed-pair checker."""
    rng = np.random.default_rng(5 if how == "permute" else 6)
    steps = 1 if how == "permute" else 5
    for combo in (COMBOS[0], COMBOS[5]):
        types = abi.make_types(*combo)
        (g1, h1), (g2, h2) = refitted(rng, 1500, types, how, steps=steps), refitted(rng, 900, types, how, steps=steps)
        cache = None
        for (ga, ha), (gb, hb) in (((g1, h1), (g2, h2)), ((g2, h2), (g1, h1))):
            for sl1, sl2 in ((1, 1), (ha.tree.levels // 2, hb.tree.levels)):
                exp = oracle_pairs(orc.traverse_pair_lvt(ha, hb, sl1, sl2)[0])
                t = ibvh.traverse(ga, gb, start_level1=sl1, start_level2=sl2)
                assert (contacts_np(t) == exp).all(), (combo, sl1, sl2)
                cache = ibvh.traverse(ga, gb, start_level1=sl1, start_level2=sl2, cache=cache)
                assert (contacts_np(cache) == exp).all(), (combo, sl1, sl2, "cache")
        assert len(exp) > 0
    gs, hs = refitted(rng, 2000, abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32), how, steps=steps)
    gb, hb = refitted(rng, 1200, abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F64, abi.I32, abi.U64), how, steps=steps)
    for (ga, ha), (gc, hc) in (((gs, hs), (gb, hb)), ((gb, hb), (gs, hs))):
        exp = mpc.traverse_pair_lvt(ha, hc)
        assert len(exp) > 0
        assert (contacts_np(ibvh.traverse(ga, gc)) == exp).all()
        assert (contacts_np(ibvh.traverse(ga, gc, cache=ibvh.traverse(ga, gc))) == exp).all()


def _rays(rng, nr, extent):
    p = (rng.random((nr, 3)) * (extent + 2) - 1).astype(np.float32)
    d = (rng.random((nr, 3)) - 0.5).astype(np.float32)
    return p, d


@pytest.mark.parametrize("how", ["permute", "drift"])
def test_rays_on_refitted_trees(how):
    """LVT rays on the per-lane walker and on the binned path (forced onto this tree), BFS rays as sets with equal checks."""
    rng = np.random.default_rng(8 if how == "permute" else 9)
    for combo in (COMBOS[2], COMBOS[8]):
        g, h = refitted(rng, 20_000, abi.make_types(*combo), how, steps=1 if how == "permute" else 5)
        p, d = _rays(rng, 2000, 10)
        P, D = cuda(p).t(), cuda(d).t()
        exp = oracle_pairs(orc.traverse_rays_lvt(h, p, d)[0])
        assert len(exp) > 0
        for mode in (0, 2):
            with rays_binned(mode):
                t = ibvh.traverse_rays(g, P, D)
                assert (contacts_np(t) == exp).all(), (combo, mode)
                assert (contacts_np(ibvh.traverse_rays(g, P, D, cache=t)) == exp).all(), (combo, mode, "cache")
        bexp, res = orc.traverse_rays_bfs(h, p, d)
        t = ibvh.traverse_rays(g, P, D, ibvh.BFSTraversal())
        assert as_set(contacts_np(t)) == as_set(oracle_pairs(bexp)) and t.num_checks == res.num_checks
        t = ibvh.traverse_rays(g, P, D, ibvh.BFSTraversal(), cache=t)
        assert as_set(contacts_np(t)) == as_set(oracle_pairs(bexp)) and t.num_checks == res.num_checks


@pytest.mark.parametrize("how", ["permute", "drift"])
def test_bfs_on_refitted_trees(how):
    """BFS self and pair: the oracle's contact sets and num_checks, with and without cache=."""
    rng = np.random.default_rng(12 if how == "permute" else 13)
    steps = 1 if how == "permute" else 5
    for combo in (COMBOS[0], COMBOS[4], COMBOS[9]):
        types = abi.make_types(*combo)
        (g1, h1), (g2, h2) = refitted(rng, 1800, types, how, steps=steps), refitted(rng, 700, types, how, steps=steps)
        cache, pair_cache = None, None
        for _ in range(2):
            exp, res = orc.traverse_bfs(h1)
            cache = ibvh.traverse(g1, ibvh.BFSTraversal(), cache=cache)
            assert as_set(contacts_np(cache)) == as_set(oracle_pairs(exp)) and cache.num_checks == res.num_checks
            exp, res = orc.traverse_pair_bfs(h1, h2)
            pair_cache = ibvh.traverse(g1, g2, ibvh.BFSTraversal(), cache=pair_cache)
            assert as_set(contacts_np(pair_cache)) == as_set(oracle_pairs(exp)) and pair_cache.num_checks == res.num_checks
        assert len(exp) > 0


def test_traversal_cache_from_before_the_refit():
    """A traversal made on the tree before a refit serves as cache= afterwards: nothing of the old nodes is reused."""
    rng = np.random.default_rng(17)
    types = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32)
    a = mpc.random_volumes(rng, 5000, abi.BSPHERE, abi.F32, scale=10.0, size=0.3)
    g = build(a, types)
    t = ibvh.traverse(g)
    n0 = t.num_contacts
    ibvh.refit(g, cuda(a[rng.permutation(len(a))]))
    t = ibvh.traverse(g, cache=t)
    exp = oracle_pairs(orc.traverse_lvt(host_bvh(g))[0])
    assert (contacts_np(t) == exp).all() and n0 > 0


def test_large_block_permuted_refit_lvt_self():
    """2^20 + 7 leaves, every leaf's volume swapped with another one's inside runs of 64 consecutive leaves: the block frontier
    and the contact cache on a tree no build makes.  The full LVT self list equals the oracle's, order included."""
    rng = np.random.default_rng(19)
    n = (1 << 20) + 7
    types = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32)
    a = mpc.random_volumes(rng, n, abi.BSPHERE, abi.F32, scale=100.0, size=0.6)
    g = build(a, types)
    vols = np.ascontiguousarray(g.leaves.volume.cpu().numpy())
    run = 64
    order = np.arange(n)
    runs = n // run
    order[:runs * run] = (rng.random((runs, run)).argsort(axis=1) + run * np.arange(runs)[:, None]).reshape(-1)
    g.leaves.volume.copy_(cuda(vols[order]))
    ibvh.refit(g)
    h = host_bvh(g)
    assert_oracle_nodes(h)
    exp = oracle_pairs(orc.traverse_lvt(h)[0])
    t = ibvh.traverse(g)
    assert t.num_contacts == len(exp) and len(exp) > n // 10
    assert (contacts_np(t) == exp).all()
    assert (contacts_np(ibvh.traverse(g, cache=t)) == exp).all()


# ---------------------------------------------------------------------------------------------
# 3. refit chains, then a rebuild through the cache= fast paths
# ---------------------------------------------------------------------------------------------
def test_refit_chain_then_rebuild_from_raw_volumes():
    """k refits, then BVH(vols, cache=bvh): leaves, nodes, skips byte-identical to a fresh build of vols, via the fast path."""
    rng = np.random.default_rng(23)
    types = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32)
    a = mpc.random_volumes(rng, 30_000, abi.BSPHERE, abi.F32, scale=10.0, size=0.2)
    g = ibvh.BVH(cuda(a))
    g = ibvh.BVH(cuda(jitter(rng, a, 0.01)), cache=g)  # (the fast path's key is made by a build with cache=)
    b = a
    for k in range(4):
        b = jitter(rng, b, 10.0 / 1024)
        ibvh.refit(g, cuda(b))
    b = jitter(rng, b, 10.0 / 1024)
    g2 = ibvh.BVH(cuda(b), cache=g)
    assert g2.leaves is g.leaves and g2._fast is g._fast  # the raw-volume fast path was taken
    o = orc.build(b, types)
    assert g2.leaves.to_numpy().tobytes() == o.leaves.tobytes()
    gn = g2.nodes.cpu().numpy()
    assert gn.tobytes() == o.nodes.view(gn.dtype).reshape(gn.shape).tobytes()
    assert g2.skips.cpu().numpy().tobytes() == o.skips.tobytes()
    ibvh.refit(g2, cuda(b))  # and the rebuilt object refits again
    assert gn.tobytes() == g2.nodes.cpu().numpy().tobytes()


def test_refit_chain_then_rebuild_in_place():
    """k in-place refits, then the reference's BVH(bvh.leaves, cache=bvh): byte-identical to a fresh build of those records."""
    rng = np.random.default_rng(29)
    types = abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32)
    n = 30_000
    a = mpc.random_volumes(rng, n, abi.BBOX, abi.F32, scale=10.0, size=0.2)
    g = ibvh.BVH(ibvh.BoundingVolumes.wrap(cuda(a), np.arange(n, 0, -1)))
    g = ibvh.BVH(g.leaves, cache=g)
    for k in range(4):
        cur = np.ascontiguousarray(g.leaves.volume.cpu().numpy())
        g.leaves.volume.copy_(cuda(jitter(rng, cur, 10.0 / 1024)))
        ibvh.refit(g)
    cur = np.ascontiguousarray(g.leaves.volume.cpu().numpy())
    moved = jitter(rng, cur, 10.0 / 1024)
    idx = g.leaves.to_numpy()["index"].copy()
    g.leaves.volume.copy_(cuda(moved))
    g2 = ibvh.BVH(g.leaves, cache=g)
    assert g2.leaves is g.leaves and g2._fast is g._fast  # the in-place fast path was taken
    o = orc.build(moved, types, indices=idx)
    assert g2.leaves.to_numpy().tobytes() == o.leaves.tobytes()
    gn = g2.nodes.cpu().numpy()
    assert gn.tobytes() == o.nodes.view(gn.dtype).reshape(gn.shape).tobytes()
    assert g2.skips.cpu().numpy().tobytes() == o.skips.tobytes()


# ---------------------------------------------------------------------------------------------
# 4. the contract
# ---------------------------------------------------------------------------------------------
def test_refit_refuses_volumes_of_another_kind_float_or_shape():
    rng = np.random.default_rng(31)
    a = mpc.random_volumes(rng, 100, abi.BSPHERE, abi.F32, scale=10.0, size=0.3)
    g = ibvh.BVH(cuda(a))
    box = mpc.random_volumes(rng, 100, abi.BBOX, abi.F32, scale=10.0, size=0.3)
    for bad in (cuda(box), cuda(a.astype(np.float64)), cuda(a[:, :3]), cuda(a.reshape(-1)), torch.from_numpy(a), a):
        with pytest.raises(ValueError):
            ibvh.refit(g, bad)
    assert ibvh.refit(g, cuda(a)) is g


def test_refit_refuses_indices_outside_the_volumes():
    """Python: an index 0, or one larger than the number of volumes given, raises ValueError before anything runs."""
    rng = np.random.default_rng(37)
    n = 500
    a = mpc.random_volumes(rng, n, abi.BSPHERE, abi.F32, scale=10.0, size=0.3)
    for bad in (0, n + 1):
        idx = np.arange(1, n + 1)
        idx[123] = bad
        g = ibvh.BVH(ibvh.BoundingVolumes.wrap(cuda(a), idx))
        nodes = g.nodes.clone()
        with pytest.raises(ValueError):
            ibvh.refit(g, cuda(a))
        assert torch.equal(nodes, g.nodes)
    with pytest.raises(ValueError):  # m smaller than the largest index
        ibvh.refit(ibvh.BVH(cuda(a)), cuda(a[:-1]))


def test_c_abi_flags_an_index_outside_the_volumes():
    """Through the C ABI the same input returns IBVH_OK, sets the flag word, and leaves that leaf's volume as it was; every
    other leaf is refitted and the nodes are the merge of exactly those leaves."""
    rng = np.random.default_rng(41)
    n = 3000
    types = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32)
    a = mpc.random_volumes(rng, n, abi.BSPHERE, abi.F32, scale=10.0, size=0.3)
    for bad in (0, n + 1, -5):
        idx = np.arange(1, n + 1)
        idx[777] = bad
        g = ibvh.BVH(ibvh.BoundingVolumes.wrap(cuda(a), idx))
        snap = snapshot(g)
        before = snap[0]
        b = jitter(rng, a, 0.3)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        bv = cuda(b)
        rc = lib.load().ibvh_refit(C.byref(g.struct()), api._ptr(bv), n, api._ptr(flag), api._stream())
        torch.cuda.synchronize()
        assert rc == abi.OK
        assert int(flag.item()) != 0
        li = before["index"].astype(np.int64)
        old = np.ascontiguousarray(before["volume"]).view(np.float32).reshape(n, 4)
        of_leaf = np.where(((li >= 1) & (li <= n))[:, None], b[np.clip(li, 1, n) - 1], old)
        assert_refit(g, snap, of_leaf, bad)
    # a clean refit leaves a zeroed flag at zero
    g = ibvh.BVH(cuda(a))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    bv = cuda(a)
    assert lib.load().ibvh_refit(C.byref(g.struct()), api._ptr(bv), n, api._ptr(flag), api._stream()) == abi.OK
    assert int(flag.item()) == 0
