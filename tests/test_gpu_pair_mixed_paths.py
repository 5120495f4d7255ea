"""IBVH_PAIR_MIXED_TYPES on the paths only larger inputs select: the shared descent of the counting pass (BlockRows,
lvt_block_frontier_kernel; forced here with lvt_blocks_min_items = 1 and, at the published size, by the default knobs), the
one-kernel scan and the dense .index copy behind it, the cross-float joint walk at size, and NaN / infinite radii with rows.
Every list equals the oracle's mixed walk (oracle_traverse_pair_lvt_* with IBVH_PAIR_MIXED_TYPES, pinned to the numpy checker
by tests/test_host_mixed_pair.py), order included, unless a test says otherwise; the launch profile shows the frontier kernel
exactly when the launch rule allows it, and never when the two trees' node types differ."""
import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_lvt_blocks import _kernels_of, _keys, _ran_frontier, forced_rows, rows_rule  # noqa: F401  (forced_rows: a fixture)
from test_gpu_parity import _positions, build_both, contacts_np, oracle_pairs, random_volumes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api  # noqa: E402

S, B, F32, F64 = abi.BSPHERE, abi.BBOX, abi.F32, abi.F64
MIXED = abi.PAIR_MIXED_TYPES
# (sphere tree, box tree): one node type, one leaf float type — the queue walker's mixed families (IBVH_FOR_MIXED_QUEUE_*)
FAMILIES = [((S, F32, B, F32), (B, F32, B, F32)), ((S, F64, B, F64), (B, F64, B, F64)),
            ((S, F32, B, F64), (B, F32, B, F64)), ((S, F64, B, F32), (B, F64, B, F32))]


def fam_id(f):
    return "_".join("%s%d%s%d" % ("SB"[c[0]], 32 << c[1], "SB"[c[2]], 32 << c[3]) for c in f)


def expected(o1, o2, code=0, sl1=None, sl2=None):
    """The oracle's mixed list for (bvh1, bvh2); IBVH_OUTPUT_POSITIONS maps it to 1-based leaf positions."""
    pos = code & abi.OUTPUT_POSITIONS
    c = orc.traverse_pair_lvt(o1, o2, sl1, sl2, (code & ~abi.OUTPUT_POSITIONS) | MIXED)[0]
    e = oracle_pairs(c)
    if pos and len(e):
        e = np.stack([_positions(o1.leaves)[e[:, 0]], _positions(o2.leaves)[e[:, 1]]], axis=1)
    return e


def device(g1, g2, code=0, sl1=None, sl2=None, cache=None):
    sl1 = max(1, g1.built_level) if sl1 is None else sl1
    sl2 = max(1, g2.built_level) if sl2 is None else sl2
    return api._traverse_lvt_pair(g1, g2, sl1, sl2, code, cache)


def drives(o1, o2, code=0):
    """(driving, walked) oracle trees of the pair (bvh1, bvh2)"""
    n1, n2 = o1.tree.real_leaves, o2.tree.real_leaves
    flip = n1 > n2 if code & abi.PAIR_SMALLER_DRIVES else not n1 >= n2
    return (o2, o1) if flip else (o1, o2)


def check_pair(o1, g1, o2, g2, code=0, sl1=None, sl2=None, shift=11, min_items=1, queue=True, cache=True, what=None):
    """The device's list equals the oracle's in order (and again through cache= / enqueue); the frontier kernel ran exactly
    when the launch rule says so (queue=False: a pair the queue walker's rows cannot serve — nodes of two types, or a
    cross-float query, which takes the joint walk).  -> the number of contacts."""
    exp = expected(o1, o2, code, sl1, sl2)
    names = _kernels_of(lambda: device(g1, g2, code, sl1, sl2))
    drv, walk = drives(o1, o2, code)
    assert _ran_frontier(names) == rows_rule(drv, walk, drv.tree.real_leaves, shift, min_items, queue), (what, names)
    t = device(g1, g2, code, sl1, sl2)
    assert contacts_np(t).shape == exp.shape and (contacts_np(t) == exp).all(), what
    if cache:
        assert (contacts_np(device(g1, g2, code, sl1, sl2, cache=t)) == exp).all(), ("enqueue", what)
    return len(exp)


def cloud(rng, n, combo, scale, idx=abi.I32, morton=abi.U32, built_level=1, size=1.0):
    return build_both(random_volumes(rng, n, combo[0], combo[1], scale=scale, size=size),
                      abi.make_types(*combo, idx, morton), built_level=built_level)


# driving size, walked size, code: ragged last blocks at every block size; 4,097 queries need the smaller tree to drive
SIZES = ((4097, 40_000, abi.PAIR_SMALLER_DRIVES), (65_537, 40_000, 0), (150_001, 60_000, 0))


@pytest.mark.parametrize("fam", FAMILIES, ids=fam_id)
def test_forced_rows_every_queue_family_both_directions(forced_rows, fam):
    """Sphere queries walking box leaves and box queries walking sphere leaves, at 4,097 / 65,537 / 150,001 driving leaves,
    both argument orders; Morton widths differ between the two trees."""
    sph_c, box_c = fam
    rng = np.random.default_rng(31 + FAMILIES.index(fam))
    total = 0
    for nd, nw, code in SIZES:
        scale = 0.9 * max(nd, nw) ** (1 / 3)
        for drv_c, walk_c in ((sph_c, box_c), (box_c, sph_c)):
            od, gd = cloud(rng, nd, drv_c, scale, morton=abi.U32)
            ow, gw = cloud(rng, nw, walk_c, scale, morton=abi.U64 if nd % 2 else abi.U16)
            assert drives(od, ow, code)[0] is od
            total += check_pair(od, gd, ow, gw, code, what=(nd, nw, drv_c))
            total += check_pair(ow, gw, od, gd, code, cache=False, what=(nw, nd, drv_c, "flipped"))
    assert total > 100_000


def test_forced_rows_narrow_positions_and_index_types(forced_rows):
    """Narrow codes, IBVH_OUTPUT_POSITIONS and Int64 indices on a mixed pair with rows (S32/B32 driving B32/B32 and back)."""
    rng = np.random.default_rng(41)
    for idx, morton in ((abi.I32, abi.U32), (abi.I64, abi.U64)):
        osph, gsph = cloud(rng, 70_001, FAMILIES[0][0], 36.0, idx, morton)
        obox, gbox = cloud(rng, 45_000, FAMILIES[0][1], 36.0, idx, abi.U16 if morton == abi.U64 else abi.U64)
        for code in (abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT, abi.OUTPUT_POSITIONS, abi.NARROW_INDEX_LT | abi.OUTPUT_POSITIONS):
            # (NARROW_MORTON_LT on two Morton widths: the wider codes are mostly the larger, so one order keeps most pairs and
            # the other next to none)
            m = check_pair(osph, gsph, obox, gbox, code, cache=code == abi.NARROW_MORTON_LT, what=(idx, code))
            m += check_pair(obox, gbox, osph, gsph, code, cache=False, what=(idx, code, "flipped"))
            assert m > 1000, code


@pytest.mark.parametrize("built_level", [3, 8, 9])
def test_forced_rows_partially_built_driving_tree(forced_rows, built_level):
    """An 18-level driving tree built from level 3 / 8 / 9 (blocks of 2^10: at 9 the block level 8 is above the built nodes,
    no rows), the walked tree from level 2; the caller's start levels at and below the built levels."""
    forced_rows("lvt_block_shift", 10)
    rng = np.random.default_rng(43 + built_level)
    for drv_c, walk_c in ((FAMILIES[0][0], FAMILIES[0][1]), (FAMILIES[1][1], FAMILIES[1][0])):
        od, gd = cloud(rng, 100_000, drv_c, 40.0, built_level=built_level)
        ow, gw = cloud(rng, 40_000, walk_c, 40.0, morton=abi.U64, built_level=2)
        for sl1, sl2 in ((built_level, 2), (built_level + 2, ow.tree.levels - 3)):
            check_pair(od, gd, ow, gw, sl1=sl1, sl2=sl2, shift=10, cache=False, what=(built_level, sl1, sl2, drv_c))
            check_pair(ow, gw, od, gd, sl1=sl2, sl2=sl1, shift=10, cache=False, what=(built_level, sl1, sl2, drv_c, "flipped"))


def test_no_rows_when_the_node_types_differ(forced_rows):
    """Rows are covers made of the DRIVING tree's nodes: a driving tree with nodes of another float type or kind never gets
    them (run<>'s same_nodes), even forced, and neither does a cross-float query (the joint walk); the lists still equal the
    oracle's."""
    rng = np.random.default_rng(47)
    ow, gw = cloud(rng, 50_000, (B, F32, B, F32), 30.0)
    for drv_c in ((S, F32, B, F64), (S, F32, S, F32), (B, F32, B, F64), (S, F64, B, F32)):
        od, gd = cloud(rng, 80_000, drv_c, 30.0, morton=abi.U64)
        for a, b in (((od, gd), (ow, gw)), ((ow, gw), (od, gd))):
            check_pair(*a, *b, queue=False, cache=False, what=drv_c)


def _torus_surface(u, v, count):
    from implicitbvh_amd.synthetic import torus_mesh
    tris = torch.from_numpy(torus_mesh(u, v)[:count].copy()).cuda()
    return ibvh.bounding_volumes_from_triangles(tris, ibvh.BBox(torch.float32))


def test_cross_float_particles_against_a_surface_at_size():
    """BSphere{Float64} particles (150,001) against a BBox{Float32} surface (50,240 triangles): cross-float queries take the
    exact joint walk whichever tree drives; no frontier kernel."""
    vols = _torus_surface(160, 157, 50_240).cpu().numpy()
    osurf, gsurf = build_both(vols, abi.make_types(B, F32, B, F32))
    lo, hi = vols[:, :3].min(0), vols[:, 3:].max(0)
    rng = np.random.default_rng(53)
    n = 150_001
    c = lo + (hi - lo) * rng.random((n, 3))
    r = 0.004 * float((hi - lo).max()) * (0.5 + 0.5 * rng.random((n, 1)))
    opart, gpart = build_both(np.concatenate([c, r], axis=1), abi.make_types(S, F64, B, F64, abi.I32, abi.U64))
    total = 0
    for code in (0, abi.PAIR_SMALLER_DRIVES, abi.NARROW_INDEX_LT):
        total += check_pair(opart, gpart, osurf, gsurf, code, queue=False, cache=code == 0, what=code)
        total += check_pair(osurf, gsurf, opart, gpart, code, queue=False, cache=False, what=(code, "flipped"))
    assert total > 10_000


@pytest.mark.parametrize("what", ["inf", "nan"])
def test_nan_and_infinite_radii_in_a_mixed_pair_with_rows(forced_rows, what):
    """Spheres with infinite or NaN radii in a mixed pair with box leaves, either tree driving.  Infinite radii only: rows on
    == rows off == the oracle, in order.  NaN radii: include/ibvh.h's statement for the same-type walk holds for the mixed walk
    too — nothing twice, rows on contains rows off contains the oracle's list."""
    rng = np.random.default_rng(59)
    n = 70_000
    vols = random_volumes(rng, n, S, F32, scale=36.0)
    bad = rng.choice(n, 200, replace=False)
    vols[bad, 3] = np.inf if what == "inf" else np.nan
    with np.errstate(all="ignore"):
        osph, gsph = build_both(vols, abi.make_types(S, F32, B, F32))
    obox_big, gbox_big = cloud(rng, 90_000, (B, F32, B, F32), 36.0, morton=abi.U64)
    obox, gbox = cloud(rng, 40_000, (B, F32, B, F32), 36.0, morton=abi.U16)
    for (o1, g1), (o2, g2) in (((osph, gsph), (obox, gbox)), ((obox_big, gbox_big), (osph, gsph))):
        drv, walk = drives(o1, o2)
        assert rows_rule(drv, walk, drv.tree.real_leaves)
        with np.errstate(all="ignore"):
            exp = expected(o1, o2)
        forced_rows("lvt_blocks", 1)
        with_rows = device(g1, g2).contacts.clone()
        forced_rows("lvt_blocks", 0)
        without = device(g1, g2).contacts.clone()
        forced_rows("lvt_blocks", 1)
        kw, kn, ko = _keys(with_rows), _keys(without), _keys(exp).cuda()
        assert torch.unique(kw).shape[0] == kw.shape[0] and torch.unique(kn).shape[0] == kn.shape[0]  # nothing twice
        assert len(exp) > 1000
        if what == "inf":
            assert with_rows.shape[0] == len(exp) and (with_rows.cpu().numpy().astype(np.int64) == exp).all()
            assert torch.equal(with_rows, without)
        else:
            assert bool(torch.isin(ko, kn).all()) and bool(torch.isin(kn, kw).all())
