"""The checker of the cross-shard contact completion (tests/dist_cross_checker.py) against the oracle's trees, and the
proof that what tests/test_gpu_dist_cross.py expects on its inputs is unambiguous and not vacuous.  CPU only.

Every comparison is exact.  "Inside" is exact where the node boxes are made from the leaves without rounding: box leaves
under box nodes at least as wide.  Everywhere else making a node rounds — the reference turns a sphere into a box with
x -+ r in the LEAF float type (to nearest: inwards half the time), merges spheres with a square root, and narrows to a
narrower node type — so inside means within a relative 1e-6 where the narrower of the two float types is Float32 and
1e-14 where both are Float64 (Float32 spheres under Float64 nodes are rounded in Float32: they get the Float32 bound)."""
import numpy as np
import pytest

import dist_cross_checker as chk
import oracle_lib as orc
from dist_cross_oracle import brute_pairs, oracle_tree, pair_codes, types_of
from implicitbvh_amd import abi


def description(case, r):
    o = oracle_tree(case, r)
    report = {}
    return chk.describe(o.nodes, o.leaves, o.tree, o.types, report), report


def leaf_boxes(case, r):
    return chk.volume_boxes(case.shards[r], case.combo[0])


def making_a_node_is_exact(combo):
    lk, lf, nk, nf = combo
    return lk == chk.BBOX and nk == chk.BBOX and nf >= lf


def assert_leaves_inside(boxes, leaves, combo, what):
    lo, up = boxes[:, None, :3], boxes[:, None, 3:]
    llo, lup = leaves[None, :, :3], leaves[None, :, 3:]
    if making_a_node_is_exact(combo):
        slack = 0.0
    else:
        rel = 1e-6 if chk.F32 in (combo[1], combo[3]) else 1e-14
        slack = rel * (np.abs(up - lo) + np.abs(lo) + np.abs(up))
    with np.errstate(invalid="ignore"):
        inside = np.all((llo >= lo - slack) & (lup <= up + slack), axis=2)
    assert inside.any(axis=0).all(), what


# ---------------------------------------------------------------------------------------------
# describe
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [chk.ALL_COMBOS[0], chk.ALL_COMBOS[1], chk.ALL_COMBOS[7], chk.ALL_COMBOS[8]], ids=chk.combo_name)
def test_describe_on_small_and_large_trees(combo):
    """A tree of <= 32 leaves is refined down to its last node level, whatever the order: 1, 1, 2, 3, 16, 16 boxes, as a
    set exactly that level's real nodes (the single leaf for n = 1); larger trees stop at 16 boxes.  Every leaf lies in one."""
    rng = np.random.default_rng(7)
    types = abi.make_types(*combo)
    for n, want in ((1, 1), (2, 1), (3, 2), (5, 3), (31, 16), (32, 16), (33, 16), (1500, 16)):
        vols = chk.volumes(rng, rng.random((n, 3)) * 6.0, combo[0], combo[1], 1.0)
        o = orc.build(vols, types)
        report = {}
        boxes = chk.describe(o.nodes, o.leaves, o.tree, types, report)
        assert boxes.shape == (want, 6) and boxes.dtype == np.float64, n
        assert want == (1 if n == 1 else min(16, -(-n // 2))), n
        assert report["ties"] == 0, n
        leaves = chk.volume_boxes(vols, combo[0])
        if n == 1:
            assert boxes.tobytes() == leaves.tobytes()
        elif n <= 32:
            level = chk.last_node_level_boxes(o.nodes, o.tree, types)
            assert sorted(map(tuple, boxes.tolist())) == sorted(map(tuple, level.tolist())), n
        assert_leaves_inside(boxes, leaves, combo, n)


def test_touches_and_export_masks_on_hand_made_boxes():
    a = np.array([[0, 0, 0, 1, 1, 1], [5, 5, 5, 6, 6, 6]], float)
    assert chk.touches(a, [[1, 1, 1, 2, 2, 2]])            # a shared corner is a contact (closed comparisons)
    assert not chk.touches(a, [[1.0000001, 0, 0, 2, 1, 1]])
    assert not chk.touches(a, [[np.nan, 0, 0, 2, 1, 1]])
    assert not chk.touches(a, np.zeros((0, 6)))
    leaves = np.array([[1, 0, 0, 2, 1, 1], [1.00001, 0, 0, 2, 1, 1], [1.001, 0, 0, 2, 1, 1], [-np.inf] * 3 + [np.inf] * 3], float)
    assert chk.must_export(leaves, a[:1]).tolist() == [True, False, False, True]
    assert chk.may_export(leaves, a[:1], 1e-4).tolist() == [True, True, False, True]  # (faces move by 1e-4 * (1 + 0 + 1))
    assert chk.box_volume([0, 0, 0, 1, 2, -3]) == 0.0 and chk.box_volume([0, 0, 0, np.inf, 1, 0]) == 0.0


# ---------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_dist_cross.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", chk.case_names(path="B"))
def test_arbitrary_shards_have_an_unambiguous_nonvacuous_answer(name):
    case = chk.case(name)
    W = case.world
    desc = [description(case, r) for r in range(W)]
    for r in range(W):
        boxes, report = desc[r]
        assert report["ties"] == 0, r
        assert_leaves_inside(boxes, leaf_boxes(case, r), case.combo, r)
    sets = {}
    for r in range(W):
        for s in range(r + 1, W):
            got = orc.traverse_pair_lvt(oracle_tree(case, r), oracle_tree(case, s))[0]
            sets[r, s] = brute_pairs(case, r, s)
            assert np.array_equal(pair_codes(got["a"], got["b"]), sets[r, s]), (r, s)
            if len(sets[r, s]):  # two slices with a contact must be found to touch, and the leaves in contact must travel
                assert chk.touches(desc[r][0], desc[s][0])
    for r, s in case.cross:
        assert len(sets[r, s]) > 0, (r, s)
    rel = chk.export_cap(case.combo[1], case.combo[3])
    for s, r in case.filtered:
        must, may = chk.must_export(leaf_boxes(case, s), desc[r][0]), chk.may_export(leaf_boxes(case, s), desc[r][0], rel)
        assert 0 < must.sum() and may.sum() < len(must) and not (must & ~may).any(), (s, r)
    # what the single cases are about
    if name == "everything-overlaps":
        assert all(chk.must_export(leaf_boxes(case, s), desc[r][0]).all() for r in range(W) for s in range(r + 1, W))
    if name == "nothing-touches":
        assert not any(chk.touches(desc[r][0], desc[s][0]) for r in range(W) for s in range(r + 1, W))
    if name.startswith("bridge-"):
        m = int(name[-1])
        assert chk.must_export(leaf_boxes(case, 1), desc[0][0]).sum() == m == chk.may_export(leaf_boxes(case, 1), desc[0][0], rel).sum()
    if name.startswith("zero-contact"):
        gaps = [s for s in (1, 2) if (0, s) not in case.cross]
        for s in gaps:
            assert len(sets[0, s]) == 0 and chk.must_export(leaf_boxes(case, s), desc[0][0]).sum() > 0
        if len(gaps) == 2:
            assert len(sets[1, 2]) == 0 and chk.must_export(leaf_boxes(case, 2), desc[1][0]).sum() > 0
    if name == "flat-shard":
        assert len(desc[0][0]) == 1
    if name.startswith("sizes-1-2-3-5-33"):
        assert [len(d[0]) for d in desc] == [1, 1, 2, 3, 16]
    if name.startswith("infinite"):
        which = int(name[-1])
        assert np.isinf(desc[which][0]).any() and len(sets[0, 1]) >= len(case.shards[1 - which])


@pytest.mark.parametrize("name", chk.case_names(path="A"))
def test_whole_cloud_answer_of_the_product_path_inputs(name):
    """The whole cloud's contact set as the oracle's tree finds it is the set all pairs tried give; equal cuts of the
    sorted sequence (what the distributed build aims at) describe themselves without ties."""
    case = chk.case(name)
    cloud = np.concatenate(case.shards)
    types = types_of(case)
    o = orc.build(cloud, types)
    got = orc.traverse_lvt(o)[0]
    a, b = got["a"].astype(np.int64), got["b"].astype(np.int64)
    want = orc.brute_force_self(case.combo[0], case.combo[1], cloud)
    assert np.array_equal(pair_codes(np.minimum(a, b), np.maximum(a, b)), pair_codes(want[:, 0], want[:, 1]))
    assert len(want) > 1000
    n = len(cloud)
    vols = o.leaves["volume"]
    flat = np.ascontiguousarray(vols).view(vols.dtype[0].base).reshape(n, -1)
    for r in range(case.world):
        lo, hi = n * r // case.world, n * (r + 1) // case.world
        sl = orc.build(flat[lo:hi], types, indices=o.leaves["index"][lo:hi], compute_extrema=False, mins=o.extrema[:3], maxs=o.extrema[3:])
        report = {}
        boxes = chk.describe(sl.nodes, sl.leaves, sl.tree, types, report)
        assert report["ties"] == 0 and len(boxes) == 16
        assert_leaves_inside(boxes, chk.volume_boxes(flat[lo:hi], case.combo[0]), case.combo, r)


def test_grid_stride_input_exports_from_both_trips():
    """The lower shard's boxes select leaves of the upper shard on both sides of sorted position 8192 * 256."""
    case = chk.stride_case()
    types = types_of(case)
    lower = orc.build(case.shards[0], types, indices=(1 + np.arange(len(case.shards[0]))).astype(np.int32))
    report = {}
    boxes = chk.describe(lower.nodes, lower.leaves, lower.tree, types, report)
    assert report["ties"] == 0
    upper = orc.build(case.shards[1], types, indices=(case.base[1] + 1 + np.arange(len(case.shards[1]))).astype(np.int32))
    assert len(upper.leaves) > 8192 * 256
    must = chk.must_export(chk.volume_boxes(upper.leaves["volume"], chk.BSPHERE), boxes)
    assert must[:8192 * 256].any() and must[8192 * 256:].any() and must.sum() < len(must) // 4
