"""Plain numpy restatement, in float64, of what the cross-shard contact completion promises (include/ibvh.h, "Cross-shard
contact completion"), and the inputs its tests run on.  No library, no oracle: only numpy.

  describe      a slice's description: "<= 16 node boxes of its tree, refined from the root by always splitting the largest"
  touches       any box of one description against any box of another, closed comparisons
  must_export   the own leaves a receiver has to get: their exact box touches one of the receiver's boxes
  may_export    the own leaves a receiver may get: the same against boxes widened by `rel` (a cap on over-selection)
  case(name)    the shard geometries (made on first use), shared by tests/test_host_dist_cross.py (which proves that the expected sets are
                unambiguous and not vacuous) and tests/test_gpu_dist_cross.py (which runs the library on them)

Volumes are (n, 4) [x, y, z, r] or (n, 6) [lo, up] arrays, or the structured arrays of the same bytes."""
import numpy as np

BSPHERE, BBOX = 0, 1          # ibvh_volume_kind
F32, F64 = 0, 1               # ibvh_float_type
I32, I64 = 0, 1               # ibvh_index_type
U16, U32, U64 = 0, 1, 2       # ibvh_morton_type
CROSS_BOXES = 16              # IBVH_DIST_CROSS_BOXES
NP_F = {F32: np.float32, F64: np.float64}


# ---------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------
def volume_boxes(vols, kind):
    """(n, 4|6) numbers or a structured volume array -> (n, 6) float64 [lo, up]: x -+ r for spheres, lo / up for boxes,
    computed in double after the exact conversion of every number to double."""
    a = np.asarray(vols)
    if a.dtype.names:
        base = a.dtype[0].base
        a = np.ascontiguousarray(a).view(base).reshape(len(a), -1)
    a = a.astype(np.float64)
    if kind == BSPHERE:
        assert a.shape[1] == 4
        return np.concatenate([a[:, :3] - a[:, 3:4], a[:, :3] + a[:, 3:4]], axis=1)
    assert a.shape[1] == 6
    return a.copy()


def box_volume(b):
    """Product of the positive extents, multiplied in the order x, y, z; a NaN volume counts as 0."""
    v = 1.0
    for k in range(3):
        d = float(b[3 + k]) - float(b[k])
        v = v * (d if d > 0 else 0.0)
    return v if v == v else 0.0


def level_layout(tree):
    """-> (real[l], start[l]) for l = 1 .. levels (index 0 unused): real nodes of level l — the virtual ones are the
    rightmost of their level — and the 0-based memory index of its first node (memory holds the real nodes only, level by level)."""
    levels, vl = int(tree.levels), int(tree.virtual_leaves)
    real, start, at = [0], [0], 0
    for lvl in range(1, levels + 1):
        r = (1 << (lvl - 1)) - (vl >> (levels - lvl))
        real.append(r)
        start.append(at)
        at += r
    return real, start


def describe(nodes, leaves, tree, types, report=None):
    """The ordered boxes rank r publishes for its slice: (n_boxes, 6) float64.
    nodes: the tree's node volumes in memory order; leaves: its sorted leaf records (field "volume") or leaf volumes.
    report (a dict): report["ties"] = refinement steps at which two candidates had exactly the same, largest, volume."""
    levels = int(tree.levels)
    if report is not None:
        report["ties"] = 0
    if int(tree.real_nodes) <= int(tree.real_leaves):  # a tree without nodes: the single leaf's box
        lv = np.asarray(leaves)
        lv = lv["volume"] if lv.dtype.names and "volume" in lv.dtype.names else lv
        return volume_boxes(lv[:1], types.leaf_kind)
    nb = volume_boxes(nodes, types.node_kind)
    real, start = level_layout(tree)
    boxes, where = [nb[0]], [(1, 0)]  # (level, position within the level) of every box
    while len(boxes) < CROSS_BOXES:
        pick, best, same = -1, 0.0, 0
        for i, (lvl, _) in enumerate(where):
            if lvl + 1 > levels - 1:  # its children are leaves
                continue
            v = box_volume(boxes[i])
            if pick < 0 or v > best:
                pick, best, same = i, v, 1
            elif v == best:
                same += 1
        if pick < 0 or best <= 0.0:
            break
        if report is not None and same > 1:
            report["ties"] += 1
        lvl, pos = where[pick]
        cl, c0 = lvl + 1, 2 * pos
        boxes[pick], where[pick] = nb[start[cl] + c0], (cl, c0)
        if c0 + 1 < real[cl]:  # the right child is real
            boxes.append(nb[start[cl] + c0 + 1])
            where.append((cl, c0 + 1))
    return np.array(boxes, dtype=np.float64).reshape(-1, 6)


def last_node_level_boxes(nodes, tree, types):
    """The boxes of the real nodes of the last node level (levels - 1)."""
    real, start = level_layout(tree)
    lvl = int(tree.levels) - 1
    return volume_boxes(nodes, types.node_kind)[start[lvl]:start[lvl] + real[lvl]]


def _touch_matrix(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1, 6), np.asarray(b, np.float64).reshape(-1, 6)
    with np.errstate(invalid="ignore"):
        return np.all((a[:, None, 3:] >= b[None, :, :3]) & (a[:, None, :3] <= b[None, :, 3:]), axis=2)


def touches(boxes_a, boxes_b):
    """Any box of a against any box of b, closed comparisons (a NaN touches nothing)."""
    if len(boxes_a) == 0 or len(boxes_b) == 0:
        return False
    return bool(_touch_matrix(boxes_a, boxes_b).any())


def must_export(leaf_boxes, receiver_boxes):
    """Mask of the leaves whose exact double box touches one of the receiver's boxes."""
    leaf_boxes = np.asarray(leaf_boxes, np.float64).reshape(-1, 6)
    keep = np.zeros(len(leaf_boxes), bool)
    for b in np.asarray(receiver_boxes, np.float64).reshape(-1, 6):  # (<= 16 boxes: the leaves stay vectorised)
        with np.errstate(invalid="ignore"):
            keep |= np.all((leaf_boxes[:, 3:] >= b[:3]) & (leaf_boxes[:, :3] <= b[3:]), axis=1)
    return keep


def may_export(leaf_boxes, receiver_boxes, rel):
    """must_export against receiver boxes whose every face is moved out by rel * (|up - lo| + |lo| + |up|)."""
    rb = np.asarray(receiver_boxes, np.float64).reshape(-1, 6)
    lo, up = rb[:, :3], rb[:, 3:]
    with np.errstate(invalid="ignore"):
        ext = np.abs(up - lo) + np.abs(lo) + np.abs(up)
        wide = np.concatenate([lo - rel * ext, up + rel * ext], axis=1)
    return must_export(leaf_boxes, wide)


def export_cap(leaf_float, node_float):
    """Ten times the library's own widening ("a few ulps of the narrower float type": 1e-5 / 1e-13)."""
    return 1e-4 if (leaf_float == F32 or node_float == F32) else 1e-12


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def volumes(rng, centres, kind, flt, size):
    """random_volumes-style sizes: radius / half extents of size * (0.1 + 0.9 u) around the given centres."""
    f = NP_F[flt]
    c = np.asarray(centres).astype(f)
    n = len(c)
    if kind == BSPHERE:
        return np.concatenate([c, (size * (0.1 + 0.9 * rng.random((n, 1)))).astype(f)], axis=1)
    h = (size * (0.1 + 0.9 * rng.random((n, 3)))).astype(f)
    return np.concatenate([c - h, c + h], axis=1)


class Case:
    """One input.  path "B": shards[r] is rank r's volumes, built as they are with global indices base[r] + 1 ...;
    path "A": shards[r] is what rank r hands the distributed build (the cloud is their concatenation).
    cross: rank pairs (r, s), r < s, that must have contacts; filtered: (sender s, receiver r) pairs for which the
    export must be a strict, non-empty subset of the sender's slice."""

    def __init__(self, name, combo, im, path, shards, cross=(), filtered=()):
        self.name, self.combo, self.im, self.path = name, tuple(combo), tuple(im), path
        self.shards = [np.ascontiguousarray(s) for s in shards]
        self.cross, self.filtered = tuple(cross), tuple(filtered)
        self.world = len(self.shards)
        sizes = [len(s) for s in self.shards]
        self.base = [int(sum(sizes[:r])) for r in range(self.world)]

    def __repr__(self):
        return self.name


DEFAULT = (BSPHERE, F32, BBOX, F32)
ALL_COMBOS = [  # tests/test_gpu_parity.py, ALL_COMBOS
    (BSPHERE, F32, BBOX, F32), (BSPHERE, F32, BSPHERE, F32), (BBOX, F32, BBOX, F32), (BSPHERE, F64, BBOX, F32),
    (BSPHERE, F64, BBOX, F64), (BSPHERE, F64, BSPHERE, F64), (BSPHERE, F64, BSPHERE, F32), (BBOX, F64, BBOX, F64),
    (BBOX, F64, BBOX, F32), (BSPHERE, F32, BBOX, F64), (BSPHERE, F32, BSPHERE, F64), (BBOX, F32, BBOX, F64),
]
COMBO_NAMES = {BSPHERE: "S", BBOX: "B"}


def combo_name(combo, im=(I32, U32)):
    f = {F32: "32", F64: "64"}
    return (f"{COMBO_NAMES[combo[0]]}{f[combo[1]]}-{COMBO_NAMES[combo[2]]}{f[combo[3]]}"
            f"-{'i32' if im[0] == I32 else 'i64'}-{('u16', 'u32', 'u64')[im[1]]}")


def slabs(seed, combo, world, per_shard, origin=(0.0, 0.0, 0.0)):
    """`world` overlapping slabs along x of one random cloud (12 units of x a slab, leaves assigned by a jittered x), so
    that a slab exports a shell to the slab below it and nothing to the one after that."""
    rng = np.random.default_rng(seed)
    n = world * per_shard
    c = rng.random((n, 3)) * np.array([12.0 * world, 12.0, 12.0])
    owner = np.clip(np.floor((c[:, 0] + rng.uniform(-1.5, 1.5, n)) / 12.0).astype(int), 0, world - 1)
    vols = volumes(rng, c + np.asarray(origin), combo[0], combo[1], 1.0)
    return [vols[owner == r] for r in range(world)]


def type_case(i, im):
    combo = ALL_COMBOS[i]
    return Case("types-" + combo_name(combo, im), combo, im, "B", slabs(100 + i, combo, 3, 1500),
                cross=[(0, 1), (1, 2)], filtered=[(1, 0), (2, 1)])


def type_keys():
    for i in range(len(ALL_COMBOS)):
        yield i, (I32, U32)
        if i in (2, 5, 9):  # a box-leaf combination, a sphere-node combination, a node float wider than the leaves'
            yield i, (I64, U64)
            yield i, (I32, U16)


def clustered_cloud(seed, kind, flt, n=12000, clusters=40):
    rng = np.random.default_rng(seed)
    mid = rng.random((clusters, 3)) * 10.0
    c = mid[rng.integers(0, clusters, n)] + 0.25 * rng.standard_normal((n, 3))
    return volumes(rng, c, kind, flt, 0.06)


PRODUCT_KEYS = ((200, (BBOX, F32, BBOX, F32), (I32, U32)), (201, (BBOX, F64, BBOX, F64), (I64, U64)),
                (202, (BSPHERE, F64, BBOX, F32), (I32, U32)), (203, (BSPHERE, F32, BBOX, F32), (I32, U16)))


def product_case(seed, combo, im):
    cloud = clustered_cloud(seed, combo[0], combo[1])
    n, world = len(cloud), 4
    shards = [cloud[n * r // world:n * (r + 1) // world] for r in range(world)]
    return Case("product-" + combo_name(combo, im), combo, im, "A", shards)


def cube(rng, n, side, combo, size, origin=(0.0, 0.0, 0.0)):
    return volumes(rng, rng.random((n, 3)) * side + np.asarray(origin), combo[0], combo[1], size)


def overlap_case():
    rng = np.random.default_rng(300)
    world = 4
    return Case("everything-overlaps", DEFAULT, (I32, U32), "B", [cube(rng, 800, 4.0, DEFAULT, 0.5) for _ in range(world)],
                cross=[(r, s) for r in range(world) for s in range(r + 1, world)])


def apart_case():
    rng = np.random.default_rng(301)
    return Case("nothing-touches", DEFAULT, (I32, U32), "B",
                [cube(rng, 300, 4.0, DEFAULT, 0.5, origin=(50.0 * r, 0, 0)) for r in range(3)])


def bridge_case(m):
    """Two far-apart blobs of 1000; m leaves of the upper shard sit inside the lower blob: rank 0 imports exactly m leaves."""
    rng = np.random.default_rng(310 + m)
    lower = cube(rng, 1000, 4.0, DEFAULT, 0.4)
    upper = cube(rng, 1000, 4.0, DEFAULT, 0.4, origin=(60.0, 0, 0))
    bridge = cube(rng, m, 1.0, DEFAULT, 0.4, origin=(1.5, 1.5, 1.5))
    mixed = np.concatenate([upper[:500], bridge, upper[500:]])
    return Case(f"bridge-{m}", DEFAULT, (I32, U32), "B", [lower, mixed], cross=[(0, 1)], filtered=[(1, 0)])


def sizes_case(sizes, side, size, seed):
    rng = np.random.default_rng(seed)
    world = len(sizes)
    return Case("sizes-" + "-".join(map(str, sizes)), DEFAULT, (I32, U32), "B", [cube(rng, n, side, DEFAULT, size) for n in sizes],
                cross=[(r, s) for r in range(world) for s in range(r + 1, world)] if world == 2 else [(world - 2, world - 1)])


def lattice_case(kinds, name):
    """Shard 0 is a jittered 8 x 8 x 8 lattice of small leaves with gaps between them.  A "gap" shard is tiny leaves at
    the centres of lattice cells — inside shard 0's boxes, touching none of its leaves (and no other gap shard: they use
    different cells); a "touch" shard is larger leaves at random places, which touch shard 0."""
    rng = np.random.default_rng(320)
    g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    shards = [volumes(rng, g + rng.uniform(-0.05, 0.05, g.shape), BSPHERE, F32, 0.2)]
    cells = np.stack(np.meshgrid(*[np.arange(7.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    parity = cells.sum(axis=1) % 2
    for i, kind in enumerate(kinds):
        if kind == "gap":
            c = cells[parity == i % 2] + 0.5
            shards.append(volumes(rng, c + rng.uniform(-0.05, 0.05, c.shape), BSPHERE, F32, 0.02))
        else:
            shards.append(volumes(rng, rng.random((200, 3)) * 7.0, BSPHERE, F32, 0.3))
    cross = [(0, 1 + i) for i, kind in enumerate(kinds) if kind == "touch"]
    return Case(name, DEFAULT, (I32, U32), "B", shards, cross=cross)


def flat_case():
    """Shard 0: box leaves of zero extent in z, all in one plane (its root box has no volume: one box, never refined)."""
    rng = np.random.default_rng(330)
    combo = (BBOX, F32, BBOX, F32)
    flat = cube(rng, 400, 6.0, combo, 0.3)
    flat[:, 2] = flat[:, 5] = np.float32(2.375)
    return Case("flat-shard", combo, (I32, U32), "B", [flat, cube(rng, 600, 6.0, combo, 0.3)], cross=[(0, 1)])


def abutting_case():
    """A slab of unit boxes, 13 layers along x that abut at the integers, cut along the face x = 6: a box of one shard and a
    box of the other never share an interior point, those of layers 5 and 6 share part of a face, an edge or nothing (closed
    comparisons: contacts).  Within a layer the boxes sit at dyadic, otherwise arbitrary (y, z) — on a full lattice every
    node volume is a small integer and the refinement has ties at every step."""
    combo = (BBOX, F32, BBOX, F32)
    rng = np.random.default_rng(331)
    per = 16
    x = np.repeat(np.arange(13.0), per)
    yz = rng.integers(0, [5 * 1024, 3 * 1024], (13 * per, 2)) / 1024.0
    lo = np.concatenate([x[:, None], yz], axis=1)
    boxes = np.concatenate([lo, lo + 1.0], axis=1).astype(np.float32)
    assert np.array_equal(boxes.astype(np.float64), np.concatenate([lo, lo + 1.0], axis=1))  # (exactly unit, exactly abutting)
    return Case("abutting-unit-boxes", combo, (I32, U32), "B", [boxes[lo[:, 0] < 6], boxes[lo[:, 0] >= 6]],
                cross=[(0, 1)], filtered=[(1, 0)])


def translated_case(combo):
    shards = slabs(340 + combo[1], combo, 2, 700, origin=(1000.0, -2000.0, 500.0))
    return Case("translated-" + combo_name(combo), combo, (I32, U32), "B", shards, cross=[(0, 1)], filtered=[(1, 0)])


def infinite_case(which):
    """One leaf of infinite radius in shard `which` (sphere leaves under box nodes): it touches every other leaf."""
    shards = slabs(350, DEFAULT, 2, 500)
    shards[which][123, 3] = np.inf
    return Case(f"infinite-radius-in-shard-{which}", DEFAULT, (I32, U32), "B", shards, cross=[(0, 1)])


def stride_case():
    """More leaves than one trip of the filter's bounded grid covers (8192 workgroups of 256): the lower shard sits in the
    corner of the unit cube whose leaves come LAST in the upper shard's Morton order, on both sides of leaf 8192 * 256."""
    rng = np.random.default_rng(360)
    upper = volumes(rng, rng.random((2_200_000, 3)), BSPHERE, F32, 0.004)
    lower = cube(rng, 200, 0.38, DEFAULT, 0.05, origin=(0.62, 0.62, 0.62))
    return Case("second-grid-stride-trip", DEFAULT, (I32, U32), "B", [lower, upper], filtered=[(1, 0)])


def _factories():
    """name -> (path, function that makes the case): every input of the GPU file that runs all four calls (the grid-stride
    input runs two: stride_case()).  Nothing is generated until a test asks for its case."""
    out = {}
    for i, im in type_keys():
        out["types-" + combo_name(ALL_COMBOS[i], im)] = ("B", lambda i=i, im=im: type_case(i, im))
    for key in PRODUCT_KEYS:
        out["product-" + combo_name(key[1], key[2])] = ("A", lambda key=key: product_case(*key))
    out["everything-overlaps"] = ("B", overlap_case)
    out["nothing-touches"] = ("B", apart_case)
    for m in (1, 2, 3):
        out[f"bridge-{m}"] = ("B", lambda m=m: bridge_case(m))
    out["sizes-1-2-3-5-33"] = ("B", lambda: sizes_case([1, 2, 3, 5, 33], 3.0, 0.5, 370))
    out["sizes-40-3000"] = ("B", lambda: sizes_case([40, 3000], 12.0, 1.0, 371))
    out["sizes-3000-40"] = ("B", lambda: sizes_case([3000, 40], 12.0, 1.0, 372))
    out["zero-contact-set-last"] = ("B", lambda: lattice_case(("touch", "gap"), "zero-contact-set-last"))
    out["zero-contact-set-first"] = ("B", lambda: lattice_case(("gap", "touch"), "zero-contact-set-first"))
    out["zero-contact-sets-only"] = ("B", lambda: lattice_case(("gap", "gap"), "zero-contact-sets-only"))
    out["flat-shard"] = ("B", flat_case)
    out["abutting-unit-boxes"] = ("B", abutting_case)
    for combo in ((BBOX, F32, BBOX, F32), (BSPHERE, F64, BBOX, F32)):
        out["translated-" + combo_name(combo)] = ("B", lambda combo=combo: translated_case(combo))
    for which in (0, 1):
        out[f"infinite-radius-in-shard-{which}"] = ("B", lambda which=which: infinite_case(which))
    return out


FACTORIES = _factories()
_MADE = {}


def case_names(path=None, prefix=""):
    """The names of the standard cases, optionally those of one path ("A" / "B") or with one prefix: no case is made."""
    return [n for n, (p, _) in FACTORIES.items() if (path is None or p == path) and n.startswith(prefix)]


def case(name):
    """The case of that name, made on first use and kept (both test files of one process see the same arrays)."""
    if name not in _MADE:
        _MADE[name] = FACTORIES[name][1]()
        assert _MADE[name].name == name and _MADE[name].path == FACTORIES[name][0]
    return _MADE[name]
