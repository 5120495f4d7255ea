"""Every device call of the library on a SIDE stream behind a delayed producer (tests/stream_kit.py): what a time-stepping
loop does, in which the host runs several steps ahead of the GPU, and what the rest of the suite — default stream, one
synchronisation per step — never creates.

A. every public device call once through stream_kit.late(): its inputs arrive behind a delay, a launch, memset or copy
   issued anywhere but on the current stream computes the decoy's answer, and the calls that promise not to read anything
   back (NONBLOCKING) must return while the delay still runs;
B. whole `cache=` chains — rebuild, refit, pair, rays — enqueued behind ONE delay without a host read, each step's snapshot
   compared with the oracle's chain afterwards;
C. a consumer on another stream: BVHTraversal._resolve orders it behind the launch stream; _PendingTotal.item() falls back
   to the device copy of the total once its pinned slot was recycled;
D. a build chain whose hint word was recycled starts cold, with a word of its own.

Expected values are the CPU oracle's (tests/oracle_lib.py) and the checkers' brute forces, never the library's own
synchronous result.  The case table (CASES) is importable without a GPU: tests/test_host_streams.py evaluates every case's
references there, so a seed whose real and decoy answers coincide is found before the GPU run."""
import functools
import time

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402

import box_contacts_checker as bcc  # noqa: E402
import capsule_checker as cc  # noqa: E402
import closest_point_checker as cpc  # noqa: E402
import mesh_query_kit as kit  # noqa: E402
import nearest_leaves_checker as nlc  # noqa: E402
import point_crossings_checker as pcc  # noqa: E402
import ray_cast_checker as rcc  # noqa: E402
import ray_triangle_checker as rtc  # noqa: E402
import sphere_cast_checker as spc  # noqa: E402
import sphere_contacts_checker as scc  # noqa: E402
import sphere_sweep_checker as ssc  # noqa: E402
import stream_kit  # noqa: E402
import triangle_contacts_checker as tcc  # noqa: E402
import triangle_distance_checker as tdc  # noqa: E402
from test_gpu_parity import TOKENS, assert_bvh_equal, contacts_np, cuda, make_options, oracle_pairs  # noqa: E402
from test_gpu_rays_binned import knobs  # noqa: E402
from test_gpu_sort_rescue import clouds as skewed_centres, volumes as skewed_volumes  # noqa: E402

NP_F = {abi.F32: np.float32, abi.F64: np.float64}
ITEMS = 400   # query items of a mesh or cloud query (the checkers' own batches, cut to their first 400; 300 triangles and capsules:
#               their brute forces are the slow ones)

# The calls that read nothing back: their gate must be pending on return.  Confirmed by reading api.py: BVH.__init__ (raw
# volumes, any options; cache= or not; pre-wrapped records too, in place and out of place) allocates, takes a hint word and
# calls ibvh_build; refit() reads the index range once per BVH object and length (its first call with volumes), never again;
# bounding_volumes_from_triangles, generate_spheres, nearest_leaves and cast_spheres (no flag word) enqueue one launch and
# torch indexing; an LVT traversal with a cached contact buffer takes the enqueue entry.  Everything else reads a flag word
# (the mesh queries), a count (fresh LVT traversals, the list queries) or counters (BFS): judged by its result only.
NONBLOCKING = ("BVH(raw volumes) cold", "BVH(raw volumes, cache=)", "BVH(wrapped) in place", "BVH(wrapped) out of place",
               "refit(bvh)", "refit(bvh, v) from its second call on", "bounding_volumes_from_triangles", "generate_spheres",
               "nearest_leaves", "cast_spheres", "traverse / traverse_rays (LVT, cache= with a contact buffer)")


def _read_only(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _tf(flt):
    return torch.float32 if flt == abi.F32 else torch.float64


# ---- inputs: computed once, shared, never modified ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(n, seed, kind=abi.BSPHERE, flt=abi.F32, scale=1.0):
    """n volumes in the unit cube whose sizes give a few contacts per leaf (scale: a factor on the sizes)"""
    rng = np.random.default_rng(seed)
    r0 = scale * 0.5 * (3 * 8 / (4 * np.pi * n)) ** (1 / 3)
    c = rng.random((n, 3))
    if kind == abi.BSPHERE:
        v = np.concatenate([c, r0 * (0.5 + 0.5 * rng.random((n, 1)))], axis=1)
    else:
        h = r0 * (0.5 + 0.5 * rng.random((n, 3)))
        v = np.concatenate([c - h, c + h], axis=1)
    return _read_only(np.ascontiguousarray(v.astype(NP_F[flt])))[0]


@functools.lru_cache(maxsize=None)
def cloud_rays(m, seed, flt=abi.F32):
    rng = np.random.default_rng(seed)
    p = (rng.random((m, 3)) * 1.2 - 0.1).astype(NP_F[flt])
    d = (rng.random((m, 3)) - 0.5).astype(NP_F[flt])
    return _read_only(p, d)


@functools.lru_cache(maxsize=None)
def mesh(which):
    """torus40, 3,200 triangles, Float32; the decoy: the same mesh displaced"""
    t = torus_mesh(*kit.MESHES["torus40"]).astype(np.float32)
    if which == "decoy":
        t = (t.reshape(-1, 3) + np.array([0.05, 0.02, -0.03], np.float32)).reshape(-1, 9)
    return _read_only(np.ascontiguousarray(t))[0]


@functools.lru_cache(maxsize=None)
def mesh_oracle(which):
    """the oracle's BVH over the mesh's boxes: the leaf order the list queries answer in"""
    boxes = orc.volumes_from_triangles(abi.BBOX, abi.F32, mesh(which)).view(np.float32).reshape(-1, 6)
    return orc.build(boxes, abi.make_types(abi.BBOX, abi.F32, abi.BBOX, abi.F32))


def leaf_order(which):
    return mesh_oracle(which).leaves["index"].astype(np.int64)


def _seed(which, base):
    return base if which == "real" else base + 1000


def _first(arrays, n=ITEMS):
    return _read_only(*[np.ascontiguousarray(a[:n]) for a in arrays])


@functools.lru_cache(maxsize=None)
def items(query, which):
    """the late inputs of a mesh or cloud query: the checker's own batch under another seed, cut to ITEMS"""
    tris = mesh("real")
    s = lambda base: _seed(which, base)
    if query == "points":
        return _first((cpc.query_points(tris, np.float32, seed=s(7)),))
    if query == "crossing points":
        return _first((pcc.query_points(tris, np.float32, 0, seed=s(3))[::2],))
    if query == "rays":
        return _first(rcc.rays(tris, np.float32, seed=s(19)))
    if query == "moving spheres":
        return _first(ssc.spheres(tris, np.float32, seed=s(29)))
    if query == "triangles":
        moved = tcc.other(tris)
        q = moved[np.random.default_rng(s(43)).choice(len(moved), 300, replace=False)].copy()
        q[2::3, 2::3] += np.float32(0.2)   # every third one lifted clear of the mesh
        return _first((q,))
    if query == "capsules":
        return _first(cc.capsules(tris, np.float32, seed=s(61)), 300)
    if query == "boxes":
        return _first(bcc.boxes(tris, np.float32, seed=s(71)))
    if query == "spheres":
        c = cpc.query_points(tris, np.float32, seed=s(7))[:ITEMS]
        r = (np.random.default_rng(s(21)).random(ITEMS) * 4 * scc.mean_edge(tris)).astype(np.float32)
        return _first((c, r))
    if query == "cloud casts":
        return _first(spc.cloud(np.float32, seed=s(7))[1:])
    if query == "cloud points":
        return _first(((np.random.default_rng(s(2)).random((ITEMS, 3)) * 1.5 - 0.25).astype(np.float32),))
    raise KeyError(query)


@functools.lru_cache(maxsize=None)
def cast_cloud():
    """the 3,300 spheres cast_spheres is asked about, and the oracle's tree over them"""
    spheres = _read_only(spc.cloud(np.float32)[0])[0]
    order, boxes, _ = spc.host_tree(spheres)
    return spheres, order, boxes


# ---- comparators --------------------------------------------------------------------------------------------------------------
def _fields(fields):
    """index by value, every other field by dtype and bit for bit"""
    def check(got, exp):
        for f in fields:
            g, e = getattr(got, f).cpu().numpy(), getattr(exp, f)
            assert g.shape == e.shape, f
            if f == "index":
                assert (g == e).all(), (f, int((g != e).sum()))
            else:
                assert g.dtype == e.dtype and kit.bits(g) == kit.bits(e), (f, int((g != e).sum()))
    return check


def _check_crossings(got, exp):
    assert (got.crossings.cpu().numpy() == exp.crossings).all() and (got.winding.cpu().numpy() == exp.winding).all()
    assert (exp.crossings > 0).sum() > ITEMS // 8


def _check_bvh(g, o):
    assert_bvh_equal(o, g)


def _check_lvt(t, exp):
    got = contacts_np(t)
    assert got.shape == exp.shape and (got == exp).all(), (got.shape, exp.shape)


def _check_bfs(t, exp):
    pairs, checks = exp
    assert sorted(map(tuple, contacts_np(t).tolist())) == pairs and t.num_checks == checks


def _sorted_pairs(c):
    return sorted(map(tuple, oracle_pairs(c).tolist()))


# ---- the case table -------------------------------------------------------------------------------------------------------------
class Case:
    """name; inputs(which) -> tuple of numpy arrays for which in ("real", "decoy"); reference(arrays) -> the CPU answer;
    call(ctx, X) -> the library's result on the current stream; check(result, answer); setup() -> ctx, run synchronously on
    the side stream before the case (None: nothing); nonblocking: the NONBLOCKING entry the call falls under, or None;
    around: a context manager factory held around the whole case (a tuning knob)"""

    def __init__(self, name, inputs, reference, call, check, setup=None, nonblocking=None, around=None):
        assert nonblocking is None or nonblocking in NONBLOCKING
        self.name, self.inputs, self.reference, self.call, self.check = name, inputs, reference, call, check
        self.setup, self.nonblocking, self.around = setup, nonblocking, around
        self._expected = {}

    def expected(self, which):
        if which not in self._expected:
            with np.errstate(all="ignore"):
                self._expected[which] = self.reference(self.inputs(which))
        return self._expected[which]


def _build_case(n, kind=abi.BSPHERE, flt=abi.F32, it=abi.I32, mt=abi.U32, tag=""):
    types = abi.make_types(kind, flt, abi.BBOX, flt, it, mt)
    plain = (kind, flt, it, mt) == (abi.BSPHERE, abi.F32, abi.I32, abi.U32)

    def call(ctx, X):
        if plain:
            return ibvh.BVH(X[0])   # (no options: the call a time-stepping loop makes)
        return ibvh.BVH(X[0], TOKENS[abi.BBOX](_tf(flt)), options=make_options(types))
    return Case(f"BVH cold {n}{tag}", lambda which: (cloud(n, _seed(which, n), kind, flt),), lambda a: orc.build(a[0], types),
                call, _check_bvh, nonblocking="BVH(raw volumes) cold")


def _cached_build_case():
    n = 20000
    setup = lambda: {"g": ibvh.BVH(cuda(cloud(n, 5)))}

    def call(ctx, X):
        ctx["g"] = ibvh.BVH(X[0], cache=ctx["g"])
        return ctx["g"]
    return Case("BVH cache= 20000", lambda which: (cloud(n, _seed(which, 6)),), lambda a: orc.build(a[0], abi.make_types()), call,
                _check_bvh, setup=setup, nonblocking="BVH(raw volumes, cache=)")


def _wrapped_case(out_of_place):
    n = 3000
    types = abi.make_types()
    user = np.random.default_rng(n).permutation(n).astype(np.int32) * 3 + 7

    def call(ctx, X):
        bv = ibvh.BoundingVolumes(types, n)
        bv.volume.copy_(X[0])
        bv.index.copy_(ctx["user"])
        g = ibvh.BVH(bv, _out_of_place=out_of_place)
        assert (g.leaves.buf.data_ptr() == bv.buf.data_ptr()) == (not out_of_place)
        return g
    name = "out of place" if out_of_place else "in place"
    return Case(f"BVH wrapped {name}", lambda which: (cloud(n, _seed(which, 8)),), lambda a: orc.build(a[0], types, indices=user),
                call, _check_bvh, setup=lambda: {"user": cuda(user)}, nonblocking=f"BVH(wrapped) {name}")


def _refit_case(with_volumes):
    """the BVH is built from a base cloud beforehand; the moved volumes arrive late, in the user's order (refit(bvh, v)) or
    already in the leaves' order, copied into the leaves on the stream (refit(bvh))"""
    n = 3000
    types = abi.make_types()
    base = cloud(n, 9)

    def moved(which):
        rng = np.random.default_rng(_seed(which, 10))
        v = base.copy()
        v[:, :3] += ((rng.random((n, 3)) * 2 - 1) * 0.01).astype(np.float32)
        if not with_volumes:
            v = v[orc.build(base, types).leaves["index"].astype(np.int64) - 1]
        return _read_only(np.ascontiguousarray(v))

    def reference(a):
        o = orc.build(base, types)
        leaves = o.leaves.copy()
        vols = orc.as_volumes(a[0], abi.BSPHERE, abi.F32)
        leaves["volume"] = vols[leaves["index"].astype(np.int64) - 1] if with_volumes else vols
        return leaves, orc.aggregate(types, o.tree, 1, leaves)

    def call(ctx, X):
        if with_volumes:
            return ibvh.refit(ctx["g"], X[0])
        ctx["g"].leaves.volume.copy_(X[0])
        return ibvh.refit(ctx["g"])

    def check(g, exp):
        leaves, nodes = exp
        assert g.leaves.to_numpy().tobytes() == leaves.tobytes() and g.nodes.cpu().numpy().tobytes() == nodes.tobytes()
        assert int(g._refit_flag.item()) == 0
    return Case("refit(bvh, v)" if with_volumes else "refit(bvh)", functools.lru_cache(maxsize=None)(moved), reference, call, check,
                setup=lambda: {"g": ibvh.BVH(cuda(base))},
                nonblocking="refit(bvh, v) from its second call on" if with_volumes else "refit(bvh)")


def _volumes_case(kind):
    token = TOKENS[kind]

    def check(got, exp):
        assert got.cpu().numpy().tobytes() == exp.tobytes()
    return Case(f"bounding_volumes_from_triangles {token.__name__}", lambda which: (mesh(which),),
                lambda a: orc.volumes_from_triangles(kind, abi.F32, a[0]), lambda ctx, X: ibvh.bounding_volumes_from_triangles(X[0], token(torch.float32)),
                check, nonblocking="bounding_volumes_from_triangles")


def _generate_case():
    def check(got, exp):
        assert got.cpu().numpy().tobytes() == exp.tobytes()
    return Case("generate_spheres", lambda which: (), lambda a: orc.generate_spheres_f32(20000, 42, r0=0.01),
                lambda ctx, X: ibvh.generate_spheres(20000, 42, r0=0.01), check, nonblocking="generate_spheres")


def _traverse_case(shape, alg, binned=False):
    """fresh traversals: the clouds (and the rays) arrive late, the BVHs are built from them on the stream"""
    n, n2, m = 3000, 2000, 500
    types = abi.make_types()
    lvt = alg == "LVT"
    token = ibvh.LVTTraversal if lvt else ibvh.BFSTraversal

    def inputs(which):
        if shape == "self":
            return (cloud(n, _seed(which, 11)),)
        if shape == "pair":
            return cloud(n, _seed(which, 12)), cloud(n2, _seed(which, 13))
        return (cloud(n, _seed(which, 14)),) + cloud_rays(m, _seed(which, 15))

    def reference(a):
        o = orc.build(a[0], types)
        if shape == "self":
            return oracle_pairs(orc.traverse_lvt(o)[0]) if lvt else (lambda c, r: (_sorted_pairs(c), r.num_checks))(*orc.traverse_bfs(o))
        if shape == "pair":
            o2 = orc.build(a[1], types)
            return oracle_pairs(orc.traverse_pair_lvt(o, o2)[0]) if lvt else (lambda c, r: (_sorted_pairs(c), r.num_checks))(*orc.traverse_pair_bfs(o, o2))
        return oracle_pairs(orc.traverse_rays_lvt(o, a[1], a[2])[0]) if lvt else (lambda c, r: (_sorted_pairs(c), r.num_checks))(*orc.traverse_rays_bfs(o, a[1], a[2]))

    def call(ctx, X):
        g = ibvh.BVH(X[0])
        if shape == "self":
            return ibvh.traverse(g, token())
        if shape == "pair":
            return ibvh.traverse(g, ibvh.BVH(X[1]), token())
        return ibvh.traverse_rays(g, X[1].t(), X[2].t(), token())
    return Case(f"traverse {shape} {alg}{' binned' if binned else ''}", inputs, reference, call, _check_lvt if lvt else _check_bfs,
                around=(lambda: knobs(rays_binned=2, rays_subtree_depth=4)) if binned else None)


def _resolve_case():
    types = abi.make_types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32)

    def inputs(which):
        p, d = rtc.aimed_rays(ITEMS, mesh("real"), np.float32)
        if which == "decoy":
            p, d = p[::-1], d[::-1]
        return (mesh(which),) + _first((p, d))

    def reference(a):
        o = orc.build(orc.volumes_from_triangles(abi.BSPHERE, abi.F32, a[0]).view(np.float32).reshape(-1, 4), types)
        contacts, counts = orc.traverse_rays_lvt(o, a[1], a[2])
        return rtc.resolve(counts, oracle_pairs(contacts).astype(np.int32), a[0], a[1], a[2])

    def call(ctx, X):
        g = ibvh.BVH(ibvh.bounding_volumes_from_triangles(X[0], ibvh.BSphere(torch.float32)))
        return ibvh.resolve_triangles(ibvh.traverse_rays(g, X[1].t(), X[2].t()), X[0], X[1].t(), X[2].t())

    def check(got, exp):
        assert (got.index.cpu().numpy() == exp.index).all() and (exp.index > 0).sum() > ITEMS // 2
        assert kit.bits(got.t.cpu().numpy()) == kit.bits(exp.t) and kit.bits(got.uv.cpu().numpy()) == kit.bits(exp.uv)
    return Case("resolve_triangles", inputs, reference, call, check)


def _mesh_setup():
    bvh, tdev = kit.build(mesh("real"))
    assert (kit.leaf_order(bvh) == leaf_order("real")).all()
    return {"bvh": bvh, "tris": tdev}


def _mesh_case(name, query, reference, call, check, **kw):
    """the BVH is built synchronously from the real mesh beforehand; the query items arrive late"""
    return Case(name, lambda which: items(query, which), lambda a: reference(mesh("real"), *a),
                lambda ctx, X: call(ctx["bvh"], ctx["tris"], *X), check, setup=_mesh_setup, **kw)


def _list_check(query):
    return lambda got, exp: kit.assert_equal(query, got, exp, query.entry)


def _late_mesh_case(name, query, reference, call, check):
    """... and with the triangles late as well: volumes, build and query behind one delay"""
    def run(ctx, X):
        boxes = ibvh.bounding_volumes_from_triangles(X[0], ibvh.BBox(torch.float32))
        return call(ibvh.BVH(boxes, ibvh.BBox(torch.float32)), *X)
    return Case(name, lambda which: (mesh(which),) + items(query, which), lambda a: reference(which_mesh(a[0]), *a), run, check)


def which_mesh(tris):
    return "real" if tris is mesh("real") else "decoy"


def _cast_spheres_setup():
    spheres, order, _ = cast_cloud()
    bvh = ibvh.BVH(cuda(spheres))
    assert (bvh.leaves.index.cpu().numpy() == order).all()
    return {"bvh": bvh}


def _nearest_setup():
    return {"bvh": ibvh.BVH(cuda(cloud(3000, 16)))}


CASES = [_build_case(1500), _build_case(3000), _build_case(20000),
         _build_case(20000, kind=abi.BBOX, tag=" BBox"), _build_case(20000, flt=abi.F64, tag=" Float64"),
         _build_case(20000, it=abi.I64, tag=" Int64"), _build_case(20000, mt=abi.U64, tag=" UInt64"),
         _cached_build_case(), _wrapped_case(False), _wrapped_case(True), _refit_case(True), _refit_case(False),
         _volumes_case(abi.BBOX), _volumes_case(abi.BSPHERE), _generate_case(),
         _traverse_case("self", "LVT"), _traverse_case("self", "BFS"), _traverse_case("pair", "LVT"), _traverse_case("pair", "BFS"),
         _traverse_case("rays", "LVT"), _traverse_case("rays", "BFS"), _traverse_case("rays", "LVT", binned=True), _resolve_case(),
         _mesh_case("closest_points", "points", lambda t, p: cpc.brute_force(t, p, idt=np.int64),
                    lambda g, T, p: ibvh.closest_points(g, T, p.t()),
                    lambda got, exp: _fields(("index", "d2", "point"))(_Renamed(got, d2="distance2"), exp)),
         Case("nearest_leaves", lambda which: items("cloud points", which),
              lambda a: nlc.brute_force(cloud(3000, 16), np.arange(1, 3001), a[0], 3, idt=np.int64),
              lambda ctx, X: ibvh.nearest_leaves(ctx["bvh"], X[0].t(), k=3), _fields(("index", "d2")), setup=_nearest_setup,
              nonblocking="nearest_leaves"),
         _mesh_case("point_crossings", "crossing points", lambda t, p: pcc.brute_force(t, p, 0, idt=np.int64),
                    lambda g, T, p: ibvh.point_crossings(g, T, p.t()), _check_crossings),
         _mesh_case("cast_rays closest", "rays", rcc.brute_force, lambda g, T, p, d: ibvh.cast_rays(g, T, p.t(), d.t()),
                    functools.partial(kit.assert_closest, kit.CAST_RAYS)),
         _mesh_case("cast_rays any-hit", "rays", rcc.brute_force, lambda g, T, p, d: ibvh.cast_rays(g, T, p.t(), d.t(), any_hit=True),
                    functools.partial(kit.assert_any, kit.CAST_RAYS)),
         _mesh_case("sweep_spheres", "moving spheres", ssc.brute_force, lambda g, T, p, d, r: ibvh.sweep_spheres(g, T, p.t(), d.t(), r),
                    functools.partial(kit.assert_closest, kit.SWEEP_SPHERES)),
         Case("cast_spheres", lambda which: items("cloud casts", which),
              lambda a: spc.brute_force(cast_cloud()[0], cast_cloud()[1], cast_cloud()[2], *a),
              lambda ctx, X: ibvh.cast_spheres(ctx["bvh"], X[0].t(), X[1].t(), X[2]), functools.partial(kit.assert_closest, kit.CAST_SPHERES),
              setup=_cast_spheres_setup, nonblocking="cast_spheres"),
         _mesh_case("triangle_distances", "triangles", tdc.brute_force, lambda g, T, q: ibvh.triangle_distances(g, T, q),
                    _fields(("index", "d2", "point_query", "point_mesh", "kind"))),
         _mesh_case("segment_distances", "capsules", lambda t, a, b, r: cc.brute_force_distances(t, a, b),
                    lambda g, T, a, b, r: ibvh.segment_distances(g, T, a.t(), b.t()), _fields(cc.FIELDS)),
         _mesh_case("sphere_contacts", "spheres", lambda t, c, r: scc.brute_force(t, c, r, leaf_order=leaf_order("real"), idt=np.int64),
                    lambda g, T, c, r: ibvh.sphere_contacts(g, T, c.t(), r), _list_check(scc.QUERY)),
         _mesh_case("triangle_contacts", "triangles", lambda t, q: tcc.brute_force(t, q, leaf_order=leaf_order("real")),
                    lambda g, T, q: ibvh.triangle_contacts(g, T, q), _list_check(tcc.QUERY)),
         _mesh_case("capsule_contacts", "capsules", lambda t, a, b, r: cc.brute_force_contacts(t, a, b, r, leaf_order=leaf_order("real")),
                    lambda g, T, a, b, r: ibvh.capsule_contacts(g, T, a.t(), b.t(), r), _list_check(cc.QUERY)),
         _mesh_case("box_contacts", "boxes", lambda t, c, h, R: bcc.brute_force_contacts(t, c, h, R, leaf_order=leaf_order("real")),
                    lambda g, T, c, h, R: ibvh.box_contacts(g, T, c.t(), h.t(), R), _list_check(bcc.QUERY)),
         _late_mesh_case("cast_rays, triangles late", "rays", lambda w, t, p, d: rcc.brute_force(t, p, d),
                         lambda g, T, p, d: ibvh.cast_rays(g, T, p.t(), d.t()), functools.partial(kit.assert_closest, kit.CAST_RAYS)),
         _late_mesh_case("sphere_contacts, triangles late", "spheres",
                         lambda w, t, c, r: scc.brute_force(t, c, r, leaf_order=leaf_order(w), idt=np.int64),
                         lambda g, T, c, r: ibvh.sphere_contacts(g, T, c.t(), r), _list_check(scc.QUERY))]


class _Renamed:
    """a result under the checker's field names"""

    def __init__(self, obj, **names):
        for new, old in names.items():
            setattr(self, new, getattr(obj, old))
        for k, v in vars(obj).items():
            if k not in names and not hasattr(self, k):
                setattr(self, k, v)


CASE_NAMES = [c.name for c in CASES]
assert len(set(CASE_NAMES)) == len(CASES)


def _log(text):
    print(text, flush=True)


@pytest.fixture(scope="module", autouse=True)
def calibration():
    stream_kit.calibrate(_log)


# ---- the kit's own test: sensitivity ------------------------------------------------------------------------------------------
def test_kit_detects_an_operation_on_the_default_stream():
    """An f that is a pure torch operation issued on the DEFAULT stream fails late() on its result — it doubled the decoy —,
    and the same f on the side stream passes.  The library is not involved."""
    real, decoy = (np.arange(4096, dtype=np.float32),), (np.arange(4096, dtype=np.float32)[::-1].copy(),)

    class WrongResult(AssertionError):
        pass

    def check(got, exp):
        if got.cpu().numpy().tobytes() != exp.tobytes():
            raise WrongResult()

    def misplaced(X):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return X[0] * 2
    args = dict(real=real, decoy=decoy, check=check, expect_real=real[0] * 2, expect_decoy=decoy[0] * 2, nonblocking=True, log=_log)
    rep = stream_kit.late(lambda X: X[0] * 2, stream=stream_kit.side_stream(), name="kit: on the side stream", **args)
    assert rep.pending
    with pytest.raises(WrongResult):
        stream_kit.late(misplaced, stream=stream_kit.side_stream(), name="kit: on the default stream", **args)
    torch.cuda.synchronize()


# ---- A. every public device call, inputs delivered late -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_late_inputs(name):
    case = CASES[CASE_NAMES.index(name)]
    S = stream_kit.side_stream()
    around = case.around() if case.around else None
    if around:
        around.__enter__()
    try:
        ctx = None
        if case.setup:
            with torch.cuda.stream(S):
                ctx = case.setup()
            S.synchronize()
        stream_kit.late(lambda X: case.call(ctx, X), case.inputs("real"), case.inputs("decoy"), S, case.check,
                        case.expected("real"), case.expected("decoy"), nonblocking=case.nonblocking is not None, name=name, log=_log)
    finally:
        if around:
            around.__exit__(None, None, None)
        torch.cuda.synchronize()


def test_two_streams_share_one_bvh():
    """S1 and S2, each behind its own delay with its own late batch: cast_rays against the mesh's BVH and nearest_leaves
    against the cloud's, both BVHs shared.  Each result is its own reference."""
    with torch.cuda.stream(stream_kit.side_stream()):
        mctx, nctx = _mesh_setup(), _nearest_setup()
    torch.cuda.synchronize()
    tris, vols = mesh("real"), cloud(3000, 16)
    streams, X, real, outs = [stream_kit.side_stream(), stream_kit.side_stream(1)], [], [], []
    batches = [tuple(items("rays", w) + items("cloud points", w)) for w in ("real", "decoy")]   # S1's batch, S2's batch
    for S, mine, other in zip(streams, batches, batches[::-1]):
        with torch.cuda.stream(S):
            real.append([cuda(a) for a in mine])
            X.append([cuda(a).clone() for a in other])   # each stream's stale state: the OTHER stream's batch
    torch.cuda.synchronize()
    gates = []
    for S, x, r in zip(streams, X, real):
        with torch.cuda.stream(S):
            stream_kit.enqueue_delay(stream_kit.MIN_DELAY_MS)
            for dst, src in zip(x, r):
                dst.copy_(src, non_blocking=True)
            gates.append(torch.cuda.Event())
            gates[-1].record(S)
    for S, x, gate in zip(streams, X, gates):   # (the calls that do not block first, on both streams)
        with torch.cuda.stream(S):
            outs.append([ibvh.nearest_leaves(nctx["bvh"], x[2].t(), k=3), None, not gate.query()])
    for S, x, out in zip(streams, X, outs):
        with torch.cuda.stream(S):
            out[1] = ibvh.cast_rays(mctx["bvh"], mctx["tris"], x[0].t(), x[1].t())
    torch.cuda.synchronize()
    for (near, cast, pending), mine in zip(outs, batches):
        assert pending, "inconclusive: nearest_leaves returned after its stream's gate had fired"
        _fields(("index", "d2"))(near, nlc.brute_force(vols, np.arange(1, 3001), mine[2], 3, idt=np.int64))
        kit.assert_closest(kit.CAST_RAYS, cast, rcc.brute_force(tris, mine[0], mine[1]))
    a, b = (rcc.brute_force(tris, m[0], m[1]) for m in batches)
    assert stream_kit.answers_differ(a, b)


# ---- B. the host runs ahead through a whole chain -----------------------------------------------------------------------------
CHAIN_N = 20000


@functools.lru_cache(maxsize=None)
def chain_clouds():
    """8 inputs of 20,000 BSphere{Float32}: a uniform cloud, then one cluster, uniform, eight clusters, ... — the distribution
    changes abruptly under a hint word that is several builds stale"""
    out = []
    for k in range(8):
        if k % 2 == 0:
            out.append(cloud(CHAIN_N, 300 + k))
        else:
            rng = np.random.default_rng(300 + k)
            out.append(_read_only(skewed_volumes(skewed_centres("one_cluster" if k % 4 == 1 else "eight_clusters", CHAIN_N, rng),
                                                 (abi.BSPHERE, abi.F32), rng))[0])
    return out


def _snapshots(g, t):
    return g.leaves.buf.clone(), g.nodes.clone(), t._cache1.clone(), t._pending[0]


def _assert_step(k, snap, leaves, nodes, pairs):
    got_leaves, got_nodes, got_list, pending = snap
    assert got_leaves.cpu().numpy().tobytes() == leaves.tobytes(), f"step {k}: leaves"
    assert got_nodes.cpu().numpy().tobytes() == nodes.tobytes(), f"step {k}: nodes"
    total = int(pending.item())
    assert total == len(pairs), f"step {k}: total {total}, the oracle's {len(pairs)}"
    assert (got_list[:total].cpu().numpy().astype(np.int64) == pairs).all(), f"step {k}: contact list"


@pytest.mark.parametrize("refits", [False, True], ids=["rebuilds", "rebuilds and refits"])
def test_chain_enqueued_behind_one_delay(refits):
    """g = BVH(X_k, cache=g) -> t = traverse(g, cache=t) -> snapshots, 8 steps behind one delay and no host read in the loop
    (the gate is still pending after it); with refits, every second step moves the leaves in place and refits instead."""
    types = abi.make_types()
    inputs = chain_clouds()
    rng = np.random.default_rng(77)
    deltas = [((rng.random((CHAIN_N, 3)) * 2 - 1) * 1e-4).astype(np.float32) for _ in range(8)]
    # the oracle's chain
    expected, o = [], None
    for k in range(8):
        if refits and k % 2 == 1:
            leaves = o.leaves.copy()
            v = np.ascontiguousarray(leaves["volume"]).view(np.float32).reshape(CHAIN_N, 4).copy()
            v[:, :3] += deltas[k]
            leaves["volume"] = orc.as_volumes(v, abi.BSPHERE, abi.F32)
            o = orc.HostBVH(types, o.tree, 1, leaves, orc.aggregate(types, o.tree, 1, leaves), o.skips, o.extrema)
        else:
            o = orc.build(inputs[k], types)
        expected.append((o.leaves, o.nodes, oracle_pairs(orc.traverse_lvt(o)[0])))
    dense = max(range(8), key=lambda k: len(expected[k][2]))
    assert min(len(e[2]) for e in expected) > 0 and all(len(expected[k][2]) != len(expected[k + 1][2]) for k in range(7))
    S = stream_kit.side_stream()
    with torch.cuda.stream(S):
        X = [cuda(v) for v in inputs]
        D = [cuda(d) for d in deltas]
        g = ibvh.BVH(X[dense])
        t = ibvh.traverse(ibvh.BVH(cuda(np.ascontiguousarray(expected[dense][0]["volume"]).view(np.float32).reshape(-1, 4))) if refits else g)
        assert t.num_contacts >= len(expected[dense][2])   # (sized by the densest step: every step takes the enqueue path)
        S.synchronize()
        t0 = time.perf_counter()
        stream_kit.enqueue_delay(stream_kit.MAX_DELAY_MS / 4)
        gate = torch.cuda.Event()
        gate.record(S)
        snaps = []
        for k in range(8):
            if refits and k % 2 == 1:
                g.leaves.volume[:, :3] += D[k]
                g = ibvh.refit(g)
            else:
                g = ibvh.BVH(X[k], cache=g)
            t = ibvh.traverse(g, cache=t)
            assert t._pending is not None, f"step {k} did not take the enqueue path"
            snaps.append(_snapshots(g, t))
        host = time.perf_counter() - t0
        pending = not gate.query()
        _log(f"chain ({'rebuilds and refits' if refits else 'rebuilds'}): delay {stream_kit.MAX_DELAY_MS / 4:.0f} ms, 8 steps enqueued in "
             f"{1e3 * host:.2f} ms on the host, gate {'pending' if pending else 'fired'} after the loop")
        assert pending, f"inconclusive: the gate fired while the loop was enqueued ({1e3 * host:.2f} ms on the host): something in it waited"
        S.synchronize()
        for k in range(8):
            _assert_step(k, snaps[k], *expected[k])


@pytest.mark.parametrize("shape", ["pair", "rays"])
def test_pair_and_ray_chains_enqueued_behind_one_delay(shape):
    """two steps each: 5,000 and 3,000 leaves, 700 rays"""
    types = abi.make_types()
    A = [cloud(5000, 400 + k) for k in range(2)]
    B = [cloud(3000, 410 + k) for k in range(2)]
    R = [cloud_rays(700, 420 + k) for k in range(2)]
    expected = []
    for k in range(2):
        oa, ob = orc.build(A[k], types), orc.build(B[k], types)
        with np.errstate(all="ignore"):
            c = orc.traverse_pair_lvt(oa, ob)[0] if shape == "pair" else orc.traverse_rays_lvt(oa, R[k][0], R[k][1])[0]
        expected.append((oa, ob, oracle_pairs(c)))
    assert len(expected[0][2]) != len(expected[1][2]) and min(len(e[2]) for e in expected) > 0
    dense = int(len(expected[1][2]) > len(expected[0][2]))
    S = stream_kit.side_stream()

    def step(k, ga, gb, t, XA, XB, XR):
        ga = ibvh.BVH(XA[k], cache=ga)
        if shape == "pair":
            gb = ibvh.BVH(XB[k], cache=gb)
            return ga, gb, ibvh.traverse(ga, gb, cache=t)
        return ga, gb, ibvh.traverse_rays(ga, XR[k][0].t(), XR[k][1].t(), cache=t)
    with torch.cuda.stream(S):
        XA, XB, XR = [cuda(a) for a in A], [cuda(b) for b in B], [(cuda(p), cuda(d)) for p, d in R]
        ga, gb, t = step(dense, None, None, None, XA, XB, XR)
        assert t.num_contacts == len(expected[dense][2])
        S.synchronize()
        stream_kit.enqueue_delay(stream_kit.MAX_DELAY_MS / 4)
        gate = torch.cuda.Event()
        gate.record(S)
        snaps = []
        for k in range(2):
            ga, gb, t = step(k, ga, gb, t, XA, XB, XR)
            assert t._pending is not None
            snaps.append((ga.leaves.buf.clone(), ga.nodes.clone(), t._cache1.clone(), t._pending[0],
                          gb.leaves.buf.clone() if gb is not None else None))
        assert not gate.query(), "inconclusive: the gate fired while the chain was enqueued"
        S.synchronize()
        for k in range(2):
            oa, ob, pairs = expected[k]
            _assert_step(k, snaps[k][:4], oa.leaves, oa.nodes, pairs)
            if shape == "pair":
                assert snaps[k][4].cpu().numpy().tobytes() == ob.leaves.tobytes()


# ---- C. a consumer on another stream ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_cloud():
    """20,000 spheres with about 2e5 contacts, and the oracle's list"""
    v = cloud(20000, 500, scale=1.8)
    pairs = oracle_pairs(orc.traverse_lvt(orc.build(v, abi.make_types()))[0])
    assert 1.5e5 < len(pairs) < 3e5, len(pairs)
    return v, pairs


@pytest.mark.parametrize("buffer", ["large enough", "too small"])
def test_contacts_read_on_another_stream(buffer):
    """A cached self-traversal is enqueued on S into a buffer filled with -1; stream B reads .contacts and clones it at once.
    The pinned total is published before the writing pass has finished, so without the wait for the launch stream in
    BVHTraversal._resolve the clone overlaps that pass and rows of -1 (or of the previous list) show.  Detection of a
    missing wait is likely, not certain — it is a race —; a correct library never fails this.  With a cached buffer that is
    too small the writing pass itself runs on B, from counts and scratch produced on S."""
    v, pairs = dense_cloud()
    S, B = stream_kit.side_stream(), stream_kit.side_stream(1)
    with torch.cuda.stream(S):
        g = ibvh.BVH(cuda(v))
        prev = ibvh.traverse(g if buffer == "large enough" else ibvh.BVH(cuda(cloud(20000, 501))))
        assert (prev.num_contacts == len(pairs)) if buffer == "large enough" else (0 < prev.num_contacts < len(pairs) // 2)
        S.synchronize()
        prev._cache1.fill_(-1)
        t = ibvh.traverse(g, cache=prev)
        assert t._pending is not None
    with torch.cuda.stream(B):
        got = t.contacts.clone()
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.int64)
    assert got.shape == pairs.shape and not (got == -1).any() and (got == pairs).all()
    assert (t._cache1.data_ptr() == prev._cache1.data_ptr()) == (buffer == "large enough")


def _tiny(seed, spread):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((8, 3)) * spread, np.full((8, 1), 0.3)], axis=1).astype(np.float32)


def test_total_read_after_its_pinned_slot_was_recycled():
    """Traversal X is enqueued on S behind a delay and not read; an independent chain Y on the default stream then takes
    pinned slots — reading each total as it goes, so that its own 64-entry ring never overflows — until X's slot has been
    handed out again, across the wrap of the real ring of 8,192 slots (whose drain waits for X's delay).  X's total then
    comes from the device copy and is X's own; every total Y read is Y's own.  Thousands of tiny traversals: about a second
    or two of host time."""
    types = abi.make_types()
    vx, vy = _tiny(1, 0.2), _tiny(2, 1.5)   # X: all 28 pairs touch; Y: spread out
    ex, ey = (len(orc.traverse_lvt(orc.build(v, types))[0]) for v in (vx, vy))
    assert ex == 28 and 0 < ey < 28
    hw = api._host_words()
    S = stream_kit.side_stream()
    with torch.cuda.stream(S):
        gx = ibvh.BVH(cuda(vx))
        x0 = ibvh.traverse(gx)
        assert x0.num_contacts == ex
        S.synchronize()
        stream_kit.enqueue_delay(200.0)
        X = ibvh.traverse(gx, cache=x0)
    pending = X._pending[0]
    takes = (pending.hslot - hw.next) % hw.SLOTS + 1   # (do not assume an empty ring)
    assert hw.generation[pending.hslot] == pending.hgen and takes == hw.SLOTS
    gy = ibvh.BVH(cuda(vy))
    ty = ibvh.traverse(gy)
    t0 = time.perf_counter()
    wrong = 0
    for _ in range(takes):
        ty = ibvh.traverse(gy, cache=ty)
        assert ty._pending is not None
        wrong += ty.num_contacts != ey
    _log(f"ring lap: {takes} cached 8-leaf traversals read one by one in {time.perf_counter() - t0:.2f} s")
    assert wrong == 0, f"{wrong} of Y's totals were not its own"
    assert hw.generation[pending.hslot] != pending.hgen, "X's slot was not handed out again"
    assert int(pending.item()) == ex
    assert X.num_contacts == ex and (contacts_np(X) == oracle_pairs(orc.traverse_lvt(orc.build(vx, types))[0])).all()
    torch.cuda.synchronize()


# ---- D. the hint ring -----------------------------------------------------------------------------------------------------------
def test_a_chain_whose_hint_word_was_recycled_starts_cold():
    """HINT_SLOTS cold builds of 8-leaf clouds recycle the hint word of a 20,000-leaf chain; its next rebuild does not take the
    fast path, holds a new word, equals the oracle and leaves the word's new owner's value alone."""
    types = abi.make_types()
    rng = np.random.default_rng(9)
    v = skewed_volumes(skewed_centres("eight_clusters", CHAIN_N, rng), (abi.BSPHERE, abi.F32), rng)
    o = orc.build(v, types)
    hw = api._host_words()
    dev = cuda(v)
    b = ibvh.BVH(dev)
    for _ in range(2):
        b = ibvh.BVH(dev, cache=b)
    torch.cuda.synchronize()
    assert_bvh_equal(o, b)
    assert b._skew.valid() and int(hw.words[b._skew.slot]) != 0, "the chain's hint is trivial"
    takes = (b._skew.slot - hw.SLOTS - hw.next_hint) % hw.HINT_SLOTS + 1   # (counted from next_hint: the ring need not be empty)
    small = cuda(_tiny(3, 1.0))
    for _ in range(takes):
        owner = ibvh.BVH(small)
    torch.cuda.synchronize()
    assert not b._skew.valid() and owner._skew.valid() and owner._skew.slot == b._skew.slot
    word = int(hw.words[owner._skew.slot])
    g = ibvh.BVH(dev, cache=b)
    torch.cuda.synchronize()
    assert g._fast is not b._fast, "the rebuild took the fast path on a recycled hint word"
    assert g._skew is not b._skew and g._skew.valid() and g._skew.slot != b._skew.slot
    assert_bvh_equal(o, g)
    assert int(hw.words[owner._skew.slot]) == word, "the rebuild wrote into the hint word another build owns"
    again = ibvh.BVH(dev, cache=g)   # ... and the chain goes on from there, on the fast path
    torch.cuda.synchronize()
    assert again._fast is g._fast and again._skew is g._skew
    assert_bvh_equal(o, again)
