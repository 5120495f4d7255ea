"""The BFS level kernel (csrc/ibvh_bfs.hip, level_kernel<I, PolA, PolB>) on every policy, volume type, index type and queue
route, step by step against tests/bfs_levels_checker.py (pinned to the oracle by tests/test_host_bfs_levels.py).

The shipped grid is CUs x bfs_wg_per_cu workgroups, so at test sizes a workgroup runs one chunk and flushes once.  The knob
"bfs_grid" launches exactly k workgroups: with k = 1 .. 3 a queue of 20,000 pairs is dozens of chunks per workgroup, and the
register rotation of the chunk pipeline, the filler lanes past the queue's end, several flushes per workgroup and the reuse
of the staging area after a flush all run on trees the checker walks in a second.  Every case first asserts FROM THE CHECKER
ALONE that its input forces the route it is named after (pigeonhole over the workgroups); every comparison is exact: per
step the source count and the generated count, the contact list as a sorted array, num_checks, and — for the overflow
protocol through the raw ABI — resume_step, resume_num, required_capacity and the kept queue's contents."""
import ctypes as C

import numpy as np
import pytest

import bfs_levels_checker as chk
import oracle_lib as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402,F401
from implicitbvh_amd import abi, api, lib  # noqa: E402

from test_gpu_parity import ALL_COMBOS, build_both, contacts_np, cuda, oracle_pairs, random_volumes  # noqa: E402
from test_host_bfs_levels import irregular_rays  # noqa: E402

INDEX_TYPES = [(abi.I32, abi.U32), (abi.I64, abi.U64)]
RAY_COMBOS = [c for c in ALL_COMBOS if c[1] == c[3]]
TORCH_I = {abi.I32: torch.int32, abi.I64: torch.int64}
PAIR_NARROWS = (abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT)


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(autouse=True)
def _default_grid():
    yield
    lib.set_tuning("bfs_grid", 0)


# ---------------------------------------------------------------------------------------------
# a traversal: what the checker, the oracle and the library each make of it
# ---------------------------------------------------------------------------------------------
class Case:
    """kind: "self" | "pair" | "rays"; o / g: the oracle's and the library's BVHs (one, or two for a pair); sl: start
    level(s); rays: (points, directions) as (n, 3) arrays of the leaf float type."""

    def __init__(self, kind, o, g, sl, rays=None):
        self.kind, self.o, self.g, self.sl, self.rays = kind, o, g, sl, rays
        self.tables, self._trace, self._oracle = {}, {}, {}
        self.types = (o[0] if kind == "pair" else o).types
        if kind == "rays":
            self.dev_rays = (cuda(rays[0]), cuda(rays[1]))

    def trace(self, narrow=abi.NARROW_NONE):
        if narrow not in self._trace:
            if self.kind == "self":
                t = chk.trace_self(self.o, self.sl, narrow, tables=self.tables)
            elif self.kind == "pair":
                t = chk.trace_pair(self.o[0], self.o[1], self.sl[0], self.sl[1], narrow, tables=self.tables)
            else:
                t = chk.trace_rays(self.o, self.rays[0], self.rays[1], self.sl, narrow, tables=self.tables)
            self._trace[narrow] = t
        return self._trace[narrow]

    def oracle(self, narrow=abi.NARROW_NONE):
        """(sorted contacts, num_checks) of the oracle's BFS (rays: no narrow on its menu)"""
        if narrow not in self._oracle:
            with np.errstate(all="ignore"):
                if self.kind == "self":
                    e, r = orc.traverse_bfs(self.o, self.sl, narrow)
                elif self.kind == "pair":
                    e, r = orc.traverse_pair_bfs(self.o[0], self.o[1], self.sl[0], self.sl[1], narrow)
                else:
                    e, r = orc.traverse_rays_bfs(self.o, self.rays[0], self.rays[1], self.sl)
            self._oracle[narrow] = (chk.sort_pairs(oracle_pairs(e)), int(r.num_checks))
        return self._oracle[narrow]

    @property
    def total_levels(self):
        return self.o[0].tree.levels + self.o[1].tree.levels if self.kind == "pair" else self.o.tree.levels

    # ---- through the Python driver (api._bfs_run) ----
    def run(self, code=abi.NARROW_NONE):
        """-> (contacts (m, 2) int64, num_checks, decoded counters)"""
        if self.kind == "self":
            t = api._traverse_bfs_single(self.g, self.sl, code, None)
        elif self.kind == "pair":
            t = api._traverse_bfs_pair(self.g[0], self.g[1], self.sl[0], self.sl[1], code, None)
        else:
            t = api._traverse_bfs_rays(self.g, self.dev_rays[0], self.dev_rays[1], self.sl, code, None)
        counters, hint = api._last_bfs_counters
        assert hint == self.total_levels
        assert t.num_contacts == t.contacts.shape[0]
        return contacts_np(t).reshape(-1, 2), int(t.num_checks), chk.decode_counters(counters.cpu().numpy(), hint)

    # ---- through the raw ABI ----
    def raw(self, q, capacity, counters, res, code=abi.NARROW_NONE):
        L = lib.load()
        tail = (q[0].data_ptr(), q[1].data_ptr(), capacity, counters.data_ptr(), C.byref(res), torch.cuda.current_stream().cuda_stream)
        assert min(q[0].shape[0], q[1].shape[0]) >= capacity  # (no queue is smaller than the capacity stated)
        if self.kind == "self":
            self._s = self.g.struct()
            return L.ibvh_traverse_bfs(C.byref(self._s), self.sl, code, *tail)
        if self.kind == "pair":
            self._s = (self.g[0].struct(), self.g[1].struct())
            return L.ibvh_traverse_pair_bfs(C.byref(self._s[0]), C.byref(self._s[1]), self.sl[0], self.sl[1], code, *tail)
        self._s = self.g.struct()
        p, d = self.dev_rays
        return L.ibvh_traverse_rays_bfs(C.byref(self._s), p.data_ptr(), d.data_ptr(), p.shape[0], self.sl, code, *tail)

    def queues(self, capacity):
        return [torch.full((max(capacity, 1), 2), -7, dtype=TORCH_I[self.types.index_type], device="cuda") for _ in range(2)]

    def new_counters(self):
        need = C.c_size_t()
        lib.call("ibvh_bfs_counters_bytes", self.total_levels, C.byref(need))
        return torch.zeros(need.value, dtype=torch.uint8, device="cuda")


def expected_counts(t):
    """the decoded counters of a completed traversal: every step's source count, then the contacts; every step's checks"""
    return [len(s.source) for s in t.steps] + [t.num_contacts], [s.generated for s in t.steps]


def assert_counters(dec, t, ctx):
    flag, source, generated = dec
    src, gen = expected_counts(t)
    assert flag == 0, ctx
    assert source[:len(src)].tolist() == src and not source[len(src):].any(), (ctx, source.tolist(), src)
    assert generated[:len(gen)].tolist() == gen and not generated[len(gen):].any(), (ctx, generated.tolist(), gen)


def assert_run(case, grid, narrow=abi.NARROW_NONE, positions=False):
    """one traversal through the Python driver at one grid: contacts, counts per step, num_checks"""
    lib.set_tuning("bfs_grid", grid)
    t = case.trace(narrow)
    got, checks, dec = case.run(narrow | (abi.OUTPUT_POSITIONS if positions else 0))
    ctx = (case.kind, grid, narrow, positions)
    want = chk.sort_pairs(t.positions if positions else t.contacts)
    assert got.shape == want.shape and (chk.sort_pairs(got) == want).all(), ctx
    assert_counters(dec, t, ctx)
    assert checks == t.num_checks, ctx
    if not positions and (case.kind != "rays" or narrow == abi.NARROW_NONE):
        exp, exp_checks = case.oracle(narrow)
        assert (want == exp).all() and checks == exp_checks, ctx


# ---- preconditions, from the checker's trace alone ----
def forces_mid_loop_flush(t, grid, node_and_leaf=True):
    """Some workgroup of `grid` flushed INSIDE its loop: a step wrote more than grid x STAGE pairs, so one workgroup staged
    more than its area holds and the last flush alone cannot have written them.  node_and_leaf: a node step and the leaf
    step each."""
    out = [s.passed for s in t.steps]
    if node_and_leaf:
        return len(out) >= 2 and max(out[:-1]) > grid * chk.STAGE and out[-1] > grid * chk.STAGE
    return max(out) > grid * chk.STAGE


def forces_many_chunks(t, grid):
    """some workgroup ran four chunks or more in one step (the rotation s_cur <- s_nxt <- s_nn ran with live data)"""
    return max(len(s.source) for s in t.steps) > 3 * grid * chk.TPB


_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ---------------------------------------------------------------------------------------------
# a. one BVH against itself: routes x types
# ---------------------------------------------------------------------------------------------
SELF_N, SELF_SCALE, SELF_SL = 3000, 13.0, 5


def self_case(combo, im, n=SELF_N, scale=SELF_SCALE, sl=SELF_SL, seed=0):
    def make():
        rng = np.random.default_rng(1000 + ALL_COMBOS.index(combo) + seed)
        o, g = build_both(random_volumes(rng, n, combo[0], combo[1], scale=scale), abi.make_types(*combo, *im))
        return Case("self", o, g, sl)
    return memo(("self", combo, im, n, scale, sl, seed), make)


@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
@pytest.mark.parametrize("combo", ALL_COMBOS, ids=_id)
def test_self_every_type_at_small_grids(combo, im):
    case = self_case(combo, im)
    t = case.trace()
    assert forces_mid_loop_flush(t, 3) and forces_many_chunks(t, 3), [(len(s.source), s.passed) for s in t.steps]
    for grid in (1, 2, 3, 0):
        assert_run(case, grid)


@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
def test_self_narrow_menu_and_positions(im):
    case = self_case(ALL_COMBOS[0], im)
    for narrow in PAIR_NARROWS:
        assert forces_mid_loop_flush(case.trace(narrow), 1) and forces_many_chunks(case.trace(narrow), 1)
        assert_run(case, 1, narrow)
        assert_run(case, 0, narrow)
    for grid in (1, 2, 0):
        assert_run(case, grid, positions=True)
    assert_run(case, 1, abi.NARROW_INDEX_LT, positions=True)


# ---------------------------------------------------------------------------------------------
# b. two BVHs: every branch of run_pair's plan
# ---------------------------------------------------------------------------------------------
# (n1, n2, start level 1, start level 2; negative: counted up from the leaf level, -1 = the leaf level)
PAIR_SHAPES = [(1500, 1025, 3, 3), (3000, 700, 2, 2), (700, 3000, 2, 2), (1500, 1025, 5, -1), (1025, 1500, -1, 5),
               (1500, 1025, 4, -2), (1025, 1500, -2, 4)]
ALL_PHASES = {"both descend", "only 1 descends", "only 2 descends", "leaf 2 fixed, 1 descends", "leaf 1 fixed, 2 descends",
              "last joint step", "leaf-leaf"}
PAIR_SCALE = 9.0


def pair_case(combo, im, shape):
    def make():
        n1, n2, sl1, sl2 = shape
        rng = np.random.default_rng(2000 + ALL_COMBOS.index(combo) + n1)
        types = abi.make_types(*combo, *im)
        o1, g1 = build_both(random_volumes(rng, n1, combo[0], combo[1], scale=PAIR_SCALE), types)
        o2, g2 = build_both(random_volumes(rng, n2, combo[0], combo[1], scale=PAIR_SCALE), types)
        sl1 = sl1 if sl1 > 0 else o1.tree.levels + 1 + sl1
        sl2 = sl2 if sl2 > 0 else o2.tree.levels + 1 + sl2
        return Case("pair", (o1, o2), (g1, g2), (sl1, sl2))
    return memo(("pair", combo, im, shape), make)


def _phases(case):
    return chk.pair_phase_names(case.o[0].tree.levels, case.o[1].tree.levels, *case.sl)


def test_pair_shapes_reach_every_branch_of_the_plan():
    """no GPU work: the shapes below, taken together, contain every branch; and trees with virtual right children"""
    seen = set()
    for shape in PAIR_SHAPES:
        seen |= set(_phases(pair_case(ALL_COMBOS[0], INDEX_TYPES[0], shape)))
    assert seen == ALL_PHASES
    for n in (1025, 1500, 700, 3000):
        assert orc.tree_shape(n).virtual_leaves > 0


PAIR_NAMED = {0: {"both descend", "last joint step"}, 1: {"both descend", "only 1 descends", "last joint step"},
              2: {"both descend", "only 2 descends", "last joint step"}, 3: {"leaf 2 fixed, 1 descends"},
              4: {"leaf 1 fixed, 2 descends"}, 5: {"only 1 descends", "last joint step"}, 6: {"only 2 descends", "last joint step"}}


@pytest.mark.parametrize("k", range(len(PAIR_SHAPES)), ids=[_id(s) for s in PAIR_SHAPES])
def test_pair_every_phase_at_small_grids(k):
    case = pair_case(ALL_COMBOS[0], INDEX_TYPES[0], PAIR_SHAPES[k])
    t = case.trace()
    assert PAIR_NAMED[k] | {"leaf-leaf"} <= set(_phases(case)), _phases(case)
    assert forces_mid_loop_flush(t, 2, node_and_leaf=False) and forces_many_chunks(t, 2), [(len(s.source), s.passed) for s in t.steps]
    for grid in (1, 2, 0):
        assert_run(case, grid)


@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
@pytest.mark.parametrize("combo", ALL_COMBOS, ids=_id)
def test_pair_deep_shape_every_type(combo, im):
    case = pair_case(combo, im, PAIR_SHAPES[1])
    t = case.trace()
    assert forces_mid_loop_flush(t, 2) and forces_many_chunks(t, 2), [(len(s.source), s.passed) for s in t.steps]
    for grid in (1, 2, 0):
        assert_run(case, grid)


@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
def test_pair_narrow_menu_and_positions(im):
    case = pair_case(ALL_COMBOS[0], im, PAIR_SHAPES[2])
    for narrow in PAIR_NARROWS:
        assert_run(case, 1, narrow)
    assert_run(case, 1, positions=True)
    assert_run(case, 0, positions=True)
    assert_run(case, 2, abi.NARROW_MORTON_LT, positions=True)


# ---------------------------------------------------------------------------------------------
# c. rays
# ---------------------------------------------------------------------------------------------
RAYS_N, RAYS_NR, RAYS_SCALE = 1500, 900, 5.0


def rays_case(combo, im, n=RAYS_N, nr=RAYS_NR, scale=RAYS_SCALE, sl=1, seed=0):
    def make():
        rng = np.random.default_rng(3000 + ALL_COMBOS.index(combo) + seed)
        vols = random_volumes(rng, n, combo[0], combo[1], scale=scale)
        o, g = build_both(vols, abi.make_types(*combo, *im))
        with np.errstate(all="ignore"):
            p, d = irregular_rays(rng, nr, scale, combo[1])
        # (some origins inside leaves: the ray narrow then removes hits)
        p[::3] = vols[rng.integers(0, n, len(p[::3])), :3] if combo[0] == abi.BSPHERE else \
            0.5 * (vols[rng.integers(0, n, len(p[::3])), :3] + vols[rng.integers(0, n, len(p[::3])), 3:])
        return Case("rays", o, g, sl, rays=(p, d))
    return memo(("rays", combo, im, n, nr, scale, sl, seed), make)


@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
@pytest.mark.parametrize("combo", RAY_COMBOS, ids=_id)
def test_rays_every_type_at_small_grids(combo, im):
    case = rays_case(combo, im)
    t = case.trace()
    assert forces_mid_loop_flush(t, 2) and forces_many_chunks(t, 2), [(len(s.source), s.passed) for s in t.steps]
    for grid in (1, 2, 0):
        assert_run(case, grid)
    tn = case.trace(abi.NARROW_RAY_ORIGIN_OUTSIDE)
    assert 0 < tn.num_contacts < t.num_contacts  # (the narrow removes some hits and keeps some)
    assert_run(case, 1, abi.NARROW_RAY_ORIGIN_OUTSIDE)
    assert_run(case, 1, positions=True)
    assert_run(case, 2, abi.NARROW_RAY_ORIGIN_OUTSIDE, positions=True)


# ---------------------------------------------------------------------------------------------
# d. queue lengths around a chunk
# ---------------------------------------------------------------------------------------------
def test_initial_queue_lengths_around_a_chunk_rays():
    """Rays from start level 1: the initial queue is exactly num_rays pairs.  255 .. 769 rays over 1 .. 5 workgroups: a
    workgroup with no chunk at all, with one ragged chunk, with exactly two chunks, with three."""
    combo, im = ALL_COMBOS[0], INDEX_TYPES[0]
    for nr in (255, 256, 257, 511, 512, 513, 769):
        case = rays_case(combo, im, n=300, nr=nr, scale=3.0, seed=nr)
        t = case.trace()
        assert len(t.steps[0].source) == nr and t.num_contacts > 0
        for grid in (1, 2, 3, 5):
            assert_run(case, grid)
    chunks = lambda nr, grid, wg: len(range(wg, -(-nr // chk.TPB), grid))  # noqa: E731  chunks of workgroup wg
    assert chunks(255, 2, 1) == 0 and chunks(257, 1, 0) == 2 and chunks(512, 1, 0) == 2 and chunks(769, 1, 0) == 4
    assert chunks(513, 1, 0) == 3 and chunks(769, 5, 4) == 0 and chunks(511, 3, 2) == 0


def test_initial_queue_lengths_around_a_chunk_self():
    """a start level whose initial queue ends just below / just above a multiple of the chunk"""
    for n, sl, rem in ((88, 6, 253), (220, 7, 4)):
        case = self_case(ALL_COMBOS[0], INDEX_TYPES[0], n=n, scale=3.0, sl=sl, seed=n)
        assert len(case.trace().steps[0].source) % chk.TPB == rem
        for grid in (1, 2, 3, 5, 0):
            assert_run(case, grid)


def test_grid_knob_is_capped():
    """a grid beyond CUs x 16 is cut to that; the result does not depend on it"""
    case = self_case(ALL_COMBOS[0], INDEX_TYPES[0], n=220, scale=3.0, sl=7, seed=220)
    assert_run(case, 1 << 30)
    assert_run(case, torch.cuda.get_device_properties(0).multi_processor_count * 16)


# ---------------------------------------------------------------------------------------------
# e. steps with nothing to do
# ---------------------------------------------------------------------------------------------
def test_steps_without_a_source():
    types = abi.make_types()
    rng = np.random.default_rng(5)

    def cluster(cx, cy, m=64):
        c = np.array([cx, cy, 0.0]) + 0.5 * rng.random((m, 3))
        return np.concatenate([c, np.full((m, 1), 0.01)], axis=1).astype(np.float32)

    # two clouds whose roots touch and whose children do not: the corners of a square, one diagonal each
    o1, g1 = build_both(np.concatenate([cluster(0, 0), cluster(10, 10)]), types)
    o2, g2 = build_both(np.concatenate([cluster(10, 0), cluster(0, 10)]), types)
    case = Case("pair", (o1, o2), (g1, g2), (1, 1))
    t = case.trace()
    assert [s.generated for s in t.steps[:2]] == [1, 4] and t.steps[0].passed == 1 and t.steps[1].passed == 0
    assert all(len(s.source) == 0 and s.generated == 0 for s in t.steps[2:]) and len(t.steps) > 4
    assert t.num_contacts == 0 and case.oracle()[1] == 5
    for grid in (1, 3, 0):
        assert_run(case, grid)
    # one BVH of far-apart leaves: only the untested (a, a) pairs go down; nothing passes a test
    far = np.concatenate([100.0 * rng.permutation(333)[:, None] + rng.random((333, 3)), np.full((333, 1), 0.01)], axis=1)
    o, g = build_both(far.astype(np.float32), types)
    for sl in (1, 4, o.tree.levels):
        case = Case("self", o, g, sl)
        t = case.trace()
        assert t.num_contacts == 0 and all((s.source[:, 0] == s.source[:, 1]).all() for s in t.steps[2:])
        for grid in (1, 3, 0):
            assert_run(case, grid)
    # rays that miss every node of the start level
    p = np.full((300, 3), -50.0, np.float32)
    d = np.tile(np.array([-1.0, -1.0, -1.0], np.float32), (300, 1))
    case = Case("rays", o, g, 3, rays=(p, d))
    t = case.trace()
    assert t.steps[0].passed == 0 and all(len(s.source) == 0 for s in t.steps[1:])
    assert t.num_checks == chk.level_num_real(o.tree, 3) * 300 > 0
    for grid in (1, 3, 0):
        assert_run(case, grid)


# ---------------------------------------------------------------------------------------------
# f. the overflow protocol through the raw ABI
# ---------------------------------------------------------------------------------------------
def run_with_resumes(case, capacity, grid):
    """The caller's side of the protocol from queues of `capacity` pairs: call; on IBVH_ERR_CAPACITY check every field of
    the result, the kept queue and the counters against the checker, grow both queues to required_capacity keeping that
    queue's prefix, call again with the same result and counters.  -> the steps that overflowed, in order."""
    lib.set_tuning("bfs_grid", grid)
    t = case.trace()
    out = [s.passed for s in t.steps]
    src, gen = expected_counts(t)
    assert src[0] <= capacity  # (the initial queue fits: a resume, not a refusal)
    q, counters, res = case.queues(capacity), case.new_counters(), abi.BfsResult()
    overflowed, start = [], 0
    while True:
        st = case.raw(q, capacity, counters, res)
        dec = chk.decode_counters(counters.cpu().numpy(), case.total_levels)
        if st != abi.ERR_CAPACITY:
            break
        s = next(k for k in range(start, len(out)) if out[k] > capacity)  # the first step from `start` on that does not fit
        need, ctx = out[s], (case.kind, grid, capacity, s)
        assert (res.resume_step, res.resume_num, res.contacts_in) == (s, src[s], 1 if s % 2 == 0 else 2), ctx
        assert res.required_capacity == need + need // 4 + 1024, ctx
        assert (res.num_contacts, res.num_checks) == (0, 0), ctx
        kept = q[res.contacts_in - 1][:res.resume_num].cpu().numpy().astype(np.int64)
        assert (chk.sort_pairs(kept) == t.steps[s].source).all(), ctx  # the overflowing step left its source intact
        flag, source, generated = dec
        assert flag == s + 1, ctx
        # the step kept counting past the capacity: its exact output; every later step returned at once
        assert source[:s + 2].tolist() == src[:s + 2] and not source[s + 2:].any(), (ctx, source.tolist())
        assert generated[:s + 1].tolist() == gen[:s + 1] and not generated[s + 1:].any(), (ctx, generated.tolist())
        overflowed.append(s)
        start, capacity = s, int(res.required_capacity)
        grown = case.queues(capacity)
        grown[res.contacts_in - 1][:res.resume_num].copy_(q[res.contacts_in - 1][:res.resume_num])
        q = grown
    assert st == abi.OK, st
    ctx = (case.kind, grid, overflowed)
    got = q[res.contacts_in - 1][:res.num_contacts].cpu().numpy().astype(np.int64)
    exp, exp_checks = case.oracle()
    assert res.num_contacts == len(exp) and (chk.sort_pairs(got) == exp).all(), ctx
    assert res.num_checks == exp_checks == t.num_checks, ctx
    assert (res.required_capacity, res.resume_step, res.resume_num) == (0, 0, 0), ctx
    assert_counters(dec, t, ctx)  # the earlier steps' counts survived every resume; no step was counted twice
    return overflowed


def overflow_case(kind, im):
    combo = ALL_COMBOS[0]
    if kind == "self":
        return self_case(combo, im, n=2000, scale=11.0, sl=4, seed=7)
    if kind == "pair":
        return pair_case(combo, im, PAIR_SHAPES[1])
    return rays_case(combo, im, n=1500, nr=600, scale=5.0, seed=7)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
@pytest.mark.parametrize("kind", ["self", "pair", "rays"])
def test_capacity_exactly_enough_and_one_short(kind, im, grid):
    case = overflow_case(kind, im)
    t = case.trace()
    out = [s.passed for s in t.steps]
    s = int(np.argmax(out))  # the step with the largest output
    need = out[s]
    assert t.steps[0].generated < need and all(o < need for o in out[:s])  # the initial and every earlier queue fit in need - 1
    assert need > grid * chk.STAGE  # (some workgroup of the overflowing step flushes more than once)
    assert run_with_resumes(case, need, grid) == []
    assert run_with_resumes(case, need - 1, grid) == [s]


@pytest.mark.parametrize("im", INDEX_TYPES, ids=_id)
def test_a_node_step_overflows_and_the_leaf_step_again(im):
    case = rays_case(ALL_COMBOS[1], im)  # sphere leaves under sphere nodes: the hit list is the longest queue
    t = case.trace()
    out = [s.passed for s in t.steps]
    last = len(out) - 1

    def plan(capacity):  # the steps that overflow from queues of `capacity` pairs, by the protocol's growth rule
        steps = []
        for k, o in enumerate(out):
            if o > capacity:
                steps, capacity = steps + [k], o + o // 4 + 1024
        return steps

    # an early node step that overflows first, such that the leaf step overflows again at the end
    s1 = next(k for k in range(1, last - 2) if max(t.steps[0].generated, *out[:k]) < out[k] and plan(out[k] - 1)[-1] == last)
    want = plan(out[s1] - 1)
    assert want[0] == s1 and want[-1] == last and len(want) >= 2
    assert run_with_resumes(case, out[s1] - 1, 1) == want


@pytest.mark.parametrize("combo", ALL_COMBOS, ids=_id)
def test_python_driver_with_queues_that_never_have_room(combo, monkeypatch):
    """BFS_INITIAL_FACTOR = BFS_GROWTH = 1: the driver's queues start at the initial pair count and grow only to what the
    library asks for, so that nearly every step overflows once and is resumed — same lists, same counts per step."""
    monkeypatch.setattr(api, "BFS_INITIAL_FACTOR", 1)
    monkeypatch.setattr(api, "BFS_GROWTH", 1)
    case = self_case(combo, INDEX_TYPES[0], n=1200, scale=9.0, sl=3, seed=11)
    out = [s.passed for s in case.trace().steps]
    cap, resumes = case.trace().steps[0].generated, 0
    for o in out:  # the driver's capacities, from the trace
        if o > cap:
            cap, resumes = o + o // 4 + 1024, resumes + 1
    assert resumes >= 2, out
    assert_run(case, 1)
    if combo[1] == combo[3]:
        case = rays_case(combo, INDEX_TYPES[0], n=700, nr=300, scale=4.0, seed=11)
        assert_run(case, 1)
    if ALL_COMBOS.index(combo) < 3:
        case = pair_case(combo, INDEX_TYPES[0], PAIR_SHAPES[1])
        assert_run(case, 1)
