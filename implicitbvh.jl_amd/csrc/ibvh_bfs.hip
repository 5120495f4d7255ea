// ibvh_bfs.hip — breadth-first traversal (BFSTraversal) on gfx950: level-synchronous expansion of a
// bounding-volume-test-tree held in two ping-pong pair queues; the "dynamic contact-pair work queue".
//
// Replaces src/traverse/breadth_first/traverse_single{,_gpu}.jl, traverse_pair{,_gpu}.jl and
// src/raytrace/breadth_first/{breadth_first,raytrace_gpu}.jl.
//
// The reference's KernelAbstractions kernels do one LDS atomic per thread to reserve slots in a
// workgroup staging buffer and one global atomic per workgroup (bfs/traverse_single_gpu.jl:65-99).
// Here slot reservation inside a wave is atomic-free: every lane produces 0..4 pairs, the count is
// split into bit planes and wave64 ballots + popcounts give each lane its exclusive offset; waves
// combine through LDS, the workgroup takes ONE global atomic on the level's queue tail, stages its
// pairs in LDS and writes them out as one contiguous, coalesced run.  Output order across workgroups
// is arbitrary — as in the reference's GPU path, whose tests compare after sorting
// (test/gputests.jl:71-78).  One kernel template serves all ten reference kernels through a policy.
#include <type_traits>

#include "ibvh_common.hpp"

namespace ibvh {
namespace bfs {

constexpr int TPB = 256;
constexpr int GEN_SLOTS = 16; // words per step the workgroups spread their check counts over (level_kernel)

// Workgroup barrier that orders LDS accesses only: __syncthreads() also drains every outstanding global store and
// load (s_waitcnt vmcnt(0)), which would make a workgroup wait for its queue writes before it may read its next chunk.
IBVH_D void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class L, class N> struct TreeRef {
    const char *leaves;
    LeafLayout lay;
    const N *nodes;
    int64_t levels, virtual_leaves;
    int64_t level;      // level of this tree's entries in the source queue
    int64_t skips;      // level_skips(level)
    int64_t leaf_first; // 2^(levels-1)
    int64_t child_real; // real nodes on level+1
    IBVH_D N node(int64_t implicit) const { return load_vol<N>(nodes + (implicit - skips - 1)); }
    IBVH_D const char *leaf_rec(int64_t implicit) const { return leaves + (implicit - leaf_first) * lay.stride; }
    // unsafe_isvirtual(tree, 2*implicit + 1): is the right child virtual?
    IBVH_D bool right_child_virtual(int64_t implicit) const {
        int64_t c = 2 * implicit + 1;
        return c - (int64_t(1) << level) >= child_real;
    }
};

template <class L, class N> TreeRef<L, N> make_ref(const ibvh_bvh &b, const LeafLayout &lay, int64_t level) {
    TreeRef<L, N> r;
    r.leaves = (const char *)b.leaves;
    r.lay = lay;
    r.nodes = (const N *)b.nodes;
    r.levels = b.tree.levels;
    r.virtual_leaves = b.tree.virtual_leaves;
    r.level = level;
    r.skips = level_skips(r.levels, r.virtual_leaves, level);
    r.leaf_first = int64_t(1) << (r.levels - 1);
    r.child_real = level < r.levels ? level_num_real(r.levels, r.virtual_leaves, level + 1) : 0;
    return r;
}

// `narrow` arguments carry the menu code and the IBVH_OUTPUT_POSITIONS flag (include/ibvh.h)
inline bool narrow_arg_ok(int32_t narrow, bool rays) {
    if (narrow & ~(IBVH_NARROW_MASK | IBVH_OUTPUT_POSITIONS)) return false;
    const int code = narrow & IBVH_NARROW_MASK;
    return rays ? (code == IBVH_NARROW_NONE || code == IBVH_NARROW_RAY_ORIGIN_OUTSIDE)
                : (code == IBVH_NARROW_NONE || code == IBVH_NARROW_MORTON_LT || code == IBVH_NARROW_INDEX_LT);
}

// ------------------------------------------------------------------------------------------
// policies.  The reference's kernels CHECK a pair of the level's queue and, if it passes, append its child pairs for
// the next level to check (bfs/traverse_single_gpu.jl:30-120): every generated pair is written to the queue, read
// back one launch later and costs two unrelated volume fetches there.  Here a step is shifted by half a level: the
// queues hold pairs that have already PASSED their check; a step enumerates the children of such a pair (no memory
// access) and checks them at once — the four children of (a, b) need the volumes 2a, 2a+1, 2b, 2b+1: two adjacent
// pairs, fetched once — and only the passing ones reach the queue (about a third).  The same pairs are checked as in
// the reference, one launch earlier: num_checks (every generated pair, bfs/traverse_single.jl:25,48) and the
// contact set are unchanged; queue traffic and volume fetches drop by 3 - 4 x.
// A policy is one level of one traversal, with the same members in all three:
//   safe()                               a pair of its level that is always real, for lanes beyond the queue's end
//   load(s), test(s, x, res)             the operands of the pair s of its level, and the check itself: does s
//                                        pass?  `res`: what goes into the queue — s, or the contact at leaf level
//   load_sides(s, parent),               the volumes of all children of the PARENT-level pair s, and the check of the
//   test_sides(c, x, res, parent)        child c among them
//   children(s, out)                     the next level's pairs of a passing pair s
// ------------------------------------------------------------------------------------------
// Register storage for a node volume OR a leaf volume, whichever the launch's (uniform) level flag says: what a lane
// prefetches for a child stays as small as the larger of the two instead of holding both.
template <class A, class B> struct Either {
    static constexpr int W = (int)((sizeof(A) > sizeof(B) ? sizeof(A) : sizeof(B)) / 4);
    uint32_t w[W];
    template <class X> IBVH_D void set(const X &x) { __builtin_memcpy(w, &x, sizeof(X)); }
    template <class X> IBVH_D X get() const {
        X x;
        __builtin_memcpy(&x, w, sizeof(X));
        return x;
    }
};

// A volume at a tree position is an Either plus (leaf levels only) the leaf's user index.  What a check needs from memory
// is fetched UNCONDITIONALLY (`implicit` is always a valid position of its level: the kernel hands over a real child or
// safe()): every lane's loads for all its <= 4 children are in flight before the first test — four dependent round
// trips per lane otherwise, and the kernel is bound by exactly that latency.
// The two parts are filled in place, where the caller keeps them: a value returned and copied into its slot, or another
// arrangement of the slots, costs the widest volume types VGPRs and occupancy.
// (`is_leaf` is uniform over the launch; `with_index` = false where no check of the step reads the index)
template <class L, class N, class I>
IBVH_D void fetch(Either<N, L> &v, I &idx, const TreeRef<L, N> &t, bool is_leaf, int64_t implicit, bool with_index = true) {
    if (is_leaf) {
        const char *r = t.leaf_rec(implicit);
        v.set(load_vol<L>(r));
        if (with_index) idx = load_index<I>(r, t.lay);
    } else {
        v.set(t.node(implicit));
    }
}
// The two children of the source position `p`, [0] the left and [1] the right one (`t` is at the CHILDREN's level).  A
// virtual right child re-reads the left one (never selected); so does a side that did not descend in the parent step
// (PairStep's one-sided phases): it holds its one position twice.
template <class L, class N, class I>
IBVH_D void fetch_children(Either<N, L> (&v)[2], I (&idx)[2], const TreeRef<L, N> &t, bool is_leaf, int64_t p, bool descended) {
    const int64_t first = int64_t(1) << (t.level - 1), nreal = level_num_real(t.levels, t.virtual_leaves, t.level);
    const int64_t c0 = descended ? 2 * p : p;
    const int64_t c1 = (descended && (c0 + 1 - first) < nreal) ? c0 + 1 : c0;
#pragma unroll
    for (int k = 0; k < 2; ++k) fetch(v[k], idx[k], t, is_leaf, k ? c1 : c0);
}
// ... and which of the two the child position `c` is
template <class I> IBVH_D int child_slot(I c, bool descended) { return descended ? (int)(c & 1) : 0; }

// What a lane fetches for a pair of volumes (self and pair traversals).  Loaded: the two operands of one check.  Sides:
// the children of a source pair (a, b) are combinations of {2a, 2a+1} x {2b, 2b+1}, so FOUR volumes (two adjacent pairs
// in memory) serve all of them — fetched once per source pair instead of twice per child pair.
template <class L, class N, class I> struct Loaded {
    Either<N, L> a, b;
    I ia, ib;
};
template <class L, class N, class I> struct Sides {
    Either<N, L> v[2][2]; // [side a / b][left / right child]
    I idx[2][2];
    // the operands of the child pair c (`da` / `db`: did that side descend in the parent step?)
    IBVH_D Loaded<L, N, I> select(IndexPair<I> c, bool da, bool db) const {
        const int ka = child_slot(c.a, da), kb = child_slot(c.b, db);
        Loaded<L, N, I> y;
        y.a = ka ? v[0][1] : v[0][0];
        y.b = kb ? v[1][1] : v[1][0];
        y.ia = ka ? idx[0][1] : idx[0][0];
        y.ib = kb ? idx[1][1] : idx[1][0];
        return y;
    }
};

// The next level's pairs of a passing pair when ONE side descends (`side` 0: a, 1: b): the left child, plus the right
// unless it is virtual ...
template <class I> IBVH_D int descend_one(IndexPair<I> s, int side, bool right_virtual, IndexPair<I> *out) {
    const I a = s.a, b = s.b;
    out[0] = side ? IndexPair<I>{a, I(2 * b)} : IndexPair<I>{I(2 * a), b};
    if (right_virtual) return 1;
    out[1] = side ? IndexPair<I>{a, I(2 * b + 1)} : IndexPair<I>{I(2 * a + 1), b};
    return 2;
}
// ... and when BOTH do: 1, 2 or 4 pairs, by which side's right child is virtual
template <class I> IBVH_D int descend_both(IndexPair<I> s, bool virtual_a, bool virtual_b, IndexPair<I> *out) {
    const I a = s.a, b = s.b;
    out[0] = {I(2 * a), I(2 * b)};
    if (virtual_a) {
        if (virtual_b) return 1;
        out[1] = {I(2 * a), I(2 * b + 1)};
        return 2;
    }
    if (virtual_b) {
        out[1] = {I(2 * a + 1), I(2 * b)};
        return 2;
    }
    out[1] = {I(2 * a), I(2 * b + 1)};
    out[2] = {I(2 * a + 1), I(2 * b)};
    out[3] = {I(2 * a + 1), I(2 * b + 1)};
    return 4;
}

template <class I> struct Identity { // the initial queue: "children" of nothing, still to be checked
    static constexpr int MAXOUT = 1;
    static constexpr bool kIdentity = true;
    IBVH_D int children(IndexPair<I> s, IndexPair<I> *out) const {
        out[0] = s;
        return 1;
    }
};

// _traverse_nodes_gpu! — bfs/traverse_single_gpu.jl:30-120 (same rules as traverse_single_cpu.jl:64-133) — and
// _traverse_leaves_gpu! — :153-211
template <class L, class N, class I> struct SelfStep {
    static constexpr int MAXOUT = 4;
    static constexpr bool kIdentity = false;
    using Loaded = bfs::Loaded<L, N, I>;
    using Sides = bfs::Sides<L, N, I>;
    TreeRef<L, N> t;
    int leaf;        // entries are leaf pairs
    int self_checks; // (nodes) :44
    int narrow;      // (leaves) menu code
    int positions;   // (leaves) IBVH_OUTPUT_POSITIONS: 1-based leaf positions instead of user indices, left leaf first
    IBVH_D IndexPair<I> safe() const { const I f = I(int64_t(1) << (t.level - 1)); return {f, f}; } // the level's first node: always real
    IBVH_D Loaded load(IndexPair<I> s) const {
        Loaded x{};
        fetch(x.a, x.ia, t, leaf, s.a);
        fetch(x.b, x.ib, t, leaf, s.b);
        return x;
    }
    IBVH_D bool test(IndexPair<I> s, const Loaded &x, IndexPair<I> &res) const {
        if (leaf) {
            if (!iscontact(x.a.template get<L>(), x.b.template get<L>())) return false;
            if (narrow != IBVH_NARROW_NONE) { // (the Morton codes are fetched only here: the menu predicates are the rare case)
                const uint64_t m1 = narrow == IBVH_NARROW_MORTON_LT ? load_morton(t.leaf_rec(s.a), t.lay) : 0;
                const uint64_t m2 = narrow == IBVH_NARROW_MORTON_LT ? load_morton(t.leaf_rec(s.b), t.lay) : 0;
                if (!narrow_eval(narrow, m1, x.ia, m2, x.ib)) return false;
            }
            if (positions) res = {I(s.a - t.leaf_first + 1), I(s.b - t.leaf_first + 1)}; // (a is left of b)
            else res = x.ia > x.ib ? IndexPair<I>{x.ib, x.ia} : IndexPair<I>{x.ia, x.ib};
            return true;
        }
        res = s;
        return s.a == s.b || iscontact(x.a.template get<N>(), x.b.template get<N>()); // (a node against itself is not tested, :52-70)
    }
    // (called on the CHILD level's policy with the parent-level source pair)
    IBVH_D Sides load_sides(IndexPair<I> s, const SelfStep &) const {
        Sides x{};
#pragma unroll
        for (int side = 0; side < 2; ++side) fetch_children(x.v[side], x.idx[side], t, leaf, side ? s.b : s.a, true);
        return x;
    }
    IBVH_D bool test_sides(IndexPair<I> c, const Sides &x, IndexPair<I> &res, const SelfStep &) const {
        return test(c, x.select(c, true, true), res);
    }
    IBVH_D int children(IndexPair<I> s, IndexPair<I> *out) const {
        const I a = s.a;
        if (a == s.b) {
            if (t.right_child_virtual(a)) {
                if (!self_checks) return 0;
                out[0] = {I(2 * a), I(2 * a)};
                return 1;
            }
            if (self_checks) {
                out[0] = {I(2 * a), I(2 * a)};
                out[1] = {I(2 * a), I(2 * a + 1)};
                out[2] = {I(2 * a + 1), I(2 * a + 1)};
                return 3;
            }
            out[0] = {I(2 * a), I(2 * a + 1)};
            return 1;
        }
        // node a is left of node b, so its children are real (traverse_single_cpu.jl:103-105)
        return descend_both(s, false, t.right_child_virtual(s.b), out);
    }
};

// The six pair kernels of bfs/traverse_pair_gpu.jl:34-609 in one policy: which side is at leaf level
// (leaf1 / leaf2) and which side descends (d1 / d2).
template <class L, class N, class I> struct PairStep {
    static constexpr int MAXOUT = 4;
    static constexpr bool kIdentity = false;
    using Loaded = bfs::Loaded<L, N, I>;
    using Sides = bfs::Sides<L, N, I>;
    TreeRef<L, N> t1, t2;
    int narrow, positions;
    int leaf1, leaf2, d1, d2;
    IBVH_D IndexPair<I> safe() const { return {I(int64_t(1) << (t1.level - 1)), I(int64_t(1) << (t2.level - 1))}; }
    IBVH_D Loaded load(IndexPair<I> s) const {
        Loaded x{};
        fetch(x.a, x.ia, t1, leaf1, s.a, leaf2); // (only a leaf-leaf check reads the indices)
        fetch(x.b, x.ib, t2, leaf2, s.b, leaf1);
        return x;
    }
    IBVH_D bool test(IndexPair<I> s, const Loaded &x, IndexPair<I> &res) const {
        res = s;
        if (leaf1 && leaf2) {
            // _traverse_leaves_pair_gpu! (:556-609): (leaf1.index, leaf2.index), not re-ordered
            if (!iscontact(x.a.template get<L>(), x.b.template get<L>())) return false;
            if (narrow != IBVH_NARROW_NONE) {
                const uint64_t m1 = narrow == IBVH_NARROW_MORTON_LT ? load_morton(t1.leaf_rec(s.a), t1.lay) : 0;
                const uint64_t m2 = narrow == IBVH_NARROW_MORTON_LT ? load_morton(t2.leaf_rec(s.b), t2.lay) : 0;
                if (!narrow_eval(narrow, m1, x.ia, m2, x.ib)) return false;
            }
            res = positions ? IndexPair<I>{I(s.a - t1.leaf_first + 1), I(s.b - t2.leaf_first + 1)} : IndexPair<I>{x.ia, x.ib};
            return true;
        }
        if (leaf1) return iscontact(x.a.template get<L>(), x.b.template get<N>()); // iscontact(leaf1.volume, node2), :461-527
        if (leaf2) return iscontact(x.a.template get<N>(), x.b.template get<L>()); // :360-426
        return iscontact(x.a.template get<N>(), x.b.template get<N>());
    }
    IBVH_D Sides load_sides(IndexPair<I> s, const PairStep &parent) const {
        Sides x{};
#pragma unroll
        for (int side = 0; side < 2; ++side)
            fetch_children(x.v[side], x.idx[side], side ? t2 : t1, side ? leaf2 : leaf1, side ? s.b : s.a, side ? parent.d2 : parent.d1);
        return x;
    }
    IBVH_D bool test_sides(IndexPair<I> c, const Sides &x, IndexPair<I> &res, const PairStep &parent) const {
        return test(c, x.select(c, parent.d1, parent.d2), res);
    }
    IBVH_D int children(IndexPair<I> s, IndexPair<I> *out) const {
        // _traverse_nodes_pair_gpu! (:34-119)
        if (d1 && d2) return descend_both(s, t1.right_child_virtual(s.a), t2.right_child_virtual(s.b), out);
        if (d1) return descend_one(s, 0, t1.right_child_virtual(s.a), out); // _left_ kernels (:155-222, :360-426)
        return descend_one(s, 1, t2.right_child_virtual(s.b), out);         // _right_ kernels (:258-325, :461-527)
    }
};

template <class T> struct Ray {
    T p[3], d[3];
};
// ray `iray` (1-based) of the 3 x num_rays arrays
template <class T> IBVH_D Ray<T> load_ray(const T *points, const T *dirs, int64_t iray) {
    Ray<T> r;
    const int64_t r0 = 3 * (iray - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.p[k] = points[r0 + k];
        r.d[k] = dirs[r0 + k];
    }
    return r;
}

// _traverse_rays_nodes_gpu! / _traverse_rays_leaves_gpu! — raytrace/breadth_first/raytrace_gpu.jl:26-179
template <class L, class N, class I> struct RayStep {
    static constexpr int MAXOUT = 2;
    static constexpr bool kIdentity = false;
    using T = typename L::elt;
    TreeRef<L, N> t;
    const T *points, *dirs;
    int leaf;
    int narrow, positions;
    struct Loaded { // the ray and one volume
        Ray<T> ray;
        Either<N, L> v;
        I idx;
    };
    struct Sides { // the ray once + the two children of its node
        Ray<T> ray;
        Either<N, L> v[2];
        I idx[2];
    };
    IBVH_D IndexPair<I> safe() const { return {I(int64_t(1) << (t.level - 1)), I(1)}; } // (num_rays >= 1 whenever a level runs)
    IBVH_D Loaded load(IndexPair<I> s) const {
        Loaded x{};
        x.ray = load_ray(points, dirs, (int64_t)s.b);
        fetch(x.v, x.idx, t, leaf, s.a);
        return x;
    }
    IBVH_D bool test(IndexPair<I> s, const Loaded &x, IndexPair<I> &res) const {
        res = s;
        if (leaf) {
            const L lv = x.v.template get<L>();
            if (!isintersection(lv, x.ray.p, x.ray.d)) return false;
            if (narrow == IBVH_NARROW_RAY_ORIGIN_OUTSIDE && !origin_outside(lv, x.ray.p)) return false; // raytrace_gpu.jl:159
            res = {positions ? I(s.a - t.leaf_first + 1) : x.idx, s.b};
            return true;
        }
        return isintersection(x.v.template get<N>(), x.ray.p, x.ray.d);
    }
    IBVH_D Sides load_sides(IndexPair<I> s, const RayStep &) const {
        Sides x{};
        x.ray = load_ray(points, dirs, (int64_t)s.b);
        fetch_children(x.v, x.idx, t, leaf, s.a, true);
        return x;
    }
    IBVH_D bool test_sides(IndexPair<I> c, const Sides &x, IndexPair<I> &res, const RayStep &) const {
        const int k = child_slot(c.a, true);
        Loaded y;
        y.ray = x.ray;
        y.v = k ? x.v[1] : x.v[0];
        y.idx = k ? x.idx[1] : x.idx[0];
        return test(c, y, res);
    }
    IBVH_D int children(IndexPair<I> s, IndexPair<I> *out) const { return descend_one(s, 0, t.right_child_virtual(s.a), out); }
};

// What a step reads for a source pair, told apart by the parent policy.  Step 0 (Identity) tests the source pair
// itself: it is of pb's level and brings its own operands.  Every later step tests the children of a source pair of
// pa's level, which share their volumes; there pa and pb are two levels of ONE policy type (the second overload set
// takes no other pairing; level_kernel asserts it).  The test itself is told apart in level_kernel: written as a
// one-child case of the loop over the children, step 0 cost its kernels registers and, for some types, occupancy.
template <class I, class PolB> IBVH_D IndexPair<I> source_safe(const Identity<I> &, const PolB &pb) { return pb.safe(); }
template <class I, class PolB> IBVH_D auto source_fetch(const Identity<I> &, const PolB &pb, IndexPair<I> s) { return pb.load(s); }
template <class Pol> IBVH_D auto source_safe(const Pol &pa, const Pol &) { return pa.safe(); }
template <class Pol, class I> IBVH_D auto source_fetch(const Pol &pa, const Pol &pb, IndexPair<I> s) { return pb.load_sides(s, pa); }

// ------------------------------------------------------------------------------------------
// the level kernel: children of the source pairs, checked at once; wave64 ballot compaction of the passing ones +
// one global atomic per workgroup
// ------------------------------------------------------------------------------------------
// counters[0]          overflow flag: 0, or 1 + the index of the first step whose destination queue was too small
// counters[1 + s]      entries in the SOURCE queue of step s (counters[1] = the initial queue; step s produces
//                      counters[2 + s], counting on past `capacity` so that the exact need is known)
// counters[chk * (1 + k) + s]   pairs step s generated and checked, slot k < GEN_SLOTS (num_checks is their sum; chk =
//                      total_levels + 8 = the length of one block).  Same-address global atomics are serialised at
//                      ~11 ns each on this part (measured: a level's time was 11 ns x (workgroups + waves) whatever
//                      its size — 108 us for 0.5 M source pairs, 140 us for 5.2 M), so a workgroup adds its count
//                      ONCE, to the slot blockIdx % GEN_SLOTS (different cache lines), not once per wave to one word
// No host read between the levels: a step takes its source count from the device word the previous step
// accumulated, so the grid is a fixed number of workgroups that stride over the source queue; once a step has
// overflowed, the later steps (already enqueued) return at once and the caller resumes from that step with larger
// queues (the source queue of the overflowed step is intact).
template <class I, class PolA, class PolB>
__global__ __launch_bounds__(TPB) void level_kernel(const IndexPair<I> *__restrict__ src, IndexPair<I> *__restrict__ dst,
                                                    int64_t capacity, unsigned long long *__restrict__ counters, int step, int chk,
                                                    PolA pa, PolB pb) {
    constexpr int MAXOUT = PolA::MAXOUT;
    static_assert(PolA::kIdentity || std::is_same<PolA, PolB>::value, "a step joins two levels of one policy");
    // Results of MANY chunks are collected in LDS and leave in one coalesced run behind ONE global atomic on the level's
    // tail (round 2 took that atomic per chunk: every chunk of a workgroup then waited out a ~2 us round trip to L2 —
    // ~34 chunks a workgroup and level at 1e6 leaves, most of the 1.4 ms of config 2).  A wave reserves its share of the
    // staging area with one LDS atomic (no workgroup barrier for the prefix); one barrier per chunk tells everybody
    // whether the area could overflow with the next chunk and must be flushed first.
    constexpr int STAGE = (sizeof(I) == 4 ? 24 : 48) * 1024 / (int)sizeof(IndexPair<I>); // 3,072 pairs: six workgroups a CU (the registers allow five)
    static_assert(STAGE >= 2 * MAXOUT * TPB, "the staging area holds at least two worst-case chunks");
    __shared__ IndexPair<I> staged[STAGE];
    __shared__ int s_fill;
    __shared__ unsigned long long s_base, s_gen;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        s_fill = 0;
        s_gen = 0ull;
    }
    lds_barrier();
    // an EARLIER step overflowed: its destination (our source) is incomplete.  The step that overflows itself keeps going
    // in every workgroup — also those that start, or reach their next chunk, after a sibling raised the flag — so that
    // counters[2 + step] ends as the exact number of pairs the step produces (required_capacity).
    const unsigned long long flag = counters[0];
    if (flag != 0ull && flag - 1ull < (unsigned long long)step) return;
    const int64_t num_src = (int64_t)counters[1 + step];
    if (num_src > capacity) return;   // (defensive: the flag covers this)
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    unsigned long long generated = 0;
    // staging area -> destination queue: one global atomic for everything collected since the last flush
    auto flush = [&]() {
        const int total = s_fill; // (all waves are behind a barrier: stable)
        if (total > 0) {
            if (threadIdx.x == 0) s_base = atomicAdd(&counters[2 + step], (unsigned long long)total);
            lds_barrier();
            const unsigned long long base = s_base;
            if (base + (unsigned long long)total > (unsigned long long)capacity) {
                if (threadIdx.x == 0) atomicMax(&counters[0], (unsigned long long)(1 + step)); // the tail keeps counting
            } else {
                for (int p = threadIdx.x; p < total; p += TPB) dst[base + p] = staged[p];
            }
        }
        lds_barrier();
        if (threadIdx.x == 0) s_fill = 0;
        lds_barrier(); // staged / s_fill / s_base are reused (LDS only: the stores above stay in flight)
    };
    // Software pipeline over the workgroup's chunks (round 3): the source pair of chunk c + 2 and the volumes of chunk
    // c + 1 are in flight while chunk c is tested, staged and flushed.  A chunk used to be three DEPENDENT round trips
    // (source pair -> volumes -> tail atomic of a flush), with nothing else for the workgroup's waves to do meanwhile: the
    // level kernels were ~82 % waiting.  Lanes beyond the queue's end carry safe() (a valid pair of the level), so every
    // load is unconditional; vmcnt counts in order, so the wait for chunk c + 1's volumes sits at the register rotation at
    // the end of the body, a whole test-and-stage phase after they were requested.
    const int64_t stride = (int64_t)gridDim.x;
    auto source_of = [&](int64_t chunk) -> IndexPair<I> {
        const int64_t i = chunk * TPB + threadIdx.x;
        return i < num_src ? src[i] : source_safe(pa, pb);
    };
    auto fetch = [&](IndexPair<I> sp) { return source_fetch(pa, pb, sp); };
    using Fetched = decltype(fetch(IndexPair<I>{}));
    IndexPair<I> s_cur = source_of((int64_t)blockIdx.x), s_nxt = source_of((int64_t)blockIdx.x + stride);
    Fetched f_cur = fetch(s_cur);
    for (int64_t chunk = blockIdx.x; chunk * TPB < num_src; chunk += stride) {
        const int64_t i = chunk * TPB + threadIdx.x;
        const Fetched f_nxt = fetch(s_nxt);
        const IndexPair<I> s_nn = source_of(chunk + 2 * stride);
        // (results stay in registers, statically indexed: `out[k++]` would put the array into scratch memory)
        IndexPair<I> kids[MAXOUT], res[MAXOUT];
        uint32_t okm = 0; // bit j: child j passed
        int nk = 0;
        if (i < num_src) nk = pa.children(s_cur, kids);
        generated += (unsigned long long)nk;
        // the source pair's children share their volumes: {2a, 2a+1} x {2b, 2b+1} (or one side kept): four volume
        // fetches per lane serve up to four checks
        if constexpr (PolA::kIdentity) { // step 0: the source pair itself is tested
            if (nk > 0 && pb.test(s_cur, f_cur, res[0])) okm = 1u;
        } else {
#pragma unroll
            for (int j = 0; j < MAXOUT; ++j) {
                const bool ok = j < nk && pb.test_sides(kids[j], f_cur, res[j], pa);
                okm |= ok ? (1u << j) : 0u;
            }
        }
        const int k = __popc(okm);

        // exclusive offset inside the wave from ballots over the bit planes of k (k <= 4)
        uint64_t b0 = __ballot(k & 1), b1 = __ballot(k & 2), b2 = __ballot(k & 4);
        int wave_prefix = __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
        int wave_sum = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
        int wave_base = 0;
        if (lane == 0 && wave_sum > 0) wave_base = atomicAdd(&s_fill, wave_sum); // (LDS atomic: the wave's share of the staging area)
        wave_base = __builtin_amdgcn_readfirstlane(wave_base);
        const int at = wave_base + wave_prefix;
#pragma unroll
        for (int j = 0; j < MAXOUT; ++j)
            if ((okm >> j) & 1u) staged[at + __popc(okm & ((1u << j) - 1u))] = res[j];
        lds_barrier(); // every wave's share is reserved and written
        if (s_fill > STAGE - MAXOUT * TPB) flush(); // (uniform: read after the barrier) the next chunk might not fit
        s_cur = s_nxt;
        f_cur = f_nxt;
        s_nxt = s_nn;
    }
    flush();
    // pairs checked by this workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) generated += __shfl_xor(generated, o, 64);
    if (lane == 0 && generated != 0ull) atomicAdd(&s_gen, generated); // (LDS)
    lds_barrier();
    if (threadIdx.x == 0 && s_gen != 0ull) atomicAdd(&counters[chk * (1 + (int)(blockIdx.x % GEN_SLOTS)) + step], s_gen);
}

// ------------------------------------------------------------------------------------------
// initial queues — fill_initial_bvtt_* (bfs/traverse_single.jl:102-167, traverse_pair.jl:195-219,
// raytrace/breadth_first/breadth_first.jl:116-137), in the CPU branch's order
// ------------------------------------------------------------------------------------------
// rows i = 0..n-1; row i holds (n - i) entries when the self pair is included, (n - 1 - i) otherwise
IBVH_D int64_t tri_before(int64_t i, int64_t n, bool with_self) {
    return with_self ? i * n - i * (i - 1) / 2 : i * (2 * n - i - 1) / 2;
}
template <class I>
__global__ __launch_bounds__(TPB) void fill_self_kernel(IndexPair<I> *q, int64_t n, int64_t first, int with_self, int64_t total) {
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= total) return;
    // exact unranking: double-precision guess of the row, then integer correction
    const double t = with_self ? 2.0 * (double)n + 1.0 : 2.0 * (double)n - 1.0;
    double disc = t * t - 8.0 * (double)k;
    int64_t i = (int64_t)((t - sqrt(disc < 0.0 ? 0.0 : disc)) * 0.5);
    const int64_t imax = with_self ? n - 1 : n - 2;
    i = i < 0 ? 0 : (i > imax ? imax : i);
    while (i > 0 && tri_before(i, n, with_self) > k) --i;
    while (i < imax && tri_before(i + 1, n, with_self) <= k) ++i;
    const int64_t off = k - tri_before(i, n, with_self);
    const int64_t j = with_self ? i + off : i + 1 + off;
    q[k] = {I(first + i), I(first + j)};
}
template <class I>
__global__ __launch_bounds__(TPB) void fill_product_kernel(IndexPair<I> *q, int64_t rows, int64_t cols, int64_t first_row,
                                                          int64_t first_col) {
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= rows * cols) return;
    q[k] = {I(first_row + k / cols), I(first_col + k % cols)};
}

// ------------------------------------------------------------------------------------------
// host drivers
// ------------------------------------------------------------------------------------------
// A traversal is a fixed sequence of steps (one level kernel each).  All steps are enqueued back to back; ONE host
// read at the end fetches the overflow flag and every step's count.
struct Run {
    hipStream_t st;
    unsigned long long *counters;
    int64_t capacity;
    int64_t total_levels;
    int chk = 0;           // index of the first per-step check counter
    int step = 0;          // index of the next step
    int first = 0;         // steps below `first` were completed by an earlier call (resume): they are not launched
    bool swapped = false;  // false: step `step` reads q[0]
    void *q[2];
    void *src() const { return q[swapped ? 1 : 0]; }
    void *dst() const { return q[swapped ? 0 : 1]; }
};

inline int level_grid() {
    static const int cus = [] {
        int dev = 0, c = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
        return c;
    }();
    // (default 4 a CU: one resident round at the self / pair kernels' occupancy; every workgroup costs a serialised tail
    // atomic per flush)
    const int per = g_tuning.bfs_wg_per_cu < 1 ? 1 : (g_tuning.bfs_wg_per_cu > 16 ? 16 : g_tuning.bfs_wg_per_cu);
    // (development knob bfs_grid: exactly that many workgroups, so that a small tree gives one workgroup many chunks)
    if (g_tuning.bfs_grid > 0) return g_tuning.bfs_grid < cus * 16 ? g_tuning.bfs_grid : cus * 16;
    return cus * per;
}

template <class I, class PolA, class PolB> int step(Run &r, const PolA &pa, const PolB &pb) {
    if (r.step >= r.first) {
        IBVH_LAUNCH((level_kernel<I, PolA, PolB>), dim3(level_grid()), dim3(TPB), 0, r.st, (const IndexPair<I> *)r.src(),
                    (IndexPair<I> *)r.dst(), r.capacity, r.counters, r.step, r.chk, pa, pb);
        IBVH_LAUNCH_CHECK();
    }
    r.step += 1;
    r.swapped = !r.swapped;
    return IBVH_OK;
}

// flag + per-step queue counts, then per-step check counts
inline size_t counters_bytes(int64_t total_levels) { return (size_t)(total_levels + 8) * 8 * (1 + GEN_SLOTS); }

// fresh run: counters zeroed, counters[1] = initial queue size.  Resume (res->resume_step > 0): the queue the
// overflowed step reads — res->contacts_in says which buffer — still holds res->resume_num entries; the flag and
// the counts from that step on are cleared, the earlier counts stay (they are part of num_checks).
inline int begin(Run &r, void *bvtt1, void *bvtt2, int64_t capacity, void *counters, int64_t total_levels, hipStream_t st,
                 const ibvh_bfs_result *res, int64_t initial) {
    r.st = st;
    r.counters = (unsigned long long *)counters;
    r.capacity = capacity;
    r.total_levels = total_levels;
    r.q[0] = bvtt1;
    r.q[1] = bvtt2;
    r.chk = (int)(total_levels + 8);
    if (res->resume_step > 0) {
        if (res->resume_step > total_levels + 4) return IBVH_ERR_INVALID_ARG;
        r.first = (int)res->resume_step;
        const size_t half = (size_t)(total_levels + 8) * 8;
        const size_t keep = (size_t)(2 + r.first) * 8; // flag + counts of the sources of steps 0 .. first
        IBVH_HIP_CHECK(hipMemsetAsync(counters, 0, 8, st));
        IBVH_HIP_CHECK(hipMemsetAsync((char *)counters + keep, 0, half - keep, st));
        // the checks of steps 0 .. first - 1 stay; step `first` runs again from the start
        for (int k = 0; k < GEN_SLOTS; ++k)
            IBVH_HIP_CHECK(hipMemsetAsync((char *)counters + half * (size_t)(1 + k) + (size_t)r.first * 8, 0, half - (size_t)r.first * 8, st));
        return IBVH_OK;
    }
    IBVH_HIP_CHECK(hipMemsetAsync(counters, 0, counters_bytes(total_levels), st));
    unsigned long long init = (unsigned long long)initial;
    IBVH_HIP_CHECK(hipMemcpyAsync((char *)counters + 8, &init, 8, hipMemcpyHostToDevice, st)); // (pageable: copied before return)
    return IBVH_OK;
}

// the one blocking read: flag + all counts
inline int finish(const Run &r, ibvh_bfs_result *res) {
    unsigned long long host[80 * (1 + GEN_SLOTS)];
    const int nsteps = r.step;
    if (nsteps + 2 > r.chk || r.chk > 80) return IBVH_ERR_INVALID_ARG;
    IBVH_HIP_CHECK(hipMemcpyAsync(host, r.counters, (size_t)r.chk * (1 + GEN_SLOTS) * 8, hipMemcpyDeviceToHost, r.st));
    IBVH_HIP_CHECK(hipStreamSynchronize(r.st));
    const unsigned long long flag = host[0];
    if (flag != 0ull) {
        const int s = (int)flag - 1; // the first step whose destination was too small
        const int64_t need = (int64_t)host[2 + s];
        res->num_contacts = 0;
        res->num_checks = 0;
        // the source queue of step s: buffer 1 if s is even (nothing swapped yet), buffer 2 otherwise
        res->contacts_in = (s % 2 == 0) ? 1 : 2;
        res->required_capacity = need + need / 4 + 1024; // exact need of the step that overflowed + headroom
        res->resume_step = s;
        res->resume_num = (int64_t)host[1 + s];
        return IBVH_ERR_CAPACITY;
    }
    // num_checks (bfs/traverse_single.jl:25,48, traverse_pair.jl:146-150): every entry of every queue of the reference
    // is one check — the initial queue plus each node-level result, i.e. every pair a step here generated and checked;
    // what passes the last (leaf) step is the contact list
    int64_t checks = 0;
    for (int k = 0; k < GEN_SLOTS; ++k)
        for (int s = 0; s < nsteps; ++s) checks += (int64_t)host[r.chk * (1 + k) + s];
    res->num_contacts = (int64_t)host[1 + nsteps];
    res->num_checks = checks;
    res->contacts_in = r.swapped ? 2 : 1;
    res->required_capacity = 0;
    res->resume_step = 0;
    res->resume_num = 0;
    return IBVH_OK;
}
inline int capacity_error(ibvh_bfs_result *res, int64_t need) {
    res->num_contacts = 0;
    res->num_checks = 0;
    res->contacts_in = 1;
    res->required_capacity = need + need / 4 + 1024;
    res->resume_step = 0; // nothing to keep: the initial queue itself did not fit
    res->resume_num = 0;
    return IBVH_ERR_CAPACITY;
}

// pairs in the initial queue of each traversal (the fill kernels above)
inline int64_t self_initial(const ibvh_bvh &b, int64_t start_level) {
    int64_t n = level_num_real(b.tree.levels, b.tree.virtual_leaves, start_level);
    return start_level != b.tree.levels ? n * (n - 1) / 2 + n : n * (n - 1) / 2;
}
inline int64_t pair_initial(const ibvh_bvh &b1, const ibvh_bvh &b2, int64_t sl1, int64_t sl2) {
    return level_num_real(b1.tree.levels, b1.tree.virtual_leaves, sl1) * level_num_real(b2.tree.levels, b2.tree.virtual_leaves, sl2);
}
inline int64_t rays_initial(const ibvh_bvh &b, int64_t num_rays, int64_t start_level) {
    return level_num_real(b.tree.levels, b.tree.virtual_leaves, start_level) * num_rays;
}

// the caller's buffers, as every entry point takes them
struct Buffers {
    void *bvtt1, *bvtt2;
    int64_t capacity;
    void *counters;
    ibvh_bfs_result *res;
    hipStream_t st;
    bool ok() const { return bvtt1 && bvtt2 && counters && capacity >= 1; }
};

// One traversal: the initial queue of `total0` pairs, which `fill(queue)` writes unless the call resumes, is checked by
// pol(0); then the children of what passed, level by level, by pol(1) .. pol(ns - 1).
template <class I, class Fill, class Pol>
int run_steps(const Buffers &q, int64_t total_levels, int64_t total0, Fill &&fill, int ns, Pol &&pol) {
    Run r;
    if (q.res->resume_step == 0 && total0 > q.capacity) return capacity_error(q.res, total0);
    if (int e = begin(r, q.bvtt1, q.bvtt2, q.capacity, q.counters, total_levels, q.st, q.res, total0)) return e;
    if (r.first == 0) fill((IndexPair<I> *)q.bvtt1);
    if (int e = step<I>(r, Identity<I>{}, pol(0))) return e;
    for (int i = 0; i + 1 < ns; ++i)
        if (int e = step<I>(r, pol(i), pol(i + 1))) return e;
    return finish(r, q.res);
}

template <class L_, class N_, class I_> struct Types { // what dispatch() hands to its callable
    using L = L_;
    using N = N_;
    using I = I_;
};

template <class L, class N, class I>
int run_self(Types<L, N, I>, const ibvh_bvh &b, int64_t start_level, int narrow, const Buffers &q) {
    ibvh_layout lay;
    LeafLayout dl;
    layout_of(b.types, lay, &dl);
    const int64_t levels = b.tree.levels;
    const int64_t n0 = level_num_real(levels, b.tree.virtual_leaves, start_level);
    const int64_t total0 = self_initial(b, start_level);
    auto fill = [&](IndexPair<I> *queue) {
        if (total0 > 0)
            IBVH_LAUNCH((fill_self_kernel<I>), dim3((unsigned)ceil_div(total0, TPB)), dim3(TPB), 0, q.st, queue, n0,
                        int64_t(1) << (start_level - 1), start_level != levels ? 1 : 0, total0);
    };
    auto at = [&](int i) {
        const int64_t level = start_level + i;
        return SelfStep<L, N, I>{make_ref<L, N>(b, dl, level), level == levels ? 1 : 0, level < levels - 1 ? 1 : 0 /* self_checks (:44) */,
                                 narrow & IBVH_NARROW_MASK, (narrow & IBVH_OUTPUT_POSITIONS) ? 1 : 0};
    };
    return run_steps<I>(q, levels, total0, fill, (int)(levels - start_level) + 1, at);
}

template <class L, class N, class I>
int run_pair(Types<L, N, I>, const ibvh_bvh &b1, const ibvh_bvh &b2, int64_t sl1, int64_t sl2, int narrow, const Buffers &q) {
    ibvh_layout lay;
    LeafLayout dl;
    layout_of(b1.types, lay, &dl);
    const int64_t L1 = b1.tree.levels, L2 = b2.tree.levels;
    const int64_t nr1 = level_num_real(L1, b1.tree.virtual_leaves, sl1), nr2 = level_num_real(L2, b2.tree.virtual_leaves, sl2);
    const int64_t total0 = pair_initial(b1, b2, sl1, sl2);
    auto fill = [&](IndexPair<I> *queue) {
        IBVH_LAUNCH((fill_product_kernel<I>), dim3((unsigned)ceil_div(total0, TPB)), dim3(TPB), 0, q.st, queue, nr1, nr2,
                    int64_t(1) << (sl1 - 1), int64_t(1) << (sl2 - 1));
    };
    // the six-phase descent of bfs/traverse_pair.jl:50-143 as a list of (levels, which side is a leaf, which descends)
    PairStep<L, N, I> seq[132];
    int ns = 0;
    int64_t l1 = sl1, l2 = sl2;
    auto add = [&](bool leaf1, bool leaf2, bool d1, bool d2) {
        PairStep<L, N, I> p;
        p.t1 = make_ref<L, N>(b1, dl, l1);
        p.t2 = make_ref<L, N>(b2, dl, l2);
        p.narrow = narrow & IBVH_NARROW_MASK;
        p.positions = (narrow & IBVH_OUTPUT_POSITIONS) ? 1 : 0;
        p.leaf1 = leaf1, p.leaf2 = leaf2, p.d1 = d1, p.d2 = d2;
        seq[ns++] = p;
    };
    while (l1 < L1 - 1 && l2 < L2 - 1) {
        add(false, false, true, true);
        ++l1, ++l2;
    }
    while (l1 < L1 - 1 && l2 == L2 - 1) {
        add(false, false, true, false);
        ++l1;
    }
    while (l2 < L2 - 1 && l1 == L1 - 1) {
        add(false, false, false, true);
        ++l2;
    }
    while (l2 == L2 && l1 < L1) {
        add(false, true, true, false);
        ++l1;
    }
    while (l1 == L1 && l2 < L2) {
        add(true, false, false, true);
        ++l2;
    }
    if (l1 == L1 - 1 && l2 == L2 - 1) {
        add(false, false, true, true);
        ++l1, ++l2;
    }
    // leaf-leaf: what passes is the contact list (num_checks is not incremented after it, bfs/traverse_pair.jl:146-150)
    add(true, true, false, false);
    return run_steps<I>(q, L1 + L2, total0, fill, ns, [&](int i) { return seq[i]; });
}

template <class L, class N, class I>
int run_rays(Types<L, N, I>, const ibvh_bvh &b, const void *points, const void *dirs, int64_t num_rays, int64_t start_level,
             int narrow, const Buffers &q) {
    using T = typename L::elt;
    ibvh_layout lay;
    LeafLayout dl;
    layout_of(b.types, lay, &dl);
    const int64_t levels = b.tree.levels;
    const int64_t nr = level_num_real(levels, b.tree.virtual_leaves, start_level);
    const int64_t total0 = rays_initial(b, num_rays, start_level);
    auto fill = [&](IndexPair<I> *queue) {
        IBVH_LAUNCH((fill_product_kernel<I>), dim3((unsigned)ceil_div(total0, TPB)), dim3(TPB), 0, q.st, queue, nr, num_rays,
                    int64_t(1) << (start_level - 1), int64_t(1));
    };
    auto at = [&](int i) {
        const int64_t level = start_level + i;
        return RayStep<L, N, I>{make_ref<L, N>(b, dl, level), (const T *)points, (const T *)dirs, level == levels ? 1 : 0,
                                narrow & IBVH_NARROW_MASK, (narrow & IBVH_OUTPUT_POSITIONS) ? 1 : 0};
    };
    return run_steps<I>(q, levels, total0, fill, (int)(levels - start_level) + 1, at);
}

inline int check_levels(const ibvh_bvh &b, int64_t sl) {
    // @argcheck bvh.tree.levels >= start_level >= bvh.built_level (bfs/traverse_single.jl:9-11)
    if (!(b.tree.levels >= sl && sl >= b.built_level && sl >= 1)) return IBVH_ERR_INVALID_ARG;
    if (b.tree.levels > 62) return IBVH_ERR_INVALID_ARG;
    return IBVH_OK;
}

// What every traversal entry does first with its in / out argument: the resume fields are input and stay, the rest is
// reset to "nothing found" (what a call that has nothing to traverse returns).  False: the resume fields are invalid.
inline bool reset_result(ibvh_bfs_result *result) {
    const ibvh_bfs_result in = *result;
    *result = {0, 0, 1, 0, in.resume_step, in.resume_num};
    return in.resume_step >= 0 && in.resume_num >= 0;
}

template <class F> int dispatch(const ibvh_types &t, F &&f) {
    return dispatch_leaf_node(t, [&](auto lt, auto nt) -> int {
        return dispatch_index(t.index_type, [&](auto it) -> int {
            return f(Types<typename decltype(lt)::type, typename decltype(nt)::type, typename decltype(it)::type>{});
        });
    });
}

} // namespace bfs
} // namespace ibvh

using namespace ibvh;
using namespace ibvh::bfs;

extern "C" {

ibvh_status ibvh_bfs_counters_bytes(int64_t total_levels, size_t *bytes_out) {
    if (!bytes_out || total_levels < 0) return IBVH_ERR_INVALID_ARG;
    *bytes_out = counters_bytes(total_levels);
    return IBVH_OK;
}

ibvh_status ibvh_bfs_initial_capacity(const ibvh_bvh *bvh, int64_t start_level, int64_t *pairs_out) {
    if (!bvh || !pairs_out) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh, start_level)) return (ibvh_status)e;
    *pairs_out = self_initial(*bvh, start_level);
    return IBVH_OK;
}
ibvh_status ibvh_bfs_pair_initial_capacity(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t sl1, int64_t sl2,
                                           int64_t *pairs_out) {
    if (!bvh1 || !bvh2 || !pairs_out) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh1, sl1)) return (ibvh_status)e;
    if (int e = check_levels(*bvh2, sl2)) return (ibvh_status)e;
    *pairs_out = pair_initial(*bvh1, *bvh2, sl1, sl2);
    return IBVH_OK;
}
ibvh_status ibvh_bfs_rays_initial_capacity(const ibvh_bvh *bvh, int64_t num_rays, int64_t start_level, int64_t *pairs_out) {
    if (!bvh || !pairs_out || num_rays < 0) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh, start_level)) return (ibvh_status)e;
    *pairs_out = rays_initial(*bvh, num_rays, start_level);
    return IBVH_OK;
}

// (each entry keeps the order of its checks: the status of a call that fails several, and whether *result was reset
// before a refusal, are observable)
ibvh_status ibvh_traverse_bfs(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow, void *bvtt1, void *bvtt2,
                              int64_t capacity, void *counters, ibvh_bfs_result *result, void *stream) {
    if (!bvh || !result) return IBVH_ERR_INVALID_ARG;
    if (!reset_result(result)) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh, start_level)) return (ibvh_status)e;
    if (!narrow_arg_ok(narrow, false)) return IBVH_ERR_INVALID_ARG;
    if (bvh->tree.real_nodes <= 1) return IBVH_OK; // bfs/traverse_single.jl:17-21
    const Buffers q{bvtt1, bvtt2, capacity, counters, result, (hipStream_t)stream};
    if (!q.ok()) return IBVH_ERR_INVALID_ARG;
    if (bvh->types.index_type == IBVH_I32 && bvh->tree.levels > 31) return IBVH_ERR_OVERFLOW;
    return (ibvh_status)dispatch(bvh->types, [&](auto t) -> int { return run_self(t, *bvh, start_level, narrow, q); });
}

ibvh_status ibvh_traverse_pair_bfs(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t sl1, int64_t sl2, int32_t narrow,
                                   void *bvtt1, void *bvtt2, int64_t capacity, void *counters, ibvh_bfs_result *result,
                                   void *stream) {
    if (!bvh1 || !bvh2 || !result) return IBVH_ERR_INVALID_ARG;
    if (!reset_result(result)) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh1, sl1)) return (ibvh_status)e;
    if (int e = check_levels(*bvh2, sl2)) return (ibvh_status)e;
    if (!same_types(bvh1->types, bvh2->types)) return IBVH_ERR_UNSUPPORTED;
    if (!narrow_arg_ok(narrow, false)) return IBVH_ERR_INVALID_ARG;
    const Buffers q{bvtt1, bvtt2, capacity, counters, result, (hipStream_t)stream};
    if (!q.ok()) return IBVH_ERR_INVALID_ARG;
    if (bvh1->types.index_type == IBVH_I32 && (bvh1->tree.levels > 31 || bvh2->tree.levels > 31)) return IBVH_ERR_OVERFLOW;
    return (ibvh_status)dispatch(bvh1->types, [&](auto t) -> int { return run_pair(t, *bvh1, *bvh2, sl1, sl2, narrow, q); });
}

ibvh_status ibvh_traverse_rays_bfs(const ibvh_bvh *bvh, const void *points, const void *dirs, int64_t num_rays,
                                   int64_t start_level, int32_t narrow, void *bvtt1, void *bvtt2, int64_t capacity,
                                   void *counters, ibvh_bfs_result *result, void *stream) {
    if (!bvh || !result || num_rays < 0 || !narrow_arg_ok(narrow, true)) return IBVH_ERR_INVALID_ARG; // (before the reset)
    if (!reset_result(result)) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh, start_level)) return (ibvh_status)e;
    if (bvh->types.leaf_float != bvh->types.node_float) return IBVH_ERR_UNSUPPORTED;
    if (num_rays == 0) return IBVH_OK;
    const Buffers q{bvtt1, bvtt2, capacity, counters, result, (hipStream_t)stream};
    if (!points || !dirs || !q.ok()) return IBVH_ERR_INVALID_ARG;
    if (bvh->types.index_type == IBVH_I32 && (bvh->tree.levels > 31 || num_rays > INT32_MAX)) return IBVH_ERR_OVERFLOW;
    return (ibvh_status)dispatch(bvh->types, [&](auto t) -> int {
        using T = decltype(t);
        if constexpr (!std::is_same<typename T::L::elt, typename T::N::elt>::value) return (int)IBVH_ERR_UNSUPPORTED;
        else return run_rays(t, *bvh, points, dirs, num_rays, start_level, narrow, q);
    });
}

} // extern "C"
