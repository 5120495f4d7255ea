// ibvh_pointwalk.hpp — what the queries that walk one item (a point, a ray, a triangle, a segment, a box) per lane through a
// BVH have in common.  Per unit: what the walk bounds a box by, and whether the query keeps a best answer or lists all.
//   ibvh_closest.hip    the squared distance from the point to the box                         best: the closest triangle
//   ibvh_nearest.hip    the same                                                               best: the k nearest leaf centres
//   ibvh_crossings.hip  0 / 1: an axis ray from the point can / cannot meet the box            sums: the crossings, their orientations
//   ibvh_cast.hip       the ray's entry distance into the box (ibvh_slab.hpp)                  best: the closest hit, or any hit
//   ibvh_sweep.hip      that entry, into the box grown by the sphere's radius                  best: the first contact, or any
//   ibvh_tridist.hip    the squared gap between the box and the triangle's box                 best: the closest triangle
//   ibvh_segdist.hip    the squared gap between the box and the segment's box                  best: the closest triangle
//   ibvh_spheres.hip    0 / 1: the point's squared distance to the box is within r * r or not  list: the triangles within r
//   ibvh_tritri.hip     0 / 1: the box is not / is apart from the triangle's box               list: the triangles it cuts
//   ibvh_capsules.hip   0 / 1: that gap within r * r and the grown entry within 1, or not      list: the triangles within r
//   ibvh_boxes.hip      0 / 1: the box is not / is apart from the oriented box's hull          list: the triangles it overlaps
//   ibvh_spherecast.hip the centre's entry into the box grown by the radius, over SPHERE leaves  best: the first leaf, or any
// No reference counterpart: every traversal of ImplicitBVH.jl is a fixed-volume overlap test (traverse/, raytrace/).
//
// For the kernels: the workgroup size, the distance queries' point-box bound (box_bound) and NaN test (hopeless), the walk,
// the mesh queries' gather of a leaf's triangle (leaf_triangle), the best-answer queries' tie rule (wins), and the list
// queries' rows (first_row, contact, store_count: the count / write protocol).  For the entry points: the rules they share
// and prepare(), the one place that applies them, in the one order a call with several faults is refused in; the
// (T, TN, I) dispatch of a tree with box leaves, and the same with a bool as a fourth tag — the pass of a list query, the
// any-hit mode of ibvh_cast.hip, ibvh_sweep.hip and ibvh_spherecast.hip —; the list queries' two-pass argument rule
// (passes_ok); the optional radius.  An entry point keeps its own checks (counts, axis, k, skip, which outputs it has) and
// its launch.  The box and triangle primitives are ibvh_trigeom.hpp's, the two pair distances' seeded walk is
// ibvh_pairwalk.hpp's, the three first-hit queries' closest / any-hit protocol — the limit, the answer, the walk under the
// mode's limit, the common stores, the mode / outputs rule — is ibvh_firsthit.hpp's.
//
// A query hands the walk three things: bound(lo, up), its lower bound for a box (box_bound below for the distance queries;
// 0 / 1 = "the ray can / cannot meet the box" for the crossings; the slab test's entry distance for the ray cast), limit(),
// the value beyond which nothing can enter its answer any more, and visit(rec), what to do with a leaf record that is still
// within it.  The walk is lossless if the
// COMPUTED bound of a box never exceeds the COMPUTED bound or distance of anything the query could find under it; each query
// argues that for its own bound.  A box is skipped iff bound > limit(): strictly, because an equal distance under it may
// carry a smaller index.
//
// Work mapping: one lane per query, everything in registers.  The lane descends to the child with the smaller bound
// first and keeps ONE bit per level — "the other child is still owed" — in a 64-bit trail word (levels <= 62): no
// indexable private array, nothing in scratch memory.  A pop scans the trail for the deepest owed bit, finds the owed
// sibling from the current path (node >> depth difference, ^ 1) and tests its bound again against the CURRENT limit: that is
// where the shrinking bound pays.  Leaves are walked like nodes (the box of their stored volume is the bound); only a leaf
// that passes is visited.  Lanes of a wave share nodes when neighbouring queries are neighbours in space: the entry points
// keep the order they are given, the host mirrors sort the batch along a Morton curve first.
#pragma once
#include "ibvh_common.hpp"

#include <limits>
#include <type_traits>

namespace ibvh {
namespace pointwalk {

constexpr int kBlock = 64; // one wave a workgroup: walks differ in length, and a wave that is done frees its slot at once

// lb(B) of include/ibvh.h: the squared distance from p to the box, by the operations of the queries' own d2
template <class T> IBVH_D T box_bound(const T *lo, const T *up, const T *p) {
    T f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T c = p[k] < lo[k] ? lo[k] : (p[k] > up[k] ? up[k] : p[k]);
        f[k] = p[k] - c;
    }
    return (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];
}

// The walk of one query from every root of the built part of the tree.  VL: the leaves' volume type, T its float
// type; TN: the nodes' (the same or wider — a node box then holds values of T, widened exactly, and narrows back exactly).
// bound(const T *lo, const T *up) -> T is the query's bound of a box (it knows the query point); limit() -> T is read
// afresh at every test; visit(const char *rec) may lower it.
template <class VL, class TN, class Bound, class Limit, class Visit>
IBVH_D void walk(const TreeDev &tree, int built_level, const char *__restrict__ leaves, const LeafLayout &lay,
                 const BBox<TN> *__restrict__ nodes, const Bound &bound, const Limit &limit, const Visit &visit) {
    using T = typename VL::elt;
    const int levels = (int)tree.levels;
    const int64_t vl = tree.virtual_leaves;
    const uint64_t leaf_first = uint64_t(1) << (levels - 1);
    const int64_t roots = level_num_real(levels, vl, built_level);

    // bound of implicit node `i` of `level`: a node box, or at the last level the box of the leaf's stored volume
    auto bound_of = [&](uint64_t i, int level) -> T {
        if (level == levels) {
            const BBox<T> b = convert_to(load_vol<VL>(leaves + (int64_t)(i - leaf_first) * lay.stride), (BBox<T> *)nullptr);
            return bound(b.lo, b.up);
        }
        const BBox<TN> n = load_vol<BBox<TN>>(nodes + ((int64_t)i - level_skips(levels, vl, level) - 1));
        const T lo[3] = {T(n.lo[0]), T(n.lo[1]), T(n.lo[2])}, up[3] = {T(n.up[0]), T(n.up[1]), T(n.up[2])};
        return bound(lo, up);
    };

    for (int64_t r = 0; r < roots; ++r) {
        uint64_t node = (uint64_t(1) << (built_level - 1)) + (uint64_t)r;
        int level = built_level;
        uint64_t trail = 0; // bit l: the sibling of the path's node at level l is still owed
        if (bound_of(node, level) > limit()) continue;
        for (;;) {
            bool descended = false;
            if (level == levels) {
                visit(leaves + (int64_t)(node - leaf_first) * lay.stride);
            } else {
                const int cl = level + 1;
                const uint64_t c0 = 2 * node, c1 = c0 + 1; // (a real node's first child is real)
                const bool real1 = (int64_t)(c1 - (uint64_t(1) << (cl - 1))) < level_num_real(levels, vl, cl);
                const T lb0 = bound_of(c0, cl), lb1 = bound_of(real1 ? c1 : c0, cl);
                const bool go0 = !(lb0 > limit()), go1 = real1 && !(lb1 > limit());
                if (go0 | go1) {
                    node = go1 && (!go0 || lb1 < lb0) ? c1 : c0; // the nearer child first
                    level = cl;
                    if (go0 & go1) trail |= uint64_t(1) << cl;
                    descended = true;
                }
            }
            if (descended) continue;
            // pop: the deepest owed sibling whose bound still reaches the limit as it stands now
            bool found = false;
            while (trail != 0) {
                const int l = 63 - __builtin_clzll(trail);
                trail &= ~(uint64_t(1) << l);
                const uint64_t sibling = (node >> (level - l)) ^ 1u;
                if (!(bound_of(sibling, l) > limit())) {
                    node = sibling;
                    level = l;
                    found = true;
                    break;
                }
            }
            if (!found) break;
        }
    }
}

// The mesh queries' visit of a leaf record that passed: the leaf's index -> `index`, and, if it names one of the
// num_triangles rows of `tris` (1-based), that triangle's nine values (36 / 72 bytes) -> tr9 and true.  false: the index lies
// outside the mesh, nothing was gathered; the caller skips the leaf and raises flag bit 1 when its lane is done.
template <class T, class I>
IBVH_D bool leaf_triangle(const char *rec, const LeafLayout &lay, const T *tris, int64_t num_triangles, I &index, T *tr9) {
    index = load_index<I>(rec, lay);
    if (!(index >= 1 && (int64_t)index <= num_triangles)) return false;
    __builtin_memcpy(tr9, __builtin_assume_aligned(tris + 9 * ((int64_t)index - 1), sizeof(T)), 9 * sizeof(T));
    return true;
}

// The list queries' rows.  Both passes walk alike and meet an item's contacts in the same order; WRITE is the second, which
// puts contact j of item i in row offsets[i] + j, otherwise the first, which only counts them.  One uint64 serves both: the
// count pass's one counter, the write pass's running row (wraps, never overflows: a wild offset is only refused).
template <bool WRITE> IBVH_D uint64_t first_row(const int64_t *offsets, int64_t item) {
    if constexpr (WRITE) return (uint64_t)offsets[item];
    else return 0;
}

// a contact was found: the write pass hands its row to put(row) if it lies below capacity (a negative row is a huge one),
// else notes `over`, for flag bit 2 when the lane is done; both passes move on to the next row
template <bool WRITE, class Put> IBVH_D void contact(uint64_t &row, int64_t capacity, bool &over, const Put &put) {
    if constexpr (WRITE) {
        if (row < (uint64_t)capacity) put(row);
        else over = true;
    }
    ++row;
}

// the item's walk is done: the count pass stores how many it met
template <bool WRITE> IBVH_D void store_count(int64_t *counts, int64_t item, uint64_t row) {
    if constexpr (!WRITE) counts[item] = (int64_t)row;
}

// a NaN coordinate makes every d2 NaN and a NaN radius admits nothing: no answer either way, and no bound could prune
template <class T> IBVH_D bool hopeless(const T *p, T max_d2) {
    return !((p[0] == p[0]) & (p[1] == p[1]) & (p[2] == p[2]) & (max_d2 == max_d2));
}

// The best-answer queries' tie rule: (x, index) lies lexicographically below (best, best_index); the first one only has to
// be within the limit `best` starts from (best_index == 0: nothing yet).  Every comparison is false on NaN
template <class T, class I> IBVH_D bool wins(T x, I index, T best, I best_index) {
    return (x < best) | ((x == best) & ((best_index == 0) | (index < best_index)));
}

// ---- the entry points' common front end (host) ---------------------------------------------------------------------

// the lossless bound needs boxes above the leaves, holding the leaves' values exactly (else IBVH_ERR_UNSUPPORTED)
inline bool box_nodes_hold_leaves(const ibvh_types &t) {
    return t.node_kind == IBVH_BBOX && !(t.leaf_float == IBVH_F64 && t.node_float == IBVH_F32);
}

// an ImplicitTree's shape the trail word can hold, built from a level that exists, with the arrays the walk reads (else
// IBVH_ERR_INVALID_ARG)
inline bool tree_ok(const ibvh_bvh *bvh) {
    const ibvh_tree &tr = bvh->tree;
    if (tr.levels < 1 || tr.levels > 62 || tr.real_leaves < 1 || tr.virtual_leaves < 0) return false;
    if (tr.real_leaves + tr.virtual_leaves != (int64_t(1) << (tr.levels - 1))) return false;
    if (bvh->built_level < 1 || bvh->built_level > tr.levels) return false;
    return bvh->leaves && (bvh->built_level == tr.levels || bvh->nodes);
}

// workgroups for num_points queries; the kernels stride over what a clamped grid leaves
inline unsigned grid_blocks(int64_t num_points) {
    const int64_t b = ceil_div(num_points, kBlock);
    return (unsigned)(b > (int64_t(1) << 22) ? (int64_t(1) << 22) : b);
}

// what a launch needs besides the entry point's own arguments; blocks == 0: nothing to launch
struct Prepared {
    TreeDev tree;
    LeafLayout lay;
    unsigned blocks = 0;
};

// The checks every entry point makes once its own are done, in the order a call with several faults is refused in: the type
// combination and — box_leaves: the query reads a triangle's box from its leaf — the leaf kind (IBVH_ERR_UNSUPPORTED), the
// tree, then pointers_ok, the caller's "the arrays this many queries need are there" (IBVH_ERR_INVALID_ARG); num == 0 is
// IBVH_OK with nothing to launch.  Otherwise fills `out` for a grid over num queries.
inline ibvh_status prepare(const ibvh_bvh *bvh, bool box_leaves, int64_t num, bool pointers_ok, Prepared &out) {
    const ibvh_types &t = bvh->types;
    if (!combo_ok(t)) return IBVH_ERR_UNSUPPORTED;
    if ((box_leaves && t.leaf_kind != IBVH_BBOX) || !box_nodes_hold_leaves(t)) return IBVH_ERR_UNSUPPORTED;
    if (!tree_ok(bvh) || !pointers_ok) return IBVH_ERR_INVALID_ARG;
    if (num == 0) return IBVH_OK;
    ibvh_layout layout;
    if (!layout_of(t, layout, &out.lay)) return IBVH_ERR_UNSUPPORTED;
    out.tree = tree_dev(bvh->tree);
    out.blocks = grid_blocks(num);
    return IBVH_OK;
}

// (T, TN, I) of a tree with box leaves that prepare() admitted — the leaves' float type, the nodes' (the same or wider) and
// the index type — as f(Tag<T>, Tag<TN>, Tag<I>)
template <class F> int dispatch_box_types(const ibvh_types &t, F &&f) {
    return dispatch_index(t.index_type, [&](auto it) -> int {
        if (t.leaf_float == IBVH_F64) return f(Tag<double>{}, Tag<double>{}, it);
        return t.node_float == IBVH_F64 ? f(Tag<float>{}, Tag<double>{}, it) : f(Tag<float>{}, Tag<float>{}, it);
    });
}

// The list queries' two passes.  Their public mode enums are one pair of values, which the rule below relies on.
static_assert(IBVH_SPHERES_COUNT == 0 && IBVH_SPHERES_WRITE == 1 && IBVH_TRIS_COUNT == 0 && IBVH_TRIS_WRITE == 1, "one pair");
static_assert(IBVH_CAPSULES_COUNT == 0 && IBVH_CAPSULES_WRITE == 1, "the same pair"); // (ibvh_capsules.hip)
static_assert(IBVH_BOXES_COUNT == 0 && IBVH_BOXES_WRITE == 1, "the same pair"); // (ibvh_boxes.hip)

// a valid mode; the count pass needs counts, the write pass offsets and at least one output (else IBVH_ERR_INVALID_ARG)
inline bool passes_ok(int32_t mode, const void *counts, const void *offsets, bool any_output) {
    return mode == IBVH_SPHERES_WRITE ? offsets && any_output : mode == IBVH_SPHERES_COUNT && counts;
}

// dispatch_box_types with a bool as a fourth tag, std::bool_constant<flag>, so that it is a template parameter of the kernel:
// the pass of a list query (write: the counting kernel carries no outputs and reads no offsets), the any-hit mode of the
// first-hit queries (ibvh_firsthit.hpp: the any-hit kernel carries no best hit)
template <class F> int dispatch_box_types_and_bool(const ibvh_types &t, bool flag, F &&f) {
    return dispatch_box_types(t, [&](auto ft, auto nt, auto it) -> int {
        return flag ? f(ft, nt, it, std::true_type{}) : f(ft, nt, it, std::false_type{});
    });
}

// an optional squared radius: the host scalar of type T behind p, +Inf where there is none
template <class T> T radius_or_inf(const void *p) { return p ? *(const T *)p : std::numeric_limits<T>::infinity(); }

} // namespace pointwalk
} // namespace ibvh
