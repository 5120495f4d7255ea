// ibvh_closest.hip — for a batch of query points, the closest triangle of the mesh a BVH was built over: which one, where
// on it, and how far (include/ibvh.h, ibvh_closest_triangles).  No reference counterpart: every traversal of ImplicitBVH.jl
// is a fixed-volume overlap test (traverse/, raytrace/); nothing there prunes on a bound that shrinks while it walks.
//
// The answer is defined over ALL triangles — the lexicographic minimum of (d2, index) — so the walk only has to be
// lossless.  It is, without an epsilon: the point-box bound below is computed by the same operations in the same order as
// the point-triangle distance, the triangle's closest point is clamped into the triangle's box, and every box of the tree
// contains the boxes below it exactly (min / max and widening conversions), so the COMPUTED bound of a box never exceeds
// the COMPUTED distance of a triangle under it (round-to-nearest subtraction, multiplication and addition are monotone).
// A box is skipped iff bound > best: strictly, because an equal distance under it may carry a smaller index.
//
// Work mapping: one lane per query, everything in registers.  The lane descends to the child with the smaller bound
// first and keeps ONE bit per level — "the other child is still owed" — in a 64-bit trail word (levels <= 62): no
// indexable private array, nothing in scratch memory.  A pop scans the trail for the deepest owed bit, finds the owed
// sibling from the current path (node >> depth difference, ^ 1) and tests its bound again against the CURRENT best: that is
// where the shrinking bound pays.  Leaves are walked like nodes (their stored box is the bound); only a leaf that passes
// gathers its triangle (36 / 72 bytes).  Lanes of a wave share nodes when neighbouring queries are neighbours in space:
// the entry point keeps the order it is given, the host mirrors sort the batch along a Morton curve first.
#include "ibvh_common.hpp"

#include <limits>

namespace ibvh {
namespace closest {

constexpr int kBlock = 64; // one wave a workgroup: walks differ in length, and a wave that is done frees its slot at once

template <class T> IBVH_D T dot3(const T *x, const T *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// lb(B) of include/ibvh.h: the squared distance from p to the box, by the operations of the point-triangle d2
template <class T> IBVH_D T box_bound(const T *lo, const T *up, const T *p) {
    T f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T c = p[k] < lo[k] ? lo[k] : (p[k] > up[k] ? up[k] : p[k]);
        f[k] = p[k] - c;
    }
    return (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];
}

// Ericson's region walk (Real-Time Collision Detection 5.1.5), the first matching case decides; then q is clamped into the
// triangle's exact box.  -ffp-contract=off: every operation is rounded once.
template <class T> IBVH_D T closest_on_triangle(const T *tr, const T *p, T *q) {
    const T *a = tr, *b = tr + 3, *c = tr + 6;
    const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const T ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const T ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const T d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    const T bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const T d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    const T cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const T d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const T vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if ((d1 <= T(0)) & (d2 <= T(0))) {
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k];
    } else if ((d3 >= T(0)) & (d4 <= d3)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k];
    } else if ((vc <= T(0)) & (d1 >= T(0)) & (d3 <= T(0))) {
        const T v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k];
    } else if ((d6 >= T(0)) & (d5 <= d6)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = c[k];
    } else if ((vb <= T(0)) & (d2 >= T(0)) & (d6 <= T(0))) {
        const T w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k];
    } else if ((va <= T(0)) & ((d4 - d3) >= T(0)) & ((d5 - d6) >= T(0))) {
        const T w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k] + w * (c[k] - b[k]);
    } else {
        const T den = T(1) / ((va + vb) + vc);
        const T v = vb * den, w = vc * den;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (a[k] + v * ab[k]) + w * ac[k];
    }
    T e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T lo = minimum3(a[k], b[k], c[k]), up = maximum3(a[k], b[k], c[k]); // bbox_from_triangle
        q[k] = q[k] < lo ? lo : (q[k] > up ? up : q[k]);                            // (NaN stays NaN)
        e[k] = p[k] - q[k];
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// T: the leaves' and triangles' float type; TN: the nodes' (the same or wider — a node box then holds values of T, widened
// exactly, and narrows back exactly)
template <class T, class TN, class I>
__global__ __launch_bounds__(kBlock) void closest_walk_kernel(TreeDev tree, int built_level, const char *__restrict__ leaves,
                                                              LeafLayout lay, const BBox<TN> *__restrict__ nodes,
                                                              const T *__restrict__ tris, int64_t num_triangles,
                                                              const T *__restrict__ points, int64_t num_points, T max_d2,
                                                              I *__restrict__ out_index, T *__restrict__ out_d2,
                                                              T *__restrict__ out_q, uint32_t *flag) {
    const int levels = (int)tree.levels;
    const int64_t vl = tree.virtual_leaves;
    const uint64_t leaf_first = uint64_t(1) << (levels - 1);
    const int64_t roots = level_num_real(levels, vl, built_level);
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_points; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {points[3 * item], points[3 * item + 1], points[3 * item + 2]};
        T best = max_d2, bq[3] = {T(0), T(0), T(0)};
        I best_index = 0;

        // bound of implicit node `i` of `level`: a node box, or at the last level the leaf's stored box
        auto bound_of = [&](uint64_t i, int level) -> T {
            if (level == levels) {
                const BBox<T> b = load_vol<BBox<T>>(leaves + (int64_t)(i - leaf_first) * lay.stride);
                return box_bound(b.lo, b.up, p);
            }
            const BBox<TN> n = load_vol<BBox<TN>>(nodes + ((int64_t)i - level_skips(levels, vl, level) - 1));
            const T lo[3] = {T(n.lo[0]), T(n.lo[1]), T(n.lo[2])}, up[3] = {T(n.up[0]), T(n.up[1]), T(n.up[2])};
            return box_bound(lo, up, p);
        };

        // a NaN coordinate makes every d2 NaN and a NaN radius admits nothing: a miss either way, and no bound could prune
        const bool hopeless = !((p[0] == p[0]) & (p[1] == p[1]) & (p[2] == p[2]) & (max_d2 == max_d2));
        for (int64_t r = 0; r < roots && !hopeless; ++r) {
            uint64_t node = (uint64_t(1) << (built_level - 1)) + (uint64_t)r;
            int level = built_level;
            uint64_t trail = 0; // bit l: the sibling of the path's node at level l is still owed
            if (bound_of(node, level) > best) continue;
            for (;;) {
                bool descended = false;
                if (level == levels) {
                    const char *rec = leaves + (int64_t)(node - leaf_first) * lay.stride;
                    const I index = load_index<I>(rec, lay);
                    if (index >= 1 && (int64_t)index <= num_triangles) {
                        T tr[9], q[3];
                        __builtin_memcpy(tr, __builtin_assume_aligned(tris + 9 * ((int64_t)index - 1), sizeof(T)), sizeof(tr));
                        const T d2 = closest_on_triangle(tr, p, q);
                        // (d2, index) lexicographically; the first one only has to be within the radius (best == max_d2)
                        if ((d2 < best) | ((d2 == best) & ((best_index == 0) | (index < best_index)))) {
                            best = d2;
                            best_index = index;
                            bq[0] = q[0];
                            bq[1] = q[1];
                            bq[2] = q[2];
                        }
                    } else {
                        bad = true;
                    }
                } else {
                    const int cl = level + 1;
                    const uint64_t c0 = 2 * node, c1 = c0 + 1; // (a real node's first child is real)
                    const bool real1 = (int64_t)(c1 - (uint64_t(1) << (cl - 1))) < level_num_real(levels, vl, cl);
                    const T lb0 = bound_of(c0, cl), lb1 = bound_of(real1 ? c1 : c0, cl);
                    const bool go0 = !(lb0 > best), go1 = real1 && !(lb1 > best);
                    if (go0 | go1) {
                        node = go1 && (!go0 || lb1 < lb0) ? c1 : c0; // the nearer child first
                        level = cl;
                        if (go0 & go1) trail |= uint64_t(1) << cl;
                        descended = true;
                    }
                }
                if (descended) continue;
                // pop: the deepest owed sibling whose bound still reaches the best found since
                bool found = false;
                while (trail != 0) {
                    const int l = 63 - __builtin_clzll(trail);
                    trail &= ~(uint64_t(1) << l);
                    const uint64_t sibling = (node >> (level - l)) ^ 1u;
                    if (!(bound_of(sibling, l) > best)) {
                        node = sibling;
                        level = l;
                        found = true;
                        break;
                    }
                }
                if (!found) break;
            }
        }
        const bool hit = best_index != 0;
        if (out_index) out_index[item] = best_index;
        if (out_d2) out_d2[item] = hit ? best : std::numeric_limits<T>::infinity();
        if (out_q) {
            out_q[3 * item] = bq[0];
            out_q[3 * item + 1] = bq[1];
            out_q[3 * item + 2] = bq[2];
        }
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace closest
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_closest_triangles(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *points,
                                   int64_t num_points, const void *max_distance2, void *closest_index, void *closest_d2,
                                   void *closest_point, void *flag, void *stream) {
    if (!bvh || num_triangles < 0 || num_points < 0) return IBVH_ERR_INVALID_ARG;
    if (!closest_index && !closest_d2 && !closest_point) return IBVH_ERR_INVALID_ARG;
    const ibvh_types &t = bvh->types;
    if (!combo_ok(t)) return IBVH_ERR_UNSUPPORTED;
    // the lossless bound needs boxes all the way up, holding the leaves' values exactly
    if (t.leaf_kind != IBVH_BBOX || t.node_kind != IBVH_BBOX) return IBVH_ERR_UNSUPPORTED;
    if (t.leaf_float == IBVH_F64 && t.node_float == IBVH_F32) return IBVH_ERR_UNSUPPORTED;
    const ibvh_tree &tr = bvh->tree;
    if (tr.levels < 1 || tr.levels > 62 || tr.real_leaves < 1 || tr.virtual_leaves < 0) return IBVH_ERR_INVALID_ARG;
    if (tr.real_leaves + tr.virtual_leaves != (int64_t(1) << (tr.levels - 1))) return IBVH_ERR_INVALID_ARG;
    if (bvh->built_level < 1 || bvh->built_level > tr.levels) return IBVH_ERR_INVALID_ARG;
    if (!bvh->leaves || (bvh->built_level < tr.levels && !bvh->nodes)) return IBVH_ERR_INVALID_ARG;
    if ((num_triangles > 0 && !triangles) || (num_points > 0 && !points)) return IBVH_ERR_INVALID_ARG;
    if (num_points == 0) return IBVH_OK;
    ibvh_layout layout;
    LeafLayout lay;
    if (!layout_of(t, layout, &lay)) return IBVH_ERR_UNSUPPORTED;
    const TreeDev tree{tr.levels, tr.real_leaves, tr.virtual_leaves};
    const int64_t b = ceil_div(num_points, closest::kBlock);
    const unsigned blocks = (unsigned)(b > (int64_t(1) << 22) ? (int64_t(1) << 22) : b);
    auto launch = [&](auto ft, auto nt, auto it) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        const T max_d2 = max_distance2 ? *(const T *)max_distance2 : std::numeric_limits<T>::infinity();
        IBVH_LAUNCH((closest::closest_walk_kernel<T, TN, I>), dim3(blocks), dim3(closest::kBlock), 0, (hipStream_t)stream, tree,
                    (int)bvh->built_level, (const char *)bvh->leaves, lay, (const BBox<TN> *)bvh->nodes, (const T *)triangles,
                    num_triangles, (const T *)points, num_points, max_d2, (I *)closest_index, (T *)closest_d2,
                    (T *)closest_point, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)dispatch_index(t.index_type, [&](auto it) -> int {
        if (t.leaf_float == IBVH_F64) return launch(Tag<double>{}, Tag<double>{}, it);
        return t.node_float == IBVH_F64 ? launch(Tag<float>{}, Tag<double>{}, it) : launch(Tag<float>{}, Tag<float>{}, it);
    });
}

} // extern "C"
