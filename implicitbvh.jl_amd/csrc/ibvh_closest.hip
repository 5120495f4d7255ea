// ibvh_closest.hip — for a batch of query points, the closest triangle of the mesh a BVH was built over: which one, where
// on it, and how far (include/ibvh.h, ibvh_closest_triangles).  No reference counterpart: every traversal of ImplicitBVH.jl
// is a fixed-volume overlap test (traverse/, raytrace/); nothing there prunes on a bound that shrinks while it walks.
//
// The answer is defined over ALL triangles — the lexicographic minimum of (d2, index) — so the walk only has to be
// lossless.  It is, without an epsilon: the walk's point-box bound is computed by the same operations in the same order
// as the point-triangle distance, the triangle's closest point is clamped into the triangle's box, and every box of the tree
// contains the boxes below it exactly (min / max and widening conversions), so the COMPUTED bound of a box never exceeds
// the COMPUTED distance of a triangle under it (round-to-nearest subtraction, multiplication and addition are monotone).
//
// The walk itself — work mapping, near child first, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's.
#include "ibvh_pointwalk.hpp"
#include "ibvh_pointtri.hpp"

#include <limits>

namespace ibvh {
namespace closest {

using pointwalk::kBlock;

using pointtri::closest_on_triangle; // the evaluation of include/ibvh.h: ibvh_pointtri.hpp, shared with ibvh_spheres.hip

// T: the leaves' and triangles' float type; TN: the nodes' (the same or wider — a node box then holds values of T, widened
// exactly, and narrows back exactly)
template <class T, class TN, class I>
__global__ __launch_bounds__(kBlock) void closest_walk_kernel(TreeDev tree, int built_level, const char *__restrict__ leaves,
                                                              LeafLayout lay, const BBox<TN> *__restrict__ nodes,
                                                              const T *__restrict__ tris, int64_t num_triangles,
                                                              const T *__restrict__ points, int64_t num_points, T max_d2,
                                                              I *__restrict__ out_index, T *__restrict__ out_d2,
                                                              T *__restrict__ out_q, uint32_t *flag) {
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_points; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {points[3 * item], points[3 * item + 1], points[3 * item + 2]};
        T best = max_d2, bq[3] = {T(0), T(0), T(0)};
        I best_index = 0;
        // only a leaf that passes gathers its triangle (36 / 72 bytes)
        auto visit = [&](const char *rec) {
            I index;
            T tr[9], q[3];
            int region; // (not part of this query's answer)
            if (pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, tr)) {
                const T d2 = closest_on_triangle(tr, p, q, region);
                if (pointwalk::wins(d2, index, best, best_index)) { // (d2, index) lexicographically; best starts at the radius
                    best = d2;
                    best_index = index;
                    bq[0] = q[0];
                    bq[1] = q[1];
                    bq[2] = q[2];
                }
            } else {
                bad = true;
            }
        };
        auto box = [&](const T *lo, const T *up) { return pointwalk::box_bound(lo, up, p); }; // lb(B) of include/ibvh.h
        if (!pointwalk::hopeless(p, max_d2)) // (a NaN point or radius: a miss)
            pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, [&]() { return best; }, visit);
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
    // box leaves: the lossless bound needs boxes all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_points == 0 || points);
    const ibvh_status st = pointwalk::prepare(bvh, true, num_points, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    return (ibvh_status)pointwalk::dispatch_box_types(bvh->types, [&](auto ft, auto nt, auto it) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        IBVH_LAUNCH((closest::closest_walk_kernel<T, TN, I>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0, (hipStream_t)stream,
                    pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay, (const BBox<TN> *)bvh->nodes,
                    (const T *)triangles, num_triangles, (const T *)points, num_points, pointwalk::radius_or_inf<T>(max_distance2),
                    (I *)closest_index, (T *)closest_d2, (T *)closest_point, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    });
}

} // extern "C"
