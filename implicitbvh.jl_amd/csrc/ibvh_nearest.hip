// ibvh_nearest.hip — for a batch of query points, the k leaves of a BVH whose CENTRES are nearest: which ones and how far
// (include/ibvh.h, ibvh_nearest_leaves).  No reference counterpart: every traversal of ImplicitBVH.jl is a fixed-volume
// overlap test.  The walk is ibvh_pointwalk.hpp's — one lane per query, near child first, a node or a leaf skipped iff its
// bound > the k-th best so far, strictly — here for the k best leaf centres, of sphere leaves and box leaves.
//
// The answer is defined over ALL leaves — the k lexicographically smallest (d2, index) — so the walk only has to be
// lossless.  It is, without an epsilon: a leaf's centre lies in the leaf's own box (x -/+ r around x; lo <= 0.5 (lo + up)
// <= up) and in every node box above it (exact minima / maxima and widening conversions), the bound of a box clamps the
// point into the box and then takes the distance by the centre distance's own operations, so per component
// |p - clamp(p)| <= |p - c|, and round-to-nearest subtraction, multiplication and addition are monotone: the COMPUTED bound
// of a box never exceeds the COMPUTED d2 of a centre inside it.
//
// The k best live in registers as a list sorted by (d2, index), K slots for a compile-time K >= k (1, 4, 8 or 16: the smallest that holds k).  A requested
// k < K uses the LAST k slots; the K - k slots in front hold d2 = -Inf and are never displaced, so the last slot is always
// the k-th best and the pruning bound is exact for every k, not only for k = K.  Slots not yet filled hold max_distance2:
// the last slot is the bound from the first step on.  An insertion is K comparisons and a fully unrolled shift with
// compile-time slot numbers only: nothing is indexed at run time, nothing lands in scratch memory.
#include "ibvh_pointwalk.hpp"

#include <limits>

namespace ibvh {
namespace nearest {

using pointwalk::kBlock;

// VL: the leaves' volume type, T its float type; TN: the nodes' (the same or wider — a node box then holds values of T,
// widened exactly, and narrows back exactly); K: slots of the list, 1 <= k <= K
template <class VL, class TN, class I, int K>
__global__ __launch_bounds__(kBlock) void nearest_walk_kernel(TreeDev tree, int built_level, const char *__restrict__ leaves,
                                                              LeafLayout lay, const BBox<TN> *__restrict__ nodes,
                                                              const typename VL::elt *__restrict__ points, int64_t num_points,
                                                              int k, typename VL::elt max_d2, I *__restrict__ out_index,
                                                              typename VL::elt *__restrict__ out_d2) {
    using T = typename VL::elt;
    const int base = K - k; // the first slot of the answer
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_points; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {points[3 * item], points[3 * item + 1], points[3 * item + 2]};
        T d[K];
        I ix[K];
        int cnt = 0; // filled slots: base .. base + cnt - 1
#pragma unroll
        for (int j = 0; j < K; ++j) {
            d[j] = j < base ? -std::numeric_limits<T>::infinity() : max_d2;
            ix[j] = 0;
        }
        auto visit = [&](const char *rec) {
            const I index = load_index<I>(rec, lay);
            T c[3];
            center(load_vol<VL>(rec), c);
            const T e[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
            const T d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
            // (d2, index) against the k-th best; while slots are free anything within the radius enters
            const bool full = cnt == k;
            if ((d2 <= max_d2) & (!full | (d2 < d[K - 1]) | ((d2 == d[K - 1]) & (index < ix[K - 1])))) {
                bool lt[K]; // the candidate sorts before slot j (a free slot is behind everything)
#pragma unroll
                for (int j = 0; j < K; ++j) lt[j] = (j >= base + cnt) | (d2 < d[j]) | ((d2 == d[j]) & (index < ix[j]));
#pragma unroll
                for (int j = K - 1; j > 0; --j) {
                    d[j] = lt[j - 1] ? d[j - 1] : (lt[j] ? d2 : d[j]);
                    ix[j] = lt[j - 1] ? ix[j - 1] : (lt[j] ? index : ix[j]);
                }
                d[0] = lt[0] ? d2 : d[0];
                ix[0] = lt[0] ? index : ix[0];
                cnt += full ? 0 : 1;
            }
        };
        auto box = [&](const T *lo, const T *up) { return pointwalk::box_bound(lo, up, p); }; // lb(B) of include/ibvh.h
        if (!pointwalk::hopeless(p, max_d2)) // (a NaN point or radius: no answer)
            pointwalk::walk<VL, TN>(tree, built_level, leaves, lay, nodes, box, [&]() { return d[K - 1]; }, visit);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j >= base) {
                const bool filled = j - base < cnt;
                if (out_index) out_index[item * k + (j - base)] = filled ? ix[j] : I(0);
                if (out_d2) out_d2[item * k + (j - base)] = filled ? d[j] : std::numeric_limits<T>::infinity();
            }
        }
    }
}

} // namespace nearest
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_nearest_leaves(const ibvh_bvh *bvh, const void *points, int64_t num_points, int32_t k,
                                const void *max_distance2, void *nearest_index, void *nearest_d2, void *stream) {
    if (!bvh || num_points < 0 || k < 1 || k > IBVH_NEAREST_MAX_K) return IBVH_ERR_INVALID_ARG;
    if (!nearest_index && !nearest_d2) return IBVH_ERR_INVALID_ARG;
    // sphere leaves too: only their centres are asked for
    pointwalk::Prepared pre;
    const ibvh_status st = pointwalk::prepare(bvh, false, num_points, num_points == 0 || points, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    const ibvh_types &t = bvh->types;
    return (ibvh_status)dispatch_volume(t.leaf_kind, t.leaf_float, [&](auto lt) -> int {
        using VL = typename decltype(lt)::type;
        using T = typename VL::elt;
        const T max_d2 = pointwalk::radius_or_inf<T>(max_distance2);
        return dispatch_index(t.index_type, [&](auto it) -> int {
            using I = typename decltype(it)::type;
            auto launch = [&](auto nt, auto kt) -> int {
                using TN = typename decltype(nt)::type;
                constexpr int K = decltype(kt)::value;
                IBVH_LAUNCH((nearest::nearest_walk_kernel<VL, TN, I, K>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0,
                            (hipStream_t)stream, pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay,
                            (const BBox<TN> *)bvh->nodes, (const T *)points, num_points, (int)k, max_d2, (I *)nearest_index,
                            (T *)nearest_d2);
                IBVH_LAUNCH_CHECK();
                return IBVH_OK;
            };
            // the smallest list that holds k
            auto with_k = [&](auto nt) -> int {
                if (k <= 1) return launch(nt, std::integral_constant<int, 1>{});
                if (k <= 4) return launch(nt, std::integral_constant<int, 4>{});
                if (k <= 8) return launch(nt, std::integral_constant<int, 8>{});
                return launch(nt, std::integral_constant<int, IBVH_NEAREST_MAX_K>{});
            };
            if constexpr (sizeof(T) == 8) return with_k(Tag<double>{});
            else return t.node_float == IBVH_F64 ? with_k(Tag<double>{}) : with_k(Tag<float>{});
        });
    });
}

} // extern "C"
