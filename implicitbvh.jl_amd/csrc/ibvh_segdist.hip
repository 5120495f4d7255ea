// ibvh_segdist.hip — for a batch of segments a -> b, the CLOSEST triangle of the mesh a BVH was built over: which one, how
// far, the closest point on the segment and on the triangle, and which rule decided (include/ibvh.h,
// ibvh_segment_distances).  The distance query beside ibvh_capsules.hip's "which triangles touch": clearance of a link, a
// rod or a step's swept path from a surface.  No reference counterpart: ImplicitBVH.jl's traversals end at pairs of BOXES;
// nothing there measures a gap.
//
// A pair (S, K) is evaluated by ibvh_segtri.hpp: the cut rule (d2 = 0 where the segment crosses K) or the smallest of five
// candidates.  The answer is defined over ALL triangles — the lexicographic minimum of (d2, index) — so the walk only has to
// be lossless.  It is, without an epsilon, by ibvh_tridist.hip's steps (1) - (4) with S's box in place of Q's: every xs lies
// in S's exact box (an end does, segseg's x1 is clamped into it); every xk lies in K's exact box, hence in K's leaf box
// (skin or not) and in every box above it; the bound of a box is the squared gap between it and S's box, computed from the
// faces by the monotone operations d2 is computed with from the points, in the same order, so the COMPUTED bound never
// exceeds a COMPUTED d2 under the box; a cut pair's boxes are not apart, so its bound is 0, the d2 the cut rule gives.  The
// definition reads the triangle's own box, not the stored one, so leaf boxes with a skin change nothing.  There is no slab
// clause here: the answer has no radius to grow a box by.
//
// The walk itself — work mapping, near child first, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, the
// gather its leaf_triangle, the bound ibvh_trigeom.hpp's box_gap.  S, its box, the best pair so far and the trail live in
// registers: one lane, one segment, one launch.
//
// The lane walks twice, by ibvh_pairwalk.hpp's routine: first ibvh_closest.hip's walk from the end a — the point candidate 0
// of ibvh_segtri.hpp's evaluation is evaluated from, which is what that routine's argument asks of its caller —, then the
// query's own walk from the limit the first one found, not from the radius: an unbounded query then prunes from its first
// node on.
#include "ibvh_pairwalk.hpp"
#include "ibvh_pointwalk.hpp"
#include "ibvh_segtri.hpp"

namespace ibvh {
namespace segdist {

using pointwalk::kBlock;

// T: the leaves', triangles' and segments' float type; TN: the nodes' (the same or wider — a node box then holds values of T,
// widened exactly, and narrows back exactly)
template <class T, class TN, class I>
__global__ __launch_bounds__(pointwalk::kBlock) void segdist_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ starts, const T *__restrict__ ends,
    int64_t num_segments, T max_d2, I *__restrict__ out_index, T *__restrict__ out_d2, T *__restrict__ out_xs,
    T *__restrict__ out_xk, uint8_t *__restrict__ out_kind, uint32_t *flag) {
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_segments; item += (int64_t)gridDim.x * kBlock) {
        const T a[3] = {starts[3 * item], starts[3 * item + 1], starts[3 * item + 2]};
        const T b[3] = {ends[3 * item], ends[3 * item + 1], ends[3 * item + 2]};
        T slo[3], sup[3]; // S's box: exact
        segtri::segment_box(a, b, slo, sup);
        // the bound of include/ibvh.h: the squared gap between S's box and the box, in d2's operation order
        auto box = [&](const T *lo, const T *up) -> T { return trigeom::box_gap(lo, up, slo, sup); };
        // only a leaf that passes gathers its triangle (36 / 72 bytes); false: it names none
        auto gather = [&](const char *rec, I &index, raytri::Tri<T> &K) -> bool {
            const bool named = pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, K.v);
            bad |= !named;
            return named;
        };
        auto pair = [&](const raytri::Tri<T> &K, trigeom::Pair<T> &r) { segtri::evaluate(a, b, slo, sup, K, r); };
        // a NaN in the segment or in the radius has no answer, and a NaN could not prune
        const bool nan = pointwalk::hopeless(a, max_d2) || pointwalk::hopeless(b, max_d2);
        trigeom::Pair<T> best;
        const I best_index = pairwalk::closest_pair<I>(tree, built_level, leaves, lay, nodes, nan, a, max_d2, box, gather, pair, best);
        pairwalk::store_pair(item, best_index, best, out_index, out_d2, out_xs, out_xk, out_kind);
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace segdist
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_segment_distances(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *starts,
                                   const void *ends, int64_t num_segments, const void *max_distance2, void *closest_index,
                                   void *closest_d2, void *point_segment, void *point_mesh, void *closest_kind, void *flag,
                                   void *stream) {
    if (!bvh || num_triangles < 0 || num_segments < 0) return IBVH_ERR_INVALID_ARG;
    if (!closest_index && !closest_d2 && !point_segment && !point_mesh && !closest_kind) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless bound needs boxes all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_segments == 0 || (starts && ends));
    const ibvh_status st = pointwalk::prepare(bvh, true, num_segments, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    return (ibvh_status)pointwalk::dispatch_box_types(bvh->types, [&](auto ft, auto nt, auto it) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        IBVH_LAUNCH((segdist::segdist_walk_kernel<T, TN, I>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0, (hipStream_t)stream,
                    pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay, (const BBox<TN> *)bvh->nodes,
                    (const T *)triangles, num_triangles, (const T *)starts, (const T *)ends, num_segments,
                    pointwalk::radius_or_inf<T>(max_distance2), (I *)closest_index, (T *)closest_d2, (T *)point_segment,
                    (T *)point_mesh, (uint8_t *)closest_kind, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    });
}

} // extern "C"
