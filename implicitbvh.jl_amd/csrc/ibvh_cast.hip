// ibvh_cast.hip — cast a batch of rays against the mesh a BVH was built over, in one launch: per ray the closest exactly
// hit triangle (index, t, u, v), or only whether anything lies in the way (include/ibvh.h, ibvh_cast_rays).  No reference
// counterpart: ImplicitBVH.jl's ray traversal stops at the (leaf, ray) candidate list of the whole infinite line
// (raytrace/leaf_vs_tree/leaf_vs_tree.jl:170-228); nothing there prunes on the best hit so far, limits a ray to a segment
// or stops at the first hit.
//
// The result is defined over ALL triangles — the lexicographic minimum of (t*, index) over the hits, t* = max(t, entry of
// the triangle's leaf box) — so the walk only has to be lossless.  It is, without an epsilon: the slab entry distance of a
// box is computed from (corner - p) * inv, round-to-nearest subtraction and multiplication by a fixed inv are monotone, and
// every box of the tree contains the boxes below it exactly (min / max, widening conversions, a skin margin, ibvh_refit).  So
// the COMPUTED entry of a node is <= that of every box below it, an admitted box has admitted ancestors, and
// t* >= entry(leaf) >= entry(every ancestor): a box whose entry exceeds the limit holds nothing that could still win.
//
// The walk itself — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, here with the slab
// entry as the bound.  The limit, the answer and the walk under the mode's limit — from the ray's own t_max down to the best
// t* so far, or to -Inf at the first hit — are ibvh_firsthit.hpp's, as are the stores of index and t*.  The exact test is
// ibvh_raytest.hpp's, the one copy ibvh_raytri.hip resolves candidate lists with.  Ray, inverse direction and best hit live
// in registers.
#include "ibvh_firsthit.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_slab.hpp"

#include <limits>

namespace ibvh {
namespace cast {

using pointwalk::kBlock;
using slab::slab_entry; // entry(box) of include/ibvh.h, the copy ibvh_sweep.hip prunes with too

// T: the leaves', triangles' and rays' float type; TN: the nodes' (the same or wider — a node box then holds values of T,
// widened exactly, and narrows back exactly); ANY: only "is there a hit", the walk ends at the first one
template <class T, class TN, class I, bool ANY>
__global__ __launch_bounds__(pointwalk::kBlock) void cast_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ points, const T *__restrict__ dirs, int64_t num_rays,
    const T *__restrict__ t_max, I *__restrict__ out_index, T *__restrict__ out_t, T *__restrict__ out_uv,
    uint8_t *__restrict__ out_occluded, uint32_t *flag) {
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_rays; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {points[3 * item], points[3 * item + 1], points[3 * item + 2]};
        const T d[3] = {dirs[3 * item], dirs[3 * item + 1], dirs[3 * item + 2]};
        const T inv[3] = {T(1) / d[0], T(1) / d[1], T(1) / d[2]};
        const T L = firsthit::limit(t_max, item);
        firsthit::Answer<T, I> answer(L);
        T best_u = T(0), best_v = T(0);
        auto box = [&](const T *lo, const T *up) { return slab_entry(lo, up, p, d, inv); };
        // only a leaf that passes gathers its triangle (36 / 72 bytes)
        auto visit = [&](const char *rec) {
            I index;
            raytri::Tri<T> tr;
            if (pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, tr.v)) {
                const BBox<T> b = load_vol<BBox<T>>(rec);
                const T entry = slab_entry(b.lo, b.up, p, d, inv);
                T t, u, v;
                if (raytri::ray_triangle(tr, p, d, t, u, v)) {
                    const T ts = entry > t ? entry : t; // t*: the clamp
                    firsthit::offer<ANY>(answer, ts, index, [&]() { best_u = u, best_v = v; });
                }
            } else {
                bad = true;
            }
        };
        // t* >= t >= 0: a negative or NaN limit admits nothing, and a NaN could not prune
        if (L >= T(0)) firsthit::walk<ANY, BBox<T>, TN>(tree, built_level, leaves, lay, nodes, answer, box, visit);
        firsthit::store<ANY>(answer, item, out_index, out_t, out_occluded);
        if constexpr (!ANY) {
            if (out_uv) out_uv[2 * item] = best_u, out_uv[2 * item + 1] = best_v;
        }
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace cast
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_cast_rays(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *points,
                           const void *directions, int64_t num_rays, const void *t_max, int32_t mode, void *hit_index,
                           void *hit_t, void *hit_uv, void *occluded, void *flag, void *stream) {
    if (!bvh || num_triangles < 0 || num_rays < 0) return IBVH_ERR_INVALID_ARG;
    if (!firsthit::outputs_ok(mode, occluded, hit_index || hit_t || hit_uv)) return IBVH_ERR_INVALID_ARG;
    const bool any = mode == IBVH_CAST_ANY;
    // box leaves: the lossless bound needs boxes that contain their triangles' boxes exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_rays == 0 || (points && directions));
    const ibvh_status st = pointwalk::prepare(bvh, true, num_rays, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto mt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool ANY = decltype(mt)::value;
        IBVH_LAUNCH((cast::cast_walk_kernel<T, TN, I, ANY>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0, (hipStream_t)stream,
                    pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay, (const BBox<TN> *)bvh->nodes,
                    (const T *)triangles, num_triangles, (const T *)points, (const T *)directions, num_rays, (const T *)t_max,
                    (I *)hit_index, (T *)hit_t, (T *)hit_uv, (uint8_t *)occluded, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)pointwalk::dispatch_box_types_and_bool(bvh->types, any, launch);
}

} // extern "C"
