// ibvh_spherecast.hip — cast rays and swept spheres against the sphere cloud a BVH was built over, in one launch: per
// query sphere of radius r >= 0 whose centre moves from p to p + d (r = 0: a ray) the FIRST leaf sphere it touches and when,
// or only whether it touches anything within its limit (include/ibvh.h, ibvh_cast_spheres).  Lidar and camera rays into a
// granular bed, line of sight between particles, a fast particle that must not tunnel through a layer.  No reference
// counterpart: ImplicitBVH.jl's ray traversal lists every leaf whose bounding sphere the whole LINE meets.
//
// The result is defined over ALL leaves — the lexicographic minimum of (t*, index) over the hits — so the walk only has to
// be lossless.  The mesh queries argue "every box of the tree contains the boxes below it exactly".  With sphere leaves that
// is FALSE at the lowest node level: the merge of two spheres a, b into a box (merge.jl:58-81) returns the box of b alone when
// length + a.r <= b.r holds in rounded arithmetic, and the box of a can then poke out of it by an ulp.  A query that starts at
// the poking tip and does not move along that axis is admitted by the leaf's own box and refused by its parent's.  So the
// parent's STORED box is part of the definition:
//     t* = max(max(t, entry of the leaf's own box grown by r), entry of the stored box directly above the leaf, grown by r)
// (the last where that level exists and is built).  Above that level every merge is an exact minimum / maximum with an exact
// widening, lo - r and up + r are round-to-nearest, hence monotone, and the slab entry is monotone in the corners
// (ibvh_sweep.hip's argument), so   t* >= entry(grown parent) >= entry(every grown ancestor),   and the walk's bound of the
// leaf itself is the entry of its own grown box, <= t*.  Hence a box skipped iff bound > limit, strictly, holds nothing that
// can still win or tie: every box on the path to a leaf that could enter the answer has a bound <= its t* <= the limit.
//
// The walk — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, unchanged, with ibvh_slab.hpp's
// entry of the grown box (grown_entry) as the bound; the leaf's time is ibvh_raysphere.hpp's.  The limit, the answer and the
// walk under the mode's limit — from the query's own t_max down to the best t* so far, or to -Inf at the first hit — are
// ibvh_firsthit.hpp's.
// visit() finds the parent from the record pointer: the leaf's position is (rec - leaves) / stride, the parent's implicit
// index (leaf_first + position) >> 1, its memory index that minus the virtual nodes before its level; the lane read that box
// a few steps earlier in the same descent.  Query, inverse displacement and best hit live in registers.
#include "ibvh_firsthit.hpp"
#include "ibvh_raysphere.hpp"
#include "ibvh_slab.hpp"

#include <limits>

namespace ibvh {
namespace spherecast {

using pointwalk::kBlock;

// T: the leaves' and queries' float type; TN: the nodes' (the same or wider — a node box then holds values of T, widened
// exactly, and narrows back exactly); ANY: only "does it touch anything", the walk ends at the first hit
template <class T, class TN, class I, bool ANY>
__global__ __launch_bounds__(pointwalk::kBlock) void cast_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ points, const T *__restrict__ disps, const T *__restrict__ radii, int64_t num,
    const T *__restrict__ t_max, const I *__restrict__ skip, I *__restrict__ out_index, T *__restrict__ out_t,
    uint8_t *__restrict__ out_touched) {
    const int levels = (int)tree.levels;
    // the level directly above the leaves, where it exists and is built: its first node's implicit index minus its memory index
    const bool has_parent = levels >= 2 && built_level <= levels - 1;
    const int64_t parent_base = has_parent ? level_skips(levels, tree.virtual_leaves, levels - 1) + 1 : 0;
    const uint64_t leaf_first = uint64_t(1) << (levels - 1);
    const bool narrow_offsets = (uint64_t)tree.real_leaves * (uint64_t)lay.stride <= 0xffffffffull; // (a 32-bit divide)
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {points[3 * item], points[3 * item + 1], points[3 * item + 2]};
        const T d[3] = {disps[3 * item], disps[3 * item + 1], disps[3 * item + 2]};
        const T inv[3] = {T(1) / d[0], T(1) / d[1], T(1) / d[2]};
        const T r = radii ? radii[item] : T(0);
        const T dd = raysphere::dot3(d, d);
        const I ignored = skip ? skip[item] : I(0);
        const T L = firsthit::limit(t_max, item);
        firsthit::Answer<T, I> answer(L);
        // the entry of the centre's ray into a box grown by r (monotone roundings: above the lowest node level a grown node
        // holds its grown children)
        auto grown = [&](const T *lo, const T *up) { return slab::grown_entry(lo, up, r, p, d, inv); };
        auto visit = [&](const char *rec) {
            const BSphere<T> s = load_vol<BSphere<T>>(rec);
            const I index = load_index<I>(rec, lay);
            const T tk = raysphere::first_touch(s.x, s.r, p, d, dd, r);
            const BBox<T> own = convert_to(s, (BBox<T> *)nullptr);
            const T entry = grown(own.lo, own.up);
            T ts = tk > entry ? tk : entry; // t*: the clamps (+Inf: no touch, or a grown box refused)
            if (has_parent) {
                const uint64_t offset = (uint64_t)(rec - leaves);
                const uint64_t position = narrow_offsets ? (uint64_t)((uint32_t)offset / (uint32_t)lay.stride) : offset / (uint64_t)lay.stride;
                const BBox<TN> n = load_vol<BBox<TN>>(nodes + ((int64_t)((leaf_first + position) >> 1) - parent_base));
                const T lo[3] = {T(n.lo[0]), T(n.lo[1]), T(n.lo[2])}, up[3] = {T(n.up[0]), T(n.up[1]), T(n.up[2])};
                const T above = grown(lo, up);
                ts = ts > above ? ts : above;
            }
            if (index != ignored) firsthit::offer<ANY>(answer, ts, index, []() {}); // (no payload)
        };
        // a NaN in the query, a negative or NaN radius touch nothing; t* >= 0: a negative or NaN limit admits nothing, and a
        // NaN could not prune
        const bool numbers = (p[0] == p[0]) & (p[1] == p[1]) & (p[2] == p[2]) & (d[0] == d[0]) & (d[1] == d[1]) & (d[2] == d[2]);
        if (numbers & (r >= T(0)) & (L >= T(0))) firsthit::walk<ANY, BSphere<T>, TN>(tree, built_level, leaves, lay, nodes, answer, grown, visit);
        firsthit::store<ANY>(answer, item, out_index, out_t, out_touched);
    }
}

} // namespace spherecast
} // namespace ibvh

using namespace ibvh;
using pointwalk::dispatch_box_types_and_bool; // (reads only the float and index types: it serves sphere leaves too)

extern "C" {

ibvh_status ibvh_cast_spheres(const ibvh_bvh *bvh, const void *points, const void *displacements, const void *radii,
                              int64_t num, const void *t_max, const void *skip, int32_t mode, void *hit_index, void *hit_t,
                              void *touched, void *stream) {
    if (!bvh || num < 0) return IBVH_ERR_INVALID_ARG;
    if (!firsthit::outputs_ok(mode, touched, hit_index || hit_t)) return IBVH_ERR_INVALID_ARG;
    const bool any = mode == IBVH_SPHERECAST_ANY;
    // sphere leaves only (the definition is theirs), under boxes that hold their values exactly
    if (bvh->types.leaf_kind != IBVH_BSPHERE) return IBVH_ERR_UNSUPPORTED;
    pointwalk::Prepared pre;
    const ibvh_status st = pointwalk::prepare(bvh, false, num, num == 0 || (points && displacements), pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto mt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool ANY = decltype(mt)::value;
        IBVH_LAUNCH((spherecast::cast_walk_kernel<T, TN, I, ANY>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0, (hipStream_t)stream,
                    pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay, (const BBox<TN> *)bvh->nodes,
                    (const T *)points, (const T *)displacements, (const T *)radii, num, (const T *)t_max, (const I *)skip,
                    (I *)hit_index, (T *)hit_t, (uint8_t *)touched);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)dispatch_box_types_and_bool(bvh->types, any, launch);
}

} // extern "C"
