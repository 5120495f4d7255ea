// ibvh_capsules.hip — for a batch of capsules (a segment a -> b with a radius r), EVERY triangle of the mesh a BVH was built
// over that lies within r of the segment: which ones, how far, the closest point on the segment and on the triangle, and
// which rule decided (include/ibvh.h, ibvh_capsule_contacts).  The narrow phase of capsule-vs-mesh contact: robot links,
// character controllers, rods and fibres, the swept volume of a particle over a step.  No reference counterpart:
// ImplicitBVH.jl's traversal ends at pairs of BOXES, and the box of a long diagonal segment is far looser than the segment.
//
// A triangle k is a contact iff (i) the slab entry of the segment's ray p = a, d = b - a into leaf k's STORED box grown by r
// is <= 1, and (ii) d2 <= r * r by ibvh_segtri.hpp's evaluation.  In real arithmetic (ii) implies (i): a point of K within r
// of a point a + t d, 0 <= t <= 1, lies in the box grown by r, so the ray is inside that box at t.  (i) is part of the
// definition so that the walk can prune on it without loss; it decides only pairs that rounding puts on the grown box's
// face.
//
// The lists are defined over ALL triangles, in leaf order, so the walk only has to be lossless and ordered.  A box is
// refused iff its squared gap to S's exact box exceeds r * r, or the slab entry of the box grown by r exceeds 1 (both false
// on NaN: such a box is entered).  Lossless, without an epsilon, by two arguments.  The gap: ibvh_tridist.hip's steps (1) -
// (4) with S's box in place of Q's — every xs lies in S's exact box (an end does, segseg's x1 is clamped into it), every xk
// lies in K's exact box, hence in its leaf's box and every box above; the gap is computed from the boxes' faces by the
// monotone operations d2 is computed with from the points, in the same order; a cut pair's boxes are not apart, its gap is 0
// — so the COMPUTED gap of a box never exceeds a COMPUTED d2 under it: a box with gap > r * r holds no pair that passes (ii).
// The slab: ibvh_sweep.hip's argument — lo - r and up + r are round-to-nearest, hence monotone, so the grown box of a node
// contains the grown boxes below it exactly; the slab entry is monotone in the corners; so a leaf that passes (i) has
// ancestors that pass.  Ordered: the walk is handed 0 ("may hold one") or 1 under a constant limit of 0, as in
// ibvh_spheres.hip: a depth-first walk from left to right, so the counting pass and the writing pass meet the same contacts
// in ascending leaf position, and contact j of the one is row j of the other.
//
// The walk itself — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, as are the gather
// (leaf_triangle), the rows of the two passes and the entry point's two-pass rule; the slab test is ibvh_slab.hpp's.  The
// walk tests a leaf's stored box like a node's, so a leaf that is visited has passed (i) already.  Segment, its box, the
// inverse direction, the squared radius and the running count live in registers; a contact goes straight from registers to
// its row.
#include "ibvh_pointwalk.hpp"
#include "ibvh_segtri.hpp"
#include "ibvh_slab.hpp"

namespace ibvh {
namespace capsules {

using pointwalk::kBlock;

// T: the leaves', triangles' and capsules' float type; TN: the nodes' (the same or wider — a node box then holds values of
// T, widened exactly, and narrows back exactly); WRITE: the second pass, which puts contact j of capsule s in row
// offsets[s] + j; otherwise the first, which only counts them
template <class T, class TN, class I, bool WRITE>
__global__ __launch_bounds__(pointwalk::kBlock) void capsules_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ starts, const T *__restrict__ ends,
    const T *__restrict__ radii, int64_t num_capsules, int64_t *__restrict__ counts, const int64_t *__restrict__ offsets,
    int64_t capacity, I *__restrict__ out_index, T *__restrict__ out_d2, T *__restrict__ out_xs, T *__restrict__ out_xk,
    uint8_t *__restrict__ out_kind, uint32_t *flag) {
    bool bad = false, over = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_capsules; item += (int64_t)gridDim.x * kBlock) {
        const T a[3] = {starts[3 * item], starts[3 * item + 1], starts[3 * item + 2]};
        const T b[3] = {ends[3 * item], ends[3 * item + 1], ends[3 * item + 2]};
        const T d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const T inv[3] = {T(1) / d[0], T(1) / d[1], T(1) / d[2]};
        const T r = radii[item];
        const T r2 = r * r;
        T slo[3], sup[3]; // S's box: exact
        segtri::segment_box(a, b, slo, sup);
        uint64_t next = pointwalk::first_row<WRITE>(offsets, item);
        // 0 = the box may hold a contact, 1 = it cannot: its gap to S's box exceeds r * r, or the segment's ray enters the box
        // grown by r beyond its end (both false on NaN: such a box is entered)
        auto box = [&](const T *lo, const T *up) -> T {
            const T gap = trigeom::box_gap(lo, up, slo, sup), entry = slab::grown_entry(lo, up, r, a, d, inv);
            return ((gap > r2) | (entry > T(1))) ? T(1) : T(0);
        };
        // only a leaf that passes — clause (i) on its stored box included — gathers its triangle (36 / 72 bytes)
        auto visit = [&](const char *rec) {
            I index;
            raytri::Tri<T> K;
            if (pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, K.v)) {
                trigeom::Pair<T> p;
                segtri::evaluate(a, b, slo, sup, K, p);
                if (p.d2 <= r2) { // clause (ii) (false on NaN)
                    pointwalk::contact<WRITE>(next, capacity, over, [&](uint64_t row) {
                        if (out_index) out_index[row] = index;
                        if (out_d2) out_d2[row] = p.d2;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            if (out_xs) out_xs[3 * row + k] = p.xq[k];
                            if (out_xk) out_xk[3 * row + k] = p.xk[k];
                        }
                        if (out_kind) out_kind[row] = (uint8_t)p.kind;
                    });
                }
            } else {
                bad = true;
            }
        };
        // a negative or NaN radius and a NaN in a or b touch nothing, and a NaN could not prune
        if ((r >= T(0)) && !pointwalk::hopeless(a, r2) && !pointwalk::hopeless(b, r2))
            pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, []() { return T(0); }, visit);
        pointwalk::store_count<WRITE>(counts, item, next);
    }
    if (bad && flag) raise_flag(flag, 2u);
    if (over && flag) raise_flag(flag, 4u);
}

} // namespace capsules
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_capsule_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *starts,
                                  const void *ends, const void *radii, int64_t num_capsules, int32_t mode, void *counts,
                                  const void *offsets, int64_t capacity, void *contact_index, void *contact_d2,
                                  void *contact_point_segment, void *contact_point_mesh, void *contact_kind, void *flag,
                                  void *stream) {
    if (!bvh || num_triangles < 0 || num_capsules < 0 || capacity < 0) return IBVH_ERR_INVALID_ARG;
    const bool any_output = contact_index || contact_d2 || contact_point_segment || contact_point_mesh || contact_kind;
    if (!pointwalk::passes_ok(mode, counts, offsets, any_output)) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless bounds need boxes that contain their triangles' boxes exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_capsules == 0 || (starts && ends && radii));
    const ibvh_status st = pointwalk::prepare(bvh, true, num_capsules, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto wt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool WRITE = decltype(wt)::value;
        IBVH_LAUNCH((capsules::capsules_walk_kernel<T, TN, I, WRITE>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0,
                    (hipStream_t)stream, pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay,
                    (const BBox<TN> *)bvh->nodes, (const T *)triangles, num_triangles, (const T *)starts, (const T *)ends,
                    (const T *)radii, num_capsules, (int64_t *)counts, (const int64_t *)offsets, capacity, (I *)contact_index,
                    (T *)contact_d2, (T *)contact_point_segment, (T *)contact_point_mesh, (uint8_t *)contact_kind,
                    (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)pointwalk::dispatch_box_types_and_bool(bvh->types, mode == IBVH_CAPSULES_WRITE, launch);
}

} // extern "C"
