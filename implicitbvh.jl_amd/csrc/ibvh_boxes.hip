// ibvh_boxes.hip — for a batch of boxes (a centre c, half extents h and, optionally, a rotation R whose rows are the box's
// axes), EVERY triangle of the mesh a BVH was built over that the box overlaps: which ones, and which of the triangle's
// vertices lie in the box (include/ibvh.h, ibvh_box_contacts).  The narrow phase of box-vs-mesh contact: an oriented box as
// a robot link, a vehicle hull or a rigid body's proxy; an axis-aligned one as a voxel, a region of interest or a culling
// cell.  No reference counterpart: ImplicitBVH.jl's traversal ends at pairs of BOXES, and the axis-aligned hull of a rotated
// box is up to sqrt(3) wider per axis than the box.
//
// A triangle k is a contact iff (i) leaf k's STORED box is not apart from the query's hull Q = c -+ e,
// e_k = ((|R_0k| * h_0 + |R_1k| * h_1) + |R_2k| * h_2) — ibvh_trigeom.hpp's six strict comparisons, every one false on NaN —
// and (ii) none of ibvh_tribox.hpp's 13 axes separates the triangle's local vertices
// v_k = ((u_k0 * w_0 + u_k1 * w_1) + u_k2 * w_2), w = p - c, from [-h, h].  In real arithmetic (ii) implies (i): a point of
// the box lies in its hull, a point of K in its leaf's box.  (i) is part of the definition so that the walk can prune on it
// without loss; it decides only pairs that rounding puts on a face of the hull.
//
// The lists are defined over ALL triangles, in leaf order, so the walk only has to be lossless and ordered.  Lossless,
// without an epsilon: a box of the tree is refused iff it is apart from Q; every box of the tree contains the boxes below it
// exactly, so a box that is apart from Q lies over leaf boxes that are apart from Q, which clause (i) refuses by definition.
// Ordered: the walk is handed 0 ("may hold one") or 1 under a constant limit of 0, as in ibvh_spheres.hip: a depth-first walk
// from left to right, so the counting pass and the writing pass meet the same contacts in ascending leaf position, and
// contact j of the one is row j of the other.
//
// The walk itself — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, as are the gather
// (leaf_triangle), the rows of the two passes and the entry point's two-pass rule; the 13 axes are ibvh_tribox.hpp's.  The
// walk tests a leaf's stored box like a node's, so a leaf that is visited has passed (i) already, and only such a leaf has
// its local vertices computed.  c, h, R, the hull and the running row live in registers; a contact goes straight from
// registers to its row.  rotations == NULL is the identity in the SAME arithmetic: one kernel, no second code path.
#include "ibvh_pointwalk.hpp"
#include "ibvh_tribox.hpp"
#include "ibvh_trigeom.hpp"

namespace ibvh {
namespace boxes {

using pointwalk::kBlock;

// T: the leaves', triangles' and boxes' float type; TN: the nodes' (the same or wider — a node box then holds values of T,
// widened exactly, and narrows back exactly); WRITE: the second pass, which puts contact j of box s in row offsets[s] + j;
// otherwise the first, which only counts them
template <class T, class TN, class I, bool WRITE>
__global__ __launch_bounds__(pointwalk::kBlock) void boxes_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ centers, const T *__restrict__ half_extents,
    const T *__restrict__ rotations, int64_t num_boxes, int64_t *__restrict__ counts, const int64_t *__restrict__ offsets,
    int64_t capacity, I *__restrict__ out_index, uint8_t *__restrict__ out_inside, uint32_t *flag) {
    bool bad = false, over = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_boxes; item += (int64_t)gridDim.x * kBlock) {
        tribox::Box<T> q;
        T finite = T(0); // 0 iff every value of c and R is finite: x - x is 0 then, NaN for a NaN or an infinity
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            q.c[k] = centers[3 * item + k];
            q.h[k] = half_extents[3 * item + k];
            finite = finite + (q.c[k] - q.c[k]);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            q.u[k] = T(k % 4 == 0 ? 1 : 0);
            if (rotations) q.u[k] = rotations[9 * item + k];
            finite = finite + (q.u[k] - q.u[k]);
        }
        T qlo[3], qup[3]; // the hull Q
        tribox::hull(q, qlo, qup);
        uint64_t next = pointwalk::first_row<WRITE>(offsets, item);
        // 0 = the box may hold a contact, 1 = it is apart from Q (false on NaN: such a box is entered)
        auto box = [&](const T *lo, const T *up) -> T { return trigeom::apart(qlo, qup, lo, up) ? T(1) : T(0); };
        // only a leaf that passes — clause (i) on its stored box — gathers its triangle (36 / 72 bytes) and turns it into
        // the box's frame
        auto visit = [&](const char *rec) {
            I index;
            T K[9], v[9]; // p1 p2 p3, and their local coordinates v_1 v_2 v_3
            if (pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, K)) {
#pragma unroll
                for (int i = 0; i < 3; ++i) tribox::to_local(q, K + 3 * i, v + 3 * i);
                if (tribox::overlaps(q.h, v)) { // clause (ii) (false on NaN)
                    pointwalk::contact<WRITE>(next, capacity, over, [&](uint64_t row) {
                        if (out_index) out_index[row] = index;
                        if (out_inside) out_inside[row] = (uint8_t)tribox::inside_mask(q.h, v);
                    });
                }
            } else {
                bad = true;
            }
        };
        // a half extent that is not >= 0 and a NaN or an infinity in c or R touch nothing, and a NaN could not prune
        if ((q.h[0] >= T(0)) & (q.h[1] >= T(0)) & (q.h[2] >= T(0)) && !pointwalk::hopeless(q.c, finite))
            pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, []() { return T(0); }, visit);
        pointwalk::store_count<WRITE>(counts, item, next);
    }
    if (bad && flag) raise_flag(flag, 2u);
    if (over && flag) raise_flag(flag, 4u);
}

} // namespace boxes
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_box_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *centers,
                              const void *half_extents, const void *rotations, int64_t num_boxes, int32_t mode, void *counts,
                              const void *offsets, int64_t capacity, void *contact_index, void *contact_inside, void *flag,
                              void *stream) {
    if (!bvh || num_triangles < 0 || num_boxes < 0 || capacity < 0) return IBVH_ERR_INVALID_ARG;
    if (!pointwalk::passes_ok(mode, counts, offsets, contact_index || contact_inside)) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless walk needs boxes that contain the boxes below them exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_boxes == 0 || (centers && half_extents)); // (rotations: optional)
    const ibvh_status st = pointwalk::prepare(bvh, true, num_boxes, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto wt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool WRITE = decltype(wt)::value;
        IBVH_LAUNCH((boxes::boxes_walk_kernel<T, TN, I, WRITE>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0,
                    (hipStream_t)stream, pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay,
                    (const BBox<TN> *)bvh->nodes, (const T *)triangles, num_triangles, (const T *)centers,
                    (const T *)half_extents, (const T *)rotations, num_boxes, (int64_t *)counts, (const int64_t *)offsets,
                    capacity, (I *)contact_index, (uint8_t *)contact_inside, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)pointwalk::dispatch_box_types_and_bool(bvh->types, mode == IBVH_BOXES_WRITE, launch);
}

} // extern "C"
