// ibvh_tritri.hip — for a batch of query triangles, EVERY triangle of the mesh a BVH was built over that the query triangle
// cuts: which ones, which of the six edge-against-triangle tests found it, and the two ends of the cut (include/ibvh.h,
// ibvh_triangle_contacts).  The narrow phase of mesh-vs-mesh contact and, with a mesh as its own queries, of
// self-intersection.  No reference counterpart: ImplicitBVH.jl's traversal of two meshes ends at pairs of triangle BOXES
// (traverse/traverse_pair.jl); nothing there tests a triangle against a triangle.
//
// The lists are defined over ALL triangles — every K whose stored leaf box is not apart from Q's box and that one of the six
// edge tests finds, in leaf order — so the walk only has to be lossless and ordered.  Lossless, without an epsilon: "apart"
// is six strict comparisons of Q's exact box with a box, every box of the tree contains the boxes below it exactly, so a box
// that is apart from Q lies over leaf boxes that are apart from Q, and being apart is part of the definition.  Ordered: the
// walk is handed 0 ("may hold one") or 1 under a constant limit of 0, as in ibvh_spheres.hip and ibvh_crossings.hip: a
// depth-first walk from left to right, whose leaf visits come in ascending leaf position whatever a visit does, so the
// counting pass and the writing pass see the same contacts in the same order.
//
// The walk itself is ibvh_pointwalk.hpp's, the gather its leaf_triangle; Q's box, "apart", the shared-vertex skip and the
// edge test (segment_cuts, on ibvh_raytest.hpp's ray_triangle — the copy ibvh_raytri.hip and ibvh_cast.hip answer with) are
// ibvh_trigeom.hpp's, shared with ibvh_tridist.hip; the rows of the two passes and the entry point's two-pass rule are
// ibvh_pointwalk.hpp's too, shared with ibvh_spheres.hip.  Q, its box and the running row live in registers, the six tests
// name their vertices statically; a contact goes straight from registers to its row.
#include "ibvh_pointwalk.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_trigeom.hpp"

namespace ibvh {
namespace tritri {

using pointwalk::kBlock;

// T: the leaves', triangles' and queries' float type; TN: the nodes' (the same or wider — a node box then holds values of T,
// widened exactly, and narrows back exactly); WRITE: the second pass, which puts contact j of query i in row offsets[i] + j;
// otherwise the first, which only counts them
template <class T, class TN, class I, bool WRITE>
__global__ __launch_bounds__(pointwalk::kBlock) void tritri_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ queries, const I *__restrict__ query_ids,
    int64_t num_queries, int skip, int64_t *__restrict__ counts, const int64_t *__restrict__ offsets, int64_t capacity,
    I *__restrict__ out_index, uint8_t *__restrict__ out_mask, T *__restrict__ out_points, uint32_t *flag) {
    bool bad = false, over = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_queries; item += (int64_t)gridDim.x * kBlock) {
        raytri::Tri<T> Q; // a b c
        bool nan = false;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            Q.v[k] = queries[9 * item + k];
            nan |= !(Q.v[k] == Q.v[k]);
        }
        T qlo[3], qup[3]; // Q's box: exact
        trigeom::triangle_box(Q.v, qlo, qup);
        I qid = 0;
        if (query_ids) qid = query_ids[item];
        uint64_t next = pointwalk::first_row<WRITE>(offsets, item);
        // 0 = the box may hold a contact, 1 = it is apart from Q's (false on NaN: such a box is entered)
        auto box = [&](const T *lo, const T *up) -> T { return trigeom::apart(qlo, qup, lo, up) ? T(1) : T(0); };
        // only a leaf whose box is not apart gathers its triangle (36 / 72 bytes)
        auto visit = [&](const char *rec) {
            I index;
            raytri::Tri<T> K; // p1 p2 p3
            if (!pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, K.v)) {
                bad = true;
                return;
            }
            if (query_ids && !(index > qid)) return;
            if ((skip & IBVH_TRIS_SKIP_SHARED_VERTEX) && trigeom::shares_vertex(Q.v, K.v)) return;
            unsigned mask = 0;
            T first[3], last[3]; // the points of the lowest and the highest set bit
            auto seg = [&](const T *p0, const T *p1, const raytri::Tri<T> &tri, unsigned bit) {
                if (!WRITE && mask != 0) return; // counting needs one set bit, not which: the first hit ends the six
                T x[3];
                if (trigeom::segment_cuts(tri, p0, p1, x)) {
                    if (mask == 0) first[0] = x[0], first[1] = x[1], first[2] = x[2];
                    last[0] = x[0], last[1] = x[1], last[2] = x[2];
                    mask |= bit;
                }
            };
            seg(Q.v, Q.v + 3, K, 1u);      // a -> b against K
            seg(Q.v + 3, Q.v + 6, K, 2u);  // b -> c
            seg(Q.v + 6, Q.v, K, 4u);      // c -> a
            seg(K.v, K.v + 3, Q, 8u);      // p1 -> p2 against Q
            seg(K.v + 3, K.v + 6, Q, 16u); // p2 -> p3
            seg(K.v + 6, K.v, Q, 32u);     // p3 -> p1
            if (mask != 0) {
                pointwalk::contact<WRITE>(next, capacity, over, [&](uint64_t row) {
                    if (out_index) out_index[row] = index;
                    if (out_mask) out_mask[row] = (uint8_t)mask;
                    if (out_points) {
                        out_points[6 * row] = first[0];
                        out_points[6 * row + 1] = first[1];
                        out_points[6 * row + 2] = first[2];
                        out_points[6 * row + 3] = last[0];
                        out_points[6 * row + 4] = last[1];
                        out_points[6 * row + 5] = last[2];
                    }
                });
            }
        };
        // a query with a NaN coordinate touches nothing, and a NaN could not prune
        if (!nan) pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, []() { return T(0); }, visit);
        pointwalk::store_count<WRITE>(counts, item, next);
    }
    if (bad && flag) raise_flag(flag, 2u);
    if (over && flag) raise_flag(flag, 4u);
}

} // namespace tritri
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_triangle_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *queries,
                                   const void *query_ids, int64_t num_queries, int32_t mode, int32_t skip, void *counts,
                                   const void *offsets, int64_t capacity, void *contact_index, void *contact_mask,
                                   void *contact_points, void *flag, void *stream) {
    if (!bvh || num_triangles < 0 || num_queries < 0 || capacity < 0) return IBVH_ERR_INVALID_ARG;
    if (skip & ~IBVH_TRIS_SKIP_SHARED_VERTEX) return IBVH_ERR_INVALID_ARG;
    if (!pointwalk::passes_ok(mode, counts, offsets, contact_index || contact_mask || contact_points)) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless walk needs boxes that contain the boxes below them exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_queries == 0 || queries);
    const ibvh_status st = pointwalk::prepare(bvh, true, num_queries, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto wt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool WRITE = decltype(wt)::value;
        IBVH_LAUNCH((tritri::tritri_walk_kernel<T, TN, I, WRITE>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0,
                    (hipStream_t)stream, pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay,
                    (const BBox<TN> *)bvh->nodes, (const T *)triangles, num_triangles, (const T *)queries,
                    (const I *)query_ids, num_queries, (int)skip, (int64_t *)counts, (const int64_t *)offsets, capacity,
                    (I *)contact_index, (uint8_t *)contact_mask, (T *)contact_points, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)pointwalk::dispatch_box_types_and_bool(bvh->types, mode == IBVH_TRIS_WRITE, launch);
}

} // extern "C"
