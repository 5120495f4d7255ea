// ibvh_spheres.hip — for a batch of spheres, EVERY triangle of the mesh a BVH was built over that lies within the sphere's
// radius of its centre: which ones, how far, where on each and on which feature — vertex, edge or face (include/ibvh.h,
// ibvh_sphere_contacts).  The narrow phase of sphere-vs-mesh contact.  No reference counterpart: ImplicitBVH.jl's traversal
// of spheres against a mesh ends at pairs (sphere, triangle BOX) (traverse/traverse_pair.jl); nothing there tests a triangle.
//
// The lists are defined over ALL triangles — every k with d2(k, c) <= r * r, in leaf order — so the walk only has to be
// lossless and ordered.  Lossless, without an epsilon, by ibvh_closest.hip's argument: the point-box bound is computed by the
// same operations in the same order as the point-triangle distance, the triangle's closest point is clamped into the
// triangle's box, and every box of the tree contains the boxes below it exactly, so the COMPUTED bound of a box never
// exceeds the COMPUTED d2 of a triangle under it: a box with bound > r * r holds no contact.  Ordered: the walk is handed
// 0 ("may hold one") or 1 under a constant limit of 0, as in ibvh_crossings.hip.  Two admitted children then always tie,
// a tie descends to the FIRST child, and a pop takes the deepest owed sibling: a depth-first walk from left to right, whose
// leaf visits come in ascending leaf position.  Nothing in that depends on what a visit does, so the counting pass and the
// writing pass see the same contacts in the same order, and contact j of the one is row j of the other.
//
// The walk itself — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's; the evaluation is
// ibvh_pointtri.hpp's, the copy ibvh_closest.hip answers with; the rows of the two passes and the entry point's two-pass rule
// are ibvh_pointwalk.hpp's too, shared with ibvh_tritri.hip.  Centre, squared radius and the running count live in
// registers; a contact goes straight from registers to its row.
#include "ibvh_pointwalk.hpp"
#include "ibvh_pointtri.hpp"

namespace ibvh {
namespace spheres {

using pointwalk::kBlock;

// T: the leaves', triangles' and spheres' float type; TN: the nodes' (the same or wider — a node box then holds values of
// T, widened exactly, and narrows back exactly); WRITE: the second pass, which puts contact j of sphere s in row
// offsets[s] + j; otherwise the first, which only counts them
template <class T, class TN, class I, bool WRITE>
__global__ __launch_bounds__(pointwalk::kBlock) void spheres_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ centers, const T *__restrict__ radii,
    int64_t num_spheres, int64_t *__restrict__ counts, const int64_t *__restrict__ offsets, int64_t capacity,
    I *__restrict__ out_index, T *__restrict__ out_d2, T *__restrict__ out_q, uint8_t *__restrict__ out_region, uint32_t *flag) {
    bool bad = false, over = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_spheres; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {centers[3 * item], centers[3 * item + 1], centers[3 * item + 2]};
        const T r = radii[item];
        const T r2 = r * r;
        uint64_t next = pointwalk::first_row<WRITE>(offsets, item);
        // 0 = the box may hold a contact, 1 = it cannot (false on NaN: such a box is entered)
        auto box = [&](const T *lo, const T *up) -> T { return pointwalk::box_bound(lo, up, p) > r2 ? T(1) : T(0); };
        // only a leaf that passes gathers its triangle (36 / 72 bytes)
        auto visit = [&](const char *rec) {
            I index;
            T tr[9], q[3];
            int region;
            if (pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, tr)) {
                const T d2 = pointtri::closest_on_triangle(tr, p, q, region);
                if (d2 <= r2) { // (false on NaN)
                    pointwalk::contact<WRITE>(next, capacity, over, [&](uint64_t row) {
                        if (out_index) out_index[row] = index;
                        if (out_d2) out_d2[row] = d2;
                        if (out_q) {
                            out_q[3 * row] = q[0];
                            out_q[3 * row + 1] = q[1];
                            out_q[3 * row + 2] = q[2];
                        }
                        if (out_region) out_region[row] = (uint8_t)region;
                    });
                }
            } else {
                bad = true;
            }
        };
        // a negative or NaN radius and a NaN centre touch nothing, and a NaN could not prune
        if ((r >= T(0)) && !pointwalk::hopeless(p, r2))
            pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, []() { return T(0); }, visit);
        pointwalk::store_count<WRITE>(counts, item, next);
    }
    if (bad && flag) raise_flag(flag, 2u);
    if (over && flag) raise_flag(flag, 4u);
}

} // namespace spheres
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_sphere_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *centers,
                                 const void *radii, int64_t num_spheres, int32_t mode, void *counts, const void *offsets,
                                 int64_t capacity, void *contact_index, void *contact_d2, void *contact_point,
                                 void *contact_region, void *flag, void *stream) {
    if (!bvh || num_triangles < 0 || num_spheres < 0 || capacity < 0) return IBVH_ERR_INVALID_ARG;
    if (!pointwalk::passes_ok(mode, counts, offsets, contact_index || contact_d2 || contact_point || contact_region)) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless bound needs boxes that contain their triangles' boxes exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_spheres == 0 || (centers && radii));
    const ibvh_status st = pointwalk::prepare(bvh, true, num_spheres, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto wt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool WRITE = decltype(wt)::value;
        IBVH_LAUNCH((spheres::spheres_walk_kernel<T, TN, I, WRITE>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0,
                    (hipStream_t)stream, pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay,
                    (const BBox<TN> *)bvh->nodes, (const T *)triangles, num_triangles, (const T *)centers, (const T *)radii,
                    num_spheres, (int64_t *)counts, (const int64_t *)offsets, capacity, (I *)contact_index, (T *)contact_d2,
                    (T *)contact_point, (uint8_t *)contact_region, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)pointwalk::dispatch_box_types_and_bool(bvh->types, mode == IBVH_SPHERES_WRITE, launch);
}

} // extern "C"
