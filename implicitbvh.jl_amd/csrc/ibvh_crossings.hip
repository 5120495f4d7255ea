// ibvh_crossings.hip — for a batch of query points, the triangles of the mesh a BVH was built over which the axis ray
// P + t*e_a, t > 0, crosses: how many, and the signed sum of their orientations (include/ibvh.h, ibvh_point_crossings): the
// side of a closed surface a point lies on.  No reference counterpart: every traversal of ImplicitBVH.jl is a fixed-volume
// overlap test (traverse/, raytrace/), and its ray test has no rule for a ray through a shared edge or vertex.
//
// Both counts are defined over ALL triangles, so the walk only has to be lossless.  It is, without an epsilon: a triangle
// can only be a crossing if the guard — five comparisons of the point against the triangle's box — holds, a box of the tree
// (a node, or a leaf's stored volume) is entered iff the same five comparisons hold on the box, and every box of the tree
// contains the boxes below it exactly (min / max, widening conversions, a skin margin, ibvh_refit): a triangle whose own
// box passes the guard has every box above it pass.  Nothing is rounded on the way: comparisons only.
//
// Watertight by construction: the edge function of an edge is evaluated on the edge's CANONICAL orientation (endpoints in
// lexicographic order), so the two triangles that share an edge compute the same bits and put the point on the same side of
// it; a tie goes left of the canonical edge for both.
//
// The walk itself — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, here with a bound that
// is 0 where the guard holds on the box and 1 where it does not, under a limit of 0.  The axis is a run-time argument,
// applied once as a coordinate permutation where values are loaded: compile-time slots picked by compares, never an
// indexed private array.
#include "ibvh_pointwalk.hpp"

namespace ibvh {
namespace crossings {

using pointwalk::kBlock;

// x[i], i in 0..2, of an array held in registers: two selects, nothing indexed at run time
template <class T> IBVH_D T pick(const T *x, int i) { return i == 0 ? x[0] : (i == 1 ? x[1] : x[2]); }

// side of p (u, v) of the directed edge x -> y (u, v, w): the edge function on the canonical pair, a tie goes LEFT of the
// canonical edge, the answer is turned back for an edge that was flipped
template <class T> IBVH_D bool edge_side(const T *x, const T *y, const T *p) {
    const bool flipped = (y[0] < x[0]) | ((y[0] == x[0]) & ((y[1] < x[1]) | ((y[1] == x[1]) & (y[2] < x[2]))));
    const T x0 = flipped ? y[0] : x[0], x1 = flipped ? y[1] : x[1];
    const T y0 = flipped ? x[0] : y[0], y1 = flipped ? x[1] : y[1];
    const T e = (y0 - x0) * (p[1] - x1) - (y1 - x1) * (p[0] - x0);
    return (e >= T(0)) != flipped;
}

// rules 1 to 4 of include/ibvh.h on a triangle and a point already in (u, v, w): +1 a ccw crossing, -1 a cw one, 0 none.
// -ffp-contract=off: every operation is rounded once.
template <class T> IBVH_D int crossing(const T *a, const T *b, const T *c, const T *p) {
    const T lo0 = minimum3(a[0], b[0], c[0]), up0 = maximum3(a[0], b[0], c[0]); // bbox_from_triangle
    const T lo1 = minimum3(a[1], b[1], c[1]), up1 = maximum3(a[1], b[1], c[1]);
    const T up2 = maximum3(a[2], b[2], c[2]);
    if (!((p[0] >= lo0) & (p[0] <= up0) & (p[1] >= lo1) & (p[1] <= up1) & (up2 >= p[2]))) return 0;
    const bool s0 = edge_side(a, b, p), s1 = edge_side(b, c, p), s2 = edge_side(c, a, p); // (unrolled by hand)
    const bool ccw = s0 & s1 & s2, cw = !(s0 | s1 | s2);
    const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const T ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const T d[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const T n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
    const T s = (n0 * d[0] + n1 * d[1]) + n2 * d[2];
    return (ccw & (s < T(0))) ? 1 : ((cw & (s > T(0))) ? -1 : 0);
}

// T: the leaves' and triangles' float type; TN: the nodes' (the same or wider — a node box then holds values of T, widened
// exactly, and narrows back exactly); u, v, w: the cyclic coordinates (axis + 1) % 3, (axis + 2) % 3, axis
template <class T, class TN, class I>
__global__ __launch_bounds__(kBlock) void crossings_walk_kernel(TreeDev tree, int built_level, const char *__restrict__ leaves,
                                                                LeafLayout lay, const BBox<TN> *__restrict__ nodes,
                                                                const T *__restrict__ tris, int64_t num_triangles,
                                                                const T *__restrict__ points, int64_t num_points, int u, int v,
                                                                int w, I *__restrict__ out_crossings, I *__restrict__ out_winding,
                                                                uint32_t *flag) {
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_points; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {points[3 * item + u], points[3 * item + v], points[3 * item + w]};
        I count = 0, winding = 0;
        // the guard on a box: 0 = the ray can meet it, 1 = it cannot (false on NaN: a NaN point enters nothing)
        auto box = [&](const T *lo, const T *up) -> T {
            const T lo0 = pick(lo, u), up0 = pick(up, u), lo1 = pick(lo, v), up1 = pick(up, v), up2 = pick(up, w);
            return ((p[0] >= lo0) & (p[0] <= up0) & (p[1] >= lo1) & (p[1] <= up1) & (up2 >= p[2])) ? T(0) : T(1);
        };
        // only a leaf that passes gathers its triangle (36 / 72 bytes).  The statements of pointwalk::leaf_triangle, spelled out:
        // behind the helper's return value the compiler joins the two paths ahead of the axis selects below, the nine values
        // cross the join, and the kernel comes out 1 % longer and waits on its loads one by one
        auto visit = [&](const char *rec) {
            const I index = load_index<I>(rec, lay);
            if (index >= 1 && (int64_t)index <= num_triangles) {
                T tr[9];
                __builtin_memcpy(tr, __builtin_assume_aligned(tris + 9 * ((int64_t)index - 1), sizeof(T)), sizeof(tr));
                const T a[3] = {pick(tr, u), pick(tr, v), pick(tr, w)};
                const T b[3] = {pick(tr + 3, u), pick(tr + 3, v), pick(tr + 3, w)};
                const T c[3] = {pick(tr + 6, u), pick(tr + 6, v), pick(tr + 6, w)};
                const int x = crossing(a, b, c, p);
                count += I(x != 0);
                winding += I(x);
            } else {
                bad = true;
            }
        };
        pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, []() { return T(0); }, visit);
        if (out_crossings) out_crossings[item] = count;
        if (out_winding) out_winding[item] = winding;
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace crossings
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_point_crossings(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *points,
                                 int64_t num_points, int32_t axis, void *crossings, void *winding, void *flag, void *stream) {
    if (!bvh || num_triangles < 0 || num_points < 0 || axis < 0 || axis > 2) return IBVH_ERR_INVALID_ARG;
    if (!crossings && !winding) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless guard needs boxes that contain their triangles exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_points == 0 || points);
    const ibvh_status st = pointwalk::prepare(bvh, true, num_points, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    const int u = (axis + 1) % 3, v = (axis + 2) % 3, w = axis; // cyclic: orientation is preserved
    return (ibvh_status)pointwalk::dispatch_box_types(bvh->types, [&](auto ft, auto nt, auto it) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        IBVH_LAUNCH((crossings::crossings_walk_kernel<T, TN, I>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0,
                    (hipStream_t)stream, pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay,
                    (const BBox<TN> *)bvh->nodes, (const T *)triangles, num_triangles, (const T *)points, num_points, u, v, w,
                    (I *)crossings, (I *)winding, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    });
}

} // extern "C"
