// ibvh_tridist.hip — for a batch of query triangles, the CLOSEST triangle of the mesh a BVH was built over: which one, how
// far, the two closest points and the pair of features they lie on (include/ibvh.h, ibvh_triangle_distances).  The distance
// query beside ibvh_tritri.hip's "do they touch" and ibvh_sweep.hip's "when": clearance between parts, the gap that sizes a
// contact solver's next step, and, with a mesh as its own queries, self-clearance.  No reference counterpart:
// ImplicitBVH.jl's traversal of two meshes ends at pairs of triangle BOXES; nothing there measures a gap.
//
// A pair (Q, K) is evaluated by two rules.  Cut: if K's exact box is not apart from Q's, the six edge-against-triangle tests
// of ibvh_tritri.hip; the first that hits gives d2 = 0 at its point.  Otherwise the smallest of fifteen candidates, one at
// a time: three vertices of Q against K and three of K against Q (ibvh_pointtri.hpp), nine edge pairs (ibvh_segseg.hpp).
//
// The answer is defined over ALL triangles — the lexicographic minimum of (d2, index) — so the walk only has to be
// lossless.  It is, without an epsilon, in four steps.  (1) Every xQ lies in Q's exact box: a vertex does, a point-triangle
// and a segment-segment point is clamped into its triangle's / segment's box, which lies inside.  (2) Every xK lies in K's
// exact box likewise, which lies in K's leaf box (skin or not) and in every box above it (min / max and widening
// conversions are exact).  (3) The bound of a box [lo, up] is (g0 g0 + g1 g1) + g2 g2 with g_k = max(0, lo_k - qup_k,
// qlo_k - up_k): round-to-nearest subtraction, multiplication and addition are monotone, |xQ_k - xK_k| is computed from
// operands that lie no closer than the two boxes' faces, and d2 adds the squares in the same order, so the COMPUTED bound
// never exceeds a COMPUTED d2 under the box.  (4) A cut pair has boxes that are not apart, so both differences are <= 0 in
// every box above it: its bound is 0, the d2 the cut rule gives.  The definition reads the triangle's own box, not the
// stored one, so leaf boxes with a skin change nothing.
//
// The walk itself — work mapping, near child first, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, the
// gather its leaf_triangle; the boxes, "apart", the bound (box_gap), the shared-vertex skip and the edge test
// (segment_cuts, on ibvh_raytest.hpp's ray_triangle) are ibvh_trigeom.hpp's, the copies ibvh_tritri.hip and
// ibvh_segtri.hpp compute with.  Q, its box, the best pair so far and the trail live in registers; there is no candidate
// list and no buffer besides the outputs: one lane, one query, one launch.
//
// The lane walks twice, by ibvh_pairwalk.hpp's routine: first ibvh_closest.hip's walk from Q's vertex a — the first point
// candidate 0 below is evaluated from, which is what that routine's argument asks of its caller —, then the query's own walk
// from the limit the first one found, not from the radius: an unbounded query then prunes from its first node on.
#include "ibvh_pairwalk.hpp"
#include "ibvh_pointtri.hpp"
#include "ibvh_pointwalk.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_segseg.hpp"
#include "ibvh_trigeom.hpp"

namespace ibvh {
namespace tridist {

using pointwalk::kBlock;
using trigeom::sel;
using trigeom::vertex_of;

constexpr int kCut = 15; // the kind of a pair the cut rule decided

// The evaluation of include/ibvh.h for one pair: Q = a b c with its exact box, K = p1 p2 p3.
template <class T> IBVH_D void evaluate(const raytri::Tri<T> &Q, const T *qlo, const T *qup, const raytri::Tri<T> &K, trigeom::Pair<T> &r) {
    // the cut rule, under the box clause only
    T klo[3], kup[3], x[3], y[3];
    trigeom::triangle_box(K.v, klo, kup);
    const bool apart = trigeom::apart(qlo, qup, klo, kup);
    if (!apart) {
        // test c: the segment p0 -> p1 (c < 3: Q's edge c against K; else K's edge c - 3 against Q); the first hit ends the six
#pragma unroll 1
        for (int c = 0; c < 6; ++c) {
            const bool mine = c < 3;
            const int i = mine ? c : c - 3;
            raytri::Tri<T> tri, from;
            T p0[3], p1[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) tri.v[k] = sel(mine, K.v[k], Q.v[k]), from.v[k] = sel(mine, Q.v[k], K.v[k]);
            trigeom::edge_of(from.v, i, p0, p1);
            if (trigeom::segment_cuts(tri, p0, p1, x)) {
                r.put(T(0), x, x, kCut);
                return;
            }
        }
    }
    // the candidate rule, one at a time.  Candidates 0 - 5: a vertex of one triangle against the other
#pragma unroll 1
    for (int c = 0; c < 6; ++c) {
        const bool mine = c < 3; // Q's vertex against K, else K's against Q
        raytri::Tri<T> tri, from;
#pragma unroll
        for (int k = 0; k < 9; ++k) tri.v[k] = sel(mine, K.v[k], Q.v[k]), from.v[k] = sel(mine, Q.v[k], K.v[k]);
        vertex_of(from.v, mine ? c : c - 3, y);
        int region; // (not part of this query's answer)
        const T d2 = pointtri::closest_on_triangle(tri.v, y, x, region);
        const T xq[3] = {sel(mine, y[0], x[0]), sel(mine, y[1], x[1]), sel(mine, y[2], x[2])};
        const T xk[3] = {sel(mine, x[0], y[0]), sel(mine, x[1], y[1]), sel(mine, x[2], y[2])};
        if (c == 0) r.put(d2, xq, xk, 0);
        else r.offer(d2, xq, xk, c);
    }
    // ... 6 + 3 i + j: edge i of Q against edge j of K
#pragma unroll 1
    for (int c = 0; c < 9; ++c) {
        const int i = c / 3, j = c - 3 * i;
        T p1[3], q1[3], p2[3], q2[3];
        trigeom::edge_of(Q.v, i, p1, q1);
        trigeom::edge_of(K.v, j, p2, q2);
        r.offer(segseg::closest_on_segments(p1, q1, p2, q2, x, y), x, y, 6 + c);
    }
}

// T: the leaves', triangles' and queries' float type; TN: the nodes' (the same or wider — a node box then holds values of T,
// widened exactly, and narrows back exactly)
template <class T, class TN, class I>
__global__ __launch_bounds__(pointwalk::kBlock) void tridist_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ queries, int64_t num_queries, int skip, T max_d2,
    I *__restrict__ out_index, T *__restrict__ out_d2, T *__restrict__ out_xq, T *__restrict__ out_xk,
    uint8_t *__restrict__ out_kind, uint32_t *flag) {
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_queries; item += (int64_t)gridDim.x * kBlock) {
        raytri::Tri<T> Q; // a b c
#pragma unroll
        for (int k = 0; k < 9; ++k) Q.v[k] = queries[9 * item + k];
        T qlo[3], qup[3]; // Q's box: exact
        trigeom::triangle_box(Q.v, qlo, qup);
        // the bound of include/ibvh.h: the squared gap between Q's box and the box, in d2's operation order
        auto box = [&](const T *lo, const T *up) -> T { return trigeom::box_gap(lo, up, qlo, qup); };
        // only a leaf that passes gathers its triangle (36 / 72 bytes); false: it names none, or the skip flag drops it
        auto gather = [&](const char *rec, I &index, raytri::Tri<T> &K) -> bool {
            if (!pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, K.v)) {
                bad = true;
                return false;
            }
            return !((skip & IBVH_TRIS_SKIP_SHARED_VERTEX) && trigeom::shares_vertex(Q.v, K.v));
        };
        auto pair = [&](const raytri::Tri<T> &K, trigeom::Pair<T> &r) { evaluate(Q, qlo, qup, K, r); };
        bool nan = max_d2 != max_d2; // a query with a NaN coordinate or radius has no answer, and a NaN could not prune
#pragma unroll
        for (int k = 0; k < 9; ++k) nan |= !(Q.v[k] == Q.v[k]);
        trigeom::Pair<T> best;
        const I best_index = pairwalk::closest_pair<I>(tree, built_level, leaves, lay, nodes, nan, Q.v, max_d2, box, gather, pair, best);
        pairwalk::store_pair(item, best_index, best, out_index, out_d2, out_xq, out_xk, out_kind);
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace tridist
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_triangle_distances(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *queries,
                                    int64_t num_queries, int32_t skip, const void *max_distance2, void *closest_index,
                                    void *closest_d2, void *point_query, void *point_mesh, void *closest_kind, void *flag,
                                    void *stream) {
    if (!bvh || num_triangles < 0 || num_queries < 0) return IBVH_ERR_INVALID_ARG;
    if (skip & ~IBVH_TRIS_SKIP_SHARED_VERTEX) return IBVH_ERR_INVALID_ARG;
    if (!closest_index && !closest_d2 && !point_query && !point_mesh && !closest_kind) return IBVH_ERR_INVALID_ARG;
    // box leaves: the lossless bound needs boxes all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_queries == 0 || queries);
    const ibvh_status st = pointwalk::prepare(bvh, true, num_queries, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    return (ibvh_status)pointwalk::dispatch_box_types(bvh->types, [&](auto ft, auto nt, auto it) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        IBVH_LAUNCH((tridist::tridist_walk_kernel<T, TN, I>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0, (hipStream_t)stream,
                    pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay, (const BBox<TN> *)bvh->nodes,
                    (const T *)triangles, num_triangles, (const T *)queries, num_queries, (int)skip,
                    pointwalk::radius_or_inf<T>(max_distance2), (I *)closest_index, (T *)closest_d2, (T *)point_query,
                    (T *)point_mesh, (uint8_t *)closest_kind, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    });
}

} // extern "C"
