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
// gather its leaf_triangle, the edge test ibvh_raytest.hpp's ray_triangle.  Q, its box, the best pair so far and the trail
// live in registers; there is no candidate list and no buffer besides the outputs: one lane, one query, one launch.
//
// The lane walks twice.  First ibvh_closest.hip's walk from Q's vertex a: the squared distance to the closest triangle the
// query may answer with is candidate 0 of that pair, so no answer lies beyond it, and the second walk — the query's own —
// starts from that limit, not from the radius: an unbounded query then prunes from its first node on.
#include "ibvh_pointwalk.hpp"
#include "ibvh_pointtri.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_segseg.hpp"

#include <limits>

namespace ibvh {
namespace tridist {

using pointwalk::kBlock;

constexpr int kCut = 15; // the kind of a pair the cut rule decided

// equal vertices: == on all three coordinates (false on NaN)
template <class T> IBVH_D bool same_vertex(const T *x, const T *y) { return (x[0] == y[0]) & (x[1] == y[1]) & (x[2] == y[2]); }

// a triangle's exact box, folded from its first vertex with `x < m ? x : m` / `x > m ? x : m`
template <class T> IBVH_D void fold_box(const T *v, T *lo, T *up) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T l = v[k], u = v[k];
        l = v[3 + k] < l ? v[3 + k] : l;
        u = v[3 + k] > u ? v[3 + k] : u;
        l = v[6 + k] < l ? v[6 + k] : l;
        u = v[6 + k] > u ? v[6 + k] : u;
        lo[k] = l;
        up[k] = u;
    }
}

// the pair's result so far: candidate 0 starts it, a later one replaces it iff its d2 is strictly smaller
template <class T> struct Pair {
    T d2, xq[3], xk[3];
    int kind;
    IBVH_D void start(T d, const T *q, const T *k) { put(d, q, k, 0); }
    IBVH_D void offer(T d, const T *q, const T *k, int c) {
        if (d < d2) put(d, q, k, c);
    }
    IBVH_D void put(T d, const T *q, const T *k, int c) {
        d2 = d;
        kind = c;
#pragma unroll
        for (int j = 0; j < 3; ++j) xq[j] = q[j], xk[j] = k[j];
    }
};

// c ? a : b on VALUES: both are read before the choice, so the choice is a select of registers.  (A ternary on two array
// elements may become a load through a chosen pointer, which puts both arrays in memory.)
template <class T> IBVH_D T sel(bool c, T a, T b) { return c ? a : b; }

// vertex i (0, 1, 2) of a triangle held in registers, by selects: the candidates below stay LOOPS — one copy of each
// routine, one candidate's registers at a time — without an indexable private array
template <class T> IBVH_D void vertex_of(const T *v, int i, T *p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = sel(i == 1, v[3 + k], sel(i == 2, v[6 + k], v[k]));
}

// The evaluation of include/ibvh.h for one pair: Q = a b c with its exact box, K = p1 p2 p3.
template <class T> IBVH_D void evaluate(const raytri::Tri<T> &Q, const T *qlo, const T *qup, const raytri::Tri<T> &K, Pair<T> &r) {
    // the cut rule, under the box clause only
    T klo[3], kup[3];
    fold_box(K.v, klo, kup);
    const bool apart = (qup[0] < klo[0]) | (qlo[0] > kup[0]) | (qup[1] < klo[1]) | (qlo[1] > kup[1]) | (qup[2] < klo[2]) | (qlo[2] > kup[2]);
    if (!apart) {
        // test c: the segment p0 -> p1 (c < 3: Q's edge c against K; else K's edge c - 3 against Q), which is the ray test with
        // d = p1 - p0, and t <= 1; the first hit ends the six
#pragma unroll 1
        for (int c = 0; c < 6; ++c) {
            const bool mine = c < 3;
            const int i = mine ? c : c - 3;
            raytri::Tri<T> tri, from;
            T p0[3], p1[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) tri.v[k] = sel(mine, K.v[k], Q.v[k]), from.v[k] = sel(mine, Q.v[k], K.v[k]);
            vertex_of(from.v, i, p0);
            vertex_of(from.v, i == 2 ? 0 : i + 1, p1);
            const T d[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
            T t, u, v;
            if (raytri::ray_triangle(tri, p0, d, t, u, v) & (t <= T(1))) {
                const T x[3] = {p0[0] + t * d[0], p0[1] + t * d[1], p0[2] + t * d[2]};
                r.put(T(0), x, x, kCut);
                return;
            }
        }
    }
    // the candidate rule, one at a time.  Candidates 0 - 5: a vertex of one triangle against the other
    T x[3], y[3];
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
        if (c == 0) r.start(d2, xq, xk);
        else r.offer(d2, xq, xk, c);
    }
    // ... 6 + 3 i + j: edge i of Q against edge j of K
#pragma unroll 1
    for (int c = 0; c < 9; ++c) {
        const int i = c / 3, j = c - 3 * i;
        T p1[3], q1[3], p2[3], q2[3];
        vertex_of(Q.v, i, p1);
        vertex_of(Q.v, i == 2 ? 0 : i + 1, q1);
        vertex_of(K.v, j, p2);
        vertex_of(K.v, j == 2 ? 0 : j + 1, q2);
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
        fold_box(Q.v, qlo, qup);
        Pair<T> best; // best.d2 is the limit: it starts at the radius, or at the first limit below
        const T zero[3] = {T(0), T(0), T(0)};
        best.put(max_d2, zero, zero, 0);
        I best_index = 0;
        // the bound of include/ibvh.h: the squared gap between Q's box and the box, in d2's operation order
        auto box = [&](const T *lo, const T *up) -> T {
            T g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const T below = lo[k] - qup[k], above = qlo[k] - up[k];
                const T m = below > above ? below : above;
                g[k] = m > T(0) ? m : T(0);
            }
            return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        };
        // only a leaf that passes gathers its triangle (36 / 72 bytes); false: it names none, or the skip flag drops it
        auto gather = [&](const char *rec, I &index, raytri::Tri<T> &K) -> bool {
            if (!pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, K.v)) {
                bad = true;
                return false;
            }
            bool shared = false;
            if (skip & IBVH_TRIS_SKIP_SHARED_VERTEX) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) shared |= same_vertex(Q.v + 3 * i, K.v + 3 * j);
            }
            return !shared;
        };
        auto visit = [&](const char *rec) {
            I index;
            raytri::Tri<T> K; // p1 p2 p3
            if (!gather(rec, index, K)) return;
            Pair<T> r;
            evaluate(Q, qlo, qup, K, r);
            // (d2, index) lexicographically; the first one only has to be within the limit it starts from (best_index == 0)
            if ((r.d2 < best.d2) | ((r.d2 == best.d2) & ((best_index == 0) | (index < best_index)))) {
                best = r;
                best_index = index;
            }
        };
        bool nan = false; // a query with a NaN coordinate has no answer, and a NaN could not prune
#pragma unroll
        for (int k = 0; k < 9; ++k) nan |= !(Q.v[k] == Q.v[k]);
        if (!nan && max_d2 == max_d2) {
            // A first limit, so that an unbounded query does not start blind: the squared distance from Q's vertex a to the
            // closest triangle S the query may answer with, by ibvh_closest.hip's walk (a fifteenth of a pair per visit).  That
            // value IS candidate 0 of the pair (Q, S), bit for bit, so that pair's d2 cannot exceed it and the answer's neither:
            // nothing beyond it can win or tie, and S itself is still reached (its bounds do not exceed its d2).
            T seed = max_d2;
            auto near_a = [&](const char *rec) {
                I index;
                raytri::Tri<T> K;
                T x[3];
                int region;
                if (!gather(rec, index, K)) return;
                const T d2 = pointtri::closest_on_triangle(K.v, Q.v, x, region);
                seed = d2 < seed ? d2 : seed;
            };
            auto box_a = [&](const T *lo, const T *up) { return pointwalk::box_bound(lo, up, Q.v); };
            pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box_a, [&]() { return seed; }, near_a);
            best.d2 = seed;
            pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box, [&]() { return best.d2; }, visit);
        }
        const bool hit = best_index != 0;
        if (out_index) out_index[item] = best_index;
        if (out_d2) out_d2[item] = hit ? best.d2 : std::numeric_limits<T>::infinity();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (out_xq) out_xq[3 * item + k] = hit ? best.xq[k] : T(0);
            if (out_xk) out_xk[3 * item + k] = hit ? best.xk[k] : T(0);
        }
        if (out_kind) out_kind[item] = hit ? (uint8_t)best.kind : (uint8_t)0;
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
