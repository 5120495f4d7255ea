// ibvh_segtri.hpp — the segment-triangle evaluation of include/ibvh.h (ibvh_capsule_contacts): the closest points xs of the
// segment S = a -> b and xk of the triangle K = p1 p2 p3, their squared distance, and which of six rules decided.  ONE copy
// for the two queries that answer with it — ibvh_capsules.hip (every triangle within a capsule's radius of its segment) and
// ibvh_segdist.hip (the closest triangle per segment) — so that both compute the same bits.  It is built from the pieces
// the tree already has one copy of: ibvh_raytest.hpp's exact test (the cut rule), ibvh_pointtri.hpp's point-triangle
// evaluation (the two ends) and ibvh_segseg.hpp's segment-segment evaluation (the three edges).  No reference counterpart:
// ImplicitBVH.jl has no segment distance and no exact triangle test.
//
// The triangle's feature under xk is NOT reported: ibvh_segseg.hpp does not classify where on an edge its point lies (an end
// or the inside), so a feature code could only be given for the kinds 0 and 1, and is given for none.
#pragma once
#include "ibvh_common.hpp"
#include "ibvh_pointtri.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_segseg.hpp"

namespace ibvh {
namespace segtri {

constexpr int kCut = 5; // the kind of a pair the cut rule decided

// the pair's result so far: candidate 0 starts it, a later one replaces it iff its d2 is strictly smaller
template <class T> struct Pair {
    T d2, xs[3], xk[3];
    int kind;
    IBVH_D void offer(T d, const T *s, const T *k, int c) {
        if (d < d2) put(d, s, k, c);
    }
    IBVH_D void put(T d, const T *s, const T *k, int c) {
        d2 = d;
        kind = c;
#pragma unroll
        for (int j = 0; j < 3; ++j) xs[j] = s[j], xk[j] = k[j];
    }
};

// c ? a : b on VALUES: both are read before the choice, so the choice is a select of registers, never a load through a
// chosen pointer (which would put both arrays in memory)
template <class T> IBVH_D T sel(bool c, T a, T b) { return c ? a : b; }

// S's exact box: [min(a, b), max(a, b)] per component by `x < y ? x : y` / `x > y ? x : y`
template <class T> IBVH_D void segment_box(const T *a, const T *b, T *lo, T *up) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = a[k] < b[k] ? a[k] : b[k];
        up[k] = a[k] > b[k] ? a[k] : b[k];
    }
}

// K's exact box, folded from its first vertex with `x < m ? x : m` / `x > m ? x : m` (ibvh_tridist.hip's fold)
template <class T> IBVH_D void triangle_box(const T *v, T *lo, T *up) {
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

// the squared gap between S's box [slo, sup] and a box [lo, up], in d2's operation order: the bound both queries prune on
// (ibvh_triangle_distances' lb(B) with S's box in place of Q's)
template <class T> IBVH_D T box_gap(const T *lo, const T *up, const T *slo, const T *sup) {
    T g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T below = lo[k] - sup[k], above = slo[k] - up[k];
        const T m = below > above ? below : above;
        g[k] = m > T(0) ? m : T(0);
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// The evaluation of include/ibvh.h for one pair: S = a -> b with its exact box, K = p1 p2 p3.
template <class T> IBVH_D void evaluate(const T *a, const T *b, const T *slo, const T *sup, const raytri::Tri<T> &K, Pair<T> &r) {
    // the cut rule, under the box clause only: the segment is the ray a + t (b - a), t <= 1
    T klo[3], kup[3];
    triangle_box(K.v, klo, kup);
    const bool apart = (sup[0] < klo[0]) | (slo[0] > kup[0]) | (sup[1] < klo[1]) | (slo[1] > kup[1]) | (sup[2] < klo[2]) | (slo[2] > kup[2]);
    if (!apart) {
        const T d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        T t, u, v;
        if (raytri::ray_triangle(K, a, d, t, u, v) & (t <= T(1))) {
            const T x[3] = {a[0] + t * d[0], a[1] + t * d[1], a[2] + t * d[2]};
            r.put(T(0), x, x, kCut);
            return;
        }
    }
    // the candidate rule, one at a time.  Candidates 0, 1: an end of S against K
    T x[3], y[3];
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const T p[3] = {sel(c == 0, a[0], b[0]), sel(c == 0, a[1], b[1]), sel(c == 0, a[2], b[2])};
        int region; // (not part of these queries' answer)
        const T d2 = pointtri::closest_on_triangle(K.v, p, x, region);
        if (c == 0) r.put(d2, p, x, 0);
        else r.offer(d2, p, x, 1);
    }
    // ... 2, 3, 4: S against K's edges p1p2, p2p3, p3p1 (vertex i by selects: no indexable private array)
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        T p2[3], q2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p2[k] = sel(c == 1, K.v[3 + k], sel(c == 2, K.v[6 + k], K.v[k]));
            q2[k] = sel(c == 0, K.v[3 + k], sel(c == 1, K.v[6 + k], K.v[k]));
        }
        r.offer(segseg::closest_on_segments(a, b, p2, q2, x, y), x, y, 2 + c);
    }
}

} // namespace segtri
} // namespace ibvh
