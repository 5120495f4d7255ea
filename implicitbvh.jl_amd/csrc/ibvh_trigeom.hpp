// ibvh_trigeom.hpp — the box and triangle primitives the mesh queries' contracts are built from (include/ibvh.h fixes every
// operation's order and every comparison's direction), ONE copy each, so that the queries that name the same piece compute
// the same bits: a triangle's exact box, "apart", the squared gap between two boxes, equal and shared vertices, a vertex and
// an edge by selects, a pair's result so far, and "a segment cuts a triangle".  Used by ibvh_tritri.hip, ibvh_boxes.hip,
// ibvh_tridist.hip, ibvh_segtri.hpp (ibvh_capsules.hip, ibvh_segdist.hip) and ibvh_pairwalk.hpp.  The exact test under the
// cut is ibvh_raytest.hpp's.  No reference counterpart: ImplicitBVH.jl's traversals end at pairs of boxes.
#pragma once
#include "ibvh_common.hpp"
#include "ibvh_raytest.hpp"

namespace ibvh {
namespace trigeom {

// a triangle's exact box, folded from its first vertex with `x < m ? x : m` / `x > m ? x : m`
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

// the query's box [qlo, qup] is apart from a box [lo, up]: six strict comparisons, every one false on NaN
template <class T> IBVH_D bool apart(const T *qlo, const T *qup, const T *lo, const T *up) {
    return (qup[0] < lo[0]) | (qlo[0] > up[0]) | (qup[1] < lo[1]) | (qlo[1] > up[1]) | (qup[2] < lo[2]) | (qlo[2] > up[2]);
}

// the squared gap between the query's box [qlo, qup] and a box [lo, up], in d2's operation order: lb(B) of
// ibvh_triangle_distances, the bound the pair distances prune on
template <class T> IBVH_D T box_gap(const T *lo, const T *up, const T *qlo, const T *qup) {
    T g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T below = lo[k] - qup[k], above = qlo[k] - up[k];
        const T m = below > above ? below : above;
        g[k] = m > T(0) ? m : T(0);
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// equal vertices: == on all three coordinates (false on NaN)
template <class T> IBVH_D bool same_vertex(const T *x, const T *y) { return (x[0] == y[0]) & (x[1] == y[1]) & (x[2] == y[2]); }

// IBVH_TRIS_SKIP_SHARED_VERTEX: one of Q's three vertices equals one of K's
template <class T> IBVH_D bool shares_vertex(const T *Q, const T *K) {
    bool shared = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) shared |= same_vertex(Q + 3 * i, K + 3 * j);
    return shared;
}

// c ? a : b on VALUES: both are read before the choice, so the choice is a select of registers.  (A ternary on two array
// elements may become a load through a chosen pointer, which puts both arrays in memory.)
template <class T> IBVH_D T sel(bool c, T a, T b) { return c ? a : b; }

// vertex i (0, 1, 2) of a triangle held in registers, by selects: the callers' candidates stay LOOPS — one copy of each
// routine, one candidate's registers at a time — without an indexable private array
template <class T> IBVH_D void vertex_of(const T *v, int i, T *p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = sel(i == 1, v[3 + k], sel(i == 2, v[6 + k], v[k]));
}

// edge i (0, 1, 2) of such a triangle, p -> q: vertex i -> vertex (i + 1) % 3, each by its own selects on i
template <class T> IBVH_D void edge_of(const T *v, int i, T *p, T *q) {
    vertex_of(v, i, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = sel(i == 0, v[3 + k], sel(i == 1, v[6 + k], v[k]));
}

// a pair's result so far: the squared distance, the point on the query and on the mesh triangle, the rule that decided.
// Candidate 0 starts it (put), a later one replaces it iff its d2 is strictly smaller (offer)
template <class T> struct Pair {
    T d2, xq[3], xk[3];
    int kind;
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

// the segment p0 -> p1 cuts the triangle: the ray test with d = p1 - p0, and t <= 1 (false on NaN); then x = p0 + t * d
template <class T> IBVH_D bool segment_cuts(const raytri::Tri<T> &tri, const T *p0, const T *p1, T *x) {
    const T d[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    T t, u, v;
    if (!(raytri::ray_triangle(tri, p0, d, t, u, v) & (t <= T(1)))) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = p0[k] + t * d[k];
    return true;
}

} // namespace trigeom
} // namespace ibvh
