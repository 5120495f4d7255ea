// ibvh_pointtri.hpp — the point-triangle evaluation of include/ibvh.h (ibvh_closest_triangles): the closest point q of a
// triangle to a point p, the squared distance, and which branch of the region walk decided.  ONE copy, so that the queries
// that answer with it — ibvh_closest.hip (the closest triangle), ibvh_spheres.hip (every triangle within a radius),
// ibvh_sweep.hip (a moving sphere's start position), ibvh_tridist.hip (a vertex against a triangle) and ibvh_segtri.hpp (a
// segment's end against a triangle) — compute the same bits.  No reference counterpart: ImplicitBVH.jl has no point-triangle distance.
#pragma once
#include "ibvh_common.hpp"

namespace ibvh {
namespace pointtri {

template <class T> IBVH_D T dot3(const T *x, const T *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// Ericson's region walk (Real-Time Collision Detection 5.1.5), the first matching case decides; then q is clamped into the
// triangle's exact box.  -ffp-contract=off: every operation is rounded once.  region: the number of the deciding case —
// 0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 face (a caller that ignores it pays nothing).
template <class T> IBVH_D T closest_on_triangle(const T *tr, const T *p, T *q, int &region) {
    const T *a = tr, *b = tr + 3, *c = tr + 6;
    const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const T ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const T ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const T d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    const T bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const T d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    const T cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const T d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const T vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if ((d1 <= T(0)) & (d2 <= T(0))) {
        region = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k];
    } else if ((d3 >= T(0)) & (d4 <= d3)) {
        region = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k];
    } else if ((vc <= T(0)) & (d1 >= T(0)) & (d3 <= T(0))) {
        region = 2;
        const T v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k];
    } else if ((d6 >= T(0)) & (d5 <= d6)) {
        region = 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = c[k];
    } else if ((vb <= T(0)) & (d2 >= T(0)) & (d6 <= T(0))) {
        region = 4;
        const T w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k];
    } else if ((va <= T(0)) & ((d4 - d3) >= T(0)) & ((d5 - d6) >= T(0))) {
        region = 5;
        const T w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k] + w * (c[k] - b[k]);
    } else {
        region = 6;
        const T den = T(1) / ((va + vb) + vc);
        const T v = vb * den, w = vc * den;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (a[k] + v * ab[k]) + w * ac[k];
    }
    T e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T lo = minimum3(a[k], b[k], c[k]), up = maximum3(a[k], b[k], c[k]); // bbox_from_triangle
        q[k] = q[k] < lo ? lo : (q[k] > up ? up : q[k]);                            // (NaN stays NaN)
        e[k] = p[k] - q[k];
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

} // namespace pointtri
} // namespace ibvh
