// ibvh_segseg.hpp — the segment-segment evaluation of include/ibvh.h (ibvh_triangle_distances): the closest points x1 of the
// segment p1 -> q1 and x2 of the segment p2 -> q2, and their squared distance.  ONE copy, beside ibvh_pointtri.hpp, so that
// whatever answers with it — ibvh_tridist.hip, and ibvh_segtri.hpp for ibvh_capsules.hip and ibvh_segdist.hip — computes the
// same bits.  No reference counterpart: ImplicitBVH.jl has no segment distance.
#pragma once
#include "ibvh_common.hpp"
#include "ibvh_pointtri.hpp"

namespace ibvh {
namespace segseg {

using pointtri::dot3;

// x clamped into [0, 1] (NaN stays NaN)
template <class T> IBVH_D T unit(T x) { return x < T(0) ? T(0) : (x > T(1) ? T(1) : x); }

// Ericson's clamped computation (Real-Time Collision Detection 5.1.9), with exact tests for a segment of length zero and for
// parallel segments (a determinant that is not positive) and no epsilon; then each point is clamped componentwise into its own
// segment's box.  -ffp-contract=off: every operation is rounded once.  Returns (e0 e0 + e1 e1) + e2 e2 with e = x1 - x2.
template <class T> IBVH_D T closest_on_segments(const T *p1, const T *q1, const T *p2, const T *q2, T *x1, T *x2) {
    const T d1[3] = {q1[0] - p1[0], q1[1] - p1[1], q1[2] - p1[2]};
    const T d2[3] = {q2[0] - p2[0], q2[1] - p2[1], q2[2] - p2[2]};
    const T r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
    const T a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r);
    T s = T(0), t = T(0);
    if (a == T(0)) {
        if (e != T(0)) t = unit(f / e); // the first segment is a point; both: s = t = 0
    } else {
        const T c = dot3(d1, r);
        if (e == T(0)) {
            s = unit(-c / a); // the second segment is a point
        } else {
            const T b = dot3(d1, d2);
            const T den = a * e - b * b;
            if (den > T(0)) s = unit((b * f - c * e) / den); // parallel (or rounded so): any s will do, 0 is taken
            t = (b * s + f) / e;
            if (t < T(0)) {
                t = T(0);
                s = unit(-c / a);
            } else if (t > T(1)) {
                t = T(1);
                s = unit((b - c) / a);
            }
        }
    }
    T g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T y1 = p1[k] + s * d1[k], y2 = p2[k] + t * d2[k];
        const T lo1 = minimum2(p1[k], q1[k]), up1 = maximum2(p1[k], q1[k]);
        const T lo2 = minimum2(p2[k], q2[k]), up2 = maximum2(p2[k], q2[k]);
        x1[k] = y1 < lo1 ? lo1 : (y1 > up1 ? up1 : y1); // (NaN stays NaN)
        x2[k] = y2 < lo2 ? lo2 : (y2 > up2 ? up2 : y2);
        g[k] = x1[k] - x2[k];
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

} // namespace segseg
} // namespace ibvh
