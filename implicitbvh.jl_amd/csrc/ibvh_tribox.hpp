// ibvh_tribox.hpp — the exact triangle-box test of include/ibvh.h (ibvh_box_contacts): does the triangle K = p1 p2 p3 overlap
// the oriented box of centre c, half extents h and axes u_0 u_1 u_2 (the rows of R)?  The separating-axis test on 13 axes
// (Akenine-Möller, "Fast 3D Triangle-Box Overlap Testing", 2001) in the box's own frame, where the box is [-h, h]: its three
// axes, the triangle's normal, and the nine cross products of a box axis with a triangle edge.  ONE copy, so that a later
// query answers with the same bits as ibvh_boxes.hip (every triangle a box overlaps).  No reference counterpart:
// ImplicitBVH.jl tests boxes against boxes and spheres, never a triangle.
//
// Every operation is rounded once and written in the order the header states; every comparison is false on NaN, touching
// counts as overlapping (<= / >=), and nothing here divides.  For a triangle of zero area the normal and some cross
// products are 0: those axes separate nothing (0 <= 0), so the test is conservative there — it may report, it never loses.
#pragma once
#include "ibvh_common.hpp"

namespace ibvh {
namespace tribox {

IBVH_D float mag(float x) { return __builtin_fabsf(x); }
IBVH_D double mag(double x) { return __builtin_fabs(x); }

// the query: centre, half extents, and the rotation's nine values row-major (row k = the box's axis u_k in world coordinates)
template <class T> struct Box {
    T c[3], h[3], u[9];
};

// the HULL of the box: c_k -+ e_k with e_k = ((|R_0k| * h_0 + |R_1k| * h_1) + |R_2k| * h_2)
template <class T> IBVH_D void hull(const Box<T> &b, T *lo, T *up) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T e = (mag(b.u[k]) * b.h[0] + mag(b.u[3 + k]) * b.h[1]) + mag(b.u[6 + k]) * b.h[2];
        lo[k] = b.c[k] - e;
        up[k] = b.c[k] + e;
    }
}

// the local coordinates of the world point p: v_k = ((u_k0 * w_0 + u_k1 * w_1) + u_k2 * w_2) with w = p - c
template <class T> IBVH_D void to_local(const Box<T> &b, const T *p, T *v) {
    const T w[3] = {p[0] - b.c[0], p[1] - b.c[1], p[2] - b.c[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (b.u[3 * k] * w[0] + b.u[3 * k + 1] * w[1]) + b.u[3 * k + 2] * w[2];
}

// the three projections p1 p2 p3 of the triangle on an axis, folded from the first with `x < m ? x : m` / `x > m ? x : m`,
// against the box's [-rad, rad]: overlapping iff min <= rad and max >= -rad
template <class T> IBVH_D bool axis_overlaps(T p1, T p2, T p3, T rad) {
    T mn = p1, mx = p1;
    mn = p2 < mn ? p2 : mn;
    mx = p2 > mx ? p2 : mx;
    mn = p3 < mn ? p3 : mn;
    mx = p3 > mx ? p3 : mx;
    return (mn <= rad) & (mx >= -rad);
}

// The SAT clause on the local vertices v = v_1 v_2 v_3 (nine values): true iff none of the 13 axes separates.  The cheap
// axes first; each family ends the test as soon as it separates (the answer is the AND of all 13 whatever the order).
template <class T> IBVH_D bool overlaps(const T *h, const T *v) {
    // the three box axes
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok &= axis_overlaps(v[k], v[3 + k], v[6 + k], h[k]);
    if (!ok) return false;
    // the edges e_0 = v_2 - v_1, e_1 = v_3 - v_2, e_2 = v_1 - v_3
    const T e[9] = {v[3] - v[0], v[4] - v[1], v[5] - v[2], v[6] - v[3], v[7] - v[4], v[8] - v[5], v[0] - v[6], v[1] - v[7], v[2] - v[8]};
    // the normal n = e_0 x e_1: d = ((n_0 * v_10 + n_1 * v_11) + n_2 * v_12), rad = ((|n_0| * h_0 + |n_1| * h_1) + |n_2| * h_2)
    const T n[3] = {e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]};
    const T d = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2];
    const T rad = (mag(n[0]) * h[0] + mag(n[1]) * h[1]) + mag(n[2]) * h[2];
    if (!((d <= rad) & (d >= -rad))) return false;
    // the nine axes a = axis_k x e_j, by their two non-zero components: p_i = a . v_i, rad = |a| . h
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const T ex = e[3 * j], ey = e[3 * j + 1], ez = e[3 * j + 2];
        // axis_0 x e_j = (0, -ez, ey)
        ok &= axis_overlaps(ey * v[2] - ez * v[1], ey * v[5] - ez * v[4], ey * v[8] - ez * v[7], mag(ez) * h[1] + mag(ey) * h[2]);
        // axis_1 x e_j = (ez, 0, -ex)
        ok &= axis_overlaps(ez * v[0] - ex * v[2], ez * v[3] - ex * v[5], ez * v[6] - ex * v[8], mag(ez) * h[0] + mag(ex) * h[2]);
        // axis_2 x e_j = (-ey, ex, 0)
        ok &= axis_overlaps(ex * v[1] - ey * v[0], ex * v[4] - ey * v[3], ex * v[7] - ey * v[6], mag(ey) * h[0] + mag(ex) * h[1]);
    }
    return ok;
}

// bit i: vertex i + 1 lies in the box, |v_i[k]| <= h_k for all k (false on NaN).  7: the triangle lies wholly inside; 0: the
// box cuts it without holding a vertex
template <class T> IBVH_D unsigned inside_mask(const T *h, const T *v) {
    unsigned mask = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const T x = mag(v[3 * i]), y = mag(v[3 * i + 1]), z = mag(v[3 * i + 2]);
        if ((x <= h[0]) & (y <= h[1]) & (z <= h[2])) mask |= 1u << i;
    }
    return mask;
}

} // namespace tribox
} // namespace ibvh
