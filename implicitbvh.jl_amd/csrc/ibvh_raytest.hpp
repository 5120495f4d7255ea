// ibvh_raytest.hpp — the exact ray-triangle test of include/ibvh.h (ibvh_rays_resolve_triangles), ONE copy for the
// queries that pin it bit for bit: ibvh_raytri.hip (the nearest hit of a candidate list), ibvh_cast.hip (the ray cast),
// ibvh_sweep.hip (a moving sphere against a face) and ibvh_trigeom.hpp's segment_cuts (a segment against a triangle: the
// edges of ibvh_tritri.hip and ibvh_tridist.hip, the segment of ibvh_segtri.hpp for ibvh_capsules.hip and ibvh_segdist.hip).
// No reference counterpart: ImplicitBVH.jl stops at the candidate list (raytrace/leaf_vs_tree/leaf_vs_tree.jl:170-228).
#pragma once
#include "ibvh_common.hpp"

namespace ibvh {
namespace raytri {

// a cross-product component: two rounded products, one rounded subtraction; a dot product: (x0 y0 + x1 y1) + x2 y2
// (-ffp-contract=off: nothing is fused)
template <class T> IBVH_D void cross3(const T *x, const T *y, T *o) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}
template <class T> IBVH_D T dot3(const T *x, const T *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

template <class T> struct Tri {
    T v[9]; // p1 p2 p3
};

// Moeller-Trumbore, two-sided, forwards only (t >= 0, like the reference's `tmax >= 0`, isintersection.jl); every
// comparison is false on NaN
template <class T> IBVH_D bool ray_triangle(const Tri<T> &tr, const T *p, const T *d, T &t, T &u, T &v) {
    const T *a = tr.v, *b = tr.v + 3, *c = tr.v + 6;
    const T e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const T e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    T pv[3], qv[3];
    cross3(d, e2, pv);
    const T det = dot3(e1, pv);
    const T inv = T(1) / det;
    const T tv[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    u = dot3(tv, pv) * inv;
    cross3(tv, e1, qv);
    v = dot3(d, qv) * inv;
    t = dot3(e2, qv) * inv;
    return (det != T(0)) & (u >= T(0)) & (v >= T(0)) & (u + v <= T(1)) & (t >= T(0));
}

} // namespace raytri
} // namespace ibvh
