// ibvh_sweep.hip — sweep a batch of spheres against the mesh a BVH was built over, in one launch: per sphere of radius r
// moving from p to p + d the first time it touches the surface — which triangle, when, where on it and on which feature —
// or only whether it touches anything within its limit (include/ibvh.h, ibvh_sweep_spheres).  Continuous collision detection
// for particles against a surface.  No reference counterpart: ImplicitBVH.jl has no moving volumes and no exact triangle test.
//
// The result is defined over ALL triangles — the lexicographic minimum of (t*, index) over the hits, t* = max(t, entry of
// the triangle's leaf box grown by r) — so the walk only has to be lossless.  It is, without an epsilon, by ibvh_cast.hip's
// argument on the grown boxes: lo - r and up + r are round-to-nearest, hence monotone, so the grown box of a node contains
// the grown box of everything below it exactly as the boxes themselves do; the slab entry is monotone in the corners; so the
// COMPUTED entry of a grown node is <= that of every grown box below it, an admitted grown box has admitted grown ancestors,
// and t* >= entry(grown leaf) >= entry(every grown ancestor): a box whose entry exceeds the limit holds nothing that could
// still win.
//
// The walk itself — work mapping, the trail word, the pop, the strict skip — is ibvh_pointwalk.hpp's, with ibvh_slab.hpp's
// entry of the grown box (grown_entry) as the bound.  The limit, the answer and the walk under the mode's limit — from the
// sphere's own t_max down to the best t* so far, or to -Inf at the first hit — are ibvh_firsthit.hpp's.  A triangle's time
// of contact is that of the centre's ray against the triangle grown by r: the two faces of its prism, three cylinders, three
// spheres.  The start position is ibvh_pointtri.hpp's evaluation (the bits ibvh_spheres.hip computes), the face is
// ibvh_raytest.hpp's exact test from the origin moved by r along the normal; the cylinders and spheres are the quadratics
// below.  Sphere, inverse displacement and best hit live in registers.
#include "ibvh_firsthit.hpp"
#include "ibvh_pointtri.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_slab.hpp"

#include <limits>

namespace ibvh {
namespace sweep {

using pointwalk::kBlock;
using raytri::dot3;

// the first touch of one triangle so far: t_k (+Inf: none yet), where, and on which feature (ibvh_sphere_contacts' codes)
template <class T> struct Touch {
    T t, q[3];
    int feature;
};

// a candidate of include/ibvh.h, taken in the header's order: a later one has to be strictly earlier
template <class T> IBVH_D void keep(Touch<T> &k, bool valid, T t, T q0, T q1, T q2, int feature) {
    if (valid & (t < k.t)) {
        k.t = t;
        k.q[0] = q0;
        k.q[1] = q1;
        k.q[2] = q2;
        k.feature = feature;
    }
}

// the face: the centre's ray from o = p moved by r along the normal towards the triangle's plane, exact test
template <class T> IBVH_D void face(Touch<T> &k, const raytri::Tri<T> &tr, const T *p, const T *d, T r) {
    const T *a = tr.v, *b = tr.v + 3, *c = tr.v + 6;
    const T e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const T e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const T pa[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    T n[3];
    raytri::cross3(e1, e2, n);
    const T len = ibvh_sqrt(dot3(n, n));
    const T s0 = dot3(n, pa);
    const T f = (s0 >= T(0) ? r : -r) / len; // (side * r) / len
    const T o[3] = {p[0] - f * n[0], p[1] - f * n[1], p[2] - f * n[2]};
    T t, u, v;
    const bool valid = raytri::ray_triangle(tr, o, d, t, u, v);
    keep(k, valid, t, o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2], 6);
}

// an edge (x, y): the centre's ray against the cylinder of radius r around it, between its ends
template <class T> IBVH_D void edge(Touch<T> &k, const T *x, const T *y, const T *p, const T *d, T dd, T r2, int feature) {
    const T e[3] = {y[0] - x[0], y[1] - x[1], y[2] - x[2]};
    const T m[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
    const T ee = dot3(e, e), me = dot3(m, e), de = dot3(d, e), md = dot3(m, d);
    const T A = ee * dd - de * de;
    const T B = ee * md - de * me;
    const T Cq = ee * (dot3(m, m) - r2) - me * me;
    const T disc = B * B - A * Cq;
    const T t = (-B - ibvh_sqrt(disc)) / A;
    const T s = me + t * de;
    const bool valid = (A > T(0)) & (disc >= T(0)) & (t >= T(0)) & (s >= T(0)) & (s <= ee);
    const T w = s / ee;
    keep(k, valid, t, x[0] + w * e[0], x[1] + w * e[1], x[2] + w * e[2], feature);
}

// a vertex x: the centre's ray against the sphere of radius r around it
template <class T> IBVH_D void vertex(Touch<T> &k, const T *x, const T *p, const T *d, T dd, T r2, int feature) {
    const T m[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
    const T B = dot3(m, d);
    const T Cq = dot3(m, m) - r2;
    const T disc = B * B - dd * Cq;
    const T t = (-B - ibvh_sqrt(disc)) / dd;
    const bool valid = (dd > T(0)) & (disc >= T(0)) & (t >= T(0));
    keep(k, valid, t, x[0], x[1], x[2], feature);
}

// T: the leaves', triangles' and spheres' float type; TN: the nodes' (the same or wider — a node box then holds values of
// T, widened exactly, and narrows back exactly); ANY: only "does it touch anything", the walk ends at the first hit
template <class T, class TN, class I, bool ANY>
__global__ __launch_bounds__(pointwalk::kBlock) void sweep_walk_kernel(
    TreeDev tree, int built_level, const char *__restrict__ leaves, LeafLayout lay, const BBox<TN> *__restrict__ nodes,
    const T *__restrict__ tris, int64_t num_triangles, const T *__restrict__ centers, const T *__restrict__ disps,
    const T *__restrict__ radii, int64_t num_spheres, const T *__restrict__ t_max, I *__restrict__ out_index,
    T *__restrict__ out_t, T *__restrict__ out_q, uint8_t *__restrict__ out_feature, uint8_t *__restrict__ out_touched,
    uint32_t *flag) {
    const T inf = std::numeric_limits<T>::infinity();
    bool bad = false;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < num_spheres; item += (int64_t)gridDim.x * kBlock) {
        const T p[3] = {centers[3 * item], centers[3 * item + 1], centers[3 * item + 2]};
        const T d[3] = {disps[3 * item], disps[3 * item + 1], disps[3 * item + 2]};
        const T inv[3] = {T(1) / d[0], T(1) / d[1], T(1) / d[2]};
        const T r = radii[item];
        const T r2 = r * r, dd = dot3(d, d);
        const T L = firsthit::limit(t_max, item);
        firsthit::Answer<T, I> answer(L);
        T best_q[3] = {T(0), T(0), T(0)};
        int best_feature = 0;
        // the entry of the centre's ray into a box grown by r (monotone roundings: a grown node holds its grown children)
        auto grown = [&](const T *lo, const T *up) { return slab::grown_entry(lo, up, r, p, d, inv); };
        // only a leaf that passes gathers its triangle (36 / 72 bytes)
        auto visit = [&](const char *rec) {
            I index;
            raytri::Tri<T> tr;
            if (pointwalk::leaf_triangle(rec, lay, tris, num_triangles, index, tr.v)) {
                const BBox<T> b = load_vol<BBox<T>>(rec);
                const T entry = grown(b.lo, b.up);
                Touch<T> k;
                k.t = inf;
                int region;
                const T d2 = pointtri::closest_on_triangle(tr.v, p, k.q, region);
                k.feature = region;
                if (d2 <= r2) { // already touching (false on NaN)
                    k.t = T(0);
                } else if (d2 > r2) { // (a NaN d2 — a NaN vertex, a NaN centre — is no hit)
                    const T *a = tr.v, *b3 = tr.v + 3, *c = tr.v + 6;
                    face(k, tr, p, d, r);
                    edge(k, a, b3, p, d, dd, r2, 2);
                    edge(k, b3, c, p, d, dd, r2, 5);
                    edge(k, c, a, p, d, dd, r2, 4);
                    vertex(k, a, p, d, dd, r2, 0);
                    vertex(k, b3, p, d, dd, r2, 1);
                    vertex(k, c, p, d, dd, r2, 3);
                }
                const T ts = entry > k.t ? entry : k.t; // t*: the clamp (+Inf: no candidate, or the grown box refused)
                firsthit::offer<ANY>(answer, ts, index, [&]() {
                    best_feature = k.feature;
#pragma unroll
                    for (int j = 0; j < 3; ++j) best_q[j] = k.q[j];
                });
            } else {
                bad = true;
            }
        };
        // a negative or NaN radius touches nothing; t* >= 0: a negative or NaN limit admits nothing, and a NaN could not prune
        if ((r >= T(0)) & (L >= T(0))) firsthit::walk<ANY, BBox<T>, TN>(tree, built_level, leaves, lay, nodes, answer, grown, visit);
        firsthit::store<ANY>(answer, item, out_index, out_t, out_touched);
        if constexpr (!ANY) {
            if (out_q) out_q[3 * item] = best_q[0], out_q[3 * item + 1] = best_q[1], out_q[3 * item + 2] = best_q[2];
            if (out_feature) out_feature[item] = (uint8_t)best_feature;
        }
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace sweep
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_sweep_spheres(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles, const void *centers,
                               const void *displacements, const void *radii, int64_t num_spheres, const void *t_max,
                               int32_t mode, void *hit_index, void *hit_t, void *hit_point, void *hit_feature, void *touched,
                               void *flag, void *stream) {
    if (!bvh || num_triangles < 0 || num_spheres < 0) return IBVH_ERR_INVALID_ARG;
    if (!firsthit::outputs_ok(mode, touched, hit_index || hit_t || hit_point || hit_feature)) return IBVH_ERR_INVALID_ARG;
    const bool any = mode == IBVH_SWEEP_ANY;
    // box leaves: the lossless bound needs boxes that contain their triangles' boxes exactly, all the way up
    pointwalk::Prepared pre;
    const bool pointers_ok = (num_triangles == 0 || triangles) && (num_spheres == 0 || (centers && displacements && radii));
    const ibvh_status st = pointwalk::prepare(bvh, true, num_spheres, pointers_ok, pre);
    if (st != IBVH_OK || pre.blocks == 0) return st;
    auto launch = [&](auto ft, auto nt, auto it, auto mt) -> int {
        using T = typename decltype(ft)::type;
        using TN = typename decltype(nt)::type;
        using I = typename decltype(it)::type;
        constexpr bool ANY = decltype(mt)::value;
        IBVH_LAUNCH((sweep::sweep_walk_kernel<T, TN, I, ANY>), dim3(pre.blocks), dim3(pointwalk::kBlock), 0, (hipStream_t)stream,
                    pre.tree, (int)bvh->built_level, (const char *)bvh->leaves, pre.lay, (const BBox<TN> *)bvh->nodes,
                    (const T *)triangles, num_triangles, (const T *)centers, (const T *)displacements, (const T *)radii,
                    num_spheres, (const T *)t_max, (I *)hit_index, (T *)hit_t, (T *)hit_point, (uint8_t *)hit_feature,
                    (uint8_t *)touched, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    return (ibvh_status)pointwalk::dispatch_box_types_and_bool(bvh->types, any, launch);
}

} // extern "C"
