// ibvh_segtri.hpp — the segment-triangle evaluation of include/ibvh.h (ibvh_capsule_contacts): the closest points xs of the
// segment S = a -> b and xk of the triangle K = p1 p2 p3, their squared distance, and which of six rules decided.  ONE copy
// for the two queries that answer with it — ibvh_capsules.hip (every triangle within a capsule's radius of its segment) and
// ibvh_segdist.hip (the closest triangle per segment) — so that both compute the same bits.  It is built from the pieces
// the tree already has one copy of: ibvh_trigeom.hpp's boxes and cut test (the cut rule, on ibvh_raytest.hpp's exact test),
// ibvh_pointtri.hpp's point-triangle evaluation (the two ends) and ibvh_segseg.hpp's segment-segment evaluation (the three
// edges).  No reference counterpart: ImplicitBVH.jl has no segment distance and no exact triangle test.
//
// The triangle's feature under xk is NOT reported: ibvh_segseg.hpp does not classify where on an edge its point lies (an end
// or the inside), so a feature code could only be given for the kinds 0 and 1, and is given for none.
#pragma once
#include "ibvh_common.hpp"
#include "ibvh_pointtri.hpp"
#include "ibvh_raytest.hpp"
#include "ibvh_segseg.hpp"
#include "ibvh_trigeom.hpp"

namespace ibvh {
namespace segtri {

constexpr int kCut = 5; // the kind of a pair the cut rule decided

// S's exact box: [min(a, b), max(a, b)] per component by `x < y ? x : y` / `x > y ? x : y`
template <class T> IBVH_D void segment_box(const T *a, const T *b, T *lo, T *up) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = a[k] < b[k] ? a[k] : b[k];
        up[k] = a[k] > b[k] ? a[k] : b[k];
    }
}

// The evaluation of include/ibvh.h for one pair: S = a -> b with its exact box, K = p1 p2 p3; r.xq is xs.
template <class T>
IBVH_D void evaluate(const T *a, const T *b, const T *slo, const T *sup, const raytri::Tri<T> &K, trigeom::Pair<T> &r) {
    using trigeom::sel;
    // the cut rule, under the box clause only: the segment is the ray a + t (b - a), t <= 1
    T klo[3], kup[3];
    trigeom::triangle_box(K.v, klo, kup);
    const bool apart = trigeom::apart(slo, sup, klo, kup);
    if (!apart) {
        T cut[3];
        if (trigeom::segment_cuts(K, a, b, cut)) {
            r.put(T(0), cut, cut, kCut);
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
    // ... 2, 3, 4: S against K's edges p1p2, p2p3, p3p1
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        T p2[3], q2[3];
        trigeom::edge_of(K.v, c, p2, q2);
        r.offer(segseg::closest_on_segments(a, b, p2, q2, x, y), x, y, 2 + c);
    }
}

} // namespace segtri
} // namespace ibvh
