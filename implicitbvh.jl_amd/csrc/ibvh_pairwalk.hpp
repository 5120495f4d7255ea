// ibvh_pairwalk.hpp — the lane routine of the two queries that answer with the closest PAIR of a query item and a mesh
// triangle, ibvh_tridist.hip (a query triangle) and ibvh_segdist.hip (a segment): the two walks, the best pair so far under
// the tie rule, and the five outputs.  A kernel keeps what is its own: loading its item, its NaN rule, its gather (which
// may drop a leaf) and its evaluation of one pair.  The walk is ibvh_pointwalk.hpp's, the pair ibvh_trigeom.hpp's.
#pragma once
#include "ibvh_pointtri.hpp"
#include "ibvh_pointwalk.hpp"
#include "ibvh_trigeom.hpp"

#include <limits>

namespace ibvh {
namespace pairwalk {

// The closest pair of one item: the lexicographic minimum of (d2, index) over the triangles gather() admits, within max_d2
// -> the triangle's index, 0 = none (then `best` holds max_d2 and zeros); hopeless: the item has no answer, nothing is walked.
//   bound(lo, up) -> T               the item's bound of a box: never above an evaluated d2 under it (the caller's argument)
//   gather(rec, index, K) -> bool    the leaf's triangle; false: the leaf names none or is dropped
//   evaluate(K, pair)                the evaluation of include/ibvh.h for (item, K)
//
// The lane walks twice.  First ibvh_closest.hip's walk from seed_point, so that an unbounded query does not start blind: the
// squared distance from seed_point to the closest triangle F that gather() admits (a fraction of a pair per visit).  THE
// CALLER'S OBLIGATION: seed_point is the first point candidate 0 of evaluate() is evaluated from — candidate 0 is
// closest_on_triangle(K, seed_point), and a later candidate only replaces it with a smaller d2.  Then that value IS
// candidate 0 of the pair (item, F), bit for bit, so that pair's d2 cannot exceed it and the answer's neither: nothing beyond
// it can win or tie, and F itself is still reached (its bounds do not exceed its d2).  The second walk — the query's own —
// starts from that limit, not from the radius, and prunes from its first node on.
template <class I, class T, class TN, class Bound, class Gather, class Evaluate>
IBVH_D I closest_pair(const TreeDev &tree, int built_level, const char *__restrict__ leaves, const LeafLayout &lay,
                      const BBox<TN> *__restrict__ nodes, bool hopeless, const T *seed_point, T max_d2, const Bound &bound,
                      const Gather &gather, const Evaluate &evaluate, trigeom::Pair<T> &best) {
    const T zero[3] = {T(0), T(0), T(0)};
    best.put(max_d2, zero, zero, 0); // best.d2 is the limit: the radius, then the first limit, then the best pair's
    I best_index = 0;
    if (hopeless) return best_index;
    T seed = max_d2;
    auto near_seed = [&](const char *rec) {
        I index;
        raytri::Tri<T> K;
        T x[3];
        int region;
        if (!gather(rec, index, K)) return;
        const T d2 = pointtri::closest_on_triangle(K.v, seed_point, x, region);
        seed = d2 < seed ? d2 : seed;
    };
    auto box_seed = [&](const T *lo, const T *up) { return pointwalk::box_bound(lo, up, seed_point); };
    pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, box_seed, [&]() { return seed; }, near_seed);
    best.d2 = seed;
    auto visit = [&](const char *rec) {
        I index;
        raytri::Tri<T> K; // p1 p2 p3
        if (!gather(rec, index, K)) return;
        trigeom::Pair<T> r;
        evaluate(K, r);
        if (pointwalk::wins(r.d2, index, best.d2, best_index)) {
            best = r;
            best_index = index;
        }
    };
    pointwalk::walk<BBox<T>, TN>(tree, built_level, leaves, lay, nodes, bound, [&]() { return best.d2; }, visit);
    return best_index;
}

// the item's five outputs, each optional: the index (0 = none), d2 (+Inf), the two points and the kind (0)
template <class T, class I>
IBVH_D void store_pair(int64_t item, I best_index, const trigeom::Pair<T> &best, I *__restrict__ out_index, T *__restrict__ out_d2,
                       T *__restrict__ out_xq, T *__restrict__ out_xk, uint8_t *__restrict__ out_kind) {
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

} // namespace pairwalk
} // namespace ibvh
