// ibvh_firsthit.hpp — the closest / any-hit protocol of the three queries that answer "what does this moving thing touch
// first, or does it touch anything at all?": ibvh_cast.hip (a ray against a mesh), ibvh_sweep.hip (a moving sphere against
// a mesh) and ibvh_spherecast.hip (a ray or a moving sphere against a sphere cloud).  Once each: the limit L from the
// optional per-item t_max, the answer and the one place a candidate (t*, index) enters it, the walk under the mode's limit,
// the stores both modes share, and the entry points' mode / outputs rule.  A kernel keeps loading its query, its own
// admissibility test (L >= 0, r >= 0, its NaN rule), its gather, its evaluation, its clamp(s) and its payload; an entry point
// its pointer checks, its prepare() call and its launch.  No reference counterpart: ImplicitBVH.jl has no first-hit query.
#pragma once
#include "ibvh_pointwalk.hpp"

namespace ibvh {
namespace firsthit {

// L of include/ibvh.h: a hit is finite (a NaN limit stays NaN and admits nothing)
template <class T> IBVH_D T limit(const T *__restrict__ t_max, int64_t item) {
    const T given = t_max ? t_max[item] : std::numeric_limits<T>::infinity();
    return given > std::numeric_limits<T>::max() ? std::numeric_limits<T>::max() : given;
}

// one item's answer so far: the best (t*, index) — best starts at L, index 0: nothing yet — or, any-hit, the bit
template <class T, class I> struct Answer {
    T L, best;
    I best_index = 0;
    bool touched = false;
    IBVH_D explicit Answer(T limit) : L(limit), best(limit) {}
};

// a candidate of include/ibvh.h is offered: any-hit only notes one within L; closest takes it if (t*, index) lies
// lexicographically below the best, and then lets the caller keep() the payload that goes with it
template <bool ANY, class T, class I, class Keep> IBVH_D void offer(Answer<T, I> &a, T ts, I index, const Keep &keep) {
    if constexpr (ANY) {
        a.touched |= ts <= a.L;
    } else if (pointwalk::wins(ts, index, a.best, a.best_index)) {
        a.best = ts;
        a.best_index = index;
        keep();
    }
}

// pointwalk::walk under the mode's limit: the closest query lowers it to the best t* so far, the any-hit query drops it to
// -Inf at its first hit, which ends the walk.  VL: BBox<T> (a mesh) or BSphere<T> (a cloud)
template <bool ANY, class VL, class TN, class T, class I, class Bound, class Visit>
IBVH_D void walk(const TreeDev &tree, int built_level, const char *__restrict__ leaves, const LeafLayout &lay,
                 const BBox<TN> *__restrict__ nodes, const Answer<T, I> &a, const Bound &bound, const Visit &visit) {
    const T inf = std::numeric_limits<T>::infinity(), L = a.L;
    if constexpr (ANY) pointwalk::walk<VL, TN>(tree, built_level, leaves, lay, nodes, bound, [&]() { return a.touched ? -inf : L; }, visit);
    else pointwalk::walk<VL, TN>(tree, built_level, leaves, lay, nodes, bound, [&]() { return a.best; }, visit);
}

// the item's walk is done: any-hit stores its byte; closest the index and t* (+Inf on a miss), then the unit its payload
template <bool ANY, class T, class I>
IBVH_D void store(const Answer<T, I> &a, int64_t item, I *__restrict__ out_index, T *__restrict__ out_t, uint8_t *__restrict__ out_any) {
    if constexpr (ANY) {
        out_any[item] = a.touched ? 1 : 0;
    } else {
        const bool hit = a.best_index != 0;
        if (out_index) out_index[item] = a.best_index;
        if (out_t) out_t[item] = hit ? a.best : std::numeric_limits<T>::infinity();
    }
}

// ---- the entry points (host) -------------------------------------------------------------------------------------------

// The two modes.  The three public enums are one pair of values, which the rule below relies on.
static_assert(IBVH_CAST_CLOSEST == 0 && IBVH_CAST_ANY == 1 && IBVH_SWEEP_CLOSEST == 0 && IBVH_SWEEP_ANY == 1, "one pair");
static_assert(IBVH_SPHERECAST_CLOSEST == 0 && IBVH_SPHERECAST_ANY == 1, "the same pair"); // (ibvh_spherecast.hip)

// a valid mode; any-hit needs its byte and none of the closest outputs, closest at least one of its own and no byte (else
// IBVH_ERR_INVALID_ARG)
inline bool outputs_ok(int32_t mode, const void *any_output, bool closest_outputs) {
    return mode == IBVH_CAST_ANY ? any_output && !closest_outputs : mode == IBVH_CAST_CLOSEST && !any_output && closest_outputs;
}

} // namespace firsthit
} // namespace ibvh
