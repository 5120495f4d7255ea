// ibvh_slab.hpp — the slab test of include/ibvh.h (ibvh_cast_rays): where a ray enters a box.  ONE copy for the four queries
// that prune on it and pin it bit for bit: ibvh_cast.hip (a ray against the leaves' boxes), and ibvh_sweep.hip,
// ibvh_spherecast.hip (a moving sphere's centre) and ibvh_capsules.hip (a capsule's segment) against the boxes grown by the
// radius (grown_entry).  No reference counterpart: the reference's isintersection answers
// yes / no for the whole line and its 0 * Inf is NaN on a box face.
#pragma once
#include "ibvh_common.hpp"

#include <limits>

namespace ibvh {
namespace slab {

// entry(box) of include/ibvh.h: the slab test's tmin where the ray meets the box, +Inf where it does not.  An axis the ray
// does not move along admits or refuses by comparing the origin; the selects keep a NaN where the header says they do.
template <class T> IBVH_D T slab_entry(const T *lo, const T *up, const T *p, const T *d, const T *inv) {
    const T inf = std::numeric_limits<T>::infinity();
    T tmin = -inf, tmax = inf;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool still = d[k] == T(0);
        const T t1 = (lo[k] - p[k]) * inv[k], t2 = (up[k] - p[k]) * inv[k];
        const T tnear = t2 < t1 ? t2 : t1, tfar = t2 > t1 ? t2 : t1;
        const T nmin = tnear > tmin ? tnear : tmin, nmax = tfar < tmax ? tfar : tmax;
        ok &= !still | ((lo[k] <= p[k]) & (p[k] <= up[k]));
        tmin = still ? tmin : nmin;
        tmax = still ? tmax : nmax;
    }
    return (ok & (tmin <= tmax) & (tmax >= T(0))) ? tmin : inf;
}

// that entry into the box grown by r.  lo - r and up + r are round-to-nearest, hence monotone: a grown box contains the
// grown box of whatever the box itself contains, so the entry stays a lossless bound (ibvh_sweep.hip)
template <class T> IBVH_D T grown_entry(const T *lo, const T *up, T r, const T *p, const T *d, const T *inv) {
    const T glo[3] = {lo[0] - r, lo[1] - r, lo[2] - r}, gup[3] = {up[0] + r, up[1] + r, up[2] + r};
    return slab_entry(glo, gup, p, d, inv);
}

} // namespace slab
} // namespace ibvh
