// ibvh_raysphere.hpp — when the centre of a moving sphere first comes within reach of a fixed sphere: steps 1 to 3 of
// include/ibvh.h (ibvh_cast_spheres) as ONE routine, the ray-against-sphere quadratic of the library.  No reference
// counterpart: the reference's isintersection(BSphere, p, d) answers yes / no for the whole line.
//
// The touching test is the library's own iscontact(BSphere, BSphere) (iscontact.jl), bit for bit: the same squared centre
// distance, the same (R + r) * (R + r); the quadratic is, operation for operation, the `vertex` candidate of ibvh_sweep.hip
// with r2 = (R + r) * (R + r).  ibvh_sweep.hip keeps its own `vertex` for now — its host tests pin its source text — so
// folding the two into this routine is a later change.
#pragma once
#include "ibvh_common.hpp"
#include "ibvh_raytest.hpp"

#include <limits>

namespace ibvh {
namespace raysphere {

using raytri::dot3;

// t_k of include/ibvh.h for the fixed sphere (c, R) and the sphere of radius r whose centre moves from p along d (dd =
// dot(d, d)): 0 where the two touch at the start, else the smaller root of the quadratic, +Inf where there is none.  Every
// operation rounds once; every comparison is false on NaN, so a NaN anywhere gives +Inf.
template <class T> IBVH_D T first_touch(const T *c, T R, const T *p, const T *d, T dd, T r) {
    const T inf = std::numeric_limits<T>::infinity();
    const T S = R + r;
    const T m[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const T mm = dot3(m, m);
    const T S2 = S * S;
    const T B = dot3(m, d);
    const T Cq = mm - S2;
    const T disc = B * B - dd * Cq;
    const T t = (-B - ibvh_sqrt(disc)) / dd;
    const bool valid = (mm > S2) & (dd > T(0)) & (disc >= T(0)) & (t >= T(0));
    return mm <= S2 ? T(0) : (valid ? t : inf);
}

} // namespace raysphere
} // namespace ibvh
