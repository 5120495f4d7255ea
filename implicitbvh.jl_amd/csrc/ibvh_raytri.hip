// ibvh_raytri.hip — resolve the (leaf.index, iray) list of an LVT ray traversal against the mesh's triangles: the exact
// ray-triangle test per candidate and the nearest hit per ray (include/ibvh.h, ibvh_rays_resolve_triangles).  No reference
// counterpart: ImplicitBVH.jl stops at the candidate list (raytrace/leaf_vs_tree/leaf_vs_tree.jl:170-228).
//
// The list is grouped by ray and the traversal's scanned counts are its CSR offsets, so the nearest hit is a segmented
// minimum: no atomics, one deterministic winner.  Work mapping: a GROUP of kGroup consecutive lanes owns one ray; the
// group reads its segment kGroup candidates a trip (neighbouring lanes read neighbouring list entries), every lane
// gathers its candidate's triangle (36 / 72 bytes) and tests it, keeps its own best, and the group's best is found by a
// butterfly over DPP lane exchanges (no LDS, no memory).  The lane that owns the winner stores the ray's outputs, so
// they carry the winner's bits untouched.  kGroup = 8: segments average ~10 candidates on a 7.2 M-triangle surface of
// sphere leaves under 1e6 rays and ~4 with box leaves.  Measured against 4 and 16 (DESIGN.md §3 "Ray hit lists against
// triangles"): 4 loses everywhere, 16 ties on the sphere leaves and idles twelve lanes of sixteen on the box leaves.
#include "ibvh_common.hpp"
#include "ibvh_raytest.hpp"

#include <limits>

#ifndef IBVH_RAYTRI_GROUP
#define IBVH_RAYTRI_GROUP 8 // lanes per ray: 4, 8 or 16 (development builds may override it)
#endif

namespace ibvh {
namespace raytri {

constexpr int kGroup = IBVH_RAYTRI_GROUP;
static_assert(kGroup == 4 || kGroup == 8 || kGroup == 16, "a lane group is a quad, half a DPP row or a DPP row");

// DPP controls: lane i <- lane i^1, i^2 of its quad; the mirror image of its half row (8 lanes) / row (16 lanes).  Once
// the four lanes of every quad agree, the half-row mirror pairs quad 0 with quad 1 (= i^4) and, once the halves agree,
// the row mirror pairs the two halves (= i^8).
enum { kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140 };

template <int CTRL, class V> IBVH_D V dpp_from(const V &v) {
    static_assert(sizeof(V) % 4 == 0, "moved as 32-bit words");
    V out;
    const int *s = (const int *)&v;
    int *d = (int *)&out;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(V) / 4); ++k) d[k] = __builtin_amdgcn_update_dpp(s[k], s[k], CTRL, 0xf, 0xf, false);
    return out;
}

// (t, k): a hit's parameter and its position in the list.  Smaller t wins; equal t (-0 == +0 included): the earlier
// entry.  "No hit" is (+Inf, kNone): it loses against every hit, also one whose t is +Inf.
template <class T, class K> struct Best {
    T t;
    K k;
};
template <class T, class K> IBVH_D bool wins(const Best<T, K> &a, const Best<T, K> &b) {
    return (a.t < b.t) | ((a.t == b.t) & (a.k < b.k));
}
template <int CTRL, class T, class K> IBVH_D void reduce_step(Best<T, K> &b) {
    const Best<T, K> o = dpp_from<CTRL>(b);
    if (wins(o, b)) b = o;
}

// (the exact test itself — cross3, dot3, Tri, ray_triangle — is ibvh_raytest.hpp's: the ray cast shares its bits)

// (raise_flag: ibvh_common.hpp.  Within one launch only ONE bit is ever raised here: bit 0 excludes all other work.)
constexpr int kBlock = 256;
constexpr int kRaysPerBlock = kBlock / kGroup;

template <class T, class I>
__global__ __launch_bounds__(kBlock) void raytri_resolve_kernel(const T *__restrict__ tris, int64_t num_triangles,
                                                                const T *__restrict__ points, const T *__restrict__ dirs,
                                                                int64_t num_rays, const I *__restrict__ counts,
                                                                const I *__restrict__ contacts, int64_t capacity,
                                                                I *__restrict__ out_index, T *__restrict__ out_t,
                                                                T *__restrict__ out_uv, T *__restrict__ cand_t, uint32_t *flag) {
    constexpr I kNone = std::numeric_limits<I>::max();
    const T inf = std::numeric_limits<T>::infinity();
    // the traversal's total, on the device: a list that did not fit its buffer was never written
    const int64_t total = (int64_t)counts[num_rays - 1];
    if (total > capacity || total < 0) {
        if (flag && blockIdx.x == 0 && threadIdx.x == 0) raise_flag(flag, 1u);
        return;
    }
    const int sub = threadIdx.x & (kGroup - 1);
    const int64_t stride = (int64_t)gridDim.x * kRaysPerBlock;
    bool bad = false;
    for (int64_t base = (int64_t)blockIdx.x * kRaysPerBlock; base < num_rays; base += stride) { // (block-uniform trips)
        const int64_t r = base + threadIdx.x / kGroup;
        const bool live = r < num_rays;
        int64_t beg = 0, end = 0;
        T p[3] = {T(0), T(0), T(0)}, d[3] = {T(0), T(0), T(0)};
        if (live) {
            beg = r > 0 ? (int64_t)counts[r - 1] : 0;
            end = (int64_t)counts[r];
            beg = beg < 0 ? 0 : beg; // (scanned counts never leave 0..total; garbage must not leave the list either)
            end = end > total ? total : end;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[k] = points[3 * r + k];
                d[k] = dirs[3 * r + k];
            }
        }
        Best<T, I> best{inf, kNone};
        T best_u = T(0), best_v = T(0);
        I best_index = 0;
        for (int64_t k = beg + sub; k < end; k += kGroup) {
            const I index = contacts[2 * k]; // IndexPair{I}.first = leaf.index; .second is iray
            T t = inf, u, v;
            if (index >= 1 && (int64_t)index <= num_triangles) {
                Tri<T> tr;
                __builtin_memcpy(&tr, __builtin_assume_aligned(tris + 9 * ((int64_t)index - 1), sizeof(T)), sizeof(tr));
                if (!ray_triangle(tr, p, d, t, u, v)) t = inf;
                else if (best.k == kNone || t < best.t) { // (k ascends in a lane: on equal t the earlier entry stays)
                    best = {t, (I)k};
                    best_u = u;
                    best_v = v;
                    best_index = index;
                }
            } else {
                bad = true;
            }
            if (cand_t) cand_t[k] = t;
        }
        const I mine = best.k;
        reduce_step<kDppXor1>(best);
        reduce_step<kDppXor2>(best);
        if constexpr (kGroup >= 8) reduce_step<kDppHalfMirror>(best);
        if constexpr (kGroup >= 16) reduce_step<kDppMirror>(best);
        // the owner of the winning entry stores it; a ray without a hit is stored by the group's first lane
        const bool hit = best.k != kNone;
        if (live && (hit ? mine == best.k : sub == 0)) {
            if (out_index) out_index[r] = hit ? best_index : I(0);
            if (out_t) out_t[r] = hit ? best.t : inf;
            if (out_uv) {
                out_uv[2 * r] = hit ? best_u : T(0);
                out_uv[2 * r + 1] = hit ? best_v : T(0);
            }
        }
    }
    if (bad && flag) raise_flag(flag, 2u);
}

} // namespace raytri
} // namespace ibvh

using namespace ibvh;

extern "C" {

ibvh_status ibvh_rays_resolve_triangles(int32_t flt, int32_t index_type, const void *triangles, int64_t num_triangles,
                                        const void *points, const void *directions, int64_t num_rays, const void *counts,
                                        const void *contacts, int64_t capacity, void *closest_index, void *closest_t,
                                        void *closest_uv, void *cand_t, void *flag, void *stream) {
    if (num_triangles < 0 || num_rays < 0 || capacity < 0) return IBVH_ERR_INVALID_ARG;
    if (!closest_index && !closest_t && !closest_uv && !cand_t) return IBVH_ERR_INVALID_ARG;
    if ((num_triangles > 0 && !triangles) || (capacity > 0 && !contacts)) return IBVH_ERR_INVALID_ARG;
    if (num_rays > 0 && (!points || !directions || !counts)) return IBVH_ERR_INVALID_ARG;
    if (flt != IBVH_F32 && flt != IBVH_F64) return IBVH_ERR_UNSUPPORTED;
    if (index_type != IBVH_I32 && index_type != IBVH_I64) return IBVH_ERR_UNSUPPORTED;
    if (num_rays == 0) return IBVH_OK;
    const int64_t b = ceil_div(num_rays, raytri::kRaysPerBlock);
    const unsigned blocks = (unsigned)(b > 16384 ? 16384 : b);
    auto launch = [&](auto ft, auto it) -> int {
        using T = typename decltype(ft)::type;
        using I = typename decltype(it)::type;
        IBVH_LAUNCH((raytri::raytri_resolve_kernel<T, I>), dim3(blocks), dim3(raytri::kBlock), 0, (hipStream_t)stream,
                    (const T *)triangles, num_triangles, (const T *)points, (const T *)directions, num_rays,
                    (const I *)counts, (const I *)contacts, capacity, (I *)closest_index, (T *)closest_t, (T *)closest_uv,
                    (T *)cand_t, (uint32_t *)flag);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    };
    if (flt == IBVH_F32)
        return (ibvh_status)(index_type == IBVH_I32 ? launch(Tag<float>{}, Tag<int32_t>{}) : launch(Tag<float>{}, Tag<int64_t>{}));
    return (ibvh_status)(index_type == IBVH_I32 ? launch(Tag<double>{}, Tag<int32_t>{}) : launch(Tag<double>{}, Tag<int64_t>{}));
}

} // extern "C"
