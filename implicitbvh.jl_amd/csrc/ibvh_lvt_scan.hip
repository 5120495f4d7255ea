// ibvh_lvt_scan.hip — the inclusive scan that turns the per-item counts of a leaf-vs-tree counting pass into list offsets
// (AK.accumulate!, traverse_single.jl:57), in place, and leaves the total where the caller asked for it: scan_counts
// (ibvh_lvt.hpp) for ibvh_lvt.hip (self, pair, rays) and ibvh_lvt_raybins.hip (the binned ray path's two helper scans).
//
// Two routes, four kernels, all built from the tile steps below (a tile: SCAN_TILE items, SCAN_IPT consecutive ones a thread):
//   scan_reduce_kernel + scan_apply_kernel                 two launches, behind any producer
//   scan_fused_kernel / scan_fused_grouped_kernel          one launch, for counts whose producer zeroed the tile aggregates
#include "ibvh_lvt.hpp"

namespace ibvh {
namespace lvt {

constexpr int SCAN_TPB = 256, SCAN_IPT = SCAN_TILE / SCAN_TPB, SCAN_WAVES = SCAN_TPB / 64;
constexpr unsigned long long THERE = 1ull << 63; // bit 63 of a published aggregate

IBVH_D int64_t block_sum(int64_t v, int64_t *s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t t = 0;
#pragma unroll
    for (int i = 0; i < SCAN_WAVES; ++i) t += s_w[i];
    __syncthreads();
    return t;
}

// ---- the steps ------------------------------------------------------------------------------------------------------------
// the array's length: min(n, *limit) when it is known only on the device — tiles beyond it hold zeros and store nothing
IBVH_D int64_t clamp_length(int64_t n, const int32_t *limit) {
    if (limit != nullptr) n = (int64_t)*limit < n ? (int64_t)*limit : n;
    return n;
}

// A thread's SCAN_IPT consecutive items of a tile (so that its running sum is in memory order): 64 or 128 contiguous bytes,
// moved with 16-byte accesses when the array allows it (`vec`; one 4-byte access per item makes every load instruction of a
// wave touch 64 different lines), item by item and guarded by the length otherwise.
IBVH_D int64_t tile_base(int64_t tile) { return tile * SCAN_TILE + (int64_t)threadIdx.x * SCAN_IPT; }
template <class I> IBVH_D bool tile_vec(const I *c, int64_t n, int64_t base) { return base + SCAN_IPT <= n && ((uintptr_t)c & 15) == 0; }
// -> the sum of the items
template <class I> IBVH_D int64_t tile_load(const I *c, int64_t n, int64_t tile, int64_t (&v)[SCAN_IPT]) {
    const int64_t base = tile_base(tile);
    if (tile_vec(c, n, base)) {
        I raw[SCAN_IPT];
        const uint4 *src = (const uint4 *)(c + base);
#pragma unroll
        for (int k = 0; k < SCAN_IPT * (int)sizeof(I) / 16; ++k) ((uint4 *)raw)[k] = src[k];
#pragma unroll
        for (int j = 0; j < SCAN_IPT; ++j) v[j] = (int64_t)raw[j];
    } else {
#pragma unroll
        for (int j = 0; j < SCAN_IPT; ++j) v[j] = base + j < n ? (int64_t)c[base + j] : 0;
    }
    int64_t sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_IPT; ++j) sum += v[j];
    return sum;
}
// the items' inclusive prefix, `run` being the sum of everything in front of v[0]
template <class I> IBVH_D void tile_store(I *c, int64_t n, int64_t tile, const int64_t (&v)[SCAN_IPT], int64_t run) {
    const int64_t base = tile_base(tile);
    if (tile_vec(c, n, base)) {
        I raw[SCAN_IPT];
#pragma unroll
        for (int j = 0; j < SCAN_IPT; ++j) {
            run += v[j];
            raw[j] = (I)run;
        }
        uint4 *dst = (uint4 *)(c + base);
#pragma unroll
        for (int k = 0; k < SCAN_IPT * (int)sizeof(I) / 16; ++k) dst[k] = ((const uint4 *)raw)[k];
    } else {
#pragma unroll
        for (int j = 0; j < SCAN_IPT; ++j) {
            run += v[j];
            if (base + j < n) c[base + j] = (I)run;
        }
    }
}
// The scan inside a tile: from every thread's sum, the sum of the threads in front of it -> returned, and of all -> tile_total.
// One barrier; s_w must be free on entry.
IBVH_D int64_t tile_scan(int64_t sum, int64_t *s_w, int64_t &tile_total) {
    int64_t inc = sum;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int64_t wb = 0;
    tile_total = 0;
#pragma unroll
    for (int k = 0; k < SCAN_WAVES; ++k) {
        if (k < w) wb += s_w[k];
        tile_total += s_w[k];
    }
    return wb + inc - sum;
}
// One-kernel routes: PUBLISH this workgroup's aggregate (bit 63 = "there"; one relaxed 64-bit agent-scope atomic store: value
// and flag travel together, no fence — an agent-scope fence on this part writes back and invalidates an XCD's whole L2) and LOOK
// BACK: add up the aggregates of the workgroups in front, polling those that are not there yet -> their sum.
IBVH_D int64_t publish_and_look_back(unsigned long long *agg, int64_t mine, int64_t *s_p) {
    if (threadIdx.x == 0) __hip_atomic_store(&agg[blockIdx.x], THERE | (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int64_t before = 0;
    for (int64_t j = threadIdx.x; j < (int64_t)blockIdx.x; j += SCAN_TPB) {
        unsigned long long a = __hip_atomic_load(&agg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (!(a & THERE)) {
            __builtin_amdgcn_s_sleep(1);
            a = __hip_atomic_load(&agg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        before += (int64_t)(a & ~THERE);
    }
    return block_sum(before, s_p);
}
// The grand total is known to the last workgroup before it scans anything: it publishes it FIRST — the host may be polling its
// pinned copy (total_host), and every microsecond it learns the count earlier is a microsecond more of the next step's launch
// work hidden behind this step's writing pass.
IBVH_D bool publishes_total() { return blockIdx.x == gridDim.x - 1 && threadIdx.x == 0; }
IBVH_D void publish_total(int64_t total, int64_t *totals, int64_t *total_host) {
    totals[0] = total;
    if (total_host) __hip_atomic_store(total_host, total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- two launches ---------------------------------------------------------------------------------------------------------
template <class I> __global__ __launch_bounds__(SCAN_TPB) void scan_reduce_kernel(const I *c, int64_t n, int64_t *partials, const int32_t *limit) {
    __shared__ int64_t s_w[SCAN_WAVES];
    n = clamp_length(n, limit);
    int64_t base = (int64_t)blockIdx.x * SCAN_TILE, v = 0;
#pragma unroll
    for (int j = 0; j < SCAN_IPT; ++j) {
        int64_t i = base + j * SCAN_TPB + threadIdx.x;
        if (i < n) v += (int64_t)c[i];
    }
    int64_t t = block_sum(v, s_w);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// Every workgroup derives its own tile offset from the raw tile sums (a redundant reduction of <= a few thousand values)
// instead of waiting for a single-workgroup scan launch in between.
template <class I>
__global__ __launch_bounds__(SCAN_TPB) void scan_apply_kernel(I *c, int64_t n, const int64_t *partials, int64_t *totals,
                                                              int64_t *total_host, const int32_t *limit) {
    __shared__ int64_t s_w[SCAN_WAVES], s_p[SCAN_WAVES];
    n = clamp_length(n, limit);
    int64_t before = 0;
    for (int64_t j = threadIdx.x; j < (int64_t)blockIdx.x; j += SCAN_TPB) before += partials[j];
    const int64_t tile_offset = block_sum(before, s_p);
    if (publishes_total()) publish_total(tile_offset + partials[blockIdx.x], totals, total_host);
    int64_t v[SCAN_IPT], tile_total;
    const int64_t sum = tile_load(c, n, blockIdx.x, v);
    tile_store(c, n, blockIdx.x, v, tile_offset + tile_scan(sum, s_w, tile_total));
}

// ---- one launch (round 5) -------------------------------------------------------------------------------------------------
// One launch and one dependent round trip less than reduce + apply, which are launch- and latency-bound (245 workgroups at 1e6
// leaves).  (Round 6 first took the tile from an atomic counter instead: 2,442 returning atomics on one word serialise at ~11 ns
// each — the 1e7-item scan 25 -> 56 us.)
// What the look-back's wait rests on: a workgroup waits for workgroups with SMALLER indices only, and the grid is at most HALF of
// what the device holds of this kernel at once (scan_counts: resident_scan_workgroups()).  With one such kernel alone on the
// device every workgroup waited for is therefore running or done, whatever order the hardware starts them in: forward progress
// is guaranteed.  With other work resident beside it (another stream's kernels, another process) the halved residency is a
// margin, not a proof: then the wait relies on the hardware dispatching a grid's workgroups in index order, so that a workgroup
// that runs never waits for one that has not been started.  The spin is not bounded.
// One tile per workgroup:
template <class I>
__global__ __launch_bounds__(SCAN_TPB) void scan_fused_kernel(I *c, int64_t n, unsigned long long *agg, int64_t *totals, int64_t *total_host,
                                                              const int32_t *limit) {
    __shared__ int64_t s_w[SCAN_WAVES], s_p[SCAN_WAVES];
    n = clamp_length(n, limit);
    int64_t v[SCAN_IPT], tile_total;
    const int64_t in_tile = tile_scan(tile_load(c, n, blockIdx.x, v), s_w, tile_total);
    const int64_t tile_offset = publish_and_look_back(agg, tile_total, s_p);
    if (publishes_total()) publish_total(tile_offset + tile_total, totals, total_host);
    tile_store(c, n, blockIdx.x, v, tile_offset + in_tile);
}
// For grids that would not be resident: a workgroup owns `tiles_per_group` CONSECUTIVE tiles.  Phase 1 sums them (one pass over
// its items), publishes ONE aggregate and looks back over the groups before it; phase 2 reads the items again (L2-hot) and scans
// tile by tile with a running base.  Grid = ceil(tiles / tiles_per_group) <= what the device holds at once.
template <class I>
__global__ __launch_bounds__(SCAN_TPB) void scan_fused_grouped_kernel(I *c, int64_t n, unsigned long long *agg, int64_t *totals, int64_t *total_host,
                                                                      int tiles_per_group, const int32_t *limit) {
    __shared__ int64_t s_w[SCAN_WAVES], s_p[SCAN_WAVES];
    const int64_t nparts = scan_tiles(n); // (of the launch: the grid was sized for it)
    n = clamp_length(n, limit);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_group, t1 = t0 + tiles_per_group < nparts ? t0 + tiles_per_group : nparts;
    int64_t sum = 0;
    for (int64_t tile = t0; tile < t1; ++tile) {
        int64_t v[SCAN_IPT];
        sum += tile_load(c, n, tile, v);
    }
    const int64_t group_total = block_sum(sum, s_p);
    int64_t run_base = publish_and_look_back(agg, group_total, s_p);
    if (publishes_total()) publish_total(run_base + group_total, totals, total_host);
    for (int64_t tile = t0; tile < t1; ++tile) {
        int64_t v[SCAN_IPT];
        const int64_t mine = tile_load(c, n, tile, v);
        // tile_scan's body, written out: called as the shared step this loop needs 68 VGPRs instead of 64 (7 waves a SIMD instead
        // of 8, scratch only when forced down), which would also move resident_scan_workgroups() — measured with
        // -Rpass-analysis=kernel-resource-usage, both index types, whatever the barrier's place and however the step is split
        int64_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        __syncthreads(); // (s_w is reused)
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        int64_t wb = 0, tile_total = 0;
#pragma unroll
        for (int k = 0; k < SCAN_WAVES; ++k) {
            if (k < w) wb += s_w[k];
            tile_total += s_w[k];
        }
        tile_store(c, n, tile, v, run_base + wb + inc - mine);
        run_base += tile_total;
    }
}

// workgroups of SCAN_TPB threads the current device holds at once, halved (the margin for anything else that is running)
template <class I> static int64_t resident_scan_workgroups() {
    static thread_local int memo_dev = -1;
    static thread_local int64_t memo = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != memo_dev) {
        int ncu = 0, per_cu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 64;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)scan_fused_grouped_kernel<I>, SCAN_TPB, 0) != hipSuccess || per_cu <= 0) per_cu = 2;
        memo = (int64_t)ncu * per_cu / 2;
        if (memo < 16) memo = 16;
        memo_dev = dev;
    }
    return memo;
}

template <class I> int scan_counts(const ScanCall<I> &s, hipStream_t st) {
    const int64_t n = s.n, nparts = scan_tiles(n);
    int64_t *totals = s.total_dev ? s.total_dev : (int64_t *)s.scratch; // where the device-side total goes (header word 0)
    int64_t *partials = (int64_t *)((char *)s.scratch + SCAN_AGG_OFFSET);
    if (s.aggregates_zeroed && g_tuning.lvt_scan_fused != 0) {
        int64_t room = resident_scan_workgroups<I>();
        if (g_tuning.lvt_scan_fused > 1 && g_tuning.lvt_scan_fused < room) room = g_tuning.lvt_scan_fused; // (development knob: a smaller grid)
        if (nparts > room) {
            const int64_t per = ceil_div(nparts, room);
            IBVH_LAUNCH((scan_fused_grouped_kernel<I>), dim3((unsigned)ceil_div(nparts, per)), dim3(SCAN_TPB), 0, st, s.counts, n, (unsigned long long *)partials,
                        totals, s.total_host, (int)per, s.limit);
        } else {
            IBVH_LAUNCH((scan_fused_kernel<I>), dim3((unsigned)nparts), dim3(SCAN_TPB), 0, st, s.counts, n, (unsigned long long *)partials, totals,
                        s.total_host, s.limit);
        }
    } else {
        IBVH_LAUNCH((scan_reduce_kernel<I>), dim3((unsigned)nparts), dim3(SCAN_TPB), 0, st, s.counts, n, partials, s.limit);
        IBVH_LAUNCH((scan_apply_kernel<I>), dim3((unsigned)nparts), dim3(SCAN_TPB), 0, st, s.counts, n, partials, totals, s.total_host, s.limit);
    }
    IBVH_LAUNCH_CHECK();
    if (!s.total_out) return IBVH_OK; // *_enqueue: the total stays in the scratch header, nobody waits
    int64_t total = 0;
    IBVH_HIP_CHECK(hipMemcpyAsync(&total, totals, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    IBVH_HIP_CHECK(hipStreamSynchronize(st));
    *s.total_out = total;
    if (sizeof(I) == 4 && total > (int64_t)INT32_MAX) return IBVH_ERR_OVERFLOW;
    return IBVH_OK;
}

// (the binned ray path scans its per-ray item counts as int32_t whatever the index type)
template int scan_counts<int32_t>(const ScanCall<int32_t> &, hipStream_t);
#ifndef IBVH_ONLY_BENCH_TYPES
template int scan_counts<int64_t>(const ScanCall<int64_t> &, hipStream_t);
#endif

} // namespace lvt
} // namespace ibvh
