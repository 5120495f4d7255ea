// ibvh_msd_finish.inc — the finish kernel of the build's sort and its launcher, as templates: every cell of the partitioned
// records (and every window of sub-cells of a crowded cell) is sorted by one workgroup in LDS and written to its final place.
// Included by ibvh_msd_finish.hip, whose dispatcher instantiates the geometries of kFinish (ibvh_msd_impl.hpp) — see
// ibvh_msd.hip for the whole picture (replaces AK.sort!(leaves, by = bv -> bv.morton), reference src/build.jl:248-253).
// gfx950 only.
#include "ibvh_msd_impl.hpp"

namespace ibvh {
namespace msd {

template <class K, int TPB, int IPT> struct FinishLds {
    static constexpr int W = TPB / 64, CAP = TPB * IPT, RB = 8, R = 1 << RB;
    K *s_keys;            // CAP
    uint16_t *s_idx;      // CAP
    uint32_t *s_vals32;   // CAP / 2 (slow path: tiles of CAP / 2 keys + 32-bit positions in the same bytes)
    uint32_t *local_base; // R
    uint32_t *gbase;      // R
    uint32_t *wave_tot;   // 16
    uint16_t *whist;      // W * R
    // resident_off != 0 (the resident kernel): the 16-bit positions of the plain path — which then only serves the ranges too
    // large to be resident — live in the record area, so that the record area is as large as possible
    IBVH_D explicit FinishLds(unsigned char *p, uint32_t resident_off = 0) {
        s_keys = (K *)p;
        s_idx = resident_off ? (uint16_t *)(p + resident_off) : (uint16_t *)(s_keys + CAP);
        s_vals32 = (uint32_t *)(s_keys + CAP / 2);
        local_base = resident_off ? (uint32_t *)(s_keys + CAP) : (uint32_t *)(s_idx + CAP);
        gbase = local_base + R;
        wave_tot = gbase + R;
        whist = (uint16_t *)(wave_tot + 16);
    }
};

// records [start, start + m) of `part`, whose keys are key_base + (an nbits-bit number): sorted into out[start ...)
// The keys of m <= CAP records sorted in LDS, the records copied to dst in that order.  GATHER = false: the records are the m
// consecutive ones at `bucket`; GATHER = true (rescue path, merge_chunk): record idx of the sequence is record gather[idx]
// of `bucket` (the sequence order is what ties are broken by: the sort is stable).
template <class K, int TPB, int IPT, bool GATHER>
IBVH_D void finish_fast(const FinishArgs &fa, const FinishLds<K, TPB, IPT> &l, const char *bucket, char *dst_bytes, int64_t m, K key_base, int nbits,
                        const uint32_t *gather) {
    constexpr int W = TPB / 64;
    constexpr int RB = 8;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int stride = fa.lay.stride;
    const int passes = (nbits + RB - 1) / RB;
    // the m keys are dealt to the waves in equal contiguous shares of `chunk` (a multiple of 64): a range of
    // CAP/4 keys keeps every wave busy with a quarter of the ranking work; (w, j, lane) order is memory order
    const int chunk = (int)((m + W * 64 - 1) / (W * 64)) * 64;
    const int jmax = chunk / 64; // <= IPT
    K key[IPT];
    uint16_t val[IPT];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const int idx = w * chunk + j * 64 + lane;
        const bool ok = j < jmax && idx < m;
        // (the strided key loads touch every line of the range's records: they are L2 hits for the copy below;
        // sentinels sort last)
        int64_t at = idx;
        if constexpr (GATHER) at = ok ? (int64_t)gather[idx] : 0;
        key[j] = ok ? (K)((K)load_morton(bucket + at * stride, fa.lay) - key_base) : (K) ~(K)0;
        val[j] = (uint16_t)idx;
    }
    if (passes == 0) {
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const int idx = w * chunk + j * 64 + lane;
            if (j < jmax) l.s_idx[idx] = val[j];
        }
        __syncthreads();
    }
    int done = 0;
    IBVH_STAMP(1, 2);
    for (int p = 0; p < passes; ++p) {
        const int bits = (nbits - done + (passes - p) - 1) / (passes - p); // even split of the remaining bits
        lds_radix_pass<K, uint16_t, TPB, IPT, RB>(key, val, done, bits, jmax, l.s_keys, l.s_idx, l.local_base, l.wave_tot, l.whist);
        done += bits;
        if (p + 1 < passes) {
#pragma unroll
            for (int j = 0; j < IPT; ++j) {
                const int idx = w * chunk + j * 64 + lane;
                if (j < jmax) {
                    key[j] = l.s_keys[idx];
                    val[j] = l.s_idx[idx];
                }
            }
            __syncthreads();
        }
    }
    // records: lane <-> 8-byte word of the output range (fully coalesced stores; the loads hit the range's
    // partitioned records, which the key loads above have just pulled through L2)
    IBVH_STAMP(1, 3);
    const uint64_t *__restrict__ src = (const uint64_t *)bucket;
    uint64_t *__restrict__ dst = (uint64_t *)dst_bytes;
    const uint32_t total = (uint32_t)m * fa.words;
    constexpr int U = 8;
    for (uint32_t g0 = threadIdx.x; g0 < total; g0 += TPB * U) {
        uint64_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + u * TPB;
            const uint32_t gc = g < total ? g : 0u;
            const uint32_t r = __umulhi(gc, fa.inv_words);
            const uint32_t part_w = gc - r * fa.words;
            uint64_t from = (uint64_t)l.s_idx[r];
            if constexpr (GATHER) from = (uint64_t)gather[from];
            v[u] = src[from * fa.words + part_w];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + u * TPB;
            if (g < total) dst[g] = v[u];
        }
    }
    IBVH_STAMP(1, 4);
    __syncthreads(); // (the LDS arrays are reused by the workgroup's next range)
}

// A range with more records than one workgroup sorts in LDS, met by a finish workgroup although the caller launched too few
// partition levels for this input (an ABRUPT change of distribution inside a `cache=` chain: the hint that sizes the levels is
// one build old): registered for the kernel's rescue workgroups (rescue_loop below) instead of being sorted by this one
// workgroup alone (rounds 2 - 5: 118 ms for a 1e7-leaf cell).  One 64-bit atomic hands out the entry number and the range's
// first window number together, so entries are in window order.
// threadIdx.x == 0, but not as a loop-invariant the compiler can see: around a loop that holds barriers, LLVM threads the
// back edge through a loop-invariant `if (threadIdx.x == 0)` — thread 0 and the other lanes of its wave then run the loop body
// in separate passes, each executing the body's s_barrier (measured: the rescue loop's ticket; lane 0 of wave 0 ran a whole
// phase apart from the other 255 threads).  The empty asm makes the value opaque in every evaluation.
IBVH_D bool leader() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t == 0;
}

struct RescueEntry {
    uint32_t start, m, base, windows; // records [start, start + m) of buffer `buf`; windows [base, base + windows)
    uint64_t key_base;
    uint32_t nbits_buf;               // nbits | buf << 8
    uint32_t done_a;                  // windows sorted so far (phase A)
    uint64_t key_and, key_or;         // AND / OR of the range's keys (minus key_base), gathered by phase A: the merge's searches
    uint64_t pad[2];                  //   bisect only the bits that vary
};
static_assert(sizeof(RescueEntry) == 64, "carve_tables sizes the table by this");
constexpr int RS_ALLOC = 4, RS_TICKET = 6, RS_NORMAL_DONE = 7; // words of Tables::needed (zeroed by the plan / the first partition)
IBVH_D bool rescue_register(const Tables &tb, const FinishArgs &fa, int buf, int64_t start, int64_t m, uint64_t key_base, int nbits, uint32_t cap) {
    const uint32_t windows = (uint32_t)((m + cap - 1) / cap);
    if (!fa.rescuers || windows > cap) return false; // (no rescue workgroups; or more runs than the merge's LDS tables hold: n > cap^2)
    if (leader()) { // (called from loops over windows that hold barriers)
        const unsigned long long got = __hip_atomic_fetch_add((unsigned long long *)(tb.needed + RS_ALLOC), ((unsigned long long)1 << 32) | windows,
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        RescueEntry *e = (RescueEntry *)tb.rescue + (uint32_t)(got >> 32);
        e->start = (uint32_t)start;
        e->m = (uint32_t)m;
        e->base = (uint32_t)got;
        e->windows = windows;
        e->key_base = key_base;
        e->nbits_buf = (uint32_t)nbits | ((uint32_t)buf << 8);
        e->done_a = 0;
        e->key_and = ~(uint64_t)0;
        e->key_or = 0;
        __threadfence(); // the entry, before this workgroup is counted in (finish_kernel's epilogue): the only agent-scope
                         // release an ordinary workgroup ever pays — such a fence writes back the XCD's whole L2
    }
    return true;
}

// records [start, start + m) of `part`, whose keys are key_base + (an nbits-bit number): sorted into out_base[start ...)
template <class K, int TPB, int IPT, bool RES>
IBVH_D void finish_range(const Tables &tb, const FinishArgs &fa, const FinishLds<K, TPB, IPT> &l, const char *part, int64_t start, int64_t m, K key_base,
                         int nbits, char *out_base) {
    constexpr int W = TPB / 64;
    constexpr int CAP = TPB * IPT;
    constexpr int RB = 8, R = 1 << RB;
    static_assert(R <= TPB, "one digit counter per thread");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int stride = fa.lay.stride;
    const char *bucket = part + start * stride;
    const int passes = (nbits + RB - 1) / RB;
    IBVH_STAMP(1, 1);
    // ---- resident path (round 4): the range's RECORDS live in LDS.  The fast path below reads every record twice from
    // memory — the strided key loads pull the range's lines through L2, the gather by sorted position fetches them again
    // (and with 512 cells of ~117 KB in flight the second read often misses: FETCH_SIZE showed the records read ~2.8 x) —
    // here each record is read from memory exactly ONCE, coalesced, into LDS; the keys are taken from the LDS copy, sorted
    // as one 32-bit word (key - base) << IDXB | position (a stable LSD on the key bits only: the position rides along), and
    // the output is gathered out of LDS.  32-bit keys whose varying bits + IDXB fit 32 bits only.
    if constexpr (RES && sizeof(K) == 4) {
        constexpr int IDXB = 32 - __builtin_clz((unsigned)(CAP - 1)); // bits of a position inside the range
        if (m <= CAP && nbits + IDXB <= 32 && (uint32_t)m * fa.words <= fa.resident_words) {
            uint64_t *s_rec = (uint64_t *)((unsigned char *)l.s_keys + fa.resident_off);
            const uint64_t *__restrict__ src = (const uint64_t *)bucket;
            const uint32_t total = (uint32_t)m * fa.words;
            constexpr int U = 8;
            for (uint32_t g0 = threadIdx.x; g0 < total; g0 += TPB * U) {
                uint64_t v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t g = g0 + u * TPB;
                    v[u] = src[g < total ? g : 0u];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t g = g0 + u * TPB;
                    if (g < total) s_rec[g] = v[u];
                }
            }
            __syncthreads();
            IBVH_STAMP(1, 2);
            const int chunk = (int)((m + W * 64 - 1) / (W * 64)) * 64;
            const int jmax = chunk / 64; // <= IPT
            const uint32_t mw = (uint32_t)fa.lay.morton_off >> 3, msh = ((uint32_t)fa.lay.morton_off & 7u) * 8u;
            const uint32_t mmask = fa.lay.morton_bytes == 2 ? 0xffffu : 0xffffffffu;
            K key[IPT];
            const rsort::NoVal none[IPT] = {};
#pragma unroll
            for (int j = 0; j < IPT; ++j) {
                const int idx = w * chunk + j * 64 + lane;
                const bool ok = j < jmax && idx < m;
                const uint32_t k = (uint32_t)(s_rec[(uint32_t)(ok ? idx : 0) * fa.words + mw] >> msh) & mmask;
                key[j] = ok ? (K)(((k - (uint32_t)key_base) << IDXB) | (uint32_t)idx) : (K) ~(K)0; // sentinels sort last
            }
            if (passes == 0) {
#pragma unroll
                for (int j = 0; j < IPT; ++j) {
                    const int idx = w * chunk + j * 64 + lane;
                    if (j < jmax) l.s_keys[idx] = key[j];
                }
                __syncthreads();
            }
            int done = 0;
            for (int p = 0; p < passes; ++p) {
                const int bits = (nbits - done + (passes - p) - 1) / (passes - p);
                lds_radix_pass<K, rsort::NoVal, TPB, IPT, RB>(key, none, IDXB + done, bits, jmax, l.s_keys, (rsort::NoVal *)nullptr, l.local_base,
                                                              l.wave_tot, l.whist);
                done += bits;
                if (p + 1 < passes) {
#pragma unroll
                    for (int j = 0; j < IPT; ++j) {
                        const int idx = w * chunk + j * 64 + lane;
                        if (j < jmax) key[j] = l.s_keys[idx];
                    }
                    __syncthreads();
                }
            }
            IBVH_STAMP(1, 3);
            uint64_t *__restrict__ dst = (uint64_t *)(out_base + start * stride);
            for (uint32_t g0 = threadIdx.x; g0 < total; g0 += TPB * U) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t g = g0 + u * TPB;
                    if (g < total) {
                        const uint32_t r = __umulhi(g, fa.inv_words);
                        const uint32_t part_w = g - r * fa.words;
                        dst[g] = s_rec[((uint32_t)l.s_keys[r] & ((1u << IDXB) - 1u)) * fa.words + part_w];
                    }
                }
            }
            IBVH_STAMP(1, 4);
            __syncthreads(); // (the LDS arrays are reused by the workgroup's next range)
            return;
        }
    }
    if (m <= CAP) { // ---- fast path: the range's keys live in LDS
        finish_fast<K, TPB, IPT, false>(fa, l, bucket, out_base + start * stride, m, key_base, nbits, nullptr);
        return;
    }
    // ---- more records than the LDS holds: the kernel's rescue workgroups sort it window by window and merge (rescue_loop)
    if (rescue_register(tb, fa, part == fa.buf[0] ? 0 : 1, start, m, (uint64_t)key_base, nbits, (uint32_t)CAP)) return;

    // ---- slow path (what the rescue does not take: ranges of more than CAP^2 records, msd_rescue = 0): tiled LSD between the
    // two (key, position) arrays, by this one workgroup ----
    K *src_k = (K *)fa.kalt + start, *dst_k = (K *)fa.kpri + start;
    uint32_t *src_v = fa.valt + start, *dst_v = fa.vpri + start;
    for (int64_t i = threadIdx.x; i < m; i += TPB) {
        src_k[i] = (K)((K)load_morton(bucket + i * stride, fa.lay) - key_base);
        src_v[i] = (uint32_t)i;
    }
    __threadfence_block();
    __syncthreads();
    for (int p = 0; p < passes; ++p) {
        const int shift = RB * p;
        const int bits = nbits - shift < RB ? nbits - shift : RB;
        const uint32_t mask = (1u << bits) - 1u;
        if (threadIdx.x < R) l.gbase[threadIdx.x] = 0;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < m; i += TPB) atomicAdd(&l.gbase[(uint32_t)(src_k[i] >> shift) & mask], 1u);
        __syncthreads();
        lds_exclusive_scan<TPB>(l.gbase, R, l.wave_tot);
        constexpr int SIPT = IPT / 2, SCAP = CAP / 2;
        for (int64_t t0 = 0; t0 < m; t0 += SCAP) {
            const int64_t cnt = m - t0 < SCAP ? m - t0 : SCAP;
            K key[SIPT];
            uint32_t val[SIPT];
#pragma unroll
            for (int j = 0; j < SIPT; ++j) {
                const int idx = w * 64 * SIPT + j * 64 + lane;
                const bool ok = idx < cnt;
                key[j] = ok ? src_k[t0 + idx] : (K) ~(K)0;
                val[j] = ok ? src_v[t0 + idx] : 0u;
            }
            uint32_t tot_d;
            lds_radix_pass<K, uint32_t, TPB, SIPT, RB>(key, val, shift, bits, SIPT, l.s_keys, l.s_vals32, l.local_base, l.wave_tot, l.whist, &tot_d);
            for (int pos = threadIdx.x; pos < cnt; pos += TPB) {
                const K kk = l.s_keys[pos];
                const uint32_t d = (uint32_t)(kk >> shift) & mask;
                const uint32_t dest = l.gbase[d] + ((uint32_t)pos - l.local_base[d]);
                dst_k[dest] = kk;
                dst_v[dest] = l.s_vals32[pos];
            }
            __syncthreads();
            // sentinels of a partial tile were counted in the last digit: real count there = cnt - local_base
            if (threadIdx.x < R) {
                uint32_t real = tot_d;
                if ((int)threadIdx.x == (int)mask && cnt < SCAP) real = (uint32_t)cnt - l.local_base[mask];
                l.gbase[threadIdx.x] += real;
            }
            __syncthreads();
        }
        // make this pass's global writes visible to the next pass's reads (same workgroup, other lanes)
        __threadfence_block();
        __syncthreads();
        K *tk = src_k;
        src_k = dst_k;
        dst_k = tk;
        uint32_t *tv = src_v;
        src_v = dst_v;
        dst_v = tv;
    }
    // `src_v` holds the range's positions in sorted order
    const uint64_t *src = (const uint64_t *)bucket;
    uint64_t *dst = (uint64_t *)(out_base + start * stride);
    const uint64_t total = (uint64_t)m * fa.words;
    for (uint64_t g = threadIdx.x; g < total; g += TPB) {
        const uint64_t r = g / fa.words;
        const uint32_t part_w = (uint32_t)(g - r * fa.words);
        dst[g] = src[(uint64_t)src_v[r] * fa.words + part_w];
    }
    __syncthreads();
}

IBVH_D int bit_length(uint32_t v) { return v == 0 ? 0 : 32 - __builtin_clz(v); }
// workgroup-uniform values loaded through vector loads: moved to scalar registers (they are live across the sort)
IBVH_D uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
IBVH_D uint64_t uni(uint64_t v) { return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v); }

// ---- rescue: ranges larger than one workgroup's LDS sort, by ALL rescue workgroups (registered by rescue_register) ---------
// The range's windows of CAP records are sorted one by one (phase A: the ordinary in-LDS sort, into the OTHER record buffer,
// whose copy of the range is dead), then every CAP-record chunk of the output is merged from the W sorted runs (phase B):
// the split of every run at the chunk's first and last rank is found by bisection on the key bits (rank_split), the records
// between the splits — CAP of them, in run order — are sorted in LDS once more (stable: equal keys keep (run, position)
// order, i.e. source order) and written to their final place.  Work items are handed out by an atomic ticket, phase A items
// first: an item only ever waits for items with LOWER tickets, which are held by workgroups that are running (or done) — no
// assumption about the order in which the hardware starts workgroups.
template <class K> IBVH_D K rel_key(const char *base, uint32_t at, int stride, const LeafLayout &lay, K key_base) {
    return (K)((K)load_morton(base + (int64_t)at * stride, lay) - key_base);
}
// s_lo[i] <- how many records of run i (records [i * CAP, min(m, (i + 1) * CAP)) of `base`, sorted) are among the first r of
// the whole range in (key, run, position) order.  0 < r < m.  s_lo / s_hi / s_p: W 16-bit words each.  Every key of the range
// is v0 + (an nvar-bit number).  A thread owns q consecutive runs and walks their binary searches U at a time, so that U
// dependent chains of loads are in flight instead of one (the searches are latency: ~1 us a probe).
template <class K, int TPB, int CAP>
IBVH_D void rank_split(const FinishArgs &fa, const char *base, uint32_t m, uint32_t W, uint32_t r, K key_base, K v0, int nvar, uint16_t *s_lo,
                       uint16_t *s_hi, uint16_t *s_p, uint32_t *wave_tot) {
    constexpr int U = 8;
    const int stride = fa.lay.stride;
    const uint32_t q = (W + TPB - 1) / TPB, i0 = threadIdx.x * q, i1 = i0 + q < W ? i0 + q : W; // my runs: consecutive ones
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t len = m - i * CAP < (uint32_t)CAP ? m - i * CAP : (uint32_t)CAP;
        s_lo[i] = 0;
        s_hi[i] = (uint16_t)len; // (CAP <= 16,384)
    }
    // first position of run i in [s_lo[i], s_hi[i]) whose key is >= cand (OR_EQUAL: > cand) -> s_p[i]; returns their sum
    auto bounds = [&](K cand, bool or_equal) -> uint32_t {
        uint32_t sum = 0;
        for (uint32_t g = i0; g < i1; g += U) {
            uint32_t lo[U], hi[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool have = g + u < i1;
                lo[u] = have ? s_lo[g + u] : 0u;
                hi[u] = have ? s_hi[g + u] : 0u;
            }
            for (;;) {
                bool open = false;
                K key[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t mid = (lo[u] + hi[u]) >> 1;
                    if (lo[u] < hi[u]) {
                        key[u] = rel_key<K>(base, (g + u) * CAP + mid, stride, fa.lay, key_base);
                        open = true;
                    }
                }
                if (!open) break;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (lo[u] < hi[u]) {
                        const uint32_t mid = (lo[u] + hi[u]) >> 1;
                        const bool right = or_equal ? key[u] <= cand : key[u] < cand;
                        if (right) lo[u] = mid + 1;
                        else hi[u] = mid;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (g + u < i1) {
                    s_p[g + u] = (uint16_t)lo[u];
                    sum += lo[u];
                }
        }
        return sum;
    };
    K v = v0; // the largest key with (number of keys below it) <= r: the key of the record of rank r
    for (int b = nvar - 1; b >= 0; --b) {
        const K cand = (K)(v | ((K)1 << b));
        const uint32_t below = bounds(cand, false);
        uint32_t total;
        block_exclusive_scan<TPB>(below, wave_tot, &total);
        if (total <= r) {
            v = cand;
            for (uint32_t i = i0; i < i1; ++i) s_lo[i] = s_p[i];
        } else {
            for (uint32_t i = i0; i < i1; ++i) s_hi[i] = s_p[i];
        }
    }
    // records with key v: the first (r - below) of them in run order
    uint32_t below = 0;
    for (uint32_t i = i0; i < i1; ++i) below += s_lo[i];
    const uint32_t upper = bounds(v, true); // (s_hi: first key >= the smallest rejected candidate, which is > v)
    const uint32_t equal = upper - below;
    uint32_t total_below;
    block_exclusive_scan<TPB>(below, wave_tot, &total_below);
    uint32_t before = block_exclusive_scan<TPB>(equal, wave_tot, nullptr); // records with key v in the runs before mine
    const uint32_t want = r - total_below;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t eq = (uint32_t)s_p[i] - (uint32_t)s_lo[i];
        const uint32_t take = before >= want ? 0u : (want - before < eq ? want - before : eq);
        s_lo[i] = (uint16_t)(s_lo[i] + take);
        before += eq;
    }
}

// chunk j (records [j * CAP, min(m, (j + 1) * CAP)) of the sorted range) from the W sorted runs in `runs`; priv: 2 * CAP words
// of scratch that belong to this workgroup
template <class K, int TPB, int IPT>
IBVH_D void merge_chunk(const FinishArgs &fa, const FinishLds<K, TPB, IPT> &l, const char *runs, char *out_base, uint32_t start, uint32_t m, uint32_t j,
                        uint32_t W, K key_base, int nbits, K v0, int nvar, uint32_t *priv) {
    constexpr int CAP = TPB * IPT;
    static_assert(sizeof(K) >= 4 && CAP <= 16384, "two 16-bit tables in the key area; positions inside a run fit 16 bits");
    const int stride = fa.lay.stride;
    const char *base = runs + (int64_t)start * stride;
    uint16_t *s_lo = (uint16_t *)l.s_keys, *s_hi = s_lo + CAP, *s_p = l.s_idx;
    uint32_t *g_from = priv, *g_first = priv + CAP; // the chunk's records in (run, position) order; every run's first record of the chunk
    const uint32_t r0 = j * CAP, r1 = r0 + CAP < m ? r0 + CAP : m, mc = r1 - r0;
    const uint32_t q = (W + TPB - 1) / TPB, i0 = threadIdx.x * q, i1 = i0 + q < W ? i0 + q : W;
    if (r0 > 0) rank_split<K, TPB, CAP>(fa, base, m, W, r0, key_base, v0, nvar, s_lo, s_hi, s_p, l.wave_tot);
    for (uint32_t i = i0; i < i1; ++i) g_first[i] = r0 > 0 ? s_lo[i] : 0u; // (read back by this thread only)
    if (r1 < m) rank_split<K, TPB, CAP>(fa, base, m, W, r1, key_base, v0, nvar, s_lo, s_hi, s_p, l.wave_tot);
    uint32_t mine = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t len = m - i * CAP < (uint32_t)CAP ? m - i * CAP : (uint32_t)CAP;
        const uint32_t last = r1 < m ? s_lo[i] : len;
        s_p[i] = (uint16_t)last;
        mine += last - g_first[i];
    }
    uint32_t at = block_exclusive_scan<TPB>(mine, l.wave_tot, nullptr);
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t first = g_first[i], last = s_p[i];
        for (uint32_t x = first; x < last; ++x) g_from[at++] = i * CAP + x;
    }
    __threadfence_block(); // (g_from: written by one thread, read by others of this workgroup)
    __syncthreads();
    finish_fast<K, TPB, IPT, true>(fa, l, base, out_base + ((int64_t)start + r0) * stride, (int64_t)mc, key_base, nbits, g_from);
}

// every wave waits until *word >= target (an agent-scope counter other workgroups add to), then sees what they wrote before
// adding.  All lanes load the same word and the branch is on a scalar: the wait is uniform control flow for the compiler (a
// lane-0-only spin inside the ticket loop made it keep per-lane loop masks, and lane 0 of wave 0 ran apart from the others)
IBVH_D void spin_until(const uint32_t *word, uint32_t target) {
    while (uni(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < target) __builtin_amdgcn_s_sleep(8);
    __threadfence();
    __syncthreads();
}

template <class K, int TPB, int IPT, bool RES>
IBVH_D void rescue_loop(const Tables &tb, const FinishArgs &fa, const FinishLds<K, TPB, IPT> &l, uint32_t me) {
    constexpr int CAP = TPB * IPT;
    // every registration has been made once all the ordinary workgroups are through
    spin_until(tb.needed + RS_NORMAL_DONE, fa.normal_wgs);
    const unsigned long long alloc = __hip_atomic_load((unsigned long long *)(tb.needed + RS_ALLOC), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t entries = uni((uint32_t)(alloc >> 32)), windows = uni((uint32_t)alloc);
    if (windows == 0) return;
    RescueEntry *table = (RescueEntry *)tb.rescue;
    uint32_t *priv = fa.rescue_priv + (size_t)me * 2 * CAP;
    for (;;) {
        if (leader()) l.wave_tot[0] = __hip_atomic_fetch_add(tb.needed + RS_TICKET, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint32_t ticket = uni(l.wave_tot[0]);
        __syncthreads();
        if (ticket >= 2 * windows) return;
        const bool merge = ticket >= windows;
        const uint32_t u = merge ? ticket - windows : ticket;
        uint32_t a = 0, b = entries; // the entry whose windows hold u (entries are in window order)
        while (b - a > 1) {
            const uint32_t mid = (a + b) >> 1;
            if (uni(table[mid].base) <= u) a = mid;
            else b = mid;
        }
        RescueEntry *e = table + a;
        const uint32_t start = uni(e->start), m = uni(e->m), w = u - uni(e->base), W = uni(e->windows), nb = uni(e->nbits_buf);
        const K key_base = (K)uni(e->key_base);
        const int nbits = (int)(nb & 0xffu), buf = (int)(nb >> 8);
        const char *src = fa.buf[buf];
        char *other = const_cast<char *>(fa.buf[buf ^ 1]);
        if (!merge) {
            const uint32_t mw = m - w * CAP < (uint32_t)CAP ? m - w * CAP : (uint32_t)CAP;
            { // AND / OR of the window's keys (the loads pull the lines the sort reads next through L2)
                K ka = (K) ~(K)0, ko = 0;
                const char *wb = src + ((int64_t)start + (int64_t)w * CAP) * fa.lay.stride;
                for (uint32_t i = threadIdx.x; i < mw; i += TPB) {
                    const K k = rel_key<K>(wb, i, fa.lay.stride, fa.lay, key_base);
                    ka &= k;
                    ko |= k;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    ka &= (K)__shfl_xor(ka, o, 64);
                    ko |= (K)__shfl_xor(ko, o, 64);
                }
                if ((threadIdx.x & 63) == 0) {
                    __hip_atomic_fetch_and(&e->key_and, (uint64_t)ka | ~(uint64_t)(K) ~(K)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_or(&e->key_or, (uint64_t)ko, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            finish_range<K, TPB, IPT, RES>(tb, fa, l, src, (int64_t)start + (int64_t)w * CAP, (int64_t)mw, key_base, nbits, other);
            __threadfence(); // the window's records, for the merging workgroups (any CU, any XCD)
            __syncthreads();
            if (leader()) __hip_atomic_fetch_add(&e->done_a, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            spin_until(&e->done_a, W);
            // the bits that vary inside the range: the searches bisect those only (a tight cluster shares a long prefix)
            const uint64_t ka = uni(__hip_atomic_load(&e->key_and, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const uint64_t ko = uni(__hip_atomic_load(&e->key_or, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const uint64_t kmask = (uint64_t)(K) ~(K)0, x = (ka ^ ko) & kmask;
            const int nvar = x ? 64 - __builtin_clzll(x) : 0;
            const K v0 = nvar >= 64 ? (K)0 : (K)(((ka & kmask) >> nvar) << nvar);
            merge_chunk<K, TPB, IPT>(fa, l, other, fa.out, start, m, w, W, key_base, nbits, v0, nvar, priv);
        }
    }
}

// grid = R + F2 + H workgroups: workgroup b < R finishes cell b (unless it became a segment); the next F2 stride over the
// tiles of every extra level: tile t of segment k finishes the window of sub-cells that START inside records
// [t * tile, (t + 1) * tile) of the segment (consecutive sub-cells: one LDS sort with the sub-cell number as the top
// bits); a window that does not fit is finished sub-cell by sub-cell, skipping those the next level took.  The last H are the
// rescue workgroups: they leave at once unless the input may hold a range that is too large for one workgroup although no
// partition level is left to split it (`needed` above the launched levels) — then they wait for the others and share those ranges.
template <class K, int TPB, int IPT, bool RES>
IBVH_D void finish_ordinary(const Tables &tb, int radix, const FinishArgs &fa, const FinishLds<K, TPB, IPT> &l) {
    if ((int)blockIdx.x < radix) {
        const uint32_t d = blockIdx.x;
        const uint32_t start = uni(tb.cell_start[d]), m = uni(tb.cell_start[d + 1]) - start;
        if (m == 0 || (m > fa.cap && fa.levels > 0)) return; // (crowded cells are finished window by window below)
        if (fa.eq_key_bits) {
            K lo;
            int nb;
            cell_range<K>(tb, d, radix, fa.eq_key_bits, &lo, &nb);
            finish_range<K, TPB, IPT, RES>(tb, fa, l, fa.buf[0], (int64_t)start, (int64_t)m, (K)uni(lo), __builtin_amdgcn_readfirstlane(nb), fa.out);
            return;
        }
        finish_range<K, TPB, IPT, RES>(tb, fa, l, fa.buf[0], (int64_t)start, (int64_t)m, (K)((K)d << fa.shift1), fa.shift1, fa.out);
        return;
    }
    constexpr int C = 1 << L2_BITS;
    const uint32_t striders = fa.normal_wgs - (uint32_t)radix;
    for (int li = 0; li < fa.levels; ++li) {
        const Level L = tb.lvl[li];
        const uint32_t ntiles = uni(L.hdr[1]);
        const char *buf = fa.buf[(li + 1) & 1];
        const bool handed_down = li + 1 < fa.levels; // crowded sub-cells are segments of the next level
        for (uint32_t t = blockIdx.x - radix; t < ntiles; t += striders) {
            const uint32_t k = uni(L.tile_seg[t]);
            const uint64_t ka = uni(L.seg_and[k]), ko = uni(L.seg_or[k]);
            const Digit dg = level_digit(ka, ko);
            if (dg.terminal) continue; // the partition wrote the segment to `out`, sorted
            const uint32_t *ssp = L.sub_start + (int64_t)k * (C + 1);
            auto ss = [&](uint32_t i) { return uni(ssp[i]); };
            const uint32_t count = uni(L.seg_count[k]), reps = segment_reps(count, fa.tile);
            const uint32_t t_in_seg = t - uni(L.seg_tile[k]);
            for (uint32_t sub = 0; sub < reps; ++sub) {
            const uint32_t lo = (t_in_seg * reps + sub) * fa.tile, hi = lo + fa.tile;
            if (lo >= count) break;
            // e0 = first sub-cell starting at or after lo, e1 = first one starting at or after hi (binary searches; the
            // whole workgroup walks the same path)
            uint32_t e0 = 0, e1 = 0;
            {
                uint32_t a = 0, b = C; // first e with ss[e] >= lo
                while (a < b) {
                    const uint32_t mid = (a + b) >> 1;
                    if (ss(mid) < lo) a = mid + 1;
                    else b = mid;
                }
                e0 = a;
                a = e0, b = C;
                while (a < b) {
                    const uint32_t mid = (a + b) >> 1;
                    if (ss(mid) < hi) a = mid + 1;
                    else b = mid;
                }
                e1 = a;
            }
            if (e0 == e1) continue; // no sub-cell starts in this window (a large one covers it)
            if (ss(e1) == ss(e0)) continue; // empty sub-cells only
            const int64_t seg0 = (int64_t)uni(L.seg_start[k]);
            const K prefix = (K)common_prefix(ka, ko);
            // runs of consecutive sub-cells that fit one LDS sort (normally the whole window), one sort each; a single
            // crowded sub-cell is a segment of the next level — or, after the last level, takes the slow path
            for (uint32_t e = e0; e < e1;) {
                const uint32_t s0 = ss(e);
                uint32_t f = e + 1;
                const bool crowded = ss(f) - s0 > fa.cap;
                if (!crowded) { // the largest f <= e1 with ss(f) - s0 <= cap (ss ascends: binary search, usually f = e1 at once)
                    if (ss(e1) - s0 <= fa.cap) {
                        f = e1;
                    } else {
                        uint32_t lo_f = f, hi_f = e1; // ss(lo_f) fits, ss(hi_f) does not
                        while (hi_f - lo_f > 1) {
                            const uint32_t mid = (lo_f + hi_f) >> 1;
                            if (ss(mid) - s0 <= fa.cap) lo_f = mid;
                            else hi_f = mid;
                        }
                        f = lo_f;
                    }
                }
                const uint32_t m = ss(f) - s0;
                if (m != 0 && !(crowded && handed_down))
                    finish_range<K, TPB, IPT, RES>(tb, fa, l, buf, seg0 + s0, (int64_t)m, (K)(prefix + ((K)e << dg.shift)),
                                              dg.shift + bit_length(f - e - 1), fa.out);
                e = f;
            }
            } // sub
        }
    }
}

template <class K, int TPB, int IPT, bool RES = false>
__global__ __launch_bounds__(TPB) void finish_kernel(Tables tb, int radix, FinishArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
    const FinishLds<K, TPB, IPT> l(bsm, RES ? fa.resident_off : 0u);
    IBVH_STAMP(1, 0);
    if (blockIdx.x == 0 && threadIdx.x == 0 && fa.skew_flag)
        *fa.skew_flag = (int32_t)(tb.needed[0] | (tb.needed[1] << 8) |
                                  (fa.eq_key_bits ? (1u << 18) | ((tb.needed[2] & 1u) << 16) | (fa.levels > 0 ? (tb.needed[3] & 1u) << 17 : 0u) : 0u));
    // may a range have stayed too large for one workgroup?  (`needed`: the levels this input would have used, capped at MAX_LEVELS)
    const bool may_crowd = fa.rescuers && (uni(tb.needed[0]) > (uint32_t)fa.levels || fa.levels >= MAX_LEVELS);
    if (blockIdx.x >= fa.normal_wgs) {
        if (may_crowd) rescue_loop<K, TPB, IPT, RES>(tb, fa, l, blockIdx.x - fa.normal_wgs);
        return;
    }
    finish_ordinary<K, TPB, IPT, RES>(tb, radix, fa, l);
    // this workgroup's registrations (made by its thread 0, each behind a fence of its own) are in: count it in
    if (may_crowd && threadIdx.x == 0) __hip_atomic_fetch_add(tb.needed + RS_NORMAL_DONE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class K, int TPB, int IPT> constexpr size_t finish_smem() {
    return (size_t)TPB * IPT * (sizeof(K) + 2) + 2 * 256 * 4 + 64 + (size_t)(TPB / 64) * 256 * 2 + 64;
}

template <class K, int FT, int FI, bool RES>
int launch_finish(const Plan &p, const Tables &tb, const FinishArgs &fa_in, hipStream_t st) {
    FinishArgs fa = fa_in;
    size_t smem = finish_smem<K, FT, FI>();
    // resident geometry (kFinish): room for a full range of records behind the sort's arrays, as long as the workgroup
    // stays within the LDS (what does not fit takes the plain path)
    if constexpr (RES) {
        static_assert(sizeof(K) == 4, "the resident finish keeps 32-bit keys");
        const size_t cap = (size_t)FT * FI;
        const size_t off = (size_t)align_up((int64_t)(smem - cap * 2), 16); // (no 16-bit positions in front of the record area)
        size_t rec = cap * (size_t)fa.lay.stride;  // a full range, or what the LDS leaves (larger ranges take the plain path)
        if (off + rec > (size_t)kMaxLds) rec = (size_t)kMaxLds > off ? (((size_t)kMaxLds - off) / 8) * 8 : 0;
        if (rec >= cap * 2 && rec >= 1024 * (size_t)fa.lay.stride) {
            fa.resident_off = (uint32_t)off;
            fa.resident_words = (uint32_t)(rec / 8);
            smem = off + rec;
        }
    }
    const int f2 = fa.levels <= 0 ? 0 : (p.max_tiles2 < 1024 ? p.max_tiles2 : 1024); // workgroups that stride over the extra levels' windows
    fa.normal_wgs = (uint32_t)p.radix() + (uint32_t)f2;
    // the kernel (resident: a kernel of its own, the resident branch must not cost the plain one registers), then its launch
    auto launch = [&](auto resident) -> int {
        const void *kernel = (const void *)finish_kernel<K, FT, FI, decltype(resident)::value>;
        IBVH_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
        // the rescue workgroups WAIT for the ordinary ones: never more of them than HALF the workgroups of this kernel the device
        // holds at once (whatever order the hardware starts workgroups in, the ordinary ones then always find room to run)
        if (fa.rescuers) {
            struct Memo { // (per host thread: the queries cost microseconds, a build is on the host's critical path)
                const void *kernel;
                size_t smem;
                int dev;
                uint32_t room;
            };
            static thread_local Memo memo{nullptr, 0, -1, 0};
            int dev = 0;
            IBVH_HIP_CHECK(hipGetDevice(&dev));
            if (memo.kernel != kernel || memo.smem != smem || memo.dev != dev) {
                int ncu = 0, per_cu = 0;
                IBVH_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
                IBVH_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, FT, smem));
                memo = Memo{kernel, smem, dev, (uint32_t)((int64_t)ncu * (per_cu > 0 ? per_cu : 1) / 2)};
            }
            if (fa.rescuers > memo.room) fa.rescuers = memo.room;
        }
        IBVH_LAUNCH((finish_kernel<K, FT, FI, decltype(resident)::value>), dim3(fa.normal_wgs + fa.rescuers), dim3(FT), smem, st, tb, p.radix(), fa);
        return IBVH_OK;
    };
    if constexpr (RES)
        if (fa.resident_words) return launch(std::bool_constant<true>{});
    return launch(std::bool_constant<false>{});
}


} // namespace msd
} // namespace ibvh
