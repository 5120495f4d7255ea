// ibvh_build.hip — BVH construction on gfx950: extrema -> Morton keys -> stable sort of the records -> bottom-up merge.
// Replaces src/build.jl:198-271 and src/morton/*.jl of the reference.  Here: the extrema and the keys, the scratch carve, the
// choice of the sort and the build driver; the sorts are ibvh_msd.hip / ibvh_sort.hip, the merge is ibvh_aggregate.hip.
//
// Data flow (BSphere{F32} leaves, n of them; bytes per leaf in brackets):
//   extrema_partial   read volumes [16]                         -> per-workgroup min/max
//   encode_hist       folds the partials + epsilon expansion    -> 6 scalars in HBM (no host readback; above 2^21 leaves
//                     a one-workgroup extrema_final does it), read volumes [16], write key [4] (values are implicit
//                     positions), and counts the sort's first digit per tile
//   sort              n >= 4,096: ibvh_msd.hip — ONE partition of the finished records by the top bits of their key
//                     (read key [4] + volume [16 random], write record [24]), every cell finished in LDS [24 + 24]
//                     n <  4,096: ibvh_sort.hip — (key, position) pairs; the last pass writes the records
//   aggregate         ibvh_aggregate.hip
#include "ibvh_common.hpp"
#include "ibvh_aggregate.hpp"
#include "ibvh_radix.hpp"
#include "ibvh_msd.hpp"
#include "ibvh_sort.hpp"

namespace ibvh {
namespace build {

constexpr int EXT_TPB = 256;
constexpr int EXT_MAX_BLOCKS = 2048;
constexpr int EXT_FOLD_BLOCKS = 512; // ibvh_build: the partials are folded by every encode workgroup (ExtremaFold)

// ------------------------------------------------------------------------------------------
// M1: extrema of the centres — morton/utils.jl:1-72
// ------------------------------------------------------------------------------------------
template <class T> IBVH_D T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        T t = __shfl_xor(v, o, 64);
        v = v < t ? v : t;
    }
    return v;
}
template <class T> IBVH_D T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        T t = __shfl_xor(v, o, 64);
        v = v > t ? v : t;
    }
    return v;
}

// Six running extrema (three minima, three maxima) through a workgroup of `waves` waves: every wave reduces its lanes, lane 0
// hands the six results over in row `w` of `s`, and behind the one barrier thread k < 6 folds value k of all rows into `v`
// (minimum k on thread k, maximum k on thread 3 + k).  True on those six threads.
template <class T> IBVH_D bool fold_extrema(const T mn[3], const T mx[3], T (*s)[6], int waves, T &v) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T a = wave_min(mn[k]), b = wave_max(mx[k]);
        if (lane == 0) {
            s[w][k] = a;
            s[w][3 + k] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x >= 6) return false;
    v = s[0][threadIdx.x];
    for (int i = 1; i < waves; ++i) {
        T t = s[i][threadIdx.x];
        v = threadIdx.x < 3 ? (v < t ? v : t) : (v > t ? v : t);
    }
    return true;
}
// A thread's share of the per-workgroup partial extrema (extrema_partial_kernel): every `step`-th of `nparts`
template <class T> IBVH_D void take_partials(const T *__restrict__ partials, int nparts, int step, T mn[3], T mx[3]) {
    for (int i = threadIdx.x; i < nparts; i += step) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T a = partials[i * 6 + k], b = partials[i * 6 + 3 + k];
            mn[k] = mn[k] < a ? mn[k] : a;
            mx[k] = mx[k] > b ? mx[k] : b;
        }
    }
}

// min/max are exact and order-free (no NaNs), so any reduction tree reproduces the reference's
// mapreduce bit for bit.  Inits: min <- floatmax(T); max <- floatmin(T) (sic, utils.jl:39-40).
template <class V>
__global__ __launch_bounds__(EXT_TPB) void extrema_partial_kernel(const char *__restrict__ recs, int64_t stride, int64_t n,
                                                                  typename V::elt *__restrict__ partials) {
    using T = typename V::elt;
    T mn[3] = {float_max<T>(), float_max<T>(), float_max<T>()};
    T mx[3] = {float_min_normal<T>(), float_min_normal<T>(), float_min_normal<T>()};
    for (int64_t i = (int64_t)blockIdx.x * EXT_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EXT_TPB) {
        V v = load_vol<V>(recs + i * stride);
        T c[3];
        center(v, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = mn[k] < c[k] ? mn[k] : c[k];
            mx[k] = mx[k] > c[k] ? mx[k] : c[k];
        }
    }
    __shared__ T s[EXT_TPB / 64][6];
    T v;
    if (fold_extrema(mn, mx, s, EXT_TPB / 64, v)) partials[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
}

// compute_skips! on device memory (build.jl:232-239), folded into whichever single-workgroup kernel the build launches
// first (one launch less than a kernel of its own)
struct SkipsOut {
    TreeDev tree;
    void *skips; // nullptr: nothing to write
    int index_bytes;
};
IBVH_D void write_skips(const SkipsOut &so) {
    const int64_t level = (int64_t)threadIdx.x + 1;
    if (so.skips == nullptr || level > so.tree.levels) return;
    const int64_t v = level_skips(so.tree.levels, so.tree.virtual_leaves, level);
    if (so.index_bytes == 4) ((int32_t *)so.skips)[level - 1] = (int32_t)v;
    else ((int64_t *)so.skips)[level - 1] = v;
}

// One workgroup folds the partials and applies the epsilon expansion of bounding_volumes_extrema (expand_bound).
template <class T>
__global__ __launch_bounds__(EXT_TPB) void extrema_final_kernel(const T *__restrict__ partials, int nparts, int expand,
                                                                T *__restrict__ out, T *__restrict__ out2, SkipsOut so) {
    write_skips(so);
    T mn[3] = {float_max<T>(), float_max<T>(), float_max<T>()};
    T mx[3] = {float_min_normal<T>(), float_min_normal<T>(), float_min_normal<T>()};
    take_partials(partials, nparts, EXT_TPB, mn, mx);
    __shared__ T s[EXT_TPB / 64][6];
    T v;
    if (fold_extrema(mn, mx, s, EXT_TPB / 64, v)) {
        if (expand) v = expand_bound(v, threadIdx.x < 3);
        out[threadIdx.x] = v;
        if (out2) out2[threadIdx.x] = v; // the caller's copy (ibvh_build's extrema_out): no separate 24-byte memcpy
    }
}

template <class T> __global__ void extrema_set_kernel(T *out, T *out2, double a0, double a1, double a2, double b0, double b1, double b2, SkipsOut so) {
    write_skips(so);
    if (threadIdx.x == 0) {
        out[0] = T(a0);
        out[1] = T(a1);
        out[2] = T(a2);
        out[3] = T(b0);
        out[4] = T(b1);
        out[5] = T(b2);
        if (out2)
            for (int k = 0; k < 6; ++k) out2[k] = out[k];
    }
}

// ------------------------------------------------------------------------------------------
// M2: Morton keys — morton/default.jl:63-108
// ------------------------------------------------------------------------------------------
template <class V, class K>
__global__ __launch_bounds__(256) void encode_kernel(const char *__restrict__ recs, int64_t stride, int64_t n,
                                                     const typename V::elt *__restrict__ ext, int morton_type,
                                                     K *__restrict__ keys) {
    using T = typename V::elt;
    const T mins[3] = {ext[0], ext[1], ext[2]}, maxs[3] = {ext[3], ext[4], ext[5]};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        V v = load_vol<V>(recs + i * stride);
        T c[3];
        center(v, c);
        keys[i] = (K)morton_encode_single(c, mins, maxs, morton_type);
    }
}

// Same, fused with the radix sort's first per-tile digit histogram: the workgroup encodes exactly the
// keys of one sort tile and counts their lowest digit in LDS, so the sort's first hist pass (a 4 B/leaf
// re-read of the keys plus a launch) disappears.
// The fold of the extrema partials rides along (ExtremaFold): every workgroup folds the <= EXT_FOLD_BLOCKS partial results
// itself (a few KB of L2 hits) and applies the epsilon expansion — the identical operations in every workgroup, min / max
// being order-free — instead of waiting for a one-workgroup launch in between (extrema_final_kernel: ~6 us of pure
// launch / dependency latency at 1e6 leaves); workgroup 0 also publishes the result (the build's `extrema` output) and
// writes the skips.
template <class T> struct ExtremaFold {
    const T *partials; // nullptr: `ext` already holds the bounds
    int nparts;
    T *out, *out2;
    SkipsOut so;
};
template <class V, class K>
__global__ __launch_bounds__(1024) void encode_hist_kernel(const char *__restrict__ recs, int64_t stride, int64_t n,
                                                          const typename V::elt *__restrict__ ext, int morton_type,
                                                          K *__restrict__ keys, int tile_elems, int shift, uint32_t mask,
                                                          uint32_t *__restrict__ tile_hist, int num_tiles, int tile_major,
                                                          ExtremaFold<typename V::elt> fold) {
    using T = typename V::elt;
    extern __shared__ uint32_t h[]; // mask + 1 counters
    __shared__ T s_fold[16][6];
    __shared__ T s_ext[6];
    for (int i = threadIdx.x; i <= (int)mask; i += blockDim.x) h[i] = 0;
    if (fold.partials != nullptr) {
        if (blockIdx.x == 0) write_skips(fold.so);
        T mn[3] = {float_max<T>(), float_max<T>(), float_max<T>()};
        T mx[3] = {float_min_normal<T>(), float_min_normal<T>(), float_min_normal<T>()};
        take_partials(fold.partials, fold.nparts, (int)blockDim.x, mn, mx);
        T v;
        if (fold_extrema(mn, mx, s_fold, (int)(blockDim.x >> 6), v)) {
            v = expand_bound(v, threadIdx.x < 3);
            s_ext[threadIdx.x] = v;
            if (blockIdx.x == 0) {
                fold.out[threadIdx.x] = v;
                if (fold.out2) fold.out2[threadIdx.x] = v;
            }
        }
    }
    __syncthreads();
    const T *bounds = fold.partials != nullptr ? s_ext : ext;
    const T mins[3] = {bounds[0], bounds[1], bounds[2]}, maxs[3] = {bounds[3], bounds[4], bounds[5]};
    const int64_t base = (int64_t)blockIdx.x * tile_elems;
    for (int j = threadIdx.x; j < tile_elems; j += blockDim.x) {
        const int64_t i = base + j;
        if (i < n) {
            V v = load_vol<V>(recs + i * stride);
            T c[3];
            center(v, c);
            const K k = (K)morton_encode_single(c, mins, maxs, morton_type);
            keys[i] = k;
            atomicAdd(&h[(uint32_t)(k >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    // digit-major ([digit][tile]) for the LSD passes of ibvh_sort.hip, tile-major ([tile][digit], one coalesced row)
    // for the MSD partition of ibvh_msd.hip
    if (tile_major)
        for (int d = threadIdx.x; d <= (int)mask; d += blockDim.x) tile_hist[(int64_t)blockIdx.x * (mask + 1) + d] = h[d];
    else
        for (int d = threadIdx.x; d <= (int)mask; d += blockDim.x) tile_hist[(int64_t)d * num_tiles + blockIdx.x] = h[d];
}

inline int grid_for(int64_t n, int tpb, int max_blocks) {
    int64_t b = ceil_div(n, tpb);
    return (int)(b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

// scratch carve-up -----------------------------------------------------------------------------
struct Scratch {
    char *partials;  // EXT_MAX_BLOCKS * 6 * 8
    char *extrema;   // 6 * 8
    char *keys, *keys_alt; // n * key_bytes
    char *vals, *vals_alt; // n * 4
    char *records;   // n * leaf_bytes: the partitioned records (and the staging of an in-place pair-sort build)
    char *records2;  // n * leaf_bytes: second partition level (oversized cells only)
    char *sort;      // rsort::scratch_bytes(n)
    size_t total;
};
inline Scratch carve(char *base, int64_t n, int key_bytes, int64_t leaf_bytes, int morton_type) {
    Scratch s;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += (size_t)align_up((int64_t)bytes, 256);
        return p;
    };
    s.partials = take((size_t)EXT_MAX_BLOCKS * 6 * 8);
    s.extrema = take(64);
    s.keys = take((size_t)n * key_bytes);
    s.keys_alt = take((size_t)n * key_bytes);
    s.vals = take((size_t)n * 4);
    s.vals_alt = take((size_t)n * 4);
    s.records = take((size_t)n * leaf_bytes);
    s.records2 = take((size_t)n * leaf_bytes);
    const size_t a = rsort::scratch_bytes(n), b = msd::scratch_bytes(n, key_bits(morton_type), key_bytes, (int)leaf_bytes);
    s.sort = take(a > b ? a : b);
    s.total = off;
    return s;
}

// the first half alone: per-workgroup partial extrema for a consumer that folds them itself (encode_hist_kernel)
template <class V> int extrema_partials(const char *recs, int64_t stride, int64_t n, char *partials, hipStream_t st, int *nparts) {
    using T = typename V::elt;
    const int blocks = grid_for(n, EXT_TPB * 4, EXT_FOLD_BLOCKS);
    IBVH_LAUNCH((extrema_partial_kernel<V>), dim3(blocks), dim3(EXT_TPB), 0, st, recs, stride, n, (T *)partials);
    *nparts = blocks;
    return IBVH_OK;
}
template <class V>
int extrema(const char *recs, int64_t stride, int64_t n, int expand, typename V::elt *out, char *partials, hipStream_t st,
            typename V::elt *out2 = nullptr, SkipsOut so = SkipsOut{TreeDev{0, 0, 0}, nullptr, 4}) {
    using T = typename V::elt;
    int blocks = grid_for(n, EXT_TPB * 4, EXT_MAX_BLOCKS);
    IBVH_LAUNCH((extrema_partial_kernel<V>), dim3(blocks), dim3(EXT_TPB), 0, st, recs, stride, n, (T *)partials);
    IBVH_LAUNCH((extrema_final_kernel<T>), dim3(1), dim3(EXT_TPB), 0, st, (const T *)partials, blocks, expand, out, out2, so);
    IBVH_LAUNCH_CHECK();
    return IBVH_OK;
}

template <class V>
int encode(const char *recs, int64_t stride, int64_t n, const typename V::elt *ext, int morton_type, void *keys, hipStream_t st) {
    int blocks = grid_for(n, 256, 256 * 16);
    return dispatch_key(key_bytes(morton_type), [&](auto kt) -> int {
        using K = typename decltype(kt)::type;
        IBVH_LAUNCH((encode_kernel<V, K>), dim3(blocks), dim3(256), 0, st, recs, stride, n, ext, morton_type, (K *)keys);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    });
}

// ------------------------------------------------------------------------------------------
// ibvh_build: extrema -> keys + the sort's first tile histogram -> sort -> merge
// ------------------------------------------------------------------------------------------
// What ibvh_build has checked and derived from its arguments: the same for every leaf / node type
struct BuildCall {
    const ibvh_build_desc *desc;
    ibvh_layout lay;
    LeafLayout dlay;
    ibvh_tree tree;
    Scratch sc;
    int64_t n;
    int key_bytes, key_bits;
    const char *src;        // raw volumes, or the source records of an already wrapped build
    int64_t src_stride;
    bool wrapped, in_place; // in_place: already wrapped, volumes == NULL: the caller's `leaves` are source and destination
    void *leaves, *nodes, *skips, *extrema_out;
    hipStream_t st;
};

// The sort of one build, chosen once: the record sort (ibvh_msd.hip) takes every build of 4,096 leaves or more, the pair
// sort (ibvh_sort.hip) the smaller ones.  Both plans live in the sort region of the scratch (carve()).
struct SortRoute {
    msd::Plan records;      // bits != 0: the record sort
    msd::Tables tables;     // ... and its tables in the sort scratch
    rsort::PairsPlan pairs; // otherwise
    // The per-tile histogram the route's first pass expects from the key encoder: a workgroup of `tpb` threads per tile of
    // `tile_elems` keys counts the digit (key >> shift) & mask; tile-major rows for the record sort, digit-major for the pairs.
    int tpb, tile_elems, num_tiles, shift, tile_major;
    uint32_t mask, *tile_hist;
    bool by_records() const { return records.bits != 0; }
};
inline SortRoute choose_route(int64_t n, int key_bits, int key_bytes, int leaf_bytes, void *sort_scratch) {
    SortRoute r{};
    r.records = msd::plan_records(n, key_bits, key_bytes, leaf_bytes);
    if (r.by_records()) {
        const msd::Plan &p = r.records;
        r.tables = msd::bind_tables(p, sort_scratch);
        r.tpb = p.part.tpb, r.tile_elems = p.tile(), r.num_tiles = p.num_tiles, r.shift = p.shift, r.tile_major = 1;
        r.mask = (uint32_t)p.radix() - 1u, r.tile_hist = r.tables.tile_hist;
    } else {
        const rsort::PairsPlan &p = r.pairs = rsort::plan_pairs(n, key_bits, key_bytes, sort_scratch);
        r.tpb = p.tile.tpb, r.tile_elems = p.tile.tile(), r.num_tiles = p.num_tiles, r.shift = p.shift, r.tile_major = 0;
        r.mask = p.mask, r.tile_hist = p.tile_hist;
    }
    return r;
}

// Extrema of the centres (or the caller's fixed bounds: morton/default.jl:52-57) and the skips: whatever is left for the
// key encoder to do comes back in `fold`.
template <class L> int launch_extrema(const BuildCall &b, ExtremaFold<typename L::elt> &fold) {
    using T = typename L::elt;
    T *ext = (T *)b.sc.extrema;
    const SkipsOut so{tree_dev(b.tree), b.skips, index_bytes(b.desc->types.index_type)};
    fold = ExtremaFold<T>{nullptr, 0, ext, (T *)b.extrema_out, so};
    // Small builds are launch-latency bound: the encode kernel's workgroups fold the partial extrema themselves (one
    // launch less on the critical path: -6 us at 1e6 leaves).  With thousands of encode workgroups the redundant folds
    // cost more than the launch they save (1e7 leaves: encode 35 -> 45 us), so large builds keep the one-workgroup fold.
    const bool fold_in_encode = b.n <= (int64_t)1 << 21;
    if (b.desc->compute_extrema && fold_in_encode) {
        int nparts = 0;
        if (int e = extrema_partials<L>(b.src, b.src_stride, b.n, b.sc.partials, b.st, &nparts)) return e;
        fold.partials = (const T *)b.sc.partials;
        fold.nparts = nparts;
    } else if (b.desc->compute_extrema) {
        if (int e = extrema<L>(b.src, b.src_stride, b.n, 1, ext, b.sc.partials, b.st, (T *)b.extrema_out, so)) return e;
    } else {
        const double *mn = b.desc->mins, *mx = b.desc->maxs;
        IBVH_LAUNCH((extrema_set_kernel<T>), dim3(1), dim3(64), 0, b.st, ext, (T *)b.extrema_out, mn[0], mn[1], mn[2], mx[0], mx[1],
                    mx[2], so);
    }
    return IBVH_OK;
}

// Morton keys, fused with the first per-tile digit histogram of the sort
template <class L> int launch_keys(const BuildCall &b, const SortRoute &h, const ExtremaFold<typename L::elt> &fold) {
    using T = typename L::elt;
    return dispatch_key(b.key_bytes, [&](auto kt) -> int {
        using K = typename decltype(kt)::type;
        IBVH_LAUNCH((encode_hist_kernel<L, K>), dim3(h.num_tiles), dim3(h.tpb), ((size_t)h.mask + 1) * 4, b.st, b.src, b.src_stride,
                    b.n, (const T *)b.sc.extrema, b.desc->types.morton_type, (K *)b.sc.keys, h.tile_elems, h.shift, h.mask,
                    h.tile_hist, h.num_tiles, h.tile_major, fold);
        IBVH_LAUNCH_CHECK();
        return IBVH_OK;
    });
}

// The records in Morton order into `leaves` (index = position + 1 for fresh volumes, build.jl:345-349, or the source
// record's own index, :220-222).
//   record sort: ONE partition of the finished records into scratch by the top bits of their key, cells finished in LDS
//                into `leaves` (an in-place build reads `leaves`, stages in scratch and writes `leaves`: no extra copy)
//   pair sort:   stable sort of (key, position); the last pass writes the records — into scratch for an in-place build,
//                which then copies them back
inline int sort_records(const BuildCall &b, const SortRoute &route) {
    const ibvh_build_desc &d = *b.desc;
    const Scratch &sc = b.sc;
    char *dst = (route.by_records() || b.in_place) ? sc.records : (char *)b.leaves;
    const rsort::RecordArgs ra{b.src, dst, b.src_stride, b.wrapped ? 1 : 0, (int32_t)(b.lay.volume_bytes / 8),
                               index_bytes(d.types.index_type), b.dlay};
    if (route.by_records()) {
        if (int e = msd::sort_records(route.records, route.tables, b.key_bytes, b.key_bits, sc.keys, ra, sc.records2, (char *)b.leaves,
                                      sc.keys_alt, (uint32_t *)sc.vals_alt, sc.keys, (uint32_t *)sc.vals, d.sort_levels,
                                      d.sort_equalize != 0, d.skew_flag, b.st))
            return e;
    } else {
        if (d.skew_flag) IBVH_HIP_CHECK(hipMemsetAsync(d.skew_flag, 0, 4, b.st)); // (the pair sort does not care about skew)
        int32_t in_alt = 0;
        if (int e = rsort::sort_pairs(route.pairs, b.key_bytes, b.key_bits, b.n, sc.keys, sc.vals, sc.keys_alt, sc.vals_alt, true,
                                      &in_alt, rsort::scratch_bytes(b.n), b.st, true, &ra))
            return e;
        if (b.in_place)
            IBVH_HIP_CHECK(hipMemcpyAsync(b.leaves, sc.records, (size_t)b.n * b.lay.leaf_bytes, hipMemcpyDeviceToDevice, b.st));
    }
    return IBVH_OK;
}

} // namespace build
} // namespace ibvh

using namespace ibvh;
using namespace ibvh::build;

extern "C" {

ibvh_status ibvh_build_scratch_bytes(const ibvh_types *types, int64_t n, size_t *bytes_out) {
    if (!types || !bytes_out) return IBVH_ERR_INVALID_ARG;
    ibvh_layout lay;
    if (!layout_of(*types, lay)) return IBVH_ERR_UNSUPPORTED;
    if (n < 1) return IBVH_ERR_DOMAIN;
    *bytes_out = carve(nullptr, n, key_bytes(types->morton_type), lay.leaf_bytes, types->morton_type).total;
    return IBVH_OK;
}

ibvh_status ibvh_extrema(const ibvh_types *types, const void *records, int32_t wrapped, int64_t n, int32_t expand,
                         void *extrema_out, void *scratch, size_t scratch_bytes, void *stream) {
    if (!types || !records || !extrema_out || !scratch) return IBVH_ERR_INVALID_ARG;
    if (n < 1) return IBVH_ERR_DOMAIN;
    if (scratch_bytes < (size_t)EXT_MAX_BLOCKS * 6 * 8) return IBVH_ERR_SCRATCH;
    ibvh_layout lay;
    if (!layout_of(*types, lay)) return IBVH_ERR_UNSUPPORTED;
    int64_t stride = wrapped ? lay.leaf_bytes : lay.volume_bytes;
    return (ibvh_status)dispatch_volume(types->leaf_kind, types->leaf_float, [&](auto lt) -> int {
        using V = typename decltype(lt)::type;
        return extrema<V>((const char *)records, stride, n, expand, (typename V::elt *)extrema_out, (char *)scratch,
                          (hipStream_t)stream);
    });
}

ibvh_status ibvh_morton_keys(const ibvh_types *types, const void *records, int32_t wrapped, int64_t n, const void *ext,
                             void *keys_out, void *stream) {
    if (!types || !records || !ext || !keys_out) return IBVH_ERR_INVALID_ARG;
    if (n < 1) return IBVH_ERR_DOMAIN;
    ibvh_layout lay;
    if (!layout_of(*types, lay)) return IBVH_ERR_UNSUPPORTED;
    int64_t stride = wrapped ? lay.leaf_bytes : lay.volume_bytes;
    return (ibvh_status)dispatch_volume(types->leaf_kind, types->leaf_float, [&](auto lt) -> int {
        using V = typename decltype(lt)::type;
        return encode<V>((const char *)records, stride, n, (const typename V::elt *)ext, types->morton_type, keys_out,
                         (hipStream_t)stream);
    });
}

ibvh_status ibvh_build(const ibvh_build_desc *desc, const void *volumes, void *leaves, void *nodes, void *skips,
                       void *extrema_out, void *scratch, size_t scratch_bytes, void *stream) {
    if (!desc || !leaves || !skips || !scratch) return IBVH_ERR_INVALID_ARG;
    const ibvh_types &ty = desc->types;
    ibvh_layout lay;
    LeafLayout dlay;
    if (!layout_of(ty, lay, &dlay)) return IBVH_ERR_UNSUPPORTED;
    ibvh_tree tree;
    if (ibvh_status e = ibvh_tree_shape(desc->n, &tree)) return e;
    if (desc->n >= (int64_t(1) << 32)) return IBVH_ERR_INVALID_ARG; // positions are uint32 in the sort
    if (ty.index_type == IBVH_I32 && tree.real_nodes > INT32_MAX) return IBVH_ERR_OVERFLOW;
    if (desc->built_level < 1 || desc->built_level > tree.levels) return IBVH_ERR_INVALID_ARG; // build.jl:314
    if (!desc->already_wrapped && !volumes) return IBVH_ERR_INVALID_ARG;
    if (tree.real_nodes >= 2 && !nodes) return IBVH_ERR_INVALID_ARG;
    BuildCall b{};
    b.desc = desc, b.lay = lay, b.dlay = dlay, b.tree = tree, b.n = desc->n;
    b.key_bytes = key_bytes(ty.morton_type);
    b.key_bits = key_bits(ty.morton_type);
    b.sc = carve((char *)scratch, b.n, b.key_bytes, lay.leaf_bytes, ty.morton_type);
    if (scratch_bytes < b.sc.total) return IBVH_ERR_SCRATCH;
    // already_wrapped with a non-NULL `volumes`: `volumes` holds the source RECORDS and `leaves` receives the sorted
    // ones (out of place: no staging copy); with volumes == NULL the caller's `leaves` are sorted in place.
    b.wrapped = desc->already_wrapped != 0;
    b.in_place = b.wrapped && volumes == nullptr;
    b.src = (const char *)(b.in_place ? leaves : volumes);
    b.src_stride = b.wrapped ? lay.leaf_bytes : lay.volume_bytes;
    b.leaves = leaves, b.nodes = nodes, b.skips = skips, b.extrema_out = extrema_out;
    b.st = (hipStream_t)stream;

    const SortRoute route = choose_route(b.n, b.key_bits, b.key_bytes, (int)lay.leaf_bytes, b.sc.sort);
    int e = dispatch_volume(ty.leaf_kind, ty.leaf_float, [&](auto lt) -> int {
        using L = typename decltype(lt)::type;
        ExtremaFold<typename L::elt> fold;
        if (int e = launch_extrema<L>(b, fold)) return e;
        return launch_keys<L>(b, route, fold);
    });
    if (!e) e = sort_records(b, route);
    if (!e) e = aggregate_tree(ty, leaves, tree, desc->built_level, nodes, b.st);
    return (ibvh_status)e;
}

} // extern "C"
