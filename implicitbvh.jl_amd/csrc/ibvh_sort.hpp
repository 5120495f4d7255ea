// ibvh_sort.hpp — host interface of ibvh_sort.hip (the stable sort of (key, uint32 position) pairs: LSD passes, or one
// MSD partition + in-LDS bucket sort) for ibvh_build.hip and ibvh_dist.hip.
#pragma once
#include "ibvh_common.hpp"
#include "ibvh_radix.hpp"

namespace ibvh {
namespace rsort {

struct Geometry {
    int tpb, ipt; // threads, keys per thread
    constexpr int tile() const { return tpb * ipt; }
};

// Everything one sort of n pairs decides, decided once (plan_pairs): a producer that fuses the first pass's per-tile
// histogram into its own kernel (ibvh_build.hip's key encoder) reads the tile and the digit from the plan that
// sort_pairs() then runs, so the two cannot disagree.
struct PairsPlan {
    Geometry tile;       // tiles of the LSD passes / of the hybrid's partition: an entry of kTiles (ibvh_sort.hip)
    int msd_bits;        // digit width of the MSD + in-LDS hybrid; 0: plain LSD passes
    Geometry bucket;     // the workgroup that sorts one bucket of the hybrid in LDS: an entry of kBuckets
    int shift, bits;     // the digit the first pass sorts on: (key >> shift) & mask (the top digit for the hybrid)
    uint32_t mask;
    int num_tiles;
    uint32_t *tile_hist; // [2^bits][num_tiles], digit-major: the start of the caller's scratch (scratch_bytes(n) of it)
};

size_t scratch_bytes(int64_t n);
PairsPlan plan_pairs(int64_t n, int key_bits, int key_bytes, void *scratch);
// vals_implicit: the values of the first pass are the element positions 0..n-1 (vals is not read).
// first_hist_done: p.tile_hist already holds the first pass's histogram.
// records: the last pass writes finished BoundingVolume records instead of sorted pairs.
int sort_pairs(const PairsPlan &p, int key_bytes, int key_bits, int64_t n, void *keys, void *vals, void *keys_alt, void *vals_alt,
               bool vals_implicit, int32_t *result_in_alt, size_t scratch_sz, hipStream_t st, bool first_hist_done,
               const RecordArgs *records);

} // namespace rsort
} // namespace ibvh
