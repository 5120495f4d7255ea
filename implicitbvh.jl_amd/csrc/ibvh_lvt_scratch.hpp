// ibvh_lvt_scratch.hpp — the layout of the ONE caller-provided scratch buffer every leaf-vs-tree call works in (self, pair,
// mixed pair, rays; *_count, *_write, *_enqueue), for the size queries and for the launch code alike.  Host arithmetic on
// plain integers only (no HIP type: a host-compiled check includes this file on its own).
//
//   [ header | scan tile sums | contact cache: K slots x n_items pairs | ...gap... | tail ]
//   0        64               scan_scratch_bytes(n)                                     scratch_bytes
//
// FRONT residents are placed forward from offset 0: the header (int64 words: [0] the total contacts, where *_count / *_enqueue
// leave it for ibvh_lvt_total; the rest reserved), the scan's tile sums, the contact cache (slot-major).  BACK residents — the
// tail — are anchored at the END of whatever size the caller passed, aligned DOWN to TAIL_ALIGN: either [index array | block
// rows] (SELF / PAIR walks under BBox nodes: Args::q_index_dense, Args::blk_rows) or the tables of the binned ray path
// (RayBinPlan::bytes).  The contact cache absorbs the gap: it gets the slots that fit between the scan sums and the tail.  A
// scratch too small for a tail runs without it: first the index array goes, then the rows (no index array without rows); the
// ray bins go as a whole.  Which tail a call is ENTITLED to is the caller's knowledge (run<> in ibvh_lvt.hip); whether it fits
// and where everything goes is decided here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ibvh {
namespace lvt {

constexpr int SCAN_TILE = 4096;  // counts per tile of the scan (ibvh_lvt_scan.hip: SCAN_TPB * SCAN_IPT)
constexpr int BLK_ROW = 512;     // 32-bit words per block row (ibvh_lvt.hpp "the shared part of the descent")
constexpr int BLK_SHIFT_MIN = 9; // (the scratch is sized for the smallest block the launch code may choose)
constexpr int MAX_CACHE_SLOTS = 64;
constexpr size_t SCRATCH_HEADER_BYTES = 64;
constexpr size_t TAIL_ALIGN = 256;
// The start of an end-anchored tail is rounded DOWN, so up to TAIL_ALIGN - 1 bytes in front of it are lost: the launch keeps
// TAIL_FIT_SLACK between the front residents and a tail.  The size queries go forward from offset 0, round the front UP and add
// TAIL_SIZE_SLACK per tail: the fitting side's worst case plus one spare alignment step (callers memoise these sizes: it stays).
constexpr size_t TAIL_FIT_SLACK = TAIL_ALIGN, TAIL_SIZE_SLACK = 2 * TAIL_ALIGN;
constexpr size_t ABSENT = ~(size_t)0;

inline size_t tail_align_up(size_t v) { return (v + TAIL_ALIGN - 1) / TAIL_ALIGN * TAIL_ALIGN; }
// The scan's scratch (scan_counts, ibvh_lvt_scan.hip), in 64-bit words: the header (word 0: the total), from SCAN_AGG_OFFSET on one
// aggregate per tile, one spare word.  (constexpr: the kernels that zero the aggregates use the same arithmetic.)
constexpr size_t SCAN_AGG_OFFSET = SCRATCH_HEADER_BYTES;
constexpr int64_t scan_tiles(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
constexpr size_t scan_agg_words(int64_t n) { return (size_t)scan_tiles(n > 0 ? n : 1) + 1; }
constexpr size_t scan_used_bytes(int64_t n) { return SCAN_AGG_OFFSET + scan_agg_words(n) * 8; }
inline size_t scan_scratch_bytes(int64_t n) { return tail_align_up(scan_used_bytes(n)); }
inline size_t blk_rows_bytes(int64_t n_items, int shift) {
    return (size_t)(((n_items > 0 ? n_items : 1) + ((int64_t)1 << shift) - 1) >> shift) * BLK_ROW * 4;
}
inline size_t index_bytes(int64_t pair_bytes) { return (size_t)pair_bytes / 2; } // of one index I of an IndexPair{I}
inline size_t index_array_bytes(int64_t n_items, int64_t pair_bytes) { return tail_align_up((size_t)n_items * index_bytes(pair_bytes)); }
// the least any call needs: header + scan sums (IBVH_ERR_SCRATCH below that)
inline bool scratch_holds_front(int64_t n_items, size_t scratch_bytes) { return scratch_bytes >= scan_scratch_bytes(n_items); }

enum ScratchTail { TAIL_NONE, TAIL_ROWS, TAIL_BINS };
struct ScratchPlan { // byte offsets into the scratch; ABSENT: the call runs without that resident
    size_t cache = ABSENT; // contact cache, K * n_items pairs
    int K = 0;
    size_t index = ABSENT, rows = ABSENT, bins = ABSENT;
};
// one call's layout in the `scratch_bytes` it was given (scratch_holds_front); bins_bytes: RayBinPlan::bytes (TAIL_BINS)
inline ScratchPlan scratch_plan(int64_t n_items, int64_t pair_bytes, ScratchTail tail, size_t bins_bytes, size_t scratch_bytes) {
    ScratchPlan p;
    const size_t front = scan_scratch_bytes(n_items);
    auto fits = [&](size_t bytes) { return scratch_bytes - front >= bytes + TAIL_FIT_SLACK; };
    size_t index = 0, rows = 0, bins = 0; // bytes of the tail: [index array | rows] or [bins]
    if (tail == TAIL_ROWS) {
        index = index_array_bytes(n_items, pair_bytes), rows = blk_rows_bytes(n_items, BLK_SHIFT_MIN);
        if (!fits(rows + index)) index = 0;
        if (!fits(rows)) rows = 0;
    } else if (tail == TAIL_BINS && fits(bins_bytes)) {
        bins = bins_bytes;
    }
    const size_t back = index + rows + bins, at = (scratch_bytes - back) & ~(TAIL_ALIGN - 1);
    if (index) p.index = at;
    if (rows) p.rows = at + index;
    if (bins) p.bins = at;
    const size_t room = scratch_bytes - front - (back ? back + TAIL_FIT_SLACK : 0);
    const size_t slot = (size_t)(n_items > 0 ? n_items : 0) * (size_t)pair_bytes; // one slot of every work item
    if (slot && room / slot) p.cache = front, p.K = (int)(room / slot > MAX_CACHE_SLOTS ? MAX_CACHE_SLOTS : room / slot);
    return p;
}
// The size a caller should pass: room for `cache_slots` slots and for every tail asked for, i.e. the scratch_bytes for which
// scratch_plan() yields K >= cache_slots with the index array and the rows (rows: BBox nodes — by node kind alone, a size query
// does not know the call's shape) and the ray bins (bins_bytes != 0) present.
inline size_t scratch_size(int64_t n_items, int64_t pair_bytes, int cache_slots, bool rows, size_t bins_bytes) {
    size_t o = scan_scratch_bytes(n_items) + (size_t)cache_slots * (size_t)n_items * (size_t)pair_bytes;
    if (rows) o = tail_align_up(o) + index_array_bytes(n_items, pair_bytes) + blk_rows_bytes(n_items, BLK_SHIFT_MIN) + TAIL_SIZE_SLACK;
    if (bins_bytes) o = tail_align_up(o) + bins_bytes + TAIL_SIZE_SLACK;
    return o;
}

} // namespace lvt
} // namespace ibvh
