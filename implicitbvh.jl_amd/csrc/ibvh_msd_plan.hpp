// ibvh_msd_plan.hpp — everything the host decides about one record sort (ibvh_msd.hip), decided once: the geometries its
// kernels exist in, the plan (digit, partition tile, finish workgroup, table counts), the partition's LDS budget and the layout
// of its tables in the sort scratch — for the size query, the launch code and the dispatchers alike.  Host arithmetic on plain
// integers only (no HIP type: a host-compiled check includes this file on its own).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ibvh {
namespace msd {

constexpr int MAX_LEVELS = 4;        // partition levels beyond the first (levels 2 .. 5)
constexpr int L2_BITS = 8;           // sub-cells per oversized cell: 2^8
constexpr int kMaxLds = 160 * 1024;  // LDS of a gfx950 CU
constexpr int kRescuers = 512;       // rescue workgroups of the finish kernel that scratch is carved for; a launch uses at most half of what the device holds at once (they WAIT for the ordinary workgroups)

struct Geometry {
    int tpb, ipt; // threads, keys per thread
    constexpr int tile() const { return tpb * ipt; }
};
// Every partition (and histogram) tile make_plan() can choose, in ascending size: X(args..., threads, keys per thread).
// sort_records() dispatches over this table and so instantiates exactly its kernels.
#define IBVH_PARTITION_GEOMETRIES(X, ...) X(__VA_ARGS__, 256, 4) X(__VA_ARGS__, 256, 8) X(__VA_ARGS__, 512, 8)
#define IBVH_PARTITION_ROW(_, T, I) Geometry{T, I},
constexpr Geometry kPartition[] = {IBVH_PARTITION_GEOMETRIES(IBVH_PARTITION_ROW, _)};
#undef IBVH_PARTITION_ROW

// Every finish workgroup make_plan() can choose: X(key type, capacity, threads, resident); keys per thread = capacity / threads.
// run_finish() (ibvh_msd_finish.hip) dispatches over this table and so instantiates exactly its kernels; `resident` marks the
// geometry whose launch may keep a range's RECORDS in LDS (its kernel exists in that form as well as the plain one).  For each
// key type the plain rows are in ascending capacity: make_plan takes the first one the average cell fits, else the last
// (64-bit keys stop at 8,192: 16,384 x 10 B does not fit the LDS).
#define IBVH_FINISH_GEOMETRIES(X)                                                                                             \
    X(uint32_t, 2048, 256, false) X(uint32_t, 4096, 256, false) X(uint32_t, 8192, 512, false) X(uint32_t, 8192, 1024, true)    \
    X(uint32_t, 16384, 512, false) X(uint64_t, 2048, 256, false) X(uint64_t, 4096, 256, false) X(uint64_t, 8192, 512, false)
struct FinishGeometry {
    int key_bytes, cap, threads;
    bool resident;
};
#define IBVH_FINISH_ROW(K, C, T, R) FinishGeometry{(int)sizeof(K), C, T, R},
constexpr FinishGeometry kFinish[] = {IBVH_FINISH_GEOMETRIES(IBVH_FINISH_ROW)};
#undef IBVH_FINISH_ROW

// Dynamic LDS of a partition workgroup: the digit's two tables, then the wave histograms or — later, in the same bytes — the
// staged tile (equalised cells: with the 2-byte cell of every staged record)
inline size_t partition_lds(Geometry g, int stride, int bits, bool eq) {
    const size_t hist = (size_t)(g.tpb / 64) * ((size_t)2 << bits), st = (size_t)g.tile() * ((size_t)stride + (eq ? 2 : 0));
    return ((size_t)8 << bits) + 128 + (hist > st ? hist : st);
}
inline bool partition_fits(Geometry g, int stride, int bits, bool eq) { return partition_lds(g, stride, bits, eq) <= (size_t)kMaxLds; }

struct Plan {
    int bits;         // MSD digit width; 0: this path does not apply (tiny input) -> ibvh_sort.hip
    int shift;        // key_bits - bits: the cell is key >> shift
    Geometry part;    // partition (and histogram) tile: a row of kPartition
    Geometry fin;     // finish workgroup: a row of kFinish
    bool resident;    // ... the one that may keep a range's records in LDS
    int64_t n;
    int num_tiles;
    int max_seg;      // S: the most crowded segments a level can have
    int max_tiles2;   // T2: the most tiles a level can have
    int rescue_slots; // H: rescue workgroups of the finish grid that scratch is carved for (whatever the msd_rescue knob says)
    constexpr int tile() const { return part.tile(); }
    constexpr int cap() const { return fin.tile(); }
    constexpr int radix() const { return 1 << bits; }
};

// msd_avg (development knob, ibvh_set_tuning): the largest average cell before another first-level bit is taken
inline Plan make_plan(int64_t n, int key_bits, int key_bytes, int leaf_bytes, int msd_avg) {
    Plan p{};
    if (n < 4096 || key_bits <= 8 || n >= ((int64_t)1 << 32) - 65536) return p;
    int bits = 6; // (>= 6: the scan kernel works on blocks of 64 digits)
    while (bits < 11 && bits < key_bits - 1 && (n >> bits) > msd_avg) ++bits;
    // 1.3e7 .. 2.7e7 leaves: 4,096 cells keep the average cell within the 8,192-record finish workgroup (the 16,384-
    // record one runs one workgroup per CU: 2e7 leaves 0.73 -> 0.40 ms for the finish, +0.05 for the wider partition)
    constexpr int64_t kCellMax8k = 8192 * 8 / 10;
    if (bits == 11 && key_bits > 13 && (n >> 11) > kCellMax8k && (n >> 12) <= kCellMax8k) bits = 12;
    if (bits >= key_bits) bits = key_bits - 1;
    if (bits < 6) return p;
    const int64_t avg = n >> bits;
    // capacity of the finish workgroup: the average cell fills at most 5/8 of it (uniform clouds vary by a few per
    // cent; denser cells get the rest of the headroom before the second partition level takes them)
    // (the last step is taken later — the average cell may fill 8/10 of the 8,192-record workgroup, a Poisson cell count
    // then stays below it — because the 16,384-record workgroup is so much slower: 1.25e7 leaves 0.43 -> 0.26 ms)
    const FinishGeometry *fin = nullptr;
    for (const FinishGeometry &f : kFinish) {
        if (f.key_bytes != key_bytes || f.resident) continue;
        fin = &f;
        if (f.cap < 8192 ? avg * 8 <= (int64_t)f.cap * 5 : avg * 10 <= (int64_t)f.cap * 8) break;
    }
    if (!fin) return p;
    // Cells of the 8,192-record geometry (~2.5 .. 6.5 k records of 24 bytes: 1e7-leaf builds) are finished with their RECORDS
    // resident in LDS — read from memory once instead of ~2.8 times (finish_range, resident path) — by one 1,024-thread
    // workgroup per CU; cells beyond the ~5,000 records that fit beside the sort's arrays take the plain path inside the same
    // kernel.  Measured at 1e7 leaves: finish 212 -> 196 us; smaller geometries lose (1e6: 24 -> 32 us) and keep the plain kernel,
    // and so do cells of ~3,000 records (1.25e7 leaves at 12 bits: 289 against 265 us): the rule asks for >= 4,096 on average.
    if (fin->cap == 8192 && avg >= 4096 && leaf_bytes <= 24)
        for (const FinishGeometry &f : kFinish)
            if (f.key_bytes == key_bytes && f.cap == fin->cap && f.resident) fin = &f;
    // partition tile: the largest row, from the input's size down, whose staged records fit the LDS and whose window of
    // sub-cells (< tile + one sub-cell) fits the finish workgroup's LDS sort
    int t = (n >= (int64_t(1) << 22) && leaf_bytes <= 32) ? 2 : 1;
    while (t > 0 && (!partition_fits(kPartition[t], leaf_bytes, bits, false) || kPartition[t].tile() > fin->cap / 2)) --t;
    if (!partition_fits(kPartition[t], leaf_bytes, bits, false)) return p;
    p.part = kPartition[t];
    // finish workgroups are small (4 or 8 waves, many keys per thread): several ranges per CU at different phases
    p.fin = Geometry{fin->threads, fin->cap / fin->threads};
    p.resident = fin->resident;
    p.bits = bits;
    p.shift = key_bits - bits;
    p.n = n;
    p.num_tiles = (int)((n + p.tile() - 1) / p.tile());
    // segments of an extra level hold more than cap records each; a segment's last tile may be partial
    p.max_seg = (int)(n / p.cap() + 1);
    p.max_tiles2 = p.num_tiles + p.max_seg;
    // no more rescue workgroups than there can be windows to sort (the launch clamps them to half of what the device holds)
    p.rescue_slots = p.max_seg < kRescuers ? p.max_seg : kRescuers;
    return p;
}

// The plan's tables in the sort scratch (Tables / Level, ibvh_msd.hpp: what each one holds), in this order, each 256-byte aligned
enum Table { T_TILE_HIST, T_TILE_SCAN, T_CELL_TOTAL, T_CELL_START, T_NEEDED, T_TILE_HIST2, T_TILE_SCAN2, T_TILE_AND, T_TILE_OR,
             T_SPLITTERS, T_DIG, T_RESCUE, T_RESCUE_PRIV, T_LEVELS };
enum LevelTable { L_HDR, L_SEG_START, L_SEG_COUNT, L_SEG_TILE, L_SEG_AND, L_SEG_OR, L_SUB_START, L_TILE_SEG, L_TABLES };
struct TableLayout {
    size_t at[T_LEVELS + MAX_LEVELS * L_TABLES]; // byte offsets: at[T_...], at[T_LEVELS + level * L_TABLES + L_...]
    size_t total;
};
inline TableLayout table_layout(const Plan &p) {
    const size_t R = (size_t)p.radix(), S = (size_t)p.max_seg, T2 = (size_t)p.max_tiles2, hist = R * p.num_tiles * 4;
    const size_t top[T_LEVELS] = {hist, hist, R * 4, (R + 1) * 4, 64, T2 * 4 << L2_BITS, T2 * 4 << L2_BITS, T2 * 8, T2 * 8,
                                  ((R + 1) * 2 + 32768) * 8, // splitters, candidates, the sorted sample lists
                                  (size_t)p.n * 2, S * 64, (size_t)p.rescue_slots * 2 * (size_t)p.cap() * 4};
    const size_t level[L_TABLES] = {64, S * 4, S * 4, S * 4, S * 8, S * 8, S * 4 * ((1 << L2_BITS) + 1), T2 * 4};
    TableLayout l{};
    for (int i = 0; i < T_LEVELS + MAX_LEVELS * L_TABLES; ++i) {
        l.at[i] = l.total;
        l.total += ((i < T_LEVELS ? top[i] : level[(i - T_LEVELS) % L_TABLES]) + 255) / 256 * 256;
    }
    return l;
}

// a record as 8-byte words: g / words == __umulhi(g, inv_words) for g < 2^29
struct RecordWords {
    uint32_t words, inv_words;
};
inline RecordWords record_words(int stride) {
    const uint32_t words = (uint32_t)stride / 8u;
    return {words, (uint32_t)((((uint64_t)1 << 32) + words - 1) / words)};
}

} // namespace msd
} // namespace ibvh
