// Host-compiled view of the record sort's plan (implicitbvh.jl_amd/csrc/ibvh_msd_plan.hpp) for tests/test_host_msd_plan.py
// and tests/test_gpu_msd_geometries.py.  Test infrastructure like the oracle: never linked into libibvh.so.
#include "../implicitbvh.jl_amd/csrc/ibvh_msd_plan.hpp"

using namespace ibvh::msd;

extern "C" {

// out[11]: bits, shift, partition (threads, keys per thread), finish (threads, keys per thread), resident, num_tiles, max_seg,
// max_tiles2, rescue slots.  Returns the bytes of the plan's tables (0, out all zero: the record sort does not apply).
uint64_t msd_plan(int64_t n, int key_bits, int key_bytes, int leaf_bytes, int msd_avg, int64_t *out) {
    const Plan p = make_plan(n, key_bits, key_bytes, leaf_bytes, msd_avg);
    const int64_t fields[11] = {p.bits, p.shift, p.part.tpb, p.part.ipt, p.fin.tpb, p.fin.ipt, p.resident, p.num_tiles, p.max_seg, p.max_tiles2,
                                p.rescue_slots};
    for (int i = 0; i < 11; ++i) out[i] = fields[i];
    return p.bits ? table_layout(p).total : 0;
}

// the offsets of that plan's tables (msd_table_count() of them, in the order of ibvh_msd_plan.hpp); returns their total
int msd_table_count() { return T_LEVELS + MAX_LEVELS * L_TABLES; }
uint64_t msd_table_offsets(int64_t n, int key_bits, int key_bytes, int leaf_bytes, int msd_avg, uint64_t *out) {
    const Plan p = make_plan(n, key_bits, key_bytes, leaf_bytes, msd_avg);
    if (!p.bits) return 0;
    const TableLayout l = table_layout(p);
    for (int i = 0; i < msd_table_count(); ++i) out[i] = l.at[i];
    return l.total;
}

// dynamic LDS of the partition launch (geometry, record stride, digit width, equalised or not)
uint64_t msd_partition_lds(int tpb, int ipt, int stride, int bits, int eq) { return partition_lds(Geometry{tpb, ipt}, stride, bits, eq != 0); }

// the geometry tables: rows of (threads, keys per thread) / (key bytes, capacity, threads, resident); returns the row count
int msd_partition_rows(int *out) {
    int r = 0;
    for (const Geometry &g : kPartition) out[2 * r] = g.tpb, out[2 * r + 1] = g.ipt, ++r;
    return r;
}
int msd_finish_rows(int *out) {
    int r = 0;
    for (const FinishGeometry &f : kFinish) out[4 * r] = f.key_bytes, out[4 * r + 1] = f.cap, out[4 * r + 2] = f.threads, out[4 * r + 3] = f.resident, ++r;
    return r;
}

} // extern "C"
