// Host-compiled view of the leaf-vs-tree scratch layout (implicitbvh.jl_amd/csrc/ibvh_lvt_scratch.hpp) for
// tests/test_host_lvt_scratch.py.  Test infrastructure like the oracle: never linked into libibvh.so.
#include "../implicitbvh.jl_amd/csrc/ibvh_lvt_scratch.hpp"

using namespace ibvh::lvt;

extern "C" {

// out: K and the offsets of cache, index array, rows, bins (-1: absent).  Returns 0 (out untouched) when the scratch does not
// even hold the front residents (the entry points answer IBVH_ERR_SCRATCH there).  tail: 0 none, 1 rows, 2 bins.
int lvt_scratch_plan(int64_t n_items, int64_t pair_bytes, int tail, uint64_t bins_bytes, uint64_t scratch_bytes, int64_t *out) {
    if (!scratch_holds_front(n_items, (size_t)scratch_bytes)) return 0;
    const ScratchPlan p = scratch_plan(n_items, pair_bytes, (ScratchTail)tail, (size_t)bins_bytes, (size_t)scratch_bytes);
    const size_t offsets[4] = {p.cache, p.index, p.rows, p.bins};
    out[0] = p.K;
    for (int i = 0; i < 4; ++i) out[1 + i] = offsets[i] == ABSENT ? -1 : (int64_t)offsets[i];
    return 1;
}

uint64_t lvt_scratch_size(int64_t n_items, int64_t pair_bytes, int cache_slots, int rows, uint64_t bins_bytes) {
    return scratch_size(n_items, pair_bytes, cache_slots, rows != 0, (size_t)bins_bytes);
}

} // extern "C"
