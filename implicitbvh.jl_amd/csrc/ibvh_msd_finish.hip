// ibvh_msd_finish.hip — the build's sort, second half: every cell of the partitioned records (and every window of sub-cells of a
// crowded cell) is sorted by one workgroup in LDS and written to its final place.  gfx950 only.  See ibvh_msd.hip for the whole
// picture (replaces AK.sort!(leaves, by = bv -> bv.morton), reference src/build.jl:248-253).
// The kernel is a template (ibvh_msd_finish.inc); this unit's dispatcher instantiates it for the geometries of kFinish
// (ibvh_msd_plan.hpp).
// Diagnostic builds (-DIBVH_PHASE_STAMPS) compile it inside ibvh_msd.hip's translation unit instead: one stamp buffer.
#if !defined(IBVH_PHASE_STAMPS) || defined(IBVH_MSD_SINGLE_TU)
#include "ibvh_msd_finish.inc"

namespace ibvh {
namespace msd {

// the finish launch for the plan's geometry: make_plan takes it from the same table, so one case matches
int run_finish(const Plan &p, const Tables &tb, int key_bytes, const FinishArgs &fa, hipStream_t st) {
#define IBVH_FIN(K, C, T, R) \
    if (sizeof(K) == (size_t)key_bytes && p.cap() == C && p.fin.tpb == T) return launch_finish<K, T, C / T, R>(p, tb, fa, st);
    IBVH_FINISH_GEOMETRIES(IBVH_FIN)
#undef IBVH_FIN
    return IBVH_ERR_INVALID_ARG;
}

} // namespace msd
} // namespace ibvh
#endif
