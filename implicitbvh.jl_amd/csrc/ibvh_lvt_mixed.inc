// ibvh_lvt_mixed.inc — the pair walks of two BVHs of different leaf / node types (IBVH_PAIR_MIXED_TYPES): launch_pair_mixed,
// instantiated by ibvh_lvt_mixed_{a,b,c,d}.hip for part of the (Q, L, N, I) combinations each (ibvh_lvt.hpp IBVH_FOR_MIXED_*), so
// that make -j spreads them.  A leaf-vs-tree walk only ever touches the driving leaves' type Q and the walked tree's L and N
// (lvt/traverse_pair.jl:176-244): these are the existing walkers with a query type of their own, no product of both trees' types.
#include "ibvh_lvt_queue.inc"

namespace ibvh {
namespace lvt {

template <class Q, class L, class N, class I>
int launch_pair_mixed(const Args<L, N, I> &a, const PairCache<I> &cache, bool write, hipStream_t st, bool *agg_zeroed) {
    return launch<L, N, I, MODE_PAIR, Q>(a, cache, write, st, RayBins{}, agg_zeroed);
}

#define IBVH_INSTANTIATE_PAIR_MIXED(Q_, L_, N_, I_) \
    template int launch_pair_mixed<Q_, L_, N_, I_>(const Args<L_, N_, I_> &, const PairCache<I_> &, bool, hipStream_t, bool *);

} // namespace lvt
} // namespace ibvh
