// ibvh_lvt_mixed_b.hip — pair walks of two BVHs of different types (ibvh_lvt_mixed.inc): part of the same-float queries, walker 2
#include "ibvh_lvt_mixed.inc"

namespace ibvh {
namespace lvt {
IBVH_FOR_MIXED_QUEUE_B(IBVH_INSTANTIATE_PAIR_MIXED)
} // namespace lvt
} // namespace ibvh
