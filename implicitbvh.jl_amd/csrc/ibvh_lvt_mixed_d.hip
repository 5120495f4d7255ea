// ibvh_lvt_mixed_d.hip — pair walks of two BVHs of different types (ibvh_lvt_mixed.inc): the cross-float queries and BSphere
// nodes, walker 1
#include "ibvh_lvt_mixed.inc"

namespace ibvh {
namespace lvt {
IBVH_FOR_MIXED_JOINT(IBVH_INSTANTIATE_PAIR_MIXED)
} // namespace lvt
} // namespace ibvh
