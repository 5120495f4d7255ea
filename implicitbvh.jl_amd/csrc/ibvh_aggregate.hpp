// ibvh_aggregate.hpp — the bottom-up merge (ibvh_aggregate.hip) as the build driver (ibvh_build.hip) calls it.
#pragma once
#include "ibvh_common.hpp"

namespace ibvh {
namespace build {

struct RefitGather; // ibvh_refit's volumes in the user's order (ibvh_aggregate.hip); nullptr everywhere else

// Merges the leaf records as they stand in `leaves` into the nodes of levels levels - 1 .. built_level, on `st`; the leaf and
// node types of `types` are dispatched inside.
int aggregate_tree(const ibvh_types &types, const void *leaves, const ibvh_tree &tree, int64_t built_level, void *nodes,
                   hipStream_t st, const RefitGather *gather = nullptr);

} // namespace build
} // namespace ibvh
