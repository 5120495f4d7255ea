// ibvh_aggregate.hip — the bottom-up merge of the sorted leaves into the nodes (build.jl:366-523), behind ibvh_aggregate,
// ibvh_refit and ibvh_build.  One launch builds up to CH_LEVELS tree levels: a workgroup owns 2*TPB consecutive inputs (leaves,
// or nodes of the level the previous launch ended on), merges them pairwise, and keeps folding through LDS, writing every
// level it makes.  The reference launches once per level (build.jl:371-375: ~levels launches); this needs
// ceil((levels-1)/CH_LEVELS), and one workgroup folds the top of the tree.
//   aggregate         read records [24 stride, 16 used], write nodes [24 * ~1]   (BSphere{F32} leaves, bytes per leaf)
#include "ibvh_aggregate.hpp"

#include <type_traits>

namespace ibvh {
namespace build {

constexpr int AGG_TPB = 256;
constexpr int CH_LEVELS = 9; // 2*256 inputs -> 256,128,...,1 nodes

// The one step of the merge: a parent is both children merged, or the lone left child converted to the node type (a node to
// its own type: the identity).  The right child is handed over where it lies (`pb`: global memory, LDS or a register copy)
// and read only when it exists, inside the merging arm.
template <class N, class In> IBVH_D N parent_of(const In &a, const void *pb, bool has_b) {
    return has_b ? merge_to(a, load_vol<In>(pb), (N *)nullptr) : convert_to(a, (N *)nullptr);
}

// The rest of a launch: fold the workgroup's nodes of `level` (`mine`; `nreal` of them on that level) upwards through LDS,
// up to CH_LEVELS - 1 more levels and not above built_level, writing every node made.
template <class N>
IBVH_D void fold_up(N *s_nodes, N mine, int64_t level, int64_t nreal, const TreeDev &tree, int64_t built_level, N *__restrict__ nodes) {
    const int t = threadIdx.x;
    int count = AGG_TPB;
#pragma unroll 1
    for (int s = 1; s < CH_LEVELS; ++s) {
        if (level - 1 < built_level) break; // uniform
        __syncthreads();
        if (t < count) s_nodes[t] = mine;
        __syncthreads();
        count >>= 1;
        level -= 1;
        const int64_t child_real = nreal;
        nreal = level_num_real(tree.levels, tree.virtual_leaves, level);
        const int64_t i = (int64_t)blockIdx.x * count + t;
        if ((t < count) && (i < nreal)) {
            const N a = s_nodes[2 * t];
            mine = parent_of<N>(a, s_nodes + 2 * t + 1, 2 * i + 1 < child_real);
            nodes[level_start(tree.levels, tree.virtual_leaves, level) - 1 + i] = mine;
        }
    }
}

template <class L, class N, bool FROM_LEAVES>
__global__ __launch_bounds__(AGG_TPB) void aggregate_kernel(const char *__restrict__ in, int64_t in_stride, int64_t in_level,
                                                            TreeDev tree, int64_t built_level, N *__restrict__ nodes) {
    using In = std::conditional_t<FROM_LEAVES, L, N>;
    __shared__ N s_nodes[AGG_TPB];
    const int64_t level = in_level - 1; // the level being produced first
    const int64_t in_real = FROM_LEAVES ? tree.real_leaves : level_num_real(tree.levels, tree.virtual_leaves, in_level);
    const int64_t i = (int64_t)blockIdx.x * AGG_TPB + threadIdx.x; // 0-based node index within `level`
    const int64_t nreal = level_num_real(tree.levels, tree.virtual_leaves, level);
    N mine;
    if (i < nreal) {
        const int64_t l = 2 * i, r = 2 * i + 1; // 0-based children within in_level
        const In a = load_vol<In>(in + l * in_stride);
        mine = parent_of<N>(a, in + r * in_stride, r < in_real);
        nodes[level_start(tree.levels, tree.virtual_leaves, level) - 1 + i] = mine;
    }
    fold_up<N>(s_nodes, mine, level, nreal, tree, built_level, nodes);
}

// Refit from new volumes in the user's order (ibvh_refit): the first launch of aggregate<L, N>, with the gather fused in.
// Each leaf takes volumes[.index - 1], stores it into its record (volume bytes only) and is merged exactly as in
// aggregate_kernel<L, N, true>.  The index is checked BEFORE the load: a leaf whose index lies outside 1..m keeps its old
// volume and stores 1 to *flag.  A 1-leaf tree has no nodes: its leaf is only gathered.
template <class L, class N, class I>
__global__ __launch_bounds__(AGG_TPB) void refit_kernel(char *__restrict__ leaves, LeafLayout lay, const char *__restrict__ volumes,
                                                        int64_t m, uint32_t *flag, TreeDev tree, int64_t built_level,
                                                        N *__restrict__ nodes) {
    __shared__ N s_nodes[AGG_TPB];
    const int64_t i = (int64_t)blockIdx.x * AGG_TPB + threadIdx.x;
    const bool one_leaf = tree.levels == 1;
    const int64_t level = tree.levels - 1;
    const int64_t nreal = one_leaf ? 1 : level_num_real(tree.levels, tree.virtual_leaves, level);
    N mine;
    if (i < nreal) {
        const bool has_b = !one_leaf && 2 * i + 1 < tree.real_leaves;
        char *ra = leaves + 2 * i * lay.stride, *rb = ra + lay.stride;
        // both indices, then both gathers, then both stores: two dependent round trips per item, not four
        const I ia = load_index<I>(ra, lay), ib = has_b ? load_index<I>(rb, lay) : I(1);
        const bool oka = ia >= 1 && (int64_t)ia <= m, okb = ib >= 1 && (int64_t)ib <= m;
        const char *sa = oka ? volumes + ((int64_t)ia - 1) * (int64_t)sizeof(L) : ra;
        const char *sb = okb ? volumes + ((int64_t)ib - 1) * (int64_t)sizeof(L) : rb;
        L a, b;
        if constexpr (sizeof(L) % 16 == 0) { // raw BSphere{F32}/{F64}, BBox{F64}: one 16-byte request per 16 bytes
            a = oka && ((uintptr_t)volumes & 15) == 0 ? load_vol16<L>(sa) : load_vol<L>(sa);
            if (has_b) b = okb && ((uintptr_t)volumes & 15) == 0 ? load_vol16<L>(sb) : load_vol<L>(sb);
        } else {
            a = load_vol<L>(sa);
            if (has_b) b = load_vol<L>(sb);
        }
        if (oka) store_vol(ra, a);
        if (has_b && okb) store_vol(rb, b);
        if (flag && !(oka && okb)) *flag = 1u;
        if (one_leaf) return; // (uniform: a one-block launch)
        mine = parent_of<N>(a, &b, has_b);
        nodes[level_start(tree.levels, tree.virtual_leaves, level) - 1 + i] = mine;
    }
    if (one_leaf) return;
    fold_up<N>(s_nodes, mine, level, nreal, tree, built_level, nodes);
}

// The top of the tree: one workgroup folds all levels above `in_level` (<= AGG_TOP_MAX inputs), a barrier per level; same
// parent_of as below, so the nodes are bit-identical.  IN_LDS (round 3; the inputs fit 128 KB): the level being folded
// lives in LDS — inputs read from memory once, every level's nodes stored as they are made, and the next level folds the
// LDS copy — instead of each level re-reading through L2 what the level before has just stored (eleven dependent
// store -> load round trips at 1e6 leaves: 8.3 us for a kernel whose work is 4 k merges).
constexpr int AGG_TOP_TPB = 1024, AGG_TOP_MAX = 4096, AGG_TOP_LDS_BYTES = 128 * 1024;
template <class N, bool IN_LDS>
__global__ __launch_bounds__(AGG_TOP_TPB) void aggregate_top_kernel(TreeDev tree, int64_t in_level, int64_t built_level, N *nodes) {
    if constexpr (IN_LDS) {
        extern __shared__ __attribute__((aligned(16))) unsigned char top_smem[];
        N *s = (N *)top_smem;
        int64_t have = level_num_real(tree.levels, tree.virtual_leaves, in_level); // nodes of the level held in LDS
        {
            const N *in = nodes + (level_start(tree.levels, tree.virtual_leaves, in_level) - 1);
            for (int64_t i = threadIdx.x; i < have; i += AGG_TOP_TPB) s[i] = load_vol<N>(in + i);
        }
        __syncthreads();
        for (int64_t level = in_level - 1; level >= built_level && level >= 1; --level) {
            const int64_t nreal = level_num_real(tree.levels, tree.virtual_leaves, level);
            N *out = nodes + (level_start(tree.levels, tree.virtual_leaves, level) - 1);
            // (nreal <= AGG_TOP_MAX / 2 <= 2 * AGG_TOP_TPB: at most two nodes per thread, read before anything is overwritten)
            N mine[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int64_t i = threadIdx.x + (int64_t)k * AGG_TOP_TPB;
                if (i < nreal) mine[k] = parent_of<N>(s[2 * i], s + 2 * i + 1, 2 * i + 1 < have);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int64_t i = threadIdx.x + (int64_t)k * AGG_TOP_TPB;
                if (i < nreal) {
                    s[i] = mine[k];
                    store_vol(out + i, mine[k]);
                }
            }
            __syncthreads();
            have = nreal;
        }
        return;
    }
    for (int64_t level = in_level - 1; level >= built_level && level >= 1; --level) {
        const int64_t nreal = level_num_real(tree.levels, tree.virtual_leaves, level);
        const int64_t child_real = level_num_real(tree.levels, tree.virtual_leaves, level + 1);
        const N *in = nodes + (level_start(tree.levels, tree.virtual_leaves, level + 1) - 1);
        N *out = nodes + (level_start(tree.levels, tree.virtual_leaves, level) - 1);
        for (int64_t i = threadIdx.x; i < nreal; i += AGG_TOP_TPB) {
            const N a = load_vol<N>(in + 2 * i);
            store_vol(out + i, parent_of<N>(a, in + 2 * i + 1, 2 * i + 1 < child_real));
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ibvh_refit from volumes in the user's order: what the first launch of aggregate() gathers into the leaf records
struct RefitGather {
    LeafLayout lay;
    int index_type;
    const void *volumes; // m raw volumes of the leaf type
    int64_t m;
    uint32_t *flag;      // optional
};

template <class L, class N>
int aggregate(const char *leaves, int64_t leaf_stride, const ibvh_tree &tree, int64_t built_level, N *nodes, hipStream_t st,
              const RefitGather *gather) {
    if (tree.real_nodes < 2 && !gather) return IBVH_OK; // build.jl:266
    const TreeDev td = tree_dev(tree);
    const auto real_on = [&](int64_t level) { return level_num_real(tree.levels, tree.virtual_leaves, level); };
    const auto grid_for = [&](int64_t level) { return dim3((unsigned)ceil_div(real_on(level), AGG_TPB)); }; // a thread per node of `level`
    // The first launch: leaves (level `levels`) -> levels-1 .. levels-CH_LEVELS, plain or gathering.  The last-level merge
    // always runs (aggregate_last_level!, build.jl:369), even when built_level == levels.
    const dim3 first_grid = tree.levels > 1 ? grid_for(tree.levels - 1) : dim3(1);
    const int64_t first_built = built_level > tree.levels - 1 ? tree.levels - 1 : built_level;
    if (gather) {
        int e = dispatch_index(gather->index_type, [&](auto it) -> int {
            using I = typename decltype(it)::type;
            IBVH_LAUNCH((refit_kernel<L, N, I>), first_grid, dim3(AGG_TPB), 0, st, (char *)leaves, gather->lay,
                        (const char *)gather->volumes, gather->m, gather->flag, td, first_built, nodes);
            return IBVH_OK;
        });
        if (e) return e;
    } else {
        IBVH_LAUNCH((aggregate_kernel<L, N, true>), first_grid, dim3(AGG_TPB), 0, st, leaves, leaf_stride, tree.levels, td,
                    first_built, nodes);
    }
    IBVH_LAUNCH_CHECK();
    if (tree.real_nodes < 2) return IBVH_OK; // (a refit of one leaf: gathered, no nodes)
    // While levels are left: few nodes -> ONE workgroup folds every remaining level (a launch costs more than these levels),
    // out of LDS if they fit; else a middle launch makes CH_LEVELS more.
    for (int64_t in_level = tree.levels - CH_LEVELS; in_level - 1 >= built_level && in_level - 1 >= 1; in_level -= CH_LEVELS) {
        const int64_t have = real_on(in_level);
        if (have <= AGG_TOP_MAX) {
            const size_t top_bytes = (size_t)have * sizeof(N);
            if (top_bytes <= (size_t)AGG_TOP_LDS_BYTES) {
                IBVH_HIP_CHECK(hipFuncSetAttribute((const void *)aggregate_top_kernel<N, true>, hipFuncAttributeMaxDynamicSharedMemorySize, AGG_TOP_LDS_BYTES));
                IBVH_LAUNCH((aggregate_top_kernel<N, true>), dim3(1), dim3(AGG_TOP_TPB), top_bytes, st, td, in_level, built_level, nodes);
            } else {
                IBVH_LAUNCH((aggregate_top_kernel<N, false>), dim3(1), dim3(AGG_TOP_TPB), 0, st, td, in_level, built_level, nodes);
            }
            IBVH_LAUNCH_CHECK();
            break;
        }
        const char *in = (const char *)(nodes + (level_start(tree.levels, tree.virtual_leaves, in_level) - 1));
        IBVH_LAUNCH((aggregate_kernel<L, N, false>), grid_for(in_level - 1), dim3(AGG_TPB), 0, st, in, (int64_t)sizeof(N), in_level,
                    td, built_level, nodes);
        IBVH_LAUNCH_CHECK();
    }
    return IBVH_OK;
}

int aggregate_tree(const ibvh_types &types, const void *leaves, const ibvh_tree &tree, int64_t built_level, void *nodes,
                   hipStream_t st, const RefitGather *gather) {
    ibvh_layout lay;
    if (!layout_of(types, lay)) return IBVH_ERR_UNSUPPORTED;
    return dispatch_leaf_node(types, [&](auto lt, auto nt) -> int {
        using L = typename decltype(lt)::type;
        using N = typename decltype(nt)::type;
        return aggregate<L, N>((const char *)leaves, lay.leaf_bytes, tree, built_level, (N *)nodes, st, gather);
    });
}

} // namespace build
} // namespace ibvh

using namespace ibvh;
using namespace ibvh::build;

extern "C" {

ibvh_status ibvh_aggregate(const ibvh_types *types, const ibvh_tree *tree, int64_t built_level, const void *leaves,
                           void *nodes, void *stream) {
    if (!types || !tree || !leaves) return IBVH_ERR_INVALID_ARG;
    if (built_level < 1 || built_level > tree->levels) return IBVH_ERR_INVALID_ARG;
    if (!combo_ok(*types)) return IBVH_ERR_UNSUPPORTED;
    if (tree->real_nodes >= 2 && !nodes) return IBVH_ERR_INVALID_ARG;
    return (ibvh_status)aggregate_tree(*types, leaves, *tree, built_level, nodes, (hipStream_t)stream);
}

ibvh_status ibvh_refit(const ibvh_bvh *bvh, const void *volumes, int64_t num_volumes, void *flag, void *stream) {
    if (!bvh || !bvh->leaves) return IBVH_ERR_INVALID_ARG;
    const ibvh_tree &tree = bvh->tree;
    if (tree.real_leaves < 1 || tree.levels < 1) return IBVH_ERR_INVALID_ARG;
    if (bvh->built_level < 1 || bvh->built_level > tree.levels) return IBVH_ERR_INVALID_ARG;
    if (tree.real_nodes >= 2 && !bvh->nodes) return IBVH_ERR_INVALID_ARG;
    if (volumes && (num_volumes < 0 || ((uintptr_t)volumes & 7) != 0)) return IBVH_ERR_INVALID_ARG;
    ibvh_layout lay;
    LeafLayout dlay;
    if (!layout_of(bvh->types, lay, &dlay)) return IBVH_ERR_UNSUPPORTED;
    const RefitGather g{dlay, bvh->types.index_type, volumes, num_volumes, (uint32_t *)flag};
    // the in-place form is exactly aggregate_oibvh! over the records as they stand
    return (ibvh_status)aggregate_tree(bvh->types, bvh->leaves, tree, bvh->built_level, (void *)bvh->nodes, (hipStream_t)stream,
                                       volumes ? &g : nullptr);
}

} // extern "C"
