// ibvh_lvt.hip — leaf-vs-tree traversal (LVTTraversal) on gfx950, entry points: one work item per leaf / ray walks
// the (same / other) implicit tree depth-first; two passes (count -> inclusive scan -> write) give
// the reference's deterministic contact order.
//
// Replaces src/traverse/leaf_vs_tree/traverse_single.jl, traverse_pair.jl and
// src/raytrace/leaf_vs_tree/leaf_vs_tree.jl.
//
// The walkers live in their own translation units (ibvh_lvt.hpp lists them); this one holds the type dispatch, the
// two-pass protocol and the extern "C" entry points, and instantiates walker 1 (lvt_joint_kernel, the exact walk).
#include "ibvh_lvt.hpp"

namespace ibvh {
namespace lvt {

// What one call walks: n_items work items (drv's leaves; RAYS: the rays, drv == nullptr) against the tree `walk`; flip: bvh2 drives
struct Walk {
    const ibvh_bvh *drv, *walk;
    const void *points, *dirs;
    int64_t n_items, start_level;
    int32_t narrow, flip;
};
// What the call does with it: the *_count, *_write or *_enqueue call below, or ibvh_lvt_work_counters' counting pass (no scratch).
enum Op { OP_COUNT, OP_WRITE, OP_ENQUEUE, OP_WORK };
struct Call {
    Op op;
    void *counts;
    int64_t *total_out;
    void *contacts;
    int64_t capacity;
    void *total_dev, *total_host;
    unsigned long long *work;
    void *scratch;
    size_t scratch_bytes;
    void *stream;
};

// shared driver of the nine entry points and ibvh_lvt_work_counters
template <int MODE> int run(const Walk &w, const Call &c) {
    const bool write = c.op == OP_WRITE, enqueue = c.op == OP_ENQUEUE, work = c.op == OP_WORK;
    const hipStream_t st = (hipStream_t)c.stream;
    int32_t narrow = w.narrow;
    const int32_t positions = (narrow & IBVH_OUTPUT_POSITIONS) ? 1 : 0;
    if (narrow & ~(IBVH_NARROW_MASK | IBVH_OUTPUT_POSITIONS)) return IBVH_ERR_INVALID_ARG;
    narrow &= IBVH_NARROW_MASK;
    if (MODE == MODE_RAYS ? (narrow != IBVH_NARROW_NONE && narrow != IBVH_NARROW_RAY_ORIGIN_OUTSIDE)
                          : (narrow != IBVH_NARROW_NONE && narrow != IBVH_NARROW_MORTON_LT && narrow != IBVH_NARROW_INDEX_LT))
        return IBVH_ERR_INVALID_ARG;
    ibvh_layout lay;
    LeafLayout wl, dl;
    if (!layout_of(w.walk->types, lay, &wl)) return IBVH_ERR_UNSUPPORTED;
    dl = wl;
    if (w.drv && !layout_of(w.drv->types, lay, &dl)) return IBVH_ERR_UNSUPPORTED;
    if (!work && (!c.scratch || !scratch_holds_front(w.n_items, c.scratch_bytes))) return IBVH_ERR_SCRATCH;
    // The tail of the scratch this call is entitled to (whether it fits, and where everything goes: scratch_plan).
    // RAYS: the binned path's tables, when the tree and the batch qualify and the cut lies at or below the start level.
    // SELF / PAIR under BBox nodes: the rows of the shared descent (ibvh_lvt.hpp "BlockRows") and, in front of them, every work
    // item's .index (the counting pass writes it for the writing pass: Args::q_index_dense); without rows every wave descends on its own
    // (the rows are covers of consecutive work items made of the DRIVING tree's nodes: only when those have the walked tree's node
    // type — a mixed pair's driving nodes of another kind or float type are not rounded into covers, a BBox{Float64} rounded to
    // Float32 may no longer contain its leaves)
    const bool same_nodes = !w.drv || (w.drv->types.node_kind == w.walk->types.node_kind && w.drv->types.node_float == w.walk->types.node_float);
    RayBinPlan bin_plan;
    ScratchTail tail = TAIL_NONE;
    if (MODE == MODE_RAYS && !work) {
        bin_plan = rays_bin_plan(*w.walk, w.n_items);
        if (bin_plan.depth && bin_plan.cut_level >= w.start_level) tail = TAIL_BINS;
    } else if (MODE != MODE_RAYS && w.walk->types.node_kind == IBVH_BBOX && same_nodes) {
        tail = TAIL_ROWS;
    }
    // (OP_WORK uses no scratch at all)
    const ScratchPlan plan = work ? ScratchPlan{} : scratch_plan(w.n_items, lay.pair_bytes, tail, bin_plan.bytes, c.scratch_bytes);
    auto at = [&](size_t offset) { return offset == ABSENT ? nullptr : (char *)c.scratch + offset; };
    const RayBins bins = plan.bins != ABSENT ? rays_bins_at(bin_plan, at(plan.bins)) : RayBins{};
    return dispatch_leaf_node(w.walk->types, [&](auto lt, auto nt) -> int {
        using L = typename decltype(lt)::type;
        using N = typename decltype(nt)::type;
        if constexpr (MODE == MODE_RAYS && !std::is_same<typename L::elt, typename N::elt>::value) {
            return (int)IBVH_ERR_UNSUPPORTED; // isintersection(::BBox{T}, ::NTuple{3,T}, ...) needs one T
        } else {
            return dispatch_index(w.walk->types.index_type, [&](auto it) -> int {
                using I = typename decltype(it)::type;
                Args<L, N, I> a;
                a.items = w.drv ? (const char *)w.drv->leaves : nullptr;
                a.items_lay = dl;
                a.points = (const typename L::elt *)w.points;
                a.dirs = (const typename L::elt *)w.dirs;
                a.n_items = w.n_items;
                a.leaves = (const char *)w.walk->leaves;
                a.lay = wl;
                a.nodes = (const N *)w.walk->nodes;
                a.tree = TreeDev{w.walk->tree.levels, w.walk->tree.real_leaves, w.walk->tree.virtual_leaves};
                a.start_level = w.start_level;
                a.built_level = w.walk->built_level;
                a.narrow = narrow;
                a.positions = positions;
                a.flip = w.flip;
                const int xcd_env = g_tuning.lvt_xcd;
                a.xcd_tiles = MODE != MODE_RAYS ? xcd_env : 0; // 0: round robin, 1: one contiguous range per XCD, n > 1: runs of n
                a.counts = (I *)c.counts;
                a.contacts = (IndexPair<I> *)c.contacts;
                a.guard_total = nullptr;
                a.guard_capacity = 0;
                a.work = c.work;
                a.gate = nullptr;
                a.blk_rows = (uint32_t *)at(plan.rows);
                a.q_index_dense = (I *)at(plan.index);
                // (the scan's tile aggregates, behind the header of the scratch: scan_counts)
                const bool may_fuse = !write && !work && MODE != MODE_RAYS;
                a.scan_agg = may_fuse ? (unsigned long long *)at(SCAN_AGG_OFFSET) : nullptr;
                a.scan_nparts = (int32_t)scan_tiles(w.n_items);
                bool agg_zeroed = false;
                a.blk_shift = 0;
                const ibvh_bvh *qside = w.drv ? w.drv : w.walk;
                a.q_nodes = same_nodes ? (const N *)qside->nodes : nullptr;
                a.q_tree = TreeDev{qside->tree.levels, qside->tree.real_leaves, qside->tree.virtual_leaves};
                a.q_built_level = qside->built_level;
                PairCache<I> cache{(IndexPair<I> *)at(plan.cache), plan.K};
                // one pass: the walked leaves' own type, or (a mixed pair, IBVH_PAIR_MIXED_TYPES) the driving leaves' type Q
                auto pass = [&](bool wr, bool *agg) -> int {
                    if constexpr (MODE != MODE_PAIR) {
                        return launch<L, N, I, MODE>(a, cache, wr, st, bins, agg);
                    } else {
                        return dispatch_volume(w.drv->types.leaf_kind, w.drv->types.leaf_float, [&](auto qt) -> int {
                            using Q = typename decltype(qt)::type;
                            if constexpr (std::is_same<Q, L>::value) return launch<L, N, I, MODE>(a, cache, wr, st, bins, agg);
                            else if constexpr (N::kind == IBVH_BSPHERE && Q::kind != IBVH_BSPHERE) return (int)IBVH_ERR_UNSUPPORTED; // (pair_common refuses it first)
                            else return launch_pair_mixed<Q, L, N, I>(a, cache, wr, st, agg);
                        });
                    }
                };
                if (int e = pass(write, &agg_zeroed)) return e;
                if (write || work) return (int)IBVH_OK;
                ScanCall<I> scan;
                scan.counts = (I *)c.counts;
                scan.n = w.n_items;
                scan.scratch = c.scratch;
                scan.total_dev = (int64_t *)c.total_dev;
                scan.total_host = (int64_t *)c.total_host;
                scan.total_out = c.total_out;
                scan.aggregates_zeroed = agg_zeroed;
                if (int e = scan_counts(scan, st)) return e;
                if (enqueue && c.capacity > 0) {
                    a.guard_total = c.total_dev ? (const int64_t *)c.total_dev : (const int64_t *)c.scratch; // the total contacts
                    a.guard_capacity = sizeof(I) == 4 && c.capacity > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : c.capacity;
                    return pass(true, nullptr);
                }
                return (int)IBVH_OK;
            });
        }
    });
}

} // namespace lvt
} // namespace ibvh

using namespace ibvh;
using namespace ibvh::lvt;

extern "C" {

// Scratch for the *_count / *_write pair of calls on n_items work items.  cache_slots = contacts
// per work item kept from the counting pass (0 = none: the writing pass walks again; 8 is a good
// default at ~2 contacts per leaf).  The SAME buffer and size must be passed to both calls.
ibvh_status ibvh_lvt_scratch_bytes(const ibvh_types *types, int64_t n_items, int32_t cache_slots, size_t *bytes_out) {
    if (!types || !bytes_out || n_items < 0 || cache_slots < 0) return IBVH_ERR_INVALID_ARG;
    ibvh_layout lay;
    if (!layout_of(*types, lay)) return IBVH_ERR_UNSUPPORTED;
    if (cache_slots > MAX_CACHE_SLOTS) cache_slots = MAX_CACHE_SLOTS;
    // (BBox nodes: room for the rows of the shared descent and every work item's .index, behind the contact cache)
    *bytes_out = scratch_size(n_items, lay.pair_bytes, cache_slots, types->node_kind == IBVH_BBOX, 0);
    return IBVH_OK;
}

// Scratch for the ray traversal entry points: ibvh_lvt_scratch_bytes for num_rays work items, or, when the binned path
// serves the batch, that path's region behind a scratch without contact cache (see include/ibvh.h).
ibvh_status ibvh_rays_scratch_bytes(const ibvh_bvh *bvh, int64_t num_rays, int32_t cache_slots, size_t *bytes_out) {
    if (!bvh || !bytes_out || num_rays < 0 || cache_slots < 0) return IBVH_ERR_INVALID_ARG;
    const RayBinPlan bp = rays_bin_plan(*bvh, num_rays);
    if (!bp.depth) return ibvh_lvt_scratch_bytes(&bvh->types, num_rays, cache_slots, bytes_out);
    ibvh_layout lay; // (a tree the binned path serves has a supported layout: rays_bin_plan)
    layout_of(bvh->types, lay);
    // the binned path keeps no contact cache: its writing pass walks the subtrees out of LDS again
    *bytes_out = scratch_size(num_rays, lay.pair_bytes, 0, bvh->types.node_kind == IBVH_BBOX, bp.bytes);
    return IBVH_OK;
}

// nothing to walk (a single leaf, no rays): no contacts, and *_enqueue leaves a total of 0 where it would have left the count
static ibvh_status nothing_to_walk(const Call &c) {
    if (c.op != OP_ENQUEUE) return IBVH_OK;
    if (hipMemsetAsync(c.total_dev ? c.total_dev : c.scratch, 0, sizeof(int64_t), (hipStream_t)c.stream) != hipSuccess) return IBVH_ERR_HIP; // (header word 0)
    if (c.total_host) *(volatile int64_t *)c.total_host = 0; // (host memory: nothing was launched that could write it later)
    return IBVH_OK;
}

// traverse(bvh, LVTTraversal()) — lvt/traverse_single.jl:1-79.  buffers: the caller's own, needed only if there is a walk (:17-21)
static ibvh_status self_common(const ibvh_bvh *bvh, int64_t sl, int32_t narrow, bool buffers, const Call &c) {
    if (int e = check_levels(*bvh, sl)) return (ibvh_status)e;
    // (*_enqueue: the scratch header holds the total even when there is nothing to walk)
    if (c.op == OP_ENQUEUE && (!c.scratch || !scratch_holds_front(bvh->tree.real_leaves, c.scratch_bytes))) return IBVH_ERR_SCRATCH;
    if (bvh->tree.real_nodes <= 1) return nothing_to_walk(c);
    if (!buffers) return IBVH_ERR_INVALID_ARG;
    return (ibvh_status)run<MODE_SELF>({.drv = bvh, .walk = bvh, .n_items = bvh->tree.real_leaves, .start_level = sl, .narrow = narrow}, c);
}
ibvh_status ibvh_traverse_lvt_count(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow, void *counts,
                                    int64_t *total_out, void *scratch, size_t scratch_bytes, void *stream) {
    if (!bvh || !total_out) return IBVH_ERR_INVALID_ARG;
    *total_out = 0;
    return self_common(bvh, start_level, narrow, counts && scratch, {.op = OP_COUNT, .counts = counts, .total_out = total_out,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}
ibvh_status ibvh_traverse_lvt_write(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow, const void *counts,
                                    void *contacts, void *scratch, size_t scratch_bytes, void *stream) {
    if (!bvh) return IBVH_ERR_INVALID_ARG;
    return self_common(bvh, start_level, narrow, counts && contacts, {.op = OP_WRITE, .counts = (void *)counts, .contacts = contacts,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}

// count + scan + writing pass in one go, WITHOUT the host read of the total in between (the reference blocks there,
// traverse_single.jl:53-60): the writing pass is launched right behind the scan and does nothing unless the total
// fits `capacity` pairs.  The total stays in the scratch header: read it with ibvh_lvt_total whenever convenient;
// if it exceeds `capacity`, call ibvh_traverse_lvt_write with a larger buffer (counts and scratch are ready for it).
ibvh_status ibvh_traverse_lvt_enqueue(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow, void *counts, void *contacts,
                                      int64_t capacity, void *total_dev, void *total_host, void *scratch, size_t scratch_bytes,
                                      void *stream) {
    if (!bvh || capacity < 0) return IBVH_ERR_INVALID_ARG;
    return self_common(bvh, start_level, narrow, counts && (capacity == 0 || contacts),
                       {.op = OP_ENQUEUE, .counts = counts, .contacts = contacts, .capacity = capacity, .total_dev = total_dev,
                        .total_host = total_host, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}
// blocking read of the total contact count a *_count / *_enqueue call left in the scratch header
ibvh_status ibvh_lvt_total(const void *scratch, int64_t *total_out, void *stream) {
    if (!scratch || !total_out) return IBVH_ERR_INVALID_ARG;
    if (hipMemcpyAsync(total_out, scratch, sizeof(int64_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return IBVH_ERR_HIP;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return IBVH_ERR_HIP;
    return IBVH_OK;
}

// Work of ONE counting pass (see include/ibvh.h)
ibvh_status ibvh_lvt_work_counters(const ibvh_bvh *bvh, const ibvh_bvh *bvh2, const void *points, const void *directions,
                                   int64_t num_rays, void *counts, void *work_out, void *stream) {
    if (!bvh || !counts || !work_out) return IBVH_ERR_INVALID_ARG;
    const Call c{.op = OP_WORK, .counts = counts, .work = (unsigned long long *)work_out, .stream = stream};
    if (hipMemsetAsync(work_out, 0, 4 * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess) return IBVH_ERR_HIP;
    const int64_t sl = bvh->built_level > 1 ? bvh->built_level : 1;
    if (int e = check_levels(*bvh, sl)) return (ibvh_status)e; // (all three shapes: levels <= 32, built_level <= start level)
    if (points) {
        if (!directions || num_rays <= 0) return IBVH_ERR_INVALID_ARG;
        return (ibvh_status)run<MODE_RAYS>({.walk = bvh, .points = points, .dirs = directions, .n_items = num_rays, .start_level = sl}, c);
    }
    if (bvh2) {
        if (!same_types(bvh->types, bvh2->types)) return IBVH_ERR_UNSUPPORTED;
        const bool flip = !(bvh->tree.real_leaves >= bvh2->tree.real_leaves); // the BVH with more leaves drives (:15-36)
        const ibvh_bvh *drv = flip ? bvh2 : bvh, *oth = flip ? bvh : bvh2;
        const int64_t slo = oth->built_level > 1 ? oth->built_level : 1;
        if (int e = check_levels(*oth, slo)) return (ibvh_status)e;
        return (ibvh_status)run<MODE_PAIR>({.drv = drv, .walk = oth, .n_items = drv->tree.real_leaves, .start_level = slo, .flip = flip ? 1 : 0}, c);
    }
    return self_common(bvh, sl, IBVH_NARROW_NONE, true, c);
}

// traverse(bvh1, bvh2, LVTTraversal()) — lvt/traverse_pair.jl:1-116
static ibvh_status pair_common(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t sl1, int64_t sl2, int32_t narrow, const Call &c) {
    if (!bvh1 || !bvh2) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh1, sl1)) return (ibvh_status)e;
    if (int e = check_levels(*bvh2, sl2)) return (ibvh_status)e;
    // IBVH_PAIR_MIXED_TYPES: any two types with one index type (:50-52); without it, one type
    const bool mixed = (narrow & IBVH_PAIR_MIXED_TYPES) != 0;
    narrow &= ~IBVH_PAIR_MIXED_TYPES;
    if (mixed ? bvh1->types.index_type != bvh2->types.index_type : !same_types(bvh1->types, bvh2->types)) return IBVH_ERR_UNSUPPORTED;
    if (!c.counts) return IBVH_ERR_INVALID_ARG;
    // the BVH with more leaves supplies the work items; flip restores (bvh1, bvh2) order (:15-36).  IBVH_PAIR_SMALLER_DRIVES: the
    // other way round (the contact SET is the same; the list's order is the smaller BVH's leaf order)
    const bool smaller = (narrow & IBVH_PAIR_SMALLER_DRIVES) != 0;
    narrow &= ~IBVH_PAIR_SMALLER_DRIVES;
    const bool flip = smaller ? bvh1->tree.real_leaves > bvh2->tree.real_leaves : !(bvh1->tree.real_leaves >= bvh2->tree.real_leaves);
    const ibvh_bvh *drv = flip ? bvh2 : bvh1, *oth = flip ? bvh1 : bvh2;
    // the walked tree's nodes are tested against NodeType(query) (:196-197): there is no BSphere(::BBox), the reference raises
    if (drv->types.leaf_kind == IBVH_BBOX && oth->types.node_kind == IBVH_BSPHERE) return IBVH_ERR_UNSUPPORTED;
    return (ibvh_status)run<MODE_PAIR>({.drv = drv, .walk = oth, .n_items = drv->tree.real_leaves, .start_level = flip ? sl1 : sl2,
                                        .narrow = narrow, .flip = flip ? 1 : 0}, c);
}
ibvh_status ibvh_traverse_pair_lvt_count(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t sl1, int64_t sl2,
                                         int32_t narrow, void *counts, int64_t *total_out, void *scratch,
                                         size_t scratch_bytes, void *stream) {
    if (!total_out || !scratch) return IBVH_ERR_INVALID_ARG;
    *total_out = 0;
    return pair_common(bvh1, bvh2, sl1, sl2, narrow, {.op = OP_COUNT, .counts = counts, .total_out = total_out, .scratch = scratch,
                       .scratch_bytes = scratch_bytes, .stream = stream});
}
ibvh_status ibvh_traverse_pair_lvt_write(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t sl1, int64_t sl2,
                                         int32_t narrow, const void *counts, void *contacts, void *scratch,
                                         size_t scratch_bytes, void *stream) {
    if (!contacts) return IBVH_ERR_INVALID_ARG;
    return pair_common(bvh1, bvh2, sl1, sl2, narrow, {.op = OP_WRITE, .counts = (void *)counts, .contacts = contacts, .scratch = scratch,
                       .scratch_bytes = scratch_bytes, .stream = stream});
}
ibvh_status ibvh_traverse_pair_lvt_enqueue(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t sl1, int64_t sl2,
                                           int32_t narrow, void *counts, void *contacts, int64_t capacity, void *total_dev,
                                           void *total_host, void *scratch, size_t scratch_bytes, void *stream) {
    if (!scratch || capacity < 0 || (capacity > 0 && !contacts)) return IBVH_ERR_INVALID_ARG;
    return pair_common(bvh1, bvh2, sl1, sl2, narrow, {.op = OP_ENQUEUE, .counts = counts, .contacts = contacts, .capacity = capacity,
                       .total_dev = total_dev, .total_host = total_host, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}

// traverse_rays(bvh, points, directions, LVTTraversal()) — raytrace/leaf_vs_tree/leaf_vs_tree.jl:1-90
static ibvh_status rays_common(const ibvh_bvh *bvh, const void *points, const void *dirs, int64_t num_rays, int64_t sl,
                               int32_t narrow, const Call &c) {
    if (!bvh || num_rays < 0) return IBVH_ERR_INVALID_ARG;
    if (int e = check_levels(*bvh, sl)) return (ibvh_status)e;
    if (bvh->types.leaf_float != bvh->types.node_float) return IBVH_ERR_UNSUPPORTED;
    if (num_rays == 0) return nothing_to_walk(c); // :22-26
    if (!points || !dirs || !c.counts) return IBVH_ERR_INVALID_ARG;
    return (ibvh_status)run<MODE_RAYS>({.walk = bvh, .points = points, .dirs = dirs, .n_items = num_rays, .start_level = sl, .narrow = narrow}, c);
}
ibvh_status ibvh_traverse_rays_lvt_count(const ibvh_bvh *bvh, const void *points, const void *dirs, int64_t num_rays,
                                         int64_t sl, int32_t narrow, void *counts, int64_t *total_out, void *scratch,
                                         size_t scratch_bytes, void *stream) {
    if (!total_out) return IBVH_ERR_INVALID_ARG;
    *total_out = 0;
    if (num_rays > 0 && !scratch) return IBVH_ERR_INVALID_ARG;
    return rays_common(bvh, points, dirs, num_rays, sl, narrow, {.op = OP_COUNT, .counts = counts, .total_out = total_out,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}
ibvh_status ibvh_traverse_rays_lvt_write(const ibvh_bvh *bvh, const void *points, const void *dirs, int64_t num_rays,
                                         int64_t sl, int32_t narrow, const void *counts, void *contacts, void *scratch,
                                         size_t scratch_bytes, void *stream) {
    if (num_rays > 0 && !contacts) return IBVH_ERR_INVALID_ARG;
    return rays_common(bvh, points, dirs, num_rays, sl, narrow, {.op = OP_WRITE, .counts = (void *)counts, .contacts = contacts,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}
ibvh_status ibvh_traverse_rays_lvt_enqueue(const ibvh_bvh *bvh, const void *points, const void *dirs, int64_t num_rays,
                                           int64_t sl, int32_t narrow, void *counts, void *contacts, int64_t capacity,
                                           void *total_dev, void *total_host, void *scratch, size_t scratch_bytes, void *stream) {
    if (!scratch || capacity < 0 || (capacity > 0 && !contacts)) return IBVH_ERR_INVALID_ARG;
    return rays_common(bvh, points, dirs, num_rays, sl, narrow, {.op = OP_ENQUEUE, .counts = counts, .contacts = contacts,
                       .capacity = capacity, .total_dev = total_dev, .total_host = total_host, .scratch = scratch,
                       .scratch_bytes = scratch_bytes, .stream = stream});
}

} // extern "C"
