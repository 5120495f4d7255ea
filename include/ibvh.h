/*
 * ibvh.h — C ABI of libibvh, the MI355X (gfx950) implicit-BVH engine.
 *
 * This is the drop-in boundary for ImplicitBVH.jl's hot path (Morton encode ->
 * stable radix sort by Morton code (an MSD partition of whole records + an in-LDS
 * LSD finish; plain LSD passes for tiny inputs: the result is the stable order
 * either way) -> bottom-up ImplicitTree merge -> LVT / BFS traversal of one BVH,
 * two BVHs, or rays).  The reference has no FFI: its back-end seam is
 * Julia method dispatch on the array type (src/build.jl:198, src/traverse/
 * leaf_vs_tree/traverse_single.jl:1, src/raytrace/raytrace.jl:71).  A package
 * extension for AMDGPU.jl's ROCArray `ccall`s the entry points below (see
 * INTEGRATION.md); every one cites the reference function it replaces.
 *
 * Conventions
 *   - plain C, no HIP/torch types: `void *stream` is a hipStream_t (NULL = default
 *     stream); all buffer pointers are DEVICE pointers owned by the caller;
 *   - record layouts are the C layouts Julia gives its isbits structs:
 *       BSphere{T}            { T x[3]; T r; }                  (bsphere.jl:26-29)
 *       BBox{T}               { T lo[3]; T up[3]; }             (bbox.jl:35-38)
 *       BoundingVolume{V,I,M} { V volume; I index; M morton; }  (bounding_volumes.jl:55-59)
 *       IndexPair{I}          { I first; I second; }            (traverse.jl:6)
 *   - indices are 1-based exactly as in the reference;
 *   - every function returns an ibvh_status; nothing is allocated or freed by the
 *     library; calls are asynchronous on `stream` unless stated otherwise.
 */
#ifndef IBVH_H
#define IBVH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct layout or an entry point's argument list changes.  A binding checks
 * ibvh_abi_version() == IBVH_ABI_VERSION (the header it was written against) right after loading the
 * library and refuses a mismatch: a stale caller would otherwise hand the GPU garbage pointers.
 *   1: round 1   2: ibvh_build_desc.sort_levels / skew_flag, ibvh_bfs_result.resume_*, *_enqueue(total_dev)
 *   3: *_enqueue(total_host), ibvh_set_tuning, ibvh_lvt_work_counters, ray `narrow`, contact positions
 *   4: the multi-GPU driver (ibvh_comm, ibvh_dist_*)
 *   5: ibvh_dist_cross_* (boundary leaves), ibvh_comm_release, ibvh_build_desc.sort_equalize (was reserved_: same layout)
 *   6: IBVH_PAIR_MIXED_TYPES (pair LVT traversals of two BVHs of different leaf / node types)
 *   7: ibvh_refit; ibvh_rays_resolve_triangles (additive under 7: a new entry point, no struct layout or existing
 *      argument list moves, so a binding written against the earlier 7 keeps working); ibvh_closest_triangles (additive
 *      under 7 in the same way); ibvh_nearest_leaves and IBVH_NEAREST_MAX_K (additive under 7 in the same way);
 *      ibvh_point_crossings (additive under 7 in the same way); ibvh_cast_rays and IBVH_CAST_CLOSEST / IBVH_CAST_ANY
 *      (additive under 7 in the same way); ibvh_sphere_contacts and IBVH_SPHERES_COUNT / IBVH_SPHERES_WRITE (additive
 *      under 7 likewise: one more entry point);
 *      ibvh_triangle_contacts and IBVH_TRIS_COUNT / IBVH_TRIS_WRITE (additive under 7 likewise: one more entry point);
 *      ibvh_sweep_spheres and IBVH_SWEEP_CLOSEST / IBVH_SWEEP_ANY (additive under 7 likewise: one more entry point);
 *      ibvh_triangle_distances (additive under 7 likewise: one more entry point);
 *      ibvh_capsule_contacts and IBVH_CAPSULES_COUNT / IBVH_CAPSULES_WRITE, ibvh_segment_distances (additive under 7
 *      likewise: two more entry points);
 *      ibvh_box_contacts and IBVH_BOXES_COUNT / IBVH_BOXES_WRITE (additive under 7 likewise: one more entry point);
 *      ibvh_cast_spheres and IBVH_SPHERECAST_CLOSEST / IBVH_SPHERECAST_ANY (additive under 7 likewise: one more entry point);
 *      argument checks only, no layout or argument list moves: ibvh_key_histogram takes
 *      what fits its LDS staging (10 rows at 12-bit digits) and refuses shift > 63 and a negative prefix_shift,
 *      ibvh_pack_records / ibvh_dist_plan answer IBVH_ERR_OVERFLOW for an index past IBVH_I32 */
#define IBVH_ABI_VERSION 7
int32_t ibvh_abi_version(void);

/* ----------------------------------------------------------------------------------- */
/* status codes -> exceptions the Julia shim raises                                      */
/* ----------------------------------------------------------------------------------- */
typedef enum ibvh_status {
    IBVH_OK = 0,
    IBVH_ERR_INVALID_ARG = 1, /* ArgumentError (@argcheck in build.jl:207,235,260; lvt/traverse_single.jl:10) */
    IBVH_ERR_DOMAIN = 2,      /* DomainError: fewer than one leaf (implicit_tree.jl:78-80)                    */
    IBVH_ERR_UNSUPPORTED = 3, /* a type combination this library does not instantiate                        */
    IBVH_ERR_CAPACITY = 4,    /* caller buffer too small; the required size is reported                      */
    IBVH_ERR_OVERFLOW = 5,    /* a count does not fit the index type I                                       */
    IBVH_ERR_HIP = 6,         /* a HIP runtime call failed                                                    */
    IBVH_ERR_SCRATCH = 7,     /* scratch buffer smaller than ibvh_build_scratch_bytes()                      */
    IBVH_ERR_PEER = 8         /* multi-GPU calls: another rank's arguments were not acceptable — every rank returns
                                 together instead of waiting for it in a collective (that rank reports its own error) */
} ibvh_status;

/* ----------------------------------------------------------------------------------- */
/* type descriptors                                                                     */
/* ----------------------------------------------------------------------------------- */
enum { IBVH_BSPHERE = 0, IBVH_BBOX = 1 };       /* volume kinds                       */
enum { IBVH_F32 = 0, IBVH_F64 = 1 };            /* float types                        */
enum { IBVH_I32 = 0, IBVH_I64 = 1 };            /* index types (BVHOptions.index)     */
enum { IBVH_U16 = 0, IBVH_U32 = 1, IBVH_U64 = 2 }; /* Morton types (morton/default.jl:21) */

/* narrow-phase menu.  The reference takes an arbitrary Julia closure that is only ever
 * evaluated as `iscontact(...) && narrow(a, b)` at leaf level
 * (lvt/traverse_single.jl:170); closures cannot cross a C ABI, so a fixed menu is offered. */
enum {
    IBVH_NARROW_NONE = 0,      /* (a, b) -> true / (bv, p, d) -> true  (the reference defaults)        */
    IBVH_NARROW_MORTON_LT = 1, /* self / pair: (a, b) -> a.morton < b.morton (runtests.jl:1239)        */
    IBVH_NARROW_INDEX_LT = 2,  /* self / pair: (a, b) -> a.index < b.index                             */
    IBVH_NARROW_RAY_ORIGIN_OUTSIDE = 3, /* rays (raytrace/raytrace.jl:76): (bv, p, d) -> p lies outside
                                  bv.volume — drops the leaves a ray STARTS in (rays cast from a surface) */
    IBVH_NARROW_MASK = 0xff,
    /* Any other pure `narrow`: OR this flag into the `narrow` argument of a traversal (of its _count AND its _write /
     * _enqueue call) and the contact list holds leaf POSITIONS instead of user indices, in the same order:
     *   one BVH   (position of the query leaf, position of its partner) in bvh.leaves, 1-based, query first
     *             (the reference evaluates narrow(query, partner); the query is the leaf with the smaller position)
     *   two BVHs  (position in bvh1.leaves, position in bvh2.leaves)
     *   rays      (position of the leaf in bvh.leaves, iray)
     * so the caller can evaluate the predicate on the records itself and keep what passes: `narrow` is only ever
     * evaluated as `iscontact(...) && narrow(...)` at leaf level (lvt/traverse_single.jl:170,
     * bfs/traverse_single_gpu.jl:187, raytrace/leaf_vs_tree/leaf_vs_tree.jl:194), i.e. a post-filter. */
    IBVH_OUTPUT_POSITIONS = 0x100,
    /* Pair LVT traversals only: let the BVH with FEWER leaves supply the work items (the reference lets the larger one,
     * lvt/traverse_pair.jl:15-36 — and so does the library without this flag).  Same pairs, still (bvh1, bvh2) order inside a
     * pair, but the LIST is ordered by the smaller BVH's leaves, so it is not the reference's order: for callers that want the
     * contact SET.  A handful of leaves against a large tree then costs (few leaves) x (tree depth) instead of one work item —
     * and 8 cached contacts of scratch — per leaf of the large tree; the cross-shard completion uses it (a slice's thin boundary
     * shell against the neighbour's whole slice).  Size the scratch and `counts` for min(n1, n2) items then. */
    IBVH_PAIR_SMALLER_DRIVES = 0x200,
    /* Pair LVT traversals only (ibvh_traverse_pair_lvt_{count,write,enqueue}): accept two BVHs of DIFFERENT leaf / node / Morton
     * types with one index type (lvt/traverse_pair.jl:50-52).  Without the flag such a pair returns IBVH_ERR_UNSUPPORTED.  The
     * walk is the reference's: the driving BVH's leaves are tested against the walked tree's nodes as NodeType(leaf.volume)
     * (:196-197) and against its leaves with iscontact on the raw mixed types (iscontact.jl:2-28, the comparisons promote);
     * IBVH_NARROW_MORTON_LT compares the two Morton widths as uint64.  Same list, order included, as the reference.  A BBox
     * query against a tree with BSphere nodes has no NodeType(query) (no BSphere(::BBox): the reference raises MethodError):
     * IBVH_ERR_UNSUPPORTED, never a list — and since the BVH with more leaves drives, whether two types are refused can
     * depend on the sizes (and on IBVH_PAIR_SMALLER_DRIVES).  Scratch: the larger of ibvh_lvt_scratch_bytes over the two
     * BVHs' types, for n_items = max(n1, n2) (min(n1, n2) with IBVH_PAIR_SMALLER_DRIVES).  Composes with every other flag. */
    IBVH_PAIR_MIXED_TYPES = 0x400
};

typedef struct ibvh_types {
    int32_t leaf_kind;   /* IBVH_BSPHERE | IBVH_BBOX */
    int32_t leaf_float;  /* IBVH_F32 | IBVH_F64      */
    int32_t node_kind;
    int32_t node_float;
    int32_t index_type;  /* IBVH_I32 | IBVH_I64      */
    int32_t morton_type; /* IBVH_U16 | IBVH_U32 | IBVH_U64 */
} ibvh_types;

/* ImplicitTree{I} (implicit_tree.jl:52-67), widened to int64 at the boundary. */
typedef struct ibvh_tree {
    int64_t levels;
    int64_t real_leaves;
    int64_t real_nodes;
    int64_t virtual_leaves;
    int64_t virtual_nodes;
} ibvh_tree;

/* Byte layout of one BoundingVolume{V,I,M} record. */
typedef struct ibvh_layout {
    int64_t volume_bytes; /* sizeof(V)                       */
    int64_t node_bytes;   /* sizeof(N), the node volume type */
    int64_t index_off;
    int64_t morton_off;
    int64_t leaf_bytes;   /* sizeof(BoundingVolume{V,I,M})   */
    int64_t pair_bytes;   /* sizeof(IndexPair{I})            */
} ibvh_layout;

/* A built BVH as the traversals see it: struct BVH (build.jl:155-166). */
typedef struct ibvh_bvh {
    ibvh_types types;
    ibvh_tree tree;
    int64_t built_level;
    const void *leaves; /* real_leaves x BoundingVolume records, Morton-sorted    */
    const void *nodes;  /* (real_nodes - real_leaves) x node volumes              */
    const void *skips;  /* levels x I, see ibvh_compute_skips                     */
} ibvh_bvh;

#define IBVH_MAX_SORT_LEVELS 4

/* Inputs of one BVH construction: BVH(bounding_volumes, node_type; built_level, options)
 * (build.jl:198-271) with options.morton = DefaultMortonAlgorithm (morton/default.jl:21-40). */
typedef struct ibvh_build_desc {
    ibvh_types types;
    int64_t n;               /* number of bounding volumes (>= 1)                              */
    int64_t built_level;     /* integer level 1..levels (use ibvh_compute_build_level)         */
    int32_t already_wrapped; /* 1: `leaves` already holds BoundingVolume records whose .index
                                is kept (build.jl:220-222); 0: wrap `volumes`, index = 1..n  */
    int32_t compute_extrema; /* 1: derive mins/maxs from the centres (morton/default.jl:53)    */
    double mins[3];          /* used when compute_extrema == 0 (alg.mins / alg.maxs)           */
    double maxs[3];
    /* Skewed inputs (clustered clouds, surfaces, duplicates).  The sort first splits the leaves into the cells of a
     * coarse Morton grid; a cell too crowded for one workgroup is split again, by the key bits that vary inside it, by
     * up to IBVH_MAX_SORT_LEVELS further partition levels.  For a uniform cloud those levels find nothing to do but
     * still cost their launches (4 per level, ~2 us each), so their number is the caller's choice:
     *   sort_levels = k (0 .. IBVH_MAX_SORT_LEVELS; negative or larger = all): launch k extra levels.  Whatever is
     *   still crowded after them is sorted by one workgroup per piece — always correct, slow when pieces are large.
     * skew_flag (optional, may be NULL): 4 bytes the GPU can write — device memory or mapped pinned host memory.  Every
     * build stores there, in the low byte, how many extra levels its input would have used (0 for a uniform cloud; at
     * most one more than it was given) and, in the second byte, how full the fullest cell of the coarse grid was, in
     * 1/128 of what one workgroup sorts (128 = exactly full, saturating at 255), so a caller that rebuilds every time
     * step can pass sort_levels = (the levels the previous build reported, plus one spare level when that is not 0 or
     * the fullest cell was close to full) without ever synchronising (build.jl:109-126 reuse pattern); a cold build
     * should pass 2 or more. */
    int32_t sort_levels;
    /* sort_equalize != 0: the cells of the first partition are key RANGES of about equal population (splitters taken from a
     * sorted sample of the keys) instead of the cells of a regular grid: a surface mesh or a clustered cloud fills few grid
     * cells, and every crowded one costs a second move of its records (the extra levels above); with equalised cells only
     * runs of EQUAL keys longer than a workgroup sorts still need a level.  Costs two small launches (~15 - 25 us) that a
     * cloud filling its box does not need; the result is byte-identical either way.  A build that ran with it stores bit 16
     * of skew_flag = 1 while the plain grid would have had a crowded cell: a caller that rebuilds every step asks for
     * equalised cells when the previous build reported extra levels (low byte != 0) or that bit.  Bit 17 (equalised builds
     * with sort_levels > 0): more than half of the records sat in crowded cells all the same — runs of equal keys, which
     * no choice of cells can split; such a chain is better off with the plain grid (the sample's launches buy nothing).
     * Bit 18: this build ran with equalised cells (so a caller that goes back to the plain grid on the strength of bit 16 = 0
     * knows it is doing so on an ESTIMATE, and can give that one build a spare level). */
    int32_t sort_equalize;
    void *skew_flag;
} ibvh_build_desc;

/* ----------------------------------------------------------------------------------- */
/* host-side shape math (no GPU needed)                                                 */
/* ----------------------------------------------------------------------------------- */

/* ImplicitTree{I}(num_leaves) — implicit_tree.jl:77-90.  IBVH_ERR_DOMAIN when n < 1. */
ibvh_status ibvh_tree_shape(int64_t num_leaves, ibvh_tree *out);

/* compute_skips! — implicit_tree.jl:100-113; writes tree->levels int64 values (host). */
ibvh_status ibvh_compute_skips(const ibvh_tree *tree, int64_t *skips_out);

/* memory_index / level_indices / isvirtual — implicit_tree.jl:128-199 (host helpers). */
ibvh_status ibvh_memory_index(const ibvh_tree *tree, int64_t implicit_index, int64_t *out);
ibvh_status ibvh_level_indices(const ibvh_tree *tree, int64_t level, int64_t *start, int64_t *stop);
ibvh_status ibvh_isvirtual(const ibvh_tree *tree, int64_t implicit_index, int32_t *out);

/* compute_build_level for a fractional argument — build.jl:309-325:
 * round(I, levels + (1 - levels) * frac), ties to even like Julia's round. */
ibvh_status ibvh_compute_build_level(const ibvh_tree *tree, double frac, int64_t *out);

/* Record layout of the given type combination; IBVH_ERR_UNSUPPORTED if not instantiated. */
ibvh_status ibvh_layout_of(const ibvh_types *types, ibvh_layout *out);

/* ----------------------------------------------------------------------------------- */
/* build                                                                                */
/* ----------------------------------------------------------------------------------- */

/* Scratch bytes ibvh_build needs for n leaves of the given types. */
ibvh_status ibvh_build_scratch_bytes(const ibvh_types *types, int64_t n, size_t *bytes_out);

/* The whole of BVH(...) on device — build.jl:198-271:
 *   wrap (build.jl:328-352) -> extrema (morton/utils.jl:1-72) -> Morton encode
 *   (morton/default.jl:63-157) -> stable ascending sort by .morton (build.jl:248-253)
 *   -> compute_skips! -> aggregate_oibvh! down to built_level (build.jl:366-523).
 * volumes : n x V raw volumes; with desc->already_wrapped: NULL (sort `leaves` in place) or n source
 *           BoundingVolume records that are left untouched (`leaves` then receives the sorted copy)
 * leaves  : n x BoundingVolume records, written (or sorted in place, see above)
 * nodes   : (real_nodes - real_leaves) x N
 * skips   : levels x I
 * extrema_out : optional 6 x double device->host copy target is NOT provided; pass NULL or a
 *           DEVICE pointer to 6 values of the leaf float type (mins then maxs, expanded).
 */
ibvh_status ibvh_build(const ibvh_build_desc *desc, const void *volumes, void *leaves, void *nodes,
                       void *skips, void *extrema_out, void *scratch, size_t scratch_bytes,
                       void *stream);

/* Stand-alone pieces of the build, exposed for tests, profiling and the multi-GPU driver. */

/* bounding_volumes_extrema (morton/utils.jl:55-72): 6 values of the leaf float type
 * (xmin,ymin,zmin,xmax,ymax,zmax), epsilon-expanded when `expand` != 0, written to DEVICE
 * memory `extrema_out`.  `records` are raw volumes (stride volume_bytes) when wrapped == 0. */
ibvh_status ibvh_extrema(const ibvh_types *types, const void *records, int32_t wrapped, int64_t n,
                         int32_t expand, void *extrema_out, void *scratch, size_t scratch_bytes,
                         void *stream);

/* _morton_encode! (morton/default.jl:63-108) into a separate key array (uint32 for U16/U32,
 * uint64 for U64) using DEVICE extrema (6 x leaf float, already expanded). */
ibvh_status ibvh_morton_keys(const ibvh_types *types, const void *records, int32_t wrapped,
                             int64_t n, const void *extrema, void *keys_out, void *stream);

/* Stable radix sort of (key, value=uint32) pairs (LSD passes, or one MSD partition + in-LDS bucket sort, chosen
 * from n: same result); key_bits = significant low bits.
 * keys/vals are sorted into keys_out/vals_out (may alias the alt buffers as documented in
 * DESIGN.md); key_bytes is 4 or 8. */
ibvh_status ibvh_sort_pairs(int32_t key_bytes, int32_t key_bits, int64_t n, void *keys, void *vals,
                            void *keys_alt, void *vals_alt, int32_t *result_in_alt, void *scratch,
                            size_t scratch_bytes, void *stream);
ibvh_status ibvh_sort_scratch_bytes(int32_t key_bytes, int64_t n, size_t *bytes_out);

/* aggregate_oibvh! alone (build.jl:366-523) over already-sorted leaves. */
ibvh_status ibvh_aggregate(const ibvh_types *types, const ibvh_tree *tree, int64_t built_level,
                           const void *leaves, void *nodes, void *stream);

/* Refit: new leaf volumes into bvh's EXISTING leaf order, then aggregate_oibvh! (build.jl:366-523) again down to
 * bvh->built_level; no extrema, Morton codes or sort.  Leaf .index / .morton, the skips and the tree are unchanged (the
 * Morton codes stay those of the last full build: they are the key the leaves are ORDERED by), and the nodes are
 * bit-identical to ibvh_aggregate over the updated records.  Every traversal stays exact; only its cost grows as the
 * leaf order drifts away from the Morton order of the new volumes — when to build again is the caller's decision.
 * bvh->leaves and bvh->nodes are WRITTEN (the const of ibvh_bvh is the traversals' view).
 *   volumes == NULL: bvh->leaves already hold the new volumes (moved in place): exactly ibvh_aggregate.
 *   volumes != NULL: num_volumes raw volumes of the leaf type (8-byte aligned, not overlapping the leaves); the leaf
 *                    with user index k receives volumes[k-1], in the first launch of the merge.
 * flag (optional, may be NULL): 4 bytes the GPU can write (device memory or mapped pinned host memory).  A leaf whose
 * .index lies outside 1..num_volumes keeps its volume, nothing outside the array is read, and the kernel stores a
 * non-zero value there.  The library never clears it: zero it before the call.  No host synchronisation. */
ibvh_status ibvh_refit(const ibvh_bvh *bvh, const void *volumes, int64_t num_volumes, void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* leaf-vs-tree traversal (LVTTraversal, the reference default)                          */
/* ----------------------------------------------------------------------------------- */
/* The reference's own two-pass protocol (lvt/traverse_single.jl:53-75):
 *   _count : pass 1 + inclusive scan of the per-work-item counts; SYNCHRONISES the stream and
 *            returns the total (the reference's `@allowscalar thread_ncontacts[end]`, :60);
 *   _write : pass 2, contact k of work item i lands at counts[i-1] + k (1-based), which makes
 *            the contact list order deterministic and identical to the reference's.
 * counts : one I per work item (cache2 of BVHTraversal on the GPU path, :31-32).
 * scratch: ibvh_lvt_scratch_bytes() bytes of device memory: scan tile sums + the contact cache + (BBox nodes) the rows of
 *          the shared descent: one list of cut-level nodes per block of 2,048 consecutive leaves, made by one small kernel
 *          in front of the counting pass and read by both passes (csrc/ibvh_lvt.hpp "BlockRows"), and a dense copy of the
 *          work items' .index (4 / 8 bytes an item) that the counting pass leaves for the writing pass, which then does not
 *          touch the leaf records at all; a scratch without room for either is served without it.
 *          Layout (csrc/ibvh_lvt_scratch.hpp, ScratchPlan — one description for the size queries and the launches):
 *            [ 64-byte header | scan tile sums | contact cache: K slots x n_items pairs | ...gap... | tail ]
 *          The tail is anchored at the END of `scratch_bytes`, aligned down to 256: [index array | rows] (self / pair under
 *          BBox nodes) or the binned ray path's tables.  A buffer smaller than the size query's answer loses the index array
 *          first, then the rows (the ray tables as a whole); the contact cache gets the slots (<= 64) that fit between the
 *          scan sums and the tail; below header + scan sums the call answers IBVH_ERR_SCRATCH.
 * NaN: with BBox nodes the walkers rely on parents being the exact minima / maxima of their children (merge.jl:30-40): a
 *      contact is decided by the leaf parent's box and the leaf test, the levels above only prune.  On volumes whose boxes
 *      hold no NaN that is the reference's list, element for element.  A NaN leaf box (a NaN radius; Inf - Inf in the
 *      sphere -> box conversion) can make merge.jl's `a < b ? a : b` produce a NaN NODE box above NaN-free leaves; the
 *      reference's walk then prunes those leaves at that node, while this library tests the node levels from level 7 down to
 *      the level of the 128-leaf subtrees and then the leaf parents: on such trees its list is a superset of the
 *      reference's (tests/test_gpu_lvt_blocks.py::test_nan_and_infinite_radii pins the relation).  Infinite boxes are exact.
 */
/* cache_slots: contacts per work item (on average) the counting pass keeps for the writing pass (0 = none: the
 * writing pass walks the tree again; 8 suits ~2 contacts per leaf).  The BBox-node and ray walkers pool the slots of
 * the 64 work items of a wave (a wave walks again only if ALL its items together found more than ~42 * cache_slots
 * contacts); the exact walk keeps the first cache_slots contacts of every item.  Pass the SAME scratch buffer and size
 * to the _count call and its _write call. */
ibvh_status ibvh_lvt_scratch_bytes(const ibvh_types *types, int64_t n_items, int32_t cache_slots,
                                   size_t *bytes_out);
ibvh_status ibvh_traverse_lvt_count(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow,
                                    void *counts, int64_t *total_out, void *scratch,
                                    size_t scratch_bytes, void *stream);
ibvh_status ibvh_traverse_lvt_write(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow,
                                    const void *counts, void *contacts, void *scratch,
                                    size_t scratch_bytes, void *stream);

/* traverse(bvh1, bvh2, LVTTraversal()) — lvt/traverse_pair.jl:1-244.  The BVH with more leaves
 * supplies the work items (:15-36); contacts are always (index in bvh1, index in bvh2).
 * counts needs max(n1, n2) entries.  Two BVHs of different types: IBVH_PAIR_MIXED_TYPES. */
ibvh_status ibvh_traverse_pair_lvt_count(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2,
                                         int64_t start_level1, int64_t start_level2,
                                         int32_t narrow, void *counts, int64_t *total_out,
                                         void *scratch, size_t scratch_bytes, void *stream);
ibvh_status ibvh_traverse_pair_lvt_write(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2,
                                         int64_t start_level1, int64_t start_level2,
                                         int32_t narrow, const void *counts, void *contacts,
                                         void *scratch, size_t scratch_bytes, void *stream);

/* traverse_rays(bvh, points, directions, LVTTraversal()) — raytrace/leaf_vs_tree/
 * leaf_vs_tree.jl:1-228.  points/directions: (3, num_rays) column-major arrays of the leaf
 * float type; contacts are (leaf.index, iray); `narrow`: IBVH_NARROW_NONE / _RAY_ORIGIN_OUTSIDE (| IBVH_OUTPUT_POSITIONS).
 * Scratch: ibvh_rays_scratch_bytes().  For trees of >= 17 levels (>= 13 under batches of <= 8,192 rays; not for a tree of
 * < 2^20 leaves under more than two rays per leaf) it holds the tables
 * of the BINNED path (csrc/ibvh_lvt.hip "(3c)": the walk is cut at a level, the hits at that level are grouped by subtree
 * and the walks are finished subtree by subtree out of LDS — the reference's walk cut in two, the same hit list in the same
 * order): 40 bytes x 16 items per ray (batches of up to 8 M rays).  A call that needs more raises a flag on the device and is served by the binary
 * walker in the same launch sequence; a caller that passes a smaller buffer (ibvh_lvt_scratch_bytes) gets the binary
 * walker from the start.  Otherwise it is ibvh_lvt_scratch_bytes(num_rays work items).  (A quantised 8-wide shadow
 * walker, measured slower than the binary walk — DESIGN.md §8.3 — was removed from the sources; commit f9264f8 is the
 * last that holds it.)  Pass the SAME scratch buffer and size to a _count call and its _write call. */
ibvh_status ibvh_rays_scratch_bytes(const ibvh_bvh *bvh, int64_t num_rays, int32_t cache_slots, size_t *bytes_out);
ibvh_status ibvh_traverse_rays_lvt_count(const ibvh_bvh *bvh, const void *points,
                                         const void *directions, int64_t num_rays,
                                         int64_t start_level, int32_t narrow, void *counts,
                                         int64_t *total_out, void *scratch, size_t scratch_bytes,
                                         void *stream);
ibvh_status ibvh_traverse_rays_lvt_write(const ibvh_bvh *bvh, const void *points,
                                         const void *directions, int64_t num_rays,
                                         int64_t start_level, int32_t narrow, const void *counts,
                                         void *contacts, void *scratch, size_t scratch_bytes,
                                         void *stream);

/* _enqueue : _count + _write without the host read in between, for callers that already own a contact
 *   buffer (the reference's `cache=` reuse, traverse.jl:54-107): pass 1, the scan and pass 2 are enqueued
 *   back to back and NOTHING synchronises the stream; pass 2 does nothing unless the total fits
 *   `capacity` pairs.  The total is written to `total_dev`, a DEVICE pointer to one int64 owned by the caller
 *   (NULL: the first 8 bytes of `scratch`), and — when `total_host` is not NULL — also to that int64 in MAPPED
 *   PINNED HOST memory (hipHostMalloc; the store is a system-scope release, so a host that set the word to a
 *   sentinel before the call can poll it instead of synchronising the stream: the reference's blocking
 *   `@allowscalar` read, lvt/traverse_single.jl:60, without the copy and the stream sync).  Otherwise
 *   fetch it with ibvh_lvt_total() when it is needed; if it exceeds
 *   `capacity`, grow the buffer and call the matching _write (counts and scratch are ready for it).  A caller that
 *   chains traversals through one scratch buffer and reads the totals late gives every call its own `total_dev`
 *   word: the scratch (header included) is rewritten by the next call.  Replaces the same reference lines as
 *   _count/_write; only the place of the blocking read (`@allowscalar`, lvt/traverse_single.jl:60) moves. */
ibvh_status ibvh_traverse_lvt_enqueue(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow,
                                      void *counts, void *contacts, int64_t capacity, void *total_dev,
                                      void *total_host, void *scratch, size_t scratch_bytes, void *stream);
ibvh_status ibvh_traverse_pair_lvt_enqueue(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2,
                                           int64_t start_level1, int64_t start_level2, int32_t narrow,
                                           void *counts, void *contacts, int64_t capacity, void *total_dev,
                                           void *total_host, void *scratch, size_t scratch_bytes, void *stream);
ibvh_status ibvh_traverse_rays_lvt_enqueue(const ibvh_bvh *bvh, const void *points,
                                           const void *directions, int64_t num_rays,
                                           int64_t start_level, int32_t narrow, void *counts, void *contacts,
                                           int64_t capacity, void *total_dev, void *total_host, void *scratch,
                                           size_t scratch_bytes, void *stream);
/* blocking read of the total a _count / _enqueue call left behind: pass the call's `total_dev`, or its `scratch`
 * when total_dev was NULL */
ibvh_status ibvh_lvt_total(const void *total_dev_or_scratch, int64_t *total_out, void *stream);

/* ----------------------------------------------------------------------------------- */
/* ray hit lists against the mesh's triangles                                           */
/* ----------------------------------------------------------------------------------- */
/* Resolve the (leaf.index, iray) list of an LVT ray traversal (ibvh_traverse_rays_lvt_{write,enqueue}) against the triangles
 * the bounding volumes were made from (ibvh_volumes_from_triangles): the exact ray-triangle test per candidate, and per
 * ray the nearest hit.  No reference counterpart (the reference stops at the candidate list); one launch, NO host
 * synchronisation.  The leaf and node kinds of the BVH do not matter: only the list is read.
 *   flt, index_type : IBVH_F32 | IBVH_F64, IBVH_I32 | IBVH_I64 (anything else: IBVH_ERR_UNSUPPORTED)
 *   triangles  : num_triangles x 9 values of `flt` (p1 p2 p3); user index k is row k - 1
 *   points, directions, num_rays : as for ibvh_traverse_rays_lvt_*
 *   counts     : the traversal's inclusive scanned counts (num_rays x I): ray i (1-based) owns candidates
 *                counts[i-1] .. counts[i] - 1 (0-based rows of `contacts`; counts[0] is taken as 0 for the first ray).
 *                The total is counts[num_rays - 1], read on the device.
 *   contacts   : the list, `capacity` rows of IndexPair{I}
 * Outputs — every pointer optional, at least one non-NULL (else IBVH_ERR_INVALID_ARG, like NULL required pointers and
 * negative sizes):
 *   closest_index : num_rays x I, the winning triangle's user index; 0 = miss
 *   closest_t     : num_rays x flt; +Inf = miss
 *   closest_uv    : num_rays x 2 x flt, the hit's barycentric (u, v) (weights of p2, p3); 0, 0 on a miss
 *   cand_t        : capacity x flt, per candidate: t of an exact hit, +Inf otherwise — for callers that want ALL exact hits;
 *                   rows at and beyond the total are not written
 * The test, in `flt`, every operation rounded once (nothing fused; correctly rounded divide), so that it can be pinned bit
 * for bit: a = p1, b = p2, c = p3, ray p + t d:
 *     e1 = b - a;  e2 = c - a;  pv = d x e2;  det = e1 . pv;  inv = 1 / det;  tv = p - a;
 *     u = (tv . pv) * inv;  qv = tv x e1;  v = (d . qv) * inv;  t = (e2 . qv) * inv
 *   with (x x y)[0] = x1*y2 - x2*y1 (cyclic) and x . y = (x0*y0 + x1*y1) + x2*y2.  A candidate is a hit iff
 *     det != 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= 0      (every comparison false on NaN)
 *   two-sided (no back-face culling) and forwards only (like the reference's `tmax >= 0`, isintersection.jl:1-65).
 * Closest hit: the smallest t wins; on equal t (-0 == +0 counts as equal) the candidate EARLIER in the list.  The outputs
 * carry the winner's bits unchanged.  A segmented minimum over the ray's candidates: no atomics, deterministic.
 * Guards: when the device total exceeds `capacity` the list was never written (see _enqueue): nothing is written except
 * bit 0 of `flag`.  A candidate whose index lies outside 1..num_triangles is a miss, nothing outside the array is read,
 * and bit 1 of `flag` is set.  flag (optional, may be NULL): 4 bytes the GPU can write, the contract of ibvh_refit's:
 * the library never clears it: zero it before the call.
 * Exact ON THE LIST IT IS GIVEN: the broad phase is the reference's rounded slab / sphere test (isintersection.jl), so a
 * grazing triangle hit that the broad phase rounded away is not recovered here, and this test is not watertight along
 * shared edges (a ray through an edge can miss both triangles or hit both).
 * Not for BFS lists (not grouped by ray: `counts` does not describe them) nor IBVH_OUTPUT_POSITIONS lists (leaf positions,
 * not triangle numbers): the library cannot tell either from the buffers, the caller must not pass them. */
ibvh_status ibvh_rays_resolve_triangles(int32_t flt, int32_t index_type, const void *triangles, int64_t num_triangles,
                                        const void *points, const void *directions, int64_t num_rays,
                                        const void *counts, const void *contacts, int64_t capacity,
                                        void *closest_index, void *closest_t, void *closest_uv, void *cand_t,
                                        void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* closest point on the mesh for a batch of query points                                */
/* ----------------------------------------------------------------------------------- */
/* For every query point: the closest triangle of the mesh the BVH was built over (ibvh_volumes_from_triangles with
 * IBVH_BBOX), the closest point on it and the squared distance.  No reference counterpart (every traversal of the reference
 * is a fixed-volume overlap test); ONE launch, NO host synchronisation, no atomics, no scratch buffer.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   points     : num_points x 3 row-major values of `flt`, processed in the order given (neighbours in memory that are
 *                neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   max_distance2 : HOST pointer to one value of `flt`, the SQUARED search radius; NULL = +Inf (unbounded)
 * Outputs — every pointer optional, at least one non-NULL:
 *   closest_index : num_points x I, the winning triangle's user index; 0 = no triangle within the radius
 *   closest_d2    : num_points x flt; +Inf = none
 *   closest_point : num_points x 3 x flt; 0, 0, 0 = none
 * All arguments are validated before any launch: NULL required pointers, negative sizes, no output at all, a tree shape
 * that is not an ImplicitTree's: IBVH_ERR_INVALID_ARG.  num_points == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found.  (d2_k, q_k) being the evaluation of triangle k below, the answer
 * for p is the LEXICOGRAPHIC MINIMUM of (d2_k, k) over all k with d2_k <= max_distance2: the smallest distance, and among
 * equal distances the SMALLER INDEX.  Every comparison is false on NaN: a triangle whose d2 is NaN never wins, a NaN query
 * point has no answer.  The outputs carry the winner's d2 and q bits unchanged.
 * The evaluation, in `flt`, every operation rounded once (nothing fused; correctly rounded divide), so that it can be
 * pinned bit for bit: x . y = (x0*y0 + x1*y1) + x2*y2, a = p1, b = p2, c = p3, and (Ericson's region walk) with
 *     ab = b - a;  ac = c - a;  ap = p - a;  d1 = ab . ap;  d2 = ac . ap
 *     bp = p - b;  d3 = ab . bp;  d4 = ac . bp;  cp = p - c;  d5 = ab . cp;  d6 = ac . cp
 *     vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *   the FIRST matching case decides:
 *     0: d1 <= 0 && d2 <= 0                        q = a
 *     1: d3 >= 0 && d4 <= d3                       q = b
 *     2: vc <= 0 && d1 >= 0 && d3 <= 0             v = d1 / (d1 - d3);  q = a + v*ab
 *     3: d6 >= 0 && d5 <= d6                       q = c
 *     4: vb <= 0 && d2 >= 0 && d6 <= 0             w = d2 / (d2 - d6);  q = a + w*ac
 *     5: va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0   w = (d4-d3) / ((d4-d3) + (d5-d6));  q = b + w*(c - b)
 *     6: otherwise                                 den = 1 / ((va + vb) + vc);  v = vb*den;  w = vc*den;  q = (a + v*ab) + w*ac
 *   then, per component, q is clamped into the triangle's exact box, lo = min3(a, b, c), up = max3(a, b, c) (the
 *   `x < y ? x : y` ternaries of BBox{T}(p1, p2, p3)):   q = q < lo ? lo : (q > up ? up : q)   (NaN stays NaN)
 *   and   e = p - q;  d2 = (e0*e0 + e1*e1) + e2*e2.
 * Why the clamp: it makes pruning lossless WITHOUT an epsilon.  For a box B that contains the triangle's box,
 *     c = clamp(p, B.lo, B.up) per component;  f = p - c;  lb(B) = (f0*f0 + f1*f1) + f2*f2
 *   is the same operation order as d2; round-to-nearest subtraction, squaring and addition are monotone and q lies inside
 *   B per component, so the COMPUTED lb(B) <= the COMPUTED d2 of every triangle under B.  The walk skips a node or a leaf
 *   iff lb > best d2 so far (which starts at max_distance2) — strictly: lb == best may hide an equal d2 of smaller index.
 *   Traversal order and work mapping therefore cannot change the result.  (On ordinary meshes the clamp changes no q: it
 *   is a guard for the proof.)
 * Accepted BVHs — the bound needs boxes that contain their triangles' boxes exactly:
 *   leaf_kind == node_kind == IBVH_BBOX, triangles and points of leaf_float, node_float the same as or wider than
 *   leaf_float (box merges are min / max plus a widening conversion: exact); any index and Morton type.  Anything else —
 *   sphere leaves, sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.
 *   Exact PROVIDED every leaf's box contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH
 *   after ibvh_refit.  Levels above bvh->built_level are not read.
 * NaN: a triangle with a NaN vertex has a NaN d2 and never wins, and a NaN query point (or radius) has no answer.  But, as
 *   for the traversals above, a NaN leaf box can make merge.jl's `a < b ? a : b` produce a node box that does NOT contain
 *   the NaN-free leaves below it (min(min(1, NaN), 5) = 5): on a mesh with NaN vertices the other triangles' answers are
 *   only guaranteed in trees of at most two leaves.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped, nothing outside the array is read, and bit 1 of `flag` is set — the flag contract of
 * ibvh_rays_resolve_triangles: optional, 4 bytes the GPU can write, a plain load and store, never cleared by the library
 * (zero it before the call). */
ibvh_status ibvh_closest_triangles(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                   const void *points, int64_t num_points, const void *max_distance2,
                                   void *closest_index, void *closest_d2, void *closest_point,
                                   void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* k nearest leaves for a batch of query points                                         */
/* ----------------------------------------------------------------------------------- */
/* For every query point: the k leaves of the BVH whose CENTRES are nearest, and their squared distances, optionally within
 * a search radius.  No reference counterpart (every traversal of the reference is a fixed-volume overlap test); ONE launch,
 * NO host synchronisation, no atomics, no scratch buffer.  Sphere leaves and box leaves.
 *   points     : num_points x 3 row-major values of bvh->types.leaf_float, `flt` below, processed in the order given
 *                (neighbours in memory that are neighbours in space walk the same nodes: sort a scattered batch along a
 *                Morton curve first)
 *   k          : 1 .. IBVH_NEAREST_MAX_K
 *   max_distance2 : HOST pointer to one value of `flt`, the SQUARED search radius; NULL = +Inf (unbounded)
 * Outputs — each optional, at least one non-NULL:
 *   nearest_index : num_points x k x I, row i = the user indices (.index of the leaf records) of point i's answers
 *   nearest_d2    : num_points x k x flt, their squared distances
 *   Row i holds the answers in ASCENDING (d2, index) order.  Slots beyond the answers hold 0 / +Inf = unfilled: fewer than k
 *   leaves, fewer than k within the radius, a NaN query point (or radius).  (With caller-supplied indices that may be 0, or an
 *   unbounded search in which a distance overflows to +Inf, the pair 0 / +Inf can also be an answer: a row has as many
 *   answers as there are leaves with d2 <= max_distance2, capped at k.)
 * All arguments are validated before any launch: NULL required pointers, negative sizes, k out of range, no output at all, a
 * tree shape that is not an ImplicitTree's: IBVH_ERR_INVALID_ARG.  num_points == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found.  In `flt`, every operation rounded once (nothing fused):
 *     c_j  = center(volume of leaf j): a sphere's x (bsphere.jl:142); a box's 0.5 * (lo + up) per component (bbox.jl:100-102)
 *     e    = p - c_j;   d2_j = (e0*e0 + e1*e1) + e2*e2          (dist3sq's order, utils.jl:168-171)
 *   and the answer for p is the k LEXICOGRAPHICALLY SMALLEST (d2_j, index_j) over ALL leaves j with d2_j <= max_distance2:
 *   the smallest distances, and among equal distances the SMALLER INDEX.  Every comparison is false on NaN: a leaf whose d2
 *   is NaN is never an answer, a NaN query point has none.  The outputs carry the winners' bits unchanged.
 * Pruning is lossless WITHOUT an epsilon, by the argument of ibvh_closest_triangles.  For a box B that contains c_j,
 *     c = clamp(p, B.lo, B.up) per component;  f = p - c;  lb(B) = (f0*f0 + f1*f1) + f2*f2
 *   is the same operation order as d2_j, |p - c| <= |p - c_j| per component, and round-to-nearest subtraction, squaring and
 *   addition are monotone: the COMPUTED lb(B) <= the COMPUTED d2_j.  The walk skips a node or a leaf iff lb > the k-th best
 *   (d2) so far (which starts at max_distance2) — strictly: lb == that may hide an equal d2 of smaller index.  A leaf is
 *   bounded by its stored volume's box — for a sphere x -/+ r computed in `flt`, as the merge forms it (merge.jl:47-51) —
 *   and only then is its centre distance taken.  Traversal order and work mapping therefore cannot change the result.
 * What makes it exact: EVERY LEAF CENTRE MUST LIE IN THE BOXES ABOVE IT (its own and every node's on its path).
 *   Boxes with lo <= up whose lo + up does not overflow: holds (lo <= 0.5 * (lo + up) <= up after rounding; node boxes are
 *   exact minima / maxima, merge.jl:30-40).  Spheres with r >= 0: x - r <= x <= x + r after rounding, and the parent of two
 *   leaves is the minima / maxima of the two x -/+ r (merge.jl:58-81) — except where that merge takes its shortcut
 *   `dist(a, b) + a.r <= b.r`: the parent is then b's box alone, and a's centre is inside it up to the rounding of that
 *   distance (a sphere inside another with less than a few ulp to spare; exact again when the centres coincide, as for
 *   duplicates).  Holds after ibvh_refit (the same merges over the moved volumes).  Infinite radii are fine (the box is all
 *   of space).  A negative radius (x + r < x - r) voids it.
 * Accepted BVHs: node_kind == IBVH_BBOX, leaf_kind IBVH_BSPHERE or IBVH_BBOX, node_float the same as or wider than leaf_float
 *   (a widening conversion is exact); any index and Morton type.  Anything else — sphere nodes, F64 leaves under F32 nodes —
 *   is IBVH_ERR_UNSUPPORTED, never an answer.  Levels above bvh->built_level are not read.
 * NaN: a leaf whose centre holds a NaN has a NaN d2 and is never an answer.  But, as for ibvh_closest_triangles, a NaN leaf
 *   box (a NaN radius; Inf - Inf) can make merge.jl's `a < b ? a : b` produce a node box that does NOT contain the NaN-free
 *   leaves below it: on volumes with NaN the other leaves' answers are only guaranteed in trees of at most two leaves.
 * No flag word: nothing is gathered through an index, there is nothing to guard. */
#define IBVH_NEAREST_MAX_K 16
ibvh_status ibvh_nearest_leaves(const ibvh_bvh *bvh, const void *points, int64_t num_points, int32_t k,
                                const void *max_distance2, void *nearest_index, void *nearest_d2, void *stream);

/* ----------------------------------------------------------------------------------- */
/* inside / outside: the triangles an axis ray from a query point crosses               */
/* ----------------------------------------------------------------------------------- */
/* For every query point P: the triangles of the mesh the BVH was built over (ibvh_volumes_from_triangles with IBVH_BBOX)
 * that the ray P + t*e_axis, t > 0, crosses — how many, and the signed sum of their orientations.  On a closed mesh that is
 * the side of the surface P lies on.  No reference counterpart (every traversal of the reference is a fixed-volume overlap
 * test, and its ray test has no rule for a ray through a shared edge or vertex); ONE launch, NO host synchronisation, no
 * atomics, no scratch buffer.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   points     : num_points x 3 row-major values of `flt`, processed in the order given (neighbours in memory that are
 *                neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   axis       : 0, 1 or 2: the ray runs along +x, +y or +z
 * Outputs — each optional, at least one non-NULL; what was not asked for is not written:
 *   crossings  : num_points x I, the number of crossing triangles
 *   winding    : num_points x I, the number of ccw crossings minus the number of cw ones: +1 inside an outward-oriented
 *                closed mesh, -1 inside an inward-oriented one, 0 outside
 * All arguments are validated before any launch: NULL required pointers, negative sizes, no output at all, an axis outside
 * 0..2, a tree shape that is not an ImplicitTree's: IBVH_ERR_INVALID_ARG.  num_points == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found: both counts run over ALL triangles.  With the CYCLIC coordinates
 *     u = (axis + 1) % 3;  v = (axis + 2) % 3;  w = axis        (cyclic: orientation is preserved)
 * a triangle (A, B, C) = (p1, p2, p3) is a crossing iff rules 1 to 4 hold, in `flt`, every operation rounded once (nothing
 * fused), so that it can be pinned bit for bit:
 *   1. Guard:  P.u >= min3(A.u, B.u, C.u) && P.u <= max3(A.u, B.u, C.u), the same for v, and max3(A.w, B.w, C.w) >= P.w
 *      (min3 / max3: the `x < y ? x : y` ternaries of BBox{T}(p1, p2, p3)).  Comparisons only, false on NaN.
 *   2. Edges:  for each directed edge (X, Y) in (A, B), (B, C), (C, A): put the endpoints in CANONICAL order —
 *        flipped = Y is lexicographically smaller than X on (u, v, w);  swap X and Y if so —
 *        e = (Y.u - X.u)*(P.v - X.v) - (Y.v - X.v)*(P.u - X.u)      on the canonical pair
 *        left = (e >= 0)      a tie goes LEFT of the canonical edge
 *        side = left XOR flipped
 *   3. Orientation:  ccw = all three sides true;  cw = all three false;  anything else is no crossing.
 *   4. Depth:  ab = B - A;  ac = C - A;  d = P - A, each in (u, v, w);
 *        N = (ab.v*ac.w - ab.w*ac.v,  ab.w*ac.u - ab.u*ac.w,  ab.u*ac.v - ab.v*ac.u);   s = (N0*d.u + N1*d.v) + N2*d.w
 *      a crossing iff (ccw && s < 0) || (cw && s > 0);  s == 0 (P on the plane) and NaN are no crossing.
 * Why the canonical edge: it makes the count WATERTIGHT without exact arithmetic.  Two triangles that share an edge — its
 *   endpoints bit-identical in both — compute the same bits for e and put P on the same side of that edge's line, ties
 *   included, so a ray through a shared edge or a shared vertex crosses the surface once, not zero or two times.
 * Why pruning is lossless WITHOUT an epsilon: a box B (a node, or a leaf's stored volume) is entered iff the guard's five
 *   comparisons hold on the box,
 *       P.u >= B.lo.u && P.u <= B.up.u && P.v >= B.lo.v && P.v <= B.up.v && B.up.w >= P.w
 *   and every box of the tree contains the boxes below it exactly (min / max, widening conversions), so a triangle whose
 *   own box passes the guard has every box above it pass.  Nothing is computed, so nothing is rounded.  Traversal order and
 *   work mapping therefore cannot change the result.
 * Limits.  A point ON the surface is ambiguous (s == 0 is no crossing; which side a point within rounding of the surface is
 *   given follows the sign of the computed s).  Watertightness holds on shared edges and vertices of a mesh whose shared
 *   vertices are bit-identical; it does not hold for T-junctions or cracks.  The parity of `crossings` is
 *   orientation-independent; `winding` needs a consistent orientation but is right for unions of overlapping closed bodies
 *   (2 inside two of them).  Zero-area triangles never count (s == 0).
 * Accepted BVHs — the guard needs boxes that contain their triangles' boxes exactly:
 *   leaf_kind == node_kind == IBVH_BBOX, triangles and points of leaf_float, node_float the same as or wider than
 *   leaf_float; any index and Morton type.  Anything else — sphere leaves (a sphere does not contain its triangle exactly),
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.
 *   Exact PROVIDED every leaf's box contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH
 *   after ibvh_refit.  Levels above bvh->built_level are not read.
 * NaN: a triangle with a NaN vertex in u or v fails the guard or an edge test and never counts; a NaN or +Inf query
 *   coordinate crosses nothing (-Inf along the axis is a ray from infinitely far away: finite where no 0 * Inf arises).  But, as for ibvh_closest_triangles, a NaN leaf box can make merge.jl's `a < b ? a : b` produce
 *   a node box that does NOT contain the NaN-free leaves below it: on a mesh with NaN vertices the other triangles' counts are
 *   only guaranteed in trees of at most two leaves.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped, nothing outside the array is read, and bit 1 of `flag` is set — the flag contract of
 * ibvh_rays_resolve_triangles: optional, 4 bytes the GPU can write, a plain load and store, never cleared by the library
 * (zero it before the call). */
ibvh_status ibvh_point_crossings(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                 const void *points, int64_t num_points, int32_t axis,
                                 void *crossings, void *winding, void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* ray cast: the closest hit, or any hit, of a batch of rays against the mesh           */
/* ----------------------------------------------------------------------------------- */
/* For every ray p + t d: the closest exactly hit triangle of the mesh the BVH was built over (ibvh_volumes_from_triangles
 * with IBVH_BBOX) with its t, u, v — or, for a visibility ray, only whether anything lies in the way.
 * No reference counterpart (the reference's ray traversal stops at the candidate list of the whole infinite line and never
 * prunes on a hit); ONE launch, NO host synchronisation, no atomics, no LDS, no scratch buffer.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   points, directions : num_rays x 3 row-major values of `flt`, processed in the order given (neighbours in memory that
 *                are neighbours in space walk the same nodes: sort a scattered batch along a Morton curve of the origins first)
 *   t_max      : optional DEVICE array of num_rays values of `flt`, the far end of each ray's segment; NULL = unbounded
 *   mode       : IBVH_CAST_CLOSEST or IBVH_CAST_ANY
 * IBVH_CAST_CLOSEST outputs — each optional, at least one non-NULL; what was not asked for is not written; `occluded`
 * must be NULL:
 *   hit_index  : num_rays x I, the winning triangle's user index; 0 = miss
 *   hit_t      : num_rays x flt; +Inf = miss
 *   hit_uv     : num_rays x 2 x flt, the hit's barycentric (u, v) (weights of p2, p3); 0, 0 on a miss
 * IBVH_CAST_ANY output:
 *   occluded   : num_rays x uint8, 1 = the ray hits something within its limit, 0 = it does not; required, and the other
 *                three outputs must be NULL: WHICH triangle stopped the ray depends on the walk order, so it is not reported.
 * All arguments are validated before any launch: a wrong combination of outputs, an unknown mode, NULL required pointers,
 * negative sizes, a tree shape that is not an ImplicitTree's: IBVH_ERR_INVALID_ARG.  num_rays == 0: IBVH_OK, nothing is
 * touched.
 * The result is defined independently of how it is found, in `flt`, every operation rounded once (nothing fused; correctly
 * rounded divide), so that it can be pinned bit for bit.
 * Slab test of a box [lo, up]:  inv_k = 1 / d_k, computed once per ray;  tmin = -Inf;  tmax = +Inf;  per axis k
 *     d_k == 0 :  the axis admits iff lo_k <= p_k && p_k <= up_k, and contributes nothing to tmin / tmax (the query's own
 *                 rule, not the reference's isintersection, whose 0 * Inf is NaN on a box face)
 *     otherwise:  t1 = (lo_k - p_k) * inv_k;  t2 = (up_k - p_k) * inv_k
 *                 tnear = t2 < t1 ? t2 : t1;  tfar = t2 > t1 ? t2 : t1
 *                 tmin = tnear > tmin ? tnear : tmin;  tmax = tfar < tmax ? tfar : tmax
 *   The box is admitted iff every zero-direction axis admits and tmin <= tmax && tmax >= 0.  Every comparison is false on
 *   NaN.   entry(box) = tmin if admitted, +Inf otherwise.
 * Triangle k: exactly the arithmetic and hit condition of ibvh_rays_resolve_triangles above:
 *     det != 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= 0
 * Clamped hit parameter:  t*_k = max(t_k, entry(leaf box of k)) = entry > t_k ? entry : t_k, where the leaf box is the stored
 *   leaf volume, skin included.
 * Ray limit:  L = min(t_max[i], largest finite flt) = t_max[i] > largest ? largest : t_max[i].  A hit must be finite, so L is
 *   never +Inf and an un-admitted box (entry +Inf) is always skipped.  A NaN or negative t_max gives no hit.
 * Hit condition: triangle k is a hit of ray i iff the exact test passes, its leaf box is admitted, and t*_k <= L (the
 *   limit is inclusive).
 * IBVH_CAST_CLOSEST is the LEXICOGRAPHIC MINIMUM of (t*_k, k) over all hits: the smallest t*, and among equal t* the
 *   SMALLER INDEX.  The outputs carry t* and the u, v of the exact test unchanged.  IBVH_CAST_ANY is 1 iff a hit exists.
 * Why pruning is lossless WITHOUT an epsilon: round-to-nearest subtraction and multiplication by a fixed inv_k are
 *   monotone, and box merges are min / max plus exact widening, so the COMPUTED entry of a node is <= that of every box
 *   below it and an admitted box has admitted ancestors:  t*_k >= entry(leaf_k) >= entry(every ancestor).  A node or leaf
 *   is skipped iff entry > limit() — strictly: an equal t* under it may carry a smaller index.  limit() starts at L; the
 *   closest hit lowers it to the best t* found so far, any hit drops it to -Inf on the first hit.  Traversal order and work
 *   mapping therefore cannot change the result.
 * Limits.  On ordinary meshes the clamp changes nothing (it is a guard for the proof; a hit within rounding of a face of its
 *   leaf's box is the exception: 1 of 606,903 hitting rays on a 7.2 M-triangle torus).  It matters for a triangle that lies
 *   flat in a face of its own box, such as an axis-aligned floor: there t* may exceed ibvh_rays_resolve_triangles's t by
 *   rounding.  The test is not watertight along shared edges (a ray through an edge can miss both triangles or hit both),
 *   as with the resolve.  Rays cast from a surface hit it at t ~ 0: there is no t_min.
 * Accepted BVHs — exactly those of ibvh_closest_triangles: leaf_kind == node_kind == IBVH_BBOX, triangles and rays of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Exact PROVIDED every leaf's box
 *   contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH after ibvh_refit.  Levels above
 *   bvh->built_level are not read.
 * NaN: a triangle with a NaN vertex fails the exact test and is never a hit; a NaN origin or direction hits nothing.  But, as
 *   for ibvh_closest_triangles, a NaN leaf box can make merge.jl's `a < b ? a : b` produce a node box that does NOT contain
 *   the NaN-free leaves below it: on a mesh with NaN vertices the other triangles' hits are only guaranteed in trees of at
 *   most two leaves.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped, nothing outside the array is read, and bit 1 of `flag` is set — the flag contract of
 * ibvh_rays_resolve_triangles: optional, 4 bytes the GPU can write, a plain load and store, never cleared by the library
 * (zero it before the call). */
enum { IBVH_CAST_CLOSEST = 0, IBVH_CAST_ANY = 1 };
ibvh_status ibvh_cast_rays(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                           const void *points, const void *directions, int64_t num_rays,
                           const void *t_max, int32_t mode,
                           void *hit_index, void *hit_t, void *hit_uv, void *occluded,
                           void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* sphere-vs-mesh contacts: every triangle within each sphere's radius                  */
/* ----------------------------------------------------------------------------------- */
/* For every sphere (centre c, radius r): ALL triangles of the mesh the BVH was built over (ibvh_volumes_from_triangles with
 * IBVH_BBOX) that lie within r of c — which ones, the squared distance, the closest point on each and the FEATURE of the
 * triangle that point lies on.  The narrow phase of sphere-vs-mesh contact (a particle in a corner touches several
 * triangles; the feature lets the caller count a shared edge or vertex once), and with one radius for all a radius search
 * around points.  No reference counterpart (the reference's traversal of spheres against a mesh ends at pairs of a sphere
 * and a triangle's BOX); a variable-length answer in TWO calls of ONE launch each — count, the caller's scan, write — with
 * NO host synchronisation inside either, no LDS, no scratch buffer, no read-modify-write of memory.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   centers    : num_spheres x 3 row-major values of `flt`, processed in the order given (neighbours in memory that are
 *                neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   radii      : num_spheres values of `flt`, one per sphere
 *   mode       : IBVH_SPHERES_COUNT or IBVH_SPHERES_WRITE
 * IBVH_SPHERES_COUNT, the first pass:
 *   counts     : num_spheres x int64 (whatever the index type), required; counts[s] = the number of contacts of sphere s.
 *                Nothing of `offsets` or the contact_* arrays is read or written: they may be NULL.
 * Between the passes the caller scans: offsets = ANY exclusive prefix sum of counts (its last element plus the last count
 *   is the number of rows the outputs need).  The scan is the caller's — hipCUB, torch.cumsum, Julia's accumulate — the
 *   library's own scan is private to the leaf-vs-tree scratch protocol.
 * IBVH_SPHERES_WRITE, the second pass, with the SAME bvh, triangles, centers and radii:
 *   offsets    : num_spheres x int64, required; contact j of sphere s goes to row offsets[s] + j.  They need NOT be monotone
 *                (a batch walked in Morton order may write its lists in the caller's order); `counts` is not read.
 *   capacity   : the number of rows every non-NULL contact_* array holds.  A row >= capacity or < 0 is never written and
 *                sets bit 2 of `flag` (value 4) instead: a wrong `offsets` array cannot write outside the caller's buffers.
 *                The guard is per ROW, not per sphere: with offsets[s] = -1 contact 0 of sphere s is refused and its
 *                contacts 1, 2, ... are written to rows 0, 1, ...
 *   contact_index  : capacity x I, the triangle's user index
 *   contact_d2     : capacity x flt, its squared distance d2
 *   contact_point  : capacity x 3 x flt, the closest point q on it
 *   contact_region : capacity x uint8, the feature q lies on: the case of the region walk that decided —
 *                    0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 face  (a = p1, b = p2, c = p3)
 *   each optional, at least one non-NULL; what was not asked for is not written.
 * All arguments are validated before any launch: NULL bvh or required pointers, negative sizes or capacity, an unknown mode,
 * no `counts` in the count pass, no `offsets` or no output at all in the write pass, a tree shape that is not an
 * ImplicitTree's: IBVH_ERR_INVALID_ARG.  num_spheres == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found.  r2 = r * r, rounded once in `flt`.  The contacts of sphere s are
 *   ALL triangles k with d2(k, c) <= r2, where d2, q and the deciding case are exactly the evaluation ibvh_closest_triangles
 *   documents above: the same operations in the same order, the same clamp of q into the triangle's box, every operation
 *   rounded once (nothing fused; correctly rounded divide).  The comparison is false on NaN: a triangle whose d2 is NaN is
 *   never a contact.  The outputs carry d2 and q bits unchanged.
 *   A sphere has NO contacts if a coordinate of its centre is NaN, or if !(r >= 0): a negative or NaN radius.  r = 0 keeps
 *   the triangles the centre lies ON (d2 == 0); r = +Inf admits every triangle with a non-NaN d2 (+Inf included).
 * Order: the contacts of one sphere come in LEAF ORDER — ascending position of the triangle's leaf in bvh->leaves — in both
 *   passes, which is what lets them agree.  A triangle that two leaves name appears twice, once per leaf.
 * Why pruning is lossless WITHOUT an epsilon: lb(B) of ibvh_closest_triangles — the point-box bound in d2's operation order
 *   — never exceeds, as COMPUTED, the COMPUTED d2 of a triangle under B.  A node or a leaf is skipped iff lb(B) > r2, so a
 *   skipped box holds no contact.  Why the order holds: both children that pass are equals to the walk, which then takes the
 *   first child first; nothing a visit does changes where the walk goes next.  Work mapping therefore cannot change the
 *   result: one lane per sphere, a register counter in the first pass, a running row in the second.
 * Accepted BVHs — exactly those of ibvh_closest_triangles: leaf_kind == node_kind == IBVH_BBOX, triangles and spheres of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Exact PROVIDED every leaf's box
 *   contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH after ibvh_refit.  Levels above
 *   bvh->built_level are not read.
 * NaN: a triangle with a NaN vertex has a NaN d2 and is never a contact.  But, as for ibvh_closest_triangles, a NaN leaf box
 *   can make merge.jl's `a < b ? a : b` produce a node box that does NOT contain the NaN-free leaves below it: on a mesh with
 *   NaN vertices the other triangles' contacts are only guaranteed in trees of at most two leaves.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped — in BOTH passes alike, so their rows still agree — nothing outside the array is read, and
 * bit 1 of `flag` (value 2) is set.  The flag contract of ibvh_rays_resolve_triangles: optional, 4 bytes the GPU can
 * write, a plain load and store, never cleared by the library (zero it before the call).  The count pass can only raise
 * bit 1.  A write pass in which BOTH faults occur raises at least one of the two bits (two plain stores may race): read
 * bit 1 after the count pass. */
enum { IBVH_SPHERES_COUNT = 0, IBVH_SPHERES_WRITE = 1 };
ibvh_status ibvh_sphere_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                 const void *centers, const void *radii, int64_t num_spheres, int32_t mode,
                                 void *counts, const void *offsets, int64_t capacity,
                                 void *contact_index, void *contact_d2, void *contact_point, void *contact_region,
                                 void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* triangle-vs-mesh contacts: every mesh triangle each query triangle cuts               */
/* ----------------------------------------------------------------------------------- */
/* For every query triangle Q = (a, b, c): ALL triangles K = (p1, p2, p3) of the mesh the BVH was built over
 * (ibvh_volumes_from_triangles with IBVH_BBOX) that Q cuts — which ones, which edge of which triangle pierces the other, and
 * the two ends of the cut.  The narrow phase of mesh-vs-mesh contact (the queries are the other mesh's triangles) and of
 * self-intersection (the queries are the mesh's own).  No reference counterpart (the reference's traversal of two meshes ends
 * at pairs of triangle BOXES); a variable-length answer in TWO calls of ONE launch each — count, the caller's scan, write —
 * with NO host synchronisation inside either, no LDS, no scratch buffer, no read-modify-write of memory.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   queries    : num_queries x 9 values (a b c) of `flt`, processed in the order given (neighbours in memory that are
 *                neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   query_ids  : optional, num_queries values of the BVH's index type I; with it K is a contact of query i only if K's
 *                index > query_ids[i].  With queries = triangles and query_ids = 1..n each unordered pair of one mesh is
 *                found once and no triangle meets itself.
 *   mode       : IBVH_TRIS_COUNT or IBVH_TRIS_WRITE
 *   skip       : 0 or IBVH_TRIS_SKIP_SHARED_VERTEX (bit 0): a K that shares a vertex with Q is no contact.  Equal means ==
 *                on all three coordinates, over the nine vertex pairs.  Neighbours in one mesh always touch; this drops them.
 * IBVH_TRIS_COUNT, the first pass:
 *   counts     : num_queries x int64 (whatever the index type), required; counts[i] = the number of contacts of query i.
 *                Nothing of `offsets` or the contact_* arrays is read or written: they may be NULL.
 * Between the passes the caller scans: offsets = ANY exclusive prefix sum of counts.  The scan is the caller's.
 * IBVH_TRIS_WRITE, the second pass, with the SAME bvh, triangles, queries, query_ids and skip:
 *   offsets    : num_queries x int64, required; contact j of query i goes to row offsets[i] + j.  They need NOT be monotone;
 *                `counts` is not read.
 *   capacity   : the number of rows every non-NULL contact_* array holds.  A row >= capacity or < 0 is never written and
 *                sets bit 2 of `flag` (value 4) instead.  The guard is per ROW, as in ibvh_sphere_contacts.
 *   contact_index  : capacity x I, K's user index
 *   contact_mask   : capacity x uint8, the tests that found the contact (bits 0..5 below)
 *   contact_points : capacity x 2 x 3 x flt, the two ends of the cut (below)
 *   each optional, at least one non-NULL; what was not asked for is not written.
 * All arguments are validated before any launch, in this order.  The entry's own checks: NULL bvh, negative sizes or
 * capacity, an unknown mode, any bit of `skip` other than bit 0, no `counts` in the count pass, no `offsets` or no output at
 * all in the write pass: IBVH_ERR_INVALID_ARG.  Then the type combination (below): IBVH_ERR_UNSUPPORTED.  Then a tree shape
 * that is not an ImplicitTree's or a missing array: IBVH_ERR_INVALID_ARG.  num_queries == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found, in `flt` throughout, every operation rounded once (nothing fused;
 * correctly rounded divide):
 *   Q's box: qlo_k / qup_k = the minimum / maximum of the three vertices' k-th coordinates, folded from a with
 *     `x < m ? x : m` / `x > m ? x : m`.  This is exact.
 *   The box clause: apart(box [lo, up]) = qup_k < lo_k || qlo_k > up_k for some k: six strict comparisons, each false on NaN.
 *   The edge tests: seg(P0, P1, Tri) = the ray-triangle test of ibvh_rays_resolve_triangles above with p = P0,
 *     d = P1 - P0 against Tri is true, AND t <= 1.  Six of them, in this order, each setting one bit of `mask`:
 *       bit 0  a -> b against K      bit 3  p1 -> p2 against Q
 *       bit 1  b -> c against K      bit 4  p2 -> p3 against Q
 *       bit 2  c -> a against K      bit 5  p3 -> p1 against Q
 *   K is a contact of query i iff  !apart(K's stored leaf box)  and  mask != 0  and  (query_ids is NULL or
 *     index > query_ids[i])  and  (bit 0 of skip is clear or no vertex of Q equals a vertex of K).
 *   The contact points: points[2 * row] = P0 + t * d of the LOWEST set bit, points[2 * row + 1] that of the HIGHEST set bit;
 *     each coordinate is one rounded product and one rounded sum.  In general position exactly two bits are set and the two
 *     points are the ends of the intersection segment; with one bit set both rows hold the same point.
 *   A query with a NaN coordinate has NO contacts (it is not walked).
 * Order: the contacts of one query come in LEAF ORDER — ascending position of K's leaf in bvh->leaves — in both passes, which
 *   is what lets them agree.  A triangle that two leaves name appears twice, once per leaf.
 * Why pruning is lossless WITHOUT an epsilon: the box clause is part of the definition, and every box of the tree contains
 *   the boxes below it exactly — through min / max, widening conversions, a skin margin and ibvh_refit.  A node that is apart
 *   from Q therefore has only leaves that are apart from Q, and a node or a leaf is skipped iff it is apart.  A NaN box is
 *   entered.  For leaves that contain their triangles the box clause only removes ghosts of rounding: a pair whose boxes are
 *   apart does not meet.  Why the order holds: as for ibvh_sphere_contacts, the walk is handed 0 / 1 under a constant limit.
 * What follows from the definition:
 *   Coplanar pairs have det == 0 in all six tests wherever the products are exact (axis-aligned planes, small integers):
 *     they are then never contacts, however much they overlap.  In general the COMPUTED det of a coplanar pair is rounding
 *     noise, not 0, and such a pair — a triangle against itself included — is decided by rounding, like a touching one:
 *     query_ids and the shared-vertex rule, not the arithmetic, keep a triangle from meeting itself and its neighbours.
 *   Touching configurations (a vertex on a face, an edge through an edge) depend on rounding.
 *   The decision is symmetric: (Q, K) and (K, Q) run the same six computations, and the masks have bits 0-2 and 3-5
 *     exchanged (given that neither stored box is apart from the other triangle's box).
 *   A test that reads a NaN coordinate is false.  A triangle with a NaN vertex can therefore be found only through the one
 *     edge between its two other vertices, and it hides no other triangle in trees of at most two leaves; above that, as for
 *     ibvh_closest_triangles, a NaN leaf box can make merge.jl's `a < b ? a : b` produce a node box that does not contain
 *     the NaN-free leaves below it.
 * Accepted BVHs — exactly those of ibvh_closest_triangles: leaf_kind == node_kind == IBVH_BBOX, triangles and queries of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Levels above bvh->built_level are
 *   not read.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped — in BOTH passes alike, so their rows still agree — nothing outside the array is read, and
 * bit 1 of `flag` (value 2) is set.  The flag contract of ibvh_sphere_contacts: optional, never cleared by the library, the
 * count pass can only raise bit 1. */
enum { IBVH_TRIS_COUNT = 0, IBVH_TRIS_WRITE = 1 };
enum { IBVH_TRIS_SKIP_SHARED_VERTEX = 1 };
ibvh_status ibvh_triangle_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                   const void *queries, const void *query_ids, int64_t num_queries, int32_t mode, int32_t skip,
                                   void *counts, const void *offsets, int64_t capacity,
                                   void *contact_index, void *contact_mask, void *contact_points, void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* swept spheres: the first time of contact of each moving sphere with the mesh          */
/* ----------------------------------------------------------------------------------- */
/* For every sphere of radius r whose centre moves from p to p + d (position p + t d): the FIRST triangle of the mesh the BVH
 * was built over (ibvh_volumes_from_triangles with IBVH_BBOX) that it touches — which one, the time t, the point of the
 * triangle it touches and the FEATURE that point lies on — or only whether it touches anything within its limit.  The
 * narrow phase of continuous collision detection for particles against a surface: ibvh_sphere_contacts finds a contact only
 * after penetration, and ibvh_cast_rays on the centres misses every grazing contact and is late by up to r on the others.
 * No reference counterpart (the reference has no moving volumes and no exact triangle test); ONE launch, NO host
 * synchronisation, no atomics, no LDS, no scratch buffer.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   centers, displacements : num_spheres x 3 row-major values of `flt`, processed in the order given (neighbours in memory
 *                that are neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   radii      : num_spheres values of `flt`, one per sphere; required
 *   t_max      : optional DEVICE array of num_spheres values of `flt`, the end of each sphere's motion (1 = the whole
 *                displacement); NULL = unbounded
 *   mode       : IBVH_SWEEP_CLOSEST or IBVH_SWEEP_ANY
 * IBVH_SWEEP_CLOSEST outputs — each optional, at least one non-NULL; what was not asked for is not written; `touched`
 * must be NULL:
 *   hit_index   : num_spheres x I, the winning triangle's user index; 0 = miss
 *   hit_t       : num_spheres x flt; +Inf = miss
 *   hit_point   : num_spheres x 3 x flt, the point of the triangle the sphere touches; 0, 0, 0 on a miss
 *   hit_feature : num_spheres x uint8, the feature that point lies on, in ibvh_sphere_contacts' codes —
 *                 0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 face  (a = p1, b = p2, c = p3);
 *                 0 on a miss
 * IBVH_SWEEP_ANY output:
 *   touched    : num_spheres x uint8, 1 = the sphere touches something within its limit, 0 = it does not; required, and the
 *                other four outputs must be NULL: WHICH triangle stopped the walk depends on the walk order.
 * All arguments are validated before any launch, with the statuses of ibvh_cast_rays and in its order: a wrong combination of
 * outputs, an unknown mode, NULL required pointers, negative sizes, a tree shape that is not an ImplicitTree's:
 * IBVH_ERR_INVALID_ARG.  num_spheres == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found, in `flt`, every operation rounded once (nothing fused; correctly
 * rounded divide and square root), every comparison false on NaN, so that it can be pinned bit for bit.  dot(x, y) =
 * (x0 y0 + x1 y1) + x2 y2 and cross are those of ibvh_rays_resolve_triangles.  Per sphere (p, d, r) and triangle
 * k = (a, b, c):
 * 1. Radius and limit.  A sphere with !(r >= 0) — a negative or NaN radius — hits nothing; as in ibvh_sphere_contacts no
 *    flag bit is raised for it.  L = min(t_max[i], largest finite flt) = t_max[i] > largest ? largest : t_max[i], the
 *    select of ibvh_cast_rays.  A NaN or negative limit gives no hit.  r2 = r * r;  dd = dot(d, d).
 * 2. Already touching.  d2, q, region = the evaluation of ibvh_closest_triangles for (k, p), unchanged.  If d2 <= r2:
 *    t_k = 0, the point is q and the feature is region — the bits ibvh_sphere_contacts computes.
 * 3. Otherwise, if d2 > r2 (false on NaN: a triangle with a NaN d2 — a NaN vertex, a NaN centre — is not hit), seven
 *    candidates, each with a t, a point and a validity:
 *    face:   n = cross(b - a, c - a);  len = sqrt(dot(n, n));  s0 = dot(n, p - a);  side = s0 >= 0 ? 1 : -1
 *            o = p - ((side * r) / len) * n, per component
 *            t and validity: the exact test of ibvh_rays_resolve_triangles for the ray (o, d) against k
 *            (det != 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= 0);  point = o + t * d, per component
 *    edges (x, y) = (a, b), (b, c), (c, a):
 *            e = y - x;  m = p - x;  ee = dot(e, e);  me = dot(m, e);  de = dot(d, e);  md = dot(m, d)
 *            A = ee * dd - de * de;  B = ee * md - de * me;  C = ee * (dot(m, m) - r2) - me * me
 *            disc = B * B - A * C;  t = (-B - sqrt(disc)) / A;  s = me + t * de
 *            valid iff A > 0 && disc >= 0 && t >= 0 && s >= 0 && s <= ee;  point = x + (s / ee) * e, per component
 *    vertices x = a, b, c:
 *            m = p - x;  B = dot(m, d);  C = dot(m, m) - r2;  disc = B * B - dd * C;  t = (-B - sqrt(disc)) / dd
 *            valid iff dd > 0 && disc >= 0 && t >= 0;  point = x
 *    t_k = the smallest valid t, with its candidate's point and feature; AMONG EQUAL t THE FIRST CANDIDATE in the order
 *    face, ab, bc, ca, a, b, c (a later candidate replaces an earlier one iff its t is strictly smaller).  No valid candidate,
 *    or none with a t below +Inf: k is not hit.
 *    Why the seven suffice: the set of centres within r of the triangle is the union of a prism (the triangle moved by up
 *    to r along +-n), three cylinders around the edges and three spheres around the vertices; the prism's side walls lie
 *    inside the cylinders, so the first point of the centre's ray in the union — the sphere starts outside it, step 2 — lies
 *    on one of the prism's two faces, on a cylinder between its edge's ends, or on a sphere.  Only the prism face on p's side
 *    can be met first.
 * 4. Clamp and limit.  The grown box of a box [lo, up] is [lo_j - r, up_j + r], j = 0, 1, 2, computed in `flt`.
 *    t*_k = max(t_k, entry(grown leaf box of k)) = entry > t_k ? entry : t_k, where entry is the slab test of ibvh_cast_rays,
 *    unchanged, for the ray (p, d), and the leaf box is the stored leaf volume, skin included.  Triangle k is a hit of sphere
 *    i iff steps 2 or 3 gave a t_k, its grown leaf box is admitted, and t*_k <= L (the limit is inclusive).
 * 5. IBVH_SWEEP_CLOSEST is the LEXICOGRAPHIC MINIMUM of (t*_k, k) over all hits: the smallest t*, and among equal t* the
 *    SMALLER INDEX.  The outputs carry t* and the point and feature of steps 2 / 3 unchanged.  IBVH_SWEEP_ANY is 1 iff a
 *    hit exists.
 * Why pruning is lossless WITHOUT an epsilon: lo_j - r and up_j + r are round-to-nearest, hence monotone in lo_j and up_j,
 *   and every box of the tree contains the boxes below it exactly (min / max, exact widening, a skin margin, ibvh_refit), so
 *   the grown box of a node contains the grown box of everything below it exactly.  The argument of ibvh_cast_rays then
 *   carries over word for word: the COMPUTED entry is monotone in the corners, an admitted box has admitted ancestors, and
 *   t*_k >= entry(grown leaf_k) >= entry(every grown ancestor).  A node or leaf is skipped iff entry > limit() — strictly: an
 *   equal t* under it may carry a smaller index.  limit() starts at L; the closest query lowers it to the best t* found so
 *   far, the any query drops it to -Inf on the first hit.  Traversal order and work mapping therefore cannot change the
 *   result.
 * Limits.  d == 0 makes every candidate of step 3 invalid (det == 0, A == 0, dd == 0): the query reduces to "is anything
 *   touching now".  A triangle whose computed normal is zero (zero area) has no face candidate (len == 0 makes o NaN or the
 *   exact test's det 0); its edges and vertices still answer.  hit_t == 0 names a triangle of the sphere's
 *   ibvh_sphere_contacts list — the one with the smallest index — except where rounding leaves the centre outside that
 *   triangle's grown leaf box (then its t* is the box's entry, or it is no hit).  Which of several features that meet at one
 *   t is reported follows the candidate order; it is not a geometric statement: a sphere that lands exactly on a corner
 *   reports the first edge that ends there.  The quadratics lose digits where the path grazes a feature (disc near 0) and
 *   for |d| much smaller or larger than the mesh: t is what the operations above give, not the nearest float to the true time.
 * Accepted BVHs — exactly those of ibvh_cast_rays: leaf_kind == node_kind == IBVH_BBOX, triangles and spheres of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Exact PROVIDED every leaf's box
 *   contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH after ibvh_refit.  Levels above
 *   bvh->built_level are not read.
 * NaN: a triangle with a NaN vertex has a NaN d2 and is never hit (step 3); a NaN centre or displacement hits nothing.  But,
 *   as for ibvh_closest_triangles, a NaN leaf box can make merge.jl's `a < b ? a : b` produce a node box that does NOT contain
 *   the NaN-free leaves below it: on a mesh with NaN vertices the other triangles' hits are only guaranteed in trees of at
 *   most two leaves.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped, nothing outside the array is read, and bit 1 of `flag` (value 2) is set — the flag contract of
 * ibvh_rays_resolve_triangles: optional, 4 bytes the GPU can write, a plain load and store, never cleared by the library
 * (zero it before the call). */
enum { IBVH_SWEEP_CLOSEST = 0, IBVH_SWEEP_ANY = 1 };
ibvh_status ibvh_sweep_spheres(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                               const void *centers, const void *displacements, const void *radii, int64_t num_spheres,
                               const void *t_max, int32_t mode,
                               void *hit_index, void *hit_t, void *hit_point, void *hit_feature, void *touched,
                               void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* triangle-vs-mesh distance: the closest mesh triangle per query triangle               */
/* ----------------------------------------------------------------------------------- */
/* For every query triangle Q = (a, b, c): the CLOSEST triangle K = (p1, p2, p3) of the mesh the BVH was built over
 * (ibvh_volumes_from_triangles with IBVH_BBOX) — which one, the squared distance, the closest point on each of the two and
 * the pair of features they lie on.  The distance query beside ibvh_triangle_contacts ("do they touch") and
 * ibvh_sweep_spheres ("when"): clearance between parts, the gap that sizes a contact solver's next step, proximity lists
 * and, with a mesh as its own queries and the skip flag, self-clearance.  ibvh_closest_triangles on Q's vertices misses
 * every edge-against-edge pair and every pair that already cuts.  No reference counterpart (the reference's traversal of
 * two meshes ends at pairs of triangle BOXES); ONE launch, NO host synchronisation, no atomics, no LDS, no scratch buffer,
 * no candidate list.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   queries    : num_queries x 9 values (a b c) of `flt`, processed in the order given (neighbours in memory that are
 *                neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   skip       : 0 or IBVH_TRIS_SKIP_SHARED_VERTEX (bit 0): a K that shares a vertex with Q is no answer.  Equal means ==
 *                on all three coordinates, over the nine vertex pairs (the rule of ibvh_triangle_contacts).
 *   max_distance2 : HOST pointer to one value of `flt`, the SQUARED search radius; NULL = +Inf (unbounded)
 * Outputs — every pointer optional, at least one non-NULL; what was not asked for is not written:
 *   closest_index : num_queries x I, the winning triangle's user index; 0 = none
 *   closest_d2    : num_queries x flt; +Inf = none
 *   point_query   : num_queries x 3 x flt, xQ, the closest point on Q; 0, 0, 0 = none
 *   point_mesh    : num_queries x 3 x flt, xK, the closest point on K; 0, 0, 0 = none
 *   closest_kind  : num_queries x uint8, the deciding candidate (below); 0 = none
 * All arguments are validated before any launch, in the order of the other point-walk entries.  The entry's own checks: NULL
 * bvh, negative sizes, any bit of `skip` other than bit 0, no output at all: IBVH_ERR_INVALID_ARG.  Then the type
 * combination (below): IBVH_ERR_UNSUPPORTED.  Then a tree shape that is not an ImplicitTree's or a missing array:
 * IBVH_ERR_INVALID_ARG.  num_queries == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found, in `flt` throughout, every operation rounded once (nothing fused;
 * correctly rounded divide), every comparison false on NaN, so that it can be pinned bit for bit.
 * x . y = (x0*y0 + x1*y1) + x2*y2.  A triangle's exact box: lo_k / up_k = the minimum / maximum of its three vertices' k-th
 * coordinates, folded from the first vertex with `x < m ? x : m` / `x > m ? x : m` (exact).  The result (d2, xQ, xK, kind)
 * of a pair (Q, K) comes from two rules.
 *   The CUT rule, only if K's exact box is not apart from Q's exact box (apart: the six strict comparisons of
 *     ibvh_triangle_contacts, qup_k < lo_k || qlo_k > up_k for some k): the six edge tests of ibvh_triangle_contacts in its
 *     order — a->b, b->c, c->a against K, p1->p2, p2->p3, p3->p1 against Q; seg(P0, P1, Tri) = the ray-triangle test of
 *     ibvh_rays_resolve_triangles with p = P0, d = P1 - P0 is true AND t <= 1.  If any hits: d2 = 0, xQ = xK = P0 + t * d of
 *     the FIRST test that hit (one rounded product and one rounded sum per coordinate), kind = 15.
 *   The CANDIDATE rule, if the cut rule did not decide: fifteen candidates, evaluated in this order; candidate 0 starts the
 *     result and a later one replaces it iff its d2 is strictly smaller (so the FIRST of the smallest wins, and a NaN d2 of
 *     candidate 0 stays).
 *       kind 0, 1, 2      : vertex a, b, c of Q against K: the evaluation of ibvh_closest_triangles for (K, vertex);
 *                           xQ = the vertex, xK = its q, d2 = its d2
 *       kind 3, 4, 5      : vertex p1, p2, p3 of K against Q: the same evaluation for (Q, vertex); xQ = its q, xK = the vertex
 *       kind 6 + 3 i + j  : edge i of Q (0: a->b, 1: b->c, 2: c->a) against edge j of K (0: p1->p2, 1: p2->p3, 2: p3->p1):
 *                           the segment-segment evaluation below for (P1, Q1) = Q's edge and (P2, Q2) = K's edge
 *     The segment-segment evaluation (Ericson, Real-Time Collision Detection 5.1.9; exact tests, no epsilon):
 *       d1 = Q1 - P1;  d2v = Q2 - P2;  r = P1 - P2;  A = d1 . d1;  E = d2v . d2v;  F = d2v . r;  s = t = 0
 *       unit(x) = x < 0 ? 0 : (x > 1 ? 1 : x)
 *       if A == 0:  if E != 0: t = unit(F / E)
 *       else:  C = d1 . r
 *         if E == 0:  s = unit(-C / A)
 *         else:  B = d1 . d2v;  den = A*E - B*B;  if den > 0: s = unit((B*F - C*E) / den)
 *                t = (B*s + F) / E
 *                if t < 0: t = 0, s = unit(-C / A)    else if t > 1: t = 1, s = unit((B - C) / A)
 *       y1 = P1 + s*d1;  y2 = P2 + t*d2v per component; each is then clamped into its own segment's box,
 *       x = y < lo ? lo : (y > up ? up : y) with lo / up = `P < Q ? P : Q` / `P > Q ? P : Q`;  xQ = x1, xK = x2;
 *       e = xQ - xK;  d2 = (e0*e0 + e1*e1) + e2*e2.
 *   Per query the answer is the LEXICOGRAPHIC MINIMUM of (d2, index) over ALL mesh triangles with d2 <= max_distance2, with
 *   bit 0 of skip clear or no vertex of Q equal to a vertex of K, and with an index that names a row of `triangles`: the tie
 *   rule of ibvh_closest_triangles.  A query with a NaN coordinate (or a NaN radius) has no answer; a pair whose d2 is NaN
 *   never wins.  The outputs carry the winner's bits unchanged.
 * Why the fifteen suffice: the closest points of two triangles that do not cut each other can be chosen with one of them on
 *   the boundary of its triangle — a vertex of one against the other triangle, or an edge against an edge.  Two triangles
 *   that cut have an edge of one through the other, which is what the cut rule tests.
 * Why pruning is lossless WITHOUT an epsilon.  (1) Every xQ lies in Q's exact box: a vertex does, and the point-triangle and
 *   segment-segment points are clamped into their triangle's / segment's box, which lies inside it.  (2) Every xK lies in K's
 *   exact box likewise, which lies in K's leaf box and in every box above it (min / max, widening conversions, a skin margin
 *   and ibvh_refit keep containment exact).  (3) The bound of a box B = [lo, up] is
 *       g_k = max(0, lo_k - qup_k, qlo_k - up_k) (both differences rounded);  lb(B) = (g0*g0 + g1*g1) + g2*g2
 *   the same operation order as d2; round-to-nearest subtraction, multiplication and addition are monotone, so the COMPUTED
 *   lb(B) <= the COMPUTED d2 of every pair under B.  (4) A cut pair has exact boxes that are not apart, so both differences
 *   are <= 0 in every box above it and lb = 0 = its d2.  The walk skips a node or a leaf iff lb > best d2 so far — strictly:
 *   lb == best may hide an equal d2 of smaller index.  The best d2 starts at max_distance2 or, if that is smaller, at the
 *   squared distance from Q's vertex a to the closest triangle S the query may answer with (ibvh_closest_triangles' walk and
 *   evaluation): that value is candidate 0 of the pair (Q, S), so the answer's d2 cannot exceed it, and S is still reached.
 *   The definition reads the triangle's OWN box, not the stored one: leaf boxes with a skin give the same result.
 * What follows from the definition: coplanar and touching pairs are decided by rounding — the cut tests of a coplanar pair
 *   have det == 0 wherever the products are exact and rounding noise elsewhere, and a pair that touches in a point or along
 *   an edge gets d2 = 0 from the cut rule or a d2 of a few ulps from a candidate, with kind accordingly.  Without the skip flag
 *   a mesh against itself answers every query with d2 = 0 (itself or a neighbour).  d2 is what the operations above give,
 *   within a few ulps of the true squared distance for well-shaped triangles, not its nearest float.
 * Accepted BVHs — exactly those of ibvh_closest_triangles: leaf_kind == node_kind == IBVH_BBOX, triangles and queries of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Exact PROVIDED every leaf's box
 *   contains its triangle's box.  Levels above bvh->built_level are not read.
 * NaN: as for ibvh_closest_triangles, a NaN leaf box can make merge.jl's `a < b ? a : b` produce a node box that does NOT
 *   contain the NaN-free leaves below it: on a mesh with NaN vertices the other triangles' answers are only guaranteed in
 *   trees of at most two leaves.
 * Guards: the triangle is read through the leaf record's .index, not its position.  A leaf whose index lies outside
 * 1..num_triangles is skipped, nothing outside the array is read, and bit 1 of `flag` (value 2) is set — the flag contract of
 * ibvh_rays_resolve_triangles: optional, 4 bytes the GPU can write, a plain load and store, never cleared by the library
 * (zero it before the call). */
ibvh_status ibvh_triangle_distances(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                    const void *queries, int64_t num_queries, int32_t skip,
                                    const void *max_distance2, void *closest_index, void *closest_d2,
                                    void *point_query, void *point_mesh, void *closest_kind,
                                    void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* capsule-vs-mesh contacts: every triangle within r of each segment                     */
/* ----------------------------------------------------------------------------------- */
/* For every capsule (a segment S = a -> b with a radius r): ALL triangles K = (p1, p2, p3) of the mesh the BVH was built
 * over (ibvh_volumes_from_triangles with IBVH_BBOX) that lie within r of S — which ones, the squared distance, the closest
 * point on the segment and on the triangle, and the rule that decided.  The primitive between the sphere
 * (ibvh_sphere_contacts) and the triangle (ibvh_triangle_contacts): robot links, character controllers, cables, rods and
 * fibres, the swept volume of a particle over a step.  No reference counterpart (the reference's traversals end at pairs of
 * BOXES, and the box of a long diagonal segment is far looser than the segment); a variable-length answer in TWO calls of
 * ONE launch each — count, the caller's scan, write — with NO host synchronisation inside either, no LDS, no scratch
 * buffer, no read-modify-write of memory.
 *   triangles  : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   starts     : num_capsules x 3 row-major values of `flt`, the ends a; processed in the order given (neighbours in memory
 *                that are neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   ends       : num_capsules x 3 row-major values of `flt`, the ends b
 *   radii      : num_capsules values of `flt`, one per capsule
 *   mode       : IBVH_CAPSULES_COUNT or IBVH_CAPSULES_WRITE
 * counts, offsets, capacity and the two passes are those of ibvh_sphere_contacts, word for word: the count pass needs
 *   `counts` (num_capsules x int64) and touches no output; the caller scans; the write pass needs `offsets` (num_capsules x
 *   int64, ANY exclusive prefix sum, not necessarily monotone) and puts contact j of capsule s in row offsets[s] + j; a row
 *   >= capacity or < 0 is never written and sets bit 2 of `flag` (value 4), per ROW.
 *   contact_index         : capacity x I, the triangle's user index
 *   contact_d2            : capacity x flt, the squared distance d2
 *   contact_point_segment : capacity x 3 x flt, xs, the closest point on S
 *   contact_point_mesh    : capacity x 3 x flt, xk, the closest point on K
 *   contact_kind          : capacity x uint8, the rule that decided, 0 - 5 (below)
 *   each optional, at least one non-NULL; what was not asked for is not written.
 * All arguments are validated before any launch, in the order of the other point-walk entries.  The entry's own checks: NULL
 * bvh, negative sizes or capacity, an unknown mode, no `counts` in the count pass, no `offsets` or no output at all in the
 * write pass: IBVH_ERR_INVALID_ARG.  Then the type combination (below): IBVH_ERR_UNSUPPORTED.  Then a tree shape that is not
 * an ImplicitTree's or a missing array: IBVH_ERR_INVALID_ARG.  num_capsules == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found, in `flt` throughout, every operation rounded once (nothing fused;
 * correctly rounded divide), every comparison false on NaN, so that it can be pinned bit for bit.
 * The SEGMENT-TRIANGLE EVALUATION (d2, xs, xk, kind) of a pair (S, K).  S's exact box: slo_k / sup_k = `a_k < b_k ? a_k : b_k`
 * / `a_k > b_k ? a_k : b_k`.  K's exact box: the fold of ibvh_triangle_distances.
 *   The CUT rule, only if K's exact box is not apart from S's exact box (apart: the six strict comparisons of
 *     ibvh_triangle_distances, sup_k < lo_k || slo_k > up_k for some k): the ray-triangle test of
 *     ibvh_rays_resolve_triangles with p = a, d = b - a is true AND t <= 1.  If it hits: d2 = 0, xs = xk = a + t * d (one
 *     rounded product and one rounded sum per coordinate), kind = 5.
 *   The CANDIDATE rule, otherwise: five candidates, evaluated in this order; candidate 0 starts the result and a later one
 *     replaces it iff its d2 is strictly smaller (so the FIRST of the smallest wins, and a NaN d2 of candidate 0 stays).
 *       kind 0, 1     : the end a, b against K: the evaluation of ibvh_closest_triangles for (K, end); xs = the end,
 *                       xk = its q, d2 = its d2
 *       kind 2, 3, 4  : S against K's edge p1->p2, p2->p3, p3->p1: the segment-segment evaluation of
 *                       ibvh_triangle_distances for (P1, Q1) = (a, b) and (P2, Q2) = the edge; xs = x1, which is clamped
 *                       into S's box, xk = x2, which is clamped into the edge's box
 *   The triangle's feature under xk is NOT reported: the segment-segment evaluation does not classify where on the edge
 *   its point lies.
 * r2 = r * r, rounded once.  The contacts of capsule s are ALL triangles k that pass both clauses:
 *   (i)  the SLAB clause: entry <= 1, where entry is entry(box) of ibvh_cast_rays for the ray p = a, d = b - a,
 *        inv_k = 1 / d_k, against leaf k's STORED box grown by r: [lo_k - r, up_k + r], each rounded once (the grown box of
 *        ibvh_sweep_spheres);
 *   (ii) the DISTANCE clause: d2 <= r2 by the evaluation above (false on NaN).
 *   In real arithmetic (ii) implies (i): a point of K within r of a + t * d, 0 <= t <= 1, lies in the box, so a + t * d lies
 *   in the grown box.  (i) is part of the definition so that the walk can prune on it without loss; it decides only pairs
 *   that rounding puts on the grown box's face.  Because (i) reads the STORED box, a skin margin on the leaves can only
 *   admit more such pairs, never fewer.
 *   A capsule has NO contacts if !(r >= 0) — a negative or NaN radius — or if a coordinate of a or b is NaN.  A segment of
 *   length zero is valid: every axis is "still" in the slab test, the cut rule cannot hit (det == 0), and the capsule is a
 *   sphere.  r = 0 keeps the triangles S touches as computed; r = +Inf admits every triangle with a non-NaN d2.
 * Order: the contacts of one capsule come in LEAF ORDER — ascending position of the triangle's leaf in bvh->leaves — in both
 *   passes, which is what lets them agree.  A triangle that two leaves name appears twice, once per leaf.
 * Why pruning is lossless WITHOUT an epsilon.  The walk refuses a node or a leaf iff the squared gap between its box and S's
 *   exact box — lb(B) of ibvh_triangle_distances with S's box in place of Q's — exceeds r2, or the slab entry of its box
 *   grown by r exceeds 1 (both comparisons false on NaN: such a box is entered).  The gap: steps (1) - (4) of
 *   ibvh_triangle_distances hold with S for Q — every xs lies in S's exact box (an end does; x1 is clamped into it), every xk
 *   lies in K's exact box and so in every box above it, the gap is computed in d2's operation order by monotone operations,
 *   and a cut pair's boxes are not apart (lb = 0 = its d2) — so the COMPUTED lb(B) never exceeds a COMPUTED d2 under B, and
 *   a box with lb > r2 holds no triangle that passes (ii).  The slab: the argument of ibvh_sweep_spheres — lo - r and up + r
 *   are monotone, so the grown box of a node contains the grown boxes below it exactly; the slab entry is monotone in the
 *   corners; so a leaf that passes (i) has ancestors that pass.  Why the order holds: as for ibvh_sphere_contacts.
 * Accepted BVHs — exactly those of ibvh_closest_triangles: leaf_kind == node_kind == IBVH_BBOX, triangles and capsules of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Exact PROVIDED every leaf's box
 *   contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH after ibvh_refit.  Levels above
 *   bvh->built_level are not read.  NaN vertices: the caveat of ibvh_sphere_contacts.
 * Guards: those of ibvh_sphere_contacts — a leaf whose index lies outside 1..num_triangles is skipped in BOTH passes alike
 * and sets bit 1 of `flag` (value 2); the same flag contract. */
enum { IBVH_CAPSULES_COUNT = 0, IBVH_CAPSULES_WRITE = 1 };
ibvh_status ibvh_capsule_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                  const void *starts, const void *ends, const void *radii, int64_t num_capsules,
                                  int32_t mode, void *counts, const void *offsets, int64_t capacity,
                                  void *contact_index, void *contact_d2, void *contact_point_segment,
                                  void *contact_point_mesh, void *contact_kind, void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* segment-to-mesh distance: the closest mesh triangle per segment                       */
/* ----------------------------------------------------------------------------------- */
/* For every segment S = a -> b: the CLOSEST triangle of the mesh the BVH was built over — which one, the squared distance,
 * the closest point on S and on the triangle, and the rule that decided.  The distance query beside ibvh_capsule_contacts:
 * the clearance of a link, a rod or a step's path.  No reference counterpart; ONE launch, NO host synchronisation, no
 * read-modify-write of memory, no LDS, no scratch buffer, no candidate list.
 *   triangles, starts, ends : as for ibvh_capsule_contacts (num_segments rows)
 *   max_distance2 : HOST pointer to one value of `flt`, the SQUARED search radius; NULL = +Inf (unbounded)
 * Outputs — every pointer optional, at least one non-NULL; what was not asked for is not written:
 *   closest_index : num_segments x I, the winning triangle's user index; 0 = none
 *   closest_d2    : num_segments x flt; +Inf = none
 *   point_segment : num_segments x 3 x flt, xs; 0, 0, 0 = none
 *   point_mesh    : num_segments x 3 x flt, xk; 0, 0, 0 = none
 *   closest_kind  : num_segments x uint8, the deciding rule, 0 - 5; 0 = none
 * All arguments are validated before any launch, in the order of the other point-walk entries: NULL bvh, negative sizes, no
 * output at all: IBVH_ERR_INVALID_ARG; the type combination: IBVH_ERR_UNSUPPORTED; the tree shape or a missing array:
 * IBVH_ERR_INVALID_ARG.  num_segments == 0: IBVH_OK, nothing is touched.
 * Per segment the answer is the LEXICOGRAPHIC MINIMUM of (d2, index) over ALL mesh triangles with d2 <= max_distance2
 *   (inclusive, false on NaN) and an index that names a row of `triangles`, where (d2, xs, xk, kind) is the segment-triangle
 *   evaluation of ibvh_capsule_contacts: the tie rule of ibvh_closest_triangles.  There is NO slab clause here.  A segment
 *   with a NaN coordinate (or a NaN radius) has no answer; a pair whose d2 is NaN never wins.  The outputs carry the
 *   winner's bits unchanged.
 * Why pruning is lossless WITHOUT an epsilon: the gap argument of ibvh_capsule_contacts.  The walk skips a node or a leaf iff
 *   lb > best d2 so far — strictly: lb == best may hide an equal d2 of smaller index.  The best d2 starts at max_distance2
 *   or, if that is smaller, at the squared distance from the end a to the closest triangle F the query may answer with
 *   (ibvh_closest_triangles' walk and evaluation): that value is candidate 0 of the pair (S, F), bit for bit, so the
 *   answer's d2 cannot exceed it, and F is still reached.  The definition reads the triangle's OWN box, not the stored one:
 *   leaf boxes with a skin give the same result.
 * Accepted BVHs, NaN and guards: those of ibvh_triangle_distances. */
ibvh_status ibvh_segment_distances(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                                   const void *starts, const void *ends, int64_t num_segments,
                                   const void *max_distance2, void *closest_index, void *closest_d2,
                                   void *point_segment, void *point_mesh, void *closest_kind,
                                   void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* box-vs-mesh contacts: every triangle an oriented box overlaps                         */
/* ----------------------------------------------------------------------------------- */
/* For every box (a centre c, half extents h and, optionally, a rotation R): ALL triangles K = (p1, p2, p3) of the mesh the
 * BVH was built over (ibvh_volumes_from_triangles with IBVH_BBOX) that the box overlaps — which ones, and which of their
 * vertices lie in the box.  The shape beside the sphere (ibvh_sphere_contacts), the triangle (ibvh_triangle_contacts) and the
 * capsule (ibvh_capsule_contacts): an oriented box as a robot link, a vehicle hull or a rigid body's proxy; an axis-aligned
 * one as a voxel, a region of interest or a culling cell.  No reference counterpart (the reference's traversals end at
 * pairs of BOXES, and the axis-aligned hull of a rotated box is up to sqrt(3) wider per axis than the box); a
 * variable-length answer in TWO calls of ONE launch each — count, the caller's scan, write — with NO host synchronisation
 * inside either, no LDS, no scratch buffer, no read-modify-write of memory.
 *   triangles    : num_triangles x 9 values (p1 p2 p3) of bvh->types.leaf_float, `flt` below; user index k is row k - 1
 *   centers      : num_boxes x 3 row-major values of `flt`, c; processed in the order given (neighbours in memory that are
 *                  neighbours in space walk the same nodes: sort a scattered batch along a Morton curve first)
 *   half_extents : num_boxes x 3 row-major values of `flt`, h: the box's half width along its own axis 0, 1, 2
 *   rotations    : num_boxes x 9 row-major values of `flt`, R: row k (values 3k, 3k + 1, 3k + 2) is the box's axis u_k in
 *                  world coordinates, ASSUMED orthonormal.  NULL = the identity for every box, in the SAME arithmetic
 *                  (u = 1 0 0, 0 1 0, 0 0 1 takes R's place; one kernel, no second code path): an axis-aligned box.
 *                  A matrix that is not orthonormal is OUTSIDE the contract, and the device does NOT check it: the result
 *                  is then what the arithmetic below gives, the overlap with the image of [-h, h] under no rigid motion.
 *   mode         : IBVH_BOXES_COUNT or IBVH_BOXES_WRITE
 * counts, offsets, capacity and the two passes are those of ibvh_sphere_contacts, word for word: the count pass needs
 *   `counts` (num_boxes x int64) and touches no output; the caller scans; the write pass needs `offsets` (num_boxes x
 *   int64, ANY exclusive prefix sum, not necessarily monotone) and puts contact j of box s in row offsets[s] + j; a row
 *   >= capacity or < 0 is never written and sets bit 2 of `flag` (value 4), per ROW.
 *   contact_index  : capacity x I, the triangle's user index (1-based)
 *   contact_inside : capacity x uint8, the INSIDE mask (below), 0 - 7
 *   each optional, at least one non-NULL; what was not asked for is not written.
 * All arguments are validated before any launch, in the order of the other point-walk entries.  The entry's own checks: NULL
 * bvh, negative sizes or capacity, an unknown mode, no `counts` in the count pass, no `offsets` or no output at all in the
 * write pass: IBVH_ERR_INVALID_ARG.  Then the type combination (below): IBVH_ERR_UNSUPPORTED.  Then a tree shape that is not
 * an ImplicitTree's or a missing array (centers or half_extents with boxes to process; rotations may always be NULL):
 * IBVH_ERR_INVALID_ARG.  num_boxes == 0: IBVH_OK, nothing is touched.
 * The result is defined independently of how it is found, in `flt` throughout, every operation rounded once (nothing fused;
 * nothing divides), every comparison false on NaN, so that it can be pinned bit for bit.  |x| clears the sign bit.
 * The HULL Q of a box, computed once per box: e_k = ((|R_0k| * h_0 + |R_1k| * h_1) + |R_2k| * h_2) — column k of R, i.e.
 *   values k, 3 + k, 6 + k — and Q = [c_k - e_k, c_k + e_k], each rounded once.
 * The LOCAL coordinates of a world point x: w = x - c per component, then v[k] = ((u_k0 * w_0 + u_k1 * w_1) + u_k2 * w_2)
 *   for k = 0, 1, 2.  v_1, v_2, v_3 are those of p1, p2, p3.
 * Triangle K, in a leaf with the stored box L = [lo, up], is a contact of the box iff both clauses hold:
 *   (i)  the BOX clause: L is not apart from Q (apart: the six strict comparisons of ibvh_triangle_contacts,
 *        Qup_k < lo_k || Qlo_k > up_k for some k; every one false on NaN);
 *   (ii) the SAT clause: none of 13 axes separates the triangle from [-h, h] in the box's frame (Akenine-Möller 2001).  An
 *        axis with the triangle's projections P_1, P_2, P_3 and the box's radius rad OVERLAPS iff min <= rad and
 *        max >= -rad, where min / max are folded from P_1: `P_2 < m ? P_2 : m`, then `P_3 < m ? P_3 : m` (and `>`).
 *        Touching counts as overlapping.  With the edges e_0 = v_2 - v_1, e_1 = v_3 - v_2, e_2 = v_1 - v_3 (per component):
 *          the three box axes, k = 0, 1, 2: P_i = v_i[k], rad = h_k;
 *          the triangle's normal n = e_0 x e_1, n_0 = e_0[1] * e_1[2] - e_0[2] * e_1[1], n_1 = e_0[2] * e_1[0] - e_0[0] * e_1[2],
 *            n_2 = e_0[0] * e_1[1] - e_0[1] * e_1[0]: d = ((n_0 * v_1[0] + n_1 * v_1[1]) + n_2 * v_1[2]),
 *            rad = ((|n_0| * h_0 + |n_1| * h_1) + |n_2| * h_2); it overlaps iff d <= rad and d >= -rad;
 *          the nine axes a = axis_k x e_j, for j = 0, 1, 2 and within j for k = 0, 1, 2, by their two non-zero components,
 *          with e = e_j:  k = 0: P_i = e[1] * v_i[2] - e[2] * v_i[1], rad = |e[2]| * h_1 + |e[1]| * h_2;
 *                         k = 1: P_i = e[2] * v_i[0] - e[0] * v_i[2], rad = |e[2]| * h_0 + |e[0]| * h_2;
 *                         k = 2: P_i = e[0] * v_i[1] - e[1] * v_i[0], rad = |e[1]| * h_0 + |e[0]| * h_1.
 *        The clause is the AND of all 13; the order they are tested in does not enter the result.
 *        For a ZERO-AREA triangle the 13 axes are CONSERVATIVE: n and some a are 0, such an axis separates nothing
 *        (0 <= 0), so the test may report a contact where the exact sets are disjoint, and never loses one.
 *   In real arithmetic (ii) implies (i): a common point of box and triangle lies in Q and in L.  (i) is part of the
 *   definition so that the walk can prune on it without loss; it decides only pairs that rounding puts on a face of the
 *   hull.  Because (i) reads the STORED box, a skin margin on the leaves can only admit more such pairs, never fewer.
 * The INSIDE mask of a contact: bit i - 1 (value 1, 2, 4 for p1, p2, p3) is set iff |v_i[k]| <= h_k for all k.  7: the
 *   triangle lies wholly inside the box; 0: the box cuts it without holding a vertex.
 * INVALID boxes: a box has NO contacts if some h_k is not >= 0 — negative or NaN — or if a value of c or R is NaN or
 *   infinite.  A half extent of zero is valid: a plate, a segment or a point.  An INFINITE half extent is not refused: the
 *   result is what the arithmetic gives (0 * Inf = NaN fails its comparison).
 * Order: the contacts of one box come in LEAF ORDER — ascending position of the triangle's leaf in bvh->leaves — in both
 *   passes, which is what lets them agree: contact j of the count pass is row j of the write pass.  A triangle that two
 *   leaves name appears twice, once per leaf.
 * Why pruning is lossless WITHOUT an epsilon.  The walk refuses a node or a leaf iff its box is apart from Q (a NaN in Q
 *   refuses nothing).  Every box of the tree contains the boxes below it exactly (minima and maxima, no rounding), so a box
 *   that is apart from Q lies over leaf boxes that are apart from Q, and those clause (i) refuses by definition.  Why the
 *   order holds: as for ibvh_sphere_contacts — the walk is handed 0 / 1 under a constant limit of 0.
 * Accepted BVHs — exactly those of ibvh_capsule_contacts: leaf_kind == node_kind == IBVH_BBOX, triangles and boxes of
 *   leaf_float, node_float the same as or wider than leaf_float; any index and Morton type.  Anything else — sphere leaves,
 *   sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED, never an answer.  Exact PROVIDED every leaf's box
 *   contains its triangle's box: a skin margin on the leaves is allowed, and so is a BVH after ibvh_refit.  Levels above
 *   bvh->built_level are not read.  NaN vertices: a triangle with one fails a comparison of (ii) and is no contact.
 * Guards: those of ibvh_sphere_contacts — a leaf whose index lies outside 1..num_triangles is skipped in BOTH passes alike
 * and sets bit 1 of `flag` (value 2); the same flag contract. */
enum { IBVH_BOXES_COUNT = 0, IBVH_BOXES_WRITE = 1 };
ibvh_status ibvh_box_contacts(const ibvh_bvh *bvh, const void *triangles, int64_t num_triangles,
                              const void *centers, const void *half_extents, const void *rotations,
                              int64_t num_boxes, int32_t mode, void *counts, const void *offsets,
                              int64_t capacity, void *contact_index, void *contact_inside,
                              void *flag, void *stream);

/* ----------------------------------------------------------------------------------- */
/* rays and swept spheres against a sphere cloud: the first leaf hit                     */
/* ----------------------------------------------------------------------------------- */
/* For every query — a sphere of radius r >= 0 whose centre moves from p to p + d (position p + t d; r = 0 is a ray) — the
 * FIRST leaf sphere of the cloud the BVH was built over that it touches and the time t, or only whether it touches anything
 * within its limit.  t is in units of d: t = 1 is the end of the displacement.  Lidar and camera rays into a granular bed,
 * line of sight and shadowing between particles, a projectile or fast particle that must not tunnel through a layer, "is the
 * path from a to b free".  ibvh_traverse_rays_* list every (leaf, ray) whose bounding sphere the whole LINE meets, a list of
 * unbounded length the caller would have to reduce.  No reference counterpart; ONE launch, NO host synchronisation, no
 * atomics, no LDS, no scratch buffer, no candidate list.
 *   points, displacements : num x 3 row-major values of bvh->types.leaf_float, `flt` below, processed in the order given
 *                (neighbours in memory that are neighbours in space walk the same nodes: sort a scattered batch along a
 *                Morton curve first)
 *   radii      : optional DEVICE array of num values of `flt`; NULL = 0 for all (rays)
 *   t_max      : optional DEVICE array of num values of `flt`, the end of each query's motion; NULL = unbounded
 *   skip       : optional DEVICE array of num x I, per query the user index of ONE leaf to ignore — a particle of the cloud
 *                swept against the cloud skips itself, and so does a ray that starts on a particle's surface —; 0 names no
 *                leaf; NULL = none
 *   mode       : IBVH_SPHERECAST_CLOSEST or IBVH_SPHERECAST_ANY
 * The output rules are those of ibvh_sweep_spheres.  IBVH_SPHERECAST_CLOSEST — each optional, at least one non-NULL; what
 * was not asked for is not written; `touched` must be NULL:
 *   hit_index  : num x I, the winning leaf's user index; 0 = miss
 *   hit_t      : num x flt; +Inf = miss
 * IBVH_SPHERECAST_ANY:
 *   touched    : num x uint8, 1 = the query touches something within its limit, 0 = it does not; required, and the other
 *                two outputs must be NULL: WHICH leaf stopped the walk depends on the walk order.
 * There is no flag argument: no index is used to read anything, so there is none to guard.
 * All arguments are validated before any launch, in the order of ibvh_sweep_spheres: the entry's own checks (a NULL bvh, a
 * negative num, an unknown mode, a wrong combination of outputs: IBVH_ERR_INVALID_ARG), then the types
 * (IBVH_ERR_UNSUPPORTED), then the tree's shape and the required pointers (IBVH_ERR_INVALID_ARG).  num == 0: IBVH_OK, nothing
 * is touched.
 * The result is defined independently of how it is found, in `flt` = T, every operation rounded once (nothing fused;
 * correctly rounded divide and square root), every comparison false on NaN, so that it can be pinned bit for bit.
 * dot(x, y) = (x0 y0 + x1 y1) + x2 y2;  max(a, b) is the select a > b ? a : b.  For query (p, d, r, L, s) and the leaf with
 * centre c, radius R and user index k:
 * 1. Sums.  S = R + r;  m = p - c;  mm = dot(m, m).
 * 2. Touching at the start iff mm <= S * S — the bits of the library's own iscontact(BSphere, BSphere) (iscontact.jl), so a
 *    pair traversal and this query agree on who overlaps.  Then t_k = 0.
 * 3. Otherwise, provided mm > S * S:  B = dot(m, d);  dd = dot(d, d);  Cq = mm - S * S;  disc = B * B - dd * Cq;
 *    t_k = (-B - sqrt(disc)) / dd, valid iff dd > 0 && disc >= 0 && t_k >= 0 — exactly the operations of
 *    ibvh_sweep_spheres' vertex candidate.  No valid t_k: k is not hit.  A NaN in the leaf makes every comparison false: no
 *    hit.  A query with a NaN in p or d, or with !(r >= 0), touches nothing.
 * 4. Own box.  own_k = entry(lo - r, up + r) for the ray (p, d), where (lo, up) = (c - R, c + R) in T — the leaf's volume as
 *    a box (convert, merge.jl:47-51), which the walk bounds the leaf with —, the grown box [lo_j - r, up_j + r] is computed
 *    in T, and entry is the slab test of ibvh_cast_rays, unchanged (+Inf: the ray does not meet the box).
 * 5. Parent box.  parent_k = the same entry of the STORED box of the node directly above leaf k — its values narrowed to T,
 *    which is exact, and grown by r the same way —, where that level exists and is built (tree.levels >= 2 and
 *    built_level <= tree.levels - 1); otherwise -Inf.
 * 6. Clamped time.  t*_k = max(max(t_k, own_k), parent_k).
 * 7. Hit.  Leaf k is a hit iff k != s and t*_k <= L, inclusive, where L = min(t_max, largest finite flt) = t_max > largest ?
 *    largest : t_max.  A NaN or negative L admits nothing.
 * 8. IBVH_SPHERECAST_CLOSEST is the LEXICOGRAPHIC MINIMUM of (t*_k, k) over ALL hits: the smallest t*, and among equal t*
 *    the SMALLER INDEX.  IBVH_SPHERECAST_ANY is 1 iff a hit exists.  A miss is index 0, t +Inf.
 * The hazard, and why step 5 is there.  The mesh queries argue "every box of the tree contains the boxes below it exactly".
 *   With sphere leaves that is FALSE at the lowest node level: merging two spheres into a box (merge.jl:58-81) returns the box
 *   of b alone when length + a.r <= b.r holds in ROUNDED arithmetic, and the box of a need not lie inside it.  Of 4e6 random
 *   Float32 pairs that are internally tangent along a coordinate axis the shortcut fired for about half, and for 3.3 % of
 *   those the inner sphere's box pokes out of the outer's by an ulp.  A query that starts at the poking tip and does not move
 *   along that axis is admitted by the leaf's own box and refused by the parent's stored box: a walk never reaches the leaf
 *   although steps 1 to 4 alone give a touch at t = 0.  With step 5 such a query is a miss BY DEFINITION, which a brute force
 *   can state without walking the tree: it needs the leaf order and the stored boxes of one level.
 * Why pruning is then lossless WITHOUT an epsilon: above the lowest node level every merge is an exact minimum / maximum
 *   with an exact widening (and ibvh_refit repeats the build's merges), lo_j - r and up_j + r are round-to-nearest, hence
 *   monotone, and the COMPUTED slab entry is monotone in the corners (the argument of ibvh_sweep_spheres), so
 *   t*_k >= parent_k >= entry(every grown ancestor), and the walk's bound of the leaf itself is own_k <= t*_k.  A node or leaf
 *   is skipped iff entry > limit() — strictly: an equal t* under it may carry a smaller index — so a skipped box holds
 *   nothing that can still win or tie.  limit() starts at L; the closest query lowers it to the best t* so far, the any query
 *   drops it to -Inf on the first hit.  Traversal order and work mapping therefore cannot change the result.
 * Limits.  d == 0 makes step 3 invalid (dd == 0): the query reduces to "what does this sphere overlap now", index order
 *   deciding.  The quadratic loses digits where the path grazes a leaf (disc near 0) and for |d| much smaller or larger than
 *   the cloud: t is what the operations above give, not the nearest float to the true time.  hit_t == 0 names a leaf that
 *   iscontact reports, except where rounding leaves the start outside a grown box of steps 4 / 5 (then t* is that box's
 *   entry, or the leaf is no hit).  A leaf with a NaN can make a box above it fail to contain its NaN-free neighbours, as
 *   for ibvh_nearest_leaves.
 * Accepted BVHs: leaf_kind == IBVH_BSPHERE, node_kind == IBVH_BBOX, node_float the same as or wider than leaf_float; any
 *   index and Morton type.  Anything else — box leaves, sphere nodes, F64 leaves under F32 nodes — is IBVH_ERR_UNSUPPORTED,
 *   never an answer.  A BVH after ibvh_refit is fine (no skin is needed: the definition reads the stored boxes).  Levels above
 *   bvh->built_level are not read. */
enum { IBVH_SPHERECAST_CLOSEST = 0, IBVH_SPHERECAST_ANY = 1 };
ibvh_status ibvh_cast_spheres(const ibvh_bvh *bvh, const void *points, const void *displacements,
                              const void *radii, int64_t num, const void *t_max, const void *skip, int32_t mode,
                              void *hit_index, void *hit_t, void *touched, void *stream);

/* ----------------------------------------------------------------------------------- */
/* breadth-first traversal (BFSTraversal): level-synchronous pair queues                 */
/* ----------------------------------------------------------------------------------- */
typedef struct ibvh_bfs_result {
    int64_t num_contacts;
    int64_t num_checks;        /* BVHTraversal.num_checks (bfs/traverse_single.jl:25,48)          */
    int64_t contacts_in;       /* 1: contacts are in bvtt1, 2: in bvtt2; with IBVH_ERR_CAPACITY: the queue that
                                  holds the pairs still to be expanded (keep its first resume_num entries)     */
    int64_t required_capacity; /* pairs each queue must hold; set when IBVH_ERR_CAPACITY          */
    /* IN/OUT — resuming after IBVH_ERR_CAPACITY instead of starting over (the reference grows its queue between two
     * levels, bfs/traverse_single.jl:38-53): zero both for a fresh traversal.  With IBVH_ERR_CAPACITY the library
     * reports the step whose destination queue was too small; call again with the SAME result struct, both queues
     * grown to required_capacity (contents of the `contacts_in` queue preserved, e.g. Julia's resize!) and the same
     * `counters` buffer: the traversal continues from that step.                                                   */
    int64_t resume_step;
    int64_t resume_num;
} ibvh_bfs_result;

/* Pairs the initial queue needs: initial_bvtt (bfs/traverse_single.jl:64-99). */
ibvh_status ibvh_bfs_initial_capacity(const ibvh_bvh *bvh, int64_t start_level, int64_t *pairs_out);
ibvh_status ibvh_bfs_pair_initial_capacity(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2,
                                           int64_t start_level1, int64_t start_level2,
                                           int64_t *pairs_out);
ibvh_status ibvh_bfs_rays_initial_capacity(const ibvh_bvh *bvh, int64_t num_rays,
                                           int64_t start_level, int64_t *pairs_out);
/* Bytes of the `counters` device scratch for a traversal that walks `total_levels` levels
 * (levels of the BVH; levels1 + levels2 for a pair). */
ibvh_status ibvh_bfs_counters_bytes(int64_t total_levels, size_t *bytes_out);

/* traverse(bvh, BFSTraversal()) — bfs/traverse_single.jl:1-61.  bvtt1/bvtt2: two queues of
 * `capacity` IndexPair{I} each (cache1/cache2).  counters: DEVICE scratch of
 * ibvh_bfs_counters_bytes() bytes (overflow flag + a queue count and a check count per level).  A queue holds pairs
 * that have already passed their check: a step enumerates their children and checks them at once (the same checks as the
 * reference's, one launch earlier; num_checks is unchanged).  All levels are enqueued back to back — a
 * level takes its queue length from the device word the previous level accumulated — and the stream is synchronised
 * ONCE, at the end (the reference reads one count per level, bfs/traverse_single_gpu.jl:24).  On IBVH_ERR_CAPACITY
 * grow both queues to result->required_capacity and call again with the same `result` (see ibvh_bfs_result: the
 * traversal resumes at the level that overflowed; the reference's resize!, bfs/traverse_single.jl:40). */
ibvh_status ibvh_traverse_bfs(const ibvh_bvh *bvh, int64_t start_level, int32_t narrow, void *bvtt1,
                              void *bvtt2, int64_t capacity, void *counters,
                              ibvh_bfs_result *result, void *stream);

/* traverse(bvh1, bvh2, BFSTraversal()) — bfs/traverse_pair.jl:1-151 (six-phase descent). */
ibvh_status ibvh_traverse_pair_bfs(const ibvh_bvh *bvh1, const ibvh_bvh *bvh2, int64_t start_level1,
                                   int64_t start_level2, int32_t narrow, void *bvtt1, void *bvtt2,
                                   int64_t capacity, void *counters, ibvh_bfs_result *result,
                                   void *stream);

/* traverse_rays(bvh, points, directions, BFSTraversal()) — raytrace/breadth_first/
 * breadth_first.jl:1-66. */
ibvh_status ibvh_traverse_rays_bfs(const ibvh_bvh *bvh, const void *points, const void *directions,
                                   int64_t num_rays, int64_t start_level, int32_t narrow, void *bvtt1, void *bvtt2,
                                   int64_t capacity, void *counters, ibvh_bfs_result *result,
                                   void *stream);

/* ----------------------------------------------------------------------------------- */
/* multi-GPU build: device pieces (collectives are issued by the host side over RCCL)    */
/* ----------------------------------------------------------------------------------- */
/* Epsilon expansion of bounding_volumes_extrema (morton/utils.jl:63-69) applied in place to 6
 * already reduced values (mins then maxs) of float type `flt` in DEVICE memory: used after the
 * all-reduce of the per-GPU extrema (ibvh_extrema with expand = 0). */
ibvh_status ibvh_expand_extrema(int32_t flt, void *extrema, void *stream);

/* The all-reduce(MAX) vector of the distributed build, assembled / taken apart on device (one launch each, no
 * host round trip): vec_out (DEVICE, 6 + nranks float64) = [-mins(3), maxs(3), one-hot leaf counts]; `extrema`:
 * this GPU's 6 UNEXPANDED centre extrema of float type `flt` (ibvh_extrema with expand = 0), ignored when
 * has_data == 0 (neutral elements of morton/utils.jl:29-40 are written).  _unpack converts the reduced vector back
 * to `flt` and applies the epsilon expansion (morton/utils.jl:63-69). */
ibvh_status ibvh_dist_pack_extrema(int32_t flt, const void *extrema, int32_t has_data, int32_t rank,
                                   int32_t nranks, int64_t n_local, void *vec_out, void *stream);
ibvh_status ibvh_dist_unpack_extrema(int32_t flt, const void *vec, void *extrema_out, void *stream);

/* Stable partition of the local leaves by destination rank (keys in [splitters[r-1], splitters[r]) go to rank r;
 * `splitters`: nranks - 1 ascending keys in HOST memory): perm_out[j] (DEVICE, n x uint32) = source position of the
 * j-th leaf in (destination, source position) order; counts_out (DEVICE, nranks x uint64, optional): leaves per
 * destination rank — for a caller that does not already know its row of the send matrix.  nranks <= 256 (more:
 * IBVH_ERR_UNSUPPORTED).  Keys equal to a splitter go to the rank on its right.  Every argument is checked before the
 * first HIP call: a refused call has touched nothing; n == 0 zeroes counts_out and touches nothing else. */
ibvh_status ibvh_dist_partition_scratch_bytes(int64_t n, size_t *bytes_out);
ibvh_status ibvh_dist_partition(int32_t key_bytes, const void *keys, int64_t n, const uint64_t *splitters,
                                int32_t nranks, void *perm_out, void *counts_out, void *scratch,
                                size_t scratch_bytes, void *stream);

/* Digit histograms for the splitter search of the distributed radix sort.  out (DEVICE,
 * max(nprefix,1) x 2^bits uint32, zeroed here): out[j][d] = number of keys whose
 * (key >> prefix_shift) == prefixes[j] and whose digit (key >> shift) & (2^bits - 1) == d;
 * nprefix == 0 counts all keys.  `prefixes` is a HOST array; a prefix listed twice gets the count in both rows.
 * 1 <= bits <= 12, 0 <= shift <= 63; prefix_shift >= 0 when nprefix > 0, and prefix_shift >= 64 means "every key has
 * prefix 0".  One call stages its rows in LDS (160 KB): nprefix <= 15 for bits <= 11, nprefix <= 10 for bits == 12
 * (anything else: IBVH_ERR_INVALID_ARG) — ibvh_dist_plan batches its undecided prefixes by the same limit.  The
 * largest configuration, 10 rows x 12 bits = exactly 160 KB of dynamic LDS, is the one verified on an MI355X: the
 * device accepts the launch and the counts are right (tests/test_gpu_dist_pieces.py launches it in every run). */
ibvh_status ibvh_key_histogram(int32_t key_bytes, const void *keys, int64_t n, int32_t shift,
                               int32_t bits, int32_t prefix_shift, const uint64_t *prefixes,
                               int32_t nprefix, void *out, void *stream);

/* Pack BoundingVolume records for the exchange: out[i] = { volumes[p], index_base + p + 1,
 * keys[p] } with p = perm[i] (uint32, repeats allowed) or i when perm == NULL.  index_base < 0: IBVH_ERR_INVALID_ARG;
 * index_base + n > INT32_MAX under IBVH_I32: IBVH_ERR_OVERFLOW (both before any HIP call). */
ibvh_status ibvh_pack_records(const ibvh_types *types, const void *volumes, const void *keys,
                              const void *perm, int64_t index_base, int64_t n, void *records_out,
                              void *stream);

/* ----------------------------------------------------------------------------------- */
/* multi-GPU build: the driver (round 4).  No reference counterpart: ImplicitBVH.jl is    */
/* single-device; BASELINE.json's north star shards the BUILD over the GPUs of one node   */
/* ("RCCL allreduce over xGMI for the global AABB and a distributed radix-sort exchange") */
/* and keeps the host in Julia behind "a thin C-ABI (ccall) shim" — this is that shim.    */
/* ----------------------------------------------------------------------------------- */
#define IBVH_DIST_MAX_RANKS 256
enum { IBVH_COMM_F64 = 0, IBVH_COMM_I64 = 1, IBVH_COMM_I32 = 2 };  /* element type of an all-reduce */
enum { IBVH_COMM_MAX = 0, IBVH_COMM_SUM = 1, IBVH_COMM_MIN = 2 };  /* its operation                 */

/* Collectives the driver needs, as a vtable: every rank calls the same sequence.  Buffers are DEVICE pointers; a call is
 * ordered behind earlier work on `stream` and later work on `stream` sees its result (RCCL semantics).  Return 0 on
 * success.  all_to_all_v: `send` is partitioned contiguously by destination (send_bytes[p] bytes for rank p), `recv`
 * contiguously by source (recv_bytes[p]); both count arrays are HOST arrays of `size` entries. */
typedef struct ibvh_comm {
    void *ctx;
    int32_t rank, size;
    int32_t (*all_reduce)(void *ctx, void *buf, int64_t count, int32_t dtype, int32_t op, void *stream); /* in place */
    int32_t (*all_gather)(void *ctx, const void *send, void *recv, int64_t bytes_per_rank, void *stream);
    int32_t (*all_to_all_v)(void *ctx, const void *send, const int64_t *send_bytes, void *recv, const int64_t *recv_bytes,
                            void *stream);
} ibvh_comm;

/* The vtable over RCCL for an ncclComm_t the caller created (ncclCommInitRank), collectives issued on the stream each
 * call is handed.  librccl.so is resolved with dlopen on first use (libibvh.so does not link it): IBVH_ERR_UNSUPPORTED
 * when it cannot be found.  all_to_all_v = grouped ncclSend / ncclRecv: xGMI is point-to-point. */
ibvh_status ibvh_comm_from_rccl(void *nccl_comm, int32_t rank, int32_t size, ibvh_comm *out);

/* Splitter search of the distributed radix sort — HOST arithmetic only (no GPU), identical on every rank: keys
 * k_1 <= ... <= k_{P-1}, rank r receives the keys in [k_r, k_{r+1}).  Protocol: init; then, until all_done: make the GLOBAL
 * histogram of the digit (key >> next_shift) & (2^next_bits - 1) — one row over all keys at level 0, later one row per
 * prefix rows[j] (keys with key >> (next_shift + next_bits) == rows[j]), num_rows rows — and hand it to _step.  A splitter
 * stops refining once the bucket it landed in holds at most tolerance * n_global / size keys (0: full key resolution). */
typedef struct ibvh_splitter_search {
    int32_t size, key_bits, decided /* key bits decided so far */, all_done;
    int32_t next_bits, next_shift, num_rows, reserved_;
    int64_t n_global;
    double tolerance;
    uint64_t rows[IBVH_DIST_MAX_RANKS];      /* prefixes the next histogram needs, ascending */
    uint64_t prefix[IBVH_DIST_MAX_RANKS];    /* per splitter: the bits decided so far        */
    uint64_t splitters[IBVH_DIST_MAX_RANKS]; /* per splitter: the final key, once done       */
    int64_t below[IBVH_DIST_MAX_RANKS];      /* per splitter: global number of keys strictly below its decided prefix range */
    int32_t row_of[IBVH_DIST_MAX_RANKS];     /* per splitter: its row of the next histogram  */
    uint8_t done[IBVH_DIST_MAX_RANKS];
} ibvh_splitter_search;
ibvh_status ibvh_splitter_search_init(ibvh_splitter_search *s, int32_t size, int32_t key_bits, int64_t n_global, double tolerance);
ibvh_status ibvh_splitter_search_step(ibvh_splitter_search *s, const int64_t *hist);

/* What ibvh_dist_plan found out (HOST memory). */
typedef struct ibvh_dist_plan_t {
    int32_t size, levels_used /* key bits the splitter search decided */;
    int64_t n_local, n_global;
    int64_t base;             /* global 0-based number of this rank's first local leaf (records carry base + p + 1)   */
    int64_t n_slice;          /* records this rank receives = leaves of its slice of the globally sorted sequence    */
    int64_t record_bytes;
    double extrema[6];        /* global centre extrema, epsilon-expanded: mins / maxs for the local ibvh_build        */
    uint64_t splitters[IBVH_DIST_MAX_RANKS];
    int64_t send_counts[IBVH_DIST_MAX_RANKS], recv_counts[IBVH_DIST_MAX_RANKS]; /* records per peer */
} ibvh_dist_plan_t;

/* Scratch for ibvh_dist_plan + ibvh_dist_exchange (the same buffer must be passed to both, untouched in between: the plan
 * leaves the keys and the partition's permutation there). */
ibvh_status ibvh_dist_scratch_bytes(const ibvh_types *types, int64_t n_local, int32_t size, size_t *bytes_out);

/* Everything up to the exchange (see csrc/ibvh_distdrv.hip): global AABB (one all-reduce(MAX) that also carries every
 * rank's leaf count), Morton keys, splitters (one all-gather; further all-reduce(SUM) levels only while a splitter's bucket
 * is heavier than `tolerance` of a shard — 0.005 is the Python mirror's default), stable partition by destination.  BLOCKS
 * on `stream` once (twice when the send matrix does not follow from the first histogram): the record counts must reach the
 * host before RCCL can be told the transfer sizes — the reference's own "count, then size, then write" shape.
 * IBVH_ERR_DOMAIN (on EVERY rank, so that none is left waiting in a collective) when there are fewer leaves than ranks or a
 * rank would receive none; IBVH_ERR_OVERFLOW (on every rank as well) when the global leaf count does not fit IBVH_I32. */
ibvh_status ibvh_dist_plan(const ibvh_types *types, const ibvh_comm *comm, const void *volumes, int64_t n_local, double tolerance,
                           void *scratch, size_t scratch_bytes, ibvh_dist_plan_t *plan_out, void *stream);

/* Pack the local leaves into BoundingVolume records with GLOBAL 1-based indices and exchange them: ONE all-to-all.
 * records_out: DEVICE, plan->n_slice records, grouped by source rank in source order — so the stable local sort of
 * ibvh_build (already_wrapped = 1, compute_extrema = 0, mins / maxs = plan->extrema) keeps global input order among equal
 * keys, and rank r ends with the r-th slice of the single-device sorted sequence, bit for bit.  Asynchronous on `stream`. */
ibvh_status ibvh_dist_exchange(const ibvh_types *types, const ibvh_comm *comm, const void *volumes, const ibvh_dist_plan_t *plan,
                               void *scratch, size_t scratch_bytes, void *records_out, void *stream);

/* Cross-shard contact completion: the contacts between leaves of DIFFERENT slices, which the
 * per-slice self-traversals cannot see.  Descriptions and leaf counts of all slices are all-gathered; for every pair of slices
 * r < s whose boxes touch, rank s sends rank r the leaves whose own box touches one of r's boxes (a slice is described by
 * <= 16 node boxes of its tree, refined from the root by always splitting the largest: a Morton slice is not convex) — a thin
 * shell of its slice, not its tree — in ONE all_to_all_v over the same vtable; rank r builds an ordinary BVH over each set it received
 * (ibvh_build, in place) and runs the ordinary pair traversal (traverse(bvh_r, bvh_s), lvt/traverse_pair.jl) against it.
 * Per-slice self contacts + these pairs = the contact set of the whole cloud, every pair once.  Count -> size -> write:
 *   _plan     collective (one all-gather, one 8-bytes-a-peer all_to_all_v); ONE host synchronisation (every slice's boxes and how
 *             many leaves every peer gets, together); a rank with unacceptable arguments still takes part — its status travels in
 *             its record — and EVERY rank returns an error: its own, or IBVH_ERR_PEER; fills the plan:
 *             export_bytes / import_bytes (the two buffers the caller hands to _exchange) and scratch_bytes (the scratch of
 *             _count / _write: traversal scratch per imported set, cache_slots as in ibvh_lvt_scratch_bytes, + the build's).
 *             `scratch` here and in _exchange: IBVH_DIST_CROSS_SCRATCH(size) bytes of device memory.
 *   _exchange collective (every rank calls it, also one that neither sends nor receives); asynchronous on `stream`.
 *   _count    per imported set: ibvh_build + the pair traversal's counting pass; totals_out[k] (may be NULL), *total_out: pairs.
 *   _write    contacts_out: *total_out IndexPair{I}, the pairs against imported set 0 first: (index in THIS slice, index in
 *             the other slice), both GLOBAL 1-based leaf numbers (the records carry them).  `totals`: what _count returned.
 * The BVH must be fully built (built_level = 1).  The pairs are a SET: the order in which a sender's boundary leaves arrive is
 * not deterministic, so leaves of equal Morton codes — and their cross contacts — may change places from run to run (the per-slice
 * lists keep the reference's order).  Errors inside a collective sequence that are not argument errors (a failed HIP call, a
 * failed collective; a rank without a communicator or scratch): the caller must abort the communicator — a rank that returns
 * early leaves its peers waiting. */
#define IBVH_DIST_CROSS_BOXES 16
typedef struct ibvh_dist_cross_plan_t {
    int32_t size, rank, n_recv /* leaf sets this rank imports */, cache_slots;
    int64_t import_bytes, scratch_bytes, export_bytes, build_offset /* where the build's scratch starts in the scratch */;
    int32_t recv_rank[IBVH_DIST_MAX_RANKS];      /* [n_recv] ascending: the ranks leaves are imported from                   */
    int64_t recv_leaves[IBVH_DIST_MAX_RANKS];    /* [n_recv] how many                                                        */
    int64_t recv_offset[IBVH_DIST_MAX_RANKS];    /* [n_recv] byte offset of that set's leaves in the import buffer (the sets are contiguous; the room for their trees' nodes and skips follows the last set) */
    int64_t scratch_offset[IBVH_DIST_MAX_RANKS]; /* [n_recv] byte offset of its counts + traversal scratch                   */
    int64_t slice_leaves[IBVH_DIST_MAX_RANKS];   /* [size] leaves of every rank's slice                                      */
    int32_t touches[IBVH_DIST_MAX_RANKS];        /* [size] 1: one of this rank's boxes (below) touches one of rank r's (r != rank) */
    int64_t send_leaves[IBVH_DIST_MAX_RANKS];    /* [size] own leaves rank r gets (r < rank: those whose box touches one of r's boxes) */
    int64_t send_offset[IBVH_DIST_MAX_RANKS];    /* [size] where they are compacted in the export buffer (contiguous, by rank) */
    int32_t n_boxes[IBVH_DIST_MAX_RANKS];        /* [size] boxes that describe rank r's slice (1 .. IBVH_DIST_CROSS_BOXES)   */
    double boxes[IBVH_DIST_MAX_RANKS][IBVH_DIST_CROSS_BOXES][6]; /* [size] ... node boxes of its tree, refined greedily (lo, up); a sphere's box is x -+ r in double */
} ibvh_dist_cross_plan_t;
/* device bytes _plan and _exchange need as `scratch` for `size` ranks */
#define IBVH_DIST_CROSS_SCRATCH(size) ((size_t)(IBVH_DIST_CROSS_BOXES * 48 + 16) * ((size_t)(size) + 1) + (size_t)16 * (size_t)(size) + 512)
ibvh_status ibvh_dist_cross_plan(const ibvh_comm *comm, const ibvh_bvh *bvh, int32_t cache_slots, void *scratch, size_t scratch_bytes,
                                 ibvh_dist_cross_plan_t *plan_out, void *stream);
ibvh_status ibvh_dist_cross_exchange(const ibvh_comm *comm, const ibvh_bvh *bvh, const ibvh_dist_cross_plan_t *plan, void *export_buf,
                                     void *import_buf, void *scratch, size_t scratch_bytes, void *stream);
ibvh_status ibvh_dist_cross_count(const ibvh_bvh *bvh, const ibvh_dist_cross_plan_t *plan, void *import_buf, void *scratch,
                                  size_t scratch_bytes, int64_t *totals_out, int64_t *total_out, void *stream);
ibvh_status ibvh_dist_cross_write(const ibvh_bvh *bvh, const ibvh_dist_cross_plan_t *plan, const void *import_buf, void *scratch,
                                  size_t scratch_bytes, const int64_t *totals, void *contacts_out, void *stream);

/* Release what ibvh_comm_from_rccl allocated for `comm` (the ncclComm_t itself stays the caller's). */
ibvh_status ibvh_comm_release(ibvh_comm *comm);

/* ----------------------------------------------------------------------------------- */
/* input preparation adjacent to the path                                               */
/* ----------------------------------------------------------------------------------- */
/* BSphere{T}(p1,p2,p3) (bsphere.jl:43-112) / BBox{T}(p1,p2,p3) (bbox.jl:59-70) for n triangles
 * stored as n x 9 values (p1 p2 p3) of float type `flt`; writes n volumes of `kind`. */
ibvh_status ibvh_volumes_from_triangles(int32_t kind, int32_t flt, const void *triangles, int64_t n,
                                        void *volumes_out, void *stream);

/* Deterministic synthetic inputs shared by bench, tests and the oracle (SplitMix64 counter
 * based).  Writes n BSphere{F32} with centres uniform in
 * [origin, origin+extent)^3 and radius r0*(0.5+0.5u). */
ibvh_status ibvh_generate_spheres_f32(int64_t n, uint64_t seed, int64_t first_index,
                                      const float origin[3], const float extent[3], float r0,
                                      void *volumes_out, void *stream);

/* Per-launch timing, used by bench.py for the roofline figures: when enabled, every kernel the
 * library launches is bracketed by HIP events on its launch stream.  _get synchronises on the
 * record's stop event; names are the kernel instantiations' source spellings. */
ibvh_status ibvh_profile_enable(int32_t on); /* also clears the records */
ibvh_status ibvh_profile_count(int64_t *count_out);
ibvh_status ibvh_profile_get(int64_t i, const char **name_out, float *ms_out);

/* Work of ONE counting pass of the leaf-vs-tree walkers (SURVEY.md §8d "touched bytes"; the reference's own counter,
 * BVHTraversal.num_checks, exists for BFS only: bfs/traverse_single.jl:25,48).  Runs the counting pass of the walk the
 * ordinary entry points would take — self (bvh2 = points = NULL), pair (bvh2), or rays (points / directions, num_rays) —
 * in an instantiation that also counts, and leaves in `work_out` (DEVICE, 4 x uint64, zeroed here):
 *   [0] node tests   (one lane-level box-box / ray-box test against a node volume)
 *   [1] leaf tests   (one exact leaf-leaf / ray-leaf test)
 *   [2] node records fetched   [3] leaf records fetched
 * `counts`: per-work-item counts as for the _count calls (max(n1, n2) / num_rays / n entries), not scanned.
 * Measurement only; instantiated for BSphere{Float32} leaves, BBox{Float32} nodes, Int32 indices, default start
 * levels, no `narrow` (anything else: IBVH_ERR_UNSUPPORTED). */
ibvh_status ibvh_lvt_work_counters(const ibvh_bvh *bvh, const ibvh_bvh *bvh2, const void *points,
                                   const void *directions, int64_t num_rays, void *counts, void *work_out,
                                   void *stream);

/* Development knobs, for measurements and tests only (the defaults are the shipped behaviour; results never depend
 * on them, only speed and which code path is taken).  One process-wide table: set a knob BEFORE the calls it should
 * affect and not concurrently with them.  The library never reads the environment.  Names (exactly the table in
 * csrc/ibvh_core.hip; meanings: csrc/ibvh_common.hpp, struct Tuning): "ray_block", "lvt_wide", "lvt_xcd", "sort_lsd",
 * "sort_msd_avg", "msd_avg", "msd_equalize", "msd_rescue", "lvt_scan_fused", "bfs_wg_per_cu", "bfs_grid" (k > 0 = exactly k
 * workgroups for every BFS level kernel, at most CUs x 16; 0 = CUs x bfs_wg_per_cu), "lvt_blocks", "lvt_block_shift", "lvt_blocks_min_items", "lvt_blocks_paired_below", "rays_binned" (1 = the binned ray path where it
 * pays, 2 = wherever the tree allows it, 0 = never), "rays_subtree_depth", "rays_items_per_ray", "rays_tail".  Unknown
 * name: IBVH_ERR_INVALID_ARG — that includes the knobs of removed experiments (lvt_dual, rays_shadow, msd_range and
 * rays_fast_slab; the last commit with them is f9264f8) and the knobs that forced sort geometries no shipped plan picks
 * (sort_tile, bucket_tpb, msd_bits, msd_cap, msd_tile, msd_ftpb, msd_resident_kb and msd_finish_pad_kb; the last
 * commit with them is 19cd0eb). */
ibvh_status ibvh_set_tuning(const char *name, int32_t value);
ibvh_status ibvh_get_tuning(const char *name, int32_t *value_out);

/* Library / device introspection. */
const char *ibvh_version(void);
const char *ibvh_status_string(int32_t status);

#ifdef __cplusplus
}
#endif
#endif /* IBVH_H */
