"""Host-side mirror of ImplicitBVH.jl's hot-path API over libibvh (HIP, gfx950).

Same names, argument meaning and error behaviour as the reference:
    BVH(bounding_volumes, node_type; built_level, cache, options)      src/build.jl:198-271
    traverse(bvh[, bvh2], alg; start_level..., narrow, cache, options)  src/traverse/traverse.jl:210-233
    traverse_rays(bvh, points, directions, alg; ...)                    src/raytrace/raytrace.jl:71-80
    BVHOptions, DefaultMortonAlgorithm, LVTTraversal, BFSTraversal, BVHTraversal, ImplicitTree,
    default_start_level, memory_index, level_indices, isvirtual.
Device memory is torch tensors on the current CUDA(HIP) device; this module allocates buffers, fills
the POD descriptors of include/ibvh.h and calls the C entry points.  Nothing is computed on the host
and there is no CPU fallback.

Python renderings of Julia types:
    BSphere{T} arrays  -> float tensor of shape (n, 4): x, y, z, r
    BBox{T} arrays     -> float tensor of shape (n, 6): lo, up
    node_type          -> BSphere(dtype) / BBox(dtype) tokens, e.g. BBox(torch.float32)
    Vector{BoundingVolume{V,I,M}} -> BoundingVolumes (byte buffer with the Julia record layout)
    Vector{IndexPair{I}}          -> integer tensor of shape (n, 2)
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import abi, lib

__all__ = [
    "load_obj_triangles", "BSphere", "BBox", "BoundingVolumes", "BVHOptions", "DefaultMortonAlgorithm", "ImplicitTree", "BVH",
    "BVHTraversal", "LVTTraversal", "BFSTraversal", "traverse", "traverse_rays", "default_start_level",
    "memory_index", "level_indices", "isvirtual", "bounding_volumes_from_triangles", "generate_spheres",
    "NARROW_MORTON_LT", "NARROW_INDEX_LT", "NARROW_RAY_ORIGIN_OUTSIDE", "LeafBatch", "lvt_work_counters", "refit",
    "resolve_triangles", "raycast", "RayHits", "closest_points", "ClosestPoints",
    "nearest_leaves", "NearestLeaves", "point_crossings", "PointCrossings", "points_inside", "signed_distance",
    "cast_rays", "RayCast", "sphere_contacts", "SphereContacts",
    "triangle_contacts", "TriangleContacts", "self_intersections", "sweep_spheres", "SphereSweep",
    "triangle_distances", "TriangleDistances", "mesh_distance", "MeshDistance", "self_clearance",
    "capsule_contacts", "CapsuleContacts", "segment_distances", "SegmentDistances",
    "box_contacts", "BoxContacts", "voxelize", "cast_spheres", "SphereCast",
]

NARROW_MORTON_LT = abi.NARROW_MORTON_LT
NARROW_INDEX_LT = abi.NARROW_INDEX_LT
NARROW_RAY_ORIGIN_OUTSIDE = abi.NARROW_RAY_ORIGIN_OUTSIDE


def _torch():
    import torch
    return torch


_gpu_checked = False


def _require_gpu():
    global _gpu_checked
    torch = _torch()
    if _gpu_checked:  # (a GPU does not go away; torch.cuda.is_available() costs 2 us a call on the time-stepping path)
        return torch
    if not torch.cuda.is_available():
        raise RuntimeError("implicitbvh_amd needs an AMD GPU (MI355X / gfx950); there is no CPU fallback")
    lib.load()
    _gpu_checked = True
    return torch


_raw_stream = None  # torch._C._cuda_getCurrentRawStream when this torch has it: 0.3 us instead of ~9 us per call


def _stream():
    """torch's current stream on the current device as a void* for the C ABI.  This sits on the host's critical path of
    a time-stepping loop that reads the contact count every step (the GPU idles until the next build's first launch
    arrives), hence the raw accessor instead of torch.cuda.current_stream()."""
    global _raw_stream
    torch = _torch()
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream:
        return C.c_void_p(_raw_stream(torch._C._cuda_getDevice()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def _float_code(dtype):
    torch = _torch()
    if dtype in (torch.float32, np.float32, "float32", float.__name__ + "32"):
        return abi.F32
    if dtype in (torch.float64, np.float64, "float64", float):
        return abi.F64
    raise ValueError(f"unsupported float type {dtype} (Float32 and Float64 are instantiated)")


def _torch_float(code):
    torch = _torch()
    return torch.float32 if code == abi.F32 else torch.float64


def _index_code(x):
    torch = _torch()
    if x in (torch.int32, np.int32, "int32") or isinstance(x, np.int32):
        return abi.I32
    if x in (torch.int64, np.int64, "int64", int) or isinstance(x, (np.int64, int)):
        return abi.I64
    raise ValueError(f"unsupported index type {x} (Int32 and Int64 are instantiated)")


def _torch_index(code):
    torch = _torch()
    return torch.int32 if code == abi.I32 else torch.int64


_morton_memo = {}


def _morton_code(x):
    if not isinstance(x, (type, str, np.dtype)):  # (instances of a Morton type: rare, not memoised)
        return _morton_code_slow(x)
    code = _morton_memo.get(x)
    if code is None:
        code = _morton_memo[x] = _morton_code_slow(x)
    return code


def _morton_code_slow(x):
    for code, dt in abi.MORTON_DTYPES.items():
        if x is dt or x == dt or isinstance(x, dt) or x == np.dtype(dt).name:
            return code
    raise ValueError(f"unsupported Morton type {x} (UInt16, UInt32, UInt64)")


# ---------------------------------------------------------------------------------------------
# type tokens
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class _VolumeType:
    kind: int
    flt: int

    def __repr__(self):
        return f"{'BSphere' if self.kind == abi.BSPHERE else 'BBox'}{{{'Float32' if self.flt == abi.F32 else 'Float64'}}}"


def BSphere(dtype=None):
    """Type token BSphere{T} (bsphere.jl:26-29)."""
    return _VolumeType(abi.BSPHERE, _float_code(dtype if dtype is not None else _torch().float32))


def BBox(dtype=None):
    """Type token BBox{T} (bbox.jl:35-38)."""
    return _VolumeType(abi.BBOX, _float_code(dtype if dtype is not None else _torch().float32))


@dataclass(frozen=True)
class DefaultMortonAlgorithm:
    """morton/default.jl:21-40.  `exemplar` is a numpy unsigned type (np.uint16/32/64)."""
    exemplar: type = np.uint32
    compute_extrema: bool = True
    mins: tuple = (float("nan"),) * 3
    maxs: tuple = (float("nan"),) * 3

    def __post_init__(self):
        _morton_code(self.exemplar)


@dataclass(frozen=True)
class BVHOptions:
    """utils.jl:34-93.  CPU threading knobs are kept for signature parity; only `index`, `morton` and
    `block_size` influence the GPU path (block_size is advisory: kernels pick their own geometry)."""
    index: object = np.int32
    morton: DefaultMortonAlgorithm = field(default_factory=DefaultMortonAlgorithm)
    num_threads: int = 1
    min_mortons_per_thread: int = 100
    min_sorts_per_thread: int = 100
    min_boundings_per_thread: int = 100
    min_traversals_per_thread: int = 100
    block_size: int = 256

    def __post_init__(self):
        for name in ("num_threads", "min_mortons_per_thread", "min_sorts_per_thread", "min_boundings_per_thread",
                     "min_traversals_per_thread", "block_size"):
            if not getattr(self, name) > 0:  # @argcheck ... > 0 (utils.jl:73-78)
                raise ValueError(f"BVHOptions: {name} > 0 must hold")
        _index_code(self.index)

    @property
    def index_code(self):
        return _index_code(self.index)

    @property
    def morton_code(self):
        return _morton_code(self.morton.exemplar)


class LVTTraversal:
    """Leaf-vs-tree traversal (traverse/leaf_vs_tree/leaf_vs_tree.jl:1), the default."""


class BFSTraversal:
    """Breadth-first BVTT traversal (traverse/breadth_first/breadth_first.jl:1)."""


# ---------------------------------------------------------------------------------------------
# ImplicitTree
# ---------------------------------------------------------------------------------------------
class ImplicitTree:
    """implicit_tree.jl:52-90."""

    def __init__(self, num_leaves):
        self._t = abi.Tree()
        lib.call("ibvh_tree_shape", int(num_leaves), C.byref(self._t))

    levels = property(lambda s: s._t.levels)
    real_leaves = property(lambda s: s._t.real_leaves)
    real_nodes = property(lambda s: s._t.real_nodes)
    virtual_leaves = property(lambda s: s._t.virtual_leaves)
    virtual_nodes = property(lambda s: s._t.virtual_nodes)

    def __repr__(self):
        return f"ImplicitTree(levels: {self.levels}, real_leaves: {self.real_leaves})"


def memory_index(tree, implicit_index):
    out = C.c_int64()
    try:
        lib.call("ibvh_memory_index", C.byref(tree._t), int(implicit_index), C.byref(out))
    except ValueError as e:
        raise IndexError(str(e))  # BoundsError (implicit_tree.jl:131-135)
    return out.value


def level_indices(tree, level):
    a, b = C.c_int64(), C.c_int64()
    try:
        lib.call("ibvh_level_indices", C.byref(tree._t), int(level), C.byref(a), C.byref(b))
    except ValueError as e:
        raise IndexError(str(e))
    return a.value, b.value


def isvirtual(tree, implicit_index):
    out = C.c_int32()
    try:
        lib.call("ibvh_isvirtual", C.byref(tree._t), int(implicit_index), C.byref(out))
    except ValueError as e:
        raise IndexError(str(e))
    return bool(out.value)


# Per-(types, n) constants of a build / traversal (tree shape, record layout, scratch sizes): pure functions of their key,
# asked of the library once.  A time-stepping caller rebuilds the same shape every step; on the step's critical path
# (the host reads the contact count, then enqueues the next build) every avoided ctypes round trip counts.
_shape_memo = {}


def _memo(key, make):
    v = _shape_memo.get(key)
    if v is None:
        if len(_shape_memo) > 256:
            _shape_memo.clear()
        v = _shape_memo[key] = make()
    return v


def _layout_of(types):
    def make():
        lay = abi.Layout()
        lib.call("ibvh_layout_of", C.byref(types), C.byref(lay))
        return lay
    return _memo(("layout", types.key()), make)


# ---------------------------------------------------------------------------------------------
# BoundingVolumes: Vector{BoundingVolume{V,I,M}} in device memory
# ---------------------------------------------------------------------------------------------
class BoundingVolumes:
    """Device array of BoundingVolume{V,I,M} records (bounding_volumes.jl:55-59) with the Julia layout."""

    def __init__(self, types, n, buf=None):
        torch = _torch()
        self.types = types
        self.n = int(n)
        lay = _layout_of(types)
        self.layout = lay
        if buf is None:
            buf = torch.zeros(self.n * lay.leaf_bytes, dtype=torch.uint8, device="cuda")
        self.buf = buf

    def __len__(self):
        return self.n

    @classmethod
    def wrap(cls, volumes, indices, options=None):
        """Manually wrapped volumes with user indices (build.jl:128-153); morton = 0."""
        torch = _require_gpu()
        options = options or BVHOptions()
        kind, flt = _volume_kind(volumes)
        types = abi.make_types(kind, flt, abi.BBOX, abi.F32, options.index_code, options.morton_code)
        out = cls(types, volumes.shape[0])
        out.volume.copy_(volumes)
        out.index.copy_(torch.as_tensor(indices, device="cuda").to(_torch_index(types.index_type)))
        return out

    def _strided(self, dtype, offset, width):
        torch = _torch()
        esz = torch.empty((), dtype=dtype).element_size()
        lb = self.layout.leaf_bytes
        assert lb % esz == 0 and offset % esz == 0
        flat = self.buf.view(dtype)
        return flat.as_strided((self.n, width), (lb // esz, 1), offset // esz)

    @property
    def volume(self):
        """(n, 4|6) strided float view of the .volume fields."""
        return self._strided(_torch_float(self.types.leaf_float), 0, abi.volume_width(self.types.leaf_kind))

    @property
    def index(self):
        return self._strided(_torch_index(self.types.index_type), self.layout.index_off, 1)[:, 0]

    @property
    def morton(self):
        """Morton codes as int64 (torch has no unsigned 32/64-bit arithmetic); values are exact for U16/U32
        and the two's-complement image for U64 (bit 63 is never set: 63 significant bits)."""
        torch = _torch()
        m = self.to_numpy()["morton"].astype(np.int64)
        return torch.from_numpy(m)

    @property
    def morton_device(self):
        """Morton codes as an int64 DEVICE tensor (a strided view widened on the fly; same value convention as .morton)."""
        torch = _torch()
        mb = {abi.U16: (torch.int16, 0xffff), abi.U32: (torch.int32, 0xffffffff), abi.U64: (torch.int64, None)}[self.types.morton_type]
        m = self._strided(mb[0], self.layout.morton_off, 1)[:, 0].to(torch.int64)
        return m if mb[1] is None else m & mb[1]

    def to_numpy(self):
        """Host copy as a numpy structured array (volume, index, morton)."""
        dt = abi.leaf_dtype(self.types)
        assert dt.itemsize == self.layout.leaf_bytes
        return self.buf.cpu().numpy().view(dt)


def _volume_kind(volumes):
    if volumes.dim() != 2 or volumes.shape[1] not in (4, 6):
        raise ValueError("bounding volumes must be an (n, 4) BSphere or (n, 6) BBox float tensor")
    if not volumes.is_cuda:
        raise ValueError("bounding volumes must live on the GPU (device='cuda')")
    return (abi.BSPHERE if volumes.shape[1] == 4 else abi.BBOX), _float_code(volumes.dtype)


# ---------------------------------------------------------------------------------------------
# words the GPU writes for the host (traversal totals, skew hints)
# ---------------------------------------------------------------------------------------------
class _HostWords:
    """ONE block of mapped pinned host memory for the whole process, allocated once and never freed, handed out word by
    word, round robin.  The GPU writes into it (the total of an enqueued traversal: `total_host` of include/ibvh.h; the
    skew hint of a build: `skew_flag`) and the host reads it WITHOUT a stream synchronisation or a device-to-host copy.
    Because the block is never returned to torch's caching host allocator, a kernel still in flight when its BVH /
    traversal object dies can only ever write into memory this module owns.  A word is recycled after SLOTS later
    requests; a reader holding an older generation of the slot is told so instead of being given another call's value."""
    SLOTS = 8192       # totals: [0, SLOTS)
    HINT_SLOTS = 1024  # skew hints: [SLOTS, SLOTS + HINT_SLOTS) — a ring of their own, so that a build still in flight
    #                    can at worst overwrite another chain's HINT (speed only), never a traversal's total
    PENDING = -(1 << 62)  # what the host stores before the launch; the GPU overwrites it

    def __init__(self):
        torch = _torch()
        self.tensor = torch.zeros(self.SLOTS + self.HINT_SLOTS, dtype=torch.int64).pin_memory()
        self.words = self.tensor.numpy()  # the same memory
        self.base = self.tensor.data_ptr()
        self.generation = [0] * (self.SLOTS + self.HINT_SLOTS)
        self.next = 0
        self.next_hint = 0
        self.devices_this_lap = set()  # devices whose streams may hold a scan kernel that writes a total slot of this lap
        import threading
        self.lock = threading.Lock()

    def take(self, initial, hint=False):
        with self.lock:
            if hint:
                slot = self.SLOTS + self.next_hint
                self.next_hint = (self.next_hint + 1) % self.HINT_SLOTS
            else:
                slot = self.next
                self.next = (self.next + 1) % self.SLOTS
                if self.next == 0:
                    # the ring wraps: a scan kernel of the previous lap that is STILL queued would overwrite the new
                    # owner's PENDING word with its own total.  One synchronisation per SLOTS traversals retires
                    # every such kernel before its slot is handed out again — of EVERY device this process drives (ADVICE
                    # r4: a traversal queued on another device is otherwise not retired), and under the lock on purpose:
                    # a thread that took a slot of the new lap meanwhile could launch behind a stale kernel of the old lap
                    # on its own stream and read that kernel's total as its own.  Cost: one device drain per 8,192 traversals.
                    # Only the devices that were handed a slot during the lap that just ended (in a one-process-per-GPU
                    # job every GPU is visible, and synchronising all of them creates a context — hundreds of MB — on each).
                    torch = _torch()
                    for d in sorted(self.devices_this_lap):
                        torch.cuda.synchronize(d)
                    self.devices_this_lap = set()
                self.devices_this_lap.add(_torch().cuda.current_device())
            self.generation[slot] += 1
            gen = self.generation[slot]
        self.words[slot] = initial
        return slot, gen

    def ptr(self, slot):
        return self.base + 8 * slot


class _HintWord:
    """A build chain's skew hint: one word of the _HostWords hint ring; word[0] reads / writes the value."""

    def __init__(self, initial):
        self.slot, self.gen = _host_words().take(initial, hint=True)
        self.holdoff = 0  # rebuilds for which the chain does not ask for equalised cells (apply)

    def valid(self):
        return _host_words().generation[self.slot] == self.gen

    def ptr(self):
        return _host_words().ptr(self.slot)

    def __getitem__(self, i):
        return int(_host_words().words[self.slot]) & 0xff  # extra levels the last build would have used (include/ibvh.h, skew_flag)

    def occupancy(self):
        """Fullest coarse cell of the last build in 1/128 of what one finish workgroup sorts (second byte of the word)."""
        return (int(_host_words().words[self.slot]) >> 8) & 0xff

    def __setitem__(self, i, v):
        _host_words().words[self.slot] = int(v)

    def equalize(self):
        """Bit 16: the last build ran with equalised cells and the plain grid would still have had a crowded cell."""
        return (int(_host_words().words[self.slot]) >> 16) & 1

    def apply(self, d):
        """sort_levels / sort_equalize of a rebuild from what the chain's previous build left in the word (read ONCE)."""
        d.sort_levels, d.sort_equalize, self.holdoff = sort_hint_rule(int(_host_words().words[self.slot]), d.n, self.holdoff)


def sort_hint_rule(word, n, holdoff):
    """(sort_levels, sort_equalize, holdoff') of a rebuild of n leaves from the hint word the previous build of its chain left
    (include/ibvh.h, ibvh_build_desc.skew_flag: low byte = extra partition levels that build would have used, second byte =
    its fullest cell in 1/128 of what a finish workgroup sorts, bit 16 = it ran with equalised cells and the plain grid would
    still have been crowded, bit 17 = equalising did not help, bit 18 = it ran with equalised cells) and the chain's counter
    `holdoff`: > 0 = rebuilds left on the plain grid after bit 17; -1 = PROBATION: the previous request went back to the plain
    grid on an equalised build's estimate (bit 16 = 0), with a spare level as insurance; <= -2 = STICKY: the probation build was
    crowded after all, so the chain stays with equalised cells for EQ_STICKY rebuilds whatever bit 16 says (round 6: a mesh
    whose fullest grid cell sits just above one workgroup's share went plain / equalised / plain ... every other build).
    Pure host logic; the Julia extension carries the same function (tests/test_host_cpu.py evaluates both)."""
    used, occupancy, eq, nohelp, ran_eq = word & 0xff, (word >> 8) & 0xff, (word >> 16) & 1, (word >> 17) & 1, (word >> 18) & 1
    sticky = 0
    if holdoff <= -2:
        if nohelp == 1:
            holdoff = EQ_HOLDOFF
        else:
            sticky = 1
            holdoff = holdoff + 1
            if holdoff == -1:
                holdoff = 0
    elif holdoff == -1:
        if used > 0:
            sticky = 1
            holdoff = -2 - EQ_STICKY
        else:
            holdoff = 0
    elif nohelp == 1 and holdoff == 0:
        # (bit 17: an equalised build found most of its records in crowded cells all the same — runs of equal keys — so the chain
        # stays with the plain grid for EQ_HOLDOFF rebuilds before it tries again)
        holdoff = EQ_HOLDOFF
    elif holdoff > 0:
        holdoff = holdoff - 1
    equalize = 1 if (used > 0 or eq == 1 or sticky == 1) and EQUALIZE and holdoff <= 0 else 0
    probation = 1 if ran_eq == 1 and equalize == 0 and holdoff == 0 and EQUALIZE else 0
    if probation == 1:
        holdoff = -1
    threshold = EQ_SPARE_OCCUPANCY if eq == 1 and equalize == 1 else SPARE_OCCUPANCY
    spare = 1 if used > 0 or occupancy >= threshold or n >= SPARE_ALWAYS_FROM or probation == 1 else 0
    return min(used + spare, abi.MAX_SORT_LEVELS), equalize, holdoff


_host_words_singleton = None


def _host_words():
    global _host_words_singleton
    if _host_words_singleton is None:
        _host_words_singleton = _HostWords()
    return _host_words_singleton


# ---------------------------------------------------------------------------------------------
# BVH
# ---------------------------------------------------------------------------------------------
class BVH:
    """struct BVH + constructor (build.jl:155-271).

        bvh = BVH(bounding_volumes, BBox(torch.float32), built_level=1, cache=None, options=BVHOptions())

    bounding_volumes: (n,4)/(n,6) CUDA float tensor, or a BoundingVolumes (kept indices, sorted IN PLACE,
    build.jl:128-153).  built_level: int level or float fraction (build.jl:309-325).  cache: a previous BVH
    whose nodes / skips / scratch buffers are reused (build.jl:232-238, 257-263).
    Fields: built_level, tree, skips, nodes, leaves (+ extrema: the expanded Morton bounds, device tensor).
    """

    def __init__(self, bounding_volumes, node_type=None, built_level=1, cache: Optional["BVH"] = None, options=None,
                 _out_of_place=False):
        torch = _require_gpu()
        # Time-stepping fast path: the same call as the one that built `cache` (raw volumes of the same shape and type,
        # default options, same node type and built level) repeats nothing but the build itself — every buffer, the tree
        # shape and the filled-in build descriptor are the cache's.  This is the host's critical path of a loop that reads
        # the contact count every step: the GPU idles from the moment the host sees the count until this call's first
        # launch arrives.
        fast = getattr(cache, "_fast", None) if cache is not None else None
        if (fast is not None and options is None and not _out_of_place and not isinstance(bounding_volumes, BoundingVolumes)
                and fast[0] == (bounding_volumes.shape, bounding_volumes.dtype, bounding_volumes.device, node_type, built_level)
                and bounding_volumes.is_cuda and bounding_volumes.is_contiguous() and cache._skew.valid()
                and bounding_volumes.data_ptr() != cache.leaves.buf.data_ptr()):
            d = fast[1]
            self.tree, self.built_level, self.types = cache.tree, cache.built_level, cache.types
            self.skips, self.nodes, self._scratch = cache.skips, cache.nodes, cache._scratch
            self.leaves, self.extrema, self._skew, self._fast = cache.leaves, cache.extrema, cache._skew, fast
            self._skew.apply(d)
            lib.call("ibvh_build", C.byref(d), _ptr(bounding_volumes), _ptr(self.leaves.buf), _ptr(self.nodes), _ptr(self.skips),
                     _ptr(self.extrema), _ptr(self._scratch), self._scratch.numel(), _stream())
            return
        # The reference's literal time-stepping loop — `bvh = BVH(bvh.leaves, N; cache=bvh)` after the leaves were moved IN
        # PLACE (build.jl:109-126, README.md:84-95): pre-wrapped records, user indices kept, the record array is input and
        # output.  Same idea: nothing but the build call itself is repeated.
        if (fast is not None and options is None and not _out_of_place and isinstance(bounding_volumes, BoundingVolumes)
                and bounding_volumes is cache.leaves and fast[0] == ("in place", bounding_volumes.buf.data_ptr(), len(bounding_volumes),
                                                                     node_type, built_level) and cache._skew.valid()):
            d = fast[1]
            self.tree, self.built_level, self.types = cache.tree, cache.built_level, cache.types
            self.skips, self.nodes, self._scratch = cache.skips, cache.nodes, cache._scratch
            self.leaves, self.extrema, self._skew, self._fast = cache.leaves, cache.extrema, cache._skew, fast
            self._skew.apply(d)
            lib.call("ibvh_build", C.byref(d), C.c_void_p(0), _ptr(self.leaves.buf), _ptr(self.nodes), _ptr(self.skips),
                     _ptr(self.extrema), _ptr(self._scratch), self._scratch.numel(), _stream())
            return
        fast_key = None
        if options is None and not _out_of_place and not isinstance(bounding_volumes, BoundingVolumes):
            fast_key = (bounding_volumes.shape, bounding_volumes.dtype, bounding_volumes.device, node_type, built_level)
        elif options is None and not _out_of_place:
            fast_key = ("in place", bounding_volumes.buf.data_ptr(), len(bounding_volumes), node_type, built_level)
        options = options or BVHOptions()
        node_type = node_type or BBox(torch.float32)  # default BBox{Float32} (build.jl:200)
        wrapped = isinstance(bounding_volumes, BoundingVolumes)
        if wrapped:
            src = bounding_volumes
            # check_bounding_volume_types (build.jl:355-361)
            if src.types.index_type != options.index_code:
                raise ValueError("BoundingVolume index type does not match BVHOptions index_exemplar type")
            if src.types.morton_type != options.morton_code:
                raise ValueError("BoundingVolume morton type does not match BVHOptions morton type")
            kind, flt, n = src.types.leaf_kind, src.types.leaf_float, len(src)
        else:
            kind, flt = _volume_kind(bounding_volumes)
            n = bounding_volumes.shape[0]
        types = abi.make_types(kind, flt, node_type.kind, node_type.flt, options.index_code, options.morton_code)
        if not abi.combo_supported(types):
            raise ValueError(f"no conversion from {'BSphere' if kind == abi.BSPHERE else 'BBox'} leaves to {node_type!r}")
        self.tree = _memo(("tree", int(n)), lambda: ImplicitTree(n))  # DomainError for n < 1
        tree = self.tree
        # compute_build_level (build.jl:309-325)
        if isinstance(built_level, (int, np.integer)):
            if not 1 <= built_level <= tree.levels:
                raise ValueError("1 <= built_level <= tree.levels must hold")
            built_ilevel = int(built_level)
        elif isinstance(built_level, float):
            out = C.c_int64()
            lib.call("ibvh_compute_build_level", C.byref(tree._t), float(built_level), C.byref(out))
            built_ilevel = out.value
        else:
            raise TypeError("built_level (the level to build BVH up to) must be an Integer or AbstractFloat")
        self.built_level = built_ilevel
        self.types = types
        idt, ndt = _torch_index(types.index_type), _torch_float(types.node_float)
        nw = abi.volume_width(types.node_kind)
        num_nodes = tree.real_nodes - tree.real_leaves
        # buffers, honouring cache= (type checks as build.jl:235,260)
        if cache is None:
            self.skips = torch.empty(tree.levels, dtype=idt, device="cuda")
            self.nodes = torch.empty((num_nodes, nw), dtype=ndt, device="cuda")
            self._scratch = None
        else:
            if cache.skips.dtype != idt:
                raise ValueError("eltype(cache.skips) === I must hold")
            if cache.nodes.dtype != ndt or cache.nodes.shape[1] != nw:
                raise ValueError("eltype(cache.nodes) === N must hold")
            self.skips = cache.skips if cache.skips.numel() == tree.levels else torch.empty(tree.levels, dtype=idt, device="cuda")
            self.nodes = cache.nodes if cache.nodes.shape[0] == num_nodes else torch.empty((num_nodes, nw), dtype=ndt, device="cuda")
            self._scratch = cache._scratch
        def scratch_need():
            need = C.c_size_t()
            lib.call("ibvh_build_scratch_bytes", C.byref(types), n, C.byref(need))
            return need.value
        need = _memo(("build_scratch", types.key(), int(n)), scratch_need)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        if wrapped and _out_of_place:
            # source records stay untouched, the sorted records go to a (reused) buffer of their own
            nbytes = n * int(_layout_of(types).leaf_bytes)
            reuse = cache is not None and cache.leaves.buf.numel() == nbytes and cache.leaves.buf.data_ptr() != bounding_volumes.buf.data_ptr()
            self.leaves = BoundingVolumes(types, n, cache.leaves.buf if reuse else torch.empty(nbytes, dtype=torch.uint8, device="cuda"))
            vol_ptr = _ptr(bounding_volumes.buf)
        elif wrapped:
            self.leaves = bounding_volumes
            self.leaves.types = types  # node type is not part of the record layout
            vol_ptr = C.c_void_p(0)
        else:
            # raw volumes: the wrapped, sorted leaves are this BVH's own array — the cached one when it has the right size
            # and type (the reference allocates a new one every time, build.jl:345-349; with cache= a time step then
            # allocates nothing at all: nodes, skips, leaves, extrema and scratch are all reused)
            nbytes = n * int(_layout_of(types).leaf_bytes)
            reuse = (cache is not None and cache.leaves.buf.numel() == nbytes and cache.leaves.types.key() == types.key()
                     and cache.leaves.buf.data_ptr() != bounding_volumes.data_ptr())
            self.leaves = BoundingVolumes(types, n, cache.leaves.buf if reuse else torch.empty(nbytes, dtype=torch.uint8, device="cuda"))
            bounding_volumes = bounding_volumes.contiguous()
            vol_ptr = _ptr(bounding_volumes)
        ext_dt = _torch_float(flt)
        self.extrema = cache.extrema if (cache is not None and cache.extrema is not None and cache.extrema.dtype == ext_dt) \
            else torch.empty(6, dtype=ext_dt, device="cuda")
        # skewed inputs: a cold build launches COLD_SORT_LEVELS extra partition levels of the sort; a build that reuses
        # `cache=` launches as many as the previous build of the chain would have used, plus a spare one (none at all
        # after a uniform cloud).  The GPU leaves that number in a pinned host word (mapped into the device's address
        # space), which is read here WITHOUT synchronising: the latest value that has arrived is good enough for a
        # hint (include/ibvh.h, ibvh_build_desc.sort_levels / skew_flag).
        if cache is not None and getattr(cache, "_skew", None) is not None and cache._skew.valid():
            self._skew = cache._skew  # the chain's hint word
        else:
            self._skew = _HintWord(COLD_SORT_LEVELS)
        d = abi.BuildDesc()
        d.types = types
        d.n = n
        d.built_level = built_ilevel
        d.already_wrapped = 1 if wrapped else 0
        alg = options.morton
        d.compute_extrema = 1 if alg.compute_extrema else 0
        if not alg.compute_extrema:
            d.mins[:] = [float(v) for v in alg.mins]
            d.maxs[:] = [float(v) for v in alg.maxs]
        # A SPARE extra level (four launches that find nothing to do: ~15 us per step at 1e6 leaves) whenever the chain is
        # anywhere near needing one: the previous build used extra levels, or its fullest cell was beyond SPARE_OCCUPANCY
        # of what a finish workgroup sorts — a cloud that contracts or clusters over many steps reaches that long before
        # a cell overflows.  Only an input that changes ABRUPTLY from comfortably uniform to clustered meets no extra
        # level: its crowded cells take the one-workgroup slow path on that one step (correct; 17 ms at 1e6 leaves,
        # tools/attic/dbg_spike.py) and the hint it leaves fixes the next.  That path's cost grows with the cell (~0.1 s at 1e7
        # leaves) while the idle level's share of a step shrinks (1 % at 1e7), so builds of SPARE_ALWAYS_FROM leaves and
        # more always launch the spare level.  SPARE_OCCUPANCY = 0 restores "always" at every size.
        # EQUALISED cells (include/ibvh.h, sort_equalize) once the chain's input has shown that it does not fill the grid: the
        # previous build needed extra levels, or — itself built with equalised cells — reported that the plain grid would still
        # have had a crowded cell (bit 16 of the hint).  A cloud that fills its box never pays the two extra launches.
        if cache is None:
            d.sort_levels, d.sort_equalize = COLD_SORT_LEVELS, 0
        else:
            self._skew.apply(d)
        d.skew_flag = self._skew.ptr()
        lib.call("ibvh_build", C.byref(d), vol_ptr, _ptr(self.leaves.buf), _ptr(self.nodes), _ptr(self.skips),
                 _ptr(self.extrema), _ptr(self._scratch), self._scratch.numel(), _stream())
        self._fast = (fast_key, d) if fast_key is not None else None

    @classmethod
    def from_buffers(cls, types, n, leaves_buf, nodes, built_level=1):
        """Wrap existing device buffers (sorted BoundingVolume records + node array, e.g. received from a peer
        GPU) as a BVH without building anything; skips are recomputed from the tree shape."""
        torch = _require_gpu()
        self = cls.__new__(cls)
        self.types = types
        self.tree = ImplicitTree(n)
        self.built_level = int(built_level)
        self.leaves = BoundingVolumes(types, n, leaves_buf)
        self.nodes = nodes
        sk = (C.c_int64 * self.tree.levels)()
        lib.call("ibvh_compute_skips", C.byref(self.tree._t), sk)
        self.skips = torch.tensor(list(sk), dtype=_torch_index(types.index_type), device="cuda")
        self.extrema = None
        self._scratch = None
        self._skew = None
        return self

    def struct(self):
        b = abi.Bvh()
        b.types = self.types
        b.tree = self.tree._t
        b.built_level = self.built_level
        b.leaves = self.leaves.buf.data_ptr()
        b.nodes = self.nodes.data_ptr() if self.nodes.numel() else 0
        b.skips = self.skips.data_ptr()
        return b

    def __repr__(self):
        return (f"BVH\n  built_level: {self.built_level}\n  tree:        {self.tree}\n  skips:       {tuple(self.skips.shape)}\n"
                f"  nodes:       {tuple(self.nodes.shape)}\n  leaves:      ({len(self.leaves)},)\n")


def refit(bvh, bounding_volumes=None):
    """Refit `bvh` IN PLACE to moved leaves and return it (include/ibvh.h, ibvh_refit): the leaf order, .index, .morton,
    skips, tree and extrema stay those of the last full build; every node is merged again bottom-up (aggregate_oibvh!,
    build.jl:366-523), bit-identical to a build's merge over the same records.  No extrema, Morton codes or sort.

        refit(bvh)                      bvh.leaves.volume was moved in place
        refit(bvh, bounding_volumes)    (m, 4) / (m, 6) CUDA tensor of the leaf type in the USER's order: the leaf with
                                        index k takes bounding_volumes[k - 1]

    Traversals stay exact; they only get slower as the Morton order goes stale — rebuild with BVH(..., cache=bvh) when
    they do.  The leaf indices are checked against m once per BVH object (one device reduction, one host read); an index
    outside 1..m raises ValueError.  The device also checks every index before it reads (bvh._refit_flag turns non-zero
    if it ever found one out of range: such a leaf keeps its volume)."""
    torch = _require_gpu()
    types = bvh.types
    vol_ptr, m = C.c_void_p(0), 0
    if bounding_volumes is not None:
        v = bounding_volumes
        if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.shape[1] != abi.volume_width(types.leaf_kind):
            raise ValueError(f"refit: bounding volumes must be an (m, {abi.volume_width(types.leaf_kind)}) tensor of the BVH's leaf kind")
        if v.dtype != _torch_float(types.leaf_float):
            raise ValueError(f"refit: bounding volumes must be {_torch_float(types.leaf_float)}, like the BVH's leaves")
        if not v.is_cuda:
            raise ValueError("refit: bounding volumes must live on the GPU (device='cuda')")
        v = v.contiguous()
        m = int(v.shape[0])
        if getattr(bvh, "_refit_checked", None) != m:
            lo, hi = (int(x) for x in torch.aminmax(bvh.leaves.index.to(torch.int64)))
            if lo < 1 or hi > m:
                raise ValueError(f"refit: leaf indices span {lo}..{hi}, outside 1..{m} (the number of bounding volumes given)")
            bvh._refit_checked = m  # refit never changes the indices; a rebuild (cache=) is a new object
        vol_ptr = _ptr(v)
    flag = getattr(bvh, "_refit_flag", None)
    if flag is None:
        flag = bvh._refit_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.call("ibvh_refit", C.byref(bvh.struct()), vol_ptr, m, _ptr(flag), _stream())
    return bvh


def default_start_level(bvh, alg=None):
    """lvt/leaf_vs_tree.jl:4-6 and bfs/breadth_first.jl:4-6."""
    if alg is None or isinstance(alg, LVTTraversal):
        return max(1, bvh.built_level)
    if isinstance(alg, BFSTraversal):
        return max(bvh.tree.levels // 2, bvh.built_level)
    raise ValueError(f"default_start_level not implemented for: {alg}")


# ---------------------------------------------------------------------------------------------
# traversal results
# ---------------------------------------------------------------------------------------------
class BVHTraversal:
    """traverse.jl:54-107.  cache1 holds the contacts ((m, 2) index tensor); cache2 is the other buffer
    (LVT: per-work-item inclusive counts; BFS: the second pair queue).  `.contacts` = cache1[:num_contacts].

    LVT traversals that were given a large-enough `cache` are enqueued without any host synchronisation
    (ibvh_traverse_*_lvt_enqueue): `num_contacts` is then read from the device the first time it is asked for
    (that read is the reference's `@allowscalar`, moved to where the value is needed).  If the contact buffer
    taken from the cache turns out too small, the writing pass runs then, into a new buffer — which needs the
    traversal's counts and scratch to be intact, i.e. not handed to a later call as `cache=` in between."""

    def __init__(self, start_level1, start_level2, num_checks, num_contacts, cache1, cache2, _scratch=None, _pending=None):
        self.start_level1 = start_level1
        self.start_level2 = start_level2
        self.num_checks = num_checks
        self._num_contacts = num_contacts
        self._cache1 = cache1
        self.cache2 = cache2
        self._scratch = _scratch
        self._pending = _pending  # (total: _PendingTotal, capacity, finish(total) -> contacts tensor)
        self._donated = False
        self._ray_list = None  # ray traversals: "lvt" (grouped by ray, user indices: what resolve_triangles takes), "bfs", "positions"

    def _resolve(self):
        if self._pending is None:
            return
        total_t, capacity, finish = self._pending
        self._pending = None
        total = int(total_t.item())  # the blocking read (the pinned word: published before the scan / writing pass finish)
        if hasattr(total_t, "order_current_stream"):
            total_t.order_current_stream()  # a consumer on another stream waits for the launch stream
        if self._cache1.dtype == _torch().int32 and total > 2**31 - 1:
            raise OverflowError("more than typemax(Int32) contacts")
        if total > capacity:
            if self._donated:
                raise RuntimeError("this traversal's buffers were reused as `cache=` before its contact count was read, and "
                                   "the cached contact buffer was too small for it: read .num_contacts before reusing the cache")
            self._cache1 = finish(total)
        self._num_contacts = total

    @property
    def num_contacts(self):
        self._resolve()
        return self._num_contacts

    @property
    def cache1(self):
        self._resolve()
        return self._cache1

    @property
    def contacts(self):
        return self.cache1[: self.num_contacts]

    def _capacity(self):
        """rows of the contact buffer, without forcing the count to be read"""
        return self._cache1.shape[0] if self._cache1 is not None else 0

    def _donate(self):
        """the buffers are about to be reused by another traversal"""
        self._donated = True
        return self._cache1


class LeafBatch:
    """What a `narrow` callable sees for one side of m candidate pairs, as tensors on the GPU: .volume (m, 4|6),
    .index (m,), .morton (m,) int64 — the fields of the reference's BoundingVolume (bounding_volumes.jl:55-59), batched."""

    def __init__(self, bvh, positions):
        rows = positions.long() - 1
        self.volume = bvh.leaves.volume[rows]
        self.index = bvh.leaves.index[rows]
        self.morton = bvh.leaves.morton_device[rows]

    def __len__(self):
        return int(self.index.shape[0])


def _narrow_code(narrow, rays=False):
    """-> (code for the C ABI, callable or None).  The reference takes any closure (traverse.jl:213, raytrace.jl:76) and
    only ever evaluates it as `iscontact(...) && narrow(...)` at leaf level, i.e. as a post-filter.  Menu entries run on
    the device; any other callable — VECTORISED: narrow(a: LeafBatch, b: LeafBatch) -> bool tensor, for rays
    narrow(bv: LeafBatch, points (m, 3), directions (m, 3)) — is applied by this mirror to the candidate list the device
    returns as leaf positions (IBVH_OUTPUT_POSITIONS, include/ibvh.h)."""
    if narrow is None:
        return abi.NARROW_NONE, None
    menu = (abi.NARROW_NONE, abi.NARROW_RAY_ORIGIN_OUTSIDE) if rays else (abi.NARROW_NONE, abi.NARROW_MORTON_LT, abi.NARROW_INDEX_LT)
    if isinstance(narrow, (int, np.integer)) and not isinstance(narrow, bool):
        if int(narrow) in menu:
            return int(narrow), None
        raise ValueError(f"narrow = {narrow} is not on the {'ray' if rays else 'pair'} menu of include/ibvh.h")
    if callable(narrow):
        return abi.OUTPUT_POSITIONS, narrow
    raise TypeError("narrow must be None, a menu constant (NARROW_*) or a vectorised callable")


def _post_filter(trav, narrow, bvh1, bvh2=None, rays=None):
    """Apply a callable `narrow` to a traversal whose contact list holds leaf POSITIONS; returns the traversal with the
    surviving contacts as user indices, order preserved (so LVT results keep the reference's order)."""
    torch = _torch()
    pos = trav.contacts
    if pos.shape[0] == 0:
        keep = torch.zeros(0, dtype=torch.bool, device=pos.device)
    if rays is not None:
        p, d = rays  # (N, 3) row-major
        a = LeafBatch(bvh1, pos[:, 0])
        r = pos[:, 1].long() - 1
        keep = narrow(a, p[r], d[r]) if pos.shape[0] else keep
        out = torch.stack([a.index, pos[:, 1]], dim=1)
    else:
        a = LeafBatch(bvh1, pos[:, 0])
        b = LeafBatch(bvh2 if bvh2 is not None else bvh1, pos[:, 1])
        keep = narrow(a, b) if pos.shape[0] else keep
        if bvh2 is None:  # (min, max) of the user indices, traverse_single.jl:176-180
            out = torch.stack([torch.minimum(a.index, b.index), torch.maximum(a.index, b.index)], dim=1)
        else:
            out = torch.stack([a.index, b.index], dim=1)
    keep = torch.as_tensor(keep, device=pos.device).to(torch.bool).reshape(-1)
    if keep.shape[0] != pos.shape[0]:
        raise ValueError("narrow must return one bool per candidate pair")
    contacts = out[keep].to(pos.dtype).contiguous()
    return BVHTraversal(trav.start_level1, trav.start_level2, trav.num_checks, int(contacts.shape[0]), contacts, trav.cache2)


def _cache_tensor(cache_t, need_rows, cols, dtype, what):
    """Reuse a cache buffer if it is large enough (resize! semantics), checking its eltype (@argcheck)."""
    torch = _torch()
    shape = (need_rows, cols) if cols else (need_rows,)
    if cache_t is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    if cache_t.dtype != dtype or (cols and (cache_t.dim() != 2 or cache_t.shape[1] != cols)) or (not cols and cache_t.dim() != 1):
        raise ValueError(f"eltype(cache.{what}) does not match the traversal's index type")
    if cache_t.shape[0] < need_rows:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return cache_t


# Equalised builds re-fit their cells to the input every time, so a chain's occupancy does not creep up on them: a cell overflows only
# by sampling chance (32 samples per cell at 1e6 leaves: never, in practice) or through runs of equal keys (then `used` > 0 and the
# levels are launched anyway), and a mildly overflowing cell without a level costs one slower finish workgroup (~15 us), what the
# idle spare level (plan + four launches) costs EVERY step.  So they launch a spare level only when the fullest cell was about full.
EQ_SPARE_OCCUPANCY = 120
EQ_HOLDOFF = 32  # rebuilds a chain stays with the plain grid after an equalised build reported that it did not help (hint bit 17)
EQ_STICKY = 32   # rebuilds a chain stays with equalised cells after a return to the plain grid turned out crowded (sort_hint_rule)
EQUALIZE = True  # rebuilds of a chain whose input is skewed ask for equalised cells (False: the regular grid + extra levels, always)
COLD_SORT_LEVELS = 2  # extra partition levels a build without cache= launches (include/ibvh.h, sort_levels)
SPARE_OCCUPANCY = 96  # (of 128) fullest coarse cell from which a cached build launches a spare extra level (BVH.__init__)
SPARE_ALWAYS_FROM = 1 << 24  # leaves from which a cached build always launches it (the slow path it avoids grows with the input,
                             # the idle level's share of a step shrinks: 0.7 % at 1.7e7 leaves)
LVT_CACHE_SLOTS = 8  # contacts per work item kept from the counting pass (include/ibvh.h)
RAY_CACHE_SLOTS = 32  # hits per ray kept from the counting pass


def _speculative_buffer(cache, idt):
    """The cached contact buffer, if the traversal may be enqueued against it without knowing the count."""
    if cache is None or not isinstance(cache, BVHTraversal):
        return None
    buf = cache._donate()
    if buf is None or buf.dim() != 2 or buf.shape[1] != 2 or buf.shape[0] == 0:
        return None
    if buf.dtype != idt:
        raise ValueError("eltype(cache.cache1) does not match the traversal's index type")
    return buf


class _LvtScratch:
    """The LVT scratch buffer of a chain of traversals that hand each other their buffers through `cache=`, plus a ring
    of device-side totals.

    A traversal that was enqueued without a host read (`*_enqueue`) fetches its total contact count later, possibly
    after later traversals have reused — and rewritten — the scratch buffer (header, tile sums and contact cache
    alike).  So the totals do NOT live in the scratch: every call hands the library its own int64 word of a separate
    64-entry ring (`total_dev` of include/ibvh.h), which nothing else writes until the ring wraps, 64 calls later; a
    total that was never read by then raises instead of returning another call's number.  The host normally gets
    the total from the pinned mirror word the scan kernel fills (`total_host`), without touching the stream."""
    SLOTS = 64

    def __init__(self, nbytes):
        torch = _torch()
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.totals = torch.zeros(self.SLOTS, dtype=torch.int64, device="cuda")
        self.calls = 0

    def capacity(self):
        return self.buf.numel()

    def data_ptr(self):
        return self.buf.data_ptr()

    def numel(self):
        return self.buf.numel()

    def next_total(self):
        """(device pointer of this call's total word, pinned host pointer of its mirror, handle to read it later)"""
        slot = self.calls % self.SLOTS
        self.calls += 1
        hw = _host_words()
        hslot, hgen = hw.take(_HostWords.PENDING)
        return C.c_void_p(self.totals.data_ptr() + 8 * slot), C.c_void_p(hw.ptr(hslot)), _PendingTotal(self, slot, self.calls, hslot, hgen)


class _PendingTotal:
    SPIN = 2_000_000  # polls of the pinned word before falling back to the event + device read (seconds of spinning)

    def __init__(self, owner, slot, calls, hslot, hgen):
        self.owner, self.slot, self.calls = owner, slot, calls
        self.hslot, self.hgen = hslot, hgen
        self.event = None

    def launched(self):
        """Remember the stream the traversal was enqueued on (the raw handle: no event is recorded on the hot path).  The
        pinned word is published BEFORE the scan and the guarded writing pass have finished, so a consumer on ANOTHER
        stream must be ordered behind this one explicitly: order_current_stream()."""
        self.stream = _stream().value or 0
        return self

    def order_current_stream(self):
        """Make torch's current stream wait for everything enqueued on the launch stream so far (a no-op when they are the
        same stream: in-order).  Called by BVHTraversal._resolve before the writing pass is re-launched or the contacts
        are handed out."""
        stream = getattr(self, "stream", None)
        if stream is None:
            return
        cur = _stream().value or 0
        if cur == stream:
            return
        torch = _torch()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream())
        torch.cuda.current_stream().wait_event(ev)

    def item(self):
        if self.owner.calls - self.calls >= self.owner.SLOTS:
            raise RuntimeError("this traversal's contact count was never read and its slot in the totals ring has been "
                               f"recycled by {self.owner.SLOTS} later traversals on the same cache")
        # The scan kernel stores the total into the pinned word as well (total_host): poll it — no stream
        # synchronisation, no device-to-host copy (the reference's blocking `@allowscalar` read costs both,
        # lvt/traverse_single.jl:60).
        hw = _host_words()
        if hw.generation[self.hslot] == self.hgen:
            words, k = hw.words, self.hslot
            for _ in range(self.SPIN):
                v = int(words[k])
                if v != _HostWords.PENDING:
                    return v
        # the word never arrived (not expected): wait for the launch stream, read the device copy
        stream = getattr(self, "stream", None)
        torch = _torch()
        if stream:
            torch.cuda.ExternalStream(stream).synchronize()
        else:
            torch.cuda.synchronize()
        return int(self.owner.totals[self.slot].item())


def _cache_slots(cache, n_items, default):
    """Contact-cache slots per work item: the default, or — when a previous traversal's contact buffer is being
    reused — about four times the contacts per item that buffer was sized for (rounded up to a power of two, at most
    64): a wave whose items together overflow their pooled slots has to walk twice (7 contacts per leaf: 0.50 ms with
    8 slots, 0.30 ms with 32 at 1e6 leaves).  Uses the buffer's size only, never forces the lazy count to be read."""
    if not isinstance(cache, BVHTraversal) or n_items <= 0:
        return default
    per_item = -(-cache._capacity() // int(n_items))  # ceil
    want = 1
    while want < 4 * per_item:
        want *= 2
    return max(default, min(64, want))


def _lvt_scratch(cache, types, n_items, slots=None, rays_bvh=None, types2=None):
    """types2: the other BVH of a pair of two types (IBVH_PAIR_MIXED_TYPES): the larger of the two sizes (include/ibvh.h)."""
    k = _cache_slots(cache, n_items, LVT_CACHE_SLOTS if slots is None else slots)

    def scratch_need():
        need = C.c_size_t()
        if rays_bvh is not None:  # rays: room for the binned path's tables where it serves the batch (include/ibvh.h)
            s = rays_bvh.struct()
            lib.call("ibvh_rays_scratch_bytes", C.byref(s), int(n_items), k, C.byref(need))
            return need.value
        best = 0
        for t in (types,) if types2 is None else (types, types2):
            lib.call("ibvh_lvt_scratch_bytes", C.byref(t), int(n_items), k, C.byref(need))
            best = max(best, need.value)
        return best
    key = ("lvt_scratch", types.key(), None if types2 is None else types2.key(), int(n_items), k) if rays_bvh is None else \
        ("rays_scratch", types.key(), int(n_items), k, len(rays_bvh.leaves), rays_bvh.built_level)
    need = _memo(key, scratch_need)
    s = cache._scratch if cache is not None else None
    if not isinstance(s, _LvtScratch) or s.capacity() < need:
        s = _LvtScratch(need)
    return s


def _check_start_level(bvh, start_level, lvt):
    """The start level's @argcheck of the LVT (lvt/traverse_single.jl:10) or the BFS (bfs/traverse_single.jl) algorithm."""
    if lvt and not (bvh.built_level <= start_level <= bvh.tree.levels <= 32):
        raise ValueError("bvh.built_level <= start_level <= bvh.tree.levels <= 32 must hold")
    if not lvt and not (bvh.tree.levels >= start_level >= bvh.built_level):
        raise ValueError("bvh.tree.levels >= start_level >= bvh.built_level must hold")


def _lvt_two_pass(entry, args, n_items, idt, cache, scratch, sl1, sl2=0, keep=None):
    """The leaf-vs-tree protocol of every traversal shape (the Julia extension's lvt_two_pass).  `entry` names the shape's
    family of entry points (ibvh_traverse_*_lvt_{count,write,enqueue}), `args` are their leading arguments, up to `narrow`.
    With a contact buffer in `cache`, count, scan and a writing pass guarded by that buffer's size are enqueued without a
    host read, and the total is read when first asked for (BVHTraversal._resolve); otherwise the blocking count, then the
    write.  keep: what `args` point into that the deferred write still reads (the rays)."""
    counts = _cache_tensor(cache.cache2 if cache else None, n_items, 0, idt, "cache2")
    sp, sn = _ptr(scratch), scratch.numel()
    spec = _speculative_buffer(cache, idt)
    if spec is not None:
        tdev, thost, pending = scratch.next_total()
        lib.call(entry + "_enqueue", *args, _ptr(counts), _ptr(spec), spec.shape[0], tdev, thost, sp, sn, _stream())
        pending.launched()

        def finish(total, keep=keep):  # (keep: bound to the closure, alive until the write has run)
            contacts = _torch().empty((total, 2), dtype=idt, device="cuda")
            lib.call(entry + "_write", *args, _ptr(counts), _ptr(contacts), sp, sn, _stream())
            return contacts
        return BVHTraversal(sl1, sl2, 0, None, spec, counts, scratch, _pending=(pending, spec.shape[0], finish))
    total = C.c_int64()
    lib.call(entry + "_count", *args, _ptr(counts), C.byref(total), sp, sn, _stream())
    contacts = _cache_tensor(cache.cache1 if cache else None, total.value, 2, idt, "cache1")
    if total.value:
        lib.call(entry + "_write", *args, _ptr(counts), _ptr(contacts), sp, sn, _stream())
    return BVHTraversal(sl1, sl2, 0, total.value, contacts, counts, scratch)


def _traverse_lvt_single(bvh, start_level, narrow, cache):
    torch = _require_gpu()
    idt = _torch_index(bvh.types.index_type)
    _check_start_level(bvh, start_level, lvt=True)
    if bvh.tree.real_nodes <= 1:  # traverse_single.jl:17-21
        return BVHTraversal(start_level, 0, 0, 0, torch.empty((0, 2), dtype=idt, device="cuda"),
                            torch.empty(0, dtype=idt, device="cuda"))
    n = len(bvh.leaves)
    return _lvt_two_pass("ibvh_traverse_lvt", (C.byref(bvh.struct()), start_level, narrow), n, idt, cache,
                         _lvt_scratch(cache, bvh.types, n), start_level)


def _traverse_lvt_pair(bvh1, bvh2, sl1, sl2, narrow, cache):
    _require_gpu()
    if bvh1.types.index_type != bvh2.types.index_type:
        raise ValueError("get_index_type(bvh2) === I must hold")  # traverse_pair.jl:50-52
    idt = _torch_index(bvh1.types.index_type)
    _check_start_level(bvh1, sl1, lvt=True)
    _check_start_level(bvh2, sl2, lvt=True)
    n = max(len(bvh1.leaves), len(bvh2.leaves))
    mixed = bvh1.types.key() != bvh2.types.key()
    if mixed:  # two types (IBVH_PAIR_MIXED_TYPES): the walked tree's nodes are tested against NodeType(leaf) (traverse_pair.jl:196-197)
        smaller = bool(narrow & abi.PAIR_SMALLER_DRIVES)
        flip = len(bvh1.leaves) > len(bvh2.leaves) if smaller else not len(bvh1.leaves) >= len(bvh2.leaves)
        drv, oth = (bvh2, bvh1) if flip else (bvh1, bvh2)
        if drv.types.leaf_kind == abi.BBOX and oth.types.node_kind == abi.BSPHERE:
            f = {abi.F32: "Float32", abi.F64: "Float64"}
            raise abi.MethodError(f"no method matching BSphere{{{f[oth.types.node_float]}}}(::BBox{{{f[drv.types.leaf_float]}}})")
        narrow |= abi.PAIR_MIXED_TYPES
    return _lvt_two_pass("ibvh_traverse_pair_lvt", (C.byref(bvh1.struct()), C.byref(bvh2.struct()), sl1, sl2, narrow), n, idt,
                         cache, _lvt_scratch(cache, bvh1.types, n, types2=bvh2.types if mixed else None), sl1, sl2)


def _traverse_lvt_rays(bvh, p, d, start_level, narrow, cache):
    """p, d: the rays as (N, 3) row-major tensors of the leaf float type"""
    nr = p.shape[0]
    t = _lvt_two_pass("ibvh_traverse_rays_lvt", (C.byref(bvh.struct()), _ptr(p), _ptr(d), nr, start_level, narrow), nr,
                      _torch_index(bvh.types.index_type), cache,
                      _lvt_scratch(cache, bvh.types, nr, slots=RAY_CACHE_SLOTS, rays_bvh=bvh), start_level, keep=(p, d))
    t._ray_list = "positions" if narrow & abi.OUTPUT_POSITIONS else "lvt"
    return t


BFS_INITIAL_FACTOR = 4  # queues start at 4x the initial pair count (bfs/traverse_single.jl:73)
_last_bfs_counters = None
BFS_GROWTH = 4          # and grow at least 4x when a level does not fit (deeper levels need more still: 2x cost twice the resumes)


def _bfs_run(entry, types, initial_capacity, cache, levels_hint, *args):
    """Shared BFS driver.  Queues start at 4x the initial pair count (the reference's sizing, bfs/traverse_single.jl:73)
    or at the size of the cached buffers; when the library reports IBVH_ERR_CAPACITY both queues are grown (the pairs of
    the level that overflowed are kept) and the SAME traversal continues from that level — the reference's resize!
    between two levels (bfs/traverse_single.jl:38-53) — instead of starting over."""
    torch = _require_gpu()
    idt = _torch_index(types.index_type)
    cap = BFS_INITIAL_FACTOR * max(int(initial_capacity), 1)
    q1 = cache.cache1 if cache else None
    q2 = cache.cache2 if cache else None
    need = C.c_size_t()
    lib.call("ibvh_bfs_counters_bytes", int(levels_hint), C.byref(need))
    counters = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    q1 = _cache_tensor(q1, cap, 2, idt, "cache1")
    q2 = _cache_tensor(q2, cap, 2, idt, "cache2")
    res = abi.BfsResult()
    while True:
        cap = min(q1.shape[0], q2.shape[0])
        st = getattr(lib.load(), entry)(*args, _ptr(q1), _ptr(q2), cap, _ptr(counters), C.byref(res), _stream())
        if st == abi.ERR_CAPACITY:
            new_cap = max(int(res.required_capacity), BFS_GROWTH * cap)
            keep = int(res.resume_num) if res.resume_step > 0 else 0
            grown = []
            for k, q in enumerate((q1, q2), start=1):
                g = torch.empty((new_cap, 2), dtype=idt, device="cuda")
                if keep and k == res.contacts_in:
                    g[:keep].copy_(q[:keep])  # the pairs the overflowed level still has to expand
                grown.append(g)
            q1, q2 = grown
            continue
        abi.check(st, entry)
        if res.contacts_in == 2:
            q1, q2 = q2, q1
        global _last_bfs_counters
        _last_bfs_counters = (counters, int(levels_hint))  # (tools/attic/dbg_bfs_levels.py reads the per-step counts)
        return res, q1, q2


def _traverse_bfs_single(bvh, start_level, narrow, cache):
    torch = _require_gpu()
    idt = _torch_index(bvh.types.index_type)
    _check_start_level(bvh, start_level, lvt=False)
    if bvh.tree.real_nodes <= 1:
        e = torch.empty((0, 2), dtype=idt, device="cuda")
        return BVHTraversal(start_level, 0, 0, 0, e, e.clone())
    s = bvh.struct()
    cap = C.c_int64()
    lib.call("ibvh_bfs_initial_capacity", C.byref(s), start_level, C.byref(cap))
    res, q1, q2 = _bfs_run("ibvh_traverse_bfs", bvh.types, cap.value, cache, bvh.tree.levels, C.byref(s), start_level, narrow)
    return BVHTraversal(start_level, 0, res.num_checks, res.num_contacts, q1, q2)


def _traverse_bfs_pair(bvh1, bvh2, sl1, sl2, narrow, cache):
    _require_gpu()
    _check_start_level(bvh1, sl1, lvt=False)
    _check_start_level(bvh2, sl2, lvt=False)
    s1, s2 = bvh1.struct(), bvh2.struct()
    cap = C.c_int64()
    lib.call("ibvh_bfs_pair_initial_capacity", C.byref(s1), C.byref(s2), sl1, sl2, C.byref(cap))
    res, q1, q2 = _bfs_run("ibvh_traverse_pair_bfs", bvh1.types, cap.value, cache, bvh1.tree.levels + bvh2.tree.levels,
                           C.byref(s1), C.byref(s2), sl1, sl2, narrow)
    return BVHTraversal(sl1, sl2, res.num_checks, res.num_contacts, q1, q2)


def _traverse_bfs_rays(bvh, p, d, start_level, narrow, cache):
    s = bvh.struct()
    nr = p.shape[0]
    cap = C.c_int64()
    lib.call("ibvh_bfs_rays_initial_capacity", C.byref(s), nr, start_level, C.byref(cap))
    res, q1, q2 = _bfs_run("ibvh_traverse_rays_bfs", bvh.types, cap.value, cache, bvh.tree.levels, C.byref(s), _ptr(p),
                           _ptr(d), nr, start_level, narrow)
    t = BVHTraversal(start_level, 0, res.num_checks, res.num_contacts, q1, q2)
    t._ray_list = "bfs"
    return t


def traverse(bvh, *args, start_level=None, start_level1=None, start_level2=None, narrow=None, cache=None, options=None):
    """traverse(bvh, alg=LVTTraversal(); start_level, narrow, cache, options)
       traverse(bvh1, bvh2, alg=LVTTraversal(); start_level1, start_level2, narrow, cache, options)
    (traverse/traverse.jl:210-233).  Returns a BVHTraversal; `.contacts` is an (m, 2) tensor of 1-based index
    pairs: (min, max) of the user indices for one BVH, (index in bvh1, index in bvh2) for two."""
    bvh2, alg = None, None
    for a in args:
        if isinstance(a, BVH):
            bvh2 = a
        elif isinstance(a, (LVTTraversal, BFSTraversal)):
            alg = a
        else:
            raise ValueError(f"Traversal algorithm not implemented: {a}")  # traverse.jl:217
    alg = alg or LVTTraversal()
    code, fn = _narrow_code(narrow)
    lvt = isinstance(alg, LVTTraversal)
    if bvh2 is None:
        sl = default_start_level(bvh, alg) if start_level is None else int(start_level)
        t = (_traverse_lvt_single if lvt else _traverse_bfs_single)(bvh, sl, code, cache)
    else:
        sl1 = default_start_level(bvh, alg) if start_level1 is None else int(start_level1)
        sl2 = default_start_level(bvh2, alg) if start_level2 is None else int(start_level2)
        t = (_traverse_lvt_pair if lvt else _traverse_bfs_pair)(bvh, bvh2, sl1, sl2, code, cache)
    return _post_filter(t, fn, bvh, bvh2) if fn else t


def traverse_rays(bvh, points, directions, alg=None, start_level=1, narrow=None, cache=None, options=None):
    """traverse_rays(bvh, points, directions, alg=LVTTraversal(); start_level=1, narrow, cache, options)
    (raytrace/raytrace.jl:71-80).  points, directions: (3, N) tensors as in the reference (column i = ray i);
    contacts are (leaf.index, iray).  Rays are converted to the leaf float type (raytrace/lvt:116-125)."""
    torch = _require_gpu()
    alg = alg or LVTTraversal()
    code, fn = _narrow_code(narrow, rays=True)
    if not (points.dim() == 2 and directions.dim() == 2 and points.shape[0] == 3 and directions.shape[0] == 3):
        raise ValueError("size(points, 1) == size(directions, 1) == 3 must hold")
    if points.shape[1] != directions.shape[1]:
        raise ValueError("size(points, 2) == size(directions, 2) must hold")
    lvt = isinstance(alg, LVTTraversal)
    _check_start_level(bvh, start_level, lvt)
    idt = _torch_index(bvh.types.index_type)
    if points.shape[1] == 0:
        e = torch.empty((0, 2), dtype=idt, device="cuda")
        t = BVHTraversal(start_level, 0, 0, 0, e, e.clone())
        t._ray_list = "lvt" if lvt else "bfs"
        return t
    ft = _torch_float(bvh.types.leaf_float)
    p = points.to(device="cuda", dtype=ft).t().contiguous()  # (N, 3) row-major == (3, N) column-major
    d = directions.to(device="cuda", dtype=ft).t().contiguous()
    t = (_traverse_lvt_rays if lvt else _traverse_bfs_rays)(bvh, p, d, start_level, code, cache)
    return _post_filter(t, fn, bvh, rays=(p, d)) if fn else t


# ---------------------------------------------------------------------------------------------
# ray hit lists against the mesh's triangles (ibvh_rays_resolve_triangles; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class RayHits:
    """Per ray: .index (N,) the nearest exactly hit triangle's user index (0 = miss), .t (N,) (+Inf = miss), .uv (N, 2)
    (0, 0 on a miss); .candidate_t (num_contacts,) — t of every candidate that is an exact hit, +Inf otherwise — when
    all_hits was asked for, else None."""

    def __init__(self, index, t, uv, candidate_t=None):
        self.index, self.t, self.uv, self.candidate_t = index, t, uv, candidate_t


def _resolve_enqueue(flt, triangles, p, d, counts, contacts, index, t, uv, cand, flag):
    """One ibvh_rays_resolve_triangles call on the current stream; reads nothing back.  p, d: (N, 3) row-major."""
    lib.call("ibvh_rays_resolve_triangles", flt, _index_code(counts.dtype), _ptr(triangles), triangles.shape[0], _ptr(p), _ptr(d),
             p.shape[0], _ptr(counts), _ptr(contacts), contacts.shape[0], _ptr(index), _ptr(t), _ptr(uv), _ptr(cand), _ptr(flag),
             _stream())


def _check_triangles(triangles, what):
    torch = _torch()
    if not isinstance(triangles, torch.Tensor) or not (
            (triangles.dim() == 2 and triangles.shape[1] == 9) or (triangles.dim() == 3 and tuple(triangles.shape[1:]) == (3, 3))):
        raise ValueError(f"{what}: triangles must be an (n, 9) or (n, 3, 3) tensor (p1 p2 p3 per triangle)")
    if triangles.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: triangles must be float32 or float64, not {triangles.dtype}")
    if not triangles.is_cuda:
        raise ValueError(f"{what}: triangles must live on the GPU (device='cuda')")
    return triangles.reshape(triangles.shape[0], 9).contiguous()


def resolve_triangles(traversal, triangles, points, directions, all_hits=False):
    """The exact ray-triangle test over the candidate list of traverse_rays(..., LVTTraversal()) and the nearest hit per ray
    (include/ibvh.h, ibvh_rays_resolve_triangles: the arithmetic, the tie rule — smallest t, then the earlier candidate —
    and the guards are spelled out there).  `triangles`: the (n, 9) / (n, 3, 3) CUDA tensor the BVH's bounding volumes were
    made from (user index k = row k - 1), float32 or float64: the test runs in ITS dtype.  points, directions: the rays the
    traversal was made with, (3, N) as for traverse_rays.  Returns a RayHits.

    Exact on the candidate list it is given: a grazing hit that the broad phase's rounded slab / sphere test dropped is not
    recovered.  ValueError: a BFS traversal (its list is not grouped by ray), a list of leaf positions or one a callable
    `narrow` filtered (the counts no longer describe it), a wrong dtype, device or shape, and a candidate whose index lies
    outside 1..n (flag bit 1; such candidates count as misses).  Reads traversal.cache1, i.e. the traversal's count, first."""
    torch = _require_gpu()
    kind = getattr(traversal, "_ray_list", None)
    if kind != "lvt":
        why = {"bfs": "a BFS ray traversal's list is not grouped by ray", "positions": "the list holds leaf positions, not triangle numbers",
               None: "not an LVT ray traversal with a device narrow (a filtered list has no counts; traverse() lists hold no rays)"}[kind]
        raise ValueError(f"resolve_triangles: {why}: use traverse_rays(..., LVTTraversal()) with narrow=None or a NARROW_* constant")
    tris = _check_triangles(triangles, "resolve_triangles")
    if not (isinstance(points, torch.Tensor) and isinstance(directions, torch.Tensor) and points.dim() == 2 and
            directions.dim() == 2 and points.shape[0] == 3 and directions.shape[0] == 3):
        raise ValueError("size(points, 1) == size(directions, 1) == 3 must hold")
    if points.shape[1] != directions.shape[1]:
        raise ValueError("size(points, 2) == size(directions, 2) must hold")
    nr = int(points.shape[1])
    contacts = traversal.cache1  # (resolves a pending count: the read a user makes anyway)
    counts = traversal.cache2
    ft, idt = tris.dtype, contacts.dtype
    if nr == 0:
        e = torch.empty(0, dtype=ft, device="cuda")
        return RayHits(torch.empty(0, dtype=idt, device="cuda"), e, torch.empty((0, 2), dtype=ft, device="cuda"), e.clone() if all_hits else None)
    if counts is None or counts.dim() != 1 or counts.shape[0] < nr or counts.dtype != idt or not counts.is_cuda:
        raise ValueError(f"resolve_triangles: the traversal's counts (cache2) do not describe {nr} rays")
    if contacts.dim() != 2 or contacts.shape[1] != 2 or not contacts.is_cuda:
        raise ValueError("resolve_triangles: the traversal's contact list (cache1) must be an (m, 2) CUDA index tensor")
    counts = counts[:nr]  # (a cached counts buffer may be longer than this batch)
    index = torch.empty(nr, dtype=idt, device="cuda")
    t = torch.empty(nr, dtype=ft, device="cuda")
    uv = torch.empty((nr, 2), dtype=ft, device="cuda")
    p = points.to(device="cuda", dtype=ft).t().contiguous()
    d = directions.to(device="cuda", dtype=ft).t().contiguous()
    cand = torch.empty(contacts.shape[0], dtype=ft, device="cuda") if all_hits else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _resolve_enqueue(_float_code(ft), tris, p, d, counts, contacts, index, t, uv, cand, flag)
    raised = int(flag.item())
    if raised & 1:
        raise RuntimeError("resolve_triangles: the contact list is shorter than the traversal's count")
    if raised & 2:
        raise ValueError(f"resolve_triangles: a candidate's index lies outside 1..{tris.shape[0]} (the number of triangles given)")
    return RayHits(index, t, uv, cand[: traversal.num_contacts] if all_hits else None)


def raycast(bvh, triangles, points, directions, **kw):
    """traverse_rays(bvh, points, directions, LVTTraversal(); **kw) followed by resolve_triangles: the nearest exactly hit
    triangle per ray.  `triangles` must be of the BVH's leaf float type (the broad phase ran in it); kw: start_level,
    narrow (None or a NARROW_* constant), cache, all_hits.  Returns (RayHits, the BVHTraversal — reusable as cache=)."""
    tris = _check_triangles(triangles, "raycast")
    if tris.dtype != _torch_float(bvh.types.leaf_float):
        raise ValueError(f"raycast: triangles must be {_torch_float(bvh.types.leaf_float)}, the BVH's leaf float type")
    all_hits = kw.pop("all_hits", False)
    if "alg" in kw and not isinstance(kw["alg"], LVTTraversal):
        raise ValueError("raycast: only LVTTraversal lists are grouped by ray")
    kw.pop("alg", None)
    if callable(kw.get("narrow")):
        raise ValueError("raycast: narrow must be None or a NARROW_* constant (a filtered list has no counts)")
    trav = traverse_rays(bvh, points, directions, LVTTraversal(), **kw)
    return resolve_triangles(trav, tris, points, directions, all_hits=all_hits), trav


# ---------------------------------------------------------------------------------------------
# closest point on the mesh for a batch of query points (ibvh_closest_triangles; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class ClosestPoints:
    """Per query point: .index (N,) the closest triangle's user index (0 = none within max_distance), .distance2 (N,) the
    SQUARED distance (+Inf = none), .point (N, 3) the closest point on that triangle (0, 0, 0 = none)."""

    def __init__(self, index, distance2, point):
        self.index, self.distance2, self.point = index, distance2, point


def _morton_order(p):
    """Permutation that sorts the (N, 3) points along a 30-bit Morton curve through their own bounding box (NaN and
    infinite coordinates land in a corner).  Only the ORDER the device walks the batch in: never the result."""
    torch = _torch()
    x = torch.nan_to_num(p.to(torch.float64), nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = x.amin(dim=0), x.amax(dim=0)
    cell = ((x - lo) / torch.clamp(hi - lo, min=1e-300) * 1023.0).to(torch.int64).clamp_(0, 1023)
    for shift, mask in ((16, 0x30000ff), (8, 0x0300f00f), (4, 0x30c30c3), (2, 0x9249249)):  # split3, morton/default.jl:130-143
        cell = (cell | (cell << shift)) & mask
    return torch.argsort((cell[:, 0] << 2) | (cell[:, 1] << 1) | cell[:, 2])


def _check_points_shape(points, what):
    torch = _torch()
    if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[0] == 3):
        raise ValueError(f"{what}: size(points, 1) == 3 must hold")


def _query_points(points, ft, max_distance, presorted, what):
    """The point queries' common input: the (3, N) CUDA tensor `points` of dtype ft, checked -> the (N, 3) contiguous tensor
    the device walks (in Morton order unless presorted), N, max_distance squared in ft as a byref host scalar (None =
    unbounded) and the permutation applied (None = none)."""
    torch = _torch()
    _check_points_shape(points, what)
    if points.dtype != ft or not points.is_cuda:
        raise ValueError(f"{what}: points must be a {ft} tensor on the GPU (device='cuda')")
    n = int(points.shape[1])
    radius2 = None
    if max_distance is not None:
        npdt = np.float32 if ft == torch.float32 else np.float64
        with np.errstate(over="ignore"):
            m = npdt(max_distance) * npdt(max_distance)
        radius2 = C.byref((C.c_float if ft == torch.float32 else C.c_double)(m))
    p = points.t().contiguous()  # (N, 3) row-major == (3, N) column-major
    order = None if presorted or n == 0 else _morton_order(p)
    return (p if order is None else p[order]), n, radius2, order


def _companion(value, n, ft, what, name, of):
    """`value`, the (3, N) CUDA tensor of dtype ft that goes with the (3, N) points named `of` (a ray's direction, a sphere's
    displacement), checked -> the (N, 3) contiguous tensor"""
    torch = _torch()
    if not (isinstance(value, torch.Tensor) and value.dim() == 2 and tuple(value.shape) == (3, n)):
        raise ValueError(f"{what}: size({name}) == size({of}) == (3, N) must hold")
    if value.dtype != ft or not value.is_cuda:
        raise ValueError(f"{what}: {name} must be a {ft} tensor on the GPU (device='cuda')")
    return value.t().contiguous()


def _unpermute(order, outputs):
    """The outputs' rows back in the caller's order (order: what _query_points returned)."""
    if order is None:
        return outputs
    torch = _torch()
    return tuple(torch.empty_like(x).index_copy_(0, order, x) for x in outputs)


def _check_box_nodes(bvh, what, leaves="leaves"):
    """What every bounded walk needs above the leaves: BBox nodes that hold the leaves' values exactly."""
    t = bvh.types
    if t.node_kind != abi.BBOX:
        raise ValueError(f"{what}: the BVH must have BBox nodes (the exact bound needs boxes that contain the {leaves})")
    if t.leaf_float == abi.F64 and t.node_float == abi.F32:
        raise ValueError(f"{what}: Float32 nodes over Float64 leaves do not contain them exactly")


def _mesh_query_setup(bvh, triangles, what):
    """The mesh queries' common checks: BBox leaves under such nodes, `triangles` of the leaves' float type -> the (n, 9)
    contiguous triangles, the float dtype, the index dtype."""
    if bvh.types.leaf_kind != abi.BBOX:
        raise ValueError(f"{what}: the BVH must have BBox leaves under BBox nodes (the exact bound needs boxes that contain "
                         "their triangles; sphere leaves are not supported)")
    _check_box_nodes(bvh, what, "triangles' boxes")
    tris = _check_triangles(triangles, what)
    ft = _torch_float(bvh.types.leaf_float)
    if tris.dtype != ft:
        raise ValueError(f"{what}: triangles must be {ft}, the BVH's leaf float type")
    return tris, ft, _torch_index(bvh.types.index_type)


def _mesh_query_call(entry, what, bvh, tris, *args):
    """One mesh query on the current stream: entry(bvh, triangles, n, *args, flag, stream) with a fresh flag word, which is
    read back afterwards (a synchronisation) -> the flag word.  Bit 1 of it: a leaf named no row of `tris`."""
    flag = _torch().zeros(1, dtype=_torch().int32, device="cuda")
    lib.call(entry, C.byref(bvh.struct()), _ptr(tris), tris.shape[0], *args, _ptr(flag), _stream())
    word = int(flag.item())
    if word & 2:
        raise ValueError(f"{what}: a leaf's index lies outside 1..{tris.shape[0]} (the number of triangles given)")
    return word


def closest_points(bvh, triangles, points, max_distance=None, presorted=False):
    """For every query point the closest triangle of the mesh `bvh` was built over, the closest point on it and the squared
    distance -> ClosestPoints (include/ibvh.h, ibvh_closest_triangles: the arithmetic, the tie rule — smallest distance, then
    the smaller index — and why pruning loses nothing are spelled out there).  One launch, exact: bit-equal to a brute
    force over all triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  points: (3, N) CUDA tensor of that dtype, as for traverse_rays.
    max_distance: search radius (None = unbounded); it is squared in the triangles' dtype on the host and a triangle
    qualifies iff its squared distance <= that product.  The device walks the batch in Morton order of the points (lanes of
    a wave then share nodes) and the outputs are put back in the caller's order; presorted=True walks it as given.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    tris, ft, idt = _mesh_query_setup(bvh, triangles, "closest_points")
    p, n, radius2, order = _query_points(points, ft, max_distance, presorted, "closest_points")
    index = torch.empty(n, dtype=idt, device="cuda")
    d2 = torch.empty(n, dtype=ft, device="cuda")
    q = torch.empty((n, 3), dtype=ft, device="cuda")
    if n == 0:
        return ClosestPoints(index, d2, q)
    _mesh_query_call("ibvh_closest_triangles", "closest_points", bvh, tris, _ptr(p), n, radius2, _ptr(index), _ptr(d2), _ptr(q))
    return ClosestPoints(*_unpermute(order, (index, d2, q)))


# ---------------------------------------------------------------------------------------------
# k nearest leaves for a batch of query points (ibvh_nearest_leaves; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class NearestLeaves:
    """Per query point, nearest first: .index (N, k) the leaves' user indices, .d2 (N, k) the SQUARED distances to their
    centres.  Slots beyond the answers (fewer than k leaves, or fewer within max_distance, or a NaN point) hold 0 / +Inf."""

    def __init__(self, index, d2):
        self.index, self.d2 = index, d2


def nearest_leaves(bvh, points, k=1, max_distance=None, presorted=False):
    """For every query point the k leaves of `bvh` whose centres are nearest -> NearestLeaves (include/ibvh.h,
    ibvh_nearest_leaves: the arithmetic, the tie rule — smallest distance, then the smaller index — and why pruning loses
    nothing are spelled out there).  One launch, exact: bit-equal to a brute force over all leaves.

    bvh: BSphere or BBox leaves under BBox nodes of the same or a wider float type (refit is fine).  points: (3, N) CUDA
    tensor of the leaves' dtype, as for traverse_rays.  k: 1 .. 16.  max_distance: search radius (None = unbounded); it is
    squared in the leaves' dtype on the host and a leaf qualifies iff its squared centre distance <= that product.  The
    device walks the batch in Morton order of the points (lanes of a wave then share nodes) and the rows are put back in the
    caller's order; presorted=True walks it as given.

    ValueError: sphere nodes, nodes narrower than the leaves, k out of range, a wrong dtype, device or shape."""
    torch = _require_gpu()
    t = bvh.types
    _check_box_nodes(bvh, "nearest_leaves", "leaves' centres")
    if not (isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= abi.NEAREST_MAX_K):
        raise ValueError(f"nearest_leaves: k must be an integer in 1..{abi.NEAREST_MAX_K}")
    ft = _torch_float(t.leaf_float)
    p, n, radius2, order = _query_points(points, ft, max_distance, presorted, "nearest_leaves")
    index = torch.empty((n, k), dtype=_torch_index(t.index_type), device="cuda")
    d2 = torch.empty((n, k), dtype=ft, device="cuda")
    if n == 0:
        return NearestLeaves(index, d2)
    lib.call("ibvh_nearest_leaves", C.byref(bvh.struct()), _ptr(p), n, int(k), radius2, _ptr(index), _ptr(d2), _stream())
    return NearestLeaves(*_unpermute(order, (index, d2)))


# ---------------------------------------------------------------------------------------------
# ray cast: the closest hit or any hit of a batch of rays against the mesh (ibvh_cast_rays; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class RayCast:
    """Per ray: .index (N,) the closest exactly hit triangle's user index (0 = miss), .t (N,) the hit parameter t* (+Inf =
    miss), .uv (N, 2) the barycentric weights of p2, p3 (0, 0 on a miss), .hit (N,) bool = index != 0."""

    ENTRY = ("ibvh_cast_rays", abi.CAST_CLOSEST, abi.CAST_ANY)

    def __init__(self, index, t, uv):
        self.index, self.t, self.uv = index, t, uv

    @property
    def hit(self):
        return self.index != 0


def cast_rays(bvh, triangles, points, directions, t_max=None, any_hit=False, presorted=False):
    """For every ray points[:, i] + t * directions[:, i] the closest exactly hit triangle of the mesh `bvh` was built over
    -> RayCast; with any_hit=True only whether the ray hits anything within its limit -> (N,) bool tensor (a visibility ray:
    the walk ends at its first hit).  One launch (include/ibvh.h, ibvh_cast_rays: the slab test, the exact test — that of
    resolve_triangles —, the clamp t* = max(t, entry of the leaf's box), the tie rule — smallest t*, then the smaller index —
    and why pruning on the best hit so far loses nothing are spelled out there); exact: bit-equal to a brute force over all
    triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  points, directions: (3, N) CUDA tensors of that dtype, as for traverse_rays.
    t_max: None (unbounded), a number, or an (N,) tensor of per-ray limits; a hit needs t* <= t_max (inclusive), a NaN or
    negative limit gives a miss.  The device walks the batch in Morton order of the origins (lanes of a wave then share
    nodes) and the outputs are put back in the caller's order; presorted=True walks it as given.

    Not watertight along shared edges, like resolve_triangles; a ray cast from a surface hits it at t ~ 0.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    tris, ft, idt = _mesh_query_setup(bvh, triangles, "cast_rays")
    p, n, _, order = _query_points(points, ft, None, presorted, "cast_rays")
    d = _companion(directions, n, ft, "cast_rays", "directions", "points")
    lim = None if t_max is None else _per_item(t_max, n, ft, "cast_rays", "t_max")
    return _first_hit(RayCast, "cast_rays", bvh, tris, p, order, (d,), (lim,), ((idt, ()), (ft, ()), (ft, (2,))), any_hit)


# ---- the list queries, sphere_contacts, triangle_contacts, capsule_contacts and box_contacts: one shape of result, one count / scan / write sequence ----
class _ContactLists:
    """Lists of contacts grouped by the item (sphere, query triangle) that owns them, in the caller's order: item i (0-based)
    owns rows offsets[i] : offsets[i + 1] of every per-contact field; .index is the first of those."""

    def __init__(self, offsets, index):
        self.offsets, self.index = offsets, index
        self.counts = offsets[1:] - offsets[:-1]
        self._owner = None

    def _owner_column(self):
        """(M,) the 1-based number of the item each row belongs to, computed when first asked for; None after count_only"""
        if self._owner is None and self.index is not None:
            torch = _torch()
            ids = torch.arange(1, self.counts.shape[0] + 1, dtype=torch.int64, device=self.counts.device)
            self._owner = torch.repeat_interleave(ids, self.counts, output_size=int(self.index.shape[0]))
        return self._owner


def _contact_lists(result, what, bvh, tris, n, walk, tail, outs, count_only):
    """A list query's two launches, a count and a write, around the scan of the counts -> result(offsets, *output columns),
    result(offsets) after count_only.  result.ENTRY: (entry, count mode, write mode); a launch is entry(bvh, triangles, *head,
    n, mode, *tail, counts, offsets, capacity, *outputs, flag, stream).  walk() -> (order, the query's own input tensors in
    walk order — `head` their pointers; order: that permutation, None = none), called once there is something to walk.
    outs: (dtype, trailing shape) per output column.  The total is read on the host; if it is 0 there is no write pass."""
    torch = _torch()
    entry, count_mode, write_mode = result.ENTRY
    empty = lambda m: [torch.empty((m,) + shape, dtype=dt, device="cuda") for dt, shape in outs]
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    if n == 0:
        return result(offsets, *([] if count_only else empty(0)))
    order, inputs = walk()  # (held to the end: the launches read them)
    head = [_ptr(t) for t in inputs]
    walked = torch.empty(n, dtype=torch.int64, device="cuda")
    _mesh_query_call(entry, what, bvh, tris, *head, n, count_mode, *tail, _ptr(walked), None, 0, *[None] * len(outs))
    # the counts back in the caller's order, scanned there: an item's rows then follow its predecessor's in that order
    torch.cumsum(_unpermute(order, (walked,))[0], dim=0, out=offsets[1:])
    if count_only:
        return result(offsets)
    total = int(offsets[-1].item())  # the one read between the passes
    columns = empty(total)
    if total > 0:
        first = offsets[:-1] if order is None else offsets[:-1][order]  # ... gathered back into walk order
        word = _mesh_query_call(entry, what, bvh, tris, *head, n, write_mode, *tail, None, _ptr(first), total, *map(_ptr, columns))
        if word & 4:
            raise RuntimeError(f"{what}: the write pass found more contacts than the count pass (inputs changed between them?)")
    return result(offsets, *columns)


def _first_hit(result, what, bvh, tris, p, order, head, tail, outs, any_hit):
    """A first-hit query's one launch -> result(*closest outputs), with any_hit the (N,) bool mask.  result.ENTRY: (entry,
    closest mode, any-hit mode); the launch is entry(bvh, [triangles, n,] p, *head, N, *tail, mode, *closest outputs, the
    any-hit byte, ...): through _mesh_query_call over a mesh, straight over a cloud (tris None).  p: the (N, 3) points in walk
    order; order: that permutation (None = none), which the other per-item tensors, head and tail (None = absent), are put in
    here.  outs: (dtype, trailing shape) per closest output.  No items: no launch."""
    torch = _torch()
    entry, closest, any_mode = result.ENTRY
    n = int(p.shape[0])
    head, tail = ([x if order is None or x is None else x[order] for x in xs] for xs in (head, tail))  # (held to the end)
    made = [torch.empty((n,) + shape, dtype=dt, device="cuda") for dt, shape in (((torch.uint8, ()),) if any_hit else outs)]
    slots = [None] * len(outs) + made if any_hit else made + [None]
    if n > 0:
        args = [_ptr(x) for x in [p] + head] + [n] + [_ptr(x) for x in tail] + [any_mode if any_hit else closest] + [_ptr(o) for o in slots]
        if tris is None:
            lib.call(entry, C.byref(bvh.struct()), *args, _stream())
        else:
            _mesh_query_call(entry, what, bvh, tris, *args)
    made = _unpermute(order, tuple(made))
    return made[0] != 0 if any_hit else result(*made)


# ---------------------------------------------------------------------------------------------
# sphere-vs-mesh contacts: every triangle within each sphere's radius (ibvh_sphere_contacts; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class SphereContacts(_ContactLists):
    """The contacts of N spheres with a mesh, M in all, grouped by sphere in the caller's order and, within a sphere, in the
    order of the triangles' leaves in the BVH: sphere s (0-based) owns rows offsets[s] : offsets[s + 1].
    .offsets (N + 1,) int64, .counts (N,) int64; per contact .index (M,) the triangle's user index, .distance2 (M,) the
    SQUARED distance, .point (M, 3) the closest point on the triangle, .region (M,) uint8 the feature that point lies on
    (0 vertex p1, 1 vertex p2, 2 edge p1p2, 3 vertex p3, 4 edge p1p3, 5 edge p2p3, 6 face) and .sphere (M,) the 1-based
    number of the sphere the row belongs to (computed when first asked for).  After count_only=True the per-contact
    fields are None."""

    def __init__(self, offsets, index=None, distance2=None, point=None, region=None):
        super().__init__(offsets, index)
        self.distance2, self.point, self.region = distance2, point, region

    sphere = property(_ContactLists._owner_column)
    ENTRY = ("ibvh_sphere_contacts", abi.SPHERES_COUNT, abi.SPHERES_WRITE)


def sphere_contacts(bvh, triangles, centers, radii, count_only=False, presorted=False):
    """For every sphere ALL triangles of the mesh `bvh` was built over that lie within its radius of its centre, with the
    squared distance, the closest point and the feature touched -> SphereContacts (include/ibvh.h, ibvh_sphere_contacts: the
    arithmetic — that of closest_points —, the order and why pruning loses nothing are spelled out there).  Two launches, a
    count and a write, around a scan of the counts here; exact: bit-equal to a brute force over all triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  centers: (3, N) CUDA tensor of that dtype, as for traverse_rays.  radii: an
    (N,) CUDA tensor of that dtype, or one number for all (a radius search around points).  A triangle is a contact iff its
    squared distance <= r * r, squared in that dtype; a negative or NaN radius and a NaN centre touch nothing.
    count_only=True stops after the first pass.  The device walks the batch in Morton order of the centres (lanes of a wave
    then share nodes) and writes each sphere's rows where the caller's order wants them; presorted=True walks it as given.
    The total is read on the host between the passes, as in traverse.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape of triangles, centers
    or radii, and a leaf whose index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "sphere_contacts"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    p, n, _, order = _query_points(centers, ft, None, presorted, what)
    r = _per_item(radii, n, ft, what, "radii")
    walk = lambda: (order, (p, r if order is None else r[order]))
    return _contact_lists(SphereContacts, what, bvh, tris, n, walk, tail=(),
                          outs=((idt, ()), (ft, ()), (ft, (3,)), (torch.uint8, ())), count_only=count_only)


# ---------------------------------------------------------------------------------------------
# swept spheres: the first time of contact of each moving sphere with the mesh (ibvh_sweep_spheres; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class SphereSweep:
    """Per moving sphere: .index (N,) the first triangle it touches, by user index (0 = miss), .t (N,) the time of contact t*
    (+Inf = miss; 0 = touching at the start), .point (N, 3) the point of the triangle it touches (0 on a miss), .feature (N,)
    uint8 the feature that point lies on (0 vertex p1, 1 vertex p2, 2 edge p1p2, 3 vertex p3, 4 edge p1p3, 5 edge p2p3,
    6 face; 0 on a miss), .hit (N,) bool = index != 0."""

    ENTRY = ("ibvh_sweep_spheres", abi.SWEEP_CLOSEST, abi.SWEEP_ANY)

    def __init__(self, index, t, point, feature):
        self.index, self.t, self.point, self.feature = index, t, point, feature

    @property
    def hit(self):
        return self.index != 0


def _per_item(value, n, ft, what, name):
    """`value`, a number for all or an (N,) CUDA tensor of dtype ft -> the (N,) contiguous tensor"""
    torch = _torch()
    if isinstance(value, torch.Tensor):
        if tuple(value.shape) == (n,) and value.dtype == ft and value.is_cuda:
            return value.contiguous()
    elif isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool):
        return torch.full((n,), float(value), dtype=ft, device="cuda")
    raise ValueError(f"{what}: {name} must be a number or an (N,) {ft} tensor on the GPU")


def sweep_spheres(bvh, triangles, centers, displacements, radii, t_max=None, any_hit=False, presorted=False):
    """For every sphere of radius radii[i] whose centre moves along centers[:, i] + t * displacements[:, i] the first
    triangle of the mesh `bvh` was built over that it touches, when, where and on which feature -> SphereSweep; with
    any_hit=True only whether it touches anything within its limit -> (N,) bool tensor (the walk ends at its first hit).
    Continuous collision detection: no tunnelling through thin walls, grazing contacts included.  One launch (include/ibvh.h,
    ibvh_sweep_spheres: the start position — the evaluation of sphere_contacts —, the seven candidates — the face by the exact
    test of resolve_triangles, three edge cylinders, three vertex spheres —, the clamp t* = max(t, entry of the leaf's box
    grown by the radius), the tie rule — smallest t*, then the smaller index — and why pruning on the best hit so far loses
    nothing are spelled out there); exact: bit-equal to a brute force over all triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  centers, displacements: (3, N) CUDA tensors of that dtype, as for traverse_rays.
    radii: an (N,) CUDA tensor of that dtype, or one number for all; a negative or NaN radius touches nothing.  t_max: None
    (unbounded), a number — 1 = the whole displacement —, or an (N,) tensor of per-sphere limits; a hit needs t* <= t_max
    (inclusive), a NaN or negative limit gives a miss.  A sphere that touches the mesh where it starts reports t = 0 and the
    closest point of the touched triangle with the smallest index.  The device walks the batch in Morton order of the
    centres (lanes of a wave then share nodes) and the outputs are put back in the caller's order; presorted=True walks it
    as given.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "sweep_spheres"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    p, n, _, order = _query_points(centers, ft, None, presorted, what)
    d = _companion(displacements, n, ft, what, "displacements", "centers")
    r = _per_item(radii, n, ft, what, "radii")
    lim = None if t_max is None else _per_item(t_max, n, ft, what, "t_max")
    return _first_hit(SphereSweep, what, bvh, tris, p, order, (d, r), (lim,),
                      ((idt, ()), (ft, ()), (ft, (3,)), (torch.uint8, ())), any_hit)


# ---------------------------------------------------------------------------------------------
# rays and swept spheres against a sphere cloud: the first leaf hit (ibvh_cast_spheres; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class SphereCast:
    """Per query: .index (N,) the first leaf sphere it touches, by user index (0 = miss), .t (N,) the time of contact t* in
    units of the displacement (+Inf = miss; 0 = touching at the start), .hit (N,) bool = index != 0."""

    ENTRY = ("ibvh_cast_spheres", abi.SPHERECAST_CLOSEST, abi.SPHERECAST_ANY)

    def __init__(self, index, t):
        self.index, self.t = index, t

    @property
    def hit(self):
        return self.index != 0

    def positions(self, points, displacements):
        """(3, N): where each query's centre is at contact, points + t * displacements; NaN columns for the misses.  Torch."""
        torch = _torch()
        t = torch.where(self.hit, self.t, torch.zeros_like(self.t))
        x = points + t[None, :] * displacements
        return torch.where(self.hit[None, :], x, torch.full_like(x, float("nan")))

    def normals(self, spheres, points, displacements):
        """(3, N): the unit vector from the hit leaf's centre to the query's centre at contact — the contact normal, which
        points from the leaf towards the query —, gathered from `spheres`, the (n, 4) tensor the BVH was built from (user
        index k = row k - 1); NaN columns for the misses and where the two centres coincide.  Torch."""
        torch = _torch()
        rows = (self.index.to(torch.int64) - 1).clamp_(min=0)
        v = self.positions(points, displacements) - spheres[rows, :3].t()
        return v / torch.linalg.vector_norm(v, dim=0, keepdim=True)


def cast_spheres(bvh, points, displacements, radii=None, t_max=None, skip=None, any_hit=False, presorted=False):
    """For every query sphere of radius radii[i] whose centre moves along points[:, i] + t * displacements[:, i] (radius 0: a
    ray) the first leaf sphere of the cloud `bvh` was built over that it touches and when -> SphereCast; with any_hit=True
    only whether it touches anything within its limit -> (N,) bool tensor (the walk ends at its first hit).  One launch
    (include/ibvh.h, ibvh_cast_spheres: the touching test — the bits of the pair traversals' iscontact —, the quadratic, the
    clamps t* = max(t, entry of the leaf's own box grown by the radius, entry of the stored box directly above the leaf grown
    likewise), the tie rule — smallest t*, then the smaller index — and why pruning on the best hit so far loses nothing are
    spelled out there); exact: bit-equal to a brute force over all leaves.

    bvh: BSphere leaves under BBox nodes of the same or a wider float type (refit is fine).  points, displacements: (3, N) CUDA
    tensors of the leaves' dtype, as for traverse_rays; t = 1 is the end of the displacement.  radii: None (rays), one number
    for all, or an (N,) CUDA tensor of that dtype; a negative or NaN radius touches nothing.  t_max: None (unbounded), a
    number — 1 = the whole displacement —, or an (N,) tensor of per-query limits; a hit needs t* <= t_max (inclusive), a NaN
    or negative limit gives a miss.  skip: None, or an (N,) integer CUDA tensor, per query the user index of one leaf to
    ignore (0 = none): a particle of the cloud swept against the cloud skips itself.  The device walks the batch in Morton
    order of the points (lanes of a wave then share nodes) and the outputs are put back in the caller's order;
    presorted=True walks it as given.

    ValueError: box leaves, sphere nodes, nodes narrower than the leaves, a wrong dtype, device or shape."""
    torch = _require_gpu()
    what = "cast_spheres"
    t = bvh.types
    if t.leaf_kind != abi.BSPHERE:
        raise ValueError(f"{what}: the BVH must have BSphere leaves (cast_rays and sweep_spheres query a mesh's BBox leaves)")
    _check_box_nodes(bvh, what, "leaves' boxes")
    ft, idt = _torch_float(t.leaf_float), _torch_index(t.index_type)
    p, n, _, order = _query_points(points, ft, None, presorted, what)
    d = _companion(displacements, n, ft, what, "displacements", "points")
    r = None if radii is None else _per_item(radii, n, ft, what, "radii")
    lim = None if t_max is None else _per_item(t_max, n, ft, what, "t_max")
    if skip is not None:
        if not (isinstance(skip, torch.Tensor) and tuple(skip.shape) == (n,) and skip.is_cuda
                and skip.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"{what}: skip must be an (N,) integer tensor on the GPU")
        skip = skip.to(idt).contiguous()
    return _first_hit(SphereCast, what, bvh, None, p, order, (d, r), (lim, skip), ((idt, ()), (ft, ())), any_hit)


# ---------------------------------------------------------------------------------------------
# triangle-vs-mesh contacts: every mesh triangle each query triangle cuts (ibvh_triangle_contacts; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class TriangleContacts(_ContactLists):
    """The contacts of N query triangles with a mesh, M in all, grouped by query in the caller's order and, within a query,
    in the order of the triangles' leaves in the BVH: query i (0-based) owns rows offsets[i] : offsets[i + 1].
    .offsets (N + 1,) int64, .counts (N,) int64; per contact .index (M,) the mesh triangle's user index, .mask (M,) uint8 the
    edge tests that found it (bits 0-2: the query's edges ab, bc, ca against the mesh triangle; bits 3-5: the mesh triangle's
    edges p1p2, p2p3, p3p1 against the query), .points (M, 2, 3) the two ends of the cut (the points of the lowest and the
    highest set bit) and .query (M,) the 1-based number of the query the row belongs to (computed when first asked for).
    After count_only=True the per-contact fields are None."""

    def __init__(self, offsets, index=None, mask=None, points=None):
        super().__init__(offsets, index)
        self.mask, self.points = mask, points

    query = property(_ContactLists._owner_column)
    ENTRY = ("ibvh_triangle_contacts", abi.TRIS_COUNT, abi.TRIS_WRITE)


def triangle_contacts(bvh, triangles, queries, query_ids=None, skip_shared_vertices=False, count_only=False, presorted=False):
    """For every query triangle ALL triangles of the mesh `bvh` was built over that it cuts, with the edge tests that found
    each and the two ends of the cut -> TriangleContacts (include/ibvh.h, ibvh_triangle_contacts: the six edge-against-triangle
    tests — the exact test of resolve_triangles on each edge, t <= 1 —, the box clause, the order and why pruning loses
    nothing are spelled out there).  Two launches, a count and a write, around a scan of the counts here; exact: bit-equal
    to a brute force over all triangles.  Coplanar and touching pairs are decided by rounding (exactly coplanar arithmetic
    finds no contact).

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  queries: (N, 9) / (N, 3, 3) CUDA tensor of that dtype.  query_ids: None, or an
    (N,) CUDA tensor of the BVH's index dtype: query i then only meets triangles whose index > query_ids[i].
    skip_shared_vertices=True drops every pair with an equal vertex.  A query with a NaN coordinate touches nothing.
    count_only=True stops after the first pass.  The device walks the batch in Morton order of the queries' first vertices
    (lanes of a wave then share nodes) and writes each query's rows where the caller's order wants them; presorted=True
    walks it as given.  The total is read on the host between the passes, as in traverse.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape of triangles, queries
    or query_ids, and a leaf whose index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "triangle_contacts"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    if not isinstance(queries, torch.Tensor) or not (
            (queries.dim() == 2 and queries.shape[1] == 9) or (queries.dim() == 3 and tuple(queries.shape[1:]) == (3, 3))):
        raise ValueError(f"{what}: queries must be an (N, 9) or (N, 3, 3) tensor (a b c per triangle)")
    if queries.dtype != ft or not queries.is_cuda:
        raise ValueError(f"{what}: queries must be a {ft} tensor on the GPU (device='cuda')")
    q = queries.reshape(queries.shape[0], 9).contiguous()
    n = int(q.shape[0])
    ids = None
    if query_ids is not None:
        if not isinstance(query_ids, torch.Tensor) or tuple(query_ids.shape) != (n,) or query_ids.dtype != idt or not query_ids.is_cuda:
            raise ValueError(f"{what}: query_ids must be None or an (N,) {idt} tensor on the GPU")
        ids = query_ids.contiguous()
    skip = abi.TRIS_SKIP_SHARED_VERTEX if skip_shared_vertices else 0
    def walk():
        order = None if presorted else _morton_order(q[:, :3])
        if order is None:
            return None, (q, ids)
        return order, (q[order], None if ids is None else ids[order])
    return _contact_lists(TriangleContacts, what, bvh, tris, n, walk, tail=(skip,),
                          outs=((idt, ()), (torch.uint8, ()), (ft, (2, 3))), count_only=count_only)


def self_intersections(bvh, triangles, count_only=False):
    """The pairs of triangles of ONE mesh that cut each other -> TriangleContacts with the mesh's triangles as the queries:
    triangle_contacts(bvh, triangles, triangles, query_ids=1..n, skip_shared_vertices=True).  Each unordered pair appears
    once, under its lower index (.query) with the higher one as .index; never a triangle with itself or with a neighbour
    that shares a vertex with it."""
    torch = _require_gpu()
    tris, _, idt = _mesh_query_setup(bvh, triangles, "self_intersections")
    ids = torch.arange(1, tris.shape[0] + 1, dtype=idt, device="cuda")
    return triangle_contacts(bvh, tris, tris, query_ids=ids, skip_shared_vertices=True, count_only=count_only)


# ---------------------------------------------------------------------------------------------
# triangle-vs-mesh distance: the closest mesh triangle per query triangle (ibvh_triangle_distances; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class TriangleDistances:
    """Per query triangle: .index (N,) the closest mesh triangle's user index (0 = none), .d2 (N,) the SQUARED distance (+Inf
    = none; 0 = the two cut each other), .point_query (N, 3) the closest point on the query triangle, .point_mesh (N, 3) the
    closest point on the mesh triangle (zeros = none), .kind (N,) uint8 the deciding candidate: 0-2 the query's vertex a, b,
    c against the mesh triangle, 3-5 the mesh triangle's vertex p1, p2, p3 against the query, 6 + 3 i + j the query's edge i
    (ab, bc, ca) against the mesh triangle's edge j (p1p2, p2p3, p3p1), 15 an edge of one cuts the other (0 = none)."""

    def __init__(self, index, d2, point_query, point_mesh, kind):
        self.index, self.d2, self.point_query, self.point_mesh, self.kind = index, d2, point_query, point_mesh, kind


class MeshDistance:
    """The one closest pair of two meshes: .distance (float; inf = none), .query the 1-based position of the query triangle
    (0 = none), .index the mesh triangle's user index (0 = none), .point_query and .point_mesh (3,) tensors."""

    def __init__(self, distance, query, index, point_query, point_mesh):
        self.distance, self.query, self.index, self.point_query, self.point_mesh = distance, query, index, point_query, point_mesh


def triangle_distances(bvh, triangles, queries, max_distance=None, skip_shared_vertices=False, presorted=False):
    """For every query triangle the closest triangle of the mesh `bvh` was built over, the squared distance, the closest
    point on each of the two and the deciding pair of features -> TriangleDistances (include/ibvh.h, ibvh_triangle_distances:
    the cut rule — the six edge tests of triangle_contacts give distance 0 —, the fifteen candidates — six vertex-against-
    triangle evaluations of closest_points and nine edge pairs —, the tie rule — smallest distance, then the smaller index —
    and why pruning on the gap between boxes loses nothing are spelled out there).  One launch, exact: bit-equal to a brute
    force over all pairs.  Coplanar and touching pairs are decided by rounding.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  queries: (N, 9) / (N, 3, 3) CUDA tensor of that dtype.  max_distance: search
    radius (None = unbounded); it is squared in the triangles' dtype on the host and a triangle qualifies iff its squared
    distance <= that product.  skip_shared_vertices=True ignores every mesh triangle with a vertex equal to one of the
    query's.  A query with a NaN coordinate has no answer.  The device walks the batch in Morton order of the queries'
    centroids (lanes of a wave then share nodes) and the outputs are put back in the caller's order; presorted=True walks
    it as given.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "triangle_distances"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    if not isinstance(queries, torch.Tensor) or not (
            (queries.dim() == 2 and queries.shape[1] == 9) or (queries.dim() == 3 and tuple(queries.shape[1:]) == (3, 3))):
        raise ValueError(f"{what}: queries must be an (N, 9) or (N, 3, 3) tensor (a b c per triangle)")
    if queries.dtype != ft or not queries.is_cuda:
        raise ValueError(f"{what}: queries must be a {ft} tensor on the GPU (device='cuda')")
    q = queries.reshape(queries.shape[0], 9).contiguous()
    n = int(q.shape[0])
    radius2 = None
    if max_distance is not None:
        npdt = np.float32 if ft == torch.float32 else np.float64
        with np.errstate(over="ignore"):
            m = npdt(max_distance) * npdt(max_distance)
        radius2 = C.byref((C.c_float if ft == torch.float32 else C.c_double)(m))
    outs = (torch.empty(n, dtype=idt, device="cuda"), torch.empty(n, dtype=ft, device="cuda"),
            torch.empty((n, 3), dtype=ft, device="cuda"), torch.empty((n, 3), dtype=ft, device="cuda"),
            torch.empty(n, dtype=torch.uint8, device="cuda"))
    if n == 0:
        return TriangleDistances(*outs)
    order = None if presorted else _morton_order((q[:, 0:3] + q[:, 3:6] + q[:, 6:9]) / 3)
    skip = abi.TRIS_SKIP_SHARED_VERTEX if skip_shared_vertices else 0
    walked = q if order is None else q[order]   # (held until the call returns: the launch reads it)
    _mesh_query_call("ibvh_triangle_distances", what, bvh, tris, _ptr(walked), n, skip, radius2, *[_ptr(o) for o in outs])
    return TriangleDistances(*_unpermute(order, outs))


def mesh_distance(bvh, triangles, queries, max_distance=None, skip_shared_vertices=False, presorted=False):
    """The one closest pair between the query triangles and the mesh `bvh` was built over -> MeshDistance:
    triangle_distances, reduced on the device to its smallest d2 — among equal ones the lowest query position — and read
    back once.  distance inf and query = index = 0 when no pair qualifies."""
    torch = _torch()
    td = triangle_distances(bvh, triangles, queries, max_distance, skip_shared_vertices, presorted)
    n = int(td.d2.shape[0])
    if n == 0:
        zero = torch.zeros(3, dtype=td.d2.dtype, device="cuda")
        return MeshDistance(float("inf"), 0, 0, zero, zero.clone())
    smallest = td.d2.min()
    pos = torch.where(td.d2 == smallest, torch.arange(n, device="cuda"), n).min()   # the first of the smallest
    index, d2 = int(td.index[pos].item()), float(td.d2[pos].item())
    return MeshDistance(float(np.sqrt(d2)), int(pos.item()) + 1 if index else 0, index, td.point_query[pos], td.point_mesh[pos])


def self_clearance(bvh, triangles, max_distance=None):
    """How close each triangle of ONE mesh comes to the rest of it -> TriangleDistances with the mesh's triangles as the
    queries: triangle_distances(bvh, triangles, triangles, skip_shared_vertices=True).  No triangle reports itself or a
    neighbour that shares a vertex with it; d2 = 0 marks a self-intersection, a small d2 one about to happen."""
    return triangle_distances(bvh, triangles, triangles, max_distance=max_distance, skip_shared_vertices=True)


# ---------------------------------------------------------------------------------------------
# capsules and segments against a mesh (ibvh_capsule_contacts, ibvh_segment_distances; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class CapsuleContacts(_ContactLists):
    """The contacts of N capsules with a mesh, M in all, grouped by capsule in the caller's order and, within a capsule, in
    the order of the triangles' leaves in the BVH: capsule s (0-based) owns rows offsets[s] : offsets[s + 1].
    .offsets (N + 1,) int64, .counts (N,) int64; per contact .index (M,) the triangle's user index, .distance2 (M,) the
    SQUARED distance between segment and triangle (0 = the segment crosses it), .point_segment (M, 3) the closest point on
    the segment, .point_mesh (M, 3) the closest point on the triangle, .kind (M,) uint8 the rule that decided (0, 1 the end
    a, b against the triangle; 2, 3, 4 the segment against the edge p1p2, p2p3, p3p1; 5 the segment crosses the triangle)
    and .capsule (M,) the 1-based number of the capsule the row belongs to (computed when first asked for).  After
    count_only=True the per-contact fields are None."""

    def __init__(self, offsets, index=None, distance2=None, point_segment=None, point_mesh=None, kind=None):
        super().__init__(offsets, index)
        self.distance2, self.point_segment, self.point_mesh, self.kind = distance2, point_segment, point_mesh, kind

    capsule = property(_ContactLists._owner_column)
    ENTRY = ("ibvh_capsule_contacts", abi.CAPSULES_COUNT, abi.CAPSULES_WRITE)


class SegmentDistances:
    """Per segment: .index (N,) the closest mesh triangle's user index (0 = none), .d2 (N,) the SQUARED distance (+Inf = none;
    0 = the segment crosses it), .point_segment (N, 3) the closest point on the segment, .point_mesh (N, 3) the closest point
    on the triangle (zeros = none), .kind (N,) uint8 the rule that decided, as in CapsuleContacts (0 = none)."""

    def __init__(self, index, d2, point_segment, point_mesh, kind):
        self.index, self.d2, self.point_segment, self.point_mesh, self.kind = index, d2, point_segment, point_mesh, kind


def _query_segments(starts, ends, ft, presorted, what):
    """The segment queries' common input: the (3, N) CUDA tensors `starts` and `ends` of dtype ft, checked -> the two (N, 3)
    contiguous tensors, N, and the Morton order of the midpoints (None: presorted, or nothing to sort)."""
    torch = _torch()
    for name, x in (("starts", starts), ("ends", ends)):
        if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[0] == 3):
            raise ValueError(f"{what}: size({name}, 1) == 3 must hold")
        if x.dtype != ft or not x.is_cuda:
            raise ValueError(f"{what}: {name} must be a {ft} tensor on the GPU (device='cuda')")
    if tuple(starts.shape) != tuple(ends.shape):
        raise ValueError(f"{what}: size(starts) == size(ends) == (3, N) must hold")
    a, b = starts.t().contiguous(), ends.t().contiguous()  # (N, 3) row-major == (3, N) column-major
    n = int(a.shape[0])
    order = None if presorted or n == 0 else _morton_order(0.5 * a.to(torch.float64) + 0.5 * b.to(torch.float64))
    return a, b, n, order


def capsule_contacts(bvh, triangles, starts, ends, radii, count_only=False, presorted=False):
    """For every capsule — the segment starts[:, i] -> ends[:, i] with the radius radii[i] — ALL triangles of the mesh `bvh`
    was built over that lie within the radius of the segment, with the squared distance, the closest point on the segment
    and on the triangle and the rule that decided -> CapsuleContacts (include/ibvh.h, ibvh_capsule_contacts: the segment-
    triangle evaluation — the exact test of resolve_triangles where the segment crosses, else the two ends by the
    evaluation of closest_points and the three edges by that of triangle_distances —, the slab clause, the order and why
    pruning loses nothing are spelled out there).  Two launches, a count and a write, around a scan of the counts here;
    exact: bit-equal to a brute force over all triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  starts, ends: (3, N) CUDA tensors of that dtype, like the centers of
    sphere_contacts.  radii: an (N,) CUDA tensor of that dtype, or one number for all.  A triangle is a contact iff its
    squared distance <= r * r, squared in that dtype; a negative or NaN radius and a NaN in a segment touch nothing; a
    segment of length zero is a sphere.  count_only=True stops after the first pass.  The device walks the batch in Morton
    order of the segments' midpoints (lanes of a wave then share nodes) and writes each capsule's rows where the caller's
    order wants them; presorted=True walks it as given.  The total is read on the host between the passes, as in traverse.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "capsule_contacts"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    a, b, n, order = _query_segments(starts, ends, ft, presorted, what)
    r = _per_item(radii, n, ft, what, "radii")
    walk = lambda: (order, (a, b, r) if order is None else (a[order], b[order], r[order]))
    return _contact_lists(CapsuleContacts, what, bvh, tris, n, walk, tail=(),
                          outs=((idt, ()), (ft, ()), (ft, (3,)), (ft, (3,)), (torch.uint8, ())), count_only=count_only)


def segment_distances(bvh, triangles, starts, ends, max_distance=None, presorted=False):
    """For every segment starts[:, i] -> ends[:, i] the closest triangle of the mesh `bvh` was built over, the squared
    distance, the closest point on the segment and on the triangle and the rule that decided -> SegmentDistances
    (include/ibvh.h, ibvh_segment_distances: the evaluation of capsule_contacts, the tie rule — smallest distance, then the
    smaller index — and why pruning on the gap between boxes loses nothing are spelled out there).  One launch, exact:
    bit-equal to a brute force over all triangles.

    bvh, triangles, starts, ends: as for capsule_contacts.  max_distance: search radius (None = unbounded); it is squared
    in the triangles' dtype on the host and a triangle qualifies iff its squared distance <= that product.  A segment with
    a NaN coordinate has no answer.  The device walks the batch in Morton order of the segments' midpoints and the outputs
    are put back in the caller's order; presorted=True walks it as given.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "segment_distances"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    a, b, n, order = _query_segments(starts, ends, ft, presorted, what)
    radius2 = None
    if max_distance is not None:
        npdt = np.float32 if ft == torch.float32 else np.float64
        with np.errstate(over="ignore"):
            m = npdt(max_distance) * npdt(max_distance)
        radius2 = C.byref((C.c_float if ft == torch.float32 else C.c_double)(m))
    outs = (torch.empty(n, dtype=idt, device="cuda"), torch.empty(n, dtype=ft, device="cuda"),
            torch.empty((n, 3), dtype=ft, device="cuda"), torch.empty((n, 3), dtype=ft, device="cuda"),
            torch.empty(n, dtype=torch.uint8, device="cuda"))
    if n == 0:
        return SegmentDistances(*outs)
    if order is not None:
        a, b = a[order], b[order]   # (held until the call returns: the launch reads them)
    _mesh_query_call("ibvh_segment_distances", what, bvh, tris, _ptr(a), _ptr(b), n, radius2, *[_ptr(o) for o in outs])
    return SegmentDistances(*_unpermute(order, outs))


# ---------------------------------------------------------------------------------------------
# boxes against a mesh (ibvh_box_contacts; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class BoxContacts(_ContactLists):
    """The contacts of N boxes with a mesh, M in all, grouped by box in the caller's order and, within a box, in the order
    of the triangles' leaves in the BVH: box s (0-based) owns rows offsets[s] : offsets[s + 1].
    .offsets (N + 1,) int64, .counts (N,) int64; per contact .index (M,) the triangle's user index, .inside (M,) uint8 the
    vertices the box holds (bit 0, 1, 2 = p1, p2, p3; 7 = the triangle lies wholly inside, 0 = the box cuts it without
    holding a vertex) and .box (M,) the 1-based number of the box the row belongs to (computed when first asked for).
    After count_only=True the per-contact fields are None."""

    def __init__(self, offsets, index=None, inside=None):
        super().__init__(offsets, index)
        self.inside = inside

    box = property(_ContactLists._owner_column)
    ENTRY = ("ibvh_box_contacts", abi.BOXES_COUNT, abi.BOXES_WRITE)


def _half_extents(value, n, ft, what):
    """`value` — one number or three numbers for all boxes, or a (3, N) CUDA tensor of dtype ft -> the (N, 3) contiguous tensor"""
    torch = _torch()
    number = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
    if isinstance(value, torch.Tensor):
        if tuple(value.shape) == (3, n) and value.dtype == ft and value.is_cuda:
            return value.t().contiguous()
    elif number(value):
        return torch.full((n, 3), float(value), dtype=ft, device="cuda")
    elif isinstance(value, (tuple, list)) and len(value) == 3 and all(number(x) for x in value):
        return torch.tensor([float(x) for x in value], dtype=ft, device="cuda").repeat(n, 1)
    raise ValueError(f"{what}: half_extents must be a number, three numbers or a (3, N) {ft} tensor on the GPU")


def box_contacts(bvh, triangles, centers, half_extents, rotations=None, count_only=False, presorted=False):
    """For every box — the centre centers[:, i], the half extents half_extents[:, i] along its own axes and, optionally, the
    rotation rotations[i], whose ROWS are those axes in world coordinates — ALL triangles of the mesh `bvh` was built over
    that the box overlaps, and which of their vertices it holds -> BoxContacts (include/ibvh.h, ibvh_box_contacts: the hull,
    the box clause, the 13 separating axes in their operation order, the order and why pruning loses nothing are spelled
    out there).  Two launches, a count and a write, around a scan of the counts here; exact: bit-equal to a brute force
    over all triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  centers: (3, N) CUDA tensor of that dtype, like the centers of
    sphere_contacts.  half_extents: a (3, N) CUDA tensor of that dtype, or one number, or three numbers for all boxes.
    rotations: an (N, 3, 3) CUDA tensor of that dtype, assumed orthonormal (not checked), or None: axis-aligned boxes, the
    identity in the same arithmetic.  A half extent that is negative or NaN and a NaN or an infinity in a centre or a
    rotation touch nothing; a half extent of zero is valid (a plate, a segment, a point).  count_only=True stops after the
    first pass.  The device walks the batch in Morton order of the centres (lanes of a wave then share nodes) and writes
    each box's rows where the caller's order wants them; presorted=True walks it as given.  The total is read on the host
    between the passes, as in traverse.

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, and a leaf whose
    index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    what = "box_contacts"
    tris, ft, idt = _mesh_query_setup(bvh, triangles, what)
    c, n, _, order = _query_points(centers, ft, None, presorted, what)
    h = _half_extents(half_extents, n, ft, what)
    r = None
    if rotations is not None:
        if not (isinstance(rotations, torch.Tensor) and tuple(rotations.shape) == (n, 3, 3) and rotations.dtype == ft and rotations.is_cuda):
            raise ValueError(f"{what}: rotations must be None or an (N, 3, 3) {ft} tensor on the GPU")
        r = rotations.contiguous()
    walk = lambda: (order, (c, h, r) if order is None else (c, h[order], None if r is None else r[order]))
    return _contact_lists(BoxContacts, what, bvh, tris, n, walk, tail=(), outs=((idt, ()), (torch.uint8, ())), count_only=count_only)


def voxelize(bvh, triangles, origin, spacing, shape):
    """The cells of a regular grid that the mesh `bvh` was built over passes through -> bool CUDA tensor of `shape` (nx, ny,
    nz): cell (i, j, k) is the axis-aligned box with the centre origin + (i + 0.5, j + 0.5, k + 0.5) * spacing and the half
    extent spacing / 2, both computed in the BVH's float type, and it is True iff box_contacts' count pass finds at least one
    triangle for it (touching counts).  One launch: the count pass alone, in the grid's own order (z fastest), which is
    coherent enough to walk as given.  origin: three numbers; spacing: one number, or three."""
    torch = _require_gpu()
    what = "voxelize"
    number = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
    if not (isinstance(shape, (tuple, list)) and len(shape) == 3 and all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) and s >= 0 for s in shape)):
        raise ValueError(f"{what}: shape must be three non-negative integers (nx, ny, nz)")
    if not (isinstance(origin, (tuple, list, np.ndarray)) and len(origin) == 3 and all(number(x) for x in origin)):
        raise ValueError(f"{what}: origin must be three numbers")
    if number(spacing):
        spacing = (spacing,) * 3
    if not (isinstance(spacing, (tuple, list, np.ndarray)) and len(spacing) == 3 and all(number(x) for x in spacing)):
        raise ValueError(f"{what}: spacing must be a number or three numbers")
    ft = _torch_float(bvh.types.leaf_float)
    step = torch.tensor([float(x) for x in spacing], dtype=ft, device="cuda")
    start = torch.tensor([float(x) for x in origin], dtype=ft, device="cuda")
    axes = [torch.arange(int(s), dtype=ft, device="cuda") + 0.5 for s in shape]
    cells = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=0).reshape(3, -1)   # (3, nx * ny * nz), z fastest
    centers = start[:, None] + cells * step[:, None]
    half = (step / 2)[:, None].expand(3, centers.shape[1])
    got = box_contacts(bvh, triangles, centers, half, count_only=True, presorted=True)
    return (got.counts > 0).reshape(tuple(int(s) for s in shape))


# ---------------------------------------------------------------------------------------------
# inside / outside of a closed mesh for a batch of query points (ibvh_point_crossings; no reference counterpart)
# ---------------------------------------------------------------------------------------------
class PointCrossings:
    """Per query point: .crossings (N,) the number of triangles the axis ray from the point crosses, .winding (N,) the ccw
    crossings minus the cw ones (+1 inside an outward-oriented closed mesh, -1 inside an inward-oriented one, 0 outside)."""

    def __init__(self, crossings, winding):
        self.crossings, self.winding = crossings, winding


def _check_axis(axis, what):
    if not (isinstance(axis, (int, np.integer)) and not isinstance(axis, bool) and 0 <= axis <= 2):
        raise ValueError(f"{what}: axis must be 0, 1 or 2")
    return int(axis)


def _check_rule(rule, what):
    if rule not in ("parity", "winding"):
        raise ValueError(f"{what}: rule must be 'parity' or 'winding'")


def point_crossings(bvh, triangles, points, axis=0, presorted=False):
    """For every query point P the triangles of the mesh `bvh` was built over that the ray P + t*e_axis, t > 0, crosses
    -> PointCrossings (include/ibvh.h, ibvh_point_crossings: the guard, the canonical edge order that makes a ray through a
    shared edge or vertex cross the surface once, the depth test and why pruning loses nothing are spelled out there).  One
    launch, exact: equal to a brute force over all triangles.

    bvh: BBox leaves made from `triangles` (bounding_volumes_from_triangles(triangles, BBox(dtype)); a skin margin and
    refit are fine) under BBox nodes of the same or a wider float type.  triangles: (n, 9) / (n, 3, 3) CUDA tensor of the
    leaves' dtype, user index k = row k - 1.  points: (3, N) CUDA tensor of that dtype, as for traverse_rays.  axis: 0, 1
    or 2.  The device walks the batch in Morton order of the points (lanes of a wave then share nodes) and the outputs are
    put back in the caller's order; presorted=True walks it as given.

    Points on the surface are ambiguous; shared vertices must be bit-identical (no T-junctions or cracks).

    ValueError: sphere leaves or nodes, nodes narrower than the leaves, a wrong dtype, device or shape, an axis outside
    0..2, and a leaf whose index lies outside 1..n (flag bit 1; such leaves are skipped)."""
    torch = _require_gpu()
    axis = _check_axis(axis, "point_crossings")
    tris, ft, idt = _mesh_query_setup(bvh, triangles, "point_crossings")
    p, n, _, order = _query_points(points, ft, None, presorted, "point_crossings")
    crossings = torch.empty(n, dtype=idt, device="cuda")
    winding = torch.empty(n, dtype=idt, device="cuda")
    if n == 0:
        return PointCrossings(crossings, winding)
    _mesh_query_call("ibvh_point_crossings", "point_crossings", bvh, tris, _ptr(p), n, axis, _ptr(crossings), _ptr(winding))
    return PointCrossings(*_unpermute(order, (crossings, winding)))


def _inside(pc, rule):
    return (pc.crossings & 1) == 1 if rule == "parity" else pc.winding != 0


def points_inside(bvh, triangles, points, axis=0, rule="parity"):
    """Which query points lie inside the closed mesh `bvh` was built over -> (N,) bool tensor, from point_crossings:
    rule="parity": the axis ray crosses an odd number of triangles (independent of the triangles' orientation);
    rule="winding": the winding number is not zero (needs a consistent orientation; right for unions of overlapping closed
    bodies).  Arguments and ValueErrors as for point_crossings; also an unknown rule."""
    _check_rule(rule, "points_inside")
    return _inside(point_crossings(bvh, triangles, points, axis=axis), rule)


def signed_distance(bvh, triangles, points, axis=0, rule="parity", max_distance=None):
    """The signed distance of every query point to the closed mesh `bvh` was built over -> (distance, ClosestPoints):
    distance (N,) = sqrt(closest_points().distance2), negated where points_inside(rule) says inside, +Inf where no triangle
    lies within max_distance.  The batch is ordered along the Morton curve once and both queries walk it in that order: two
    launches; torch computes the sign and the square root only.  Arguments and ValueErrors as for closest_points and
    points_inside."""
    torch = _require_gpu()
    _check_rule(rule, "signed_distance")
    axis = _check_axis(axis, "signed_distance")
    _check_points_shape(points, "signed_distance")
    order = None
    if points.shape[1] > 0 and points.is_cuda:
        order = _morton_order(points.t())
        points = points[:, order]
    cp = closest_points(bvh, triangles, points, max_distance=max_distance, presorted=True)
    inside = _inside(point_crossings(bvh, triangles, points, axis=axis, presorted=True), rule)
    distance = torch.sqrt(cp.distance2)
    distance = torch.where(inside & (cp.index != 0), -distance, distance)
    distance, index, d2, q = _unpermute(order, (distance, cp.index, cp.distance2, cp.point))
    return distance, ClosestPoints(index, d2, q)


def lvt_work_counters(bvh, bvh2=None, points=None, directions=None):
    """Measurement helper (ibvh_lvt_work_counters, include/ibvh.h): the work of ONE counting pass of the leaf-vs-tree walk
    the ordinary call would take — traverse(bvh), traverse(bvh, bvh2) or traverse_rays(bvh, points, directions) — as a dict
    {node_tests, leaf_tests, node_fetches, leaf_fetches, touched_bytes}.  Bench types only (the reference
    counts such work for BFS only, BVHTraversal.num_checks)."""
    torch = _require_gpu()
    idt = _torch_index(bvh.types.index_type)
    work = torch.zeros(4, dtype=torch.int64, device="cuda")
    s = bvh.struct()
    if points is not None:
        ft = _torch_float(bvh.types.leaf_float)
        p = points.to(device="cuda", dtype=ft).t().contiguous()
        d = directions.to(device="cuda", dtype=ft).t().contiguous()
        counts = torch.empty(p.shape[0], dtype=idt, device="cuda")
        lib.call("ibvh_lvt_work_counters", C.byref(s), None, _ptr(p), _ptr(d), p.shape[0], _ptr(counts), _ptr(work), _stream())
    elif bvh2 is not None:
        s2 = bvh2.struct()
        counts = torch.empty(max(len(bvh.leaves), len(bvh2.leaves)), dtype=idt, device="cuda")
        lib.call("ibvh_lvt_work_counters", C.byref(s), C.byref(s2), None, None, 0, _ptr(counts), _ptr(work), _stream())
    else:
        counts = torch.empty(len(bvh.leaves), dtype=idt, device="cuda")
        lib.call("ibvh_lvt_work_counters", C.byref(s), None, None, None, 0, _ptr(counts), _ptr(work), _stream())
    w = [int(x) for x in work.cpu().tolist()]
    lay = bvh.leaves.layout
    return {"node_tests": w[0], "leaf_tests": w[1], "node_fetches": w[2], "leaf_fetches": w[3],
            "touched_bytes": w[2] * int(lay.node_bytes) + w[3] * int(lay.leaf_bytes), "contacts_counted": int(counts.sum().item())}


# ---------------------------------------------------------------------------------------------
# input preparation
# ---------------------------------------------------------------------------------------------
def bounding_volumes_from_triangles(triangles, volume_type=None):
    """BSphere{T}(p1,p2,p3) / BBox{T}(p1,p2,p3) for an (n, 3, 3) or (n, 9) CUDA tensor of triangles
    (bsphere.jl:43-112, bbox.jl:59-70)."""
    torch = _require_gpu()
    t = triangles.reshape(triangles.shape[0], 9).contiguous()
    vt = volume_type or BSphere(t.dtype)
    t = t.to(_torch_float(vt.flt))
    out = torch.empty((t.shape[0], abi.volume_width(vt.kind)), dtype=t.dtype, device="cuda")
    lib.call("ibvh_volumes_from_triangles", vt.kind, vt.flt, _ptr(t), t.shape[0], _ptr(out), _stream())
    return out


def load_obj_triangles(path, dtype=None):
    """Minimal Wavefront OBJ reader (`v x y z` / `f a b c ...`, 1-based or negative indices, `a/b/c` forms,
    polygons fan-triangulated) -> (n, 3, 3) CUDA tensor of triangles, the input of
    bounding_volumes_from_triangles.  Stands in for MeshIO/FileIO in the reference's benchmark scripts
    (benchmark/bvh_contact.jl:30-36); parsing is host-side file I/O, not part of the hot path."""
    torch = _require_gpu()
    verts, faces = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                verts.append([float(x) for x in line.split()[1:4]])
            elif line.startswith("f "):
                idx = [int(tok.split("/")[0]) for tok in line.split()[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fa = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(fa) and (fa.min() < 0 or fa.max() >= len(v)):
        raise ValueError("OBJ face index out of range")
    tri = v[fa] if len(fa) else np.zeros((0, 3, 3))
    return torch.from_numpy(tri).to(device="cuda", dtype=dtype or torch.float32)


def generate_spheres(n, seed, first_index=0, origin=(0.0, 0.0, 0.0), extent=(1.0, 1.0, 1.0), r0=0.01):
    """Deterministic synthetic BSphere{Float32} cloud (counter-based SplitMix64), on device."""
    torch = _require_gpu()
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    o = (C.c_float * 3)(*origin)
    e = (C.c_float * 3)(*extent)
    lib.call("ibvh_generate_spheres_f32", int(n), C.c_uint64(seed), int(first_index), o, e, C.c_float(r0), _ptr(out), _stream())
    return out
