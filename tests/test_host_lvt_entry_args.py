"""The status every leaf-vs-tree entry point (ibvh_traverse_{lvt,pair_lvt,rays_lvt}_{count,write,enqueue}) returns for a bad
argument, one at a time against an otherwise well-formed call, plus a few pairs of bad arguments that pin which check comes
first.  Every case returns before the library makes any HIP call, so the buffers are host memory the library never touches.
The front ends differ on purpose in places (a NULL scratch is IBVH_ERR_SCRATCH for the self enqueue and the writes, but
IBVH_ERR_INVALID_ARG for the other counts and enqueues); this pins them as they are.  No GPU."""
import ctypes as C

import pytest

import implicitbvh_amd as ibvh  # noqa: F401  (registers the package under its import name)
from implicitbvh_amd import abi, lib

OK, INVALID, UNSUPPORTED, SCRATCH = abi.OK, abi.ERR_INVALID_ARG, abi.ERR_UNSUPPORTED, abi.ERR_SCRATCH

# the parameters of each entry point, in order (include/ibvh.h)
PARAMS = {
    "lvt_count": "bvh sl narrow counts total_out scratch scratch_bytes stream",
    "lvt_write": "bvh sl narrow counts contacts scratch scratch_bytes stream",
    "lvt_enqueue": "bvh sl narrow counts contacts capacity total_dev total_host scratch scratch_bytes stream",
    "pair_lvt_count": "bvh1 bvh2 sl1 sl2 narrow counts total_out scratch scratch_bytes stream",
    "pair_lvt_write": "bvh1 bvh2 sl1 sl2 narrow counts contacts scratch scratch_bytes stream",
    "pair_lvt_enqueue": "bvh1 bvh2 sl1 sl2 narrow counts contacts capacity total_dev total_host scratch scratch_bytes stream",
    "rays_lvt_count": "bvh points dirs num_rays sl narrow counts total_out scratch scratch_bytes stream",
    "rays_lvt_write": "bvh points dirs num_rays sl narrow counts contacts scratch scratch_bytes stream",
    "rays_lvt_enqueue": "bvh points dirs num_rays sl narrow counts contacts capacity total_dev total_host scratch scratch_bytes stream",
}
SELF = ("lvt_count", "lvt_write", "lvt_enqueue")
PAIR = ("pair_lvt_count", "pair_lvt_write", "pair_lvt_enqueue")
RAYS = ("rays_lvt_count", "rays_lvt_write", "rays_lvt_enqueue")
ALL = SELF + PAIR + RAYS

N1, N2, NR = 100, 60, 50  # leaves of bvh / bvh1, of bvh2; rays
BIG = 1 << 30             # a scratch_bytes no size check refuses
_buf = C.create_string_buffer(4096)  # stands in for every device buffer: never read or written by a call that fails its checks
BUF = C.cast(_buf, C.c_void_p)


def _bvh(n, types=None, built_level=1):
    tree = abi.Tree()
    lib.call("ibvh_tree_shape", n, C.byref(tree))
    return abi.Bvh(types if types is not None else abi.make_types(), tree, built_level, BUF, BUF, BUF)


def _call(entry, **bad):
    """entry(good arguments, with `bad` replacing some of them) -> status"""
    total = C.c_int64(-1)
    good = dict(bvh=_bvh(N1), bvh1=_bvh(N1), bvh2=_bvh(N2), sl=1, sl1=1, sl2=1, narrow=abi.NARROW_NONE, counts=BUF,
                total_out=C.byref(total), contacts=BUF, capacity=16, total_dev=None, total_host=None, scratch=BUF,
                scratch_bytes=BIG, stream=None, points=BUF, dirs=BUF, num_rays=NR)
    good.update(bad)
    args = [good[p] for p in PARAMS[entry].split()]
    args = [C.byref(a) if isinstance(a, abi.Bvh) else a for a in args]
    return getattr(lib.load(), "ibvh_traverse_" + entry)(*args)


MIXED_FLOAT = abi.make_types(leaf_float=abi.F64)                            # BSphere{Float64} leaves, BBox{Float32} nodes
BOX_BOX = abi.make_types(leaf_kind=abi.BBOX)                                # BBox{Float32} leaves and nodes
SPH_SPH = abi.make_types(node_kind=abi.BSPHERE)                             # BSphere{Float32} leaves and nodes
NO_COMBO = abi.make_types(leaf_kind=abi.BBOX, node_kind=abi.BSPHERE)        # no BSphere(::BBox): not instantiated
NO_INDEX = abi.Types(abi.BSPHERE, abi.F32, abi.BBOX, abi.F32, 7, abi.U32)   # an index type that does not exist
SMALL = 8                                                                   # below scan_scratch_bytes(n) for any n

CASES = [
    # ---- every entry point --------------------------------------------------------------------------------------------
    *[(e, dict(narrow=0x1000), INVALID, "unknown narrow bit") for e in ALL],
    *[(e, dict(counts=None), INVALID, "NULL counts") for e in ALL],
    *[(e, dict(scratch_bytes=SMALL), SCRATCH, "scratch below scan_scratch_bytes") for e in ALL],
    *[(e, dict(capacity=-1), INVALID, "capacity < 0") for e in ("lvt_enqueue", "pair_lvt_enqueue", "rays_lvt_enqueue")],
    *[(e, dict(contacts=None), INVALID, "capacity > 0, NULL contacts") for e in ("lvt_enqueue", "pair_lvt_enqueue", "rays_lvt_enqueue")],
    *[(e, dict(contacts=None), INVALID, "NULL contacts") for e in ("lvt_write", "pair_lvt_write", "rays_lvt_write")],
    *[(e, dict(total_out=None), INVALID, "NULL total_out") for e in ("lvt_count", "pair_lvt_count", "rays_lvt_count")],
    # NULL scratch: the front ends differ
    ("lvt_count", dict(scratch=None), INVALID, "NULL scratch"),
    ("lvt_write", dict(scratch=None), SCRATCH, "NULL scratch"),
    ("lvt_enqueue", dict(scratch=None), SCRATCH, "NULL scratch"),
    ("pair_lvt_count", dict(scratch=None), INVALID, "NULL scratch"),
    ("pair_lvt_write", dict(scratch=None), SCRATCH, "NULL scratch"),
    ("pair_lvt_enqueue", dict(scratch=None), INVALID, "NULL scratch"),
    ("rays_lvt_count", dict(scratch=None), INVALID, "NULL scratch"),
    ("rays_lvt_write", dict(scratch=None), SCRATCH, "NULL scratch"),
    ("rays_lvt_enqueue", dict(scratch=None), INVALID, "NULL scratch"),
    # ---- self ---------------------------------------------------------------------------------------------------------
    *[(e, dict(bvh=None), INVALID, "NULL bvh") for e in SELF],
    *[(e, dict(sl=0), INVALID, "start level 0") for e in SELF],
    *[(e, dict(bvh=_bvh(N1, built_level=3), sl=2), INVALID, "start level below built_level") for e in SELF],
    *[(e, dict(sl=_bvh(N1).tree.levels + 1), INVALID, "start level above levels") for e in SELF],
    *[(e, dict(bvh=_bvh(1 << 33), sl=_bvh(1 << 33).tree.levels), INVALID, "levels > 32") for e in SELF],
    *[(e, dict(narrow=abi.NARROW_RAY_ORIGIN_OUTSIDE), INVALID, "rays-only narrow") for e in SELF],
    *[(e, dict(narrow=abi.PAIR_SMALLER_DRIVES), INVALID, "pair-only flag") for e in SELF],
    *[(e, dict(bvh=_bvh(N1, NO_COMBO)), UNSUPPORTED, "BBox leaves, BSphere nodes") for e in SELF],
    *[(e, dict(bvh=_bvh(N1, NO_INDEX)), UNSUPPORTED, "unknown index type") for e in SELF],
    # a single leaf: nothing to walk, no buffer needed (the enqueue zeroes its totals on the device: GPU suite)
    ("lvt_count", dict(bvh=_bvh(1), counts=None, scratch=None), OK, "single leaf"),
    ("lvt_write", dict(bvh=_bvh(1), counts=None, contacts=None, scratch=None), OK, "single leaf"),
    # which check comes first
    ("lvt_count", dict(sl=0, counts=None), INVALID, "bad level before NULL counts"),
    ("lvt_count", dict(bvh=_bvh(1), sl=0), INVALID, "bad level before the single-leaf return"),
    ("lvt_write", dict(narrow=0x1000, scratch=None), INVALID, "narrow before scratch"),
    ("lvt_write", dict(bvh=_bvh(N1, NO_COMBO), scratch=None), UNSUPPORTED, "types before scratch"),
    ("lvt_enqueue", dict(sl=0, scratch=None), INVALID, "bad level before scratch"),
    ("lvt_enqueue", dict(scratch=None, counts=None), SCRATCH, "scratch before NULL counts"),
    ("lvt_enqueue", dict(bvh=_bvh(1), scratch=None), SCRATCH, "scratch before the single-leaf return"),
    ("lvt_enqueue", dict(scratch_bytes=SMALL, narrow=0x1000), SCRATCH, "scratch before narrow"),
    # ---- pair ---------------------------------------------------------------------------------------------------------
    *[(e, dict(bvh1=None), INVALID, "NULL bvh1") for e in PAIR],
    *[(e, dict(bvh2=None), INVALID, "NULL bvh2") for e in PAIR],
    *[(e, dict(sl1=0), INVALID, "start level 0") for e in PAIR],
    *[(e, dict(sl2=_bvh(N2).tree.levels + 1), INVALID, "start level above levels") for e in PAIR],
    *[(e, dict(bvh2=_bvh(N2, built_level=2), sl2=1), INVALID, "start level below built_level") for e in PAIR],
    *[(e, dict(bvh1=_bvh(1 << 33), sl1=_bvh(1 << 33).tree.levels), INVALID, "levels > 32") for e in PAIR],
    *[(e, dict(narrow=abi.NARROW_RAY_ORIGIN_OUTSIDE), INVALID, "rays-only narrow") for e in PAIR],
    *[(e, dict(bvh2=_bvh(N2, MIXED_FLOAT)), UNSUPPORTED, "two types without the flag") for e in PAIR],
    *[(e, dict(bvh2=_bvh(N2, abi.make_types(index_type=abi.I64)), narrow=abi.PAIR_MIXED_TYPES), UNSUPPORTED,
       "the flag, two index types") for e in PAIR],
    *[(e, dict(bvh1=_bvh(N1, NO_COMBO), bvh2=_bvh(N2, NO_COMBO)), UNSUPPORTED, "BBox leaves, BSphere nodes") for e in PAIR],
    # BBox leaves driving BSphere nodes are refused; the same two trees the other way round are accepted (and then fail on
    # the scratch, just before the walk)
    *[(e, dict(bvh1=_bvh(N1, BOX_BOX), bvh2=_bvh(N2, SPH_SPH), narrow=abi.PAIR_MIXED_TYPES), UNSUPPORTED,
       "BBox leaves drive BSphere nodes") for e in PAIR],
    *[(e, dict(bvh1=_bvh(N1, BOX_BOX), bvh2=_bvh(N2, SPH_SPH), narrow=abi.PAIR_MIXED_TYPES | abi.PAIR_SMALLER_DRIVES,
               scratch_bytes=SMALL), SCRATCH, "smaller drives: BSphere leaves drive BBox nodes") for e in PAIR],
    *[(e, dict(bvh1=_bvh(N1, SPH_SPH), bvh2=_bvh(N2, BOX_BOX), narrow=abi.PAIR_MIXED_TYPES, scratch_bytes=SMALL), SCRATCH,
       "BSphere leaves drive BBox nodes") for e in PAIR],
    *[(e, dict(bvh1=_bvh(N1, SPH_SPH), bvh2=_bvh(N2, BOX_BOX), narrow=abi.PAIR_MIXED_TYPES | abi.PAIR_SMALLER_DRIVES),
       UNSUPPORTED, "smaller drives: BBox leaves drive BSphere nodes") for e in PAIR],
    *[(e, dict(bvh1=_bvh(N1, MIXED_FLOAT), bvh2=_bvh(N2, NO_COMBO), narrow=abi.PAIR_MIXED_TYPES), UNSUPPORTED,
       "the flag, a walked tree of no instantiated type") for e in PAIR],
    # which check comes first
    ("pair_lvt_count", dict(scratch=None, bvh1=None), INVALID, "NULL scratch before NULL bvh1"),
    ("pair_lvt_count", dict(bvh2=_bvh(N2, MIXED_FLOAT), counts=None), UNSUPPORTED, "types before NULL counts"),
    ("pair_lvt_count", dict(sl1=0, bvh2=_bvh(N2, MIXED_FLOAT)), INVALID, "levels before types"),
    ("pair_lvt_write", dict(contacts=None, bvh2=_bvh(N2, MIXED_FLOAT)), INVALID, "NULL contacts before types"),
    ("pair_lvt_write", dict(scratch=None, narrow=0x1000), INVALID, "narrow before scratch"),
    ("pair_lvt_enqueue", dict(capacity=-1, bvh2=_bvh(N2, MIXED_FLOAT)), INVALID, "capacity before types"),
    ("pair_lvt_enqueue", dict(bvh1=_bvh(N1, BOX_BOX), bvh2=_bvh(N2, SPH_SPH), narrow=abi.PAIR_MIXED_TYPES, counts=None),
     INVALID, "NULL counts before the BSphere(::BBox) refusal"),
    # ---- rays ---------------------------------------------------------------------------------------------------------
    *[(e, dict(bvh=None), INVALID, "NULL bvh") for e in RAYS],
    *[(e, dict(num_rays=-1), INVALID, "num_rays < 0") for e in RAYS],
    *[(e, dict(sl=0), INVALID, "start level 0") for e in RAYS],
    *[(e, dict(bvh=_bvh(N1, built_level=3), sl=2), INVALID, "start level below built_level") for e in RAYS],
    *[(e, dict(sl=_bvh(N1).tree.levels + 1), INVALID, "start level above levels") for e in RAYS],
    *[(e, dict(bvh=_bvh(1 << 33), sl=_bvh(1 << 33).tree.levels), INVALID, "levels > 32") for e in RAYS],
    *[(e, dict(points=None), INVALID, "NULL points") for e in RAYS],
    *[(e, dict(dirs=None), INVALID, "NULL dirs") for e in RAYS],
    *[(e, dict(narrow=abi.NARROW_MORTON_LT), INVALID, "MORTON_LT") for e in RAYS],
    *[(e, dict(narrow=abi.PAIR_MIXED_TYPES), INVALID, "pair-only flag") for e in RAYS],
    *[(e, dict(bvh=_bvh(N1, MIXED_FLOAT)), UNSUPPORTED, "leaf_float != node_float") for e in RAYS],
    *[(e, dict(bvh=_bvh(N1, NO_COMBO)), UNSUPPORTED, "BBox leaves, BSphere nodes") for e in RAYS],
    *[(e, dict(bvh=_bvh(N1, NO_INDEX)), UNSUPPORTED, "unknown index type") for e in RAYS],
    # no rays: nothing to walk, no buffer needed (the enqueue zeroes its totals on the device: GPU suite)
    ("rays_lvt_count", dict(num_rays=0, points=None, dirs=None, counts=None), OK, "no rays"),
    ("rays_lvt_write", dict(num_rays=0, points=None, dirs=None, counts=None, contacts=None, scratch=None), OK, "no rays"),
    # which check comes first
    ("rays_lvt_count", dict(num_rays=0, scratch=None, sl=0), INVALID, "bad level before the no-ray return"),
    ("rays_lvt_count", dict(bvh=_bvh(N1, MIXED_FLOAT), points=None), UNSUPPORTED, "float types before NULL points"),
    ("rays_lvt_write", dict(bvh=_bvh(N1, MIXED_FLOAT), contacts=None), INVALID, "NULL contacts before float types"),
    ("rays_lvt_write", dict(num_rays=0, bvh=_bvh(N1, MIXED_FLOAT)), UNSUPPORTED, "float types before the no-ray return"),
    ("rays_lvt_enqueue", dict(scratch=None, bvh=None), INVALID, "NULL scratch before NULL bvh"),
    ("rays_lvt_enqueue", dict(narrow=abi.NARROW_MORTON_LT, scratch_bytes=SMALL), INVALID, "narrow before scratch"),
]


@pytest.mark.parametrize("entry, bad, status, what", CASES,
                         ids=[f"{e}-{w.replace(' ', '_')}-{i}" for i, (e, _, _, w) in enumerate(CASES)])
def test_entry_point_status(entry, bad, status, what):
    got = _call(entry, **bad)
    assert got == status, f"ibvh_traverse_{entry} ({what}): status {got}, expected {status}"


def test_count_resets_total_before_its_checks():
    """*_count writes 0 to *total_out once it has a total_out (and, for self, a bvh), before the other checks."""
    for entry, bad in (("lvt_count", dict(sl=0)), ("pair_lvt_count", dict(bvh1=None)), ("rays_lvt_count", dict(bvh=None))):
        total = C.c_int64(-1)
        assert _call(entry, total_out=C.byref(total), **bad) == INVALID
        assert total.value == 0, entry
    total = C.c_int64(-1)
    assert _call("lvt_count", bvh=None, total_out=C.byref(total)) == INVALID
    assert total.value == -1
