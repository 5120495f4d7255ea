"""The three routes by which ibvh_build gets the bounds its Morton keys are scaled by (csrc/ibvh_build.hip launch_extrema), each
named by the launches it makes and compared with the oracle bit for bit:
    n <= 2^21            extrema_partial_kernel, then every workgroup of encode_hist_kernel folds the partials for itself
    n >  2^21            extrema_partial_kernel, the one-workgroup extrema_final_kernel (which also writes the caller's copy of
                         the extrema and the skips), encode_hist_kernel
    compute_extrema=0    extrema_set_kernel with the caller's bounds, encode_hist_kernel
assert_bvh_equal covers the extrema output, the Morton code of every leaf (so the bounds EVERY encode workgroup folded), the
skips and the nodes.  Sizes: 1; 1,025 = two partials, the second of one leaf; 3,001 = three with a ragged last block; 524,289 =
the first size with EXT_FOLD_BLOCKS = 512 partials and a grid-stride trip; 2^21 and 2^21 + 1 = either side of the switch (the
threshold cannot be reached with fewer leaves).  BSphere{Float32} and BBox{Float64} leaves, under BBox nodes of the leaf float
type."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_parity import TOKENS, assert_bvh_equal, cuda, make_options, random_volumes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi  # noqa: E402
from test_gpu_build_routes import base_name  # noqa: E402
from test_gpu_lvt_blocks import _kernels_of  # noqa: E402

LEAVES = {"bsphere-f32": (abi.BSPHERE, abi.F32), "bbox-f64": (abi.BBOX, abi.F64)}
FOLD_MAX = 1 << 21  # the largest build whose encoder folds the partials
PARTIAL, FINAL, SET, ENCODE = "extrema_partial_kernel", "extrema_final_kernel", "extrema_set_kernel", "encode_hist_kernel"
IN_ENCODER, ONE_WORKGROUP, FIXED = [PARTIAL, ENCODE], [PARTIAL, FINAL, ENCODE], [SET, ENCODE]


def types_of(leaf):
    kind, flt = LEAVES[leaf]
    return abi.make_types(kind, flt, abi.BBOX, flt)


def node_type(leaf):
    return TOKENS[abi.BBOX](torch.float32 if LEAVES[leaf][1] == abi.F32 else torch.float64)


@functools.lru_cache(maxsize=None)
def volumes(leaf, n):
    vols = random_volumes(np.random.default_rng(11 * n + len(leaf)), n, *LEAVES[leaf])
    vols.setflags(write=False)
    return vols


def extrema_launches(fn):
    """the extrema and key launches of the build inside fn(), in order"""
    return [k for k in map(base_name, _kernels_of(fn)) if k in (PARTIAL, FINAL, SET, ENCODE)]


@pytest.mark.parametrize("leaf", list(LEAVES))
@pytest.mark.parametrize("n", [1, 1025, 3001, 524289, FOLD_MAX, FOLD_MAX + 1])
def test_computed_extrema_fold_in_the_encoder_up_to_the_switch(n, leaf):
    types = types_of(leaf)
    o = orc.build(volumes(leaf, n), types)
    dev, holder = cuda(volumes(leaf, n).copy()), {}
    ran = extrema_launches(lambda: holder.update(g=ibvh.BVH(dev, node_type(leaf), options=make_options(types))))
    assert ran == (IN_ENCODER if n <= FOLD_MAX else ONE_WORKGROUP), (n, leaf, ran)
    assert_bvh_equal(o, holder["g"])


@pytest.mark.parametrize("leaf", list(LEAVES))
def test_fixed_bounds_launch_no_reduction(leaf):
    n, types = 1000, types_of(leaf)
    mins, maxs = (-0.5, -0.25, -1.0), (6.5, 7.0, 6.25)  # (the centres lie in [0, 6]^3)
    o = orc.build(volumes(leaf, n), types, compute_extrema=False, mins=mins, maxs=maxs)
    opts = ibvh.BVHOptions(morton=ibvh.DefaultMortonAlgorithm(np.uint32, compute_extrema=False, mins=mins, maxs=maxs))
    dev, holder = cuda(volumes(leaf, n).copy()), {}
    ran = extrema_launches(lambda: holder.update(g=ibvh.BVH(dev, node_type(leaf), options=opts)))
    assert ran == FIXED, (leaf, ran)
    assert_bvh_equal(o, holder["g"])


@pytest.mark.parametrize("leaf", list(LEAVES))
def test_wrapped_records_in_place_read_the_centres_at_the_record_stride(leaf):
    n, types = 3001, types_of(leaf)
    indices = np.random.default_rng(n).permutation(n) + 100
    o = orc.build(volumes(leaf, n), types, indices=indices)
    opts = make_options(types)
    bv = ibvh.BoundingVolumes.wrap(cuda(volumes(leaf, n).copy()), indices, opts)
    holder = {}
    ran = extrema_launches(lambda: holder.update(g=ibvh.BVH(bv, node_type(leaf), options=opts)))
    assert ran == IN_ENCODER, (leaf, ran)
    assert holder["g"].leaves.buf.data_ptr() == bv.buf.data_ptr()
    assert_bvh_equal(o, holder["g"])
