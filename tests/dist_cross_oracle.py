"""What the two test files of the cross-shard contact completion share on the oracle's side: the oracle's tree over a shard
of a case of tests/dist_cross_checker.py, and the contacts between two shards with all pairs tried."""
import numpy as np

import oracle_lib as orc
from implicitbvh_amd import abi

_TREES = {}


def types_of(case):
    return abi.make_types(*case.combo, *case.im)


def oracle_tree(case, r):
    """The oracle's tree over shard r as path (B) builds it: the volumes as they are, global 1-based indices."""
    key = (case.name, r)
    if key not in _TREES:
        n = len(case.shards[r])
        idx = (case.base[r] + 1 + np.arange(n)).astype(abi.INDEX_DTYPES[case.im[0]])
        _TREES[key] = orc.build(case.shards[r], types_of(case), indices=idx)
    return _TREES[key]


def pair_codes(a, b):
    """Pairs of (small, positive) indices as sorted int64 codes: sets compare as arrays."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert a.size == 0 or (0 < a.min() and a.max() < 2**31 and 0 < b.min() and b.max() < 2**31)
    return np.sort((a << 32) | b)


def brute_pairs(case, r, s):
    """Contacts between shards r and s as the leaf type's own test finds them, all pairs tried: codes of (global index
    in r, global index in s)."""
    p = orc.brute_force_pair(case.combo[0], case.combo[1], case.shards[r], case.shards[s])
    return pair_codes(p[:, 0] + case.base[r], p[:, 1] + case.base[s])
