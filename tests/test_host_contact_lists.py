"""The comparators both list queries' GPU tests rest on (tests/mesh_query_kit.py: same, for what the two passes through the C
entry point return, and assert_equal, for a Python result) are not blind: handed a checker result as the query's own answer
they pass, and with ONE field changed by one bit — a count or an index off by one, a float by one unit in the last place, one
bit of a mask or a region — they fail, whichever field it is.  Numpy only, no GPU."""
import types

import numpy as np
import pytest

import mesh_query_kit as kit
import sphere_contacts_checker as scc
import triangle_contacts_checker as tcc
from triangle_contacts_checker import FAR, FLAT, PIERCING, TOUCHING


def _spheres():
    """the unit triangle's seven regions, each from a sphere that just reaches it, and a sphere that reaches nothing"""
    f = np.float32
    c = np.array([[-1, -1, 1], [2, -0.5, 1], [0.5, -1, 1], [-0.5, 2, 1], [-1, 0.5, 1], [1, 1, 1], [0.25, 0.25, 1], [0.25, 0.25, 1]], f)
    r = np.append(np.nextafter(np.sqrt(np.array([3, 2.25, 2, 2.25, 2, 1.5, 1], f)), f(np.inf)), f(0.5))
    exp = scc.brute_force(np.array([FLAT, FAR], f), c, r, idt=np.int32)
    assert exp.counts.tolist() == [1] * 7 + [0] and exp.region.tolist() == list(range(7))
    return scc.QUERY, exp


def _triangles():
    """a piercing and a touching query over three stacked triangles and a far one, and a query that cuts nothing"""
    f = np.float64
    tris = np.array([FLAT, [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5], FAR, [0, 0, -0.5, 1, 0, -0.5, 0, 1, -0.5]], f)
    exp = tcc.brute_force(tris, np.array([PIERCING, [50, 50, 50, 51, 50, 50, 50, 51, 50], TOUCHING], f), idt=np.int64)
    assert exp.counts.tolist() == [3, 0, 2] and exp.index.tolist() == [1, 2, 4, 1, 2] and len(set(exp.mask.tolist())) >= 2
    return tcc.QUERY, exp


def _flipped(a, row):
    """a copy of `a` with the lowest bit of row `row`'s first element flipped"""
    out = np.array(a)
    out.view(np.uint8).reshape(len(out), -1)[row, 0] ^= 1
    return out


def _two_passes_of(query, exp):
    """what kit.two_passes() returns for a library that answers `exp`"""
    got = dict(status_count=0, status=0, counts=exp.counts, total=len(exp.index))
    got.update({k: getattr(exp, col.checker) for k, col in query.columns.items()})
    return got


def _result_of(query, exp, count_only=False):
    """the Python result of a library that answers `exp`, as numpy arrays"""
    got = types.SimpleNamespace(offsets=exp.offsets, counts=exp.counts)
    for col in query.columns.values():
        setattr(got, col.result, None if count_only else getattr(exp, col.checker))
    setattr(got, query.owner, None if count_only else getattr(exp, query.owner) + 1)
    return got


@pytest.mark.parametrize("case", [_spheres, _triangles], ids=["spheres", "triangles"])
def test_each_comparator_fails_on_one_changed_bit_of_any_field(case):
    query, exp = case()
    last, busy = len(exp.index) - 1, int(np.flatnonzero(exp.counts)[-1])
    assert 4 <= last < 8 and len(query.columns) >= 3
    # unchanged: both pass
    kit.same(query, _two_passes_of(query, exp), exp)
    kit.assert_equal(query, _result_of(query, exp), exp, "unchanged")
    kit.assert_equal(query, _result_of(query, exp, count_only=True), exp, "unchanged", count_only=True)
    # the C entry's: a count, then every column in turn; and a column that was not asked for must keep its sentinel
    for key, row in [("counts", busy)] + [(k, last) for k in query.columns]:
        got = _two_passes_of(query, exp)
        got[key] = _flipped(got[key], row)
        assert kit.bits(got[key]) != kit.bits(_two_passes_of(query, exp)[key])
        with pytest.raises(AssertionError):
            kit.same(query, got, exp, key)
    for key in query.columns:
        with pytest.raises(AssertionError):
            kit.same(query, _two_passes_of(query, exp), exp, key, outs="".join(query.columns).replace(key, ""))
    # the Python result's: a count, an offset, every column, the owner column; after count_only any column at all
    names = [("counts", busy), ("offsets", busy)] + [(col.result, last) for col in query.columns.values()] + [(query.owner, last)]
    for name, row in names:
        got = _result_of(query, exp)
        setattr(got, name, _flipped(getattr(got, name), row))
        with pytest.raises(AssertionError):
            kit.assert_equal(query, got, exp, name)
    for name, _ in names[2:]:
        got = _result_of(query, exp, count_only=True)
        setattr(got, name, getattr(_result_of(query, exp), name))
        with pytest.raises(AssertionError):
            kit.assert_equal(query, got, exp, name, count_only=True)
