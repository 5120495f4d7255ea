"""The triangle-vs-mesh contact query (ibvh_triangle_contacts) on the benchmark meshes, beside the way to get there without it.

    python tools/bench_triangle_contacts.py [--workloads published,config3] [--steps K] [--warmup W]

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks)
  config3    the 7.2 M-triangle torus (bench.py's surface)
The queries are the other mesh of the tests: the same mesh rotated by 0.5 rad about the x axis and shifted by
(0.9, 0.05, 0.02) (tests/triangle_contacts_checker.py, other()), one query per triangle.
Timed between two device events, each as K chained calls after W warm-up calls, into preallocated outputs:
  count / write    the two passes of the C entry, each on its own, the offsets scanned once beforehand;
                   `given`: the queries in the mesh's own order, `sorted`: the same queries already in Morton order
  mirror           triangle_contacts(...) as a user calls it: Morton sort of the first vertices, count, scan, the read of the
                   total, write — its events bracket host work too; `presorted`: the same without the sort
  self            self_intersections(...) on the two meshes joined into one (twice the triangles, its own BVH, built
                   outside the timing): the mirror with ids and the shared-vertex rule
Before anything is timed the sorted and the given order must give the same lists.  The comparison on the same queries:
  traverse + torch   what a user does without this query: a BVH over the queries' boxes, traverse(bvh_queries, bvh_mesh)
                     for the (query box, triangle box) candidates, then include/ibvh.h's box clause and six edge tests as
                     torch operations on the candidate list; timed with and without the query build; its contacts must be
                     the library's as a set of (query, triangle) pairs
Prints one JSON line.  bench.py is not involved."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

from bench_closest import _dot, mesh  # noqa: E402
from bench_sphere_contacts import timed  # noqa: E402

NAME = "ibvh_triangle_contacts"
ANGLE, SHIFT = 0.5, (0.9, 0.05, 0.02)


def other(tris):
    """tests/triangle_contacts_checker.py's other(): the rigid transform of the mesh, in float64, cast back"""
    p = tris.astype(np.float64).reshape(-1, 3)
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    out = np.stack([p[:, 0] + SHIFT[0], c * p[:, 1] - s * p[:, 2] + SHIFT[1], s * p[:, 1] + c * p[:, 2] + SHIFT[2]], axis=1)
    return out.reshape(-1, 9).astype(tris.dtype)


class Query:
    """both passes of the C entry on one batch, into preallocated buffers, nothing read back while timed; q: (N, 9)"""

    def __init__(self, bvh, tdev, q):
        n = q.shape[0]
        self.bvh, self.tdev, self.q, self.n = bvh.struct(), tdev, q, n
        self.counts = torch.empty(n, dtype=torch.int64, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.count()
        self.offsets = torch.cumsum(self.counts, 0) - self.counts
        self.total = int(self.counts.sum().item())
        m = max(self.total, 1)
        self.index = torch.empty(m, dtype=torch.int32, device="cuda")
        self.mask = torch.empty(m, dtype=torch.uint8, device="cuda")
        self.points = torch.empty((m, 2, 3), dtype=torch.float32, device="cuda")
        self.write()
        torch.cuda.synchronize()
        assert self.flag.item() == 0

    def _call(self, mode, counts, offsets, capacity, outs):
        lib.call(NAME, C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.q), None, self.n, mode, 0,
                 counts, offsets, capacity, *outs, api._ptr(self.flag), api._stream())

    def count(self):
        self._call(abi.TRIS_COUNT, api._ptr(self.counts), None, 0, (None, None, None))

    def write(self):
        self._call(abi.TRIS_WRITE, None, api._ptr(self.offsets), self.index.shape[0],
                   [C.c_void_p(x.data_ptr()) for x in (self.index, self.mask, self.points)])

    def pairs(self, order=None):
        """the contacts as sorted keys query * 2^32 + triangle (order: the permutation this batch was walked in)"""
        s = torch.repeat_interleave(torch.arange(self.n, device="cuda"), self.counts)
        s = s if order is None else order[s]
        return torch.sort((s << 32) | self.index[:self.total].to(torch.int64)).values


def _cross(x, y):
    return torch.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], dim=1)


def _seg(p0, p1, tri):
    """include/ibvh.h's edge test as torch operations: the ray test with d = p1 - p0 against tri, and t <= 1"""
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    d = p1 - p0
    e1, e2 = b - a, c - a
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    inv = 1 / det
    tv = p0 - a
    u = _dot(tv, pv) * inv
    qv = _cross(tv, e1)
    v = _dot(d, qv) * inv
    t = _dot(e2, qv) * inv
    return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def _box(t):
    a, b, c = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    lo = torch.where(b < a, b, a)
    up = torch.where(b > a, b, a)
    return torch.where(c < lo, c, lo), torch.where(c > up, c, up)


def torch_narrow(tris, queries, qi, ti, chunk=4_000_000):
    """the box clause (tight boxes) and the six edge tests on the candidate pairs (qi[i], ti[i]), 0-based
    -> sorted keys query * 2^32 + (tri + 1) of the contacts"""
    keys = []
    for s in range(0, qi.shape[0], chunk):
        si, tt = qi[s:s + chunk], ti[s:s + chunk]
        q, k = queries[si], tris[tt]
        (qlo, qup), (lo, up) = _box(q), _box(k)
        hit = ~((qup < lo) | (qlo > up)).any(dim=1)
        qa, qb, qc, k1, k2, k3 = q[:, 0:3], q[:, 3:6], q[:, 6:9], k[:, 0:3], k[:, 3:6], k[:, 6:9]
        found = _seg(qa, qb, k) | _seg(qb, qc, k) | _seg(qc, qa, k) | _seg(k1, k2, q) | _seg(k2, k3, q) | _seg(k3, k1, q)
        hit &= found
        keys.append((si[hit] << 32) | (tt[hit] + 1))
    return torch.sort(torch.cat(keys)).values if keys else torch.empty(0, dtype=torch.int64, device="cuda")


def run(name, steps, warmup):
    tris, _ = mesh(name)
    f32 = ibvh.BBox(torch.float32)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, f32), f32)
    q = torch.from_numpy(other(tris)).cuda()
    m = int(q.shape[0])
    order = api._morton_order(q[:, :3])
    given, srt = Query(bvh, tdev, q), Query(bvh, tdev, q[order].contiguous())
    same = given.total == srt.total and torch.equal(given.pairs(), srt.pairs(order))
    bits = [int(((given.mask[:given.total] >> b) & 1).sum().item()) for b in range(6)]
    out = {"workload": name, "triangles": int(tdev.shape[0]), "queries": m, "levels": int(bvh.tree.levels), "contacts": given.total,
           "queries_with_contacts": int((given.counts > 0).sum().item()), "largest_list": int(given.counts.max().item()),
           "per_bit": bits, "sorted_equals_given": bool(same)}
    mirror = lambda: ibvh.triangle_contacts(bvh, tdev, q)
    mirror_count = lambda: ibvh.triangle_contacts(bvh, tdev, q, count_only=True)
    mirror_given = lambda: ibvh.triangle_contacts(bvh, tdev, q, presorted=True)
    for _ in range(warmup):
        for f in (given.count, given.write, srt.count, srt.write, mirror, mirror_count, mirror_given):
            f()
    for key, f in (("count_given_ms", given.count), ("write_given_ms", given.write), ("count_sorted_ms", srt.count),
                   ("write_sorted_ms", srt.write)):
        out[key] = round(timed(f, steps), 4)
    out["mirror_ms"] = round(timed(mirror, max(2, steps // 2)), 4)
    out["mirror_count_only_ms"] = round(timed(mirror_count, max(2, steps // 2)), 4)
    out["mirror_presorted_ms"] = round(timed(mirror_given, max(2, steps // 2)), 4)

    # ---- what a user does without the query: a BVH over the queries, the pair traversal, the arithmetic in torch -------
    qvols = ibvh.bounding_volumes_from_triangles(q, f32)
    state = {}

    def build_queries():
        state["bvh"] = ibvh.BVH(qvols, f32)

    def candidates_and_narrow():
        cand = ibvh.traverse(state["bvh"], bvh).contacts
        state["candidates"] = int(cand.shape[0])
        state["keys"] = torch_narrow(tdev, q, cand[:, 0].to(torch.int64) - 1, cand[:, 1].to(torch.int64) - 1)

    def whole():
        build_queries()
        candidates_and_narrow()
    for _ in range(max(1, warmup - 1)):
        whole()
    k = max(2, steps // 4)
    out["traverse_torch"] = {"query_build_ms": round(timed(build_queries, k), 4),
                             "traverse_and_torch_ms": round(timed(candidates_and_narrow, k), 4),
                             "build_traverse_and_torch_ms": round(timed(whole, k), 4), "candidates": state["candidates"],
                             "contacts": int(state["keys"].shape[0]),
                             "same_pairs_as_library": bool(state["keys"].shape[0] == given.total and torch.equal(state["keys"], given.pairs()))}
    del state

    # ---- one mesh against itself: the two meshes joined ------------------------------------------------------------------
    both = torch.cat([tdev, q]).contiguous()
    bvh2 = ibvh.BVH(ibvh.bounding_volumes_from_triangles(both, f32), f32)
    selfq = lambda: ibvh.self_intersections(bvh2, both)
    got = selfq()
    for _ in range(warmup):
        selfq()
    out["self"] = {"triangles": int(both.shape[0]), "pairs": int(got.index.shape[0]), "self_intersections_ms": round(timed(selfq, max(2, steps // 2)), 4),
                   "same_pairs_as_other_against_mesh": bool(int(got.index.shape[0]) == given.total)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"bench_triangle_contacts": [run(n, a.steps, a.warmup) for n in a.workloads.split(",") if n]}
    print(json.dumps(out), flush=True)
    if not all(w["sorted_equals_given"] for w in out["bench_triangle_contacts"]):
        raise SystemExit("the sorted and the given order give different lists: the times are not like for like")
    if not all(w["traverse_torch"]["same_pairs_as_library"] for w in out["bench_triangle_contacts"]):
        raise SystemExit("traverse + torch and the library give different sets of pairs")


if __name__ == "__main__":
    main()
