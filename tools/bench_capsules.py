"""The capsule-vs-mesh contact query (ibvh_capsule_contacts) and the segment-to-mesh distance (ibvh_segment_distances) on the
benchmark meshes, beside the way to get the contacts without them.

    python tools/bench_capsules.py [--workloads published,config3] [--steps K] [--warmup W]

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks), 100,000 capsules
  config3    the 7.2 M-triangle torus (bench.py's surface), 1e6 capsules
Capsules: starts within three mean edge lengths of the surface (a random barycentric point of a random triangle plus a random
offset), lengths uniform in 0 - 12 mean edge lengths in random directions, radii uniform in one to three mean edge lengths.
Timed between two device events, each as K chained calls after W warm-up calls, into preallocated outputs:
  count / write    the two passes of the C entry, each on its own, the offsets scanned once beforehand;
                   `given`: capsules in the order they were drawn (no coherence between the lanes of a wave),
                   `sorted`: the same capsules already in Morton order of their midpoints
  mirror           capsule_contacts(...) as a user calls it: Morton sort, count, scan, the read of the total, write — its
                   events bracket host work too
  distances        ibvh_segment_distances on the sorted segments, unbounded and within six mean edge lengths
Before anything is timed the sorted and the given order must give the same lists.  Two comparisons on the same capsules:
  traverse + torch   what a user does without this query: a BBox BVH over the capsules' boxes grown by their radii,
                     traverse(bvh_capsules, bvh_mesh) for the (capsule, triangle box) candidates, then include/ibvh.h's
                     segment-triangle evaluation as torch operations on the candidate list and the d2 <= r * r filter; timed
                     with and without the capsule build; its contacts are compared with the library's as sets of pairs
  sphere_contacts    the two passes of ibvh_sphere_contacts on the capsules' midpoints with the same radii, as context: the
                     same walk on a point bound, one fifth of the evaluation per visit
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

from bench_closest import mesh  # noqa: E402
from bench_sphere_contacts import Query as SphereQuery, timed  # noqa: E402
from bench_triangle_distances import _box, _point_triangle, _seg, _segments  # noqa: E402

NAME, DISTANCES = "ibvh_capsule_contacts", "ibvh_segment_distances"


def capsules_near(tris, m, seed=59):
    """-> starts (m, 3), ends (m, 3), radii (m,) float32, the mean edge length"""
    rng = np.random.default_rng(seed)
    t = tris[rng.integers(0, len(tris), m)].reshape(-1, 3, 3).astype(np.float64)
    edge = float(np.linalg.norm(t[:, 1] - t[:, 0], axis=1).mean())
    w = rng.dirichlet((1.0, 1.0, 1.0), m)
    off = rng.normal(size=(m, 3))
    off *= (3 * edge * rng.random((m, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
    a = (w[:, :, None] * t).sum(axis=1) + off
    d = rng.normal(size=(m, 3))
    d *= (12 * edge * rng.random((m, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    r = edge * (1 + 2 * rng.random(m))
    return a.astype(np.float32), (a + d).astype(np.float32), r.astype(np.float32), edge


class Query:
    """both passes of the C entry on one batch, into preallocated buffers, nothing read back while timed; a, b: (N, 3) row-major"""

    def __init__(self, bvh, tdev, a, b, r):
        n = a.shape[0]
        self.bvh, self.tdev, self.a, self.b, self.r, self.n = bvh.struct(), tdev, a, b, r, n
        self.counts = torch.empty(n, dtype=torch.int64, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.count()
        self.offsets = torch.cumsum(self.counts, 0) - self.counts
        self.total = int(self.counts.sum().item())
        m = max(self.total, 1)
        self.index = torch.empty(m, dtype=torch.int32, device="cuda")
        self.d2 = torch.empty(m, dtype=torch.float32, device="cuda")
        self.xs = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        self.xk = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        self.kind = torch.empty(m, dtype=torch.uint8, device="cuda")
        self.write()
        torch.cuda.synchronize()
        assert self.flag.item() == 0

    def _call(self, mode, counts, offsets, capacity, outs):
        lib.call(NAME, C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.a), api._ptr(self.b), api._ptr(self.r),
                 self.n, mode, counts, offsets, capacity, *outs, api._ptr(self.flag), api._stream())

    def count(self):
        self._call(abi.CAPSULES_COUNT, api._ptr(self.counts), None, 0, (None,) * 5)

    def write(self):
        self._call(abi.CAPSULES_WRITE, None, api._ptr(self.offsets), self.index.shape[0],
                   [C.c_void_p(x.data_ptr()) for x in (self.index, self.d2, self.xs, self.xk, self.kind)])

    def pairs(self, order=None):
        """the contacts as sorted keys capsule * 2^32 + triangle (order: the permutation this batch was walked in)"""
        s = torch.repeat_interleave(torch.arange(self.n, device="cuda"), self.counts)
        s = s if order is None else order[s]
        return torch.sort((s << 32) | self.index[:self.total].to(torch.int64)).values


def torch_narrow(tris, a, b, r2, capsule, tri, chunk=2_000_000):
    """include/ibvh.h's segment-triangle evaluation as torch operations on the candidate pairs (capsule[i], tri[i]), 0-based,
    then d2 <= r2 -> sorted keys capsule * 2^32 + (tri + 1) of the contacts"""
    keys = []
    for s in range(0, capsule.shape[0], chunk):
        si, ti = capsule[s:s + chunk], tri[s:s + chunk]
        k, pa, pb = tris[ti], a[si], b[si]
        d2 = _point_triangle(k, pa)[1]
        for cand in (_point_triangle(k, pb)[1], _segments(pa, pb, k[:, 0:3], k[:, 3:6])[2], _segments(pa, pb, k[:, 3:6], k[:, 6:9])[2],
                     _segments(pa, pb, k[:, 6:9], k[:, 0:3])[2]):
            d2 = torch.where(cand < d2, cand, d2)
        klo, kup = _box(k)
        slo, sup = torch.where(pa < pb, pa, pb), torch.where(pa > pb, pa, pb)
        near = ~((sup < klo) | (slo > kup)).any(dim=1)
        d2 = torch.where(near & _seg(pa, pb, k)[0], torch.zeros_like(d2), d2)
        hit = d2 <= r2[si]
        keys.append((si[hit] << 32) | (ti[hit] + 1))
    return torch.sort(torch.cat(keys)).values if keys else torch.empty(0, dtype=torch.int64, device="cuda")


def run(name, steps, warmup):
    tris, m = mesh(name)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    ah, bh, rh, edge = capsules_near(tris, m)
    a, b, r = torch.from_numpy(ah).cuda(), torch.from_numpy(bh).cuda(), torch.from_numpy(rh).cuda()
    order = api._morton_order(0.5 * a.double() + 0.5 * b.double())
    sa, sb, sr = a[order].contiguous(), b[order].contiguous(), r[order].contiguous()
    given, srt = Query(bvh, tdev, a, b, r), Query(bvh, tdev, sa, sb, sr)
    same = given.total == srt.total and torch.equal(given.pairs(), srt.pairs(order))
    out = {"workload": name, "triangles": int(tdev.shape[0]), "capsules": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6),
           "contacts": given.total, "contacts_per_capsule": round(given.total / m, 2), "largest_list": int(given.counts.max().item()),
           "capsules_without": int((given.counts == 0).sum().item()), "sorted_equals_given": bool(same),
           "kinds": torch.bincount(given.kind[:given.total].long(), minlength=6).tolist()}
    mirror = lambda: ibvh.capsule_contacts(bvh, tdev, a.t(), b.t(), r)
    mirror_count = lambda: ibvh.capsule_contacts(bvh, tdev, a.t(), b.t(), r, count_only=True)
    for _ in range(warmup):
        for f in (given.count, given.write, srt.count, srt.write, mirror, mirror_count):
            f()
    for key, f in (("count_given_ms", given.count), ("write_given_ms", given.write), ("count_sorted_ms", srt.count),
                   ("write_sorted_ms", srt.write)):
        out[key] = round(timed(f, steps), 4)
    out["mirror_ms"] = round(timed(mirror, max(2, steps // 2)), 4)
    out["mirror_count_only_ms"] = round(timed(mirror_count, max(2, steps // 2)), 4)

    # ---- the distance query on the sorted segments: unbounded, and within six edge lengths ------------------------------
    di = torch.empty(m, dtype=torch.int32, device="cuda")
    dd = torch.empty(m, dtype=torch.float32, device="cuda")
    ds, dk = torch.empty((m, 3), dtype=torch.float32, device="cuda"), torch.empty((m, 3), dtype=torch.float32, device="cuda")
    dkind = torch.empty(m, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(1, dtype=torch.int32, device="cuda")
    bs = bvh.struct()
    six = np.float32(6 * edge)
    r2six = C.c_float(six * six)
    distances = lambda radius2: lib.call(DISTANCES, C.byref(bs), api._ptr(tdev), tdev.shape[0], api._ptr(sa), api._ptr(sb), m, radius2,
                                         api._ptr(di), api._ptr(dd), api._ptr(ds), api._ptr(dk), api._ptr(dkind), api._ptr(fl), api._stream())
    unbounded, within = (lambda: distances(None)), (lambda: distances(C.byref(r2six)))
    for _ in range(warmup):
        unbounded()
        within()
    out["distances"] = {"unbounded_sorted_ms": round(timed(unbounded, steps), 4), "within_six_edges_sorted_ms": round(timed(within, steps), 4),
                        "answered_within_six_edges": int((di > 0).sum().item())}

    # ---- what a user does without the query: a box BVH of the grown boxes, pair traversal, the arithmetic in torch --------
    lo, up = torch.where(a < b, a, b) - r[:, None], torch.where(a > b, a, b) + r[:, None]
    vols = torch.cat([lo, up], dim=1).contiguous()
    r2 = r * r
    state = {}

    def build_capsules():
        state["bvh"] = ibvh.BVH(vols, ibvh.BBox(torch.float32))

    def candidates_and_narrow():
        trav = ibvh.traverse(state["bvh"], bvh)
        cand = trav.contacts
        state["candidates"] = int(cand.shape[0])
        state["keys"] = torch_narrow(tdev, a, b, r2, cand[:, 0].to(torch.int64) - 1, cand[:, 1].to(torch.int64) - 1)

    def whole():
        build_capsules()
        candidates_and_narrow()
    for _ in range(max(1, warmup - 1)):
        whole()
    k = max(2, steps // 4)
    out["traverse_torch"] = {"capsule_build_ms": round(timed(build_capsules, k), 4),
                             "traverse_and_torch_ms": round(timed(candidates_and_narrow, k), 4),
                             "build_traverse_and_torch_ms": round(timed(whole, k), 4), "candidates": state["candidates"],
                             "contacts": int(state["keys"].shape[0]),
                             "same_pairs_as_library": bool(state["keys"].shape[0] == given.total and torch.equal(state["keys"], given.pairs()))}
    del state

    # ---- context: spheres of the same radii on the midpoints ------------------------------------------------------------
    mid = (0.5 * sa + 0.5 * sb).contiguous()
    spheres = SphereQuery(bvh, tdev, mid, sr)
    for _ in range(warmup):
        spheres.count()
        spheres.write()
    out["sphere_contacts_on_midpoints"] = {"count_sorted_ms": round(timed(spheres.count, steps), 4),
                                           "write_sorted_ms": round(timed(spheres.write, steps), 4), "contacts": spheres.total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"bench_capsules": [run(n, a.steps, a.warmup) for n in a.workloads.split(",") if n]}
    print(json.dumps(out), flush=True)
    if not all(w["sorted_equals_given"] for w in out["bench_capsules"]):
        raise SystemExit("the sorted and the given order give different lists: the times are not like for like")
    if not all(w["traverse_torch"]["same_pairs_as_library"] for w in out["bench_capsules"]):
        raise SystemExit("the list route and the library disagree on the pairs")


if __name__ == "__main__":
    main()
