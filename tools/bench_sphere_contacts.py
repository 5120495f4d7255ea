"""The sphere-vs-mesh contact query (ibvh_sphere_contacts) on the benchmark meshes, beside the two ways to get there without it.

    python tools/bench_sphere_contacts.py [--workloads published,config3] [--steps K] [--warmup W]

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks), 100,000 spheres
  config3    the 7.2 M-triangle torus (bench.py's surface), 1e6 spheres
Spheres: centres within three mean edge lengths of the surface (a random barycentric point of a random triangle plus a random
offset), radii uniform in one to three mean edge lengths.
Timed between two device events, each as K chained calls after W warm-up calls, into preallocated outputs:
  count / write    the two passes of the C entry, each on its own, the offsets scanned once beforehand;
                   `given`: spheres in the order they were drawn (no coherence between the lanes of a wave),
                   `sorted`: the same spheres already in Morton order
  mirror           sphere_contacts(...) as a user calls it: Morton sort of the centres, count, scan, the read of the total,
                   write — its events bracket host work too
Before anything is timed the sorted and the given order must give the same lists.  Two comparisons on the same spheres:
  traverse + torch   what a user does without this query: a BSphere BVH over the spheres, traverse(bvh_spheres, bvh_mesh)
                     (mixed types) for the (sphere, triangle box) candidates, then include/ibvh.h's evaluation as torch
                     operations on the candidate list and the d2 <= r * r filter; timed with and without the sphere build;
                     its contacts are compared with the library's as sets of (sphere, triangle) pairs
  closest_points     closest_points(max_distance=r) at ONE radius (two mean edge lengths) on the same centres — the same walk
                     with a shrinking bound and one answer per point — against count + write at that scalar radius
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

NAME = "ibvh_sphere_contacts"


def spheres_near(tris, m, seed=47):
    """-> centres (m, 3), radii (m,) float32, the mean edge length"""
    rng = np.random.default_rng(seed)
    t = tris[rng.integers(0, len(tris), m)].reshape(-1, 3, 3).astype(np.float64)
    edge = float(np.linalg.norm(t[:, 1] - t[:, 0], axis=1).mean())
    w = rng.dirichlet((1.0, 1.0, 1.0), m)
    off = rng.normal(size=(m, 3))
    off *= (3 * edge * rng.random((m, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
    c = (w[:, :, None] * t).sum(axis=1) + off
    r = edge * (1 + 2 * rng.random(m))
    return c.astype(np.float32), r.astype(np.float32), edge


def timed(fn, k):
    """ms per call of k chained calls, between two device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(k):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / k


class Query:
    """both passes of the C entry on one batch, into preallocated buffers, nothing read back while timed; c: (N, 3) row-major"""

    def __init__(self, bvh, tdev, c, r):
        n = c.shape[0]
        self.bvh, self.tdev, self.c, self.r, self.n = bvh.struct(), tdev, c, r, n
        self.counts = torch.empty(n, dtype=torch.int64, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.count()
        self.offsets = torch.cumsum(self.counts, 0) - self.counts
        self.total = int(self.counts.sum().item())
        m = max(self.total, 1)
        self.index = torch.empty(m, dtype=torch.int32, device="cuda")
        self.d2 = torch.empty(m, dtype=torch.float32, device="cuda")
        self.q = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        self.region = torch.empty(m, dtype=torch.uint8, device="cuda")
        self.write()
        torch.cuda.synchronize()
        assert self.flag.item() == 0

    def _call(self, mode, counts, offsets, capacity, outs):
        lib.call(NAME, C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.c), api._ptr(self.r), self.n, mode,
                 counts, offsets, capacity, *outs, api._ptr(self.flag), api._stream())

    def count(self):
        self._call(abi.SPHERES_COUNT, api._ptr(self.counts), None, 0, (None, None, None, None))

    def write(self):
        self._call(abi.SPHERES_WRITE, None, api._ptr(self.offsets), self.index.shape[0],
                   [C.c_void_p(x.data_ptr()) for x in (self.index, self.d2, self.q, self.region)])

    def pairs(self, order=None):
        """the contacts as sorted keys sphere * 2^32 + triangle (order: the permutation this batch was walked in)"""
        s = torch.repeat_interleave(torch.arange(self.n, device="cuda"), self.counts)
        s = s if order is None else order[s]
        return torch.sort((s << 32) | self.index[:self.total].to(torch.int64)).values


def torch_narrow(tris, c, r2, sphere, tri, chunk=4_000_000):
    """include/ibvh.h's evaluation as torch operations on the candidate pairs (sphere[i], tri[i]), 0-based, then d2 <= r2
    -> sorted keys sphere * 2^32 + (tri + 1) of the contacts"""
    keys = []
    for s in range(0, sphere.shape[0], chunk):
        si, ti = sphere[s:s + chunk], tri[s:s + chunk]
        t = tris[ti]
        a, b, cc = t[:, 0:3], t[:, 3:6], t[:, 6:9]
        ab, ac = b - a, cc - a
        lo = torch.where(a < b, torch.where(a < cc, a, cc), torch.where(b < cc, b, cc))
        up = torch.where(a > b, torch.where(a > cc, a, cc), torch.where(b > cc, b, cc))
        pp = c[si]
        ap, bp, cp = pp - a, pp - b, pp - cc
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        c0 = (d1 <= 0) & (d2 <= 0)
        c1 = (d3 >= 0) & (d4 <= d3)
        c2 = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        c3 = (d6 >= 0) & (d5 <= d6)
        c4 = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        c5 = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        den = 1 / ((va + vb) + vc)
        q = (a + (vb * den)[:, None] * ab) + (vc * den)[:, None] * ac
        q = torch.where(c5[:, None], b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (cc - b), q)
        q = torch.where(c4[:, None], a + (d2 / (d2 - d6))[:, None] * ac, q)
        q = torch.where(c3[:, None], cc, q)
        q = torch.where(c2[:, None], a + (d1 / (d1 - d3))[:, None] * ab, q)
        q = torch.where(c1[:, None], b, q)
        q = torch.where(c0[:, None], a, q)
        q = torch.where(q < lo, lo, torch.where(q > up, up, q))
        e = pp - q
        dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        hit = dd <= r2[si]
        keys.append((si[hit] << 32) | (ti[hit] + 1))
    return torch.sort(torch.cat(keys)).values if keys else torch.empty(0, dtype=torch.int64, device="cuda")


def run(name, steps, warmup):
    tris, m = mesh(name)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    ch, rh, edge = spheres_near(tris, m)
    c, r = torch.from_numpy(ch).cuda(), torch.from_numpy(rh).cuda()
    order = api._morton_order(c)
    given, srt = Query(bvh, tdev, c, r), Query(bvh, tdev, c[order].contiguous(), r[order].contiguous())
    same = given.total == srt.total and torch.equal(given.pairs(), srt.pairs(order))
    out = {"workload": name, "triangles": int(tdev.shape[0]), "spheres": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6),
           "contacts": given.total, "contacts_per_sphere": round(given.total / m, 2), "largest_list": int(given.counts.max().item()),
           "spheres_without": int((given.counts == 0).sum().item()), "sorted_equals_given": bool(same)}
    mirror = lambda: ibvh.sphere_contacts(bvh, tdev, c.t(), r)
    mirror_count = lambda: ibvh.sphere_contacts(bvh, tdev, c.t(), r, count_only=True)
    for _ in range(warmup):
        for f in (given.count, given.write, srt.count, srt.write, mirror, mirror_count):
            f()
    for key, f in (("count_given_ms", given.count), ("write_given_ms", given.write), ("count_sorted_ms", srt.count),
                   ("write_sorted_ms", srt.write)):
        out[key] = round(timed(f, steps), 4)
    out["mirror_ms"] = round(timed(mirror, max(2, steps // 2)), 4)
    out["mirror_count_only_ms"] = round(timed(mirror_count, max(2, steps // 2)), 4)

    # ---- what a user does without the query: sphere BVH, mixed-type pair traversal, the arithmetic in torch ----------
    vols = torch.cat([c, r[:, None]], dim=1).contiguous()
    r2 = r * r
    state = {}

    def build_spheres():
        state["bvh"] = ibvh.BVH(vols, ibvh.BBox(torch.float32))

    def candidates_and_narrow():
        trav = ibvh.traverse(state["bvh"], bvh)
        cand = trav.contacts
        state["candidates"] = int(cand.shape[0])
        state["keys"] = torch_narrow(tdev, c, r2, cand[:, 0].to(torch.int64) - 1, cand[:, 1].to(torch.int64) - 1)

    def whole():
        build_spheres()
        candidates_and_narrow()
    for _ in range(max(1, warmup - 1)):
        whole()
    k = max(2, steps // 4)
    out["traverse_torch"] = {"sphere_build_ms": round(timed(build_spheres, k), 4),
                             "traverse_and_torch_ms": round(timed(candidates_and_narrow, k), 4),
                             "build_traverse_and_torch_ms": round(timed(whole, k), 4), "candidates": state["candidates"],
                             "contacts": int(state["keys"].shape[0]),
                             "same_pairs_as_library": bool(state["keys"].shape[0] == given.total and torch.equal(state["keys"], given.pairs()))}
    del state

    # ---- the same walk with a shrinking bound: one answer per point, one scalar radius ---------------------------------
    radius = np.float32(2 * edge)
    cs = c[order].contiguous()
    scalar = Query(bvh, tdev, cs, torch.full((m,), float(radius), dtype=torch.float32, device="cuda"))
    ci = torch.empty(m, dtype=torch.int32, device="cuda")
    cd = torch.empty(m, dtype=torch.float32, device="cuda")
    cq = torch.empty((m, 3), dtype=torch.float32, device="cuda")
    fl = torch.zeros(1, dtype=torch.int32, device="cuda")
    r2c = C.c_float(radius * radius)
    bs = bvh.struct()
    closest = lambda: lib.call("ibvh_closest_triangles", C.byref(bs), api._ptr(tdev), tdev.shape[0], api._ptr(cs), m, C.byref(r2c), api._ptr(ci),
                               api._ptr(cd), api._ptr(cq), api._ptr(fl), api._stream())
    for _ in range(warmup):
        closest()
        scalar.count()
        scalar.write()
    out["scalar_radius"] = {"radius_in_edges": 2, "closest_points_sorted_ms": round(timed(closest, steps), 4),
                            "count_sorted_ms": round(timed(scalar.count, steps), 4), "write_sorted_ms": round(timed(scalar.write, steps), 4),
                            "contacts": scalar.total, "points_answered": int((ci > 0).sum().item()),
                            "spheres_with_contacts": int((scalar.counts > 0).sum().item())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"bench_sphere_contacts": [run(n, a.steps, a.warmup) for n in a.workloads.split(",") if n]}
    print(json.dumps(out), flush=True)
    if not all(w["sorted_equals_given"] for w in out["bench_sphere_contacts"]):
        raise SystemExit("the sorted and the given order give different lists: the times are not like for like")
    for w in out["bench_sphere_contacts"]:
        s = w["scalar_radius"]
        if s["points_answered"] != s["spheres_with_contacts"]:
            raise SystemExit("closest_points and sphere_contacts disagree on which centres have a triangle within the radius")


if __name__ == "__main__":
    main()
