"""The closest-point query (ibvh_closest_triangles) on the benchmark meshes.

    python tools/bench_closest.py [--workloads published,config3] [--steps K] [--warmup W] [--no-torch]

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks), 100,000 points
  config3    the 7.2 M-triangle torus (bench.py's surface), 1e6 points
Point sets: `box` — uniform in the mesh's box inflated by 25 % each way; `near` — within three mean edge lengths of the
surface (a random barycentric point of a random triangle plus a random offset).
Timed per set, each as K chained calls between two device synchronisations after W warm-up calls, into preallocated outputs:
  given      the one launch, points in the order they were drawn (no coherence between the lanes of a wave)
  sorted     the one launch, the same points already in Morton order
  mirror     closest_points(...) as a user calls it: Morton sort of the points, the launch, the flag read, the un-permute
each unbounded and with max_distance = three mean edge lengths.  Before anything is timed the sorted and the given order must
give the same bits.  `torch`: the same arithmetic as torch operations, brute force over ALL triangles, at 3,200 triangles and
10,000 points only (it is O(n m)); compared bit for bit with the library, then timed — a sanity ratio, not a baseline at
size.  Prints one JSON line.  bench.py is not involved."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import api, lib  # noqa: E402
from implicitbvh_amd.synthetic import torus_mesh  # noqa: E402


def mesh(name):
    if name == "config3":
        return torus_mesh(), 1_000_000
    if name == "published":
        n = 249_882
        u = int(np.sqrt(n / 2)) + 2
        return torus_mesh(u, u)[:n], 100_000
    if name == "small":
        return torus_mesh(40, 40), 10_000
    raise SystemExit(f"unknown workload {name}")


def point_sets(tris, m, seed=43):
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = hi - lo
    box = (lo - 0.25 * ext) + 1.5 * ext * rng.random((m, 3))
    t = tris[rng.integers(0, len(tris), m)].reshape(-1, 3, 3).astype(np.float64)
    edge = float(np.linalg.norm(t[:, 1] - t[:, 0], axis=1).mean())
    w = rng.dirichlet((1.0, 1.0, 1.0), m)
    off = rng.normal(size=(m, 3))
    off *= (3 * edge * rng.random((m, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
    near = (w[:, :, None] * t).sum(axis=1) + off
    return {"box": box.astype(np.float32), "near": near.astype(np.float32)}, edge


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3, out


class Query:
    """the one launch into preallocated outputs, nothing read back; p: (N, 3) row-major"""

    def __init__(self, bvh, tdev, p, radius):
        n = p.shape[0]
        self.bvh, self.tdev, self.p = bvh.struct(), tdev, p
        self.index = torch.empty(n, dtype=torch.int32, device="cuda")
        self.d2 = torch.empty(n, dtype=torch.float32, device="cuda")
        self.q = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.r2 = None if radius is None else C.c_float(np.float32(radius) * np.float32(radius))

    def __call__(self):
        lib.call("ibvh_closest_triangles", C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.p), self.p.shape[0],
                 None if self.r2 is None else C.byref(self.r2), api._ptr(self.index), api._ptr(self.d2), api._ptr(self.q),
                 api._ptr(self.flag), api._stream())


def _same(a, b, order):
    return (torch.equal(a.index, b.index[order]) and torch.equal(a.d2.view(torch.int32), b.d2[order].view(torch.int32))
            and torch.equal(a.q.view(torch.int32), b.q[order].view(torch.int32)))


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def torch_brute_force(tris, p, chunk=2000):
    """include/ibvh.h's evaluation as torch operations over ALL (point, triangle) pairs, then the lexicographic minimum"""
    a, b, c = tris[None, :, 0:3], tris[None, :, 3:6], tris[None, :, 6:9]
    ab, ac = b - a, c - a
    lo = torch.where(a < b, torch.where(a < c, a, c), torch.where(b < c, b, c))
    up = torch.where(a > b, torch.where(a > c, a, c), torch.where(b > c, b, c))
    index, dist2, point = [], [], []
    for s in range(0, p.shape[0], chunk):
        pp = p[s:s + chunk, None, :]
        ap, bp, cp = pp - a, pp - b, pp - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        c0 = (d1 <= 0) & (d2 <= 0)
        c1 = (d3 >= 0) & (d4 <= d3)
        c2 = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        c3 = (d6 >= 0) & (d5 <= d6)
        c4 = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        c5 = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        den = 1 / ((va + vb) + vc)
        q = (a + (vb * den)[..., None] * ab) + (vc * den)[..., None] * ac
        q = torch.where(c5[..., None], b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b), q)
        q = torch.where(c4[..., None], a + (d2 / (d2 - d6))[..., None] * ac, q)
        q = torch.where(c3[..., None], c.expand_as(q), q)
        q = torch.where(c2[..., None], a + (d1 / (d1 - d3))[..., None] * ab, q)
        q = torch.where(c1[..., None], b.expand_as(q), q)
        q = torch.where(c0[..., None], a.expand_as(q), q)
        q = torch.where(q < lo, lo, torch.where(q > up, up, q))
        e = pp - q
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        key = torch.where(dd == dd, dd, torch.full_like(dd, float("inf")))
        best, k = key.min(dim=1, keepdim=True)
        k = ((key == best) & (dd == dd)).to(torch.int8).argmax(dim=1)  # the smallest index among the minima
        rows = torch.arange(k.shape[0], device=k.device)
        index.append((k + 1).to(torch.int32))
        dist2.append(dd[rows, k])
        point.append(q[rows, k])
    return torch.cat(index), torch.cat(dist2), torch.cat(point)


def run(name, steps, warmup):
    tris, m = mesh(name)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    sets, edge = point_sets(tris, m)
    out = {"workload": name, "triangles": int(tdev.shape[0]), "points": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6), "sets": {}}
    for sname, ph in sets.items():
        p = torch.from_numpy(ph).cuda()
        order = api._morton_order(p)
        ps = p[order].contiguous()
        res = {}
        for rname, radius in (("unbounded", None), ("bounded", 3 * edge)):
            given, srt = Query(bvh, tdev, p, radius), Query(bvh, tdev, ps, radius)
            given()
            srt()
            torch.cuda.synchronize()
            assert given.flag.item() == 0 and srt.flag.item() == 0
            same = _same(srt, given, order)
            mirror = lambda: ibvh.closest_points(bvh, tdev, p.t(), max_distance=radius)
            for _ in range(warmup):
                given()
                srt()
                mirror()
            ms_given, _ = timed(given, steps)
            ms_sorted, _ = timed(srt, steps)
            ms_mirror, _ = timed(mirror, max(2, steps // 2))
            res[rname] = {"given_ms": round(ms_given, 4), "sorted_ms": round(ms_sorted, 4), "mirror_ms": round(ms_mirror, 4),
                          "answered": int((given.index > 0).sum().item()), "sorted_equals_given": bool(same)}
        out["sets"][sname] = res
    return out


def torch_ratio(steps, warmup):
    tris, m = mesh("small")
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    sets, _ = point_sets(tris, m)
    p = torch.from_numpy(sets["near"]).cuda()
    q = Query(bvh, tdev, p, None)
    q()
    index, d2, point = torch_brute_force(tdev, p)
    torch.cuda.synchronize()
    equal = (torch.equal(q.index, index) and torch.equal(q.d2.view(torch.int32), d2.view(torch.int32))
             and torch.equal(q.q.view(torch.int32), point.view(torch.int32)))
    for _ in range(warmup):
        q()
    torch_brute_force(tdev, p)
    ms_lib, _ = timed(q, steps)
    ms_torch, _ = timed(lambda: torch_brute_force(tdev, p), 2)
    return {"triangles": int(tdev.shape[0]), "points": m, "library_ms": round(ms_lib, 4), "torch_brute_force_ms": round(ms_torch, 3),
            "torch_over_library": round(ms_torch / ms_lib, 1), "torch_equal": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    out = {"bench_closest": [run(n, a.steps, a.warmup) for n in a.workloads.split(",") if n]}
    if not a.no_torch:
        out["torch_sanity"] = torch_ratio(a.steps, a.warmup)
    print(json.dumps(out))
    ok = all(r["sorted_equals_given"] for w in out["bench_closest"] for s in w["sets"].values() for r in s.values())
    if not ok or not out.get("torch_sanity", {"torch_equal": True})["torch_equal"]:
        raise SystemExit("results differ between orders or from the torch brute force: the times are not like for like")


if __name__ == "__main__":
    main()
