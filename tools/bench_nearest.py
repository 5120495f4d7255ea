"""The k-nearest-leaves query (ibvh_nearest_leaves) on the benchmark's particle cloud.

    python tools/bench_nearest.py [--n 1000000] [--points 1000000] [--ks 1,8,16] [--steps K] [--warmup W] [--no-torch]

Workload: bench.py's cloud — n BSphere{Float32} leaves (generate_spheres, seed 42, the config-2 radius law) under BBox{Float32}
nodes, Int32 indices — and as many query points drawn uniformly in the unit cube (numpy, seed 43).
Timed per k, the launch ALONE between two device events (K chained launches after W warm-up launches, into preallocated
outputs, nothing read back), unbounded and with max_distance = three mean spacings (3 n^(-1/3)):
  sorted     the query points already in Morton order (what nearest_leaves hands the device)
  given      the same points in the order they were drawn (no coherence between the lanes of a wave): the unsorted penalty
  mirror     nearest_leaves(...) as a user calls it: Morton sort of the points, the launch, the un-permute (host clock
             around a synchronised call, k = 8 only)
Before anything is timed the sorted and the given order must give the same bits.  `torch`: a brute force as torch
operations — torch.cdist squared plus topk — at 20,000 leaves and 10,000 points (it is O(n m) in time and memory); at that
size the library's answer must be bit-equal to the numpy checker of the definition (tests/nearest_leaves_checker.py) and
the launch must be faster than the torch call (the ratio is printed).  How far torch's own answer is from the definition
(rows that name the same leaves in the same order, distances within rtol 1e-5) is printed as a figure, not required: cdist
is not the definition's arithmetic.  Prints one JSON line.  bench.py is not involved."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import api, lib  # noqa: E402


def cloud(n, seed=42):
    r0 = 0.5 * (3 * 8 / (4 * math.pi * n)) ** (1 / 3)
    return ibvh.generate_spheres(n, seed, r0=r0)


def event_ms(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / k


def host_ms(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


class Query:
    """the one launch into preallocated outputs, nothing read back; p: (N, 3) row-major"""

    def __init__(self, bvh, p, k, radius):
        n = p.shape[0]
        self.bvh, self.p, self.k = bvh.struct(), p, k
        self.index = torch.empty((n, k), dtype=torch.int32, device="cuda")
        self.d2 = torch.empty((n, k), dtype=torch.float32, device="cuda")
        self.r2 = None if radius is None else C.c_float(np.float32(radius) * np.float32(radius))

    def __call__(self):
        lib.call("ibvh_nearest_leaves", C.byref(self.bvh), api._ptr(self.p), self.p.shape[0], self.k,
                 None if self.r2 is None else C.byref(self.r2), api._ptr(self.index), api._ptr(self.d2), api._stream())


def _same(a, b, order):
    return torch.equal(a.index, b.index[order]) and torch.equal(a.d2.view(torch.int32), b.d2[order].view(torch.int32))


def run(n, m, ks, steps, warmup):
    vols = cloud(n)
    bvh = ibvh.BVH(vols, ibvh.BBox(torch.float32))
    p = torch.from_numpy(np.random.default_rng(43).random((m, 3)).astype(np.float32)).cuda()
    order = api._morton_order(p)
    ps = p[order].contiguous()
    spacing = n ** (-1 / 3)
    out = {"leaves": n, "points": m, "levels": int(bvh.tree.levels), "mean_spacing": round(spacing, 6), "k": {}}
    for k in ks:
        res = {}
        for rname, radius in (("unbounded", None), ("bounded", 3 * spacing)):
            given, srt = Query(bvh, p, k, radius), Query(bvh, ps, k, radius)
            given()
            srt()
            torch.cuda.synchronize()
            same = _same(srt, given, order)
            for _ in range(warmup):
                given()
                srt()
            ms_sorted, ms_given = event_ms(srt, steps), event_ms(given, steps)
            res[rname] = {"sorted_ms": round(ms_sorted, 4), "given_ms": round(ms_given, 4),
                          "given_over_sorted": round(ms_given / ms_sorted, 2),
                          "answers_per_point": round(float((srt.d2 < float("inf")).sum().item()) / m, 3),
                          "sorted_equals_given": bool(same)}
            if k == 8:
                mirror = lambda: ibvh.nearest_leaves(bvh, p.t(), k=k, max_distance=radius)
                mirror()
                res[rname]["mirror_ms"] = round(host_ms(mirror, max(2, steps // 2)), 4)
        out["k"][str(k)] = res
    return out


def torch_brute_force(centres, p, k):
    d2, j = torch.topk(torch.cdist(p, centres, compute_mode="donot_use_mm_for_euclid_dist") ** 2, k, dim=1, largest=False, sorted=True)
    return (j + 1).to(torch.int32), d2


def torch_ratio(steps, warmup, n=20_000, m=10_000, k=8):
    import nearest_leaves_checker as nlc
    vols = cloud(n)
    bvh = ibvh.BVH(vols, ibvh.BBox(torch.float32))
    ph = np.random.default_rng(44).random((m, 3)).astype(np.float32)
    p = torch.from_numpy(ph).cuda()
    ps = p[api._morton_order(p)].contiguous()
    q = Query(bvh, ps, k, None)
    q()
    torch.cuda.synchronize()
    vh, ph, gi, gd = vols.cpu().numpy(), ps.cpu().numpy(), q.index.cpu().numpy(), q.d2.cpu().numpy()
    equal = True
    for s in range(0, m, 1000):  # (the checker holds a points x leaves matrix: a thousand points at a time)
        exp = nlc.brute_force(vh, np.arange(1, n + 1), ph[s:s + 1000], k)
        equal = equal and bool((gi[s:s + 1000] == exp.index).all() and gd[s:s + 1000].tobytes() == exp.d2.tobytes())
    centres = vols[:, :3].contiguous()
    ti, td = torch_brute_force(centres, ps, k)
    # cdist is not the definition's arithmetic: how close it comes is reported, not required
    agree = float((ti == q.index).all(dim=1).float().mean().item())
    close = bool(torch.allclose(td, q.d2, rtol=1e-5, atol=1e-12))
    for _ in range(warmup):
        q()
    torch_brute_force(centres, ps, k)
    ms_lib = event_ms(q, steps)
    ms_torch = event_ms(lambda: torch_brute_force(centres, ps, k), 3)
    return {"leaves": n, "points": m, "k": k, "library_ms": round(ms_lib, 4), "torch_cdist_topk_ms": round(ms_torch, 3),
            "torch_over_library": round(ms_torch / ms_lib, 1), "library_equals_checker": equal,
            "torch_rows_with_the_same_indices": round(agree, 5), "torch_distances_close": close}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--ks", default="1,8,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    out = {"bench_nearest": run(a.n, a.points, [int(k) for k in a.ks.split(",") if k], a.steps, a.warmup)}
    if not a.no_torch:
        out["torch_brute_force"] = torch_ratio(a.steps, a.warmup)
    print(json.dumps(out))
    ok = all(r["sorted_equals_given"] for kr in out["bench_nearest"]["k"].values() for r in kr.values())
    t = out.get("torch_brute_force")
    if not ok or (t and not (t["library_equals_checker"] and t["torch_over_library"] > 1)):
        raise SystemExit("results differ between orders or from the checker, or the launch is not faster than the torch brute force")


if __name__ == "__main__":
    main()
