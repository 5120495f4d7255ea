"""The ray-triangle resolve pass (ibvh_rays_resolve_triangles) against the traversal in front of it and against the torch
plumbing a user needs without it.

    python tools/bench_rays_resolve.py [--workloads config3,published] [--leaves bsphere|bbox] [--steps K] [--warmup W]
    python tools/bench_rays_resolve.py --profile closest|all --workloads config3 [--steps K]   (the program to put under rocprofv3)

Workloads (BSphere{Float32} leaves from the triangles — bench.py's; --leaves bbox: BBox{Float32} leaves, whose tighter volumes
leave fewer than half the candidates per ray — BBox{Float32} nodes, Int32 indices, random rays in the box of the leaf centres):
  config3    the 7.2 M-triangle torus under 1e6 rays (bench.py's config 3, tools/bench_rays_config3.py)
  published  249,882 triangles under 100,000 rays (the size of the reference's published ray benchmark)
Timed, each as K chained calls between two device synchronisations after W warm-up calls:
  traverse        traverse_rays(...; cache=previous) and the host's read of the count           (what the list costs today)
  resolve         the resolve pass alone, closest hit only (index, t, uv), into preallocated outputs
  resolve_all     the same with cand_t (t of every exact hit)
  torch           the same arithmetic as torch operations on the same list: gather the triangles and the rays per candidate,
                  elementwise Moeller-Trumbore (no fused operations: the same bits), scatter_reduce(amin) per ray, and the tie
                  resolution (the earliest candidate among those that reach the minimum); compared bit for bit with the
                  library's result before anything is timed (a difference is reported and fails the run after the line)
Reported: candidates per ray, the byte floor H (8 + 36) + R (24 + 4 + 16) (+ 4 H with cand_t) for H candidates and R rays
(one pass over the list and its triangles, the rays, their counts and the outputs; a triangle shared by neighbouring rays
is counted once per candidate, so the floor is generous where the caches serve repeats), the achieved bytes/s against it,
and the resolve as a fraction of the traversal.  Prints one JSON line.  bench.py is not involved."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api  # noqa: E402
from implicitbvh_amd.synthetic import random_rays, torus_mesh  # noqa: E402


def workload(name, leaves="bsphere"):
    if name == "config3":
        tris, nr = torus_mesh(), 1_000_000
    elif name == "published":
        n = 249_882
        u = int(np.sqrt(n / 2)) + 2
        tris, nr = torus_mesh(u, u)[:n], 100_000
    else:
        raise SystemExit(f"unknown workload {name}")
    tdev = torch.from_numpy(tris).cuda()
    centres = ibvh.bounding_volumes_from_triangles(tdev)[:, :3]
    lo, hi = centres.min(0).values.cpu().numpy(), centres.max(0).values.cpu().numpy()
    if leaves == "bbox":
        bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    else:
        bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev))
    ph, dh = random_rays(nr, lo, hi, seed=43)
    return bvh, tdev, torch.from_numpy(ph).cuda(), torch.from_numpy(dh).cuda()


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3, out


def _cross(x, y):
    return torch.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                        x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], dim=1)


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def torch_resolve(tris, p, d, contacts, total):
    """What a user writes today over the (leaf.index, iray) list: the arithmetic of include/ibvh.h as torch operations."""
    c = contacts[:total]
    nr, inf = p.shape[0], float("inf")
    tri = tris[c[:, 0].long() - 1]
    ray = c[:, 1].long() - 1
    pp, dd = p[ray], d[ray]
    a = tri[:, 0:3]
    e1, e2 = tri[:, 3:6] - a, tri[:, 6:9] - a
    pv = _cross(dd, e2)
    det = _dot(e1, pv)
    inv = 1 / det
    tv = pp - a
    u = _dot(tv, pv) * inv
    qv = _cross(tv, e1)
    v = _dot(dd, qv) * inv
    t = _dot(e2, qv) * inv
    hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
    tt = torch.where(hit, t, torch.full_like(t, inf))
    best = torch.full((nr,), inf, dtype=t.dtype, device=t.device).scatter_reduce(0, ray, tt, "amin")
    # the tie rule: among the hits that reach the minimum, the earliest candidate
    k = torch.arange(total, device=t.device)
    first = torch.full((nr,), total, dtype=torch.int64, device=t.device).scatter_reduce(
        0, ray, torch.where(hit & (tt == best[ray]), k, torch.full_like(k, total)), "amin")
    has = first < total
    w = first.clamp(max=max(total - 1, 0))
    index = torch.where(has, c[w, 0], torch.zeros_like(c[w, 0]))
    tw = torch.where(has, tt[w], torch.full_like(tt[w], inf))
    uv = torch.where(has[:, None], torch.stack([u[w], v[w]], dim=1), torch.zeros((nr, 2), dtype=t.dtype, device=t.device))
    return index, tw, uv, tt


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Resolve:
    """the resolve pass into preallocated outputs, nothing read back (api._resolve_enqueue: one C call)"""

    def __init__(self, trav, tdev, p, d, with_cand):
        nr = p.shape[0]
        self.args = (abi.F32, tdev, p, d, trav.cache2[:nr], trav.cache1)
        self.index = torch.empty(nr, dtype=trav.cache1.dtype, device="cuda")
        self.t = torch.empty(nr, dtype=torch.float32, device="cuda")
        self.uv = torch.empty((nr, 2), dtype=torch.float32, device="cuda")
        self.cand = torch.empty(trav.cache1.shape[0], dtype=torch.float32, device="cuda") if with_cand else None
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def __call__(self):
        api._resolve_enqueue(*self.args, self.index, self.t, self.uv, self.cand, self.flag)


def run(name, leaves, steps, warmup):
    bvh, tdev, p, d = workload(name, leaves)
    P, D = p.t(), d.t()
    st = {"t": None}

    def traverse():
        st["t"] = ibvh.traverse_rays(bvh, P, D, cache=st["t"])
        return st["t"].num_contacts
    for _ in range(warmup):
        traverse()
    ms_trav, total = timed(traverse, steps)
    trav = st["t"]
    nr = p.shape[0]
    closest, everything = Resolve(trav, tdev, p, d, False), Resolve(trav, tdev, p, d, True)
    closest()
    everything()
    # the baseline must compute the same thing before its time means anything
    index, t, uv, tt = torch_resolve(tdev, p, d, trav.cache1, total)
    torch.cuda.synchronize()
    assert everything.flag.item() == 0 and closest.flag.item() == 0
    differ = {"index": int((everything.index != index).sum().item()),
              "t": int((everything.t.view(torch.int32) != t.view(torch.int32)).sum().item()),
              "uv": int((everything.uv.view(torch.int32) != uv.view(torch.int32)).any(dim=1).sum().item()),
              "cand_t": int((everything.cand[:total].view(torch.int32) != tt.view(torch.int32)).sum().item())}
    assert torch.equal(closest.index, everything.index) and _same_bits(closest.t, everything.t) and _same_bits(closest.uv, everything.uv)
    del index, t, uv, tt
    for _ in range(warmup):
        closest()
        everything()
        torch_resolve(tdev, p, d, trav.cache1, total)
    ms_closest, _ = timed(closest, steps)
    ms_all, _ = timed(everything, steps)
    ms_torch, _ = timed(lambda: torch_resolve(tdev, p, d, trav.cache1, total), max(2, steps // 4))
    floor = total * (8 + 36) + nr * (24 + 4 + 16)
    floor_all = floor + 4 * total
    return {"workload": name, "leaves": leaves, "triangles": int(tdev.shape[0]), "rays": nr, "candidates": int(total),
            "candidates_per_ray": round(total / nr, 3), "rays_hit": int((closest.index > 0).sum().item()),
            "exact_hits": int(torch.isfinite(everything.cand[:total]).sum().item()),
            "traverse_ms": round(ms_trav, 4), "resolve_ms": round(ms_closest, 4), "resolve_all_ms": round(ms_all, 4),
            "torch_ms": round(ms_torch, 4), "floor_bytes": floor, "floor_bytes_all": floor_all,
            "resolve_GBps_of_floor": round(floor / ms_closest / 1e6, 1), "resolve_all_GBps_of_floor": round(floor_all / ms_all / 1e6, 1),
            "resolve_over_traverse": round(ms_closest / ms_trav, 4), "resolve_all_over_traverse": round(ms_all / ms_trav, 4),
            "torch_over_resolve_all": round(ms_torch / ms_all, 2),
            # entries where the torch baseline's bits differ from the library's (all 0: it computes the same thing)
            "torch_equal": not any(differ.values()), "torch_differs": differ}


def profile(name, leaves, form, steps):
    bvh, tdev, p, d = workload(name, leaves)
    trav = ibvh.traverse_rays(bvh, p.t(), d.t())
    total = trav.num_contacts
    r = Resolve(trav, tdev, p, d, form == "all")
    for _ in range(steps):
        r()
    torch.cuda.synchronize()
    return {"workload": name, "profile": form, "resolves": steps, "candidates": int(total)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="config3,published")
    ap.add_argument("--leaves", choices=("bsphere", "bbox"), default="bsphere")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", choices=("closest", "all"))
    a = ap.parse_args()
    names = a.workloads.split(",")
    out = [profile(n, a.leaves, a.profile, a.steps) if a.profile else run(n, a.leaves, a.steps, a.warmup) for n in names]
    print(json.dumps({"bench_rays_resolve": out}))
    if not a.profile and not all(o["torch_equal"] for o in out):
        raise SystemExit("the torch baseline did not reproduce the library's result: its time is not a like-for-like baseline")


if __name__ == "__main__":
    main()
