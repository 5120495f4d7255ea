"""Rays and swept spheres against the benchmark's sphere cloud (ibvh_cast_spheres), beside the route a user had before it: the
leaf-vs-tree ray traversal's list of every (leaf, ray) whose bounding sphere the whole line meets, reduced to the first hit in
torch — on the same rays, the same BVH, in the same process.

    python tools/bench_cast_spheres.py [--leaves 100000,1000000] [--steps K] [--warmup W]

The cloud is the bench line's: n random BSphere{Float32} (generate_spheres, seed 42, the config-2 radius law) under BBox{Float32}
nodes, Int32 indices; n queries whose origins are uniform in the cloud's box inflated by a tenth each way, displacements i.i.d.
uniform [0, 1) (the reference benchmark's rays).  Timed, each after W warm-up calls, the launch alone, K chained calls between
two DEVICE EVENTS, into preallocated outputs — every combination of
  given | sorted      the queries as drawn (no coherence between the lanes of a wave) | in Morton order of their origins
  closest | any       the first leaf and its time | only whether anything is touched
  free | unit         unbounded | t_max = 1
  ray | fat           r = 0 | r of one to three times the law's r0
and, between two device synchronisations by the host's clock (it reads the count on the host),
  list_route          traverse_rays(...; cache=previous) on the same rays, then steps 1 to 3 of include/ibvh.h on its list and a
                      segmented minimum of (t, index) in torch: r = 0, unbounded
  closest_given_ray_free_wall   the launch alone by the host's clock, for a like-for-like ratio against it
Before anything is timed the sorted and the given order must give the same bits and any-hit must equal closest-hit's mask.
The list route's candidate count is reported, and whether both routes name the same leaf for every ray: they may differ where
the traversal's rounded line test drops a grazing hit, or where a clamp of the definition moves a tie; those rays are counted.
Prints one JSON line.  bench.py is not involved."""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402
from implicitbvh_amd.synthetic import random_rays, sphere_radius_law  # noqa: E402

from bench_cast import event_timed  # noqa: E402
from bench_rays_resolve import timed  # noqa: E402


class Cast:
    """the one launch into preallocated outputs, nothing read back; p, d: (N, 3) row-major"""

    def __init__(self, bvh, p, d, r=None, t_max=None, any_hit=False):
        n = p.shape[0]
        self.bvh, self.p, self.d, self.r, self.t_max, self.any_hit = bvh.struct(), p, d, r, t_max, any_hit
        self.index = None if any_hit else torch.empty(n, dtype=torch.int32, device="cuda")
        self.t = None if any_hit else torch.empty(n, dtype=torch.float32, device="cuda")
        self.touched = torch.empty(n, dtype=torch.uint8, device="cuda") if any_hit else None

    def __call__(self):
        lib.call("ibvh_cast_spheres", C.byref(self.bvh), api._ptr(self.p), api._ptr(self.d), api._ptr(self.r), self.p.shape[0],
                 api._ptr(self.t_max), None, abi.SPHERECAST_ANY if self.any_hit else abi.SPHERECAST_CLOSEST, api._ptr(self.index),
                 api._ptr(self.t), api._ptr(self.touched), api._stream())


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def first_hits_of_list(contacts, vols, p, d):
    """steps 1 to 3 of include/ibvh.h (r = 0) on the traversal's (leaf, ray) list and the lexicographic minimum of (t, index)
    per ray -> index (N,) int64 (0 = miss), t (N,)"""
    leaf, ray = contacts[:, 0].long() - 1, contacts[:, 1].long() - 1
    c, R = vols[leaf, :3], vols[leaf, 3]
    P, D = p[ray], d[ray]
    m = P - c
    mm, S2, B, dd = _dot(m, m), R * R, _dot(m, D), _dot(D, D)
    disc = B * B - dd * (mm - S2)
    t = (-B - torch.sqrt(disc)) / dd
    inf = torch.full_like(t, float("inf"))
    tk = torch.where(mm <= S2, torch.zeros_like(t), torch.where((mm > S2) & (dd > 0) & (disc >= 0) & (t >= 0), t, inf))
    n = p.shape[0]
    best = torch.full((n,), float("inf"), dtype=t.dtype, device=t.device).scatter_reduce(0, ray, tk, "amin")
    wins = (tk == best[ray]) & (tk < float("inf"))
    big = torch.iinfo(torch.int64).max
    who = torch.full((n,), big, dtype=torch.int64, device=t.device).scatter_reduce(0, ray[wins], leaf[wins] + 1, "amin")
    return torch.where(who == big, torch.zeros_like(who), who), best


def run(n, steps, warmup):
    r0 = sphere_radius_law(n)
    vols = ibvh.generate_spheres(n, 42, r0=r0)
    bvh = ibvh.BVH(vols)
    lo, hi = vols[:, :3].amin(dim=0).cpu().numpy().astype("float64"), vols[:, :3].amax(dim=0).cpu().numpy().astype("float64")
    ph, dh = random_rays(n, lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), seed=43)
    p, d = torch.from_numpy(ph).cuda(), torch.from_numpy(dh).cuda()
    g = torch.Generator(device="cuda").manual_seed(7)
    fat = (r0 * (1 + 2 * torch.rand(n, generator=g, device="cuda"))).to(torch.float32)
    one = torch.ones(n, dtype=torch.float32, device="cuda")
    order = api._morton_order(p)
    q = {}
    for given, any_hit, unit, thick in itertools.product((True, False), (False, True), (False, True), (False, True)):
        pick = (lambda x: x) if given else (lambda x: x[order].contiguous())
        name = "_".join(("given" if given else "sorted", "any" if any_hit else "closest", "unit" if unit else "free", "fat" if thick else "ray"))
        q[name] = Cast(bvh, pick(p), pick(d), pick(fat) if thick else None, one if unit else None, any_hit)
    for c in q.values():
        c()
    torch.cuda.synchronize()
    same, any_equals_closest = True, True
    for any_hit, unit, thick in itertools.product(("closest", "any"), ("free", "unit"), ("ray", "fat")):
        a, b = q[f"given_{any_hit}_{unit}_{thick}"], q[f"sorted_{any_hit}_{unit}_{thick}"]
        if any_hit == "any":
            same &= torch.equal(b.touched, a.touched[order])
            any_equals_closest &= torch.equal(a.touched != 0, q[f"given_closest_{unit}_{thick}"].index != 0)
        else:
            same &= torch.equal(b.index, a.index[order]) and torch.equal(b.t.view(torch.int32), a.t[order].view(torch.int32))
    st = {"t": None}

    def list_route():
        st["t"] = ibvh.traverse_rays(bvh, p.t(), d.t(), cache=st["t"])
        return first_hits_of_list(st["t"].contacts, vols, p, d)
    index, t = list_route()
    torch.cuda.synchronize()
    candidates = int(st["t"].num_contacts)
    base = q["given_closest_free_ray"]
    differs = base.index.long() != index
    for _ in range(warmup):
        for c in q.values():
            c()
        list_route()
    ms = {k + "_ms": event_timed(c, steps) for k, c in q.items()}
    ms["given_closest_free_ray_wall_ms"] = timed(base, steps)[0]
    ms["list_route_ms"] = timed(list_route, steps)[0]
    out = {"leaves": n, "queries": n, "levels": int(bvh.tree.levels), "r0": round(r0, 6)}
    out.update({k: round(v, 4) for k, v in ms.items()})
    out.update(rays_hit=int((base.index != 0).sum().item()), rays_hit_within_unit=int((q["given_closest_unit_ray"].index != 0).sum().item()),
               fat_hit=int((q["given_closest_free_fat"].index != 0).sum().item()),
               list_candidates_per_ray=round(candidates / n, 3),
               list_route_over_closest_given=round(ms["list_route_ms"] / ms["given_closest_free_ray_wall_ms"], 3),
               sorted_over_given=round(ms["sorted_closest_free_ray_ms"] / ms["given_closest_free_ray_ms"], 3),
               any_over_closest_given=round(ms["given_any_free_ray_ms"] / ms["given_closest_free_ray_ms"], 3),
               unit_over_free_given=round(ms["given_closest_unit_ray_ms"] / ms["given_closest_free_ray_ms"], 3),
               fat_over_ray_given=round(ms["given_closest_free_fat_ms"] / ms["given_closest_free_ray_ms"], 3),
               sorted_equals_given=bool(same), any_equals_closest=bool(any_equals_closest),
               list_route_names_the_same_leaf=not bool(differs.any().item()), rays_that_differ=int(differs.sum().item()),
               of_them_the_list_route_misses=int((differs & (index == 0)).sum().item()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", default="100000,1000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    out = [run(int(n), a.steps, a.warmup) for n in a.leaves.split(",") if n]
    print(json.dumps({"bench_cast_spheres": out}))
    if not all(o["sorted_equals_given"] and o["any_equals_closest"] for o in out):
        raise SystemExit("results differ between orders or between the two modes: the times are not like for like")


if __name__ == "__main__":
    main()
