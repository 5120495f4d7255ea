"""The swept-sphere query (ibvh_sweep_spheres) on the benchmark meshes, beside the ray cast of the centres (ibvh_cast_rays) on
the same (p, d): what a user without the query has today, which misses every grazing contact and is late by up to a radius.

    python tools/bench_sweep.py [--workloads published,config3] [--steps K] [--warmup W]
    python tools/bench_sweep.py --profile closest|any|cast --workloads config3 [--steps K]   (the program to put under rocprofv3)

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks), 100,000 spheres
  config3    the 7.2 M-triangle torus (bench.py's surface), 1e6 spheres
Spheres: tools/bench_sphere_contacts.py's — centres within three mean edge lengths of the surface, radii uniform in one to
three mean edge lengths — each displaced by two to six of its radii in a random direction.
Timed, each after W warm-up calls, the launch alone, K chained calls between two DEVICE EVENTS, into preallocated outputs, on
the spheres as they were drawn (`given`: no coherence between the lanes of a wave) and on the same spheres in Morton order of
their centres (`sorted`):
  closest          the first contact (index, t, point, feature), unbounded
  closest_1        the first contact within the displacement, t_max = 1
  any / any_1      does it touch anything, unbounded / within the displacement
  cast / cast_1    ibvh_cast_rays' closest hit on the centres' rays, unbounded / t_max = 1: the baseline
and between two device synchronisations by the host's clock (it includes the host's work):
  mirror           sweep_spheres(..., t_max=1) as a user calls it: Morton sort of the centres, the launch, the flag read, the
                   un-permute
Before anything is timed the sorted and the given order must give the same bits and the any mask must equal the closest one's.
Prints one JSON line.  bench.py is not involved."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

from bench_cast import Cast, event_timed  # noqa: E402
from bench_closest import mesh  # noqa: E402
from bench_rays_resolve import timed  # noqa: E402
from bench_sphere_contacts import spheres_near  # noqa: E402


def displacements(radii, seed=53):
    """one per sphere: two to six radii long, in a random direction -> (m, 3) float32"""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(len(radii), 3))
    g *= ((2 + 4 * rng.random(len(radii))) * radii.astype(np.float64) / np.linalg.norm(g, axis=1))[:, None]
    return g.astype(np.float32)


class Sweep:
    """the one launch into preallocated outputs, nothing read back; p, d: (N, 3) row-major, r: (N,)"""

    def __init__(self, bvh, tdev, p, d, r, t_max=None, any_hit=False):
        n = p.shape[0]
        self.bvh, self.tdev, self.p, self.d, self.r, self.t_max, self.any_hit = bvh.struct(), tdev, p, d, r, t_max, any_hit
        self.index = None if any_hit else torch.empty(n, dtype=torch.int32, device="cuda")
        self.t = None if any_hit else torch.empty(n, dtype=torch.float32, device="cuda")
        self.point = None if any_hit else torch.empty((n, 3), dtype=torch.float32, device="cuda")
        self.feature = None if any_hit else torch.empty(n, dtype=torch.uint8, device="cuda")
        self.touched = torch.empty(n, dtype=torch.uint8, device="cuda") if any_hit else None
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def __call__(self):
        lib.call("ibvh_sweep_spheres", C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.p), api._ptr(self.d),
                 api._ptr(self.r), self.p.shape[0], api._ptr(self.t_max), abi.SWEEP_ANY if self.any_hit else abi.SWEEP_CLOSEST,
                 api._ptr(self.index), api._ptr(self.t), api._ptr(self.point), api._ptr(self.feature), api._ptr(self.touched),
                 api._ptr(self.flag), api._stream())


def _bits(x):
    return x.contiguous().view(torch.int32)


def _inputs(name):
    tris, m = mesh(name)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    ch, rh, edge = spheres_near(tris, m)
    p, r, d = torch.from_numpy(ch).cuda(), torch.from_numpy(rh).cuda(), torch.from_numpy(displacements(rh)).cuda()
    return bvh, tdev, p, d, r, edge


def run(name, steps, warmup):
    bvh, tdev, p, d, r, edge = _inputs(name)
    m = p.shape[0]
    order = api._morton_order(p)
    ps, ds, rs = p[order].contiguous(), d[order].contiguous(), r[order].contiguous()
    one = torch.ones(m, dtype=torch.float32, device="cuda")
    q = {}
    for tag, (pp, dd, rr) in (("given", (p, d, r)), ("sorted", (ps, ds, rs))):
        q["closest_" + tag] = Sweep(bvh, tdev, pp, dd, rr)
        q["closest_1_" + tag] = Sweep(bvh, tdev, pp, dd, rr, one)
        q["any_" + tag] = Sweep(bvh, tdev, pp, dd, rr, any_hit=True)
        q["any_1_" + tag] = Sweep(bvh, tdev, pp, dd, rr, one, any_hit=True)
        q["cast_" + tag] = Cast(bvh, tdev, pp, dd)
        q["cast_1_" + tag] = Cast(bvh, tdev, pp, dd, one)
    for c in q.values():
        c()
    torch.cuda.synchronize()
    assert all(c.flag.item() == 0 for c in q.values())
    g, s, g1 = q["closest_given"], q["closest_sorted"], q["closest_1_given"]
    same = (torch.equal(s.index, g.index[order]) and torch.equal(_bits(s.t), _bits(g.t[order])) and torch.equal(_bits(s.point), _bits(g.point[order]))
            and torch.equal(s.feature, g.feature[order]) and torch.equal(q["any_sorted"].touched, q["any_given"].touched[order])
            and torch.equal(q["closest_1_sorted"].index, g1.index[order]))
    any_equals_closest = (torch.equal(q["any_given"].touched != 0, g.index != 0) and torch.equal(q["any_1_given"].touched != 0, g1.index != 0))
    mirror = lambda: ibvh.sweep_spheres(bvh, tdev, p.t(), d.t(), r, t_max=1.0)
    for _ in range(warmup):
        for c in q.values():
            c()
        mirror()
    ms = {k + "_ms": event_timed(c, steps) for k, c in q.items()}
    ms["mirror_ms"] = timed(mirror, max(2, steps // 2))[0]
    hit1, cast1 = g1.index != 0, q["cast_1_given"].index != 0
    moving = hit1 & (g1.t > 0)
    out = {"workload": name, "triangles": int(tdev.shape[0]), "spheres": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6)}
    out.update({k: round(v, 4) for k, v in ms.items()})
    out.update(touching_at_start=int((hit1 & (g1.t == 0)).sum().item()), hit_while_moving=int(moving.sum().item()),
               miss_within_1=int((~hit1).sum().item()), hit_unbounded=int((g.index != 0).sum().item()),
               features_of_moving_hits=torch.bincount(g1.feature[moving].long(), minlength=7).tolist(),
               cast_hits_within_1=int(cast1.sum().item()), contacts_the_cast_misses=int((hit1 & ~cast1).sum().item()),
               closest_1_over_cast_1_sorted=round(ms["closest_1_sorted_ms"] / ms["cast_1_sorted_ms"], 3),
               closest_1_over_cast_1_given=round(ms["closest_1_given_ms"] / ms["cast_1_given_ms"], 3),
               closest_over_cast_sorted=round(ms["closest_sorted_ms"] / ms["cast_sorted_ms"], 3),
               any_1_over_closest_1_sorted=round(ms["any_1_sorted_ms"] / ms["closest_1_sorted_ms"], 3),
               sorted_equals_given=bool(same), any_equals_closest=bool(any_equals_closest))
    return out


def profile(name, form, steps):
    bvh, tdev, p, d, r, _ = _inputs(name)
    one = torch.ones(p.shape[0], dtype=torch.float32, device="cuda")
    c = Cast(bvh, tdev, p, d, one) if form == "cast" else Sweep(bvh, tdev, p, d, r, one, any_hit=form == "any")
    for _ in range(steps):
        c()
    torch.cuda.synchronize()
    return {"workload": name, "profile": form, "calls": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", choices=("closest", "any", "cast"))
    a = ap.parse_args()
    names = [n for n in a.workloads.split(",") if n]
    out = [profile(n, a.profile, a.steps) if a.profile else run(n, a.steps, a.warmup) for n in names]
    print(json.dumps({"bench_sweep": out}))
    if not a.profile and not all(o["sorted_equals_given"] and o["any_equals_closest"] for o in out):
        raise SystemExit("results differ between orders or between the two modes: the times are not like for like")


if __name__ == "__main__":
    main()
