"""The ray cast (ibvh_cast_rays) on the benchmark meshes, against raycast() — the leaf-vs-tree ray traversal plus the resolve —
on the same rays, the same BVH, in the same process.

    python tools/bench_cast.py [--workloads published,config3] [--steps K] [--warmup W]
    python tools/bench_cast.py --profile closest|any|raycast --workloads config3 [--steps K]   (the program to put under rocprofv3)

Workloads are tools/bench_rays_resolve.py's with --leaves bbox (BBox{Float32} leaves from the triangles — the ray cast needs
boxes —, BBox{Float32} nodes, Int32 indices, the reference benchmark's random rays in the box of the leaf centres):
  published  249,882 triangles under 100,000 rays      config3  the 7.2 M-triangle torus under 1e6 rays
Timed, each after W warm-up calls.  The launch alone, K chained calls between two DEVICE EVENTS, into preallocated outputs,
on the rays as they were drawn (`given`: no coherence between the lanes of a wave) and on the same rays in Morton order of
their origins (`sorted`):
  closest          the closest hit (index, t, uv), unbounded rays
  any              any hit, unbounded rays
  closest_half     the closest hit with t_max = half the scene's diagonal (per ray: 0.5 |diagonal| / |d|)
and between two device synchronisations by the host's clock (they include the host's work):
  raycast          raycast(...; cache=previous): traversal (count, scan, write), the host's read of the count, resolve — the
                   baseline: that code is the parent commit's
  mirror           cast_rays(...) as a user calls it: Morton sort of the origins, the launch, the flag read, the un-permute
  closest_*_wall   the launch alone by the host's clock, for a like-for-like ratio against raycast
Before anything is timed the sorted and the given order must give the same bits, any-hit must equal closest-hit's mask, and
the closest hit must equal raycast()'s nearest hit on every ray: the index, and the bits of t except where the clamp is active
(counted as `clamp_active`: there t* exceeds the resolve's t by rounding).  Prints one JSON line.  bench.py is
not involved."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import abi, api, lib  # noqa: E402

from bench_rays_resolve import timed, workload  # noqa: E402


class Cast:
    """the one launch into preallocated outputs, nothing read back; p, d: (N, 3) row-major"""

    def __init__(self, bvh, tdev, p, d, t_max=None, any_hit=False):
        n = p.shape[0]
        self.bvh, self.tdev, self.p, self.d, self.t_max, self.any_hit = bvh.struct(), tdev, p, d, t_max, any_hit
        self.index = None if any_hit else torch.empty(n, dtype=torch.int32, device="cuda")
        self.t = None if any_hit else torch.empty(n, dtype=torch.float32, device="cuda")
        self.uv = None if any_hit else torch.empty((n, 2), dtype=torch.float32, device="cuda")
        self.occluded = torch.empty(n, dtype=torch.uint8, device="cuda") if any_hit else None
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def __call__(self):
        lib.call("ibvh_cast_rays", C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.p), api._ptr(self.d),
                 self.p.shape[0], api._ptr(self.t_max), abi.CAST_ANY if self.any_hit else abi.CAST_CLOSEST, api._ptr(self.index),
                 api._ptr(self.t), api._ptr(self.uv), api._ptr(self.occluded), api._ptr(self.flag), api._stream())


def event_timed(fn, k):
    """ms per call of k chained calls between two device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(k):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / k


def _bits(x):
    return x.contiguous().view(torch.int32)


def _half_diagonal(tdev, d):
    v = tdev.reshape(-1, 3)
    diagonal = torch.linalg.norm(v.amax(dim=0) - v.amin(dim=0))
    return (0.5 * diagonal / torch.linalg.norm(d, dim=1)).to(torch.float32).contiguous()


def run(name, steps, warmup):
    bvh, tdev, p, d = workload(name, "bbox")
    nr = p.shape[0]
    order = api._morton_order(p)
    ps, ds = p[order].contiguous(), d[order].contiguous()
    lim = _half_diagonal(tdev, d)
    lims = lim[order].contiguous()
    q = {"closest_given": Cast(bvh, tdev, p, d), "closest_sorted": Cast(bvh, tdev, ps, ds),
         "any_given": Cast(bvh, tdev, p, d, any_hit=True), "any_sorted": Cast(bvh, tdev, ps, ds, any_hit=True),
         "closest_half_given": Cast(bvh, tdev, p, d, lim), "closest_half_sorted": Cast(bvh, tdev, ps, ds, lims)}
    for c in q.values():
        c()
    st = {"t": None}

    def raycast():
        hits, st["t"] = ibvh.raycast(bvh, tdev, p.t(), d.t(), cache=st["t"])
        return hits
    hits = raycast()
    torch.cuda.synchronize()
    assert all(c.flag.item() == 0 for c in q.values())
    g, s = q["closest_given"], q["closest_sorted"]
    same = (torch.equal(s.index, g.index[order]) and torch.equal(_bits(s.t), _bits(g.t[order])) and torch.equal(_bits(s.uv), _bits(g.uv[order]))
            and torch.equal(q["any_sorted"].occluded, q["any_given"].occluded[order])
            and torch.equal(q["closest_half_sorted"].index, q["closest_half_given"].index[order]))
    any_equals_closest = torch.equal(q["any_given"].occluded != 0, g.index != 0)
    # t* = max(t, entry of the leaf's box): where the clamp is active it exceeds the resolve's t, by rounding only
    moved = _bits(g.t) != _bits(hits.t)
    clamped = moved & (g.t > hits.t) & (g.t - hits.t <= 4 * torch.finfo(torch.float32).eps * hits.t)
    differs = {"index": int((g.index != hits.index).sum().item()), "t_beyond_the_clamp": int((moved & ~clamped).sum().item())}
    candidates = int(st["t"].num_contacts)
    mirror = lambda: ibvh.cast_rays(bvh, tdev, p.t(), d.t())
    for _ in range(warmup):
        for c in q.values():
            c()
        raycast()
        mirror()
    ms = {k + "_ms": event_timed(c, steps) for k, c in q.items()}
    ms["closest_given_wall_ms"] = timed(g, steps)[0]
    ms["closest_sorted_wall_ms"] = timed(s, steps)[0]
    ms["raycast_ms"] = timed(raycast, steps)[0]
    ms["mirror_ms"] = timed(mirror, max(2, steps // 2))[0]
    out = {"workload": name, "triangles": int(tdev.shape[0]), "rays": nr, "levels": int(bvh.tree.levels)}
    out.update({k: round(v, 4) for k, v in ms.items()})
    out.update(rays_hit=int((g.index != 0).sum().item()), rays_hit_within_half=int((q["closest_half_given"].index != 0).sum().item()),
               raycast_candidates_per_ray=round(candidates / nr, 3),
               raycast_over_closest_given=round(ms["raycast_ms"] / ms["closest_given_wall_ms"], 3),
               raycast_over_closest_sorted=round(ms["raycast_ms"] / ms["closest_sorted_wall_ms"], 3),
               raycast_over_mirror=round(ms["raycast_ms"] / ms["mirror_ms"], 3),
               any_over_closest_sorted=round(ms["any_sorted_ms"] / ms["closest_sorted_ms"], 3),
               half_over_closest_sorted=round(ms["closest_half_sorted_ms"] / ms["closest_sorted_ms"], 3),
               sorted_equals_given=bool(same), any_equals_closest=bool(any_equals_closest),
               raycast_equal=not any(differs.values()), raycast_differs=differs, clamp_active=int(clamped.sum().item()))
    return out


def profile(name, form, steps):
    bvh, tdev, p, d = workload(name, "bbox")
    if form == "raycast":
        trav = None
        for _ in range(steps):
            _, trav = ibvh.raycast(bvh, tdev, p.t(), d.t(), cache=trav)
    else:
        c = Cast(bvh, tdev, p, d, any_hit=form == "any")
        for _ in range(steps):
            c()
    torch.cuda.synchronize()
    return {"workload": name, "profile": form, "calls": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", choices=("closest", "any", "raycast"))
    a = ap.parse_args()
    names = [n for n in a.workloads.split(",") if n]
    out = [profile(n, a.profile, a.steps) if a.profile else run(n, a.steps, a.warmup) for n in names]
    print(json.dumps({"bench_cast": out}))
    if not a.profile and not all(o["sorted_equals_given"] and o["any_equals_closest"] for o in out):
        raise SystemExit("results differ between orders or between the two modes: the times are not like for like")
    if not a.profile and not all(o["raycast_equal"] for o in out):
        raise SystemExit("the closest hit differs from raycast()'s nearest hit: the baseline did not compute the same thing")


if __name__ == "__main__":
    main()
