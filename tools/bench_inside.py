"""The inside / outside query (ibvh_point_crossings) on the benchmark meshes.

    python tools/bench_inside.py [--workloads published,config3] [--steps K] [--warmup W] [--axis A] [--no-torch]

Workloads and point sets are tools/bench_closest.py's (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32
indices; `box` — uniform in the mesh's box inflated by 25 % each way; `near` — within three mean edge lengths of the surface).
Timed per set, each as K chained calls between two device synchronisations after W warm-up calls, into preallocated outputs:
  given      the one launch, points in the order they were drawn (no coherence between the lanes of a wave)
  sorted     the one launch, the same points already in Morton order
  mirror     point_crossings(...) as a user calls it: Morton sort of the points, the launch, the flag read, the un-permute
  closest_sorted          ibvh_closest_triangles with max_distance = three mean edge lengths on the same sorted points
  closest_points_mirror   closest_points(..., max_distance = three mean edge lengths) as a user calls it
  signed_distance_mirror  signed_distance(...) with the same radius: what the sign costs over the distance alone
Before anything is timed the sorted and the given order must give the same bits.  `torch`: rules 1 to 4 of include/ibvh.h as
torch operations, brute force over ALL triangles, at 3,200 triangles and 10,000 points only (it is O(n m)); compared with the
library, then timed — a sanity ratio, not a baseline at size.  Prints one JSON line.  bench.py is not involved."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd import api, lib  # noqa: E402

from bench_closest import Query as ClosestQuery, mesh, point_sets, timed  # noqa: E402


class Query:
    """the one launch into preallocated outputs, nothing read back; p: (N, 3) row-major"""

    def __init__(self, bvh, tdev, p, axis):
        n = p.shape[0]
        self.bvh, self.tdev, self.p, self.axis = bvh.struct(), tdev, p, axis
        self.crossings = torch.empty(n, dtype=torch.int32, device="cuda")
        self.winding = torch.empty(n, dtype=torch.int32, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def __call__(self):
        lib.call("ibvh_point_crossings", C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.p), self.p.shape[0],
                 self.axis, api._ptr(self.crossings), api._ptr(self.winding), api._ptr(self.flag), api._stream())


def _edge_side(x, y, p):
    flipped = (y[..., 0] < x[..., 0]) | ((y[..., 0] == x[..., 0]) & ((y[..., 1] < x[..., 1]) | ((y[..., 1] == x[..., 1]) & (y[..., 2] < x[..., 2]))))
    f = flipped[..., None]
    x, y = torch.where(f, y, x), torch.where(f, x, y)
    e = (y[..., 0] - x[..., 0]) * (p[..., 1] - x[..., 1]) - (y[..., 1] - x[..., 1]) * (p[..., 0] - x[..., 0])
    return (e >= 0) ^ flipped


def torch_brute_force(tris, p, axis, chunk=2000):
    """include/ibvh.h's rules 1 to 4 as torch operations over ALL (point, triangle) pairs, then the two counts"""
    perm = [(axis + 1) % 3, (axis + 2) % 3, axis]
    a, b, c = (tris[None, :, k:k + 3][..., perm] for k in (0, 3, 6))
    lo = torch.where(a < b, torch.where(a < c, a, c), torch.where(b < c, b, c))
    up = torch.where(a > b, torch.where(a > c, a, c), torch.where(b > c, b, c))
    ab, ac = b - a, c - a
    n0 = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1]
    n1 = ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2]
    n2 = ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
    crossings, winding = [], []
    for s in range(0, p.shape[0], chunk):
        pp = p[s:s + chunk, None, :][..., perm]
        guard = ((pp[..., 0] >= lo[..., 0]) & (pp[..., 0] <= up[..., 0]) & (pp[..., 1] >= lo[..., 1]) & (pp[..., 1] <= up[..., 1])
                 & (up[..., 2] >= pp[..., 2]))
        s0, s1, s2 = _edge_side(a, b, pp), _edge_side(b, c, pp), _edge_side(c, a, pp)
        d = pp - a
        depth = (n0 * d[..., 0] + n1 * d[..., 1]) + n2 * d[..., 2]
        pos, neg = guard & s0 & s1 & s2 & (depth < 0), guard & ~(s0 | s1 | s2) & (depth > 0)
        crossings.append((pos | neg).sum(dim=1).to(torch.int32))
        winding.append((pos.sum(dim=1) - neg.sum(dim=1)).to(torch.int32))
    return torch.cat(crossings), torch.cat(winding)


def run(name, steps, warmup, axis):
    tris, m = mesh(name)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    sets, edge = point_sets(tris, m)
    radius = 3 * edge
    out = {"workload": name, "triangles": int(tdev.shape[0]), "points": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6),
           "axis": axis, "sets": {}}
    for sname, ph in sets.items():
        p = torch.from_numpy(ph).cuda()
        order = api._morton_order(p)
        ps = p[order].contiguous()
        given, srt, closest = Query(bvh, tdev, p, axis), Query(bvh, tdev, ps, axis), ClosestQuery(bvh, tdev, ps, radius)
        given()
        srt()
        closest()
        torch.cuda.synchronize()
        assert given.flag.item() == 0 and srt.flag.item() == 0 and closest.flag.item() == 0
        same = torch.equal(srt.crossings, given.crossings[order]) and torch.equal(srt.winding, given.winding[order])
        mirror = lambda: ibvh.point_crossings(bvh, tdev, p.t(), axis=axis)
        cp_mirror = lambda: ibvh.closest_points(bvh, tdev, p.t(), max_distance=radius)
        sd_mirror = lambda: ibvh.signed_distance(bvh, tdev, p.t(), axis=axis, max_distance=radius)
        for _ in range(warmup):
            for fn in (given, srt, closest, mirror, cp_mirror, sd_mirror):
                fn()
        ms = {"given_ms": timed(given, steps)[0], "sorted_ms": timed(srt, steps)[0], "mirror_ms": timed(mirror, max(2, steps // 2))[0],
              "closest_sorted_ms": timed(closest, steps)[0], "closest_points_mirror_ms": timed(cp_mirror, max(2, steps // 2))[0],
              "signed_distance_mirror_ms": timed(sd_mirror, max(2, steps // 2))[0]}
        res = {k: round(v, 4) for k, v in ms.items()}
        res.update(inside_parity=int((given.crossings & 1).sum().item()), inside_winding=int((given.winding != 0).sum().item()),
                   crossings_per_point=round(float(given.crossings.float().mean().item()), 3), sorted_equals_given=bool(same))
        out["sets"][sname] = res
    return out


def torch_ratio(steps, warmup, axis):
    tris, m = mesh("small")
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    sets, _ = point_sets(tris, m)
    p = torch.from_numpy(sets["near"]).cuda()
    q = Query(bvh, tdev, p, axis)
    q()
    crossings, winding = torch_brute_force(tdev, p, axis)
    torch.cuda.synchronize()
    equal = torch.equal(q.crossings, crossings) and torch.equal(q.winding, winding)
    for _ in range(warmup):
        q()
    torch_brute_force(tdev, p, axis)
    ms_lib, _ = timed(q, steps)
    ms_torch, _ = timed(lambda: torch_brute_force(tdev, p, axis), 2)
    return {"triangles": int(tdev.shape[0]), "points": m, "library_ms": round(ms_lib, 4), "torch_brute_force_ms": round(ms_torch, 3),
            "torch_over_library": round(ms_torch / ms_lib, 1), "torch_equal": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--axis", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    out = {"bench_inside": [run(n, a.steps, a.warmup, a.axis) for n in a.workloads.split(",") if n]}
    if not a.no_torch:
        out["torch_sanity"] = torch_ratio(a.steps, a.warmup, a.axis)
    print(json.dumps(out))
    ok = all(s["sorted_equals_given"] for w in out["bench_inside"] for s in w["sets"].values())
    if not ok or not out.get("torch_sanity", {"torch_equal": True})["torch_equal"]:
        raise SystemExit("results differ between orders or from the torch brute force: the times are not like for like")


if __name__ == "__main__":
    main()
