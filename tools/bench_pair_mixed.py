"""Pair LVT traversal of two BVHs of different volume types (IBVH_PAIR_MIXED_TYPES) against the same-type yardstick.

    python tools/bench_pair_mixed.py [--steps K] [--warmup W] [--rounds R] [--only particles_1e6|published_100k|particles_drive]

Each workload is a particle cloud of BSphere{Float32} leaves (BBox{Float32} nodes) filling the bounding box of a triangle
surface whose leaves are BBox{Float32}:
  particles_1e6     1e6 particles against synthetic.torus_mesh() (7.2 M triangles): the triangles drive (box queries)
  published_100k    100,000 particles against the 249,882-triangle torus (the readme_250k size): the triangles drive
  particles_drive   1e6 particles against the 249,882-triangle torus: the PARTICLES drive (sphere queries, the other walker
                    instantiation)
Particle radii follow the config-2 law (synthetic.sphere_radius_law), scaled to the surface's box.  The yardstick is the same
pair with the particles given as their BBox{Float32} boxes: one volume type on both sides, the existing path.  A step is one
traverse(particles, surface; cache=previous) and the host's read of the count.  Steps are timed as bench.py times them: K
chained steps between two device synchronisations (the read of the count returns as soon as the total is published, before
the writing pass has finished; the closing synchronisation counts that pass), divided by K.  The mixed and the yardstick
pair alternate for `--rounds` rounds; the median round is reported.
Prints one JSON line: per workload the two medians, their ratio (mixed / same type) and both contact counts (they must agree:
the box iscontact(::BSphere, ::BBox) forms is the yardstick's leaf).  bench.py is not involved."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd.synthetic import sphere_radius_law, torus_mesh  # noqa: E402


class Chain:
    """One cache= chain of traversals of a pair; run(K) -> ms per step over K chained steps (whole traversals: see above)."""

    def __init__(self, a, b, warmup):
        self.a, self.b, self.t = a, b, None
        for _ in range(max(warmup, 2)):  # (the second call with a cache is the steady state, bench.py _timed)
            self.step()
        torch.cuda.synchronize()

    def step(self):
        self.t = ibvh.traverse(self.a, self.b, cache=self.t)
        return self.t.num_contacts  # (the host's read of the count: part of every step)

    def run(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            n = self.step()
        torch.cuda.synchronize()  # (the last step's writing pass included)
        return (time.perf_counter() - t0) / steps * 1e3, n


def time_pairs(mixed, same, steps, rounds):
    ms_m, ms_s = [], []
    for _ in range(rounds):
        m, n_m = mixed.run(steps)
        s, n_s = same.run(steps)
        ms_m.append(m)
        ms_s.append(s)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return med(ms_m), n_m, med(ms_s), n_s


def workload(tris, n_particles, steps, warmup, rounds, seed=42):
    f32 = torch.float32
    surf_vols = ibvh.bounding_volumes_from_triangles(tris, ibvh.BBox(f32))
    surface = ibvh.BVH(surf_vols, ibvh.BBox(f32))
    lo, hi = surf_vols[:, :3].min(0).values, surf_vols[:, 3:].max(0).values
    ext = (hi - lo).tolist()
    r0 = sphere_radius_law(n_particles) * (ext[0] * ext[1] * ext[2]) ** (1 / 3)  # (the law's density in the surface's box)
    spheres = ibvh.generate_spheres(n_particles, seed, origin=tuple(lo.tolist()), extent=tuple(ext), r0=r0)
    particles = ibvh.BVH(spheres, ibvh.BBox(f32))
    boxes = torch.cat([spheres[:, :3] - spheres[:, 3:4], spheres[:, :3] + spheres[:, 3:4]], dim=1).contiguous()  # (Float32, as iscontact)
    as_boxes = ibvh.BVH(boxes, ibvh.BBox(f32))
    mixed_ms, mixed_n, same_ms, same_n = time_pairs(Chain(particles, surface, warmup), Chain(as_boxes, surface, warmup), steps, rounds)
    return {"particles": n_particles, "triangles": int(tris.shape[0]),
            "driver": "particles" if n_particles >= int(tris.shape[0]) else "triangles", "mixed_ms": round(mixed_ms, 4), "same_type_ms": round(same_ms, 4),
            "ratio": round(mixed_ms / same_ms, 3), "contacts_mixed": mixed_n, "contacts_same_type": same_n,
            "contacts_agree": mixed_n == same_n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("particles_1e6", "published_100k", "particles_drive"), default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"what": "traverse(particles BSphere{Float32}, surface BBox{Float32}) vs the particles as BBox{Float32} (same type)",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    if args.only in (None, "particles_1e6"):
        tris = torch.from_numpy(torus_mesh()).cuda()
        out["particles_1e6"] = workload(tris, 1_000_000, args.steps, args.warmup, args.rounds)
        del tris
    tris = torch.from_numpy(torus_mesh(354, 353)[:249_882].copy()).cuda()
    if args.only in (None, "published_100k"):
        out["published_100k"] = workload(tris, 100_000, args.steps, args.warmup, args.rounds)
    if args.only in (None, "particles_drive"):
        out["particles_drive"] = workload(tris, 1_000_000, args.steps, args.warmup, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
