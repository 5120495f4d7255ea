"""Refit against rebuild on bench.py's `timestep` workload.

    python tools/bench_refit.py [--sizes 1e6,1e7] [--steps K] [--warmup W]
    python tools/bench_refit.py --profile inplace|gathered --sizes 1e6 [--steps K]   (the program to put under rocprofv3)

The workload is bench.py::run_timestep's: config-2 law BSphere{Float32} leaves (BBox{Float32} nodes), user indices in reversed
numbering, every leaf moved by at most one cell of the 1024^3 Morton grid per step (the same move law).  Three chains run side by
side from the same cloud:
  (a) rebuild   move bvh.leaves.volume in place; bvh = BVH(bvh.leaves; cache=bvh)             (today's idiom, build.jl:109-126)
  (b) refit     move bvh.leaves.volume in place; refit(bvh)                                     (ibvh_refit, volumes = NULL)
  (c) gathered  move a (n, 4) user-order tensor;  refit(bvh, vols)                              (ibvh_refit from user order)
each followed by traverse(bvh; cache=traversal) and the host's read of the count.  A step is timed as bench.py times it: K
chained steps between two device synchronisations, minus the same K moves timed alone, after W warm-up steps; the refit alone
is timed the same way.

Then the traversal alone (traverse + count) on chain (b)'s tree after 1, 10, 50 and 200 steps of drift, against the traversal
of a tree rebuilt at that step.  A rebuild step costs a constant; a refit step costs the refit plus a traversal that slows as
the order goes stale, so the report names the first drift (interpolated between the measured ones) at which a refit step
costs as much as a rebuild step: the point where (a) catches up with (b).
--profile runs K refits of one form and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/bench_refit.py
--profile ...`.  Prints one JSON line.  bench.py is not involved."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import implicitbvh_amd as ibvh  # noqa: E402
from implicitbvh_amd.synthetic import sphere_radius_law  # noqa: E402

DRIFTS = (1, 10, 50, 200)


class Cloud:
    """The bench's time-stepping cloud: a BVH over pre-wrapped records with reversed user indices, moved by a seeded law."""

    def __init__(self, n, form):
        self.n, self.form = n, form
        vols = ibvh.generate_spheres(n, 47, r0=sphere_radius_law(n))
        user = torch.arange(n, 0, -1, dtype=torch.int32, device="cuda")
        # (c) keeps its state in user order: row k - 1 is the volume of user index k
        self.vols = torch.empty_like(vols)
        self.vols[user.long() - 1] = vols
        self.bvh = ibvh.BVH(ibvh.BoundingVolumes.wrap(vols, user))
        self.t = None
        self.gen = torch.Generator(device="cuda").manual_seed(11)
        self.step_size = 1.0 / 1024.0

    def move(self):
        d = (torch.rand((self.n, 3), generator=self.gen, device="cuda") * 2 - 1) * self.step_size
        if self.form == "gathered":
            self.vols[:, :3] += d
        else:
            self.bvh.leaves.volume[:, :3] += d

    def update(self):
        if self.form == "rebuild":
            self.bvh = ibvh.BVH(self.bvh.leaves, cache=self.bvh)
        elif self.form == "refit":
            ibvh.refit(self.bvh)
        else:
            ibvh.refit(self.bvh, self.vols)

    def traverse(self):
        self.t = ibvh.traverse(self.bvh, cache=self.t)
        return self.t.num_contacts

    def step(self):
        self.move()
        self.update()
        return self.traverse()


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3, out


def run(n, steps, warmup):
    # per-step cost of the three chains, one after the other, after the same warm-up
    chains = {f: Cloud(n, f) for f in ("rebuild", "refit", "gathered")}
    for c in chains.values():
        for _ in range(warmup):
            c.step()
    per_step, counts = {}, {}
    for f, c in chains.items():
        ms_all, counts[f] = timed(c.step, steps)
        ms_move, _ = timed(c.move, steps)
        per_step[f] = round(ms_all - ms_move, 4)
    # the refit alone (the same volumes again: the same work)
    refit_only = {f: round(timed(chains[f].update, steps)[0], 4) for f in ("refit", "gathered")}
    del chains
    # the traversal alone after d steps of drift: a refitted tree against one rebuilt at the same step
    pair = {f: Cloud(n, f) for f in ("rebuild", "refit")}
    trav, drift = {"rebuild": {}, "refit": {}}, 0
    for d in DRIFTS:
        for c in pair.values():
            for _ in range(d - drift):
                c.step()
        drift = d
        for f, c in pair.items():
            c.traverse()
            trav[f][d] = round(timed(c.traverse, steps)[0], 4)
    # a refit step at drift d ~ refit + traversal(d); a rebuild step is constant: first d where they meet (linear in between)
    cost = [(d, refit_only["refit"] + trav["refit"][d] - per_step["rebuild"]) for d in DRIFTS]
    catch = f"> {DRIFTS[-1]}"
    if cost[0][1] >= 0:
        catch = f"<= {DRIFTS[0]}"
    for (d0, v0), (d1, v1) in zip(cost, cost[1:]):
        if v0 < 0 <= v1:
            catch = round(d0 + (d1 - d0) * (-v0) / (v1 - v0), 1)
            break
    return {"n": n, "ms_per_step": per_step, "refit_ms": refit_only, "contacts": counts,
            "traverse_ms_after_drift_steps": trav, "rebuild_catches_up_with_refit_at_drift_steps": catch}


def profile(n, form, steps):
    c = Cloud(n, "refit" if form == "inplace" else "gathered")
    for _ in range(steps):
        c.move()
        c.update()
    torch.cuda.synchronize()
    return {"n": n, "profile": form, "refits": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e6,1e7")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", choices=("inplace", "gathered"))
    a = ap.parse_args()
    sizes = [int(float(s)) for s in a.sizes.split(",")]
    if a.profile:
        out = [profile(n, a.profile, a.steps) for n in sizes]
    else:
        out = [run(n, a.steps, a.warmup) for n in sizes]
    print(json.dumps({"bench_refit": out}))


if __name__ == "__main__":
    main()
