"""The box-vs-mesh contact query (ibvh_box_contacts) on the benchmark meshes, beside the way to get the contacts without it.

    python tools/bench_boxes.py [--workloads published,config3] [--steps K] [--warmup W]

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks), 100,000 boxes
  config3    the 7.2 M-triangle torus (bench.py's surface), 1e6 boxes
Boxes: centres within three mean edge lengths of the surface (a random barycentric point of a random triangle plus a random
offset), half extents uniform in 0.5 - 2 mean edge lengths per axis.  Two batches on the same centres and half extents,
reported separately: `oriented`, each box under a random rotation, and `aligned`, no rotations at all (rotations = NULL).
Timed between two device events, each as K chained calls after W warm-up calls, into preallocated outputs:
  count / write    the two passes of the C entry, each on its own, the offsets scanned once beforehand;
                   `given`: boxes in the order they were drawn (no coherence between the lanes of a wave),
                   `sorted`: the same boxes already in Morton order of their centres
  mirror           box_contacts(...) as a user calls it: Morton sort, count, scan, the read of the total, write — its events
                   bracket host work too
Before anything is timed the sorted and the given order must give the same lists.  One comparison on the same boxes:
  traverse + torch   what a user does without this query: a BBox BVH over the boxes' axis-aligned hulls,
                     traverse(bvh_boxes, bvh_mesh) for the (box, triangle box) candidates, then include/ibvh.h's 13 separating
                     axes as torch operations on the candidate list; timed with and without the box build; its contacts are
                     compared with the library's as sets of pairs
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

from bench_closest import mesh  # noqa: E402
from bench_sphere_contacts import timed  # noqa: E402

NAME = "ibvh_box_contacts"


def boxes_near(tris, m, seed=71):
    """-> centres (m, 3), half extents (m, 3), rotations (m, 3, 3) float32 (proper, orthonormal to rounding), the mean edge length"""
    rng = np.random.default_rng(seed)
    t = tris[rng.integers(0, len(tris), m)].reshape(-1, 3, 3).astype(np.float64)
    edge = float(np.linalg.norm(t[:, 1] - t[:, 0], axis=1).mean())
    w = rng.dirichlet((1.0, 1.0, 1.0), m)
    off = rng.normal(size=(m, 3))
    off *= (3 * edge * rng.random((m, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
    c = (w[:, :, None] * t).sum(axis=1) + off
    h = edge * (0.5 + 1.5 * rng.random((m, 3)))
    q = np.linalg.qr(rng.normal(size=(m, 3, 3)))[0]
    q[:, 2] *= np.linalg.det(q)[:, None]
    return c.astype(np.float32), h.astype(np.float32), q.astype(np.float32), edge


class Query:
    """both passes of the C entry on one batch, into preallocated buffers, nothing read back while timed; c, h: (N, 3) row-major,
    R: (N, 3, 3) or None"""

    def __init__(self, bvh, tdev, c, h, R):
        n = c.shape[0]
        self.bvh, self.tdev, self.c, self.h, self.R, self.n = bvh.struct(), tdev, c, h, R, n
        self.counts = torch.empty(n, dtype=torch.int64, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.count()
        self.offsets = torch.cumsum(self.counts, 0) - self.counts
        self.total = int(self.counts.sum().item())
        m = max(self.total, 1)
        self.index = torch.empty(m, dtype=torch.int32, device="cuda")
        self.inside = torch.empty(m, dtype=torch.uint8, device="cuda")
        self.write()
        torch.cuda.synchronize()
        assert self.flag.item() == 0

    def _call(self, mode, counts, offsets, capacity, outs):
        lib.call(NAME, C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.c), api._ptr(self.h), api._ptr(self.R),
                 self.n, mode, counts, offsets, capacity, *outs, api._ptr(self.flag), api._stream())

    def count(self):
        self._call(abi.BOXES_COUNT, api._ptr(self.counts), None, 0, (None,) * 2)

    def write(self):
        self._call(abi.BOXES_WRITE, None, api._ptr(self.offsets), self.index.shape[0],
                   [C.c_void_p(x.data_ptr()) for x in (self.index, self.inside)])

    def pairs(self, order=None):
        """the contacts as sorted keys box * 2^32 + triangle (order: the permutation this batch was walked in)"""
        s = torch.repeat_interleave(torch.arange(self.n, device="cuda"), self.counts)
        s = s if order is None else order[s]
        return torch.sort((s << 32) | self.index[:self.total].to(torch.int64)).values


def _axis(p1, p2, p3, rad):
    mn = torch.where(p2 < p1, p2, p1)
    mn = torch.where(p3 < mn, p3, mn)
    mx = torch.where(p2 > p1, p2, p1)
    mx = torch.where(p3 > mx, p3, mx)
    return (mn <= rad) & (mx >= -rad)


def hulls(c, h, R):
    """(N, 6) lo up: include/ibvh.h's hull of every box"""
    e = torch.stack([(R[:, 0, k].abs() * h[:, 0] + R[:, 1, k].abs() * h[:, 1]) + R[:, 2, k].abs() * h[:, 2] for k in range(3)], dim=1)
    return torch.cat([c - e, c + e], dim=1).contiguous()


def torch_narrow(tris, c, h, R, box, tri, chunk=4_000_000):
    """include/ibvh.h's 13 separating axes as torch operations on the candidate pairs (box[i], tri[i]), 0-based -> sorted keys
    box * 2^32 + (tri + 1) of the contacts.  (The candidates are the pairs of a hull and a triangle box that overlap: the box
    clause holds for every one of them.)"""
    keys = []
    for s in range(0, box.shape[0], chunk):
        si, ti = box[s:s + chunk], tri[s:s + chunk]
        k, cc, H, u = tris[ti], c[si], h[si], R[si]
        v = []
        for i in range(3):
            w = k[:, 3 * i:3 * i + 3] - cc
            v.append([(u[:, a, 0] * w[:, 0] + u[:, a, 1] * w[:, 1]) + u[:, a, 2] * w[:, 2] for a in range(3)])
        ok = _axis(v[0][0], v[1][0], v[2][0], H[:, 0]) & _axis(v[0][1], v[1][1], v[2][1], H[:, 1]) & _axis(v[0][2], v[1][2], v[2][2], H[:, 2])
        e = [[v[1][j] - v[0][j] for j in range(3)], [v[2][j] - v[1][j] for j in range(3)], [v[0][j] - v[2][j] for j in range(3)]]
        n = [e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]]
        d = (n[0] * v[0][0] + n[1] * v[0][1]) + n[2] * v[0][2]
        rad = (n[0].abs() * H[:, 0] + n[1].abs() * H[:, 1]) + n[2].abs() * H[:, 2]
        ok &= (d <= rad) & (d >= -rad)
        for ex, ey, ez in e:
            ok &= _axis(*[ey * v[i][2] - ez * v[i][1] for i in range(3)], ez.abs() * H[:, 1] + ey.abs() * H[:, 2])
            ok &= _axis(*[ez * v[i][0] - ex * v[i][2] for i in range(3)], ez.abs() * H[:, 0] + ex.abs() * H[:, 2])
            ok &= _axis(*[ex * v[i][1] - ey * v[i][0] for i in range(3)], ey.abs() * H[:, 0] + ex.abs() * H[:, 1])
        keys.append((si[ok] << 32) | (ti[ok] + 1))
    return torch.sort(torch.cat(keys)).values if keys else torch.empty(0, dtype=torch.int64, device="cuda")


def batch(bvh, tdev, c, h, R, order, steps, warmup):
    """one batch — R (N, 3, 3), or None for no rotations — through the library and through the list route"""
    n = c.shape[0]
    sc, sh, sR = c[order].contiguous(), h[order].contiguous(), None if R is None else R[order].contiguous()
    given, srt = Query(bvh, tdev, c, h, R), Query(bvh, tdev, sc, sh, sR)
    same = given.total == srt.total and torch.equal(given.pairs(), srt.pairs(order))
    out = {"contacts": given.total, "contacts_per_box": round(given.total / n, 2), "largest_list": int(given.counts.max().item()),
           "boxes_without": int((given.counts == 0).sum().item()), "sorted_equals_given": bool(same),
           "inside": torch.bincount(given.inside[:given.total].long(), minlength=8).tolist()}
    mirror = lambda: ibvh.box_contacts(bvh, tdev, c.t(), h.t(), R)
    mirror_count = lambda: ibvh.box_contacts(bvh, tdev, c.t(), h.t(), R, count_only=True)
    for _ in range(warmup):
        for f in (given.count, given.write, srt.count, srt.write, mirror, mirror_count):
            f()
    for key, f in (("count_given_ms", given.count), ("write_given_ms", given.write), ("count_sorted_ms", srt.count),
                   ("write_sorted_ms", srt.write)):
        out[key] = round(timed(f, steps), 4)
    out["mirror_ms"] = round(timed(mirror, max(2, steps // 2)), 4)
    out["mirror_count_only_ms"] = round(timed(mirror_count, max(2, steps // 2)), 4)

    # ---- what a user does without the query: a box BVH of the hulls, pair traversal, the 13 axes in torch ------------------
    eye = torch.eye(3, dtype=torch.float32, device="cuda").expand(n, 3, 3)
    Rt = eye if R is None else R
    vols = hulls(c, h, Rt)
    state = {}

    def build_boxes():
        state["bvh"] = ibvh.BVH(vols, ibvh.BBox(torch.float32))

    def candidates_and_narrow():
        trav = ibvh.traverse(state["bvh"], bvh)
        cand = trav.contacts
        state["candidates"] = int(cand.shape[0])
        state["keys"] = torch_narrow(tdev, c, h, Rt, cand[:, 0].to(torch.int64) - 1, cand[:, 1].to(torch.int64) - 1)

    def whole():
        build_boxes()
        candidates_and_narrow()
    for _ in range(max(1, warmup - 1)):
        whole()
    k = max(2, steps // 4)
    out["traverse_torch"] = {"box_build_ms": round(timed(build_boxes, k), 4), "traverse_and_torch_ms": round(timed(candidates_and_narrow, k), 4),
                             "build_traverse_and_torch_ms": round(timed(whole, k), 4), "candidates": state["candidates"],
                             "contacts": int(state["keys"].shape[0]),
                             "same_pairs_as_library": bool(state["keys"].shape[0] == given.total and torch.equal(state["keys"], given.pairs()))}
    return out


def run(name, steps, warmup):
    tris, m = mesh(name)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, ibvh.BBox(torch.float32)), ibvh.BBox(torch.float32))
    ch, hh, Rh, edge = boxes_near(tris, m)
    c, h, R = torch.from_numpy(ch).cuda(), torch.from_numpy(hh).cuda(), torch.from_numpy(Rh).cuda()
    order = api._morton_order(c)
    return {"workload": name, "triangles": int(tdev.shape[0]), "boxes": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6),
            "oriented": batch(bvh, tdev, c, h, R, order, steps, warmup), "aligned": batch(bvh, tdev, c, h, None, order, steps, warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"bench_boxes": [run(n, a.steps, a.warmup) for n in a.workloads.split(",") if n]}
    print(json.dumps(out), flush=True)
    batches = [w[b] for w in out["bench_boxes"] for b in ("oriented", "aligned")]
    if not all(b["sorted_equals_given"] for b in batches):
        raise SystemExit("the sorted and the given order give different lists: the times are not like for like")
    if not all(b["traverse_torch"]["same_pairs_as_library"] for b in batches):
        raise SystemExit("the list route and the library disagree on the pairs")


if __name__ == "__main__":
    main()
