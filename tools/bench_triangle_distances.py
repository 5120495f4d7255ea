"""The triangle-vs-mesh distance query (ibvh_triangle_distances) on the benchmark meshes, beside the ways to get there without it.

    python tools/bench_triangle_distances.py [--workloads published,config3] [--steps K] [--warmup W] [--gap G]

Workloads (BBox{Float32} leaves from the triangles, BBox{Float32} nodes, Int32 indices):
  published  249,882 triangles (the size of the reference's published benchmarks), 100,000 queries
  config3    the 7.2 M-triangle torus (bench.py's surface), 1,000,000 queries
The queries are triangles of the mesh itself, evenly drawn, shifted along z by G (default 3) mean edge lengths and a little
sideways: a second copy of the surface at a gap of a few edge lengths, which near the torus's flanks comes closer.
Timed between two device events, each as K chained calls after W warm-up calls, into preallocated outputs:
  launch          the C entry alone; `given`: the queries in the mesh's own order, `sorted`: already in Morton order of their
                  centroids; `unbounded` and `within`: with a max_distance of 2 G edge lengths
  mirror          triangle_distances(...) as a user calls it: Morton sort, launch, flag read, un-permute — its events bracket
                  host work too; `presorted`: the same without the sort; mesh_distance on top of it
Before anything is timed the sorted and the given order must give the same bits.  For context, on the same queries:
  closest_points  ibvh_closest_triangles on the queries' 3 N vertices, sorted — the shortcut a user has without this query;
                  `shortcut_wrong` counts the queries whose smallest vertex distance is NOT the triangle distance
  triangle_contacts  the count pass of ibvh_triangle_contacts on the same queries ("do they touch" costs this much)
  torch           include/ibvh.h's evaluation as torch operations over ALL pairs of 10,000 queries x 3,200 triangles
                  (torus40), against the library on the same batch; the two must be bit-equal
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

from bench_closest import _dot, mesh  # noqa: E402
from bench_sphere_contacts import timed  # noqa: E402

NAME = "ibvh_triangle_distances"


def mean_edge(tris):
    t = tris[:: max(1, len(tris) // 100_000)].reshape(-1, 3, 3).astype(np.float64)
    return float(np.linalg.norm(t[:, 1] - t[:, 0], axis=1).mean())


def shifted(tris, m, gap):
    """m triangles of the mesh, evenly drawn (again from the start, one more gap up, once they run out), shifted along z by
    `gap` and by a hundredth of it along x and y; float64, cast back"""
    i = (np.arange(m) * max(1, len(tris) // m)) % len(tris)
    up = gap * (1 + (np.arange(m) * max(1, len(tris) // m)) // len(tris))
    off = np.stack([0.013 * up, 0.007 * up, up], axis=1)
    return (tris[i].astype(np.float64) + np.tile(off, 3)).astype(tris.dtype)


class Query:
    """the one launch into preallocated outputs, nothing read back while timed; q: (N, 9)"""

    def __init__(self, bvh, tdev, q, radius=None):
        n = q.shape[0]
        self.bvh, self.tdev, self.q, self.n = bvh.struct(), tdev, q, n
        self.index = torch.empty(n, dtype=torch.int32, device="cuda")
        self.d2 = torch.empty(n, dtype=torch.float32, device="cuda")
        self.xq, self.xk = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        self.kind = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.r2 = None if radius is None else C.c_float(np.float32(radius) * np.float32(radius))

    def __call__(self):
        lib.call(NAME, C.byref(self.bvh), api._ptr(self.tdev), self.tdev.shape[0], api._ptr(self.q), self.n, 0,
                 None if self.r2 is None else C.byref(self.r2), api._ptr(self.index), api._ptr(self.d2), api._ptr(self.xq),
                 api._ptr(self.xk), api._ptr(self.kind), api._ptr(self.flag), api._stream())

    def outputs(self, order=None):
        outs = (self.index, self.d2, self.xq, self.xk, self.kind)
        return outs if order is None else api._unpermute(order, outs)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


# ---- include/ibvh.h's evaluation as torch operations, over broadcast pairs -----------------------------------------------
def _clamp(x, lo, up):
    return torch.where(x < lo, lo, torch.where(x > up, up, x))


def _point_triangle(tri, p):
    a, b, c = tri[..., 0:3], tri[..., 3:6], tri[..., 6:9]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    den = 1 / ((va + vb) + vc)
    q = (a + (vb * den)[..., None] * ab) + (vc * den)[..., None] * ac
    for case, point in reversed((((d1 <= 0) & (d2 <= 0), a), ((d3 >= 0) & (d4 <= d3), b),
                                 ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[..., None] * ab),
                                 ((d6 >= 0) & (d5 <= d6), c), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[..., None] * ac),
                                 ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b)))):
        q = torch.where(case[..., None], point, q)        # (applied last to first: the FIRST matching case decides)
    lo = torch.where(a < b, torch.where(a < c, a, c), torch.where(b < c, b, c))
    up = torch.where(a > b, torch.where(a > c, a, c), torch.where(b > c, b, c))
    q = _clamp(q, lo, up)
    e = p - q
    return q, _dot(e, e)


def _unit(x):
    return torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))


def _segments(p1, q1, p2, q2):
    d1, d2v, r = q1 - p1, q2 - p2, p1 - p2
    A, E, F, Cc, B = _dot(d1, d1), _dot(d2v, d2v), _dot(d2v, r), _dot(d1, r), _dot(d1, d2v)
    den = A * E - B * B
    zero = torch.zeros_like(den)
    s_in = torch.where(den > 0, _unit((B * F - Cc * E) / den), zero)
    t_in = (B * s_in + F) / E
    s_lo, s_up = _unit(-Cc / A), _unit((B - Cc) / A)
    s_gen = torch.where(t_in < 0, s_lo, torch.where(t_in > 1, s_up, s_in))
    s = torch.where(A == 0, zero, torch.where(E == 0, s_lo, s_gen))
    t = torch.where(A == 0, torch.where(E != 0, _unit(F / E), zero), torch.where(E == 0, zero, _unit(t_in)))
    x1 = _clamp(p1 + s[..., None] * d1, torch.where(p1 < q1, p1, q1), torch.where(p1 > q1, p1, q1))
    x2 = _clamp(p2 + t[..., None] * d2v, torch.where(p2 < q2, p2, q2), torch.where(p2 > q2, p2, q2))
    e = x1 - x2
    return x1, x2, _dot(e, e)


def _cross(x, y):
    return torch.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                        x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], dim=-1)


def _seg(p0, p1, tri):
    a, b, c = tri[..., 0:3], tri[..., 3:6], tri[..., 6:9]
    d = p1 - p0
    e1, e2 = b - a, c - a
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    inv = 1 / det
    tv = p0 - a
    u = _dot(tv, pv) * inv
    qv = _cross(tv, e1)
    v = _dot(d, qv) * inv
    t = _dot(e2, qv) * inv
    return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1), p0 + t[..., None] * d


def _box(t):
    a, b, c = t[..., 0:3], t[..., 3:6], t[..., 6:9]
    lo, up = torch.where(b < a, b, a), torch.where(b > a, b, a)
    return torch.where(c < lo, c, lo), torch.where(c > up, c, up)


def torch_brute_force(tris, queries, chunk=250):
    """both rules over ALL (query, triangle) pairs, then the lexicographic minimum -> (index, d2, xQ, xK, kind)"""
    k = tris[None]
    ends = ((0, 3), (3, 6), (6, 0))
    outs = []
    for s in range(0, queries.shape[0], chunk):
        q = queries[s:s + chunk, None, :]
        shape = (q.shape[0], k.shape[1])
        best = None
        for c in range(15):
            if c < 3:
                v = q[..., 3 * c:3 * c + 3]
                x, d2 = _point_triangle(k, v)
                xq, xk = v, x
            elif c < 6:
                v = k[..., 3 * (c - 3):3 * (c - 3) + 3]
                x, d2 = _point_triangle(q, v)
                xq, xk = x, v
            else:
                (i0, i1), (j0, j1) = ends[(c - 6) // 3], ends[(c - 6) % 3]
                xq, xk, d2 = _segments(q[..., i0:i0 + 3], q[..., i1:i1 + 3], k[..., j0:j0 + 3], k[..., j1:j1 + 3])
            xq, xk = xq.expand(shape + (3,)), xk.expand(shape + (3,))
            if best is None:
                best = [d2, xq, xk, torch.zeros(shape, dtype=torch.uint8, device=tris.device)]
                continue
            better = d2 < best[0]
            best = [torch.where(better, d2, best[0]), torch.where(better[..., None], xq, best[1]),
                    torch.where(better[..., None], xk, best[2]), torch.where(better, torch.full_like(best[3], c), best[3])]
        (qlo, qup), (lo, up) = _box(q), _box(k)
        near = ~((qup < lo) | (qlo > up)).any(dim=-1)
        cut, point = torch.zeros(shape, dtype=torch.bool, device=tris.device), torch.zeros(shape + (3,), dtype=tris.dtype, device=tris.device)
        tests = [(q[..., i0:i0 + 3], q[..., i1:i1 + 3], k) for i0, i1 in ends] + [(k[..., j0:j0 + 3], k[..., j1:j1 + 3], q) for j0, j1 in ends]
        for p0, p1, tri in tests:
            hit, x = _seg(p0, p1, tri)
            first = hit & near & ~cut
            point = torch.where(first[..., None], x, point)
            cut |= first
        d2 = torch.where(cut, torch.zeros_like(best[0]), best[0])
        xq, xk = torch.where(cut[..., None], point, best[1]), torch.where(cut[..., None], point, best[2])
        kind = torch.where(cut, torch.full_like(best[3], 15), best[3])
        valid = d2 <= float("inf")
        key = torch.where(valid, d2, torch.full_like(d2, float("inf")))
        cand = valid & (key == key.amin(dim=1, keepdim=True))
        n = k.shape[1]
        j = torch.where(cand, torch.arange(n, device=tris.device)[None], n).amin(dim=1)      # the first = the smallest index
        has = j < n
        j = j.clamp(max=n - 1)
        r = torch.arange(shape[0], device=tris.device)
        zero3 = torch.zeros((shape[0], 3), dtype=tris.dtype, device=tris.device)
        outs.append((torch.where(has, j + 1, 0).to(torch.int32), torch.where(has, d2[r, j], torch.full_like(d2[r, j], float("inf"))),
                     torch.where(has[:, None], xq[r, j], zero3), torch.where(has[:, None], xk[r, j], zero3),
                     torch.where(has, kind[r, j], torch.zeros_like(kind[r, j]))))
    return tuple(torch.cat(x) for x in zip(*outs))


def run(name, steps, warmup, gap_edges):
    tris, m = mesh(name)
    f32 = ibvh.BBox(torch.float32)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, f32), f32)
    edge = mean_edge(tris)
    q = torch.from_numpy(shifted(tris, m, gap_edges * edge)).cuda()
    order = api._morton_order((q[:, 0:3] + q[:, 3:6] + q[:, 6:9]) / 3)
    qs = q[order].contiguous()
    radius = 2 * gap_edges * edge
    launches = {"given_unbounded": Query(bvh, tdev, q), "sorted_unbounded": Query(bvh, tdev, qs),
                "given_within": Query(bvh, tdev, q, radius), "sorted_within": Query(bvh, tdev, qs, radius)}
    for f in launches.values():
        f()
    torch.cuda.synchronize()
    assert all(f.flag.item() == 0 for f in launches.values())
    given, srt = launches["given_unbounded"], launches["sorted_unbounded"]
    same = same_bits(given.outputs(), srt.outputs(order)) and same_bits(launches["given_within"].outputs(), launches["sorted_within"].outputs(order))
    kinds = torch.bincount(given.kind.to(torch.int64), minlength=16).tolist()
    out = {"workload": name, "triangles": int(tdev.shape[0]), "queries": m, "levels": int(bvh.tree.levels), "mean_edge": round(edge, 6),
           "gap_edges": gap_edges, "median_distance_edges": round(float(given.d2.sqrt().median().item()) / edge, 3),
           "answered_within": int((launches["given_within"].index != 0).sum().item()), "kinds": kinds, "sorted_equals_given": bool(same)}
    mirror = lambda: ibvh.triangle_distances(bvh, tdev, q)
    mirror_given = lambda: ibvh.triangle_distances(bvh, tdev, qs, presorted=True)
    mirror_within = lambda: ibvh.triangle_distances(bvh, tdev, q, max_distance=radius)
    whole_mesh = lambda: ibvh.mesh_distance(bvh, tdev, q)
    # for context: the shortcut on the queries' vertices, and "do they touch" on the same queries
    vertices = qs.reshape(-1, 3).contiguous()
    ci, cd2, cq = (torch.empty(3 * m, dtype=torch.int32, device="cuda"), torch.empty(3 * m, dtype=torch.float32, device="cuda"),
                   torch.empty((3 * m, 3), dtype=torch.float32, device="cuda"))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    struct = bvh.struct()
    closest = lambda: lib.call("ibvh_closest_triangles", C.byref(struct), api._ptr(tdev), tdev.shape[0], api._ptr(vertices), 3 * m, None,
                               api._ptr(ci), api._ptr(cd2), api._ptr(cq), api._ptr(flag), api._stream())
    counts = torch.empty(m, dtype=torch.int64, device="cuda")
    contacts = lambda: lib.call("ibvh_triangle_contacts", C.byref(struct), api._ptr(tdev), tdev.shape[0], api._ptr(qs), None, m,
                                abi.TRIS_COUNT, 0, api._ptr(counts), None, 0, None, None, None, api._ptr(flag), api._stream())
    closest()
    out["shortcut_wrong"] = int((cd2.reshape(m, 3).amin(dim=1) != srt.d2).sum().item())
    for _ in range(warmup):
        for f in list(launches.values()) + [mirror, mirror_given, mirror_within, whole_mesh, closest, contacts]:
            f()
    for key, f in launches.items():
        out["launch_" + key + "_ms"] = round(timed(f, steps), 4)
    k = max(2, steps // 2)
    out["mirror_ms"] = round(timed(mirror, k), 4)
    out["mirror_presorted_ms"] = round(timed(mirror_given, k), 4)
    out["mirror_within_ms"] = round(timed(mirror_within, k), 4)
    out["mesh_distance_ms"] = round(timed(whole_mesh, k), 4)
    out["closest_points_on_vertices_ms"] = round(timed(closest, steps), 4)
    out["triangle_contacts_count_ms"] = round(timed(contacts, steps), 4)
    md = whole_mesh()
    out["mesh_distance_edges"] = round(md.distance / edge, 4)
    return out


def against_torch(steps, warmup, gap_edges):
    tris, _ = mesh("small")
    f32 = ibvh.BBox(torch.float32)
    tdev = torch.from_numpy(tris).cuda()
    bvh = ibvh.BVH(ibvh.bounding_volumes_from_triangles(tdev, f32), f32)
    q = torch.from_numpy(shifted(tris, 10_000, gap_edges * mean_edge(tris))).cuda()
    order = api._morton_order((q[:, 0:3] + q[:, 3:6] + q[:, 6:9]) / 3)
    qs = q[order].contiguous()
    launch = Query(bvh, tdev, qs)
    brute = lambda: torch_brute_force(tdev, qs)
    for _ in range(warmup):
        launch()
    exp = brute()
    return {"triangles": int(tdev.shape[0]), "queries": int(qs.shape[0]), "launch_ms": round(timed(launch, steps), 4),
            "torch_all_pairs_ms": round(timed(brute, 2), 4), "bit_equal": bool(same_bits(launch.outputs(), exp))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="published,config3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gap", type=float, default=3.0, help="the shift of the queries, in mean edge lengths")
    a = ap.parse_args()
    out = {"bench_triangle_distances": [run(n, a.steps, a.warmup, a.gap) for n in a.workloads.split(",") if n],
           "torch": against_torch(a.steps, a.warmup, a.gap)}
    print(json.dumps(out), flush=True)
    if not all(w["sorted_equals_given"] for w in out["bench_triangle_distances"]):
        raise SystemExit("the sorted and the given order give different bits: the times are not like for like")
    if not out["torch"]["bit_equal"]:
        raise SystemExit("the torch brute force and the library give different bits")


if __name__ == "__main__":
    main()
