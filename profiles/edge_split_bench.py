"""What the edge split costs (tn_edge_split_count_tables, tn_edge_split_emit, cpp.split_edges), against the same statement written in
torch on the same GPU tensors.

    python profiles/edge_split_bench.py [--rounds 7] [--out profiles/edge_split_bench.txt] [--sizes C2,C4,C5]

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra) with a tenth of the tetrahedra selected at random.  The face table is the tracer's own.
  count     tn_edge_split_count_tables alone, 20 back-to-back calls between two device events
  emit      tn_edge_split_emit alone on the count's arrays, outputs allocated once, the same way
  whole     cpp.split_edges: both entries, their allocations and the one read-back, by the wall clock
  torch     the same statement in torch on the GPU tensors, by the wall clock; its arrays are compared with the kernels' once
Needs the GPU; there is no fallback.

Expected before any run.  COUNT is a chain of eleven small launches: the nomination reads 17 B per tetrahedron and 48 B of
positions per asked one; the sort moves T 64-bit keys (2.4 / 7.2 / 24 MB per pass, 6 to 7 passes of 8 bits at these V); the row
pass reads EVERY row and its four positions (64 B per tetrahedron) and does six binary searches of ~17 steps in a list of 0.1 T
keys, which stays in L2; the hull pass reads 20 B per face.  The isosurface's emit, which sorts a third as many pairs, takes 0.07 /
0.09 / 0.18 ms: expect 0.1 / 0.2 / 0.5 ms here, the sort and the row pass sharing most of it.  EMIT reads 24 B and writes 20 B per
tetrahedron and copies the vertices: as tn_split_emit, 0.01 ms, launch-bound.  The torch statement needs a unique, six
searchsorted and several scatters: 10 x the entries or more."""
import argparse
import importlib
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SIZES = (("C2", 15000, 0), ("C4", 45000, 2), ("C5", 150000, 3))      # bench.py's meshes
FRACTION = 0.10
REPS = 20       # calls per timed window of the device-side candidates
EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def med(ts):
    return f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def event_ms(fn, reps=REPS):
    fn(); fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps=3):
    total = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t
    return 1e3 * total / reps


def interleaved(fns, rounds, warm=1):
    for _ in range(warm):
        for f, timer in fns:
            timer(f)
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, (f, timer) in enumerate(fns):
            ts[k].append(timer(f))
    return ts


def torch_statement(geometry, xyz, cells, select, faces, face_tets):
    """geometry.split_edges_statement in torch on the device of its arguments (every id valid, no NaN)"""
    dev = xyz.device
    V, T = xyz.shape[0], cells.shape[0]
    c = cells.long()
    p = xyz[c]
    rows = torch.arange(T, device=dev)
    a, b = (torch.tensor([e[k] for e in EDGE_CORNERS], device=dev) for k in (0, 1))
    a_low = c[:, a] < c[:, b]
    slot_lo, slot_hi = torch.where(a_low, a, b), torch.where(a_low, b, a)
    lo_id, hi_id = c.gather(1, slot_lo), c.gather(1, slot_hi)
    key = (lo_id << 32) | hi_id
    d = p[rows[:, None], slot_hi] - p[rows[:, None], slot_lo]
    len2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    beats = lambda le, ke, lf, kf: (le > lf) | ((le == lf) & (ke < kf))   # noqa: E731
    sign = lambda q: torch.sign(geometry._vol6(q.double()))   # noqa: E731
    s = sign(p)
    best = torch.zeros(T, dtype=torch.long, device=dev)
    for e in range(1, 6):
        best = torch.where(beats(len2[:, e], key[:, e], len2[rows, best], key[rows, best]), e, best)
    cand = torch.unique(key[rows, best][select.bool() & (s != 0)])
    C = cand.numel()

    def find(k):
        at = torch.searchsorted(cand, k)
        ok = (at < C) & (cand[at.clamp(max=max(C - 1, 0))] == k)
        return torch.where(ok, at, -1)

    found = find(key)
    w = torch.full((T,), -1, dtype=torch.long, device=dev)
    for e in range(6):
        wc = w.clamp(min=0)
        better = (found[:, e] >= 0) & ((w < 0) | beats(len2[:, e], key[:, e], len2[rows, wc], key[rows, wc]))
        w = torch.where(better, e, w)
    has_w, wc = w >= 0, w.clamp(min=0)
    lo_p, hi_p = p[rows, slot_lo[rows, wc]], p[rows, slot_hi[rows, wc]]
    mid = ((lo_p + hi_p) + (lo_p + hi_p)) * 0.25
    flat = s == 0
    for replaced in (slot_hi[rows, wc], slot_lo[rows, wc]):
        q = p.clone()
        q[rows, replaced] = mid
        flat |= sign(q) != s
    win = torch.where(has_w, found[rows, wc], -1)
    refused = torch.zeros(C, dtype=torch.bool, device=dev)
    lost = (found >= 0) & (found != win[:, None])
    refused[found[lost]] = True
    refused[win[has_w & flat]] = True
    hull = faces.long()[face_tets[:, 1] == -1]
    for k in range(3):
        u, v = hull[:, k], hull[:, (k + 1) % 3]
        at = find((torch.minimum(u, v) << 32) | torch.maximum(u, v))
        refused[at[at >= 0]] = True
    accepted = ~refused
    rank = torch.cumsum(accepted, 0) - 1
    bisected = has_w & accepted[win.clamp(min=0)]
    keys = cand[accepted]
    lo, hi = keys >> 32, keys & 0xFFFFFFFF
    vertices = torch.cat([xyz, ((xyz[lo] + xyz[hi]) + (xyz[lo] + xyz[hi])) * 0.25])
    parents = bisected.nonzero()[:, 0]
    j = rank[win[parents]]
    old = c[parents]
    child0 = torch.where(old == hi[j][:, None], (V + j)[:, None], old)
    child1 = torch.where(old == lo[j][:, None], (V + j)[:, None], old)
    out = torch.cat([c, child1])
    out[parents] = child0
    return {"vertices": vertices, "cells": out.int(), "cell_parent": torch.cat([rows, parents]).int(),
            "vertex_parents": torch.stack([lo, hi, lo, hi], 1).int(), "bisected": bisected.to(torch.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "edge_split_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    geometry = importlib.import_module("tetra-nerf_amd.geometry")
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"edge_split_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        V, T = len(pts), len(cells)
        x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev)
        tr = tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(x, c)
        faces, face_tets = (a.to(dev) for a in tr.face_tables())
        tr.close()
        F = faces.shape[0]
        stream = torch.cuda.current_stream().cuda_stream
        select = torch.from_numpy((np.random.default_rng(seed + 1).random(T) < FRACTION).astype(np.uint8)).to(dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)   # noqa: E731
        tet_offsets, tet_edge, bisected, edges, counters = i32(T + 1), i32(T), torch.empty(T, dtype=torch.uint8, device=dev), i32(T, 2), i32(10)

        def count():
            assert lib.tn_edge_split_count_tables(0, V, T, x.data_ptr(), c.data_ptr(), select.data_ptr(), F, faces.data_ptr(), face_tets.data_ptr(),
                                                  tet_offsets.data_ptr(), tet_edge.data_ptr(), bisected.data_ptr(), edges.data_ptr(),
                                                  counters.data_ptr(), stream) == 0

        count()
        n = counters.tolist()
        Kv, Kt = n[8], n[9]
        vertices, new_cells, parent, vp = torch.empty((V + Kv, 3), device=dev), i32(T + Kt, 4), i32(T + Kt), i32(Kv, 4)

        def emit():
            assert lib.tn_edge_split_emit(V, T, x.data_ptr(), c.data_ptr(), tet_offsets.data_ptr(), tet_edge.data_ptr(), edges.data_ptr(), Kv, Kt,
                                          vertices.data_ptr(), new_cells.data_ptr(), parent.data_ptr(), vp.data_ptr(), stream) == 0

        got = tn.cpp.split_edges(x, c, select, faces, face_tets)
        want = torch_statement(geometry, x, c, select, faces, face_tets)
        same = all(got[k].shape == want[k].shape and torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)) for k in want)
        t_count, t_emit, t_whole, t_torch = interleaved(
            [(count, event_ms), (emit, event_ms), (lambda: tn.cpp.split_edges(x, c, select, faces, face_tets), wall_ms),
             (lambda: torch_statement(geometry, x, c, select, faces, face_tets), wall_ms)], args.rounds)
        say(f"{name} {T} tets, {V} vertices, {F} faces, {FRACTION:.0%} selected: counters {n} (kernels {'==' if same else '!='} the torch statement "
            f"on the GPU, byte for byte):")
        say(f"  count     {med(t_count)}")
        say(f"  emit      {med(t_emit)}")
        say(f"  whole     cpp.split_edges {med(t_whole)}")
        say(f"  torch     the statement in torch on the GPU tensors {med(t_torch)} = {m(t_torch) / (m(t_count) + m(t_emit)):.1f} x (count + emit)")


if __name__ == "__main__":
    main()
