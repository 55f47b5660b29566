"""What the tetrahedron split costs (tn_split_count, tn_split_emit, tn_split_vertex_rows, TetrahedraTracer.split_tetrahedra), against
the same statement written in torch on the same GPU tensors, and against the reload that has to follow it.

    python profiles/split_bench.py [--rounds 7] [--out profiles/split_bench.txt] [--sizes C2,C4,C5]

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra) with 1 % and 10 % of the tetrahedra selected at random.  The field is N(0, 1), f32 [64, V].
  count     tn_split_count alone, 20 back-to-back calls between two device events
  emit      tn_split_emit alone on the count's offsets, outputs allocated once, the same way
  rows vm   tn_split_vertex_rows on the [64, V] field WITH its vertex-major shadow as values_vm, writing out and out_vm
  rows fm   the same WITHOUT values_vm: the parent columns are gathered from the feature-major array and the old part of out_vm
            is a transposition, not a copy
  new vm / new fm   the two gather sources alone: the same two calls without out_vm, minus `copy`
  copy      tn_split_vertex_rows with the same V and ONE new vertex and no out_vm: the row copy between the two strides
  torch     the same statement in torch on the GPU tensors (cells, vertices, parents, the field and its shadow), by the wall clock;
            its arrays are compared with the kernels' once
  reload    tracer.load_tetrahedra on the split mesh, by the wall clock
  whole     tracer.split_tetrahedra(select, vertex_rows=(field,)): both entries, the read-back, the field, and the reload
Needs the GPU; there is no fallback.

Expected before any run.  COUNT reads 17 B per tetrahedron and 48 B of positions per asked one and writes 4 B; its five
orientations are ~150 double operations on the asked tetrahedra only.  It should sit beside k_iso_count (3 .. 8 us,
profiles/isosurface_bench.txt) plus one scan, i.e. 15 .. 30 us per call, launch-bound, barely ordered by size.  EMIT reads 24 B and
writes 20 B per tetrahedron plus 92 B per accepted one and copies the 12 V bytes of the vertices: 5 / 14 / 46 MB at 10 %, a few
us of traffic; 10 .. 25 us per call, again launch-bound.  ROWS moves the field once or twice: 256 V B read, 256 (V + K) B written,
doubled with the shadow -- 16 / 47 / 160 MB at 10 % with the shadow.  At 2 .. 4 TB/s of cache-resident traffic that is 8 / 20 /
60 us; the strided copy has unaligned 16-byte loads and should stay within 1.5 x of a plain copy.  The gather of the new columns
is 4 K rows of 256 B from the shadow, or 4 * 64 * K single floats from the feature-major array, each of which pulls a whole
line: the shadow should win the gather by 3 x or more, but the gather is K / V ~ 7 % (1 %) to 70 % (10 %: K = 0.1 T = 0.67 V) of
the copy's elements, so on the whole call the difference should be visible at 10 % only.  Without values_vm the old part of the
shadow is a transposition instead of a copy, which costs about the same bytes.  The RELOAD (6 .. 27 ms on the unsplit meshes,
larger on the split ones) should dominate the whole operation by two orders of magnitude: the whole call = reload + ~0.3 ms."""
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
FRACTIONS = (0.01, 0.10)
REPS = 20       # calls per timed window of the device-side candidates


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


def wall_ms(fn, reps=3, before=None):
    total = 0.0
    for _ in range(reps):
        if before is not None:
            before()
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


def torch_statement(geometry, xyz, cells, select, field):
    """geometry.split_tetrahedra_statement + split_vertex_rows_statement in torch on the device of its arguments (every id valid)"""
    dev = xyz.device
    V, T = xyz.shape[0], cells.shape[0]
    c = cells.long()
    p = xyz[c]
    cen = ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])) * 0.25
    sign = lambda q: torch.sign(geometry._vol6(q.double()))   # noqa: E731
    s = sign(p)
    fine = select.bool() & (s != 0)
    for i in range(4):
        q = p.clone()
        q[:, i] = cen
        fine &= sign(q) == s
    parents = fine.nonzero()[:, 0]
    K = parents.numel()
    vertices = torch.cat([xyz, cen[parents]])
    new_id = V + torch.arange(K, device=dev)
    out = torch.cat([c, c.new_zeros((3 * K, 4))])
    for i in range(4):
        child = c[parents].clone()
        child[:, i] = new_id
        out[parents if i == 0 else T + 3 * torch.arange(K, device=dev) + (i - 1)] = child
    cell_parent = torch.cat([torch.arange(T, device=dev), parents.repeat_interleave(3)])
    vp = c[parents]
    a, b, cc, d = (field[:, vp[:, j]] for j in range(4))
    grown = torch.cat([field, ((a + b) + (cc + d)) * 0.25], 1)
    return {"vertices": vertices, "cells": out.int(), "cell_parent": cell_parent.int(), "vertex_parents": vp.int(), "field": grown,
            "field_vm": grown.t().contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "split_bench.txt"))
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

    say(f"split_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        V, T = len(pts), len(cells)
        x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev)
        torch.manual_seed(seed)
        field = torch.randn(64, V, device=dev)
        field_vm = field.t().contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        tr = tn.TetrahedraTracer(dev)
        for fraction in FRACTIONS:
            select = torch.from_numpy((np.random.default_rng(seed + 1).random(T) < fraction).astype(np.uint8)).to(dev)
            offsets, counters = torch.empty(T + 1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev)

            def count():
                assert lib.tn_split_count(V, T, x.data_ptr(), c.data_ptr(), select.data_ptr(), offsets.data_ptr(), counters.data_ptr(), stream) == 0

            count()
            K = int(offsets[T])
            asked = int(counters[0])
            vertices = torch.empty((V + K, 3), device=dev)
            new_cells, parent = torch.empty((T + 3 * K, 4), dtype=torch.int32, device=dev), torch.empty(T + 3 * K, dtype=torch.int32, device=dev)
            vp = torch.empty((K, 4), dtype=torch.int32, device=dev)

            def emit():
                assert lib.tn_split_emit(V, T, x.data_ptr(), c.data_ptr(), offsets.data_ptr(), K, vertices.data_ptr(), new_cells.data_ptr(),
                                         parent.data_ptr(), vp.data_ptr(), stream) == 0

            emit()
            out, out_vm = torch.empty((64, V + K), device=dev), torch.empty((V + K, 64), device=dev)
            out1 = torch.empty((64, V + 1), device=dev)

            def rows(vm, shadow, k=K, dst=out):
                assert lib.tn_split_vertex_rows(64, V, k, field.data_ptr(), field_vm.data_ptr() if vm else None, vp.data_ptr(), 0,
                                                dst.data_ptr(), out_vm.data_ptr() if shadow else None, stream) == 0

            got = tn.cpp.split_tetrahedra(x, c, select)
            want = torch_statement(geometry, x, c, select, field)
            rows(True, True)
            same = all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in ("vertices", "cells", "cell_parent", "vertex_parents"))
            same = same and torch.equal(out.view(torch.int32), want["field"].view(torch.int32)) and torch.equal(out_vm.view(torch.int32), want["field_vm"].view(torch.int32))
            rows(False, True)
            same = same and torch.equal(out.view(torch.int32), want["field"].view(torch.int32)) and torch.equal(out_vm.view(torch.int32), want["field_vm"].view(torch.int32))

            def reload_split():
                tr.load_tetrahedra(got["vertices"], got["cells"])

            def load_unsplit():
                tr.load_tetrahedra(x, c)

            whole = lambda f: wall_ms(f, before=load_unsplit)   # noqa: E731
            t = interleaved(
                [(count, event_ms), (emit, event_ms), (lambda: rows(True, True), event_ms), (lambda: rows(False, True), event_ms),
                 (lambda: rows(True, False), event_ms), (lambda: rows(False, False), event_ms), (lambda: rows(False, False, 1, out1), event_ms),
                 (lambda: torch_statement(geometry, x, c, select, field), wall_ms), (reload_split, wall_ms),
                 (lambda: tr.split_tetrahedra(select, vertex_rows=(field,)), whole)], args.rounds)
            t_count, t_emit, t_vm, t_fm, t_nvm, t_nfm, t_copy, t_torch, t_reload, t_whole = t
            mb = lambda n: f"{n / 1e6:.1f} MB"   # noqa: E731
            say(f"{name} {T} tets, {V} vertices, {fraction:.0%} selected: {asked} asked, {K} accepted (kernels {'==' if same else '!='} the torch "
                f"statement on the GPU, byte for byte):")
            say(f"  count     {med(t_count)}  must move {mb(17 * T + 48 * asked + 4 * (T + 1))}, then one scan over {T + 1} words")
            say(f"  emit      {med(t_emit)}  must move {mb(24 * T + 48 * K + 12 * V + 20 * (T + 3 * K) + 12 * (V + K) + 16 * K)}")
            say(f"  rows vm   {med(t_vm)}  must move {mb(2 * 256 * V + 2 * 256 * (V + K) + 4 * 256 * K)} = {(2 * 256 * V + 2 * 256 * (V + K) + 4 * 256 * K) / 1e9 / m(t_vm):.2f} TB/s")
            say(f"  rows fm   {med(t_fm)}  must move {mb(2 * 256 * V + 2 * 256 * (V + K) + 4 * 256 * K)} = {(2 * 256 * V + 2 * 256 * (V + K) + 4 * 256 * K) / 1e9 / m(t_fm):.2f} TB/s")
            say(f"  copy      {med(t_copy)}  must move {mb(2 * 256 * V)} = {2 * 256 * V / 1e9 / m(t_copy):.2f} TB/s")
            say(f"  new vm    {med(t_nvm)} - copy = {m(t_nvm) - m(t_copy):.3f} ms for {mb(5 * 256 * K)} of whole rows")
            say(f"  new fm    {med(t_nfm)} - copy = {m(t_nfm) - m(t_copy):.3f} ms for {4 * 64 * K} single floats and {mb(256 * K)} written")
            say(f"  torch     the statement in torch on the GPU tensors {med(t_torch)} = {m(t_torch) / (m(t_count) + m(t_emit) + m(t_vm)):.1f} x (count + emit + rows vm)")
            say(f"  reload    load_tetrahedra on the split mesh ({T + 3 * K} tets) {med(t_reload)}")
            say(f"  whole     tracer.split_tetrahedra with the field {med(t_whole)} = reload + {m(t_whole) - m(t_reload):.3f} ms")
        tr.close()


if __name__ == "__main__":
    main()
