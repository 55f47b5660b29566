"""What vertex pruning costs (tn_prune_count, tn_prune_emit, tn_prune_vertex_rows, TetrahedraTracer.remove_vertices), against the
same statement written in torch on the same GPU tensors, and against the Qhull triangulation and the reload that have to follow it.

    python profiles/prune_bench.py [--rounds 7] [--out profiles/prune_bench.txt] [--sizes C2,C4,C5]

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra, split_bench.py's) with a ball around (0.5, 0.5, 0.5) holding 10 % of the tetrahedra dead.  The field
is N(0, 1), f32 [64, V].
  count     tn_prune_count on the loaded mesh's own tables, 20 back-to-back calls between two device events
  emit      tn_prune_emit alone on the count's offsets, outputs allocated once, the same way
  rows vm   tn_prune_vertex_rows on the [64, V] field WITH its vertex-major shadow as values_vm, writing out and out_vm
  rows fm   the same WITHOUT values_vm: the kept columns are gathered from the feature-major array
  rows      the same without values_vm and without out_vm
  torch     the same statement in torch on the GPU tensors (cells, dead, the face table, vertices, the field), by the wall clock;
            its arrays are compared with the kernels' once
  qhull     triangulate() of the kept points, by the wall clock (one call per round)
  load      tracer.load_tetrahedra on the pruned mesh, by the wall clock
  whole     tracer.remove_vertices(dead, vertex_rows=(field,)), the unpruned mesh loaded again before each call
Needs the GPU; there is no fallback.

Expected before any run.  COUNT reads 17 B per tetrahedron, 20 B per face and writes three mark bytes and one keep word per
vertex: 2 .. 20 MB, launch-bound like tn_split_count (0.02 .. 0.04 ms: three kernels, one scan, one allocation, one memset).
EMIT reads 8 B and writes 4 B per vertex plus 16 B per kept one: below 5 MB, ~0.01 ms, launch-bound.  ROWS moves the field twice
with the shadow (256 V' B read as whole rows, 2 x 256 V' B written): like the split's new columns, 0.01 .. 0.05 ms, and without
the shadow the column gather of single floats should cost 2 .. 5 x that at 1M tetrahedra.  QHULL on 15k .. 150k points on the
host should take 0.1 .. 2 s and the LOAD 6 .. 30 ms: the two should dominate the whole call by three orders of magnitude over
the kernels, and the torch statement should sit at ~1 ms like the split's."""
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
DEAD = 0.10
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


def wall_ms(fn, reps=1, before=None):
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


def torch_statement(xyz, cells, dead, faces, face_tets, field):
    """geometry.prune_vertices_statement + prune_vertex_rows_statement in torch on the device of its arguments (every id valid)"""
    V, dev = xyz.shape[0], xyz.device
    c = cells.long()
    named, live, hull = (torch.zeros(V, dtype=torch.bool, device=dev) for _ in range(3))
    named[c.reshape(-1)] = True
    live[c[dead == 0].reshape(-1)] = True
    hull[faces[face_tets[:, 1] == -1].long().reshape(-1)] = True
    keep = live | hull | ~named
    kept_ids = keep.nonzero()[:, 0]
    offsets = torch.cat([keep.new_zeros(1, dtype=torch.int64), torch.cumsum(keep, 0)])
    new_id = torch.full((V,), -1, dtype=torch.int64, device=dev)
    new_id[kept_ids] = torch.arange(kept_ids.numel(), device=dev)
    out = field[:, kept_ids]
    return {"vertices": xyz[kept_ids], "new_id": new_id.int(), "kept_ids": kept_ids.int(), "offsets": offsets.int(), "field": out,
            "field_vm": out.t().contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prune_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"prune_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        V, T = len(pts), len(cells)
        x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev)
        dist = np.linalg.norm(pts.astype(np.float64)[cells].mean(1) - 0.5, axis=1)
        dead = torch.from_numpy((dist < np.quantile(dist, DEAD)).astype(np.uint8)).to(dev)
        torch.manual_seed(seed)
        field = torch.randn(64, V, device=dev)
        field_vm = field.t().contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        tr = tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(x, c)
        faces, face_tets = (t.to(dev) for t in tr.face_tables())
        F = faces.shape[0]
        offsets, counters = torch.empty(V + 1, dtype=torch.int32, device=dev), torch.empty(5, dtype=torch.int32, device=dev)

        def count():
            assert lib.tn_prune_count(tr._h, V, dead.data_ptr(), None, offsets.data_ptr(), counters.data_ptr(), stream) == 0

        count()
        Vp = int(offsets[V])
        vertices, new_id, kept = torch.empty((Vp, 3), device=dev), torch.empty(V, dtype=torch.int32, device=dev), torch.empty(Vp, dtype=torch.int32, device=dev)

        def emit():
            assert lib.tn_prune_emit(V, x.data_ptr(), offsets.data_ptr(), Vp, new_id.data_ptr(), kept.data_ptr(), vertices.data_ptr(), stream) == 0

        emit()
        out, out_vm = torch.empty((64, Vp), device=dev), torch.empty((Vp, 64), device=dev)

        def rows(vm, shadow):
            assert lib.tn_prune_vertex_rows(64, V, Vp, field.data_ptr(), field_vm.data_ptr() if vm else None, kept.data_ptr(), out.data_ptr(),
                                            out_vm.data_ptr() if shadow else None, stream) == 0

        want = torch_statement(x, c, dead, faces, face_tets, field)
        got = {"vertices": vertices, "new_id": new_id, "kept_ids": kept, "offsets": offsets}
        same = all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in got)
        for vm in (True, False):
            rows(vm, True)
            same = same and torch.equal(out.view(torch.int32), want["field"].view(torch.int32)) and torch.equal(out_vm.view(torch.int32), want["field_vm"].view(torch.int32))
        new_cells = tn.cpp.triangulate(vertices).to(torch.int32).contiguous()
        Tp = new_cells.shape[0]

        tr2 = tn.TetrahedraTracer(dev)                                  # the loads: `tr` keeps the unpruned mesh for the count

        def load_pruned():
            tr2.load_tetrahedra(vertices, new_cells)

        def load_unpruned():
            tr2.load_tetrahedra(x, c)

        whole = lambda f: wall_ms(f, before=load_unpruned)   # noqa: E731
        t = interleaved(
            [(count, event_ms), (emit, event_ms), (lambda: rows(True, True), event_ms), (lambda: rows(False, True), event_ms),
             (lambda: rows(False, False), event_ms), (lambda: torch_statement(x, c, dead, faces, face_tets, field), lambda f: wall_ms(f, reps=3)),
             (lambda: tn.cpp.triangulate(vertices), wall_ms), (load_pruned, lambda f: wall_ms(f, reps=3)),
             (lambda: tr2.remove_vertices(dead, vertex_rows=(field,)), whole)], args.rounds)
        t_count, t_emit, t_vm, t_fm, t_plain, t_torch, t_qhull, t_load, t_whole = t
        mb = lambda n: f"{n / 1e6:.1f} MB"   # noqa: E731
        say(f"{name} {T} tets, {V} vertices, {F} faces, {int(dead.sum())} dead: counters {counters.tolist()}, V' = {Vp}, T' = {Tp} "
            f"(kernels {'==' if same else '!='} the torch statement on the GPU, byte for byte):")
        say(f"  count     {med(t_count)}  must move {mb(17 * T + 20 * F + 3 * V + 4 * (V + 1))}, then one scan over {V + 1} words")
        say(f"  emit      {med(t_emit)}  must move {mb(8 * V + 4 * V + 16 * Vp)}")
        rb = 256 * Vp + 2 * 256 * Vp
        say(f"  rows vm   {med(t_vm)}  must move {mb(rb)} = {rb / 1e9 / m(t_vm):.2f} TB/s")
        say(f"  rows fm   {med(t_fm)}  must move {mb(rb)} = {rb / 1e9 / m(t_fm):.2f} TB/s")
        say(f"  rows      {med(t_plain)}  must move {mb(2 * 256 * Vp)} = {2 * 256 * Vp / 1e9 / m(t_plain):.2f} TB/s")
        say(f"  torch     the statement in torch on the GPU tensors {med(t_torch)} = {m(t_torch) / (m(t_count) + m(t_emit) + m(t_vm)):.1f} x (count + emit + rows vm)")
        say(f"  qhull     triangulate of the {Vp} kept points {med(t_qhull)}")
        say(f"  load      load_tetrahedra on the pruned mesh ({Tp} tets) {med(t_load)}")
        say(f"  whole     tracer.remove_vertices with the field {med(t_whole)} = qhull + load + {m(t_whole) - m(t_qhull) - m(t_load):.3f} ms")
        tr.close()
        tr2.close()


if __name__ == "__main__":
    main()
