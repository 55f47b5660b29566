"""What the Delaunay repair by flips costs (tn_flip_count, tn_flip_emit_loaded, TetrahedraTracer.flip_to_delaunay), against the
re-triangulation it stands in for (TetrahedraTracer.retriangulate: Qhull on the CPU) and against the numpy statement.

    python profiles/flip_bench.py [--rounds 7] [--sizes C2,C4,C5] [--out profiles/flip_bench.txt]

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra).  Each mesh is moved by a Gaussian step of 20 % of the mean spacing, shortened by
limit_vertex_step(fraction 0.45) so that no tetrahedron inverts -- the repair's precondition --, which leaves roughly a tenth of
the interior faces violated.
  count        tn_flip_count on the tracer's own tables (first round), by device events over 20 back-to-back calls
  emit         tn_flip_emit_loaded into preallocated outputs, likewise
  statement    geometry.flip_faces_statement in numpy on the same round, copies to the host included, by the wall clock (there is
               no torch statement of the flip; the numpy one is what the tests compare with)
  repair       the whole flip_to_delaunay call by the wall clock, synchronised, on a tracer freshly loaded with the moved mesh
               (the load is not timed); rounds, what is left violated / unflippable, and the share of the call spent in the reloads
  retriangulate  the whole retriangulate call on the same input, likewise
No target time is written down in advance: the file reports what was measured.  Needs the GPU; there is no fallback."""
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
REPS = 20


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "flip_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    geometry = importlib.import_module("tetra-nerf_amd.geometry")
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"flip_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        step = 0.2 / np.cbrt(points)
        moved = (pts + np.random.default_rng(seed + 100).normal(scale=step, size=pts.shape)).astype(np.float32)
        x0, x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(moved).to(dev), torch.from_numpy(cells).to(dev)
        tr = tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(x0, c, refittable=True)
        limited = tr.limit_vertex_step(x0, x, 0.45)[0].tolist()              # x is shortened in place
        tr.load_tetrahedra(x, c, refittable=True)
        T, V = len(cells), len(pts)
        count = tr.flip_count()
        first = count["counters"].tolist()
        F = count["face_flip"].size(0)
        K23, K32 = first[8], first[9]
        new_cells = torch.empty((T + K23 - K32, 4), dtype=torch.int32, device=dev)
        sources = torch.empty((T + K23 - K32, 3), dtype=torch.int32, device=dev)

        def emit():
            _lib.check(lib.tn_flip_emit_loaded(tr._h, count["tet_offsets"].data_ptr(), count["tet_flip"].data_ptr(),
                                               count["face_flip"].data_ptr(), K23, K32, new_cells.data_ptr(), sources.data_ptr(), None))

        faces, face_tets = (a.numpy() for a in tr.face_tables())

        def statement():
            return geometry.flip_faces_statement(x.cpu().numpy(), c.cpu().numpy(), faces, face_tets)

        emit()
        want = statement()
        same = want["counters"].tolist() == first and np.array_equal(new_cells.cpu().numpy(), want["cells"]) and \
            np.array_equal(sources.cpu().numpy(), want["cell_sources"])
        results = {}

        def repair():
            results["flip"] = tr.flip_to_delaunay()

        def qhull():
            results["qhull"] = tr.retriangulate(x)

        def reload():
            tr.load_tetrahedra(x, c, refittable=True)

        for f in (tr.flip_count, emit, repair, reload, qhull, reload):       # warm-up
            f()
        t_count, t_emit, t_stmt, t_repair, t_qhull, t_load = [], [], [], [], [], []
        for _ in range(args.rounds):
            t_count.append(event_ms(tr.flip_count))
            t_emit.append(event_ms(emit))
            t_stmt.append(wall_ms(statement))
            t_repair.append(wall_ms(repair))
            t_load.append(wall_ms(reload))
            t_qhull.append(wall_ms(qhull))
            after = tr.delaunay_check()["counters"].tolist()
            reload()
        out = results["flip"]
        say(f"{name} {T} tets, {V} vertices, {F} faces, Gaussian step {step:.2e} under the limiter (clamped {limited[0]}, flipped {limited[2]}): "
            f"{first[1]} of {first[0]} interior faces violated = {first[1] / max(first[0], 1):.1%}; first round {first} "
            f"(kernels {'==' if same else '!='} numpy statement)")
        say(f"  count        tn_flip_count {med(t_count)}")
        say(f"  emit         tn_flip_emit_loaded ({K23} 2-3, {K32} 3-2 flips) {med(t_emit)}")
        say(f"  statement    geometry.flip_faces_statement in numpy, copies included {med(t_stmt)} = {m(t_stmt) / (m(t_count) + m(t_emit)):.0f} x the two entries")
        reloads = out["num_rounds"] * m(t_load)
        say(f"  repair       flip_to_delaunay {med(t_repair)}: {out['num_rounds']} rounds, {out['violated']} faces left violated "
            f"({out['violated'] / max(first[1], 1):.2%} of those at the start; unflippable {out['unflippable']}), T {T} -> {out['num_tetrahedra']}; "
            f"one load_tetrahedra(refittable=True) {med(t_load)}, so the {out['num_rounds']} reloads are about {reloads / m(t_repair):.0%} of the call")
        say(f"  retriangulate  the whole call (Qhull on the CPU, the load) {med(t_qhull)} = {m(t_qhull) / m(t_repair):.2f} x flip_to_delaunay; "
            f"afterwards the monitor reports {after}")
        tr.close()


if __name__ == "__main__":
    main()
