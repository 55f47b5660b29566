"""What the face table without a tracer costs (tn_face_table_count, tn_face_table_emit) beside the load it stands in for inside the
flip loop, and what TetrahedraTracer.flip_to_delaunay(reload="once") gains over reload="round" (the loop that loads every round).

    python profiles/face_table_bench.py [--rounds 7] [--sizes C2,C4,C5] [--out profiles/face_table_bench.txt]

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on the moved meshes of
profiles/flip_bench.py (bench.py's three meshes, about 100k / 300k / 1M tetrahedra, every vertex moved by a Gaussian step of 20 % of
the mean spacing under limit_vertex_step(fraction 0.45)).
  count        tn_face_table_count on the moved mesh's cells, by device events over 20 back-to-back calls
  emit         tn_face_table_emit into preallocated outputs (tet_faces included), likewise
  load         load_tetrahedra(refittable=True) on the same cells by the wall clock, synchronised: what a round of reload="round"
               pays for its table
  round        the whole flip_to_delaunay(reload="round") by the wall clock, synchronised, on a tracer freshly loaded with the moved
               mesh (that load is not timed): the yardstick
  once         the whole flip_to_delaunay(reload="once") likewise, its one final load included
The two repairs must agree in every round's counters and in the cells they return.  No target time is written down in advance: the
file reports what was measured.  Needs the GPU; there is no fallback."""
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "face_table_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"face_table_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
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
        tr.limit_vertex_step(x0, x, 0.45)                                    # x is shortened in place
        tr.load_tetrahedra(x, c, refittable=True)
        T, V = len(cells), len(pts)
        partner = torch.empty(4 * T, dtype=torch.int32, device=dev)
        face_index = torch.empty(4 * T + 1, dtype=torch.int32, device=dev)
        counters = torch.empty(4, dtype=torch.int32, device=dev)

        def count():
            _lib.check(lib.tn_face_table_count(0, V, T, c.data_ptr(), partner.data_ptr(), face_index.data_ptr(), counters.data_ptr(), None))

        count()
        F, hull, flags, _ = counters.tolist()
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        face_tets = torch.empty((F, 2), dtype=torch.int32, device=dev)
        tet_faces = torch.empty((T, 4), dtype=torch.int32, device=dev)

        def emit():
            _lib.check(lib.tn_face_table_emit(T, c.data_ptr(), partner.data_ptr(), face_index.data_ptr(), F, faces.data_ptr(),
                                              face_tets.data_ptr(), tet_faces.data_ptr(), None))

        emit()
        own = tr.face_tables()
        same = flags == 0 and torch.equal(faces.cpu(), own[0]) and torch.equal(face_tets.cpu(), own[1])
        results = {}

        def repair(mode):
            def run():
                results[mode] = tr.flip_to_delaunay(reload=mode)
            return run

        def reload():
            tr.load_tetrahedra(x, c, refittable=True)

        for f in (count, emit, repair("round"), reload, repair("once"), reload):   # warm-up
            f()
        t_count, t_emit, t_load, t_round, t_once = [], [], [], [], []
        for _ in range(args.rounds):
            t_count.append(event_ms(count))
            t_emit.append(event_ms(emit))
            t_round.append(wall_ms(repair("round")))
            t_load.append(wall_ms(reload))
            t_once.append(wall_ms(repair("once")))
            reload()
        a, b = results["round"], results["once"]
        agree = a["rounds"] == b["rounds"] and torch.equal(a["cells"], b["cells"]) and torch.equal(a["cell_sources"], b["cell_sources"])
        n = a["num_rounds"]
        say(f"{name} {T} tets, {V} vertices, {F} faces ({hull} on the hull), Gaussian step {step:.2e} under the limiter "
            f"(entries {'==' if same else '!='} the loaded tracer's table)")
        say(f"  count        tn_face_table_count {med(t_count)}")
        say(f"  emit         tn_face_table_emit {med(t_emit)}")
        say(f"  load         load_tetrahedra(refittable=True) {med(t_load)} = {m(t_load) / (m(t_count) + m(t_emit)):.1f} x the two entries")
        say(f"  round        flip_to_delaunay(reload=\"round\") {med(t_round)}: {n} rounds, {a['violated']} faces left violated, "
            f"T {T} -> {a['num_tetrahedra']}; its {n} loads are about {n * m(t_load) / m(t_round):.0%} of the call")
        say(f"  once         flip_to_delaunay(reload=\"once\") {med(t_once)}: {b['num_rounds']} rounds, results {'==' if agree else '!='} "
            f"reload=\"round\"; round / once = {m(t_round) / m(t_once):.2f} x; without its one load {m(t_once) - m(t_load):.3f} ms = "
            f"{(m(t_once) - m(t_load)) / max(n, 1):.3f} ms per round")
        tr.close()


if __name__ == "__main__":
    main()
