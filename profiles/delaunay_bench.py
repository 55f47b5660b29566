"""What the Delaunay monitor (TetrahedraTracer.delaunay_check), the per-tetrahedron state transfer (remap_tet_values) and a
re-triangulation (TetrahedraTracer.retriangulate) cost, against what they stand beside and what they replace.

    python profiles/delaunay_bench.py [--rounds 7] [--out profiles/delaunay_bench.txt]
    python profiles/delaunay_bench.py --kernels      7 x (delaunay_check, remap_tet_values) per mesh and nothing else timed: for
                                                     rocprofv3 --kernel-trace --stats -- python ... --kernels, a run of its own

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra), each moved by a Gaussian step of 5 % of the mean spacing so that there is something to find.  A
device-side candidate is timed over 20 back-to-back calls between two device events (per call: a launch or two and a fill):
  check        delaunay_check (counters only; with both optional arrays) by device events, beside limit_vertex_step and
               update_vertices on the same tracer for scale, against geometry.delaunay_face_statement in torch on the same GPU
               tensors and in numpy (copies to the host included): what a user would otherwise write
  transfer     remap_tet_values from the loaded cells to the re-triangulated ones, by device events
  retriangulate  its three parts by the wall clock, each synchronised: triangulate (Qhull on the CPU, with the copy to the host),
               the transfer, load_tetrahedra(refittable=True)
Needs the GPU; there is no fallback.

Expected before any run: one pass of the monitor moves about 8 B of face_tets per face and, per interior face, 32 B of cells and
five 12-byte vertex gathers -- 100 B --, with about 150 double operations per face behind them; like k_star_width (21 / 56 /
172 us at these sizes, profiles/vertex_guard_bench.txt) it should be bound by its gathers, not by arithmetic, at about twice the
lanes (F is about 2 T) and no atomics to speak of."""
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


def med(ts):
    return f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


REPS = 20       # calls per timed window of the device-side candidates: one call is tens of microseconds, too short for a window


def event_ms(fn, reps=REPS):
    """milliseconds per call over `reps` back-to-back calls, after two untimed ones (the candidate before it in the round may have
    left the device idle for a second: numpy, Qhull)"""
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


def interleaved(fns, rounds, warm=1):
    """fns: (callable, timer) pairs -> one list of milliseconds per pair"""
    for _ in range(warm):
        for f, _ in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, (f, timer) in enumerate(fns):
            ts[k].append(timer(f))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "delaunay_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    geometry = importlib.import_module("tetra-nerf_amd.geometry")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"delaunay_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        step = 0.05 / np.cbrt(points)
        moved = (pts + np.random.default_rng(seed + 100).normal(scale=step, size=pts.shape)).astype(np.float32)
        x0, x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(moved).to(dev), torch.from_numpy(cells).to(dev)
        tr = tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(x0, c, refittable=True)
        ft = tr.face_tables()[1].to(dev)
        T, F = len(cells), len(ft)
        if args.kernels:
            occupancy = torch.rand(T, device=dev)
            for _ in range(args.rounds):
                tr.delaunay_check(x)
                tn.cpp.remap_tet_values(c, c, occupancy, len(pts))
            torch.cuda.synchronize()
            say(f"kernels: {args.rounds} x (delaunay_check, remap_tet_values onto the same cells) at {T} tets, {F} faces done")
            tr.close()
            continue
        got = tr.delaunay_check(x, face_state=True, tet_violations=True)
        want = geometry.delaunay_face_statement(c, ft, x)
        same = all(torch.equal(got[k].long(), want[k].long()) for k in ("face_state", "tet_violations", "counters"))
        counters = got["counters"].tolist()
        work = x.clone()

        def limit():
            work.copy_(x)
            tr.limit_vertex_step(x0, work, 0.25)

        def numpy_statement():
            geometry.delaunay_face_statement(c.cpu().numpy(), ft.cpu().numpy(), x.cpu().numpy())

        t_chk, t_all, t_lim, t_refit, t_torch, t_numpy = interleaved(
            [(lambda: tr.delaunay_check(x), event_ms), (lambda: tr.delaunay_check(x, face_state=True, tet_violations=True), event_ms),
             (limit, event_ms), (lambda: tr.update_vertices(x0), event_ms),
             (lambda: geometry.delaunay_face_statement(c, ft, x), event_ms), (numpy_statement, wall_ms)], args.rounds)
        nbytes = 8 * F + 92 * counters[0]
        say(f"{name} {T} tets, {len(pts)} vertices, {F} faces, Gaussian step {step:.2e} (counters {counters}, kernel "
            f"{'==' if same else '!='} torch statement on the GPU):")
        say(f"  check        delaunay_check, counters only {med(t_chk)} = {nbytes / 1e6:.1f} MB of tables and gathers -> "
            f"{nbytes / m(t_chk) / 1e6:.0f} GB/s; with face_state and tet_violations {med(t_all)}")
        say(f"               for scale, same tracer: copy + limit_vertex_step {med(t_lim)}; update_vertices {med(t_refit)}")
        say(f"               the statement in torch on the GPU tensors {med(t_torch)} = {m(t_torch) / m(t_chk):.0f} x the kernel; in numpy, "
            f"copies to the host included {med(t_numpy)} = {m(t_numpy) / m(t_chk):.0f} x")
        # the transfer and the parts of a re-triangulation
        new_cells = tn.cpp.triangulate(x).to(torch.int32).contiguous()
        occupancy = torch.rand(T, device=dev)
        out = tn.cpp.remap_tet_values(c, new_cells, occupancy, len(pts))
        ok = torch.equal(out, geometry.remap_tet_values_statement(c, new_cells, occupancy, len(pts))["values"])
        t_remap, t_qhull, t_load = interleaved(
            [(lambda: tn.cpp.remap_tet_values(c, new_cells, occupancy, len(pts)), event_ms), (lambda: tn.cpp.triangulate(x), wall_ms),
             (lambda: tr.load_tetrahedra(x, new_cells, refittable=True), wall_ms)], args.rounds, warm=0)
        moved_bytes = 20 * T + 20 * len(new_cells) + 4 * len(pts)
        say(f"  transfer     remap_tet_values {T} -> {len(new_cells)} tets {med(t_remap)} (kernels {'==' if ok else '!='} statement): "
            f"{moved_bytes / 1e6:.1f} MB of cells and values, 4 T atomic maxima and 4 T' gathers -> {moved_bytes / m(t_remap) / 1e6:.0f} GB/s")
        say(f"  retriangulate  triangulate (Qhull, CPU) {med(t_qhull)}; transfer {med(t_remap)}; load_tetrahedra(refittable=True) {med(t_load)}: "
            f"Qhull is {m(t_qhull) / (m(t_qhull) + m(t_remap) + m(t_load)):.1%} of the call")
        after = tr.delaunay_check()["counters"].tolist()
        say(f"               afterwards: counters {after}")
        tr.close()


if __name__ == "__main__":
    main()
