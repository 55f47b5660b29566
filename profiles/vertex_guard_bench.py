"""What the vertex step limiter (TetrahedraTracer.limit_vertex_step) costs, against what it stands beside and what it replaces.

    python profiles/vertex_guard_bench.py cost        limit_vertex_step with and without the verify pass against (a) update_vertices
                                                      and (b) geometry.limit_vertex_step_statement on the GPU tensors (what a user
                                                      would otherwise write) at ~100k / 300k / 1M tets, one process, interleaved
    python profiles/vertex_guard_bench.py kernels     limit + refit in turn, nothing else (for rocprofv3 --kernel-trace --stats --
                                                      python ... kernels: (c) k_star_width against k_refit_tet_thin, same process)

Both need the GPU and APPEND their lines to --out (default profiles/vertex_guard_bench.txt).  Device events around the calls
(the limiter never synchronises; update_vertices is blocking, so its figure includes its two read-backs).  Medians (min .. max).
The default path against the parent build: profiles/refit_bench.py default LABEL --out profiles/vertex_guard_bench.txt, run
alternately with TETRANERF_HIP_LIB=<the parent commit's library> and without.

Expected before any run: the refit's thin pass has the same gathers and the same 4T atomic minima (21 / 56 / 173 us in
profiles/refit_bench.txt) and is bound by those atomics; the star pass adds three cross products and a maximum in double.  So
k_star_width within about 1.5 x of k_refit_tet_thin; the clamp moves 28 B per vertex and the verify pass gathers twice what
the star pass gathers without its atomics."""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SIZES = (("C2", 15000, 0), ("C4", 45000, 2), ("C5", 150000, 3))      # bench.py's meshes


def med(ts):
    return f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(fns, rounds, warm=2):
    for _ in range(warm):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(event_ms(f))
    return ts


def case(tn, scenes, geometry, dev, points, seed):
    """a tracer loaded refittable on a random mesh, its vertices, and a raw step of 3 star widths (tests/vertex_guard_cases.py)"""
    pts, cells = scenes.random_mesh(points, seed)
    x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(x, c, refittable=True)
    star = tr.tet_quality()["star_width"]
    star = torch.where(torch.isfinite(star), star, torch.zeros_like(star))
    g = torch.Generator(device=dev).manual_seed(11)
    v = torch.randn(x.shape, device=dev, generator=g)
    raw = x + 3.0 * star[:, None] * v / v.norm(dim=1, keepdim=True)
    return tr, x, c, raw


def cost(tn, scenes, geometry, dev, rounds, lines):
    for name, points, seed in SIZES:
        tr, x, c, raw = case(tn, scenes, geometry, dev, points, seed)
        work = raw.clone()

        def limit(verify):
            work.copy_(raw)
            return tr.limit_vertex_step(x, work, 0.45, verify=verify)

        counters, _ = limit(True)
        want = geometry.limit_vertex_step_statement(x, raw, c, 0.45)
        same = torch.equal(work.view(torch.int32), want["xyz"].view(torch.int32)) and counters.tolist() == want["counters"].tolist()
        t_copy, t_v, t_nv, t_refit, t_stmt = interleaved(
            [lambda: work.copy_(raw), lambda: limit(True), lambda: limit(False), lambda: tr.update_vertices(x),
             lambda: geometry.limit_vertex_step_statement(x, raw, c, 0.45)], rounds)
        m = statistics.median
        lines.append(f"{name} {len(c)} tets, {len(x)} vertices (counters {counters.tolist()}, kernels {'==' if same else '!='} statement on "
                     f"the GPU): the copy that resets the step {med(t_copy)}; copy + limit_vertex_step with verify {med(t_v)}, without "
                     f"{med(t_nv)}; (a) update_vertices {med(t_refit)}; (b) the torch statement on the GPU tensors {med(t_stmt)} = "
                     f"{m(t_stmt) / (m(t_v) - m(t_copy)):.0f} x the limiter with verify")
        print(lines[-1], flush=True)


def kernels(tn, scenes, geometry, dev, rounds, lines):
    for name, points, seed in SIZES:
        tr, x, c, raw = case(tn, scenes, geometry, dev, points, seed)
        work = raw.clone()
        for _ in range(rounds):
            work.copy_(raw)
            tr.limit_vertex_step(x, work, 0.45)
            tr.update_vertices(x)
        torch.cuda.synchronize()
        lines.append(f"kernels: {rounds} x (limit, refit) at {len(c)} tets done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("cost", "kernels"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vertex_guard_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    geometry = importlib.import_module("tetra-nerf_amd.geometry")
    lines = [f"vertex_guard_bench {args.mode}: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max)"]
    {"cost": cost, "kernels": kernels}[args.mode](tn, scenes, geometry, dev, args.rounds, lines)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
