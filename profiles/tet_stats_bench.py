"""What the per-tetrahedron training statistics cost (tn_tet_stats_accumulate, TetraRenderer.render_train(tet_stats=True) +
accumulate_tet_stats), against the same statement written in torch on the same GPU tensors, and what they leave of the default
path.

    python profiles/tet_stats_bench.py [--rounds 7] [--out profiles/tet_stats_bench.txt] [--ab PARENT_TREE [--this-first] [--ab-only]]

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's C4 mesh (45,000 points,
about 300k tetrahedra) and its training batch of 4096 outside-in rays, 513 final samples per ray (256 coarse + 256 fine + 1).
  kernel      tn_tet_stats_accumulate alone on the pending tensors of a real training batch, 20 back-to-back calls between two
              device events; then on the same sigma / edges with EVERY sample in tetrahedron 0 (all atomics on one row) and with
              every sample in a tetrahedron of its own (no run to fold: 3 atomics per sample) -- the two contention extremes
  torch       the same statement in torch: cpp.composite(sigma, None, edges) for the weights, clamps, torch.round, index_add_ on
              int64; its result is compared with the kernel's once (equal bytes)
  iteration   trace + render_train + loss + backward + SGD step for both shipped configurations, without and with tet_stats
              (with: + the per-ray squared error and accumulate_tet_stats), interleaved
  --ab        the DEFAULT iteration and an evaluation frame (65,536 rays) in fresh processes that alternate between this tree and
              the parent commit's tree given on the command line (each with its own build of the library): per-process medians,
              their median and spread per side (--this-first: this commit's process opens every pair; --ab-only: nothing
              else runs).  Without --ab this part reads "not measured".
Needs the GPU; there is no fallback.

Expected before any run.  The kernel reads 12 B per sample (cell, sigma, edge), 25 MB per batch: ~10 us of HBM traffic, so it
is bound by the composite's two wave scans per 64-sample chunk and by the fold's 6 x 5 cross-lane moves per chunk -- a little
above tn_composite without colours -- plus the atomics.  A tetrahedron holds ~10 .. 30 consecutive samples at this mesh size, so
~4096 * 513 / 20 = 100k runs, 300k 64-bit atomics per batch.  What 64-bit integer atomics cost on this part has not been
measured by anyone: one row for all of them is the worst case and should show it.  The iteration takes ~20 ms: anything below
0.1 ms is below 0.5 % of it and inside the round-to-round spread."""
import argparse
import importlib
import json
import statistics
import subprocess
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--ab", default=None, help="a checkout of the parent commit with its library built")
ap.add_argument("--processes", type=int, default=4, help="fresh processes per side of --ab")
ap.add_argument("--this-first", action="store_true", help="with --ab: this, parent, this, parent, ... instead of parent first")
ap.add_argument("--ab-only", action="store_true", help="with --ab: only the alternating processes")
ap.add_argument("--root", default=None, help="(child of --ab) the tree to import")
ap.add_argument("--default-only", action="store_true", help="(child of --ab) print one JSON line: default iteration and frame")
args = ap.parse_args()
ROOT = Path(args.root).resolve() if args.root else Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REPS, M = 20, 512
CONFIGS = (("tetra-nerf-original", (256, 256, False, False)), ("tetra-nerf", (128, 128, True, True)))
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(ts):
    return f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def ab_side(label, root, n):
    """n fresh processes' (iteration, frame) medians"""
    out = []
    for _ in range(n):
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--default-only", "--root", str(root), "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"{label}: child failed\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return out


ab = None
if args.ab and not args.default_only:
    # before this process opens the GPU: alternate parent, this, parent, this, ...
    ab = {"parent": [], "this": []}
    sides = (("parent", Path(args.ab)), ("this", ROOT))
    for _ in range(args.processes):
        for label, root in (sides[::-1] if args.this_first else sides):
            ab[label] += ab_side(label, root, 1)


def report_ab():
    say("default iteration (tetra-nerf-original) and evaluation frame (65,536 rays), fresh processes alternating "
        + ("this / parent commit:" if args.this_first else "parent / this commit:"))
    if ab is None:
        say("  not measured")
        return
    for key in ("iteration_ms", "frame_ms"):
        for side in ("parent", "this"):
            v = [p[key] for p in ab[side]]
            say(f"  {key:13s} {side:7s} {med(v)}   per process: {', '.join(f'{x:.3f}' for x in v)}")


if args.ab_only:
    report_ab()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")
    sys.exit(0)

import numpy as np   # noqa: E402
import torch   # noqa: E402

tn = importlib.import_module("tetra-nerf_amd")
render = importlib.import_module("tetra-nerf_amd.render")
scenes = importlib.import_module("tetra-nerf_amd.scenes")
dev = torch.device("cuda:0")
cpp = tn.cpp


def event_ms(fn, reps=REPS):
    fn(); fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


pts, cells_np = scenes.random_mesh(45000, 2)
T = len(cells_np)
tracer = tn.TetrahedraTracer(dev)
tracer.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells_np).to(dev))
o, d = (torch.from_numpy(a).to(dev) for a in scenes.outside_in_rays(4096, 1))
target = torch.rand(len(o), 3, device=dev)


def trainer(s_c, s_f, biased, scaling, with_stats):
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    field = ((torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4)
    field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
    field.requires_grad_(True)
    opt = torch.optim.SGD([field] + list(mlp.parameters()), lr=1e-3)
    rd = render.TetraRenderer(tracer, field, mlp, s_c, M, fused=True, num_fine_samples=s_f, biased=biased)
    stats = cpp.tet_stats_new(T, dev) if with_stats else None

    def step():
        opt.zero_grad(set_to_none=True)
        out = rd.render_train(o, d, gradient_scaling=scaling, **({"tet_stats": True} if with_stats else {}))
        err = ((out["rgb"] - target) ** 2)
        err.mean().backward()
        if with_stats:
            rd.accumulate_tet_stats(stats, out["tet_stats_pending"], err.sum(-1).detach())
        opt.step()
        return out
    return rd, step


if args.default_only:
    rd, step = trainer(*CONFIGS[0][1], False)
    fo, fd = (torch.from_numpy(a).to(dev) for a in scenes.outside_in_rays(65536, 5))
    with torch.no_grad():
        frame = lambda: rd.render(fo, fd)   # noqa: E731
        its, frs = [], []
        for _ in range(args.rounds):
            with torch.enable_grad():
                its.append(event_ms(step, 10))
            frs.append(event_ms(frame, 3))
    print(json.dumps({"iteration_ms": statistics.median(its), "frame_ms": statistics.median(frs)}))
    sys.exit(0)

say(f"tn_tet_stats_accumulate on {torch.cuda.get_device_name(0)}; C4 mesh: {len(pts)} vertices, {T} tetrahedra; 4096 rays; "
    f"medians (min .. max) of {args.rounds} interleaved rounds, {REPS} calls per window")

# ---- the kernel alone and the torch statement, on the pending tensors of a real batch ----------------------------------------
rd, step = trainer(*CONFIGS[0][1], True)
pending = step()["tet_stats_pending"]
cells, sigma, edges, ridx, count = (pending[k] for k in ("cell_indices", "sigma", "edges", "ray_index", "count"))
r, S = cells.shape
ray_value = 3 * torch.rand(len(o), device=dev)
valid = (cells >= 0) & (cells < T)
runs = int((valid & torch.cat([torch.ones_like(cells[:, :1], dtype=torch.bool), cells[:, 1:] != cells[:, :-1]], 1)).sum())
say(f"batch: {r} rows x {S} samples, count = {None if count is None else int(count.item())}, {int(valid.sum())} matched samples in {runs} runs "
    f"({int(valid.sum()) / max(runs, 1):.1f} samples per run), {int(torch.unique(cells[valid]).numel())} distinct tetrahedra")
patterns = {"batch": (cells, T), "one tetrahedron": (torch.zeros_like(cells), T),
            "all distinct": (torch.arange(r * S, device=dev, dtype=torch.int32).view(r, S), r * S)}


def torch_statement(stats, cells, n_cells):
    w = cpp.composite(sigma, None, edges)
    rows = r if count is None else int(count.item())       # (the read-back the kernel does not need)
    c, w = cells[:rows].long(), w[:rows]
    v = ray_value[ridx[:rows].long()]
    wh = torch.where(w >= 0, w.clamp_max(1.0), torch.zeros_like(w))
    vh = torch.where(v >= 0, v.clamp_max(256.0), torch.zeros_like(v))
    ok = (c >= 0) & (c < n_cells)
    terms = torch.stack([torch.ones_like(c), torch.round(wh * 2.0 ** 32).long(), torch.round((wh * vh[:, None]) * 2.0 ** 32).long()], -1)
    return stats.index_add_(0, c[ok], terms[ok])


cands = {}
for name, (c, n_cells) in patterns.items():
    st_k, st_t = cpp.tet_stats_new(n_cells, dev), cpp.tet_stats_new(n_cells, dev)
    cpp.tet_stats_accumulate(st_k, c, sigma, edges, ray_value=ray_value, ray_index=ridx, count=count)
    torch_statement(st_t, c, n_cells)
    say(f"  {name}: kernel == torch statement: {bool(torch.equal(st_k, st_t))}")
    cands[f"kernel, {name}"] = (lambda st=st_k, c=c: cpp.tet_stats_accumulate(st, c, sigma, edges, ray_value=ray_value, ray_index=ridx, count=count))
    cands[f"torch,  {name}"] = (lambda st=st_t, c=c, n=n_cells: torch_statement(st, c, n))
cands["composite weights alone (tn_composite, no colours)"] = lambda: cpp.composite(sigma, None, edges)
times = {k: [] for k in cands}
for _ in range(args.rounds):
    for k, fn in cands.items():
        times[k].append(event_ms(fn, REPS if k.startswith("kernel") or k.startswith("composite") else 5))
for k in cands:
    say(f"  {k:52s} {med(times[k])}")
say(f"  reads: {12 * r * S / 1e6:.1f} MB per batch; atomics: {3 * runs} on the batch, {3 * r} on one tetrahedron (the carry: 3 per row), {3 * r * S} all distinct")

# ---- a training iteration without and with tet_stats, both shipped configurations --------------------------------------------
for name, cfg in CONFIGS:
    steps = {"without": trainer(*cfg, False)[1], "with tet_stats": trainer(*cfg, True)[1]}
    ts = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, fn in steps.items():
            ts[k].append(event_ms(fn, 10))
    say(f"iteration, {name}:")
    for k in steps:
        say(f"  {k:16s} {med(ts[k])}")
    say(f"  difference of the medians: {statistics.median(ts['with tet_stats']) - statistics.median(ts['without']):+.3f} ms")

# ---- the default path against the parent commit ----------------------------------------------------------------------------
report_ab()

if args.out:
    Path(args.out).write_text("\n".join(lines) + "\n")
