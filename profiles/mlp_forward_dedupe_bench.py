#!/usr/bin/env python3
"""Did the fused-MLP forward keep its speed?  This build against another build of the library (the parent commit's), in
alternating child processes (TETRANERF_HIP_LIB), the way train_x3_bench.py --parent-lib does, on the legs that run the code
the forward kernels share:

    python profiles/mlp_forward_dedupe_bench.py --parent-lib OLD.so [--rounds 7] [--out FILE]

  1. mlp_forward_gather (full network) and mlp_forward_gather_train, fp32 and bf16x3, n = 4096 x 513 samples;
  2. the training iteration of train_x3_bench.py, `tetra-nerf-original` and `tetra-nerf`, forward in fp32 and in bf16x3;
  3. the 800 x 800 frame of bench.py's render leg (15,000-point mesh, M = 512, 65,536-ray chunks, trace + compaction + the ONE
     persistent launch), `tetra-nerf-original` (256 + 256), fp32 and bf16x3.
Per process: the median of `rounds` warmed rounds; per leg: the median of the three processes' medians of each library, their
ratio, and the parent's own spread (max - min over its processes) -- the margin the ratio is read against.
Needs a GPU; there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_x3_bench as tb   # noqa: E402  (interleaved(), iteration_fns())


def child(rounds):
    import faulthandler

    import torch

    faulthandler.enable()
    tn = importlib.import_module("tetra-nerf_amd")
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    bench = importlib.import_module("bench")
    dev = torch.device("cuda:0")
    res = {}

    def run(fns, reps):
        for k, ms in tb.interleaved(torch, fns, rounds, reps=reps).items():
            res[k] = statistics.median(ms)

    V, R, S = 45000, 4096, 513
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(dev)
    w = [x.detach() for x in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=dev) * 0.7
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1)
    vi = torch.randint(0, V, (R * S, 4), dtype=torch.int32, device=dev)
    bc = (torch.rand(R * S, 3, device=dev) / 3).contiguous()
    fns = {}
    for m in ("fp32", "bf16x3"):
        fns[f"mlp_forward_gather {R}x{S} {m}"] = lambda m=m: tn.cpp.mlp_forward_gather(vi, bc, field, dirs, w, S, mode=m)
        fns[f"mlp_forward_gather_train {R}x{S} {m}"] = lambda m=m: tn.cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, mode=m)
    run(fns, 5)
    del fns, vi, bc
    run({f"training iteration {name} {mode}": fn
         for (name, mode), fn in tb.iteration_fns(torch, tn, dev, ("fp32", "bf16x3")).items()}, 5)

    pts, cells = scenes.random_mesh(15000, 0)
    tracer = tn.TetrahedraTracer(dev)
    tracer.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = bench.frame_rays(scenes, 0, 800, 800)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    field = ((torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4)
    field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
    fns = {}
    for m in ("fp32", "bf16x3"):
        rd = render.TetraRenderer(tracer, field, mlp, 256, 512, fused=True, num_fine_samples=256, mlp_mode=m)
        assert rd._one_launch_ok(m)

        def frame(rd=rd):
            for s in range(0, o.shape[0], 65536):
                rd.render(o[s:s + 65536], d[s:s + 65536])
        fns[f"render 800x800 tetra-nerf-original one launch {m}"] = frame
    run(fns, 2)
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mlp_forward_dedupe_bench.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.rounds)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    libs = {"parent": str(Path(args.parent_lib).resolve()), "branch": str(ROOT / "tetra-nerf_amd" / "libtetranerf_hip.so")}
    got = {k: {} for k in libs}
    for _ in range(args.processes):
        for k, path in libs.items():
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rounds", str(args.rounds)],
                               env=dict(os.environ, TETRANERF_HIP_LIB=path), capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # nothing further starts on the GPU
                raise RuntimeError(f"child process on {path} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1]
            for leg, ms in json.loads(line[6:]).items():
                got[k].setdefault(leg, []).append(ms)
            print(k, "process done", flush=True)
    lines = [f"ms per call; {args.processes} alternating processes per library, per process the median of {args.rounds} warmed rounds",
             f"{'leg':60s} {'parent (per process)':28s} {'branch (per process)':28s} {'parent':>8s} {'branch':>8s} {'ratio':>7s} {'spread':>7s}  verdict"]
    for leg in got["parent"]:
        a, b = got["parent"][leg], got["branch"][leg]
        ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
        lines.append(f"{leg:60s} {' '.join(f'{x:8.3f}' for x in a):28s} {' '.join(f'{x:8.3f}' for x in b):28s} {ma:8.3f} {mb:8.3f} "
                     f"{mb / ma:7.4f} {spread / ma * 100:6.2f}%  {'within' if mb - ma <= spread else 'SLOWER than parent + spread'}")
    print("\n".join(lines), flush=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
