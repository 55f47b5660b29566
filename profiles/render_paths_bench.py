#!/usr/bin/env python3
"""Did the host path of TetraRenderer.render get slower?  This tree against a built checkout of the parent commit.

    python profiles/render_paths_bench.py PARENT_TREE [--runs 5] [--reps 5] [--out profiles/render_paths_bench.txt]

Alternating child processes (parent, this, parent, ...), `--runs` per side.  Each child imports ITS OWN tree -- package, library,
bench.py -- builds the scene of bench.py's render leg (random_mesh(15000, 0), the 800 x 800 frame of rank 0, M = 512, 256 coarse
samples, 65,536-ray chunks) and times the frame through render() at default (the persistent launch), with fused_pass=False (the
kernel chain), with an occupancy (random field, threshold 0.5) and with aux_outputs=True; the figure of a process is the median
over `--reps` frames after a warm-up frame.  Bar, per entry: the median of this tree's processes lies inside the min .. max of
the parent's own processes, or below it.  (profiles/render_paths_bench.txt holds this report and, behind it, that of
profiles/mlp_train_entries_bench.py PARENT_TREE for the training paths.)  Needs a GPU; there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def child(root, out_path, reps):
    sys.path.insert(0, root)
    import torch

    import bench

    tn = importlib.import_module("tetra-nerf_amd")
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    for m in (bench, tn, render, scenes):
        assert os.path.relpath(os.path.abspath(m.__file__), root).split(os.sep)[0] in ("bench.py", "tetra-nerf_amd"), "a module of another tree was imported"
    dev = torch.device("cuda:0")
    pts, cells = scenes.random_mesh(15000, 0)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = (torch.from_numpy(x).to(dev) for x in bench.frame_rays(scenes, 0, 800, 800))
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    field = (torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4
    field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
    occ = torch.rand(len(cells), generator=torch.Generator().manual_seed(1)).to(dev)
    entries = (("render default (persistent launch)", {}, {}), ("render fused_pass=False (kernel chain)", {"fused_pass": False}, {}),
               ("render occupancy + threshold", {}, {"occupancy": occ, "occupancy_threshold": 0.5}), ("render aux_outputs", {}, {"aux_outputs": True}))
    res = {}
    for name, rkw, ckw in entries:
        rd = render.TetraRenderer(tr, field, mlp, 256, 512, fused=True, **rkw)

        def frame():
            for s in range(0, o.shape[0], 65536):
                rd.render(o[s:s + 65536], d[s:s + 65536], **ckw)
            torch.cuda.synchronize()

        frame()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            frame()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = statistics.median(ms)
    Path(out_path).write_text(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree", nargs="?")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, metavar=("TREE", "JSON"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.child[0]), args.child[1], args.reps)
    sides = {"parent": (os.path.abspath(args.parent_tree), []), "this": (str(ROOT), [])}
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(args.runs):
            for side, (tree, runs) in sides.items():
                path = os.path.join(tmp, f"{side}_{k}.json")
                subprocess.run([sys.executable, __file__, "--child", tree, path, "--reps", str(args.reps)], check=True, timeout=300)
                runs.append(json.loads(Path(path).read_text()))
        lines, above = [f"render(): the 800 x 800 frame; {args.runs} processes per side, alternating; ms per frame", ""], 0
        for key in sides["parent"][1][0]:
            p, t = ([r[key] for r in sides[s][1]] for s in ("parent", "this"))
            med = statistics.median(t)
            verdict = "inside" if min(p) <= med <= max(p) else "below" if med < min(p) else "ABOVE"
            above += verdict == "ABOVE"
            lines += [key, "    parent  " + "  ".join(f"{x:8.3f}" for x in p) + f"   min {min(p):8.3f}  median {statistics.median(p):8.3f}  max {max(p):8.3f}",
                      "    this    " + "  ".join(f"{x:8.3f}" for x in t) + f"   median {med:8.3f}  ({med / statistics.median(p):.4f} x the parent's median): {verdict}"]
        lines += ["", f"{above} entries above the parent's range"]
    print("\n".join(lines))
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 1 if above else 0


if __name__ == "__main__":
    sys.exit(main())
