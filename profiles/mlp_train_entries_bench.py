#!/usr/bin/env python3
"""Did the host paths of the fused MLP training stages get slower?  This tree against a built checkout of the parent commit.

    python profiles/mlp_train_entries_bench.py PARENT_TREE [--runs 5] [--rounds 5] [--out profiles/mlp_train_entries_bench.txt]

Alternating child processes (parent, this, parent, ...), `--runs` per side.  Each child imports ITS OWN tree -- package, library,
bench.py, profiles/ -- builds the C4-sized mesh (45,000 points, seed 2) and runs
  * the training leg of bench.py: 4096 outside-in rays, both shipped configurations, fused and PyTorch autograd;
  * the iteration leg of profiles/occupancy_train_bench.py: no occupancy, a threshold that culls nothing, synthetic occupancies
    at the thresholds 0.5 / 0.9, all three arithmetic switches fp32 and all three bf16x3 (`--rounds` interleaved rounds; the
    figure of a process is the median over its rounds).
Bar, per entry: the median of this tree's processes lies inside the min .. max of the parent's own processes, or below it.  The
first child that fails ends the run.  Needs a GPU; there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def child(root, out_path, rounds):
    sys.path[:0] = [root, os.path.join(root, "profiles")]
    import torch

    import bench
    import occupancy_train_bench as otb

    tn = importlib.import_module("tetra-nerf_amd")
    assert all(os.path.abspath(m.__file__).startswith(root) for m in (bench, otb, tn)), "a module of another tree was imported"
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    dev = torch.device("cuda:0")
    pts, cells = scenes.random_mesh(45000, 2)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    leg = bench.train_leg(tn, tr, len(pts), scenes, 512, dev)
    res = {f"bench.py train step | {name} | {what}": leg[name][what]["ms_per_iteration"]
           for name in ("tetra-nerf-original", "tetra-nerf") for what in ("fused", "pytorch_autograd")}
    del tr
    records, interleaved = [], otb.interleaved
    otb.interleaved = lambda *a, **k: (lambda r: (records.append(r), r)[1])(interleaved(*a, **k))
    otb.iteration_leg(torch, tn, dev, rounds, lambda line: None)
    groups = [(name, modes) for name, _ in otb.CONFIGS for modes in ("fp32", "bf16x3")]
    assert len(records) == len(groups)
    for (name, modes), rec in zip(groups, records):
        for label, ms in rec.items():
            res[f"occupancy_train_bench iteration | {name} | all {modes} | {label}"] = statistics.median(ms)
    Path(out_path).write_text(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree", nargs="?")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, metavar=("TREE", "JSON"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.child[0]), args.child[1], args.rounds)
    sides = {"parent": (os.path.abspath(args.parent_tree), []), "this": (str(ROOT), [])}
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(args.runs):
            for side, (tree, runs) in sides.items():
                path = os.path.join(tmp, f"{side}_{k}.json")
                subprocess.run([sys.executable, __file__, "--child", tree, path, "--rounds", str(args.rounds)], check=True, timeout=600)
                runs.append(json.loads(Path(path).read_text()))
    lines, above = [f"{args.runs} processes per side, alternating; ms per iteration", ""], 0
    for key in sides["parent"][1][0]:
        p, t = ([r[key] for r in sides[s][1]] for s in ("parent", "this"))
        med = statistics.median(t)
        verdict = "inside" if min(p) <= med <= max(p) else "below" if med < min(p) else "ABOVE"
        above += verdict == "ABOVE"
        lines += [key, "    parent  " + "  ".join(f"{x:7.3f}" for x in p) + f"   min {min(p):7.3f}  median {statistics.median(p):7.3f}  max {max(p):7.3f}",
                  "    this    " + "  ".join(f"{x:7.3f}" for x in t) + f"   median {med:7.3f}  ({med / statistics.median(p):.4f} x the parent's median): {verdict}"]
    lines += ["", f"{above} entries above the parent's range"]
    print("\n".join(lines))
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 1 if above else 0


if __name__ == "__main__":
    sys.exit(main())
