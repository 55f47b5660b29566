#!/usr/bin/env python3
"""What the occupancy-guided sampler costs and where its samples go (TetraRenderer.render(occupancy_sampler=True);
csrc/tn_live_sampler.hip).

    python profiles/occupancy_sampler_bench.py [--parent-lib OLD.so] [--rounds 7] [--out profiles/occupancy_sampler_bench.txt]

One process, the candidates interleaved, medians over the rounds after a warm-up (device events around each call), as in
profiles/occupancy_bench.py, whose scene and helpers this file takes.
  ops     4096 outside-in rays of the C4-sized mesh (45,000 points), M = 512, S = 256: sample_live and live_to_distance (n = 256 /
          513) beside sample_coarse and find_visited_cells on the same rows, with the algorithmic bytes of the two new kernels
          (what they must read and write once) and the bandwidth those bytes imply; the bytes actually moved were not counted
  frame   the 800 x 800 frame of occupancy_bench.py (tetra-nerf-original, 256 + 256, 65,536-ray chunks) with its synthetic
          uniform occupancies at thresholds 0.5 / 0.9 (about 50 % / 10 % of the tetrahedra live): the uniform sampler + culling at
          S, the live sampler at S (more live samples: slower), the live sampler at S x (live fraction) (equal live-sample
          density), the live share of the final samples of each, and the share of find_visited_cells in the live frame.
          No quality figure: that needs a trained scene, and a synthetic occupancy says nothing about one.
  parent  (--parent-lib) the DEFAULT frame and the DEFAULT training iteration of this build against another build of the
          library (the parent commit's), in alternating child processes (TETRANERF_HIP_LIB).
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles"))
import occupancy_bench as ob  # noqa: E402
from occupancy_bench import fmt, interleaved  # noqa: E402
from train_x3_adjoint_bench import _NotExported  # noqa: E402
import train_x3_dw_bench as dwb  # noqa: E402

NEW = ("tn_sample_live", "tn_live_to_distance")
S_COARSE, S_FINE = ob.S_COARSE, ob.S_FINE


def ops_leg(torch, tn, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    cpp = tn.cpp
    pts, cells = scenes.random_mesh(45000, 2)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = scenes.outside_in_rays(4096, 1)
    M, S = 512, 256
    out = tr.trace_rays(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), M)
    lists = render.trace_rows(out)
    order, count = cpp.compact_hits(out["num_visited_cells"])
    r = int(count)
    order = order[:r].contiguous()
    occ = torch.rand(len(cells), generator=torch.Generator().manual_seed(1)).to(dev)
    rows = (lists[0], lists[1], lists[3], order)
    segs = int(out["num_visited_cells"].sum())
    say(f"the ops alone: {r} hitting rays of 4096 (C4-sized mesh, {len(cells)} tetrahedra), M = {M}, {segs} segments "
        f"({segs / max(r, 1):.1f} per ray), S = {S}, uniform occupancy, threshold 0.5:")
    edges, _ = cpp.sample_live(*rows, S, occ, 0.5)
    vals = {n: torch.sort(edges[:, :1] + torch.rand(r, n, device=dev) * (edges[:, -1:] - edges[:, :1]), dim=1).values.contiguous()
            for n in (256, 513)}
    dist = {n: cpp.live_to_distance(v, *rows, occ, 0.5)[0] for n, v in vals.items()}
    fns = {"sample_coarse (uniform)": lambda: cpp.sample_coarse(lists[0], lists[3], order, S),
           "sample_coarse (biased)": lambda: cpp.sample_coarse(lists[0], lists[3], order, S, biased=True),
           "sample_live": lambda: cpp.sample_live(*rows, S, occ, 0.5)}
    for n in (256, 513):
        fns[f"live_to_distance, n = {n}"] = lambda n=n: cpp.live_to_distance(vals[n], *rows, occ, 0.5)
        fns[f"find_visited_cells, n = {n}"] = lambda n=n: tr.find_visited_cells(*lists, dist[n], ray_index=order)
    res = interleaved(torch, fns, rounds, warm=2, reps=5)
    # what the two kernels must move once: per segment its two distances, its cell id and that cell's occupancy (a 4-byte gather);
    # per edge / value the output (and, for the map, the value read and the 8-byte row of the segment it landed in)
    per_seg = 8 + 4 + 4
    alg = {"sample_live": segs * per_seg + r * ((S + 1) * 4 + 8 + 8)}
    for n in (256, 513):
        alg[f"live_to_distance, n = {n}"] = segs * per_seg + r * (n * (4 + 8 + 4 + 4) + 8)
    for k, ms in res.items():
        note = ""
        if k in alg:
            note = f"   algorithmic {alg[k] / 1e6:.2f} MB -> {alg[k] / statistics.median(ms) / 1e6:.1f} GB/s"
        say(f"    {k:32s} {fmt(ms)}{note}")
    say("    (algorithmic bytes: each segment's distances, cell id and occupancy once, each output once; the bytes the kernels actually "
        "moved were not measured with counters)")


def _matcher_share(torch, tr, frame):
    """(ms inside find_visited_cells, ms of the frame) of one frame, by device events around every matcher call"""
    real = tr.find_visited_cells
    spans = []

    def spy(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = real(*a, **k)
        e1.record()
        spans.append((e0, e1))
        return res

    tr.find_visited_cells = spy
    try:
        total = ob.timed(torch, frame)
    finally:
        del tr.find_visited_cells
    return sum(a.elapsed_time(b) for a, b in spans), total


def frame_leg(torch, tn, dev, rounds, say):
    render, tr, field, mlp, o, d, cells = ob.frame_setup(torch, tn, dev)
    R, chunk, T = o.shape[0], 65536, cells.shape[0]
    occ = torch.rand(T, generator=torch.Generator().manual_seed(1)).to(dev)

    def frame_of(rd, **kw):
        return lambda: torch.cat([rd.render(o[s:s + chunk], d[s:s + chunk], **kw)["rgb"] for s in range(0, R, chunk)])

    say(f"800 x 800 frame, tetra-nerf-original ({S_COARSE} + {S_FINE}), 15,000-point mesh ({T} tetrahedra), 65,536-ray chunks (trace + "
        "TetraRenderer.render), synthetic uniform occupancy:")
    for mode in ob.MODES:
        def renderer(s_c, s_f):
            return render.TetraRenderer(tr, field, mlp, s_c, 512, fused=True, num_fine_samples=s_f, mlp_mode=mode, fused_pass=False)

        full = renderer(S_COARSE, S_FINE)
        say(f"  {mode}:")
        for thr, frac in ((0.5, 0.5), (0.9, 0.1)):
            small = renderer(max(1, round(S_COARSE * frac)), max(1, round(S_FINE * frac)))
            kw = dict(occupancy=occ, occupancy_threshold=thr)
            fns = {"chain, no occupancy (for scale)": frame_of(full),
                   f"uniform sampler + culling, S = {full.S} + {full.S_fine}": frame_of(full, **kw),
                   f"live sampler, S = {full.S} + {full.S_fine}": frame_of(full, occupancy_sampler=True, **kw),
                   f"live sampler, S = {small.S} + {small.S_fine} (S x live fraction)": frame_of(small, occupancy_sampler=True, **kw)}
            res = interleaved(torch, fns, rounds)
            ref = statistics.median(res[f"uniform sampler + culling, S = {full.S} + {full.S_fine}"])
            say(f"    threshold {thr} (about {frac:.0%} of the tetrahedra live):")
            for (k, ms), fn in zip(res.items(), fns.values()):
                note = ""
                if "no occupancy" not in k:
                    ran, total, matched, live_matched = ob.live_fraction(torch, tn, fn)
                    note = f"   network on {ran} of {total} samples ({ran / max(total, 1):.3f}), both passes"
                say(f"      {k:52s} {fmt(ms)}   {statistics.median(ms) / ref:.3f} x uniform + culling{note}")
            inside, total = _matcher_share(torch, tr, fns[f"live sampler, S = {full.S} + {full.S_fine}"])
            say(f"      find_visited_cells in the live-sampler frame at S = {full.S} + {full.S_fine}: {inside:.2f} of {total:.2f} ms ({inside / total:.3f}) -- "
                "what emitting the matcher's outputs from `slot` could save at most")
    say("  (no quality figure: the occupancy is synthetic; what the resolution buys needs a trained scene)")


class _OlderLibrary(ctypes.CDLL):
    """The parent commit's library lacks the two entries of NEW, which this build's binding declares (and calls with
    occupancy_sampler=True only).  Those names resolve to _NotExported."""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name not in NEW:
                raise
            fn = _NotExported(name)
            setattr(self, name, fn)
            return fn


def child(rounds):
    """the default frame and the default training iteration (no keyword at all) of whatever library TETRANERF_HIP_LIB names"""
    import faulthandler

    import torch

    faulthandler.enable()
    tn = importlib.import_module("tetra-nerf_amd")
    binding = importlib.import_module("tetra-nerf_amd._lib")
    binding.C = types.SimpleNamespace(**{**vars(ctypes), "CDLL": _OlderLibrary})
    dev = torch.device("cuda:0")
    render, tr, field, mlp, o, d, _ = ob.frame_setup(torch, tn, dev)
    rd = render.TetraRenderer(tr, field, mlp, S_COARSE, 512, fused=True, num_fine_samples=S_FINE)
    R, chunk = o.shape[0], 65536
    fns = {"frame 800x800 (256 + 256)": lambda: [rd.render(o[s:s + chunk], d[s:s + chunk])["rgb"] for s in range(0, R, chunk)]}
    out = {k: statistics.median(v) for k, v in interleaved(torch, fns, rounds).items()}
    res = interleaved(torch, dwb.iteration_fns(torch, tn, dev, [None]), rounds, reps=5)
    out.update({f"training iteration, {name}": statistics.median(ms) for (name, _), ms in res.items()})
    print("CHILD " + json.dumps(out), flush=True)


def parent_leg(parent_lib, rounds, say, alternations=5):
    libs = {"this build": str(ROOT / "tetra-nerf_amd" / "libtetranerf_hip.so"), "parent": str(Path(parent_lib).resolve())}
    got = {k: {} for k in libs}
    for _ in range(alternations):
        for k, path in libs.items():
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rounds", str(rounds)],
                               env=dict(os.environ, TETRANERF_HIP_LIB=path), capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"child process on {path} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1]
            for name, ms in json.loads(line[6:]).items():
                got[k].setdefault(name, []).append(ms)
    say(f"the default paths (no occupancy, fp32), this build against the parent commit's library, {alternations} alternating processes "
        f"each (per process: median of {rounds} rounds):")
    for name in got["parent"]:
        for k in libs:
            say(f"    {name:42s} {k:10s} " + " ".join(f"{x:8.3f}" for x in got[k][name]) + f"   median {statistics.median(got[k][name]):8.3f} ms")
        med = statistics.median(got["parent"][name])
        say(f"    {name:42s} this build / parent = {statistics.median(got['this build'][name]) / med:.4f}; the parent's own processes span "
            f"{min(got['parent'][name]) / med:.4f} .. {max(got['parent'][name]) / med:.4f} of their median")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_sampler_bench.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="ops,frame,parent")
    ap.add_argument("--alternations", type=int, default=5, help="child processes per build of the parent leg")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("medians over at least 7 rounds")
    if args.child:
        return child(args.rounds)
    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    tn = importlib.import_module("tetra-nerf_amd")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    say(f"{torch.cuda.get_device_name(0)} | {lib.tn_version().decode()} | torch {torch.__version__}")
    legs = args.legs.split(",")
    if "ops" in legs:
        ops_leg(torch, tn, dev, args.rounds, say)
    if "frame" in legs:
        frame_leg(torch, tn, dev, args.rounds, say)
    if args.parent_lib and "parent" in legs:
        torch.cuda.synchronize()
        parent_leg(args.parent_lib, args.rounds, say, args.alternations)


if __name__ == "__main__":
    main()
