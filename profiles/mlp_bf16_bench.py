#!/usr/bin/env python3
"""What the plain-bf16 evaluation arithmetic buys (tn_mlp_forward_gather mode 2; TetraRenderer(mlp_mode="bf16")) and what it costs.

    python profiles/mlp_bf16_bench.py [--parent-lib OLD.so] [--staged-lib STAGED.so] [--rounds 7] [--out profiles/mlp_bf16_bench.txt]

One process, the modes interleaved as fp32, bf16x3, bf16, medians over the rounds after a warm-up (device events around `reps`
calls per round):
  1. mlp_forward_gather, full and density only, at n = 4096 x 513 and 65,536 x 256 samples, V = 45,000 vertices, random sample
     placement; with --staged-lib also the bf16 kernel with per-layer staging instead of the resident network, a variant library
     (make -C tetra-nerf_amd/csrc BUILD=build_staged OUT=../variants/libtetranerf_hip_staged.so EXTRA=-DTN_BF16_STAGED=1) in a
     child process of its own;
  2. the 800 x 800 frame of bench.py (15,000-point mesh seed 0, 65,536-ray chunks) through TetraRenderer.render in the three modes,
     for `tetra-nerf-original` (256 + 256) and `tetra-nerf` (128 + 128, biased); for bf16 also max / mean |d rgb| and the PSNR
     against the fp32 frame;
  3. the tolerance of tests/test_mlp_bf16_gpu.py::test_render_in_bf16, measured on the reference side (no kernel under test):
     render_reference with the PyTorch rounding statement against render_reference with the plain TetraMLP on that test's scene.
--parent-lib: 4. the fp32 and bf16x3 frames of THIS build against another build of the library (the parent commit's), in
alternating child processes (TETRANERF_HIP_LIB), three each, to show that the existing modes did not move.
Needs a GPU; there is no fallback."""
import argparse
import importlib
import json
import math
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
CONFIGS = (("tetra-nerf-original", (256, 256, False)), ("tetra-nerf", (128, 128, True)))
MODES = ("fp32", "bf16x3", "bf16")
SHAPES = ((4096, 513), (65536, 256))


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(torch, fns, rounds, reps, warm=2):
    """{name: [ms per call, one figure per round]}: every round times each candidate once, in turn"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(torch, fn, reps))
    return out


def fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):8.3f}, max {max(ms):8.3f}, {len(ms)} rounds)"


def forward_fns(torch, tn, dev, R, S, modes):
    render = importlib.import_module("tetra-nerf_amd.render")
    V = 45000
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(dev)
    w = [x.detach() for x in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=dev) * 0.7
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1)
    n = R * S
    vi = torch.randint(0, V, (n, 4), dtype=torch.int32, device=dev)
    bc = (torch.rand(n, 3, device=dev) / 3).contiguous()
    fns = {}
    for m in modes:
        fns[("full", m)] = lambda m=m: tn.cpp.mlp_forward_gather(vi, bc, field, dirs, w, S, mode=m)
        fns[("density only", m)] = lambda m=m: tn.cpp.mlp_forward_gather(vi, bc, field, None, w, S, mode=m)
    return fns


def forward_leg(torch, tn, dev, rounds, say, staged_lib=None):
    staged = None
    if staged_lib:
        p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "staged", "--rounds", str(rounds)],
                           env=dict(os.environ, TETRANERF_HIP_LIB=str(Path(staged_lib).resolve())), capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"staged child failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
        staged = json.loads([l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
    for R, S in SHAPES:
        res = interleaved(torch, forward_fns(torch, tn, dev, R, S, MODES), rounds, reps=5)
        say(f"mlp_forward_gather, n = {R} x {S} = {R * S} samples:")
        for form in ("full", "density only"):
            for m in MODES:
                say(f"    {form:13s} {m:7s} {fmt(res[(form, m)])}")
            a, b, c = (statistics.median(res[(form, m)]) for m in MODES)
            line = f"    {form:13s} fp32 / bf16 = {a / c:.2f}x   bf16x3 / bf16 = {b / c:.2f}x"
            if staged:
                st = staged[f"{R}x{S} {form}"]
                say(f"    {form:13s} bf16, per-layer staging (variant library, own process) {fmt(st)}")
                line += f"   staged / resident = {statistics.median(st) / c:.2f}x"
            say(line)


def frame_setup(torch, tn, dev):
    import numpy as np

    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    pts, cells = scenes.random_mesh(15000, 0)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    c = np.array([0.5, 0.5, 0.5], np.float32)
    eye = c + 2.0 * np.array([0.0, 1.0, 0.0], np.float32)
    o, d = scenes.pinhole_rays(800, 800, eye=tuple(eye), lookat=tuple(c), up=(0.0, 0.0, 1.0), fov_y=45.0)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    field = (torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4
    field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
    return render, tr, field, mlp, o, d


def frame_fns(torch, tn, dev, modes):
    """{(config, mode): callable rendering the frame in 65,536-ray chunks and returning its rgb}"""
    render, tr, field, mlp, o, d = frame_setup(torch, tn, dev)
    R, chunk = o.shape[0], 65536
    fns = {}
    for name, (s_c, s_f, biased) in CONFIGS:
        for mode in modes:
            rd = render.TetraRenderer(tr, field, mlp, s_c, 512, fused=True, num_fine_samples=s_f, biased=biased, mlp_mode=mode)
            fns[(name, mode)] = lambda rd=rd: torch.cat([rd.render(o[s:s + chunk], d[s:s + chunk])["rgb"] for s in range(0, R, chunk)])
    return fns


def frame_leg(torch, tn, dev, rounds, say):
    fns = frame_fns(torch, tn, dev, MODES)
    res = interleaved(torch, fns, rounds, reps=1, warm=1)
    for name, _ in CONFIGS:
        say(f"800 x 800 frame, {name}, 15,000-point mesh, 65,536-ray chunks (trace + TetraRenderer.render):")
        for m in MODES:
            say(f"    {m:7s} {fmt(res[(name, m)])}")
        a, b, c = (statistics.median(res[(name, m)]) for m in MODES)
        spread = max(max(res[(name, m)]) - min(res[(name, m)]) for m in ("bf16x3", "bf16"))
        say(f"    fp32 / bf16 = {a / c:.2f}x   bf16x3 / bf16 = {b / c:.2f}x   (bf16x3 - bf16 = {b - c:.2f} ms; widest min-max spread of the two: {spread:.2f} ms)")
        want, got = fns[(name, "fp32")](), fns[(name, "bf16")]()
        diff = (got - want).abs()
        mse = float(((got - want).double() ** 2).mean())
        say(f"    bf16 frame against the fp32 frame: max |d rgb| {float(diff.max()):.3e}, mean |d rgb| {float(diff.mean()):.4e}, "
            f"PSNR {10 * math.log10(1.0 / mse):.2f} dB")


def tolerance_leg(torch, tn, dev, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    pts, cells = scenes.random_mesh(5000, 9)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    torch.manual_seed(2)
    mlp = render.TetraMLP().to(dev)
    field = torch.randn(64, len(pts), device=dev) * 0.5
    o, d = scenes.outside_in_rays(3000, 4)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with torch.no_grad():
        a = render.render_reference(tr, tn.cpp.interpolate_values, field, mlp, o, d, 64, 256, num_fine_samples=64)
        b = render.render_reference(tr, tn.cpp.interpolate_values, field, render.Bf16StatementMLP(mlp), o, d, 64, 256, num_fine_samples=64)
    dev_rgb = float((b["rgb"] - a["rgb"]).abs().max())
    dev_acc = float((b["accumulation"] - a["accumulation"]).abs().max())
    say("scene of tests/test_mlp_bf16_gpu.py::test_render_in_bf16 (5000-point mesh, 3000 rays, 64 + 64 samples), reference side only --")
    say(f"    render_reference with the bf16 rounding statement against render_reference with the plain TetraMLP: max |d rgb| {dev_rgb:.3e}, "
        f"max |d accumulation| {dev_acc:.3e}  (the test's tolerances: twice these)")
    got = render.TetraRenderer(tr, field, mlp, 64, 256, fused=True, num_fine_samples=64, mlp_mode="bf16").render(o, d)
    want = render.TetraRenderer(tr, field, mlp, 64, 256, fused=True, num_fine_samples=64).render(o, d)
    say(f"    the kernels on the same scene, bf16 against fp32: max |d rgb| {float((got['rgb'] - want['rgb']).abs().max()):.3e}, "
        f"max |d accumulation| {float((got['accumulation'] - want['accumulation']).abs().max()):.3e}")


def child(kind, rounds):
    import faulthandler

    import torch

    faulthandler.enable()
    tn = importlib.import_module("tetra-nerf_amd")
    dev = torch.device("cuda:0")
    if kind == "staged":      # the bf16 forward kernels of whatever library TETRANERF_HIP_LIB names
        out = {}
        for R, S in SHAPES:
            res = interleaved(torch, forward_fns(torch, tn, dev, R, S, ("bf16",)), rounds, reps=5)
            for (form, _), ms in res.items():
                out[f"{R}x{S} {form}"] = ms
    else:                     # the fp32 and bf16x3 frames of whatever library TETRANERF_HIP_LIB names
        res = interleaved(torch, frame_fns(torch, tn, dev, ("fp32", "bf16x3")), rounds, reps=1, warm=1)
        out = {f"{name} {mode}": statistics.median(ms) for (name, mode), ms in res.items()}
    print("CHILD " + json.dumps(out), flush=True)


def parent_leg(parent_lib, rounds, say, alternations=3):
    libs = {"this build": str(ROOT / "tetra-nerf_amd" / "libtetranerf_hip.so"), "parent": str(Path(parent_lib).resolve())}
    got = {k: {} for k in libs}
    for _ in range(alternations):
        for k, path in libs.items():
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "frames", "--rounds", str(rounds)],
                               env=dict(os.environ, TETRANERF_HIP_LIB=path), capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"child process on {path} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
            for name, ms in json.loads([l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1][6:]).items():
                got[k].setdefault(name, []).append(ms)
    say(f"fp32 and bf16x3 frames, this build against the parent commit's library, {alternations} alternating processes each "
        f"(per process: median of {rounds} rounds):")
    for name in got["parent"]:
        for k in libs:
            say(f"    {name:28s} {k:10s} " + " ".join(f"{x:8.3f}" for x in got[k][name]) + f"   median {statistics.median(got[k][name]):8.3f} ms")
        pa = got["parent"][name]
        say(f"    {name:28s} this build / parent = {statistics.median(got['this build'][name]) / statistics.median(pa):.4f}"
            f"   (the parent's own three runs: max / min = {max(pa) / min(pa):.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--staged-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mlp_bf16_bench.txt"))
    ap.add_argument("--child", choices=("staged", "frames"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("medians over at least 5 rounds")
    if args.child:
        return child(args.child, args.rounds)
    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    tn = importlib.import_module("tetra-nerf_amd")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    say(f"{torch.cuda.get_device_name(0)} | {lib.tn_version().decode()} | torch {torch.__version__}")
    forward_leg(torch, tn, dev, args.rounds, say, args.staged_lib)
    frame_leg(torch, tn, dev, args.rounds, say)
    tolerance_leg(torch, tn, dev, say)
    if args.parent_lib:
        torch.cuda.synchronize()
        parent_leg(args.parent_lib, args.rounds, say)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
