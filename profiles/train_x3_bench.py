#!/usr/bin/env python3
"""What the bf16x3 training forward buys (tn_mlp_forward_gather_train_ex mode 1; TetraRenderer(train_mlp_mode="bf16x3")).

    python profiles/train_x3_bench.py [--parent-lib OLD.so] [--rounds 7] [--out profiles/train_x3_bench.txt]

One process, the two modes interleaved, medians over the rounds after a warm-up (device events around `reps` calls per round):
  1. mlp_forward_gather_train, fp32 against bf16x3, at n = 4096 x 513 and 4096 x 257 samples (the fine passes of the two shipped
     configurations), V = 45,000 vertices, random sample placement;
  2. one whole training iteration -- trace_rays + render_train + loss.backward() + SGD step, as bench.py's train leg -- in both
     modes, for `tetra-nerf-original` (256 + 256) and `tetra-nerf` (128 + 128, biased, gradient scaling), 4096 outside-in rays
     of the C4-sized mesh (45,000 points, seed 2).
--parent-lib: 3. the fp32 iteration of THIS build against another build of the library (the parent commit's), in alternating
child processes (TETRANERF_HIP_LIB), to show that the default path did not move.
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
CONFIGS = (("tetra-nerf-original", (256, 256, False, False)), ("tetra-nerf", (128, 128, True, True)))


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(torch, fns, rounds, reps, warm=3):
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
    return f"median {statistics.median(ms):7.3f} ms  (min {min(ms):7.3f}, max {max(ms):7.3f}, {len(ms)} rounds)"


def forward_leg(torch, tn, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    V, R = 45000, 4096
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(dev)
    w = [x.detach() for x in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=dev) * 0.7
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1)
    for S in (513, 257):
        n = R * S
        vi = torch.randint(0, V, (n, 4), dtype=torch.int32, device=dev)
        bc = (torch.rand(n, 3, device=dev) / 3).contiguous()
        fns = {m: (lambda m=m: tn.cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, mode=m)) for m in ("fp32", "bf16x3")}
        fns["bf16x3, nothing saved"] = lambda: tn.cpp.mlp_forward_gather(vi, bc, field, dirs, w, S, mode="bf16x3")
        res = interleaved(torch, fns, rounds, reps=5)
        say(f"mlp_forward_gather_train, n = {R} x {S} = {n} samples (saves {n * 2368 / 1e9:.2f} GB):")
        for k, ms in res.items():
            say(f"    {k:24s} {fmt(ms)}")
        a, b = statistics.median(res["fp32"]), statistics.median(res["bf16x3"])
        say(f"    bf16x3 / fp32 = {b / a:.3f}  (fp32 / bf16x3 = {a / b:.2f}x); the saves alone at the time of the bf16x3 call: "
            f"{n * 2368 / (b * 1e-3) / 1e9:.0f} GB/s")


def iteration_fns(torch, tn, dev, modes):
    """{(config, mode): step} on the C4-sized mesh, bench.py's train leg"""
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    pts, cells = scenes.random_mesh(45000, 2)
    tracer = tn.TetrahedraTracer(dev)
    tracer.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = scenes.outside_in_rays(4096, 1)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    target = torch.rand(len(o), 3, device=dev)
    fns = {}
    for name, (s_c, s_f, biased, scaling) in CONFIGS:
        torch.manual_seed(0)
        mlp = render.TetraMLP().to(dev)
        field = ((torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4)
        field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
        field.requires_grad_(True)
        opt = torch.optim.SGD([field] + list(mlp.parameters()), lr=1e-3)
        rd = render.TetraRenderer(tracer, field, mlp, s_c, 512, fused=True, num_fine_samples=s_f, biased=biased)
        for mode in modes:
            def step(rd=rd, opt=opt, scaling=scaling, kw=({} if mode is None else {"mlp_mode": mode})):
                opt.zero_grad(set_to_none=True)
                out = rd.render_train(o, d, gradient_scaling=scaling, **kw)
                ((out["rgb"] - target) ** 2).mean().backward()
                opt.step()
            fns[(name, mode)] = step
    return fns


def iteration_leg(torch, tn, dev, rounds, say):
    res = interleaved(torch, iteration_fns(torch, tn, dev, ("fp32", "bf16x3")), rounds, reps=5)
    for name, _ in CONFIGS:
        say(f"training iteration, {name}, 4096 rays, C4-sized mesh (trace + render_train + backward + SGD step):")
        for mode in ("fp32", "bf16x3"):
            say(f"    forward in {mode:7s} {fmt(res[(name, mode)])}")
        a, b = statistics.median(res[(name, "fp32")]), statistics.median(res[(name, "bf16x3")])
        say(f"    bf16x3 / fp32 = {b / a:.3f}  ({(1 - b / a) * 100:.1f} % of an iteration saved)")


def tolerate_older_library():
    """The parent commit's library has no tn_mlp_forward_gather_train_ex, which this build's binding declares (and calls for
    bf16x3 only: the default iteration goes through tn_mlp_forward_gather_train in both builds).  Give such a library's handle
    an attribute of that name so that the binding loads; it is never called here."""
    import ctypes

    new, real = "tn_mlp_forward_gather_train_ex", ctypes.CDLL

    def cdll(path, *a, **kw):
        lib = real(path, *a, **kw)
        if "tetranerf_hip" in str(path) and not hasattr(lib, new):
            setattr(lib, new, lib._FuncPtr(("tn_mlp_forward_gather_train", lib)))
        return lib

    ctypes.CDLL = cdll


def child(rounds):
    """the default (fp32) iteration of whatever library TETRANERF_HIP_LIB names: one JSON line"""
    import faulthandler

    import torch

    faulthandler.enable()
    tolerate_older_library()
    tn = importlib.import_module("tetra-nerf_amd")
    dev = torch.device("cuda:0")
    res = interleaved(torch, iteration_fns(torch, tn, dev, (None,)), rounds, reps=5)
    print("CHILD " + json.dumps({name: statistics.median(ms) for (name, _), ms in res.items()}), flush=True)


def parent_leg(parent_lib, rounds, say, alternations=3):
    libs = {"this build": str(ROOT / "tetra-nerf_amd" / "libtetranerf_hip.so"), "parent": str(Path(parent_lib).resolve())}
    got = {k: {name: [] for name, _ in CONFIGS} for k in libs}
    for _ in range(alternations):
        for k, path in libs.items():
            env = dict(os.environ, TETRANERF_HIP_LIB=path)
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rounds", str(rounds)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"child process on {path} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1]
            for name, ms in json.loads(line[6:]).items():
                got[k][name].append(ms)
    say(f"default (fp32) training iteration, this build against the parent commit's library, {alternations} alternating processes each "
        f"(per process: median of {rounds} rounds):")
    for name, _ in CONFIGS:
        for k in libs:
            say(f"    {name:20s} {k:10s} " + " ".join(f"{x:7.3f}" for x in got[k][name]) + f"   median {statistics.median(got[k][name]):7.3f} ms")
        say(f"    {name:20s} this build / parent = {statistics.median(got['this build'][name]) / statistics.median(got['parent'][name]):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_x3_bench.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("medians over at least 5 rounds")
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

    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    say(f"{torch.cuda.get_device_name(0)} | {lib.tn_version().decode()} | torch {torch.__version__}")
    forward_leg(torch, tn, dev, args.rounds, say)
    iteration_leg(torch, tn, dev, args.rounds, say)
    if args.parent_lib:
        torch.cuda.synchronize()
        parent_leg(args.parent_lib, args.rounds, say)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
