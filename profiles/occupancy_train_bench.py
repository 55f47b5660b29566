#!/usr/bin/env python3
"""What occupancy-culled training costs and buys (TetraRenderer.render_train(occupancy=, occupancy_threshold=);
csrc/tn_occupancy_train.hip, csrc/tn_occupancy_dw.hip).

    python profiles/occupancy_train_bench.py [--parent-lib OLD.so] [--rounds 7] [--out profiles/occupancy_train_bench.txt]

One process, the candidates interleaved, medians over the rounds after a warm-up (device events around `reps` calls per round; the
helpers are profiles/train_x3_bench.py's and profiles/train_x3_dw_bench.py's):
  (a) one whole training iteration -- trace_rays + render_train + loss.backward() + SGD step, as bench.py's train leg -- of
      `tetra-nerf-original` (256 + 256) and `tetra-nerf` (128 + 128, biased, gradient scaling), 4096 outside-in rays of the C4-sized
      mesh (45,000 points, seed 2): without an occupancy (the reference); with a threshold that culls nothing (the cost of
      cull_samples + the read-back of the live count + the row compaction); and with SYNTHETIC occupancies (uniform random per
      tetrahedron) at the thresholds 0.5 / 0.9, which leave about 50 % / 10 % of the matched samples live (the fraction reached
      is reported).  Each with all three arithmetic switches fp32 and with all three bf16x3.  A culled iteration contains one
      host synchronisation (the read-back), which the device events include.  What a trained scene gains depends on its empty
      share; nothing is claimed for one.
  (b) the kernels alone at 4096 x 513 samples, listed all / half / a tenth, next to their unindexed entries on all samples: the
      saving forward, the dX chain (the unchanged entry on n_live compact columns, with the six row compactions it needs) and
      param_grads.
--parent-lib: (c) the default iteration (no occupancy, fp32) of THIS build against another build of the library (the parent
commit's), in alternating child processes (TETRANERF_HIP_LIB), and (d) profiles/compare_device_code.py PARENT.so THIS.so.
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
from train_x3_bench import CONFIGS, fmt, interleaved  # noqa: E402
from train_x3_adjoint_bench import _NotExported, device_code_leg  # noqa: E402
import train_x3_dw_bench as dwb  # noqa: E402

NEW = ("tn_mlp_forward_gather_train_indexed", "tn_mlp_param_grads_indexed", "tn_mlp_ray_head_grad_indexed", "tn_compact_rows")
CASES = (("no occupancy (the reference)", None), ("threshold 0 (culls nothing)", 0.0), ("uniform occupancy, threshold 0.5", 0.5),
         ("uniform occupancy, threshold 0.9", 0.9))


def iteration_leg(torch, tn, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    pts, cells = scenes.random_mesh(45000, 2)
    tracer = tn.TetrahedraTracer(dev)
    tracer.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = scenes.outside_in_rays(4096, 1)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    target = torch.rand(len(o), 3, device=dev)
    occ = torch.rand(len(cells), generator=torch.Generator().manual_seed(1)).to(dev)
    for name, (s_c, s_f, biased, scaling) in CONFIGS:
        for modes in ("fp32", "bf16x3"):
            torch.manual_seed(0)
            mlp = render.TetraMLP().to(dev)
            field = ((torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4)
            field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
            field.requires_grad_(True)
            opt = torch.optim.SGD([field] + list(mlp.parameters()), lr=1e-3)
            rd = render.TetraRenderer(tracer, field, mlp, s_c, 512, fused=True, num_fine_samples=s_f, biased=biased,
                                      train_mlp_mode=modes, train_adjoint_mode=modes, train_dw_mode=modes)

            def step(thr=None):
                kw = {} if thr is None else dict(occupancy=occ, occupancy_threshold=thr)
                opt.zero_grad(set_to_none=True)
                out = rd.render_train(o, d, gradient_scaling=scaling, **kw)
                ((out["rgb"] - target) ** 2).mean().backward()
                opt.step()

            res = interleaved(torch, {label: (lambda thr=thr: step(thr)) for label, thr in CASES}, rounds, reps=5)
            ref = statistics.median(res[CASES[0][0]])
            say(f"training iteration, {name}, 4096 rays, C4-sized mesh ({len(cells)} tetrahedra), forward / dX / dW all {modes} "
                "(trace + render_train + backward + SGD step):")
            for label, thr in CASES:
                note = ""
                if thr:
                    seen = []
                    real = tn.cpp.cull_samples
                    tn.cpp.cull_samples = lambda *a, **k: (lambda r: (seen.append((int(r[1]), a[0].numel())), r)[1])(real(*a, **k))
                    try:
                        step(thr)
                    finally:
                        tn.cpp.cull_samples = real
                    note = "   live: " + ", ".join(f"{a} of {b} ({a / b:.3f})" for a, b in seen) + " (coarse, fine pass)"
                say(f"    {label:36s} {fmt(res[label])}   {statistics.median(res[label]) / ref:.3f} x the reference{note}")


def kernel_leg(torch, tn, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    cpp = tn.cpp
    lib = cpp._lib.load()
    R, S, V = 4096, 513, 45000
    n = R * S
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(dev)
    w = [x.detach() for x in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=dev) * 0.7
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1).contiguous()
    vi = torch.randint(0, V, (n, 4), dtype=torch.int32, device=dev)
    bc = (torch.rand(n, 3, device=dev) / 3).contiguous()
    d_sigma = (torch.randn(n, device=dev) * 1e-3).contiguous()
    d_rgb = (torch.randn(n, 3, device=dev) * 1e-3).contiguous()
    mh = cpp.fused_mlp(w)
    stream = cpp._stream(dev)
    say(f"the kernels alone, n = {R} x {S} = {n} samples, V = {V} (unindexed entries on all samples against the indexed ones on lists):")
    for mode, m in (("fp32", 0), ("bf16x3", 1)):
        fwd, dx, dw = {}, {}, {}
        keep = []
        for label, frac in (("all samples, unindexed entries", None), ("listed 1.000", 1.0), ("listed 0.500", 0.5), ("listed 0.100", 0.1)):
            if frac is None:
                k, live = n, None
                sigma, rgb, saved = cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, mode=mode)
                fwd[label] = lambda: cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, mode=mode)
            else:
                k = int(n * frac)
                live = torch.sort(torch.randperm(n, device=dev)[:k]).values.to(torch.int32).contiguous()
                sigma, rgb = torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev)
                _, _, saved = cpp.mlp_forward_gather_train_indexed(live, k, vi, bc, field, dirs, w, S, mode=mode, sigma=sigma, rgb=rgb)
                fwd[label] = (lambda live=live, k=k, sigma=sigma, rgb=rgb: cpp.mlp_forward_gather_train_indexed(
                    live, k, vi, bc, field, dirs, w, S, mode=mode, sigma=sigma, rgb=rgb))
            a = saved.acts
            buf = torch.empty((4 * 128 + 4, k), dtype=torch.float32, device=dev)
            rows = torch.empty((k, 64), dtype=torch.float32, device=dev)
            bs = cpp._MlpBackwardBuffers(a[0:64].data_ptr(), a[64:192].data_ptr(), a[192:320].data_ptr(), a[320:448].data_ptr(),
                                         a[448:576].data_ptr(), saved.masks.data_ptr(), buf[0:128].data_ptr(), buf[128:256].data_ptr(),
                                         buf[256:384].data_ptr(), buf[384:512].data_ptr(), buf[512:516].data_ptr(), rows.data_ptr())
            grads = [torch.zeros(shp, dtype=torch.float32, device=dev) for shp in cpp._WEIGHT_SHAPES]
            gs = cpp._MlpWeightsStruct(*[g.data_ptr() for g in grads])
            keep.append((saved, buf, rows, bs, grads, gs, live, sigma, rgb))

            def chain(k=k, live=live, sigma=sigma, rgb=rgb, bs=bs):
                s, c, ds, dc = sigma, rgb, d_sigma, d_rgb
                if live is not None:      # what cpp.mlp_backward compacts for the unchanged per-sample kernels
                    cpp.compact_rows(vi, live, k), cpp.compact_rows(bc, live, k)
                    s, c, ds, dc = (cpp.compact_rows(x, live, k) for x in (sigma, rgb, d_sigma, d_rgb))
                cpp._lib.check(lib.tn_mlp_backward_ex(mh.handle, k, s.data_ptr(), c.data_ptr(), ds.data_ptr(), dc.data_ptr(),
                                                      ctypes.byref(bs), m, stream))

            chain()
            dx[label] = chain
            if live is None:
                dw[label] = lambda bs=bs, gs=gs: cpp._lib.check(lib.tn_mlp_param_grads_ex(mh.handle, n, S, dirs.data_ptr(), ctypes.byref(bs),
                                                                                         ctypes.byref(gs), m, stream))
            else:
                dw[label] = lambda bs=bs, gs=gs, k=k, live=live: cpp._lib.check(lib.tn_mlp_param_grads_indexed(
                    mh.handle, k, n, S, live.data_ptr(), dirs.data_ptr(), ctypes.byref(bs), ctypes.byref(gs), m, stream))
        for what, fns in (("saving forward", fwd), ("dX chain (+ six row compactions when listed)", dx), ("param_grads", dw)):
            res = interleaved(torch, fns, rounds, reps=3)
            ref = statistics.median(next(iter(res.values())))
            say(f"  {mode}, {what}:")
            for label, ms in res.items():
                say(f"    {label:36s} {fmt(ms)}   {statistics.median(ms) / ref:.3f} x")
        del keep, fwd, dx, dw
        torch.cuda.empty_cache()


class _OlderLibrary(ctypes.CDLL):
    """The parent commit's library lacks the four entries of NEW, which this build's binding declares (and calls for culled
    batches only).  Those names resolve to _NotExported."""

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
    """the default iteration (no keyword at all) of whatever library TETRANERF_HIP_LIB names: one JSON line"""
    import faulthandler

    import torch

    faulthandler.enable()
    # only the binding's own load call sees the tolerant loader: its `C` becomes a copy of the ctypes namespace with that one
    # name replaced (ctypes itself, and whoever else constructs a CDLL in this process, are untouched)
    tn = importlib.import_module("tetra-nerf_amd")
    binding = importlib.import_module("tetra-nerf_amd._lib")
    binding.C = types.SimpleNamespace(**{**vars(ctypes), "CDLL": _OlderLibrary})
    dev = torch.device("cuda:0")
    res = interleaved(torch, dwb.iteration_fns(torch, tn, dev, [None]), rounds, reps=5)
    print("CHILD " + json.dumps({name: statistics.median(ms) for (name, _), ms in res.items()}), flush=True)


def parent_leg(parent_lib, rounds, say, alternations=3):
    """profiles/train_x3_dw_bench.py's, with this file's child (the parent lacks this build's new entries)"""
    libs = {"this build": str(ROOT / "tetra-nerf_amd" / "libtetranerf_hip.so"), "parent": str(Path(parent_lib).resolve())}
    got = {k: {name: [] for name, _ in CONFIGS} for k in libs}
    for _ in range(alternations):
        for k, path in libs.items():
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rounds", str(rounds)],
                               env=dict(os.environ, TETRANERF_HIP_LIB=path), capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"child process on {path} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1]
            for name, ms in json.loads(line[6:]).items():
                got[k][name].append(ms)
    say(f"default training iteration (no occupancy, fp32), this build against the parent commit's library, {alternations} alternating "
        f"processes each (per process: median of {rounds} rounds):")
    for name, _ in CONFIGS:
        for k in libs:
            say(f"    {name:20s} {k:10s} " + " ".join(f"{x:7.3f}" for x in got[k][name]) + f"   median {statistics.median(got[k][name]):7.3f} ms")
        med = statistics.median(got["parent"][name])
        say(f"    {name:20s} this build / parent = {statistics.median(got['this build'][name]) / med:.4f}; the parent's own processes span "
            f"{min(got['parent'][name]) / med:.4f} .. {max(got['parent'][name]) / med:.4f} of their median")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_train_bench.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="iteration,kernels,parent")
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
        Path(args.out).write_text("\n".join(lines) + "\n")

    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    say(f"{torch.cuda.get_device_name(0)} | {lib.tn_version().decode()} | torch {torch.__version__}")
    legs = args.legs.split(",")
    if "iteration" in legs:
        iteration_leg(torch, tn, dev, args.rounds, say)
    if "kernels" in legs:
        kernel_leg(torch, tn, dev, args.rounds, say)
    if args.parent_lib and "parent" in legs:
        torch.cuda.synchronize()
        parent_leg(args.parent_lib, args.rounds, say)
        device_code_leg(args.parent_lib, say)


if __name__ == "__main__":
    main()
