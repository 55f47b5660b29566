#!/usr/bin/env python3
"""What the bf16x3 weight-gradient GEMMs buy (tn_mlp_param_grads_ex mode 1; TetraRenderer(train_dw_mode="bf16x3")).

    python profiles/train_x3_dw_bench.py [--parent-lib OLD.so] [--rounds 7] [--out profiles/train_x3_dw_bench.txt]

One process, the candidates interleaved, medians over the rounds after a warm-up (device events around `reps` calls per round;
the helpers are profiles/train_x3_bench.py's and profiles/train_x3_adjoint_bench.py's):
  (a) the parameter gradients alone, tn_mlp_param_grads against tn_mlp_param_grads_ex(mode 1), at n = 4096 x 513 and 4096 x 257
      samples (the fine passes of the two shipped configurations), on the buffers an fp32 training forward and dX chain left
      (V = 45,000 vertices, random sample placement, upstream gradients at a loss's scale).  Both calls contain the direction
      encoding, the four GEMMs with their reductions and the rgb-head pass (528 B per sample, identical in both); the GEMMs must
      read 3840 B per sample, against which the achieved bytes/s of the whole call are stated;
  (b) one whole training iteration -- trace_rays + render_train + loss.backward() + SGD step, as bench.py's train leg -- with dW
      bf16x3 alone, with the forward and the dX chain in bf16x3, and with all three, against the default, for
      `tetra-nerf-original` (256 + 256) and `tetra-nerf` (128 + 128, biased, gradient scaling), 4096 outside-in rays of the
      C4-sized mesh (45,000 points, seed 2).
--parent-lib: (c) the default (fp32 everything) iteration of THIS build against another build of the library (the parent
commit's), in alternating child processes (TETRANERF_HIP_LIB), with the parent's own process-to-process spread beside the ratio;
and (d) profiles/compare_device_code.py PARENT.so THIS.so (no GPU needed): the device symbols that differ between the two.
--trace-leg S: nothing but ten calls of either entry at 4096 x S samples, for a per-kernel split of (a) under a tracer
(rocprofv3 --kernel-trace --stats -- python profiles/train_x3_dw_bench.py --trace-leg 513): the GEMM kernels and
k_reduce_partials without the encoding and the rgb-head pass that both entries share.
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles"))
from train_x3_bench import CONFIGS, fmt, interleaved  # noqa: E402
from train_x3_adjoint_bench import _NotExported, device_code_leg  # noqa: E402

NEW = ("tn_mlp_param_grads_ex",)
GEMM_BYTES = 3840            # per sample: d1..d4, h1..h3 (128 rows each) and x0 (64 rows), 4 bytes each
HEAD_BYTES = 528             # per sample: h4 (128 rows) and dhead (4 rows), the rgb-head pass of both modes


def kernel_leg(torch, tn, dev, rounds, say, trace=None):
    render = importlib.import_module("tetra-nerf_amd.render")
    cpp = tn.cpp
    lib = cpp._lib.load()
    V, R = 45000, 4096
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(dev)
    w = [x.detach() for x in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=dev) * 0.7
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1).contiguous()
    for S in (513, 257) if trace is None else (trace,):
        n = R * S
        vi = torch.randint(0, V, (n, 4), dtype=torch.int32, device=dev)
        bc = (torch.rand(n, 3, device=dev) / 3).contiguous()
        sigma, rgb, saved = cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S)
        d_sigma = (torch.randn(n, device=dev) * 1e-3).contiguous()
        d_rgb = (torch.randn(n, 3, device=dev) * 1e-3).contiguous()
        a = saved.acts
        buf = torch.empty((4 * 128 + 4, n), dtype=torch.float32, device=dev)
        rows = torch.empty((n, 64), dtype=torch.float32, device=dev)
        bs = cpp._MlpBackwardBuffers(a[0:64].data_ptr(), a[64:192].data_ptr(), a[192:320].data_ptr(), a[320:448].data_ptr(),
                                     a[448:576].data_ptr(), saved.masks.data_ptr(), buf[0:128].data_ptr(), buf[128:256].data_ptr(),
                                     buf[256:384].data_ptr(), buf[384:512].data_ptr(), buf[512:516].data_ptr(), rows.data_ptr())
        mh = cpp.fused_mlp(w)
        stream = cpp._stream(dev)
        cpp._lib.check(lib.tn_mlp_backward(mh.handle, n, sigma.data_ptr(), rgb.data_ptr(), d_sigma.data_ptr(), d_rgb.data_ptr(),
                                           ctypes.byref(bs), stream))
        grads = [torch.zeros(shp, dtype=torch.float32, device=dev) for shp in cpp._WEIGHT_SHAPES]
        gs = cpp._MlpWeightsStruct(*[g.data_ptr() for g in grads])
        head = (mh.handle, n, S, dirs.data_ptr(), ctypes.byref(bs), ctypes.byref(gs))
        fns = {"fp32   (tn_mlp_param_grads)": lambda: cpp._lib.check(lib.tn_mlp_param_grads(*head, stream)),
               "bf16x3 (tn_mlp_param_grads_ex, mode 1)": lambda: cpp._lib.check(lib.tn_mlp_param_grads_ex(*head, 1, stream))}
        if trace is not None:
            for _ in range(10):
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            say(f"ten calls of either entry at n = {R} x {S} = {n} samples")
            return
        res = interleaved(torch, fns, rounds, reps=5)
        say(f"parameter gradients alone (encoding + four dW GEMMs + reductions + rgb head), n = {R} x {S} = {n} samples "
            f"(the GEMMs read {n * GEMM_BYTES / 1e9:.2f} GB, the rgb head {n * HEAD_BYTES / 1e9:.2f} GB):")
        for k, ms in res.items():
            say(f"    {k:40s} {fmt(ms)}")
        a_ms, b_ms = (statistics.median(ms) for ms in res.values())
        total = n * (GEMM_BYTES + HEAD_BYTES)
        say(f"    bf16x3 / fp32 = {b_ms / a_ms:.3f}  (fp32 / bf16x3 = {a_ms / b_ms:.2f}x); 122.4 kFLOP per sample: "
            f"{n * 122.4e3 / (a_ms * 1e-3) / 1e12:.1f} -> {n * 122.4e3 / (b_ms * 1e-3) / 1e12:.1f} TFLOP/s; "
            f"{GEMM_BYTES + HEAD_BYTES} B per sample: {total / (a_ms * 1e-3) / 1e12:.2f} -> {total / (b_ms * 1e-3) / 1e12:.2f} TB/s achieved "
            f"({GEMM_BYTES} B of them the GEMMs')")
        del saved, a, buf, rows, bs, head, fns, grads, gs
        torch.cuda.empty_cache()


COMBOS = [("fp32", "fp32", "fp32"), ("fp32", "fp32", "bf16x3"), ("bf16x3", "bf16x3", "fp32"), ("bf16x3", "bf16x3", "bf16x3")]


def iteration_fns(torch, tn, dev, combos):
    """{(config, forward, adjoint, dw): step} on the C4-sized mesh, bench.py's train leg; combos of None: no keyword is passed"""
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
        for combo in combos:
            kw = {} if combo is None else dict(mlp_mode=combo[0], adjoint_mode=combo[1], dw_mode=combo[2])

            def step(rd=rd, opt=opt, scaling=scaling, kw=kw):
                opt.zero_grad(set_to_none=True)
                out = rd.render_train(o, d, gradient_scaling=scaling, **kw)
                ((out["rgb"] - target) ** 2).mean().backward()
                opt.step()
            fns[(name, combo)] = step
    return fns


def iteration_leg(torch, tn, dev, rounds, say):
    res = interleaved(torch, iteration_fns(torch, tn, dev, COMBOS), rounds, reps=5)
    for name, _ in CONFIGS:
        say(f"training iteration, {name}, 4096 rays, C4-sized mesh (trace + render_train + backward + SGD step):")
        med = {c: statistics.median(res[(name, c)]) for c in COMBOS}
        base = med[COMBOS[0]]
        for c in COMBOS:
            say(f"    forward {c[0]:7s} dX {c[1]:7s} dW {c[2]:7s} {fmt(res[(name, c)])}   / default = {med[c] / base:.3f}")
        say(f"    dW bf16x3 alone: {(1 - med[COMBOS[1]] / base) * 100:+.1f} % of an iteration saved; on top of the other two: "
            f"{(1 - med[COMBOS[3]] / med[COMBOS[2]]) * 100:+.1f} %; all three against the default: {(1 - med[COMBOS[3]] / base) * 100:+.1f} %")


class _OlderLibrary(ctypes.CDLL):
    """The parent commit's library has no tn_mlp_param_grads_ex, which this build's binding declares (and calls for the bf16x3
    weight gradients only: the default iteration goes through tn_mlp_param_grads in both builds).  That name resolves to
    _NotExported."""

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
    """the default iteration (no mode keyword at all) of whatever library TETRANERF_HIP_LIB names: one JSON line"""
    import faulthandler

    import torch

    faulthandler.enable()
    ctypes.CDLL = _OlderLibrary      # (this child process only; the binding loads its library through ctypes.CDLL)
    tn = importlib.import_module("tetra-nerf_amd")
    dev = torch.device("cuda:0")
    res = interleaved(torch, iteration_fns(torch, tn, dev, [None]), rounds, reps=5)
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
    say(f"default (fp32 forward, dX chain and dW) training iteration, this build against the parent commit's library, {alternations} "
        f"alternating processes each (per process: median of {rounds} rounds):")
    for name, _ in CONFIGS:
        for k in libs:
            say(f"    {name:20s} {k:10s} " + " ".join(f"{x:7.3f}" for x in got[k][name]) + f"   median {statistics.median(got[k][name]):7.3f} ms")
        ratio = statistics.median(got["this build"][name]) / statistics.median(got["parent"][name])
        lo, hi = min(got["parent"][name]), max(got["parent"][name])
        say(f"    {name:20s} this build / parent = {ratio:.4f}; the parent's own processes span {lo / statistics.median(got['parent'][name]):.4f} "
            f".. {hi / statistics.median(got['parent'][name]):.4f} of their median")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_x3_dw_bench.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace-leg", type=int, metavar="S")
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

    if args.trace_leg:
        return kernel_leg(torch, tn, dev, args.rounds, print, trace=args.trace_leg)
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    say(f"{torch.cuda.get_device_name(0)} | {lib.tn_version().decode()} | torch {torch.__version__}")
    kernel_leg(torch, tn, dev, args.rounds, say)
    iteration_leg(torch, tn, dev, args.rounds, say)
    if args.parent_lib:
        torch.cuda.synchronize()
        parent_leg(args.parent_lib, args.rounds, say)
        device_code_leg(args.parent_lib, say)


if __name__ == "__main__":
    main()
