#!/usr/bin/env python3
"""What the fused RAdam step costs next to torch.optim.RAdam (optim.FusedRAdam; csrc/tn_optim.hip).

    python profiles/radam_bench.py [--rounds 7] [--out profiles/radam_bench.txt] [--legs step,iteration]
    python profiles/radam_bench.py --torch-step-only       (for ONE `rocprofv3 --kernel-trace --stats -- python ...` run, on its own:
                                                            the launches of torch's RAdam step on the field + its transposition)

One process, the candidates interleaved, medians over the rounds after a warm-up, device events around `reps` calls per round
(profiles/train_x3_bench.py's helpers):
  (a) the step alone, gradients fixed: the C4-sized field [64, 45,000], a field of V = 1,000,000 and the MLP's 12 tensors only.
      torch.optim.RAdam (default: foreach) PLUS the tn_transpose_f32 its in-place step causes for a registered field
      (cpp.field_vertex_major after the step) against FusedRAdam (whose step leaves the shadow behind: field_vertex_major after it
      is a cache hit).  For the fields also in GB/s of the 2 KB per vertex a single pass must move (4 reads + 4 writes of 256 B).
  (b) bench.py's training leg re-stated: trace + render_train + backward + optimiser step at 4096 rays of the C4-sized mesh, both
      shipped configurations, with SGD (what README's training figures use), torch.optim.RAdam and FusedRAdam.
Needs a GPU; there is no fallback."""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles"))
from train_x3_bench import CONFIGS, fmt, interleaved  # noqa: E402

BYTES_PER_VERTEX = 8 * 64 * 4      # p, g, exp_avg, exp_avg_sq read; p, exp_avg, exp_avg_sq, shadow written


def _field_candidates(torch, tn, optim, dev, V):
    """{label: step} on two registered fields with fixed gradients: torch's RAdam + the transposition it causes, FusedRAdam"""
    cpp = tn.cpp
    fns, keep = {}, []
    for label, cls in (("torch.optim.RAdam (foreach) + tn_transpose_f32", torch.optim.RAdam), ("FusedRAdam (field + shadow in one pass)", optim.FusedRAdam)):
        field = ((torch.rand(64, V, device=dev) * 2 - 1) * 0.5).requires_grad_(True)
        field.grad = torch.randn(64, V, device=dev) * 1e-3
        cpp.register_field(field)
        opt = cls([field], lr=1e-3)
        keep.append((field, opt))

        def step(field=field, opt=opt):
            opt.step()
            cpp.field_vertex_major(field)

        fns[label] = step
    return fns, keep


def step_leg(torch, tn, optim, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    for V, reps in ((45000, 20), (1000000, 5)):
        fns, keep = _field_candidates(torch, tn, optim, dev, V)
        res = interleaved(torch, fns, rounds, reps=reps)
        say(f"the step alone, field [64, {V}] ({64 * V * 4 / 1e6:.1f} MB), registered (the next gather needs its [V, 64] shadow):")
        for label, ms in res.items():
            med = statistics.median(ms)
            say(f"    {label:52s} {fmt(ms)}   {V * BYTES_PER_VERTEX / (med * 1e-3) / 1e9:7.0f} GB/s of 2 KB per vertex")
        a, b = (statistics.median(v) for v in res.values())
        say(f"    torch + transposition / fused = {a / b:.2f}x")
        for field, _ in keep:
            tn.cpp.unregister_field(field)
        del fns, keep
        torch.cuda.empty_cache()
    fns, keep = {}, []
    for label, cls in (("torch.optim.RAdam (foreach)", torch.optim.RAdam), ("FusedRAdam (one launch)", optim.FusedRAdam)):
        torch.manual_seed(0)
        mlp = render.TetraMLP().to(dev)
        params = list(mlp.parameters())
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        opt = cls(params, lr=1e-3)
        keep.append((mlp, opt))
        fns[label] = opt.step
    res = interleaved(torch, fns, rounds, reps=20)
    say(f"the step alone, the MLP's {len(params)} tensors ({sum(p.numel() for p in params)} elements): launch-bound on both sides")
    for label, ms in res.items():
        say(f"    {label:52s} {fmt(ms)}")


def iteration_leg(torch, tn, optim, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    pts, cells = scenes.random_mesh(45000, 2)
    tracer = tn.TetrahedraTracer(dev)
    tracer.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = scenes.outside_in_rays(4096, 1)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    target = torch.rand(len(o), 3, device=dev)
    optimisers = (("SGD (bench.py's training leg)", lambda ps: torch.optim.SGD(ps, lr=1e-3)),
                  ("torch.optim.RAdam (foreach)", lambda ps: torch.optim.RAdam(ps, lr=1e-3)),
                  ("FusedRAdam", lambda ps: optim.FusedRAdam(ps, lr=1e-3)))
    for name, (s_c, s_f, biased, scaling) in CONFIGS:
        fns, keep = {}, []
        for label, make in optimisers:
            torch.manual_seed(0)
            mlp = render.TetraMLP().to(dev)
            field = ((torch.rand(64, len(pts), device=dev) * 2 - 1) * 1e-4)
            field[1:4] = torch.rand(3, len(pts), device=dev) * 2 - 1
            field.requires_grad_(True)
            opt = make([field] + list(mlp.parameters()))
            rd = render.TetraRenderer(tracer, field, mlp, s_c, 512, fused=True, num_fine_samples=s_f, biased=biased)
            keep.append((mlp, field, opt, rd))

            def step(opt=opt, rd=rd):
                opt.zero_grad(set_to_none=True)
                out = rd.render_train(o, d, gradient_scaling=scaling)
                ((out["rgb"] - target) ** 2).mean().backward()
                opt.step()

            fns[label] = step
        res = interleaved(torch, fns, rounds, reps=5)
        say(f"training iteration, {name}, 4096 rays, C4-sized mesh ({len(pts)} vertices, {len(cells)} tetrahedra): trace + render_train + "
            "backward + optimiser step")
        ref = statistics.median(res[optimisers[1][0]])
        for label, ms in res.items():
            say(f"    {label:36s} {fmt(ms)}   {statistics.median(ms) / ref:.3f} x torch's RAdam")
        for _, field, _, _ in keep:
            tn.cpp.unregister_field(field)
        del fns, keep
        torch.cuda.empty_cache()


def torch_step_only(torch, tn, optim, dev):
    """20 steps of torch's RAdam on the V = 1M field, each followed by the transposition: what one kernel-trace run counts"""
    fns, keep = _field_candidates(torch, tn, optim, dev, 1000000)
    step = next(iter(fns.values()))
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    print("20 steps of torch.optim.RAdam (foreach) on a registered [64, 1000000] field, each followed by field_vertex_major")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "radam_bench.txt"))
    ap.add_argument("--legs", default="step,iteration")
    ap.add_argument("--torch-step-only", action="store_true")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("medians over at least 5 rounds")
    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    tn = importlib.import_module("tetra-nerf_amd")
    optim = importlib.import_module("tetra-nerf_amd.optim")
    dev = torch.device("cuda:0")
    if args.torch_step_only:
        return torch_step_only(torch, tn, optim, dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    say(f"{torch.cuda.get_device_name(0)} | {lib.tn_version().decode()} | torch {torch.__version__}")
    legs = args.legs.split(",")
    if "step" in legs:
        step_leg(torch, tn, optim, dev, args.rounds, say)
    if "iteration" in legs:
        iteration_leg(torch, tn, optim, dev, args.rounds, say)


if __name__ == "__main__":
    main()
