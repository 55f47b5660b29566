#!/usr/bin/env python3
"""What expected depth and distortion loss cost (TetraRenderer.render_train(aux_outputs=True); csrc/tn_ray_aux.hip).

    python profiles/ray_aux_bench.py [--parent-tree DIR] [--rounds 7] [--out profiles/ray_aux_bench.txt]

One process, the candidates interleaved, medians over the rounds after a warm-up (device events around each call), as in
profiles/occupancy_sampler_bench.py, whose helpers this file takes.
  ops        4096 rays x 513 samples (thin rays, sigma < 4; edges from 1.0 on): composite beside composite + composite_aux;
             composite_backward without and with the two cotangents; and the same two quantities AND their gradient w.r.t. sigma
             written in PyTorch on the materialised weights (render.ray_weights under autograd): the pairwise O(S^2) form
             (render.composite_aux_statement; in 8 blocks of 512 rays, 0.5 GB per [512, 513, 513] temporary) and a cumsum form.
  iteration  a tetra-nerf-original and a tetra-nerf training iteration at 4096 rays (trace + render_train + backward + SGD step),
             without aux_outputs and with aux_outputs=True + a loss on both outputs.
  parent     (--parent-tree: a checkout of the parent commit with its library built) the DEFAULT frame and the DEFAULT training
             iteration of this tree against the parent commit's, Python and library, in alternating child processes.
Needs a GPU; there is no fallback."""
import argparse
import importlib
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "profiles"))


def _use_tree(tree):
    """import the package (and the bench helpers) from `tree`"""
    for p in (str(Path(tree) / "profiles"), str(tree)):
        sys.path.insert(0, p)


def ops_leg(torch, tn, dev, rounds, say):
    from occupancy_bench import fmt, interleaved

    render = importlib.import_module("tetra-nerf_amd.render")
    cpp = tn.cpp
    R, S = 4096, 513
    g = torch.Generator().manual_seed(0)
    sigma = (torch.rand(R, S, generator=g) * 4).to(dev)
    rgb = torch.rand(R, S, 3, generator=g).to(dev)
    edges = (1 + torch.cumsum(torch.rand(R, S + 1, generator=g) * 0.02, -1)).to(dev).contiguous()
    g_rgb, g_acc = torch.randn(R, 3, generator=g).to(dev), torch.randn(R, generator=g).to(dev)
    g_m, g_d = torch.randn(R, generator=g).to(dev), torch.randn(R, generator=g).to(dev)

    def torch_pairwise():
        grads = []
        for a in range(0, R, 512):
            s = sigma[a:a + 512].clone().requires_grad_(True)
            m, d = render.composite_aux_statement(s, edges[a:a + 512])
            ((m * g_m[a:a + 512]).sum() + (d * g_d[a:a + 512]).sum()).backward()
            grads.append(s.grad)
        return torch.cat(grads)

    def torch_cumsum():
        s = sigma.clone().requires_grad_(True)
        w = render.ray_weights(s, edges)
        e0 = edges[:, :1]
        u = ((edges[:, :-1] - e0) + (edges[:, 1:] - e0)) / 2
        wu = w * u
        W, WU = torch.cumsum(w, -1) - w, torch.cumsum(wu, -1) - wu
        m = e0[:, 0] * w.sum(-1) + wu.sum(-1)
        d = 2 * (w * (u * W - WU)).sum(-1) + (w * w * (edges[:, 1:] - edges[:, :-1])).sum(-1) / 3
        ((m * g_m).sum() + (d * g_d).sum()).backward()
        return s.grad

    def ours_aux_and_adjoint():
        cpp.composite_aux(sigma, edges)
        return cpp.composite_backward(sigma, rgb, edges, None, None, 1.0, d_depth_moment=g_m, d_distortion=g_d)[0]

    # the three agree before they are timed (the pairwise statement is the oracle)
    want = torch_pairwise()
    scale = float(want.abs().max())
    for name, fn in (("cumsum form", torch_cumsum), ("kernels", ours_aux_and_adjoint)):
        err = float((fn() - want).abs().max()) / scale
        assert err < 1e-4, (name, err)
    fns = {"composite": lambda: cpp.composite(sigma, rgb, edges),
           "composite + composite_aux": lambda: (cpp.composite(sigma, rgb, edges), cpp.composite_aux(sigma, edges)),
           "composite_backward (g_rgb, g_acc)": lambda: cpp.composite_backward(sigma, rgb, edges, g_rgb, g_acc, 1.0),
           "composite_backward (+ g_depth, g_dist)": lambda: cpp.composite_backward(sigma, rgb, edges, g_rgb, g_acc, 1.0, d_depth_moment=g_m, d_distortion=g_d),
           "both sums + d sigma: composite_aux + composite_backward (g_depth, g_dist)": ours_aux_and_adjoint,
           "both sums + d sigma: PyTorch, cumsum form, autograd": torch_cumsum,
           "both sums + d sigma: PyTorch, pairwise form, autograd, 8 x 512 rays": torch_pairwise}
    say(f"the ops alone, {R} rays x {S} samples:")
    res = interleaved(torch, fns, rounds, warm=2, reps=3)
    for k, ms in res.items():
        say(f"    {k:76s} {fmt(ms)}")
    med = {k: statistics.median(v) for k, v in res.items()}
    keys = list(fns)
    say(f"    composite_aux on top of composite: +{med[keys[1]] - med[keys[0]]:.3f} ms; the two cotangents on top of composite_backward: "
        f"+{med[keys[3]] - med[keys[2]]:.3f} ms; PyTorch cumsum form / kernels = {med[keys[5]] / med[keys[4]]:.1f} x, pairwise form / kernels = "
        f"{med[keys[6]] / med[keys[4]]:.1f} x")


def iteration_fns(torch, tn, dev, with_aux):
    """train_x3_dw_bench.iteration_fns' default step per configuration, and (with_aux) the same with aux_outputs=True and a loss on
    both outputs"""
    from train_x3_bench import CONFIGS

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

        def step(aux=False, rd=rd, opt=opt, scaling=scaling):
            opt.zero_grad(set_to_none=True)
            out = rd.render_train(o, d, gradient_scaling=scaling, **({"aux_outputs": True} if aux else {}))
            loss = ((out["rgb"] - target) ** 2).mean()
            if aux:
                loss = loss + 0.01 * out["distortion"].mean() + 0.01 * out["expected_depth"].mean()
            loss.backward()
            opt.step()
        fns[(name, "default")] = step
        if with_aux:
            fns[(name, "aux_outputs + loss on both")] = lambda step=step: step(True)
    return fns


def iteration_leg(torch, tn, dev, rounds, say):
    from occupancy_bench import fmt, interleaved

    res = interleaved(torch, iteration_fns(torch, tn, dev, True), rounds, reps=5)
    say("training iteration, 4096 rays, C4-sized mesh (trace + render_train + backward + SGD step):")
    for (name, kind), ms in res.items():
        say(f"    {name:22s} {kind:28s} {fmt(ms)}")
    for name in dict.fromkeys(n for n, _ in res):
        a, b = statistics.median(res[(name, "default")]), statistics.median(res[(name, "aux_outputs + loss on both")])
        say(f"    {name}: aux_outputs + loss / default = {b / a:.4f} (+{b - a:.3f} ms)")


def child(rounds, tree):
    """the default frame and the default training iteration (no keyword at all) of the tree"""
    import faulthandler

    _use_tree(tree)
    import torch
    import occupancy_bench as ob

    faulthandler.enable()
    tn = importlib.import_module("tetra-nerf_amd")
    assert Path(tn.__file__).resolve().is_relative_to(Path(tree).resolve()), tn.__file__
    dev = torch.device("cuda:0")
    render, tr, field, mlp, o, d, _ = ob.frame_setup(torch, tn, dev)
    rd = render.TetraRenderer(tr, field, mlp, ob.S_COARSE, 512, fused=True, num_fine_samples=ob.S_FINE)
    R, chunk = o.shape[0], 65536
    fns = {"frame 800x800 (256 + 256)": lambda: [rd.render(o[s:s + chunk], d[s:s + chunk])["rgb"] for s in range(0, R, chunk)]}
    out = {k: statistics.median(v) for k, v in ob.interleaved(torch, fns, rounds).items()}
    res = ob.interleaved(torch, iteration_fns(torch, tn, dev, False), rounds, reps=5)
    out.update({f"training iteration, {name}": statistics.median(ms) for (name, _), ms in res.items()})
    print("CHILD " + json.dumps(out), flush=True)


def parent_leg(parent_tree, rounds, say, alternations):
    trees = {"this tree": str(ROOT), "parent": str(Path(parent_tree).resolve())}
    got = {k: {} for k in trees}
    for _ in range(alternations):
        for k, tree in trees.items():
            p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", tree, "--rounds", str(rounds)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"child process on {tree} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1]
            for name, ms in json.loads(line[6:]).items():
                got[k].setdefault(name, []).append(ms)
    say(f"the default paths (no aux_outputs, fp32), this tree against a checkout of the parent commit (Python and library), {alternations} "
        f"alternating processes each (per process: median of {rounds} rounds):")
    for name in got["parent"]:
        for k in trees:
            say(f"    {name:42s} {k:10s} " + " ".join(f"{x:8.3f}" for x in got[k][name]) + f"   median {statistics.median(got[k][name]):8.3f} ms")
        med = statistics.median(got["parent"][name])
        ratio = statistics.median(got["this tree"][name]) / med
        lo, hi = min(got["parent"][name]) / med, max(got["parent"][name]) / med
        say(f"    {name:42s} this tree / parent = {ratio:.4f}; the parent's own processes span {lo:.4f} .. {hi:.4f} of their median: "
            f"{'inside' if lo <= ratio <= hi else 'OUTSIDE'} that spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ray_aux_bench.txt"))
    ap.add_argument("--child", metavar="TREE")
    ap.add_argument("--legs", default="ops,iteration,parent")
    ap.add_argument("--alternations", type=int, default=5, help="child processes per tree of the parent leg")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("medians over at least 7 rounds")
    if args.alternations < 5:
        ap.error("at least five alternations: three did not pin the spread (profiles/occupancy_sampler_bench.txt)")
    if args.child:
        return child(args.rounds, args.child)
    _use_tree(ROOT)
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
    if "iteration" in legs:
        iteration_leg(torch, tn, dev, args.rounds, say)
    if args.parent_tree and "parent" in legs:
        torch.cuda.synchronize()
        parent_leg(args.parent_tree, args.rounds, say, args.alternations)


if __name__ == "__main__":
    main()
