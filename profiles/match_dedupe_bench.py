#!/usr/bin/env python3
"""Did the matcher keep its bits and its speed?  This build against the parent commit's, in alternating child processes, the
way mlp_forward_dedupe_bench.py does:

    python profiles/match_dedupe_bench.py --parent-lib OLD.so  [--identity]     same Python, two libraries (TETRANERF_HIP_LIB)
    python profiles/match_dedupe_bench.py --parent-root DIR                     two built checkouts, Python included (frame legs)

Speed legs:
  1. find_visited_cells at 4096 x 256 and 4096 x 513 samples on the mesh of bench.py's ops leg (45,000 points, seed 2), M = 512;
  2. the 800 x 800 `tetra-nerf-original` frame of bench.py's render leg (15,000-point mesh, M = 512, 256 + 256 samples,
     65,536-ray chunks) as kernel chain and as one launch, fp32, and as one launch, bf16x3.
Per process: the median of `rounds` warmed rounds; per leg: the median of the three processes' medians of each side, their ratio,
and the parent's own spread (max - min over its processes) -- the margin the ratio is read against.
--identity: every array of tests/test_match_gpu.py's cases, the frames of test_one_launch_render_is_bit_identical_to_the_kernel_chain
(chain and one launch, fp32 and bf16x3) and the find_visited_cells outputs of leg 1, written by one process per library and
compared byte for byte.
Needs a GPU; there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")


def ops_inputs(torch, tn, scenes, dev, M=512):
    """trace rows of 4096 outside-in rays through the ops-leg mesh; {S: distances}"""
    pts, cells = scenes.random_mesh(45000, 2)
    tracer = tn.TetrahedraTracer(dev)
    tracer.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    o, d = scenes.outside_in_rays(4096, 1)
    out = tracer.trace_rays(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), M)
    lists = [out[k] for k in KEYS]
    near = lists[3][:, 0, 0][:, None]
    far = torch.gather(lists[3][:, :, 1], 1, (lists[0].long()[:, None] - 1).clamp_min(0))
    dists = {}
    for S in (256, 513):
        ts = torch.linspace(0.0, 1.0, S, device=dev)[None]
        dists[S] = (near * (1 - ts) + far * ts).contiguous()
    return tracer, lists, dists


def child_speed(root, rounds):
    import torch

    import train_x3_bench as tb   # (interleaved(); puts its own tree on the path)
    sys.path.insert(0, str(root))
    tn = importlib.import_module("tetra-nerf_amd")
    assert Path(tn.__file__).resolve().parents[1] == root, tn.__file__
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    bench = importlib.import_module("bench")
    dev = torch.device("cuda:0")
    res = {}

    def run(fns, reps):
        for k, ms in tb.interleaved(torch, fns, rounds, reps=reps).items():
            res[k] = statistics.median(ms)

    tracer, lists, dists = ops_inputs(torch, tn, scenes, dev)
    run({f"find_visited_cells 4096x{S} M=512": (lambda s=s: tracer.find_visited_cells(*lists, s)) for S, s in dists.items()}, 20)
    del tracer, lists, dists

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
    for name, one, m in (("kernel chain fp32", False, "fp32"), ("one launch fp32", True, "fp32"), ("one launch bf16x3", True, "bf16x3")):
        rd = render.TetraRenderer(tracer, field, mlp, 256, 512, fused=True, num_fine_samples=256, mlp_mode=m, fused_pass=one)
        assert rd._one_launch_ok(m) == one

        def frame(rd=rd):
            for s in range(0, o.shape[0], 65536):
                rd.render(o[s:s + 65536], d[s:s + 65536])
        fns[f"render 800x800 tetra-nerf-original {name}"] = frame
    run(fns, 2)
    print("CHILD " + json.dumps(res), flush=True)


def child_dump(out_dir):
    import numpy as np
    import torch

    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import test_match_gpu as tm
    import test_render_rays_gpu as trr
    tn = importlib.import_module("tetra-nerf_amd")
    render = importlib.import_module("tetra-nerf_amd.render")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    dev = torch.device("cuda:0")
    arrays = {}

    def put(name, tensors):
        for k, v in tensors.items():
            arrays[f"{name}/{k}"] = v.cpu().numpy()

    pts, cells = scenes.cube_mesh()
    cube = tn.TetrahedraTracer(dev)
    cube.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
    for M in (1024, 2048):
        rows, dists = tm.match_cases(M)
        lists = [torch.from_numpy(rows[k]).to(dev) for k in KEYS]
        for S, s in dists.items():
            put(f"match M={M} S={S}", cube.find_visited_cells(*lists, torch.from_numpy(s).to(dev)))
    for S, S_fine, M, mode in tm.RENDER_CASES:
        a, b = tm.render_case(tn, dev, cube, S, S_fine, M, mode)
        put(f"long rows {S}+{S_fine} M={M} {mode} one launch", a)
        put(f"long rows {S}+{S_fine} M={M} {mode} chain", b)
    tr, mlp, field = trr._setup(tn, scenes, render, dev)
    fo, fd = trr._frame(scenes, dev, 120, 90)
    for S, S_fine, biased, M in ((64, 0, False, 256), (100, 37, False, 256), (256, 256, False, 512), (128, 128, True, 512), (64, 64, True, 1024),
                                 (33, 20, False, 256)):
        for mode in ("fp32", "bf16x3"):
            for one in (True, False):
                rd = render.TetraRenderer(tr, field, mlp, S, M, fused=True, num_fine_samples=S_fine, biased=biased, fused_pass=one, mlp_mode=mode)
                put(f"frame {S}+{S_fine} biased={biased} M={M} {mode} {'one launch' if one else 'chain'}", rd.render(fo, fd))
    tracer, lists, dists = ops_inputs(torch, tn, scenes, dev)
    for S, s in dists.items():
        put(f"ops mesh 4096x{S}", tracer.find_visited_cells(*lists, s))
    np.savez(out_dir, **arrays)
    print("CHILD " + json.dumps({"arrays": len(arrays)}), flush=True)


def run_child(args, env, timeout=600):
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), *args], env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:   # nothing further starts on the GPU
        raise RuntimeError(f"child process {args} failed ({p.returncode}):\n{p.stdout[-1000:]}\n{p.stderr[-3000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-root")
    ap.add_argument("--identity", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=str(HERE / "match_dedupe_bench.txt"))
    ap.add_argument("--child-speed")
    ap.add_argument("--child-dump")
    args = ap.parse_args()
    if args.child_speed:
        return child_speed(Path(args.child_speed), args.rounds)
    if args.child_dump:
        return child_dump(args.child_dump)
    if bool(args.parent_lib) == bool(args.parent_root):
        ap.error("one of --parent-lib / --parent-root is required")
    if args.parent_lib:
        sides = {"parent": (ROOT, dict(os.environ, TETRANERF_HIP_LIB=str(Path(args.parent_lib).resolve()))),
                 "branch": (ROOT, dict(os.environ, TETRANERF_HIP_LIB=str(ROOT / "tetra-nerf_amd" / "libtetranerf_hip.so")))}
    else:
        env = {k: v for k, v in os.environ.items() if k != "TETRANERF_HIP_LIB"}
        sides = {"parent": (Path(args.parent_root).resolve(), env), "branch": (ROOT, env)}
    lines = []
    if args.identity:
        import numpy as np

        with tempfile.TemporaryDirectory() as tmp:
            for k, (_, env) in sides.items():
                print(k, run_child(["--child-dump", f"{tmp}/{k}.npz"], env), flush=True)
            a, b = np.load(f"{tmp}/parent.npz"), np.load(f"{tmp}/branch.npz")
            assert sorted(a.files) == sorted(b.files)
            differ = [k for k in a.files if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
        lines += [f"byte identity, parent library against branch library: {len(a.files)} arrays compared, {len(differ)} differ", *differ]
    else:
        got = {k: {} for k in sides}
        for _ in range(args.processes):
            for k, (root, env) in sides.items():
                for leg, ms in run_child(["--child-speed", str(root), "--rounds", str(args.rounds)], env).items():
                    got[k].setdefault(leg, []).append(ms)
                print(k, "process done", flush=True)
        lines += [f"ms per call; {args.processes} alternating processes per side ({'libraries' if args.parent_lib else 'checkouts'}), "
                  f"per process the median of {args.rounds} warmed rounds",
                  f"{'leg':55s} {'parent (per process)':28s} {'branch (per process)':28s} {'parent':>8s} {'branch':>8s} {'ratio':>7s} {'spread':>7s}  verdict"]
        for leg in got["parent"]:
            a, b = got["parent"][leg], got["branch"][leg]
            ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
            lines.append(f"{leg:55s} {' '.join(f'{x:8.3f}' for x in a):28s} {' '.join(f'{x:8.3f}' for x in b):28s} {ma:8.3f} {mb:8.3f} "
                         f"{mb / ma:7.4f} {spread / ma * 100:6.2f}%  {'within' if mb - ma <= spread else 'SLOWER than parent + spread'}")
    print("\n".join(lines), flush=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, str(HERE))
    main()
