"""What a refit (TetrahedraTracer.update_vertices) costs and what it costs later, against load_tetrahedra.

    python profiles/refit_bench.py cost               refit vs load at ~100k / 300k / 1M tets (15,000 / 45,000 / 150,000 points)
    python profiles/refit_bench.py train              a 4096-ray training iteration on the C4 mesh (position_gradients on):
                                                      alone, + refit, + reload
    python profiles/refit_bench.py drift              trace_rays on a tracer refitted k = 1, 10, 100 times along a smooth random
                                                      drift against a fresh load of the same vertices (rows must be identical)
    python profiles/refit_bench.py default LABEL      the C2 frame and load_tetrahedra with the option OFF; run it alternately with
                                                      TETRANERF_HIP_LIB=<the parent commit's library> and without, >= 3 processes each
    python profiles/refit_bench.py kernels            nothing but refits (for rocprofv3 --kernel-trace --stats -- python ... kernels)

Every mode needs the GPU and APPENDS its lines to --out (default profiles/refit_bench.txt).  Load and refit are timed in the same
process, alternately, with a host clock around the blocking call (both end in a stream synchronise, and both include host work:
the hull tree, the read-backs); the trace calls with device events.  Medians (min .. max).

Expected before any run, from the bytes each pass moves (F = 2.05 T faces, about T / 3 binary nodes at 16-face leaves):
    thin pass       T x (16 B cells + 48 B gathered positions) + 4 T atomic minima into V words
    records         4 T x (32 B read + 32 B written) + T x (4 B order + 16 B cells) + cached gathers      ~ 280 B per tet
    BVH boxes       F x (4 B order + 12 B ids + 36 B gathered positions) + 24 B per node                   ~ 115 B per tet
    leaf triangles  F x (4 + 12 + 36 B) read, 36 B x 16 slots per leaf written (leaves are 9..16 full)      ~ 205 B per tet
    wide boxes      64 x 24 B per wide node (one per ~50 leaves)                                            ~   5 B per tet
so about 0.7 KB per tet: 0.02 / 0.07 / 0.2 ms at 100k / 300k / 1M tets if the passes ran at 3-4 TB/s.  They will not: the rest
is about 30 small launches (one per BVH level), the blocking read-back of the hull faces and of max |coordinate|, the host's
hull tree (a sort of n_hull keys) -- a few tenths of a millisecond, nearly independent of T.
"""
import argparse
import importlib
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SIZES = (("C2", 15000, 0), ("C4", 45000, 2), ("C5", 150000, 3))      # bench.py's meshes
KEYS = ("num_visited_cells", "visited_cells", "vertex_indices", "hit_distances", "barycentric_coordinates")


def med(ts):
    return f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(fns, rounds, timer, warm=2):
    for _ in range(warm):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(timer(f))
    return ts


def mesh(scenes, dev, points, seed):
    pts, cells = scenes.random_mesh(points, seed)
    return pts, cells, torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev)


def frame_rays(scenes, dev):
    """bench.py's C2 frame: 800 x 800 pinhole rays"""
    c = np.array([0.5, 0.5, 0.5], np.float32)
    o, d = scenes.pinhole_rays(800, 800, eye=tuple(c + 2.0 * np.array([0.0, 1.0, 0.0], np.float32)), lookat=tuple(c), up=(0.0, 0.0, 1.0))
    return torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)


def cost(tn, scenes, dev, rounds, lines):
    for name, points, seed in SIZES:
        pts, cells, x, c = mesh(scenes, dev, points, seed)
        tr, plain = tn.TetrahedraTracer(dev), tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(x, c, refittable=True)
        t_plain, t_load, t_refit = interleaved([lambda: plain.load_tetrahedra(x, c), lambda: tr.load_tetrahedra(x, c, refittable=True),
                                                lambda: tr.update_vertices(x)], rounds, wall_ms)
        kept = tr.refit_table_bytes()
        lines.append(f"{name} {len(cells)} tets, {len(pts)} vertices: load_tetrahedra {med(t_plain)}, with refit tables {med(t_load)}, "
                     f"update_vertices {med(t_refit)} = {statistics.median(t_plain) / statistics.median(t_refit):.1f} x; "
                     f"kept {kept} B = {kept / len(cells):.1f} B per tet")
        print(lines[-1], flush=True)


def kernels(tn, scenes, dev, rounds, lines):
    for name, points, seed in SIZES:
        _, cells, x, c = mesh(scenes, dev, points, seed)
        tr = tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(x, c, refittable=True)
        for _ in range(rounds):
            tr.update_vertices(x)
        torch.cuda.synchronize()
        lines.append(f"kernels: {rounds} refits at {len(cells)} tets done")


def train(tn, scenes, dev, rounds, lines):
    render = importlib.import_module("tetra-nerf_amd.render")
    pts, cells, x, c = mesh(scenes, dev, 45000, 2)
    tr = tn.TetrahedraTracer(dev)
    verts = x.clone().requires_grad_(True)
    tr.load_tetrahedra(verts.detach(), c, refittable=True)
    o, d = scenes.outside_in_rays(4096, 1)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    V = len(pts)
    f2 = ((torch.rand(64, V, device=dev) * 2 - 1) * 1e-4)
    f2[1:4] = torch.rand(3, V, device=dev) * 2 - 1
    f2.requires_grad_(True)
    opt = torch.optim.SGD([f2] + list(mlp.parameters()), lr=1e-3)       # (the vertices get a gradient and are left where they are)
    rd = render.TetraRenderer(tr, f2, mlp, 256, 512, fused=True, num_fine_samples=256)
    target = torch.rand(len(o), 3, device=dev)

    def step(follow):
        opt.zero_grad(set_to_none=True)
        verts.grad = None
        res = rd.render_train(o, d, position_gradients=True, vertices=verts)
        ((res["rgb"] - target) ** 2).mean().backward()
        opt.step()
        if follow == "refit":
            tr.update_vertices(verts.detach())
        elif follow == "reload":
            tr.load_tetrahedra(verts.detach(), c, refittable=True)

    t0, t1, t2 = interleaved([lambda: step(None), lambda: step("refit"), lambda: step("reload")], rounds, wall_ms)
    m0, m1, m2 = (statistics.median(t) for t in (t0, t1, t2))
    lines.append(f"C4 {len(cells)} tets, 4096-ray training iteration (256 + 513 samples, position_gradients on; trace + forward + backward + "
                 f"SGD): alone {med(t0)}; + update_vertices {med(t1)} (+{(m1 / m0 - 1) * 100:.1f} %, {(m1 - m0) / m1 * 100:.1f} % of the "
                 f"iteration); + load_tetrahedra {med(t2)} (+{(m2 / m0 - 1) * 100:.1f} %)")
    print(lines[-1], flush=True)


def drift(tn, scenes, dev, rounds, lines):
    """smooth drift: every step adds 0.002 x a fixed low-frequency field (three sines per axis) -- 100 steps move a vertex by up
    to ~0.2 of the unit cube while neighbours move together.  The tetrahedra whose signed volume changes sign are counted in
    float64 and reported: a random Delaunay mesh has near-flat slivers on its hull that any non-affine drift inverts."""
    def volumes(p):
        q = np.asarray(p, np.float64)[cells.astype(np.int64)]
        return np.einsum("ij,ij->i", np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), q[:, 3] - q[:, 0])

    pts, cells, x, c = mesh(scenes, dev, 15000, 0)
    rng = np.random.default_rng(7)
    freq, phase, amp = rng.uniform(1.0, 3.0, (3, 3)), rng.uniform(0, 2 * np.pi, (3, 3)), rng.normal(size=(3, 3))
    p64 = pts.astype(np.float64)
    field = np.stack([(amp[a] * np.sin(p64 * freq[a] + phase[a])).sum(1) for a in range(3)], 1)
    field /= np.abs(field).max()
    fo, fd = frame_rays(scenes, dev)
    o4, d4 = scenes.outside_in_rays(4096, 1)
    o4, d4 = torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(x, c, refittable=True)
    done = 0
    for k in (1, 10, 100):
        while done < k:
            done += 1
            cur = torch.from_numpy((p64 + 0.002 * done * field).astype(np.float32)).to(dev)
            tr.update_vertices(cur)
        now = cur.cpu().numpy()
        flips = int(np.count_nonzero(volumes(pts) * volumes(now) < 0))
        fresh = tn.TetrahedraTracer(dev)
        fresh.load_tetrahedra(cur, c)
        for label, (to, td), walk in (("4096 rays, BVH path", (o4, d4), 0), ("C2 frame 640,000 rays, walk", (fo, fd), 1)):
            tr.set_option("walk", walk); fresh.set_option("walk", walk)
            a, b = tr.trace_rays(to, td, 512), fresh.trace_rays(to, td, 512)
            same = all(torch.equal(a[q].view(torch.int32), b[q].view(torch.int32)) for q in KEYS)
            del a, b
            ta, tb = interleaved([lambda: tr.trace_rays(to, td, 512), lambda: fresh.trace_rays(to, td, 512)], rounds, event_ms)
            lines.append(f"drift k = {k:3d} ({flips} flipped tets), {label}: refitted {med(ta)}, fresh load {med(tb)} "
                         f"({(statistics.median(ta) / statistics.median(tb) - 1) * 100:+.1f} %), rows {'identical' if same else 'DIFFER'}")
            print(lines[-1], flush=True)


def default(tn, scenes, dev, rounds, lines, label):
    lib = importlib.import_module("tetra-nerf_amd._lib")
    _, cells, x, c = mesh(scenes, dev, 15000, 0)
    fo, fd = frame_rays(scenes, dev)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(x, c)
    (t_load,) = interleaved([lambda: tr.load_tetrahedra(x, c)], rounds, wall_ms)
    (t_frame,) = interleaved([lambda: tr.trace_rays(fo, fd, 512)], rounds, event_ms)
    lines.append(f"default {label} ({Path(str(lib.LIB_PATH)).name}): C2 frame {med(t_frame)}, load_tetrahedra {med(t_load)}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("cost", "train", "drift", "default", "kernels"))
    ap.add_argument("label", nargs="?", default="this build")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refit_bench.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    lines = []
    if args.mode == "default":
        default(tn, scenes, dev, args.rounds, lines, args.label)
    else:
        lines.append(f"refit_bench {args.mode}: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max)")
        {"cost": cost, "train": train, "drift": drift, "kernels": kernels}[args.mode](tn, scenes, dev, args.rounds, lines)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
