"""What the isosurface refinement costs (tn_isosurface_refine_*, cpp.isosurface_refine, render.extract_mesh(refine_rounds=...)),
against the same statement written in torch on the same GPU tensors, and what it buys: the residual |density - level| of the
surface vertices per round, on a network.

    python profiles/isosurface_refine_bench.py [--rounds 7] [--out profiles/isosurface_refine_bench.txt]
    python profiles/isosurface_refine_bench.py --kernels   7 x cpp.isosurface_refine(2 rounds) per mesh and nothing else timed: for
                                                           rocprofv3 --kernel-trace --stats -- python ... --kernels, a run of its own

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra).  The network: a default-initialised TetraMLP (seed 0) on the field  field[:, v] = A cos(4 pi x_v)
+ B sin(4 pi x_v)  with A, B random [64, 3] -- smooth in space, as a trained field is, so that a level exists which about a tenth
of the tetrahedra cross (a field of independent random columns is crossed by seven tetrahedra in eight at any level).  The level
is found by bisection on the kernel's own vertex densities.
  begin / points / select / vertices   each entry alone, 20 back-to-back calls between two device events
  forward    the density-only gathering forward on the 7 N candidates of a round (tn_mlp_forward_gather, fp32), the same way
  refine     cpp.isosurface_refine with 2 and 4 rounds on an extracted surface: allocations included, no read-back, the same way
  mesh       render.extract_mesh with refine_rounds = 0 / 2 / 4, colours included, by the wall clock with a synchronise either side
  torch      the refinement's statement in torch on the GPU tensors, 2 rounds, the density by the PyTorch modules, by the wall clock;
             its brackets are compared with the kernels' once (they may differ where the two densities round apart at a candidate)
  residual   max and mean |density64(vertex) - level| over the surface vertices after 0 .. 4 rounds, density64 = the network in
             float64 on the float64 interpolation of the float32 field
Needs the GPU; there is no fallback.

Expected before any run.  A round is 7 N density-only samples: profiles/mlp_bf16_bench.txt has the density-only fp32 forward at
1.561 ms for 2.1M samples, 0.74 us per thousand.  7 N should be some 46k / 140k / 466k candidates (N as in
profiles/isosurface_bench.txt), 0.03 / 0.10 / 0.35 ms if that rate held at a size that no longer fills the device, which it
will not quite; either way the forward should DOMINATE the round.  The three small kernels request 33 N (begin), 25 N + 196 N (points), 61 N (select) and 64 N (vertices)
bytes, at most 15 MB for points at 1M tetrahedra: a few microseconds each, so launch-bound.  A refinement of 2 rounds should then
cost about 2 x the forward, and extract_mesh with it less than twice the unrefined call, whose read-backs and allocations stay."""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles"))
from isosurface_bench import SIZES, event_ms, interleaved, med, wall_ms   # noqa: E402

C = 7


def smooth_field(pts, seed):
    g = np.random.default_rng(seed)
    A, B = g.normal(size=(64, 3)), g.normal(size=(64, 3))
    x = 4 * np.pi * pts.astype(np.float64)
    return (0.5 * (A @ np.cos(x).T + B @ np.sin(x).T)).astype(np.float32)


def level_for(values, cells, fraction):
    """the level between the median and the maximum of the vertex values that `fraction` of the tetrahedra cross, by bisection"""
    v = values[cells]

    def crossing(level):
        inside = v >= np.float32(level)
        return float((inside.any(1) & ~inside.all(1)).mean())

    lo, hi = float(np.median(values)), float(values.max())
    if crossing(lo) <= fraction:
        return lo, crossing(lo)
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if crossing(mid) > fraction else (lo, mid)
    level = float(np.float32(lo))
    return level, crossing(level)


@torch.no_grad()
def torch_refine(render, mlp, field_rows, xyz, ev, values, level, rounds):
    """geometry.isosurface_refine_statement in torch on the device (every id valid), the density by the PyTorch modules"""
    a, b = ev[:, 0].long(), ev[:, 1].long()
    N = len(a)
    L = torch.tensor(level, dtype=torch.float32, device=xyz.device)
    j = (torch.arange(1, C + 1, device=xyz.device, dtype=torch.float32) * 0.125)[None]
    lo, hi, slo, shi = torch.zeros(N, device=xyz.device), torch.ones(N, device=xyz.device), values[a], values[b]
    frozen = torch.zeros(N, dtype=torch.bool, device=xyz.device)
    fa, fb = field_rows[a], field_rows[b]
    for _ in range(rounds):
        t = lo[:, None] + j * (hi - lo)[:, None]
        feats = (1.0 - t)[..., None] * fa[:, None] + t[..., None] * fb[:, None]
        s = render.coarse_sigma(mlp, feats.reshape(N * C, 64)).reshape(N, C)
        ts = torch.cat([lo[:, None], t, hi[:, None]], 1)
        ss = torch.cat([slo[:, None], s, shi[:, None]], 1)
        inside = ss >= L
        differ = inside[:, :-1] != inside[:, 1:]
        first = differ.int().argmax(1, keepdim=True)
        frozen = frozen | ~(s.abs() < 2.0 ** 126).all(1) | ~differ.any(1)
        pick = lambda x, k: torch.gather(x, 1, first + k)[:, 0]   # noqa: E731
        lo, hi, slo, shi = (torch.where(frozen, old, new) for old, new in
                            ((lo, pick(ts, 0)), (hi, pick(ts, 1)), (slo, pick(ss, 0)), (shi, pick(ss, 1))))
    q = (L - slo) / (shi - slo)
    m = q * (hi - lo)
    t = torch.where(lo == 0, m, lo + m)
    t = torch.where(~(t >= lo), lo, torch.where(t > hi, hi, t))
    return {"edge_t": t, "positions": xyz[a] + t[:, None] * (xyz[b] - xyz[a]), "edge_bracket": torch.stack([lo, hi, slo, shi], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "isosurface_refine_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    render = importlib.import_module("tetra-nerf_amd.render")
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    cpp = tn.cpp
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"isosurface_refine_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    m64 = render.TetraMLP().double().to(dev)
    m64.load_state_dict({k: v.double() for k, v in mlp.state_dict().items()})
    w = [t.detach() for t in render.mlp_weights(mlp)]
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        field = torch.from_numpy(smooth_field(pts, seed)).to(dev).contiguous()
        x, c = torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev)
        values = cpp.mlp_forward(field, None, w, 1)
        level, crossing = level_for(values.cpu().numpy(), cells, 0.1)
        V, T = len(pts), len(cells)
        surface = cpp.isosurface(x, c, values, level)
        ev = surface["edge_vertices"]
        N = len(ev)
        if args.kernels:
            for _ in range(args.rounds):
                cpp.isosurface_refine(surface, x, values, level, field, w, 2)
            torch.cuda.synchronize()
            say(f"kernels: {args.rounds} x cpp.isosurface_refine(2 rounds) at {T} tets, {N} welded vertices, {C * N} candidates per round done")
            continue
        stream = torch.cuda.current_stream().cuda_stream
        br, fl = torch.empty((N, 4), device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
        vi, bc = torch.empty((N * C, 4), dtype=torch.int32, device=dev), torch.empty((N * C, 3), device=dev)
        et, pos = torch.empty(N, device=dev), torch.empty((N, 3), device=dev)
        p = lambda t: t.data_ptr()   # noqa: E731

        def begin():
            assert lib.tn_isosurface_refine_begin(V, N, p(ev), p(values), level, p(br), p(fl), stream) == 0

        def points_():
            assert lib.tn_isosurface_refine_points(V, N, 0, p(ev), p(br), p(fl), p(vi), p(bc), stream) == 0

        begin()
        points_()
        dens = cpp.mlp_forward_gather(vi, bc, field, None, w, 1)
        saved = br.clone()

        def select():      # (in place: every call of a window but the first narrows a narrower bracket, with the same loads and stores)
            assert lib.tn_isosurface_refine_select(N, 0, level, p(dens), p(br), p(fl), stream) == 0

        def vertices():
            assert lib.tn_isosurface_refine_vertices(V, N, p(x), p(ev), p(br), level, p(et), p(pos), stream) == 0

        def forward():
            cpp.mlp_forward_gather(vi, bc, field, None, w, 1)

        rows = field.t().contiguous()
        got = cpp.isosurface_refine(surface, x, values, level, field, w, 2)
        want = torch_refine(render, mlp, rows, x, ev, values, level, 2)
        same = float((got["edge_bracket"][:, :2] == want["edge_bracket"][:, :2]).all(1).float().mean())
        apart = float((got["positions"] - want["positions"]).abs().max())
        ts = interleaved(
            [(begin, event_ms), (points_, event_ms), (forward, event_ms), (select, event_ms), (vertices, event_ms),
             (lambda: cpp.isosurface_refine(surface, x, values, level, field, w, 2), event_ms),
             (lambda: cpp.isosurface_refine(surface, x, values, level, field, w, 4), event_ms),
             (lambda: render.extract_mesh(x, c, field, mlp, level), wall_ms),
             (lambda: render.extract_mesh(x, c, field, mlp, level, refine_rounds=2), wall_ms),
             (lambda: render.extract_mesh(x, c, field, mlp, level, refine_rounds=4), wall_ms),
             (lambda: torch_refine(render, mlp, rows, x, ev, values, level, 2), wall_ms)], args.rounds)
        br.copy_(saved)
        t_begin, t_points, t_fwd, t_select, t_vert, t_r2, t_r4, t_m0, t_m2, t_m4, t_torch = ts
        say(f"{name} {T} tets, {V} vertices, level {level:.6f}: {crossing:.1%} of the tetrahedra cross, {surface['num_triangles']} triangles, "
            f"{N} welded vertices, {C * N} candidates per round:")
        say(f"  begin    {med(t_begin)}      vertices {med(t_vert)}      (once per refinement)")
        say(f"  points   {med(t_points)}      select   {med(t_select)}      (once per round)")
        say(f"  forward  {med(t_fwd)} = {1e3 * m(t_fwd) / (C * N) * 1e3:.2f} us per thousand candidates = "
            f"{m(t_fwd) / (m(t_points) + m(t_select) + m(t_fwd)):.0%} of a round")
        say(f"  refine   2 rounds {med(t_r2)}, 4 rounds {med(t_r4)}; the sum of the parts: "
            f"{m(t_begin) + m(t_vert) + 2 * (m(t_points) + m(t_select) + m(t_fwd)):.3f} / {m(t_begin) + m(t_vert) + 4 * (m(t_points) + m(t_select) + m(t_fwd)):.3f} ms")
        say(f"  mesh     extract_mesh with 0 / 2 / 4 rounds {med(t_m0)} / {med(t_m2)} / {med(t_m4)} = 1 / {m(t_m2) / m(t_m0):.2f} / {m(t_m4) / m(t_m0):.2f}")
        say(f"  torch    the statement in torch, 2 rounds {med(t_torch)} = {m(t_torch) / m(t_r2):.1f} x cpp.isosurface_refine; {same:.2%} of its brackets "
            f"are the kernels', positions at most {apart:.2e} apart")
        # the residual per round, against the float64 network
        rows64 = rows.double()
        res = []
        for r in range(5):
            out = cpp.isosurface_refine(surface, x, values, level, field, w, r)
            t = out["edge_t"].double()[:, None]
            with torch.no_grad():
                s64 = render.coarse_sigma(m64, (1.0 - t) * rows64[ev[:, 0].long()] + t * rows64[ev[:, 1].long()])
            e = (s64 - level).abs()
            res.append(f"{float(e.max()):.2e} ({float(e.mean()):.2e})")
            frozen = int((out["edge_frozen"] != 0).sum())
        say(f"  residual max (mean) |density64 - level| after 0 .. 4 rounds: {' / '.join(res)}; frozen edges {frozen}; "
            f"vertex densities {float(values.min()):.3f} .. {float(values.max()):.3f}")


if __name__ == "__main__":
    main()
