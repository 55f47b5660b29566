#!/usr/bin/env python3
"""What the per-tetrahedron occupancy field costs and buys on the evaluation frame (TetraRenderer.render(occupancy=,
occupancy_threshold=); csrc/tn_occupancy.hip).

    python profiles/occupancy_bench.py [--rounds 7] [--out profiles/occupancy_bench.txt]

One process, the candidates interleaved, medians over the rounds after a warm-up (device events around each call).  The frame is
the 800 x 800 frame of bench.py's C2 scene (15,000-point mesh seed 0, 65,536-ray chunks), `tetra-nerf-original` (256 + 256
samples), in fp32 and bf16x3.  The reference of every comparison is the kernel chain WITHOUT an occupancy in the same process
(fused_pass=False: what a culled call is built from; the persistent launch does not cull):
  (a) the culled chain with a threshold that culls nothing: the overhead of cull_samples + the indexed forward;
  (b) the culled chain with SYNTHETIC occupancies (uniform random per tetrahedron) and the thresholds 0.5 / 0.9, which leave
      about 50 % / 10 % of the matched samples live; the live fraction actually reached is reported;
  (c) the three new kernels alone at 4096 x 513 samples, the indexed forward next to mlp_forward_gather on the same samples;
  (d) the frame difference with occupancy_from_field and one stated threshold: max |d rgb| and PSNR against the unculled frame.
Needs a GPU; there is no fallback."""
import argparse
import importlib
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
MODES = ("fp32", "bf16x3")
S_COARSE, S_FINE = 256, 256


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(torch, fns, rounds, warm=1, reps=1):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(sum(timed(torch, fn) for _ in range(reps)) / reps)
    return out


def fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):8.3f}, max {max(ms):8.3f}, {len(ms)} rounds)"


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
    return render, tr, field, mlp, o, d, torch.from_numpy(cells).to(dev)


def live_fraction(torch, tn, frame):
    """(samples the network ran on, samples of the hitting rays, matched samples, live matched samples) of one frame, both passes"""
    real = tn.cpp.cull_samples
    seen = []

    def spy(cells, occupancy, threshold, sigma, rgb=None, samples_per_ray=None, count=None):
        live, live_count = real(cells, occupancy, threshold, sigma, rgb, samples_per_ray=samples_per_ray, count=count)
        n = int(count) * cells.size(-1) if count is not None else cells.numel()
        c = cells.reshape(-1)[:n]
        matched = (c >= 0) & (c < occupancy.numel())
        below = (occupancy[c.clamp(0, occupancy.numel() - 1).long()] < threshold) & (threshold > 0)
        seen.append((int(live_count), n, int(matched.sum()), int((matched & ~below).sum())))
        return live, live_count

    tn.cpp.cull_samples = spy
    try:
        frame()
    finally:
        tn.cpp.cull_samples = real
    return tuple(sum(x[i] for x in seen) for i in range(4))


def frame_leg(torch, tn, dev, rounds, say):
    render, tr, field, mlp, o, d, cells = frame_setup(torch, tn, dev)
    R, chunk, T = o.shape[0], 65536, cells.shape[0]
    occ = torch.rand(T, generator=torch.Generator().manual_seed(1)).to(dev)

    def frame_of(rd, **kw):
        return lambda: torch.cat([rd.render(o[s:s + chunk], d[s:s + chunk], **kw)["rgb"] for s in range(0, R, chunk)])

    say(f"800 x 800 frame, tetra-nerf-original ({S_COARSE} + {S_FINE}), 15,000-point mesh ({T} tetrahedra), 65,536-ray chunks "
        "(trace + TetraRenderer.render):")
    for mode in MODES:
        chain = render.TetraRenderer(tr, field, mlp, S_COARSE, 512, fused=True, num_fine_samples=S_FINE, mlp_mode=mode, fused_pass=False)
        one = render.TetraRenderer(tr, field, mlp, S_COARSE, 512, fused=True, num_fine_samples=S_FINE, mlp_mode=mode)
        fns = {"chain, no occupancy (the reference)": frame_of(chain),
               "one persistent launch, no occupancy": frame_of(one),
               "(a) culled chain, threshold 0 (culls nothing)": frame_of(chain, occupancy=occ, occupancy_threshold=0.0),
               "(b) culled chain, uniform occupancy, threshold 0.5": frame_of(chain, occupancy=occ, occupancy_threshold=0.5),
               "(b) culled chain, uniform occupancy, threshold 0.9": frame_of(chain, occupancy=occ, occupancy_threshold=0.9)}
        res = interleaved(torch, fns, rounds)
        ref = statistics.median(res["chain, no occupancy (the reference)"])
        say(f"  {mode}:")
        for k, ms in res.items():
            say(f"    {k:52s} {fmt(ms)}   {statistics.median(ms) / ref:.3f} x the reference")
        for thr in (0.5, 0.9):
            ran, total, matched, live_matched = live_fraction(torch, tn, frame_of(chain, occupancy=occ, occupancy_threshold=thr))
            say(f"    threshold {thr}: the network ran on {ran} of {total} samples of the hitting rays ({ran / max(total, 1):.3f}); "
                f"{live_matched} of {matched} matched samples live ({live_matched / max(matched, 1):.3f}); both passes")
        same = torch.equal(fns["(a) culled chain, threshold 0 (culls nothing)"](), fns["chain, no occupancy (the reference)"]())
        say(f"    (a) frame bit-identical to the reference: {same}")
    # (d) a starting occupancy from the field itself
    chain = render.TetraRenderer(tr, field, mlp, S_COARSE, 512, fused=True, num_fine_samples=S_FINE, fused_pass=False)
    occ_f = render.occupancy_from_field(cells, field, mlp)
    thr = float(torch.quantile(occ_f, 0.10))
    want = frame_of(chain)()
    got = frame_of(chain, occupancy=occ_f, occupancy_threshold=thr)()
    ran, total, matched, live_matched = live_fraction(torch, tn, frame_of(chain, occupancy=occ_f, occupancy_threshold=thr))
    diff = (got - want).abs()
    mse = float(((got - want).double() ** 2).mean())
    psnr = float("inf") if mse == 0 else 10 * math.log10(1.0 / mse)
    say(f"(d) occupancy_from_field (fp32): occupancy min {float(occ_f.min()):.4f} / median {float(occ_f.median()):.4f} / max "
        f"{float(occ_f.max()):.4f}; threshold = its 10th percentile = {thr:.6f} (this scene's field is ~0: a nearly uniform density, no "
        "empty space -- the figure is the damage of culling the emptiest tenth of the tetrahedra of a full volume)")
    say(f"    {live_matched} of {matched} matched samples live ({live_matched / max(matched, 1):.3f}); culled frame against the unculled "
        f"fp32 frame: max |d rgb| {float(diff.max()):.3e}, mean |d rgb| {float(diff.mean()):.3e}, PSNR {psnr:.2f} dB")


def kernel_leg(torch, tn, dev, rounds, say):
    render = importlib.import_module("tetra-nerf_amd.render")
    R, S, V, T = 4096, 513, 45000, 100000
    n = R * S
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(dev)
    w = [x.detach() for x in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=dev) * 0.7
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1)
    vi = torch.randint(0, V, (n, 4), dtype=torch.int32, device=dev)
    bc = (torch.rand(n, 3, device=dev) / 3).contiguous()
    # matched cells in runs of about four samples, as along a ray
    cells = torch.randint(0, T, (n // 4 + 1,), dtype=torch.int32, device=dev).repeat_interleave(4)[:n].contiguous().view(R, S)
    occ = torch.rand(T, device=dev)
    sigma = torch.rand(n, device=dev) * 5
    rgb = torch.rand(n, 3, device=dev)
    say(f"the new kernels alone, n = {R} x {S} = {n} samples, {T} tetrahedra (cells in runs of 4), V = {V}:")
    fns = {"occupancy_update": lambda: tn.cpp.occupancy_update(occ.clone(), cells, sigma, 0.95)}
    for thr in (0.0, 0.5, 0.9):
        fns[f"cull_samples, threshold {thr} (sigma and rgb)"] = lambda thr=thr: tn.cpp.cull_samples(cells, occ, thr, sigma, rgb, samples_per_ray=S)
    res = interleaved(torch, fns, rounds, warm=2, reps=3)
    for k, ms in res.items():
        say(f"    {k:52s} {fmt(ms)}")
    say("    (occupancy_update includes a clone of the 100,000-float field per call)")
    lists = {thr: tn.cpp.cull_samples(cells, occ, thr, sigma.clone(), rgb.clone(), samples_per_ray=S) for thr in (0.0, 0.5, 0.9)}
    for mode in MODES:
        for form, dd in (("full", dirs), ("density only", None)):
            out_s = torch.empty(n, device=dev)
            out_c = None if dd is None else torch.empty(n, 3, device=dev)
            fns = {"mlp_forward_gather (all samples)": lambda dd=dd: tn.cpp.mlp_forward_gather(vi, bc, field, dd, w, S, mode=mode)}
            for thr, (live, live_count) in lists.items():
                frac = int(live_count) / n
                fns[f"indexed, {frac:.3f} of the samples listed"] = (
                    lambda dd=dd, live=live, live_count=live_count: tn.cpp.mlp_forward_gather_indexed(
                        live, live_count, vi, bc, field, dd, w, S, mode=mode, sigma=out_s, rgb=out_c))
            res = interleaved(torch, fns, rounds, warm=2, reps=3)
            ref = statistics.median(res["mlp_forward_gather (all samples)"])
            say(f"  {mode}, {form}:")
            for k, ms in res.items():
                say(f"    {k:52s} {fmt(ms)}   {statistics.median(ms) / ref:.3f} x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_bench.txt"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("medians over at least 5 rounds")
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
    frame_leg(torch, tn, dev, args.rounds, say)
    kernel_leg(torch, tn, dev, args.rounds, say)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
