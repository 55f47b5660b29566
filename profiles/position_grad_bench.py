"""Timing of the position-gradient kernels against the only way to compute the same quantities without them.

(A) tn_interpolate_values_backward_bary_vm and (B) tn_sample_positions_backward at 4096 x 256 and 4096 x 257 samples of the
C4 mesh (45,000 points seed 2; 4096 outside-in rays seed 1), each against its PyTorch composition:
    (A)  field_vm[vi] gather + einsum over the row differences
    (B)  table[vi] gather + add_barycentrics_grad (batched torch.linalg.solve) + index_add_ into [V,3] + per-ray sums,
         on the MATCHED samples only, compacted outside the timed window (a singular T of an unmatched sample stops the solve)
HIP events after warm-up, the two sides interleaved in one process (kernel, yardstick, kernel, ...), medians reported.
(A)'s achieved bytes/s is over its ALGORITHMIC bytes: 5 rows of 4 F bytes read (G and the 4 vertex rows) + 4 (D - 1) bytes
written per sample.  Then one training iteration (trace + render_train + backward + SGD, tetra-nerf-original 256 + 256) with
position_gradients on against off, interleaved the same way.

    python profiles/position_grad_bench.py [--out FILE]     (needs the GPU; writes FILE, default profiles/position_grad_bench.txt)
"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(fns, rounds, warm=3):
    """median ms of each callable, run alternately"""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(timed(f))
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "position_grad_bench.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    render = importlib.import_module("tetra-nerf_amd.render")
    cpp = tn.cpp
    lines = [f"position_grad_bench: {torch.cuda.get_device_name(0)}, C4 mesh (45,000 points seed 2), 4096 outside-in rays seed 1; "
             f"medians of {args.rounds} interleaved rounds (min .. max)"]

    pts, cells = scenes.random_mesh(45000, 2)
    table = torch.from_numpy(pts).to(dev)
    tr = tn.TetrahedraTracer(dev)
    tr.load_tetrahedra(table, torch.from_numpy(cells).to(dev))
    o, d = scenes.outside_in_rays(4096, 1)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    M, V, R = 512, len(pts), len(o)
    out = tr.trace_rays(o, d, M)
    nv = out["num_visited_cells"]
    near = out["hit_distances"][:, 0, 0]
    far = torch.gather(out["hit_distances"][:, :, 1], 1, (nv[:, None].long() - 1).clamp_min(0))[:, 0]
    torch.manual_seed(0)
    field = torch.randn(64, V, device=dev)
    field_vm = field.t().contiguous()
    cpp.register_field(field)

    for S in (256, 257):
        ts = ((torch.arange(S, device=dev, dtype=torch.float32) + 0.5) / S)[None]
        dist = (near[:, None] * (1 - ts) + far[:, None] * ts).contiguous()
        m = tr.find_visited_cells(nv, out["visited_cells"], out["barycentric_coordinates"], out["hit_distances"], out["vertex_indices"], dist)
        vi, bc, mask = m["vertex_indices"], m["barycentric_coordinates"], m["mask"]
        n = R * S
        G = torch.randn(n, 64, device=dev)
        gb = torch.randn(R, S, 3, device=dev)
        vil = vi.reshape(-1, 4).long()
        present = (vil >= 0)

        def a_kernel():
            return cpp.interpolate_values_backward_barycentrics(vi, field, G)

        def a_torch():
            rows = field_vm[vil.clamp_min(0)] * present[..., None]
            return torch.einsum("nc,nkc->nk", G, rows[:, 1:] - rows[:, :1])

        # (B): the yardstick works on the matched samples, compacted beforehand
        sel = mask.reshape(-1).nonzero()[:, 0]
        ray_of = sel // S
        vi_m, bc_m, gb_m, t_m = vil[sel], bc.reshape(-1, 3)[sel], gb.reshape(-1, 3)[sel], dist.reshape(-1)[sel]

        def b_kernel():
            return cpp.sample_positions_backward(vi, bc, gb, table, dist, want_origins=True, want_directions=True, want_vertices=True)

        def b_torch():
            tv = table[vi_m].requires_grad_(True)                                   # [n, 4, 3]
            p = torch.zeros(len(sel), 3, device=dev, requires_grad=True)
            tn.add_barycentrics_grad(bc_m, tv, p).backward(gb_m)
            gv = torch.zeros(V, 3, device=dev).index_add_(0, vi_m.reshape(-1), tv.grad.reshape(-1, 3))
            go = torch.zeros(R, 3, device=dev).index_add_(0, ray_of, p.grad)
            gd = torch.zeros(R, 3, device=dev).index_add_(0, ray_of, t_m[:, None] * p.grad)
            return go, gd, gv

        # the two sides compute the same thing (to fp32 round-off, relative to the largest entry)
        ka, ta = a_kernel().reshape(-1, 3), a_torch()
        kb, tb = b_kernel(), b_torch()
        agree = [float((ka - ta).abs().max() / ta.abs().max())] + [float((x - y).abs().max() / y.abs().max()) for x, y in zip(kb[1:], tb)]
        (ma, mt, mb, mbt), spread = interleaved([a_kernel, a_torch, b_kernel, b_torch], args.rounds)
        a_bytes = n * (5 * 4 * 64 + 4 * 3)
        lines += [
            f"{R} x {S} = {n} samples ({len(sel)} matched); kernel vs composition, max relative difference (A, origins, directions, vertices): "
            + ", ".join(f"{x:.2e}" for x in agree),
            f"  (A) kernel {ma * 1e3:8.1f} us ({spread[0][0] * 1e3:.1f} .. {spread[0][1] * 1e3:.1f})   PyTorch gather + einsum {mt * 1e3:9.1f} us "
            f"({spread[1][0] * 1e3:.1f} .. {spread[1][1] * 1e3:.1f})   ratio {mt / ma:6.1f}x   algorithmic {a_bytes / 1e6:.1f} MB -> {a_bytes / (ma * 1e-3) / 1e12:.2f} TB/s",
            f"  (B) kernel {mb * 1e3:8.1f} us ({spread[2][0] * 1e3:.1f} .. {spread[2][1] * 1e3:.1f})   gather + add_barycentrics_grad + index_add_ {mbt * 1e3:9.1f} us "
            f"({spread[3][0] * 1e3:.1f} .. {spread[3][1] * 1e3:.1f})   ratio {mbt / mb:6.1f}x",
        ]
        print("\n".join(lines[-3:]), flush=True)

    # one training iteration, switch on against off (parent = off)
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(dev)
    f2 = ((torch.rand(64, V, device=dev) * 2 - 1) * 1e-4)
    f2[1:4] = torch.rand(3, V, device=dev) * 2 - 1
    f2.requires_grad_(True)
    opt = torch.optim.SGD([f2] + list(mlp.parameters()), lr=1e-3)
    rd = render.TetraRenderer(tr, f2, mlp, 256, M, fused=True, num_fine_samples=256)
    target = torch.rand(R, 3, device=dev)
    o_g, d_g, v_g = o.clone().requires_grad_(True), d.clone().requires_grad_(True), table.clone().requires_grad_(True)

    def step(on):
        opt.zero_grad(set_to_none=True)
        o_g.grad = d_g.grad = v_g.grad = None
        if on:
            res = rd.render_train(o_g, d_g, position_gradients=True, vertices=v_g)
        else:
            res = rd.render_train(o, d)
        ((res["rgb"] - target) ** 2).mean().backward()
        opt.step()

    (m_off, m_on), spread = interleaved([lambda: step(False), lambda: step(True)], args.rounds)
    lines.append(f"render_train iteration (4096 rays, 256 coarse + 513 fine samples, trace + forward + backward + SGD): "
                 f"off {m_off:.2f} ms ({spread[0][0]:.2f} .. {spread[0][1]:.2f}), position_gradients on {m_on:.2f} ms "
                 f"({spread[1][0]:.2f} .. {spread[1][1]:.2f}): +{(m_on / m_off - 1) * 100:.1f} %")
    print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
