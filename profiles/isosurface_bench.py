"""What the isosurface extraction costs (tn_isosurface_count, tn_isosurface_emit, cpp.isosurface), against the same statement
written in torch on the same GPU tensors: what a user would otherwise write.

    python profiles/isosurface_bench.py [--rounds 7] [--out profiles/isosurface_bench.txt]
    python profiles/isosurface_bench.py --kernels    7 x (count, emit) per mesh and nothing else timed: for
                                                     rocprofv3 --kernel-trace --stats -- python ... --kernels, a run of its own

One process, the candidates interleaved, medians (min .. max) over the rounds after a warm-up, on bench.py's three meshes (about
100k / 300k / 1M tetrahedra).  The field is cos(4 pi x) + cos(4 pi y) + cos(4 pi z), the level found by bisection so that about
a tenth of the tetrahedra cross it.
  count    tn_isosurface_count alone, 20 back-to-back calls between two device events
  emit     tn_isosurface_emit alone on the count's arrays and totals, outputs allocated once, the same way
  call     cpp.isosurface: both entries, the allocations and the two read-backs, by the wall clock with a synchronise either side
  torch    the same statement in torch on the GPU tensors (torch.unique on the 64-bit keys, about three dozen launches), the same
           way; its arrays are compared with the kernels' once
Needs the GPU; there is no fallback.

Expected before any run.  The COUNT pass requests 16 B of cells and four 4-byte value gathers per tetrahedron and writes 8 B; it
has no arithmetic to speak of and no atomics, so it should sit beside k_remap and k_delaunay_faces (profiles/delaunay_bench.txt:
4 .. 31 us at these sizes), at 10 .. 30 us, plus its two scans.  EMIT should be the radix sort on num_refs 64-bit keys (num_refs is
about 0.35 T at a tenth of the tetrahedra crossing): its other kernels each pass once over T tetrahedra or over num_refs
references."""
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
REPS = 20       # calls per timed window of the device-side candidates


def med(ts):
    return f"{statistics.median(ts):.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def event_ms(fn, reps=REPS):
    fn(); fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps


def interleaved(fns, rounds, warm=1):
    for _ in range(warm):
        for f, _ in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, (f, timer) in enumerate(fns):
            ts[k].append(timer(f))
    return ts


def torch_statement(geometry, xyz, cells, values, level):
    """geometry.isosurface_statement in torch on the device of its arguments (no mask, every id valid)"""
    dev = values.device
    table = torch.tensor(geometry.ISO_TRI_TABLE, device=dev)
    ec = torch.tensor(geometry.ISO_EDGE_CORNERS, device=dev)
    level = torch.tensor(level, dtype=torch.float32, device=dev)
    c = cells.long()
    v = values[c]
    ok = (v.abs() < geometry.ISO_VALUE_LIMIT).all(1)
    code = torch.where(ok, ((v >= level) * torch.tensor([1, 2, 4, 8], device=dev)).sum(1), 0)
    ntri = (table[code][:, :, 0] >= 0).sum(1)
    cross = (((code[:, None] >> ec[None, :, 0]) ^ (code[:, None] >> ec[None, :, 1])) & 1).bool()
    tri_offsets = torch.cat([ntri.new_zeros(1), ntri.cumsum(0)])
    ref_offsets = torch.cat([ntri.new_zeros(1), cross.sum(1).cumsum(0)])
    tt, ee = cross.nonzero(as_tuple=True)
    u, w = c[tt, ec[ee, 0]], c[tt, ec[ee, 1]]
    ukey, slot_id = torch.unique(torch.minimum(u, w) << 32 | torch.maximum(u, w), return_inverse=True)
    a, b = ukey >> 32, ukey & 0xFFFFFFFF
    t = (level - values[a]) / (values[b] - values[a])
    positions = xyz[a] + t[:, None] * (xyz[b] - xyz[a])
    rank = cross.long().cumsum(1) - cross.long()
    negative = geometry._vol6(xyz.double()[c]) < 0
    M = int(tri_offsets[-1])
    triangles = torch.zeros((M, 3), dtype=torch.int64, device=dev)
    triangle_tets = torch.zeros(M, dtype=torch.int64, device=dev)
    for row in (0, 1):
        tets = (ntri > row).nonzero()[:, 0]
        edges = table[code[tets], row]
        edges = torch.where(negative[tets, None], edges[:, [0, 2, 1]], edges)
        slots = ref_offsets[tets][:, None] + rank[tets[:, None], edges]
        triangles[tri_offsets[tets] + row] = slot_id[slots]
        triangle_tets[tri_offsets[tets] + row] = tets
    return {"positions": positions, "triangles": triangles.int(), "triangle_tets": triangle_tets.int(),
            "edge_vertices": torch.stack([a, b], 1).int(), "edge_t": t}


def field_of(pts):
    """cos(4 pi x) + cos(4 pi y) + cos(4 pi z) in float32: level sets of about 4.7 units of area per unit volume at level 0 (a
    sphere inside the unit cube has at most 3.1, which the million-tetrahedron mesh would cross with 6 % of its cells)"""
    return np.cos(4 * np.pi * pts.astype(np.float64)).sum(1).astype(np.float32)


def level_for(values, cells, fraction):
    """the level in [0, 3) that `fraction` of the tetrahedra cross, by bisection (the surface shrinks as the level rises); 0 where
    even that one crosses fewer"""
    v = values[cells]

    def crossing(level):
        inside = v >= np.float32(level)
        return float((inside.any(1) & ~inside.all(1)).mean())

    lo, hi = 0.0, 3.0
    if crossing(lo) <= fraction:
        return lo, crossing(lo)
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if crossing(mid) > fraction else (lo, mid)
    level = float(np.float32(lo))
    return level, crossing(level)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "isosurface_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="C2,C4,C5")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    tn = importlib.import_module("tetra-nerf_amd")
    scenes = importlib.import_module("tetra-nerf_amd.scenes")
    geometry = importlib.import_module("tetra-nerf_amd.geometry")
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"isosurface_bench: {torch.cuda.get_device_name(0)}, medians of {args.rounds} interleaved rounds (min .. max), one process")
    m = statistics.median
    for name, points, seed in SIZES:
        if name not in args.sizes.split(","):
            continue
        pts, cells = scenes.random_mesh(points, seed)
        values = field_of(pts)
        level, crossing = level_for(values, cells, 0.1)
        x, c, v = torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev), torch.from_numpy(values).to(dev)
        V, T = len(pts), len(cells)
        stream = torch.cuda.current_stream().cuda_stream
        offsets = torch.empty((2, T + 1), dtype=torch.int32, device=dev)

        def count():
            assert lib.tn_isosurface_count(V, T, c.data_ptr(), v.data_ptr(), level, None, offsets[0].data_ptr(), offsets[1].data_ptr(), stream) == 0

        count()
        M, R = offsets[:, T].tolist()
        tris, tets = torch.empty((M, 3), dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
        ev, et = torch.empty((R, 2), dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
        pos, n = torch.empty((R, 3), dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)

        def emit():
            assert lib.tn_isosurface_emit(V, T, x.data_ptr(), c.data_ptr(), v.data_ptr(), level, None, offsets[0].data_ptr(), offsets[1].data_ptr(),
                                          M, R, tris.data_ptr(), tets.data_ptr(), ev.data_ptr(), et.data_ptr(), pos.data_ptr(), n.data_ptr(),
                                          stream) == 0

        if args.kernels:
            for _ in range(args.rounds):
                count()
                emit()
            torch.cuda.synchronize()
            say(f"kernels: {args.rounds} x (count, emit) at {T} tets, {R} edge references, {M} triangles done")
            continue
        got = tn.cpp.isosurface(x, c, v, level)
        want = torch_statement(geometry, x, c, v, level)
        same = all(got[k].shape == want[k].shape and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in want)
        N = len(got["positions"])
        t_count, t_emit, t_call, t_torch = interleaved(
            [(count, event_ms), (emit, event_ms), (lambda: tn.cpp.isosurface(x, c, v, level), wall_ms),
             (lambda: torch_statement(geometry, x, c, v, level), wall_ms)], args.rounds)
        say(f"{name} {T} tets, {V} vertices, level {level:.6f}: {crossing:.1%} of the tetrahedra cross, {M} triangles, {R} edge references, "
            f"{N} welded vertices (kernels {'==' if same else '!='} the torch statement on the GPU, byte for byte):")
        say(f"  count    {med(t_count)} = {(28 * T + 8) / 1e6:.1f} MB of cells, gathers and counts, then two scans over {T + 1} words")
        say(f"  emit     {med(t_emit)} for {R} keys of {32 + max(V - 1, 1).bit_length()} sorted bits")
        say(f"  call     cpp.isosurface with its allocations and two read-backs {med(t_call)} = {m(t_call) / (m(t_count) + m(t_emit)):.1f} x "
            f"(count + emit)")
        say(f"  torch    the statement in torch on the GPU tensors {med(t_torch)} = {m(t_torch) / m(t_call):.1f} x the call")


if __name__ == "__main__":
    main()
