"""Ray binning (option "bin_rays" / TN_TRACE_BIN_RAYS) measured in one process: flag off / flag on / HOST-presorted rays with
the flag off, interleaved, medians over fresh allocations of the output rows (torch.cuda.empty_cache() between them: new
physical pages, cf. r06t_alloc_sweep.py).  The presorted line is the ceiling -- the same walk order without key kernel,
sort and indirection; the parts come from bench.trace_breakdown (option "timing": kernels serialised, so they do not add
up to the overlapped call).

    python profiles/bin_rays_sweep.py sweep  ALLOCS WORKLOAD ...     workloads: C5 C4-1M C4-64k C4-64k-compact C2-frame
    python profiles/bin_rays_sweep.py default:LABEL ALLOCS WORKLOAD ...   flag off only, no option touched: the regression
                                                                     check against the parent commit -- run from a checkout
                                                                     of each, in alternating processes
"""
import importlib
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402

tn = importlib.import_module("tetra-nerf_amd")
scenes = importlib.import_module("tetra-nerf_amd.scenes")
dev = torch.device("cuda:0")

MESHES = {"C2": (15000, 0), "C4": (45000, 2), "C5": (150000, 3)}
# workload -> (mesh, rays, compact rows)
WORKLOADS = {
    "C5": ("C5", lambda: scenes.outside_in_rays(1 << 20, 4), False),
    "C4-1M": ("C4", lambda: scenes.outside_in_rays(1 << 20, 4), False),
    "C4-64k": ("C4", lambda: scenes.outside_in_rays(65536, 4), False),
    "C4-64k-compact": ("C4", lambda: scenes.outside_in_rays(65536, 4), True),
    "C2-frame": ("C2", lambda: bench.frame_rays(scenes, 0, 800, 800), False),
}
M = 512
_mesh_cache = {}


def tracer_for(mesh):
    if mesh not in _mesh_cache:
        _mesh_cache.clear()                      # one mesh resident at a time
        pts, cells = scenes.random_mesh(*MESHES[mesh])
        tr = tn.TetrahedraTracer(dev)
        tr.load_tetrahedra(torch.from_numpy(pts).to(dev), torch.from_numpy(cells).to(dev))
        _mesh_cache[mesh] = (tr, pts, cells)
    return _mesh_cache[mesh]


def timed(tr, o, d, calls=3):
    tr.trace_rays(o, d, M)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        tr.trace_rays(o, d, M)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def sweep(allocs, name):
    ray_order = importlib.import_module("tetra-nerf_amd.ray_order")
    mesh, rays, compact = WORKLOADS[name]
    tr, pts, cells = tracer_for(mesh)
    o, d = rays()
    used = pts[np.unique(cells)]
    order = np.argsort(ray_order.ray_keys(o, d, used.min(0), used.max(0)), kind="stable")
    given = tuple(torch.from_numpy(x).to(dev) for x in (o, d))
    sorted_ = tuple(torch.from_numpy(np.ascontiguousarray(x[order])).to(dev) for x in (o, d))
    variants = (("off", 0, given), ("on", 1, given), ("presorted", 0, sorted_))
    tr.set_option("dense_tails", 0 if compact else 1)
    print(f"== {name}: {len(cells)} tets, {len(o)} rays, M = {M}{', compact rows' if compact else ''}; "
          f"ms per call (median of 5 x 3 calls) per fresh allocation", flush=True)
    tot = {n: [] for n, _, _ in variants}
    for a in range(allocs):
        torch.cuda.empty_cache()
        res = {n: [] for n, _, _ in variants}
        for _ in range(5):
            for n, flag, (vo, vd) in variants:
                tr.set_option("bin_rays", flag)
                res[n].append(timed(tr, vo, vd))
        for n in res:
            tot[n].append(statistics.median(res[n]))
        print(f"alloc {a}: " + "  ".join(f"{n} {tot[n][-1]:.3f}" for n in res), flush=True)
    med = {n: statistics.median(v) for n, v in tot.items()}
    print("median: " + "  ".join(f"{n} {v:.3f} ({100 * (v / med['off'] - 1):+.1f} %)" for n, v in med.items()))
    for n, flag, (vo, vd) in variants:            # serialised parts of one call each
        tr.set_option("bin_rays", flag)
        bd = bench.trace_breakdown(tr, vo, vd, M)
        print(f"parts {n:9s}: " + "  ".join(f"{k} {v:.3f}" for k, v in bd.items()), flush=True)
    tr.set_option("bin_rays", 0)
    tr.set_option("dense_tails", 1)


def default(allocs, name):
    mesh, rays, compact = WORKLOADS[name]
    assert not compact
    tr, _, cells = tracer_for(mesh)
    o, d = (torch.from_numpy(x).to(dev) for x in rays())
    meds = []
    for _ in range(allocs):
        torch.cuda.empty_cache()
        meds.append(statistics.median(timed(tr, o, d) for _ in range(5)))
    print(f"default {name} ({len(cells)} tets, {len(o)} rays) build {LABEL}: "
          + " ".join(f"{m:.3f}" for m in meds) + f"  median {statistics.median(meds):.3f} ms", flush=True)


if __name__ == "__main__":
    (mode, _, LABEL), allocs = sys.argv[1].partition(":"), int(sys.argv[2])
    for w in sys.argv[3:]:
        {"sweep": sweep, "default": default}[mode](allocs, w)
