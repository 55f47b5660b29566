"""Inputs, float64 references and error measures of the occupancy-guided sampler tests: tests/test_live_sampler.py (CPU: the
statements of render.py alone) and tests/test_live_sampler_gpu.py (tn_sample_live / tn_live_to_distance) draw the SAME tensors
from here.  The rows are ray_stage_lib.coarse_rows -- M = 256; 0, 1, 2, 63, 64, 65, 129, 255 and 256 segments, six rays each,
contiguous segments, a zero-length and a backward segment per ray of four segments or more -- once per LIVENESS PATTERN, with a
cell id per segment and an occupancy [T] that realises the pattern at THRESHOLD."""
import functools
import importlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
render = importlib.import_module("tetra-nerf_amd.render")

import ray_stage_lib as lib  # noqa: E402

M = lib.COARSE_M
THRESHOLD = 0.5
PATTERNS = ("all live", "all culled", "alternating", "middle run", "ends culled", "invalid id", "nan occupancy")
S_VALUES = lib.COARSE_S                                   # 1, 63, 64, 65, 200
# values per ray of tn_live_to_distance: the kernel walks groups of 256 values (4 per lane), so 255 / 256 / 257 are the edges of
# one group and 513 takes three; 63 / 64 / 65: the edges of one lane-chunk
N_VALUES = (1, 63, 64, 65, 200, 255, 256, 257, 513)
FLOOR = lib.FLOOR


def _culled_segments(pattern, nv):
    """bool [nv]: the segments whose cell lies below the threshold.  "ends culled" culls segment 0 and segment nv - 1 from three
    segments on; with two it culls the first only and with one nothing (a ray keeps a live segment in every pattern but
    "all culled")."""
    k = torch.arange(nv)
    if pattern == "all live":
        return torch.zeros(nv, dtype=torch.bool)
    if pattern == "alternating":
        return k % 2 == 1
    if pattern == "middle run":
        lo = nv // 3
        hi = max(lo + 1, 2 * nv // 3)
        return ~((k >= lo) & (k < hi))
    if pattern == "ends culled":
        return ((k == 0) & (nv >= 2)) | ((k == nv - 1) & (nv >= 3))
    return torch.ones(nv, dtype=torch.bool)       # all culled; invalid id / nan occupancy: culled but for their live segments


@functools.lru_cache(maxsize=None)
def _live_rows(seed):
    base = lib.coarse_rows(seed)
    R0 = len(base["num_visited"])
    nv_all, hd_all, cells_all, pat_all, occ = [], [], [], [], []
    for p, pattern in enumerate(PATTERNS):
        for r in range(R0):
            nv = int(base["num_visited"][r])
            cells = torch.full((M,), -1, dtype=torch.int32)
            culled = _culled_segments(pattern, nv)
            first = len(occ)
            cells[:nv] = torch.arange(first, first + nv, dtype=torch.int32)
            occ += [0.0 if c else 1.0 for c in culled.tolist()]
            if nv and pattern == "invalid id":
                cells[nv // 2] = -1                      # unmatched
                cells[0] = 0x7FFFFF00                    # >= T  (nv == 1: this one)
            if nv and pattern == "nan occupancy":
                for k in range(nv // 4, min(nv // 4 + 2, nv)):
                    occ[first + k] = float("nan")
            nv_all.append(nv); hd_all.append(base["hit_distances"][r]); cells_all.append(cells); pat_all.append(p)
    occ += [0.0] * 3                                      # (cells nothing refers to)
    return {"num_visited": torch.tensor(nv_all, dtype=torch.int32), "hit_distances": torch.stack(hd_all).contiguous(),
            "visited_cells": torch.stack(cells_all).contiguous(), "occupancy": torch.tensor(occ, dtype=torch.float32),
            "pattern": torch.tensor(pat_all), "zero_slot": base["zero_slot"].repeat(len(PATTERNS)),
            "neg_slot": base["neg_slot"].repeat(len(PATTERNS))}


def live_rows(seed=0):
    """num_visited i32 [378], hit_distances f32 [378,256,2], visited_cells i32 [378,256] (-1 behind the last segment), occupancy f32
    [T], pattern [378] (index into PATTERNS), zero_slot / neg_slot [378]: 54 rays per pattern."""
    return dict(_live_rows(seed))


def contiguous(rows):
    """The same rows with every exit distance but the last set to the NEXT entry distance, bit for bit (coarse_rows' segments are
    contiguous up to the fp32 rounding of t_in + length; its backward segment becomes a zero-length one): with every segment live
    the live-length coordinate of such a row IS the distance."""
    hd = rows["hit_distances"].clone()
    inner = torch.arange(M - 1, device=hd.device)[None] < (rows["num_visited"].long()[:, None] - 1)
    hd[:, :-1, 1] = torch.where(inner, hd[:, 1:, 0], hd[:, :-1, 1])
    return dict(rows, hit_distances=hd.contiguous())


def draws(n, seed=0):
    """U[0,1) [378, n]"""
    g = torch.Generator().manual_seed(17 * n + seed)
    return torch.rand(len(PATTERNS) * len(lib.COARSE_NV) * lib.COARSE_RAYS_PER_NV, n, generator=g)


def live_statement(rows, dtype, threshold=THRESHOLD):
    """render.live_lengths_statement in `dtype`, on the device the rows are on"""
    return render.live_lengths_statement(rows["num_visited"], rows["visited_cells"], rows["hit_distances"].to(dtype), rows["occupancy"],
                                         threshold)


def values_in_span(live, u):
    """live-length values [r, n] from draws u [r, n] in [0, 1): near + u L, the first at near and the last at near + L exactly"""
    s = live["near"] + u.to(live["near"].dtype) * live["length"]
    s[:, 0] = live["near"][:, 0]
    s[:, -1] = (live["near"] + live["length"])[:, 0]
    return s.sort(dim=1).values


def forward_map64(live64, slot, t):
    """The forward map in float64: the live length before distance t of segment `slot` -- cum[slot] + clamp(t - t_in, 0, w)."""
    hd = live64["hit_distances"]
    slot = slot.long()
    t_in = torch.gather(hd[..., 0], 1, slot)
    w = torch.gather(live64["w"], 1, slot)
    return torch.gather(live64["cum"], 1, slot) + torch.minimum((t.double() - t_in).clamp_min(0), w)


def edge_error(got, want64, live64):
    """Per ray: max |edges - want| / (L + |near + L|) -- ray_stage_lib.coarse_error with L for far - near."""
    L, far = live64["length"][:, 0], (live64["near"] + live64["length"])[:, 0]
    return (got.double() - want64).abs().max(-1).values / (L.abs() + far.abs())


def far_of(rows):
    """[r] last exit distance (1 for the rows without a segment)"""
    return lib.coarse_near_far({"num_visited": rows["num_visited"], "hit_distances": rows["hit_distances"]})[1]


def to_device(d, device):
    return lib.to_device(d, device)
