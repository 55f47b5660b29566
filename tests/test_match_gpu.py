"""GPU tests of the matcher (rayops::ray_match, csrc/tn_ray_ops.h -- the ONE per-ray function behind find_visited_cells and
behind the matcher phases of the persistent render kernel) on CRAFTED trace rows: rays of up to 2048 segments, so that the
second staging pass of the segment bounds (rays with more than 512 segments) runs, which no mesh of this suite reaches
(reference: find_matched_cells_kernel, src/tetrahedra_tracer.cu:115-160, restated by the oracle)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")
V = 5000                                             # vertex ids of the crafted rows lie below this
COUNTS_1024 = (0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024)
SAMPLES = (1, 2, 255, 256, 257, 321, 577)            # both sides of the UM switch (256), partial last groups, no ascending loop


def crafted_rows(counts, M, seed):
    """Dense trace rows [R, M, ...] of rays with counts[r] ascending, abutting segments (t_out[k] = t_in[k + 1]), random cell and
    vertex ids and random barycentrics; slots beyond the count hold the dense defaults (0xFFFFFFFF / 0)."""
    rng = np.random.default_rng(seed)
    R = len(counts)
    rows = {"num_visited_cells": np.asarray(counts, np.int32),
            "visited_cells": np.full((R, M), -1, np.int32),
            "barycentric_coordinates": np.zeros((R, M, 2, 3), np.float32),
            "hit_distances": np.zeros((R, M, 2), np.float32),
            "vertex_indices": np.full((R, M, 4), -1, np.int32)}
    for r, n in enumerate(counts):
        b = np.cumsum(np.concatenate([[0.5 + rng.random()], 0.002 + 0.01 * rng.random(n)]).astype(np.float32), dtype=np.float32)
        rows["hit_distances"][r, :n, 0] = b[:-1]
        rows["hit_distances"][r, :n, 1] = b[1:]
        rows["visited_cells"][r, :n] = rng.integers(0, 4 * V, n)
        rows["vertex_indices"][r, :n] = rng.integers(0, V, (n, 4))
        rows["barycentric_coordinates"][r, :n] = rng.random((n, 2, 3), dtype=np.float32)
    return rows


def sorted_distances(rows, S, seed):
    """[R, S] ascending random distances reaching a little beyond both ends of every ray's segments."""
    rng = np.random.default_rng(seed)
    nv, hd = rows["num_visited_cells"], rows["hit_distances"]
    near = hd[:, 0, 0]
    far = hd[np.arange(len(nv)), np.maximum(nv - 1, 0), 1]
    far = np.where(nv > 0, far, near + 1.0)
    u = np.sort(rng.random((len(nv), S)), axis=-1) * 1.2 - 0.1
    return np.ascontiguousarray((near[:, None] + u * (far - near)[:, None]).astype(np.float32))


def match_cases(M):
    """(rows, {S: distances}) of test 1: one ray per segment count with sorted distances, then three more rays -- M = 1024: of
    513 / 1023 / 1024 segments, M = 2048: of 2048 / 1025 / 2048 -- with a descending row (literal branch across the 512
    boundary), a row with one inversion, and a row with every sample exactly on the boundary between segments 599 and 600."""
    counts = COUNTS_1024 + (513, 1023, 1024) if M == 1024 else (1025, 2048, 2048, 1025, 2048)
    rows = crafted_rows(counts, M, seed=M)
    dists = {}
    for S in SAMPLES:
        s = sorted_distances(rows, S, seed=1000 + S)
        s[-3] = s[-3, ::-1]                          # descending
        if S > 2:
            s[-2, S // 2] = s[-2, 0]                 # one inversion
        s[-1] = rows["hit_distances"][len(counts) - 1, 600, 0]
        dists[S] = np.ascontiguousarray(s)
    return rows, dists


@pytest.fixture(scope="module")
def cube_tracer(tn, device, scenes):
    import torch

    pts, cells = scenes.cube_mesh()
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    return tr


def _to_device(rows, device):
    import torch

    return [torch.from_numpy(rows[k]).to(device) for k in KEYS]


def _assert_equals_oracle(got, want, msg):
    for k in ("mask", "cell_indices", "vertex_indices"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{msg} {k}")
    np.testing.assert_array_equal(got["barycentric_coordinates"].view(np.uint32), want["barycentric_coordinates"].view(np.uint32),
                                  err_msg=msg)


@pytest.mark.parametrize("M", [1024, 2048])
def test_find_visited_cells_on_long_rows_equals_the_oracle(tn, device, oracle, cube_tracer, monkeypatch, M):
    """Rays of 0 ... M segments x 1 ... 577 samples: mask, cell and vertex ids equal to the oracle's, barycentrics equal in
    bits (the bar of test_trace_gpu.py::test_find_visited_cells_edge_cases); then a permuted subset of the rays through
    `ray_index` with a device-side `count` below its length: the rows beyond `count` stay as they were allocated."""
    import torch

    rows, dists = match_cases(M)
    lists = _to_device(rows, device)
    R = len(rows["num_visited_cells"])
    perm = np.random.default_rng(3).permutation(R)[: R - 2].astype(np.int32)
    keep = len(perm) - 3
    monkeypatch.setattr(tn.cpp, "_POISON", True)     # outputs pre-filled with NaN / 0x7f7f7f7f / True
    for S, s in dists.items():
        want = oracle.find_visited_cells(*[rows[k] for k in KEYS], s)
        if S > 2:                                    # not vacuous: the sorted rows of the long rays are mostly matched
            assert want["mask"][: R - 3][rows["num_visited_cells"][: R - 3] > 512].mean() > 0.5
        got = {k: v.cpu().numpy() for k, v in cube_tracer.find_visited_cells(*lists, torch.from_numpy(s).to(device)).items()}
        _assert_equals_oracle(got, want, f"M={M} S={S}")
        # a subset, in another order, sized on the device
        want_p = oracle.find_visited_cells(*[rows[k][perm[:keep]] for k in KEYS], s[perm[:keep]])
        got_p = cube_tracer.find_visited_cells(*lists, torch.from_numpy(np.ascontiguousarray(s[perm])).to(device),
                                               ray_index=torch.from_numpy(perm).to(device),
                                               count=torch.tensor([keep], dtype=torch.int32, device=device))
        got_p = {k: v.cpu().numpy() for k, v in got_p.items()}
        _assert_equals_oracle({k: v[:keep] for k, v in got_p.items()}, want_p, f"M={M} S={S} ray_index")
        assert got_p["mask"][keep:].all(), (M, S)
        assert (got_p["cell_indices"][keep:] == 0x7F7F7F7F).all() and (got_p["vertex_indices"][keep:] == 0x7F7F7F7F).all(), (M, S)
        assert np.isnan(got_p["barycentric_coordinates"][keep:]).all(), (M, S)


class RowsTracer:
    """A tracer whose trace_rays returns crafted rows; find_visited_cells is a real tracer's (it takes the rows as they are)."""

    def __init__(self, real, rows):
        self.real, self.rows = real, rows

    def trace_rays(self, origins, directions, max_ray_triangles):
        assert max_ray_triangles == self.rows["visited_cells"].shape[1] and origins.shape[0] == self.rows["visited_cells"].shape[0]
        return self.rows

    def find_visited_cells(self, *a, **kw):
        return self.real.find_visited_cells(*a, **kw)


def render_case(tn, device, cube_tracer, S, S_fine, M, mode, copies=24):
    """The one-launch render and the kernel chain of `copies` rays per segment count (several rays per block of the persistent
    kernel): ({"rgb", "accumulation", "depth"} of each)."""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    counts = (tuple(n for n in COUNTS_1024 if n >= 1) if M == 1024 else (1025, 2048)) * copies
    rows = crafted_rows(counts, M, seed=7 * M + S)
    tracer = RowsTracer(cube_tracer, {k: torch.from_numpy(rows[k]).to(device) for k in KEYS})
    torch.manual_seed(11)
    mlp = render.TetraMLP().to(device)
    field = torch.randn(64, V, device=device) * 0.5
    d = torch.nn.functional.normalize(torch.randn(len(counts), 3, device=device), dim=-1)
    o = torch.zeros_like(d)
    kw = dict(fused=True, num_fine_samples=S_fine, mlp_mode=mode)
    one = render.TetraRenderer(tracer, field, mlp, S, M, fused_pass=True, **kw)
    chain = render.TetraRenderer(tracer, field, mlp, S, M, fused_pass=False, **kw)
    assert one._one_launch_ok(mode) and not chain._one_launch_ok(mode)
    return one.render(o, d), chain.render(o, d)


RENDER_CASES = [(64, 0, 1024, "fp32"), (64, 37, 1024, "fp32"), (100, 200, 1024, "fp32"), (64, 37, 2048, "fp32"),
                (64, 37, 1024, "bf16x3")]


@pytest.mark.parametrize("S,S_fine,M,mode", RENDER_CASES)
def test_one_launch_render_on_long_rows_is_bit_identical_to_the_kernel_chain(tn, device, cube_tracer, S, S_fine, M, mode):
    """The matcher phases of tn_render_rays against find_visited_cells inside the kernel chain on rays of up to M segments
    (the third case has 301 final samples: the render kernel's larger sample group)."""
    import torch

    a, b = render_case(tn, device, cube_tracer, S, S_fine, M, mode)
    assert bool(a["ray_mask"].all()) and torch.equal(a["ray_mask"], b["ray_mask"])
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (k, float((a[k] - b[k]).abs().max()))
    assert bool(torch.isfinite(a["rgb"]).all()) and float(a["accumulation"].max()) > 0.05
