"""Opt-in ray binning of trace_rays (TN_TRACE_BIN_RAYS / trace_rays(bin_rays=True) / option "bin_rays"): the library walks
the rays in the order of their keys (tetra-nerf_amd/ray_order.py) and writes every row at the caller's index, so the five
output arrays of a binned call are those of an unbinned call BIT FOR BIT, every tail byte included, and the statistics of
the two calls are the same numbers.  Every comparison is on raw bits (`view(int32)`)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("num_visited_cells", "visited_cells", "vertex_indices", "hit_distances", "barycentric_coordinates")
ROW_KEYS = KEYS[1:]


def _tracer(tn, device, pts, cells, walk=2, **opts):
    import torch

    tr = tn.TetrahedraTracer(device)
    tr.set_option("walk", walk)
    for k, v in opts.items():
        tr.set_option(k, v)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    return tr


def _oracle(oracle, pts, cells):
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(pts, cells)
    return ot


def _dev(device, *arrays):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def _numbers(tr):
    """everything the library reports about the last call"""
    return {"stats": tr.trace_stats(), "reasons": tr.flag_reasons(), "cross_check": tr.cross_check()}


def _assert_same_rows(a, b, ctx):
    import torch

    for k in KEYS:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            diff = (a[k].view(torch.int32) != b[k].view(torch.int32)).reshape(len(a[k]), -1).any(1)
            raise AssertionError(f"{ctx}: {k} of the binned call differs on {int(diff.sum())} rays "
                                 f"(first: ray {int(diff.nonzero()[0, 0])})")


def _both(tr, to, td, M, ctx, **kw):
    """unbinned, then binned; rows and reported numbers must be the same.  Returns (binned rows, numbers, order)."""
    plain = tr.trace_rays(to, td, M, **kw)
    n_plain = _numbers(tr)
    assert len(tr.ray_order()) == 0, ctx
    binned = tr.trace_rays(to, td, M, bin_rays=True, **kw)
    n_binned = _numbers(tr)
    order = tr.ray_order()
    assert n_plain == n_binned, (ctx, n_plain, n_binned)
    if not kw.get("compact_rows"):
        _assert_same_rows(plain, binned, ctx)
    return plain, binned, n_binned, order


def _against_oracle(out, ot, o, d, M, rows, ctx):
    import torch

    rows = np.asarray(rows)
    want = ot.trace_rays(np.ascontiguousarray(o[rows]), np.ascontiguousarray(d[rows]), M)
    tsel = torch.from_numpy(rows).to(out[KEYS[0]].device)
    for k in KEYS:
        g = out[k].index_select(0, tsel).cpu().numpy()
        w = np.ascontiguousarray(want[k])
        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(rows), -1).any(1))[0]
            raise AssertionError(f"{ctx}: {k} differs from the oracle on {len(bad)} rays (first: ray {rows[bad[0]]})")


def _mesh_box(pts, cells):
    used = pts[np.unique(cells)]
    return used.min(0), used.max(0)


def _assert_order(order, o, d, pts, cells, ctx):
    ray_order = importlib.import_module("tetra-nerf_amd.ray_order")
    R = len(o)
    assert order.dtype == np.int64 and order.shape == (R,), (ctx, order.shape)
    assert np.array_equal(np.sort(order), np.arange(R)), f"{ctx}: ray_order() is not a permutation"
    lo, hi = _mesh_box(pts, cells)
    want = np.argsort(ray_order.ray_keys(o, d, lo, hi), kind="stable")
    if not np.array_equal(order, want):
        raise AssertionError(f"{ctx}: ray_order() differs from argsort(ray_keys) at {int((order != want).sum())} of {R} positions")


def _shuffled(seed, *sets):
    o = np.concatenate([s[0] for s in sets], 0)
    d = np.concatenate([s[1] for s in sets], 0)
    perm = np.random.default_rng(seed).permutation(len(o))
    return np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm])


# ---------------------------------------------------------------------------------------------------- 1
def test_c4_mixed_incoherent_rays(tn, device, oracle, scenes):
    """300k tets, 98,304 outside-in + 32,768 inside-out rays shuffled: binned == unbinned on every byte, both == the CPU oracle
    on 16,384 rows, the walked order is argsort(ray_keys), and the library reports the same numbers for both calls."""
    pts, cells = scenes.random_mesh(45000, 2)
    print(f"C4: {len(cells)} tets, mesh sha256 {scenes.mesh_sha256(pts, cells)}")
    o, d = _shuffled(11, scenes.outside_in_rays(98304, 4), scenes.inside_out_rays(32768, 2))
    R, M = len(o), 512
    tr = _tracer(tn, device, pts, cells, walk=1)
    to, td = _dev(device, o, d)
    plain, binned, numbers, order = _both(tr, to, td, M, "C4 mixed")
    del plain
    _assert_order(order, o, d, pts, cells, "C4 mixed")
    st, xc = numbers["stats"], numbers["cross_check"]
    assert st["walk"] + st["general"] == R and st["walk"] > 0.9 * R, st
    assert xc["checked"] > 0 and xc["mismatches"] == 0 and xc["risk"]["mismatches"] == 0, xc
    assert numbers["reasons"].get(14, 0) == 0, numbers
    rows = np.concatenate([np.arange(8192), np.sort(np.random.default_rng(12).choice(np.arange(8192, R), 8192, replace=False))])
    _against_oracle(binned, _oracle(oracle, pts, cells), o, d, M, rows, "C4 mixed, binned")


# ---------------------------------------------------------------------------------------------------- 2
HAND_OVER_MESHES = {
    "grid": lambda s: s.grid_mesh(),
    "shells": lambda s: s.shells_mesh(),
    "near_duplicates": lambda s: s.near_duplicates_mesh(),
    "colmap_like": lambda s: s.colmap_like_mesh(),
}
# (options, what must be non-empty so that the option's path ran)
HAND_OVER_OPTIONS = (
    ({"literal": 0}, "fallback_only"),
    ({"verify_stride": 4, "verify_inject": 1}, "injected"),
    ({"spec_fill": 1, "spec_k0": 32}, None),
    ({"cert_ends": 1}, None),
    ({"cert_ends": 3}, None),
    ({"writer_table": 1}, None),
    ({"writer_table": 2}, None),
    ({"hull_flat": 0}, None),
    ({"fill_blocks": -2}, None),
    ({"fill_blocks": 512}, None),
)


def _classes(numbers):
    literal = numbers["reasons"].get(13, 0)
    return literal, numbers["stats"]["general"] - literal       # literal pairing of the log | BVH re-trace


@pytest.mark.parametrize("name", sorted(HAND_OVER_MESHES))
def test_hand_over_paths(tn, device, oracle, scenes, name):
    """Adversarial meshes, 20,001 rays (not a multiple of 8, 64 or 256) of which half pass through two mesh vertices: the
    literal pairing kernel (rows by order[item]), the BVH re-trace (caller ids in the list), the late cross-check's re-trace,
    both writer tables, the speculative fill and every tail fill, binned against unbinned; the defaults also against the oracle."""
    pts, cells = HAND_OVER_MESHES[name](scenes)
    o, d = _shuffled(13, scenes.vertex_to_vertex_rays(pts, 10001, 14), scenes.outside_in_rays(10000, 15))
    R, M = len(o), 512
    assert R == 20001
    to, td = _dev(device, o, d)
    tr = _tracer(tn, device, pts, cells, walk=2)
    plain, binned, numbers, order = _both(tr, to, td, M, f"{name} defaults")
    del plain
    _assert_order(order, o, d, pts, cells, name)
    literal, fallback = _classes(numbers)
    print(f"{name}: {len(cells)} tets; literal rays {literal}, BVH re-traced rays {fallback}, {numbers}")
    assert literal > 0 and fallback > 0, (name, numbers)
    _against_oracle(binned, _oracle(oracle, pts, cells), o, d, M, np.arange(R), f"{name} defaults, binned")
    del binned
    for opts, expect in HAND_OVER_OPTIONS:
        tr = _tracer(tn, device, pts, cells, walk=2, **opts)
        _, _, numbers, order = _both(tr, to, td, M, f"{name} {opts}")
        assert len(order) == R, (name, opts)
        lit, fb = _classes(numbers)
        if expect == "fallback_only":
            assert lit == 0 and fb >= literal + fallback, (name, opts, numbers)
        elif expect == "injected":
            assert numbers["reasons"].get(14, 0) > 0.5 * (R - literal - fallback) / 4, (name, opts, numbers)
        else:
            assert lit + fb > 0, (name, opts, numbers)


# ---------------------------------------------------------------------------------------------------- 3, 4
def test_compact_rows(tn, device, scenes):
    import torch

    pts, cells = scenes.random_mesh(15000, 0)
    o, d = _shuffled(16, scenes.outside_in_rays(49152, 4), scenes.inside_out_rays(16384, 2))
    tr = _tracer(tn, device, pts, cells, walk=1)
    to, td = _dev(device, o, d)
    plain, binned, _, order = _both(tr, to, td, 512, "compact rows", compact_rows=True)
    assert len(order) == len(o)
    n = plain["num_visited_cells"]
    assert torch.equal(n, binned["num_visited_cells"]) and int(n.max()) > 0
    live = torch.arange(512, device=device)[None, :] < n[:, None]
    for k in ROW_KEYS:
        a, b = plain[k].view(torch.int32).reshape(len(o), 512, -1), binned[k].view(torch.int32).reshape(len(o), 512, -1)
        assert torch.equal(a[live], b[live]), f"compact rows: {k}"


def test_rays_that_miss(tn, device, scenes):
    pts, cells = scenes.random_mesh(15000, 0)
    o, d = scenes.outside_in_rays(32768, 5)
    away = np.random.default_rng(17).random(len(o)) < 0.5
    d = np.ascontiguousarray(np.where(away[:, None], -d, d))
    tr = _tracer(tn, device, pts, cells, walk=1)
    to, td = _dev(device, o, d)
    _, binned, _, order = _both(tr, to, td, 512, "rays that miss")
    assert len(order) == len(o)
    n = binned["num_visited_cells"].cpu().numpy()
    assert 0.4 * len(o) < away.sum() < 0.6 * len(o)
    assert (n[away] == 0).all() and (n[~away] > 0).mean() > 0.99


# ---------------------------------------------------------------------------------------------------- 5
def test_ineligible_calls_ignore_the_flag(tn, device, scenes):
    pts, cells = scenes.random_mesh(15000, 0)
    tr = _tracer(tn, device, pts, cells, walk=1)
    # a small batch takes the BVH path
    to, td = _dev(device, *scenes.outside_in_rays(4096, 6))
    plain = tr.trace_rays(to, td, 512)
    binned = tr.trace_rays(to, td, 512, bin_rays=True)
    assert tr.trace_stats()["walk"] == 0 and len(tr.ray_order()) == 0
    _assert_same_rows(plain, binned, "BVH path")
    # an eligible call on the same tracer, with the tracer option instead of the flag
    o, d = scenes.outside_in_rays(131072, 7)
    to, td = _dev(device, o, d)
    plain = tr.trace_rays(to, td, 512)
    assert len(tr.ray_order()) == 0
    tr.set_option("bin_rays", 1)
    binned = tr.trace_rays(to, td, 512)
    _assert_order(tr.ray_order(), o, d, pts, cells, "option bin_rays")
    _assert_same_rows(plain, binned, "option bin_rays")
    del binned
    # the same call in chunks of 8192 rays
    tr.set_option("log_cap_mb", 64)
    chunked = tr.trace_rays(to, td, 512, bin_rays=True)
    assert len(tr.ray_order()) == 0
    _assert_same_rows(plain, chunked, "chunked call")


def test_environment_variable_switches_binning_on(tn, device, scenes, monkeypatch):
    pts, cells = scenes.random_mesh(5000, 9)
    o, d = scenes.outside_in_rays(16384, 8)
    to, td = _dev(device, o, d)
    plain = _tracer(tn, device, pts, cells, walk=1).trace_rays(to, td, 256)
    monkeypatch.setenv("TETRANERF_HIP_BIN_RAYS", "1")
    tr = _tracer(tn, device, pts, cells, walk=1)
    monkeypatch.delenv("TETRANERF_HIP_BIN_RAYS")
    binned = tr.trace_rays(to, td, 256)
    _assert_order(tr.ray_order(), o, d, pts, cells, "TETRANERF_HIP_BIN_RAYS")
    _assert_same_rows(plain, binned, "TETRANERF_HIP_BIN_RAYS")


# ---------------------------------------------------------------------------------------------------- 6
def test_c5_full_size(tn, device, scenes):
    """1M tets, 2^20 outside-in rays, M = 512 (28 GB of rows per call): binned == unbinned on all of them, all five arrays.
    The unbinned call is pinned to the oracle by test_parity_configs_gpu.py::test_c5_stress_sample_bit_exact."""
    import torch

    pts, cells = scenes.random_mesh(150000, 3)
    assert len(cells) > 1_000_000
    o, d = scenes.outside_in_rays(1 << 20, 4)
    tr = _tracer(tn, device, pts, cells, walk=1)
    to, td = _dev(device, o, d)
    plain = tr.trace_rays(to, td, 512)
    n_plain = _numbers(tr)
    assert len(tr.ray_order()) == 0
    binned = tr.trace_rays(to, td, 512, bin_rays=True)
    assert _numbers(tr) == n_plain, (n_plain, _numbers(tr))
    assert n_plain["stats"]["walk"] > 0.8 * len(o), n_plain
    assert len(tr.ray_order()) == len(o)
    for k in KEYS:                       # array by array, each pair freed as soon as it is compared
        a, b = plain.pop(k), binned.pop(k)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"C5: {k}"
        del a, b
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- 7
def test_renderer_bin_rays(tn, device, scenes):
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    pts, cells = scenes.random_mesh(5000, 9)
    tr = _tracer(tn, device, pts, cells, walk=2)
    torch.manual_seed(3)
    mlp = render.TetraMLP().to(device)
    field = torch.randn(64, len(pts), device=device) * 0.5
    o, d = _shuffled(18, scenes.outside_in_rays(12288, 4), scenes.inside_out_rays(4096, 2))
    to, td = _dev(device, o, d)
    outs = {}
    for flag in (False, True):
        rd = render.TetraRenderer(tr, field, mlp, 64, 256, fused=True, num_fine_samples=64, bin_rays=flag)
        outs[flag] = rd.render(to, td)
        assert (len(tr.ray_order()) > 0) == flag
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(outs[False][k].view(torch.int32), outs[True][k].view(torch.int32)), k
    assert float(outs[True]["accumulation"].max()) > 0.1
