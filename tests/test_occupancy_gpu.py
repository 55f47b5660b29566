"""The per-tetrahedron occupancy field on the GPU (csrc/tn_occupancy.hip): tn_occupancy_update and tn_cull_samples bit for bit
against their PyTorch statements (render.occupancy_update_statement / cull_mask_statement), tn_mlp_forward_gather_indexed bit for
bit against tn_mlp_forward_gather at the listed samples, the culled render against the chain assembled here from the existing ops,
the training update, and occupancy_from_field against float64.

Sizes at which the kernels change form (from tn_occupancy.hip):
  update, decay pass     256 tetrahedra per block (OC_BLOCK), at most 2048 blocks (OC_MAX_GRID): a thread strides from T = 524288 on
  update, scatter-max    64 samples per wave step (the segmented fold), 256 per block, 2048 blocks: strides from n = 524288 on
  cull                   64 samples per ballot step, 1024 per wave tile (CU_TILE), 4 tiles per block, 1024 tiles per pass of the
                         one-block scan (CU_SCAN): n > 1048576 takes a second pass
  indexed forward        32 listed samples per wave, 256 per group, 256 blocks: a block strides from 65536 listed samples on
"""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

render = importlib.import_module("tetra-nerf_amd.render")
EMPTY = -1            # int32 view of the matcher's 0xFFFFFFFF


def bits(x):
    """int32 bit patterns with every NaN mapped to one value (a NaN's payload is not part of any statement)"""
    x = x.detach().reshape(-1)
    return torch.where(torch.isnan(x), torch.full_like(x, float("nan")).view(torch.int32), x.contiguous().view(torch.int32)).cpu()


def _samples(T, n, gen, dev, one_cell=None):
    """n samples over T tetrahedra with every excluded class mixed in: unmatched, ids >= T, NaN, negative and -0 densities"""
    cells = torch.randint(0, T, (n,), generator=gen, dtype=torch.int32) if one_cell is None else torch.full((n,), one_cell, dtype=torch.int32)
    sigma = torch.rand(n, generator=gen) * 8
    if n:
        # runs of equal cells, as consecutive samples of a ray give them
        if one_cell is None:
            cells = cells[torch.div(torch.arange(n), 3, rounding_mode="floor") * 3 % n]
        kind = torch.randint(0, 16, (n,), generator=gen)
        cells[kind == 0] = EMPTY
        cells[kind == 1] = T + int(torch.randint(0, 5, (1,), generator=gen))
        sigma[kind == 2] = float("nan")
        sigma[kind == 3] = -sigma[kind == 3] - 0.5
        sigma[kind == 4] = float("inf")
        sigma[kind == 5] = -0.0
        sigma[kind == 6] = 0.0
    return cells.to(dev), sigma.to(dev)


@pytest.mark.parametrize("T", [1, 255, 256, 257, 70001, 524289])
def test_update_equals_statement(tn, device, T):
    gen = torch.Generator().manual_seed(T)
    occ0 = (torch.rand(T, generator=gen) * 6).to(device)
    occ0[::7] = 0.0
    if T > 3:
        occ0[3] = float("nan")
    sizes = (0, 1, 63, 64, 65, 255, 256, 257) + ((524287, 524288, 524289) if T in (1, 257, 70001) else (3001,))
    for n in sizes:
        for one_cell in ((None, T - 1) if n in (257, 524289, 3001) else (None,)):       # + everything in ONE tetrahedron
            cells, sigma = _samples(T, n, gen, device, one_cell)
            want = render.occupancy_update_statement(occ0, cells, sigma, 0.9)
            runs = []
            for _ in range(2):
                occ = occ0.clone()
                assert tn.cpp.occupancy_update(occ, cells, sigma, 0.9) is occ
                runs.append(bits(occ))
            assert torch.equal(runs[0], bits(want)), (T, n, one_cell)
            assert torch.equal(runs[0], runs[1]), (T, n, one_cell)


@pytest.mark.parametrize("S", [1, 5, 257])
def test_update_device_count(tn, device, S):
    gen = torch.Generator().manual_seed(S)
    T, R, live = 300, 41, 29
    cells, sigma = _samples(T, R * S, gen, device)
    cells, sigma = cells.view(R, S).clone(), sigma.view(R, S).clone()
    cells[live:] = torch.randint(0, T, (R - live, S), generator=gen, dtype=torch.int32).to(device)
    sigma[live::2] = float("nan")            # rows beyond the count: poisoned -- NaN, and values that would win every maximum
    sigma[live + 1::2] = float("inf")
    occ0 = torch.rand(T, generator=gen).to(device)
    want = render.occupancy_update_statement(occ0, cells[:live], sigma[:live], 0.5)
    count = torch.tensor([live], dtype=torch.int32, device=device)
    for kw in (dict(samples_per_ray=S), dict()):          # (default: the last dimension of 2-D cells)
        occ = occ0.clone()
        tn.cpp.occupancy_update(occ, cells, sigma, 0.5, count=count, **kw)
        assert torch.equal(bits(occ), bits(want))
    with pytest.raises(RuntimeError, match="samples_per_ray"):
        tn.cpp.occupancy_update(occ0.clone(), cells.view(-1), sigma.view(-1), 0.5, count=count)


def _cull_case(n, k, gen, dev):
    """cells of n samples of which exactly k are live at threshold 0.5, through every live class"""
    occ = torch.tensor([0.0, 1.0, float("nan"), 0.25, 0.5], dtype=torch.float32)       # cells 0 and 3 are culled
    cells = torch.where(torch.rand(n, generator=gen) < 0.5, 0, 3).to(torch.int32)
    live_at = torch.randperm(n, generator=gen)[:k]
    live_kind = torch.tensor([1, 2, 4, EMPTY, 5, 1000], dtype=torch.int32)              # occupied, NaN, == threshold, unmatched, >= T
    cells[live_at] = live_kind[torch.randint(0, len(live_kind), (k,), generator=gen)]
    return cells.to(dev), occ.to(dev)


def _check_cull(tn, cells, occ, thr, S, rows, with_rgb, dev):
    n = cells.numel()
    sigma = torch.full((n,), float("nan"), device=dev)
    rgb = torch.full((n, 3), float("nan"), device=dev) if with_rgb else None
    count = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev)
    live, live_count = tn.cpp.cull_samples(cells, occ, thr, sigma, rgb, samples_per_ray=S, count=count)
    n_eff = n if rows is None else rows * S
    culled = render.cull_mask_statement(cells.view(-1), occ, thr)
    culled[n_eff:] = False
    in_range = torch.arange(n, device=dev) < n_eff
    want = torch.nonzero(~culled & in_range)[:, 0].to(torch.int32)
    assert int(live_count) == want.numel()
    assert live.dtype == torch.int32 and live.numel() == n
    assert torch.equal(live[:want.numel()], want)
    # exactly the culled positions are 0, everything else (live positions, rows beyond the count) is still NaN
    assert torch.equal(sigma == 0, culled) and torch.equal(torch.isnan(sigma), ~culled)
    if with_rgb:
        assert torch.equal(rgb == 0, culled[:, None].expand(n, 3)) and torch.equal(torch.isnan(rgb), ~culled[:, None].expand(n, 3))
    return want.numel()


@pytest.mark.parametrize("S", [1, 5, 257])
def test_cull_equals_statement(tn, device, S):
    gen = torch.Generator().manual_seed(100 + S)
    R = {1: 1300, 5: 260, 257: 6}[S]        # n = 1300 / 1300 / 1542: more than one tile, not a multiple of 64
    n = R * S
    for k in (0, 1, 31, 32, 33, 255, 256, 257, n):
        cells, occ = _cull_case(n, k, gen, device)
        assert _check_cull(tn, cells.view(R, S), occ, 0.5, S, None, k % 2 == 0, device) == k
    # a device-side ray count: nothing beyond it is listed or touched
    cells, occ = _cull_case(n, 300, gen, device)
    _check_cull(tn, cells.view(R, S), occ, 0.5, S, R - 2, True, device)
    _check_cull(tn, cells.view(R, S), occ, 0.5, S, 0, True, device)
    # threshold <= 0 and NaN cull nothing, even with negative occupancies
    for thr in (0.0, -1.0, float("nan")):
        assert _check_cull(tn, cells.view(R, S), -occ, thr, S, None, False, device) == n
    # n = 0, n = 1
    assert _check_cull(tn, cells[:0], occ, 0.5, 1, None, True, device) == 0
    assert _check_cull(tn, torch.tensor([1], dtype=torch.int32, device=device), occ, 0.5, 1, None, True, device) == 1
    assert _check_cull(tn, torch.tensor([0], dtype=torch.int32, device=device), occ, 0.5, 1, None, True, device) == 0


def test_cull_spans_two_passes_of_the_scan(tn, device):
    gen = torch.Generator().manual_seed(7)
    n = 1024 * 1024 + 1500          # 1026 tiles: the one-block scan takes a second pass with a carry
    cells, occ = _cull_case(n, n // 3, gen, device)
    assert _check_cull(tn, cells, occ, 0.5, 1, None, False, device) == n // 3
    _check_cull(tn, cells.view(-1, 4), occ, 0.5, 4, (n // 4) - 300, True, device)


def _forward_problem(R, S, dev, seed):
    rng = np.random.default_rng(seed)
    V = 700
    vi = rng.integers(0, V, (R, S, 4)).astype(np.int32)
    vi[rng.random((R, S)) < 0.2] = -1
    bc = (rng.random((R, S, 3)).astype(np.float32)) / 4
    torch.manual_seed(seed)
    mlp = render.TetraMLP().to(dev)
    field = torch.randn(64, V, device=dev)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1)
    bias = torch.randn(R, 128, device=dev) * 0.7
    return torch.from_numpy(vi).to(dev), torch.from_numpy(bc).to(dev), field, dirs, bias, render.mlp_weights(mlp)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("R,S,counts", [(64, 5, (0, 1, 31, 32, 33, 255, 256, 257, 320)), (300, 257, (257, 70000, 77100))])
def test_indexed_forward_equals_plain_forward_at_the_listed_samples(tn, device, mode, R, S, counts):
    """(S = 5: the 32 lanes of a wave's tile belong to seven rays; 70000 listed samples: a block strides over two groups)"""
    vi, bc, field, dirs, bias, w = _forward_problem(R, S, device, 11 + S)
    n = R * S
    gen = torch.Generator().manual_seed(S)
    for kind in ("density", "heads", "heads+bias"):
        d = None if kind == "density" else dirs
        hb = bias if kind == "heads+bias" else None
        full = tn.cpp.mlp_forward_gather(vi, bc, field, d, w, S, mode=mode, ray_head_bias=hb)
        full_sigma, full_rgb = (full, None) if d is None else full
        for k in counts:
            listed = torch.sort(torch.randperm(n, generator=gen)[:k]).values.to(device)
            live = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=device)      # (entries beyond the count: not a sample)
            live[:k] = listed.to(torch.int32)
            live_count = torch.tensor([k], dtype=torch.int32, device=device)
            sigma = torch.full((n,), float("nan"), device=device)
            rgb = None if d is None else torch.full((n, 3), float("nan"), device=device)
            out = tn.cpp.mlp_forward_gather_indexed(live, live_count, vi, bc, field, d, w, S, mode=mode, ray_head_bias=hb,
                                                    sigma=sigma, rgb=rgb)
            assert (out is sigma) if d is None else (out[0] is sigma and out[1] is rgb)
            is_listed = torch.zeros(n, dtype=torch.bool, device=device)
            is_listed[listed] = True
            assert torch.equal(sigma[listed].view(torch.int32), full_sigma[listed].view(torch.int32)), (kind, k)
            assert bool(torch.isnan(sigma[~is_listed]).all()) and not bool(torch.isnan(sigma[listed]).any()), (kind, k)
            if d is not None:
                assert torch.equal(rgb[listed].view(torch.int32), full_rgb[listed].view(torch.int32)), (kind, k)
                assert bool(torch.isnan(rgb[~is_listed]).all()), (kind, k)


def test_indexed_forward_arguments(tn, device):
    R, S = 8, 5
    vi, bc, field, dirs, bias, w = _forward_problem(R, S, device, 3)
    n = R * S
    live = torch.arange(n, dtype=torch.int32, device=device)
    live_count = torch.tensor([n], dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="bf16"):
        tn.cpp.mlp_forward_gather_indexed(live, live_count, vi, bc, field, dirs, w, S, mode="bf16")
    rc = tn.cpp._lib.load().tn_mlp_forward_gather_indexed(tn.cpp.fused_mlp(w).handle, n, S, live.data_ptr(), live_count.data_ptr(),
                                                         vi.data_ptr(), bc.data_ptr(), tn.cpp.field_vertex_major(field).data_ptr(),
                                                         dirs.data_ptr(), 2, torch.empty(n, device=device).data_ptr(),
                                                         torch.empty(n, 3, device=device).data_ptr(), None, None, None)
    assert rc != 0 and b"mode 2" in tn.cpp._lib.load().tn_last_error()
    # a device-side ray count: listed samples of rows beyond it are skipped; so is a list entry that is no sample at all
    count = torch.tensor([R - 3], dtype=torch.int32, device=device)
    sigma = torch.full((n,), float("nan"), device=device)
    bad = live.clone()
    bad[2] = 0x7F7F7F7F
    tn.cpp.mlp_forward_gather_indexed(bad, live_count, vi, bc, field, None, w, S, count=count, sigma=sigma)
    full = tn.cpp.mlp_forward_gather(vi, bc, field, None, w, S)
    keep = torch.arange(n, device=device) < (R - 3) * S
    keep[2] = False
    assert torch.equal(sigma[keep].view(torch.int32), full[keep].view(torch.int32)) and bool(torch.isnan(sigma[~keep]).all())


@pytest.fixture(scope="module")
def small_scene(tn, device, scenes):
    pts, cells = scenes.random_mesh(900, 12)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(330, 13)
    o, d = np.concatenate([o, o[:37] + 40.0]), np.concatenate([d, d[:37]])       # + rays that miss
    perm = np.random.default_rng(1).permutation(len(o))
    torch.manual_seed(5)
    mlp = render.TetraMLP().to(device)
    field = torch.randn(64, len(pts), device=device) * 0.5
    to = torch.from_numpy(np.ascontiguousarray(o[perm], dtype=np.float32)).to(device)
    td = torch.from_numpy(np.ascontiguousarray(d[perm], dtype=np.float32)).to(device)
    return dict(tr=tr, mlp=mlp, field=field, o=to, d=td, T=len(cells), cells=torch.from_numpy(cells).to(device))


def _assembled(tn, rd, o, d, occ, thr, mode, hb=None):
    """The culled frame from the EXISTING ops of the kernel chain, with the densities and colours masked in torch"""
    cpp, S = tn.cpp, rd.S
    out = rd._trace(o, d)
    lists = render.trace_rows(out)
    nv = out["num_visited_cells"]
    rgb, acc, depth = rd._miss_frame(o.shape[0], rd.background, o.device)
    order, count = cpp.compact_hits(nv)
    w = render.mlp_weights(rd.mlp)
    dirs_o = d.index_select(0, order.long())
    hb_o = None if hb is None else hb.index_select(0, order.long()).contiguous()
    edges, near_far = cpp.sample_coarse(lists[0], lists[3], order, S, biased=rd.biased, count=count)
    traced = rd._locate(lists, edges, order, count)
    if rd.S_fine:
        sigma_c = cpp.mlp_forward_gather(traced["vertex_indices"], traced["barycentric_coordinates"], rd.field, None, w, S, mode=mode,
                                         count=count).view(-1, S)
        sigma_c = torch.where(render.cull_mask_statement(traced["cell_indices"], occ, thr), torch.zeros_like(sigma_c), sigma_c)
        weights_c = cpp.composite(sigma_c.contiguous(), None, edges, count=count)
        edges = cpp.sample_pdf(edges, weights_c, near_far, rd.S_fine, count=count)
        traced = rd._locate(lists, edges, order, count)
    Sf = edges.shape[1] - 1
    sigma, col = cpp.mlp_forward_gather(traced["vertex_indices"], traced["barycentric_coordinates"], rd.field, dirs_o, w, Sf, mode=mode,
                                        ray_head_bias=hb_o, count=count)
    culled = render.cull_mask_statement(traced["cell_indices"], occ, thr)
    sigma = torch.where(culled, torch.zeros_like(culled, dtype=torch.float32), sigma.view(-1, Sf)).contiguous()
    col = torch.where(culled[..., None], torch.zeros_like(col.view(-1, Sf, 3)), col.view(-1, Sf, 3)).contiguous()
    cpp.composite(sigma, col, edges, background=rd.background, clamp=True, out=(rgb, acc, depth), ray_index=order, count=count)
    return {"rgb": rgb, "accumulation": acc, "depth": depth, "culled": int(culled[:int(count)].sum()), "samples": int(count) * Sf}


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("S,S_fine,device_samplers", [(11, 7, True), (13, 0, True), (11, 7, False)])
def test_culled_render(tn, device, small_scene, monkeypatch, mode, S, S_fine, device_samplers):
    sc = small_scene
    o, d = sc["o"], sc["d"]
    kw = dict(num_fine_samples=S_fine, mlp_mode=mode, device_samplers=device_samplers)
    chain = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], S, 256, fused_pass=False, **kw)
    rd = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], S, 256, **kw)        # fused_pass="auto"
    plain = chain.render(o, d)
    assert 0 < int(plain["ray_mask"].sum()) < len(o)
    if device_samplers:
        assert rd._one_launch_ok(mode)          # this renderer takes the persistent launch without an occupancy ...
    calls = []
    real = tn.cpp.render_rays
    monkeypatch.setattr(tn.cpp, "render_rays", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device)
    hb = torch.randn(len(o), 128, device=device) * 0.5
    keys = ("rgb", "accumulation", "depth")
    # threshold 0: the chain's frame, bit for bit
    zero = rd.render(o, d, occupancy=occ, occupancy_threshold=0.0)
    for k in keys:
        assert torch.equal(zero[k], plain[k]), k
    assert torch.equal(zero["ray_mask"], plain["ray_mask"])
    if device_samplers:
        # a random occupancy and a mid threshold, and everything culled: the chain assembled from the existing ops
        for thr, bias in ((0.5, None), (0.5, hb), (2.0, None)):
            got = rd.render(o, d, occupancy=occ, occupancy_threshold=thr, ray_head_bias=bias)
            want = _assembled(tn, chain, o, d, occ, thr, mode, bias)
            if thr == 0.5:
                assert 0.2 * want["samples"] < want["culled"] < 0.8 * want["samples"]
            for k in keys:
                assert torch.equal(got[k], want[k]), (thr, k)
            assert not torch.equal(got["rgb"], plain["rgb"])
    else:
        got = rd.render(o, d, occupancy=occ, occupancy_threshold=0.5)
        assert not torch.equal(got["rgb"], plain["rgb"])
    assert not calls                              # ... and never with one
    rd.render(o, d)
    assert len(calls) == (1 if device_samplers else 0)
    with pytest.raises(RuntimeError, match="bf16"):
        rd.render(o, d, occupancy=occ, occupancy_threshold=0.5, mlp_mode="bf16")
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render(o, d, occupancy=occ)


@pytest.mark.parametrize("sync_free", [True, False])
def test_train_update_leaves_the_batch_alone(tn, device, small_scene, monkeypatch, sync_free):
    sc = small_scene
    monkeypatch.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
    mlp = render.TetraMLP().to(device)
    mlp.load_state_dict(sc["mlp"].state_dict())
    field = sc["field"].clone().requires_grad_(True)
    rd = render.TetraRenderer(sc["tr"], field, mlp, 11, 256, num_fine_samples=7, sync_free_train=sync_free, sync_free_min_hits=0.0)
    params = [field] + list(mlp.parameters())
    target = torch.rand(len(sc["o"]), 3, generator=torch.Generator().manual_seed(2)).to(device)
    recorded = []
    real = tn.cpp.occupancy_update

    def recording(occupancy, cells, sigma, decay, **kw):
        recorded.append((occupancy.clone(), cells.clone(), sigma.clone(), decay, kw))
        return real(occupancy, cells, sigma, decay, **kw)

    monkeypatch.setattr(tn.cpp, "occupancy_update", recording)

    def batch(**kw):
        torch.manual_seed(9)
        for p in params:
            p.grad = None
        out = rd.render_train(sc["o"], sc["d"], **kw)
        ((out["rgb"] - target) ** 2).mean().backward()
        return out, [p.grad.clone() for p in params]

    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(4)).to(device)
    occ_in = occ.clone()
    out0, g0 = batch()
    assert not recorded
    out1, g1 = batch(occupancy=occ, occupancy_decay=0.75)
    for k in ("rgb", "accumulation", "depth", "ray_mask"):
        assert torch.equal(out0[k], out1[k]), k
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert len(recorded) == 1
    occ_before, cells, sigma, decay, kw = recorded[0]
    assert torch.equal(occ_before, occ_in) and decay == 0.75 and cells.shape == sigma.shape and cells.shape[1] == 11 + 7 + 1
    assert not sigma.requires_grad
    want = render.occupancy_update_statement(occ_before, cells, sigma, decay)
    assert torch.equal(bits(occ), bits(want))
    assert not torch.equal(occ, occ_in) and bool((occ >= 0.75 * occ_in).all())
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render_train(sc["o"], sc["d"], occupancy=occ)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_occupancy_from_field_vs_float64(tn, device, small_scene, mode):
    """The kernels are fp32 MFMA (or bf16x3 at the same bar), the reference float64: agreement within the margin
    tests/test_render_gpu.py:72 grants mlp_forward_gather against the PyTorch statement (rtol 1e-5, atol 1e-5)."""
    sc = small_scene
    cells, field, mlp = sc["cells"], sc["field"], sc["mlp"]
    got = render.occupancy_from_field(cells, field, mlp, mode=mode)
    assert got.shape == (sc["T"],) and got.dtype == torch.float32
    f64 = field.double().cpu()
    m64 = render.TetraMLP().double()
    m64.load_state_dict({k: v.double().cpu() for k, v in mlp.state_dict().items()})
    rows = f64[:, cells.long().cpu()]                                  # [64, T, 4]
    probes = torch.cat([rows.mean(-1, keepdim=True), rows], -1)         # centroid + the four vertices: [64, T, 5]
    with torch.no_grad():
        want = render.coarse_sigma(m64, probes.permute(1, 2, 0)).max(dim=1).values
    np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert float(want.max()) > float(want.min())
