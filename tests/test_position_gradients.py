"""Position gradients, CPU side: the closed forms of tetra-nerf_amd/geometry.py -- the statement the HIP kernels of
csrc/tn_position_grad.hip implement -- against float64 autograd through the forward statement itself, their exact zeros,
and the new C-ABI / Python surface.  The kernels are held to geometry.py in tests/test_position_gradients_gpu.py."""
import importlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -24      # fp32 unit round-off


@pytest.fixture(scope="module")
def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def _problem(seed, R=7, S=5, V=40, Fd=6, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(V, 3, generator=g, dtype=dtype)
    ids = torch.stack([torch.randperm(V, generator=g)[:4] for _ in range(R * S)]).to(torch.int32)
    field_vm = torch.randn(V, Fd, generator=g, dtype=dtype)
    o = torch.randn(R, 3, generator=g, dtype=dtype)
    d = torch.randn(R, 3, generator=g, dtype=dtype)
    t = torch.rand(R, S, generator=g, dtype=dtype) + 0.5
    G = torch.randn(R * S, Fd, generator=g, dtype=dtype)
    return verts, ids, field_vm, o, d, t, G


def test_closed_forms_equal_autograd_through_the_forward_statement(geometry):
    """b = solve(T^T, p - x0), phi = the weighted sum of field rows, p = o + t d: float64 autograd of that statement gives
    dL/db, dL/dp, dL/d(vertex table), dL/do and dL/dd; (A) and (B) must equal them."""
    R, S = 7, 5
    verts, ids, field_vm, o, d, t, G = _problem(0, R, S)
    verts.requires_grad_(True)
    o.requires_grad_(True)
    d.requires_grad_(True)
    p = (o[:, None, :] + t[..., None] * d[:, None, :]).reshape(-1, 3)
    p.retain_grad()
    b = geometry.barycentrics_of(p, verts[ids.long()])
    b.retain_grad()
    rows = field_vm[ids.long()]                                                  # [n, 4, F]
    phi = b[:, 0:1] * rows[:, 1] + b[:, 1:2] * rows[:, 2] + b[:, 2:3] * rows[:, 3] + (1 - b.sum(-1, keepdim=True)) * rows[:, 0]
    (phi * G).sum().backward()

    gb = geometry.gather_backward_barycentrics(ids, field_vm, G)
    torch.testing.assert_close(gb, b.grad, rtol=1e-10, atol=1e-10)
    out = geometry.sample_positions_backward(ids, b.detach(), gb, verts.detach(), t.reshape(-1), S)
    assert bool(out["live"].all())
    scale = float(p.grad.abs().max())
    for name, want in (("points", p.grad), ("vertices", verts.grad), ("origins", o.grad), ("directions", d.grad)):
        err = float((out[name] - want).abs().max())
        assert err <= 1e-9 * scale, (name, err, scale)


@pytest.mark.parametrize("D", [2, 3, 4, 6])
def test_gather_adjoint_any_dimension_and_empty_rows(geometry, D):
    g = torch.Generator().manual_seed(D)
    V, Fd, n = 30, 5, 50
    ids = torch.randint(0, V, (n, D), generator=g, dtype=torch.int32)
    ids[::7, 0] = -1
    ids[3::7, D - 1] = -1
    field_vm = torch.randn(V, Fd, generator=g, dtype=torch.float64)
    G = torch.randn(n, Fd, generator=g, dtype=torch.float64)
    b = torch.rand(n, D - 1, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.cat([1 - b.sum(-1, keepdim=True), b], -1)
    rows = field_vm[ids.long().clamp_min(0)] * (ids >= 0)[..., None]
    ((w[..., None] * rows).sum(1) * G).sum().backward()
    torch.testing.assert_close(geometry.gather_backward_barycentrics(ids, field_vm, G), b.grad, rtol=1e-12, atol=1e-12)


def test_masked_empty_and_zero_volume_samples_give_exact_zeros(geometry):
    R, S = 4, 6
    verts, ids, field_vm, o, d, t, G = _problem(1, R, S)
    ids[0, 2] = -1                      # one EMPTY id
    ids[1] = -1                         # an unmatched sample: all ids EMPTY
    ids[2] = torch.tensor([5, 5, 9, 11], dtype=torch.int32)     # x1 == x0: zero volume
    verts[20] = verts[21] + 0.5 * (verts[22] - verts[21])
    ids[3] = torch.tensor([21, 22, 20, 23], dtype=torch.int32)  # three collinear vertices: zero volume
    b = torch.rand(R * S, 3, dtype=torch.float64) / 3
    gb = torch.randn(R * S, 3, dtype=torch.float64)
    dead = [0, 1, 2]
    for dtype in (torch.float64, torch.float32):
        out = geometry.sample_positions_backward(ids, b.to(dtype), gb.to(dtype), verts.to(dtype), t.reshape(-1).to(dtype), S)
        live = out["live"]
        assert not bool(live[dead].any())
        assert bool(live[4:].all())
        assert bool((out["points"][~live] == 0).all())
        # the same call without the dead samples' gradient: nothing they could have touched differs by a bit
        gb2 = gb.to(dtype).clone()
        gb2[~live] = 0
        ref = geometry.sample_positions_backward(ids, b.to(dtype), gb2, verts.to(dtype), t.reshape(-1).to(dtype), S)
        for k in ("points", "vertices", "origins", "directions"):
            assert torch.equal(out[k], ref[k]), k
        assert bool(torch.isfinite(out["vertices"]).all())
    # a ray made only of dead samples receives exact zeros
    ids[:S] = -1
    out = geometry.sample_positions_backward(ids, b, gb, verts, t.reshape(-1), S)
    assert bool((out["origins"][0] == 0).all()) and bool((out["directions"][0] == 0).all())
    # (A): EMPTY rows are zero rows
    ga = geometry.gather_backward_barycentrics(ids[:S], field_vm, G[:S])
    assert bool((ga == 0).all())


def test_fp32_closed_form_meets_the_conditioning_bound_on_a_delaunay_mesh(geometry, scenes):
    """The bound the GPU test holds the kernel to, ||m32 - m64|| <= 8 u cond2(T) ||m64||, checked for the closed form in
    float32 on every tetrahedron of a Delaunay mesh of uniform points (float64 solve on the same float32 inputs)."""
    pts, cells = scenes.random_mesh(2000, 3)
    verts = torch.from_numpy(pts)
    ids = torch.from_numpy(cells.astype(np.int32))
    g = torch.randn(len(ids), 3, generator=torch.Generator().manual_seed(0))
    m32, live = geometry.sample_point_gradient(ids, g, verts)
    assert bool(live.all())
    x = verts.double()[ids.long()]
    T = x[:, 1:] - x[:, :1]
    m64 = torch.linalg.solve(T, g.double().unsqueeze(-1)).squeeze(-1)
    sv = torch.linalg.svdvals(T)
    cond = sv[:, 0] / sv[:, -1]
    ratio = (m32.double() - m64).norm(dim=-1) / (U * cond * m64.norm(dim=-1))
    print(f"cond max {float(cond.max()):.3g}, worst error / (u cond |m|) = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 8.0


def test_new_symbols_declared_and_bound():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    text = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("tn_interpolate_values_backward_bary_vm", "tn_sample_positions_backward"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS
    assert "#define TN_ABI_VERSION 6" in text and _lib.ABI_VERSION == 6      # no existing signature changed
    lib = _lib.load()
    assert len(lib.tn_interpolate_values_backward_bary_vm.argtypes) == 8
    assert len(lib.tn_sample_positions_backward.argtypes) == 13


def test_public_surface(tn):
    assert callable(tn.sample_positions_grad) and "sample_positions_grad" in tn.__all__
    assert callable(tn.add_barycentrics_grad)
    for name in ("interpolate_values_backward_barycentrics", "sample_positions_backward"):
        assert callable(getattr(tn.cpp, name))
    import inspect

    render = importlib.import_module("tetra-nerf_amd.render")
    sig = inspect.signature(render.TetraRenderer.render_train)
    assert sig.parameters["position_gradients"].default is False and sig.parameters["vertices"].default is None
    sig = inspect.signature(tn.cpp.mlp_backward)
    assert sig.parameters["want_bary_grad"].default is False and sig.parameters["return_dx0"].default is False


def test_new_ops_reject_cpu_tensors(tn):
    vi = torch.zeros((2, 3, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        tn.cpp.interpolate_values_backward_barycentrics(vi, torch.zeros((64, 10)), torch.zeros((2, 3, 64)))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        tn.cpp.sample_positions_backward(vi, torch.zeros((2, 3, 3)), torch.zeros((2, 3, 3)), torch.zeros((10, 3)),
                                         torch.zeros((2, 3)), want_origins=True)


def test_render_train_position_gradients_equal_autograd_of_the_whole_statement(tn, oracle, scenes, geometry, monkeypatch):
    """The wiring of render_train(position_gradients=True), on the CPU: the unfused statement on the oracle tracer, with the
    HIP kernel behind sample_positions_grad replaced by its statement in geometry.py, against float64 autograd of the
    WHOLE chain on the same sample placement -- p = o + t d (t constant), b = solve(T^T, p - x0) from the vertex table,
    gather, MLP with the view direction, renderers, loss.  Tolerance 1e-3 of the largest entry: u cond for the float32 chain
    through tets of cond <= ~1e4 is 6e-4; a wrong sign, vertex order, ray parameter or a missing view term is O(1)."""
    import sys

    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import reference_model as rm

    render = importlib.import_module("tetra-nerf_amd.render")

    def stand_in(vi, bc, gb, vertices, distances=None, want_points=False, want_origins=False, want_directions=False,
                 want_vertices=False):
        S = vi.shape[1]
        out = geometry.sample_positions_backward(vi.reshape(-1, 4), bc.reshape(-1, 3), gb.reshape(-1, 3), vertices,
                                                 None if distances is None else distances.reshape(-1), S)
        return (out["points"].reshape(-1, S, 3) if want_points else None, out["origins"] if want_origins else None,
                out["directions"] if want_directions else None, out["vertices"] if want_vertices else None)

    monkeypatch.setattr(tn.cpp, "sample_positions_backward", stand_in)

    class Tracer(rm.OracleTorchTracer):
        def trace_rays(self, origins, directions, max_ray_triangles):
            return super().trace_rays(origins.detach(), directions.detach(), max_ray_triangles)

    pts, cells = scenes.random_mesh(600, 3)
    tracer = Tracer(oracle, pts, cells)
    tracer.tetrahedra_vertices = torch.from_numpy(pts)
    o_np, d_np = scenes.outside_in_rays(48, 4)
    S, S_fine, M = 8, 8, 256
    torch.manual_seed(0)
    mlp = render.TetraMLP()
    for p in mlp.parameters():
        p.data.mul_(1.5)
    field = (torch.rand(64, len(pts)) * 2 - 1).requires_grad_(True)
    rd = render.TetraRenderer(tracer, field, mlp, S, M, num_fine_samples=S_fine, cache_field=False, device_samplers=False,
                              interpolate_values=rm.einsum_interpolate_values)
    o = torch.from_numpy(o_np).requires_grad_(True)
    d = torch.from_numpy(d_np).requires_grad_(True)
    verts = torch.from_numpy(pts).clone().requires_grad_(True)
    hit = int((tracer.trace_rays(o, d, M)["num_visited_cells"] > 0).sum())
    rand = {"coarse": torch.rand(hit, S + 1), "fine": torch.rand(hit, S_fine + 1)}
    target = torch.rand(len(o_np), 3)

    def loss_of(rgb, acc):
        return ((rgb - target.to(rgb.dtype)) ** 2).mean() + 0.1 * acc.mean()

    cap = {}
    out = rd.render_train(o, d, rand=rand, fused=False, capture=cap, position_gradients=True, vertices=verts)
    assert cap["barycentric_positions"].requires_grad and torch.equal(cap["barycentric_positions"], cap["barycentric_coordinates"])
    loss_of(out["rgb"], out["accumulation"]).backward()
    field_grad_on = field.grad.clone()

    # float64 autograd of the whole statement on the captured placement
    idx, vi, edges = cap["idx"], cap["vertex_indices"], cap["edges"].double()
    o64, d64, v64 = (x.detach().double().requires_grad_(True) for x in (o, d, verts))
    t = (edges[:, 1:] + edges[:, :-1]) / 2
    p = o64[idx][:, None, :] + t[..., None] * d64[idx][:, None, :]
    matched = (vi >= 0).all(-1)
    b = torch.zeros(*vi.shape[:2], 3, dtype=torch.float64)
    b = b.masked_scatter(matched[..., None].expand(-1, -1, 3), geometry.barycentrics_of(p[matched], v64[vi[matched].long()]))
    assert float((b.detach() - cap["barycentric_coordinates"].double()).abs().max()) < 1e-3      # the convention, on the CPU
    mlp64 = render.TetraMLP().double()
    mlp64.load_state_dict({k: v.double() for k, v in mlp.state_dict().items()})
    feats = rm.einsum_interpolate_values(vi, b, field.detach().double())
    S2 = cap["samples_per_ray"]
    sg, col = mlp64(feats, d64[idx][:, None, :].expand(-1, S2, -1))
    rgb_r, acc_r, _, _ = render.composite(sg, col, edges[:, :-1, None], edges[:, 1:, None])
    R = len(o_np)
    rgb = torch.ones(R, 3, dtype=torch.float64).index_copy(0, idx, rgb_r)
    acc = torch.zeros(R, 1, dtype=torch.float64).index_copy(0, idx, acc_r)
    loss_of(rgb, acc).backward()
    for name, got, want in (("origins", o.grad, o64.grad), ("directions", d.grad, d64.grad), ("vertices", verts.grad, v64.grad)):
        scale = float(want.abs().max())
        err = float((got.double() - want).abs().max())
        print(f"{name}: max |gradient| {scale:.3g}, max error {err:.3g}")
        assert scale > 0 and err <= 1e-3 * scale, (name, err, scale)

    # off is off: the same call without the switch gives the same outputs, the same field gradient (to round-off: the
    # einsum gather of this CPU statement is differentiated by torch, which contracts in another order once both of its
    # operands require a gradient) and no gradient reaches the origins
    field.grad = None
    o2 = torch.from_numpy(o_np).requires_grad_(True)
    out2 = rd.render_train(o2, torch.from_numpy(d_np), rand=rand, fused=False)
    loss_of(out2["rgb"], out2["accumulation"]).backward()
    assert torch.equal(out2["rgb"], out["rgb"]) and o2.grad is None
    torch.testing.assert_close(field.grad, field_grad_on, rtol=1e-4, atol=1e-6 * float(field_grad_on.abs().max()))
