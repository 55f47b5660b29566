"""Position gradients on the GPU: tn_interpolate_values_backward_bary_vm (A) and tn_sample_positions_backward (B), and the
autograd wiring above them, held to the float64 statement of tetra-nerf_amd/geometry.py.

Every bound below is a priori; u = 2^-24 is the fp32 unit round-off:
  (A)  |g32 - g64| <= (2F + 2) u sum_c |G_c| (|F[v_{k+1},c]| + |F[v_0,c]|): the dot-product bound (one subtraction, one
       product and at most F additions per term), no exclusions.
  (B)  ||m32 - m64|| <= 8 u cond2(T) ||m64|| per sample against a float64 solve on the kernel's own fp32 inputs: the backward
       error of a 3 x 3 solve in fp32; the closed form measures <= 2.6 u cond on Delaunay meshes on the CPU
       (tests/test_position_gradients.py), torch's fp32 LU <= 2.8.  No exclusions.
  sums: the per-sample bounds of (B) times |w_k| (vertices), 1 (origins), |t| (directions), plus n_terms u sum |terms| for
       the fp32 summation of n_terms terms in any order (each product w_k m / t m is one more rounding of a term and is covered
       by n_terms >= 1).  The weights w are the forward's own: w_0 = 1 - ((b0 + b1) + b2) evaluated in fp32, the bits that
       tn_interp.hip's kernels, the deterministic adjoint and k_sample_positions_bwd all form from the same barycentrics, so
       the float64 reference sums w32_k m64 (geometry.sample_positions_backward(weights=gather_weights(b32))).
The reference and the bounds of (B) are position_grad_cases.m64_and_cond / sample_bound / sums_and_bounds, shared with
tests/test_position_grad_edges_gpu.py, which holds (B) to them at the edges of its launch and on dead samples.
"""
import importlib

import numpy as np
import pytest
import torch

import position_grad_cases as pgc

pytestmark = pytest.mark.gpu

U = pgc.U
BIG = (45000, 2, 4096, 256)      # the C4 mesh and training batch: points, seed, rays, samples per ray
SMALL = (1500, 1, 37, 19)        # one small odd size


@pytest.fixture(scope="module")
def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


@pytest.fixture(scope="module")
def render():
    return importlib.import_module("tetra-nerf_amd.render")


_CACHE = {}


def _batch(tn, scenes, device, spec):
    """Matched samples of `spec` = (mesh points, mesh seed, rays, samples per ray): outside-in rays, S distances spread
    between each ray's entry and exit."""
    if spec in _CACHE:
        return _CACHE[spec]
    npts, seed, R, S = spec
    pts, cells = scenes.random_mesh(npts, seed)
    o, d = scenes.outside_in_rays(R, 1)
    tr = tn.TetrahedraTracer(device)
    verts = torch.from_numpy(pts).to(device)
    tr.load_tetrahedra(verts, torch.from_numpy(cells).to(device))
    to, td = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    M = 512
    out = tr.trace_rays(to, td, M)
    nv = out["num_visited_cells"]
    near = out["hit_distances"][:, 0, 0]
    far = torch.gather(out["hit_distances"][:, :, 1], 1, (nv[:, None].long() - 1).clamp_min(0))[:, 0]
    ts = ((torch.arange(S, device=device, dtype=torch.float32) + 0.5) / S)[None]
    dist = (near[:, None] * (1 - ts) + far[:, None] * ts).contiguous()
    m = tr.find_visited_cells(nv, out["visited_cells"], out["barycentric_coordinates"], out["hit_distances"],
                              out["vertex_indices"], dist)
    b = dict(tracer=tr, verts=verts, o=to, d=td, dist=dist, vi=m["vertex_indices"], bc=m["barycentric_coordinates"],
             mask=m["mask"], R=R, S=S, V=len(pts))
    assert int(b["mask"].sum()) > 0.5 * R * S
    _CACHE[spec] = b
    return b


def _check_bary_adjoint(geometry, got, vi, field_vm, rows, what):
    """(A) against the float64 contraction, in chunks of samples"""
    n, D = vi.shape
    Fd = field_vm.shape[1]
    worst = 0.0
    f64 = field_vm.double()
    for a in range(0, n, 1 << 17):
        sl = slice(a, a + (1 << 17))
        want = geometry.gather_backward_barycentrics(vi[sl], f64, rows[sl].double())
        ids = vi[sl].long()
        fr = f64[ids.clamp_min(0)].abs() * (ids >= 0)[..., None]
        bound = (2 * Fd + 2) * U * torch.einsum("nc,nkc->nk", rows[sl].double().abs(), fr[:, 1:] + fr[:, :1])
        err = (got[sl].double() - want).abs()
        assert bool(torch.isfinite(got[sl]).all()), what
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        bad = err > bound
        assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()))
    print(f"(A) {what}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("n", [BIG[2] * BIG[3], SMALL[2] * SMALL[3]])
@pytest.mark.parametrize("Fd", [3, 64, 80])
@pytest.mark.parametrize("D", [2, 3, 4, 6])
def test_bary_adjoint_stand_alone(tn, device, geometry, D, Fd, n):
    g = torch.Generator(device=device).manual_seed(100 * D + Fd)
    V = 45000 if n > 10000 else 1500
    field = torch.randn(Fd, V, device=device, generator=g)
    vi = torch.randint(0, V, (n, D), device=device, generator=g, dtype=torch.int32)
    vi[::13, 0] = -1                 # EMPTY rows are zero rows, in slot 0 too
    vi[5::17, D - 1] = -1
    rows = torch.randn(n, Fd, device=device, generator=g)
    got = tn.cpp.interpolate_values_backward_barycentrics(vi, field, rows)
    assert got.shape == (n, D - 1) and got.dtype == torch.float32
    _check_bary_adjoint(geometry, got, vi, field.t().contiguous(), rows, f"D={D} F={Fd} n={n}")


@pytest.mark.parametrize("spec", [BIG, SMALL])
def test_bary_adjoint_through_mlp_backward(tn, device, scenes, geometry, render, spec):
    b = _batch(tn, scenes, device, spec)
    R, S, V = b["R"], b["S"], b["V"]
    torch.manual_seed(4)
    mlp = render.TetraMLP().to(device)
    w = [p.detach() for p in render.mlp_weights(mlp)]
    field = torch.randn(64, V, device=device) * 0.5
    vi, bc = b["vi"], b["bc"]
    sigma, rgb, saved = tn.cpp.mlp_forward_gather_train(vi, bc, field, b["d"], w, S)
    saved.sigma = saved.rgb = None
    d_sigma, d_rgb = torch.randn(R * S, device=device), torch.randn(R * S, 3, device=device)
    plain = tn.cpp.mlp_backward(saved, vi, bc, field, b["d"], w, sigma, rgb, d_sigma, d_rgb)
    res = tn.cpp.mlp_backward(saved, vi, bc, field, b["d"], w, sigma, rgb, d_sigma, d_rgb, want_bary_grad=True, return_dx0=True)
    assert len(plain) == 2 and len(res) == 4
    grad_bary, dx0 = res[2], res[3]
    assert grad_bary.shape == (R * S, 3) and dx0.shape == (R * S, 64)
    # the twelve weight gradients do not depend on the switch (they are summed without atomics)
    for a, c in zip(plain[1], res[1]):
        assert torch.equal(a, c)
    _check_bary_adjoint(geometry, grad_bary, vi.reshape(-1, 4), field.t().contiguous(), dx0, f"mlp_backward {spec}")
    assert bool((grad_bary[~b["mask"].reshape(-1)] == 0).all())


def test_interpolate_values_gives_the_barycentric_gradient(tn, device, scenes, geometry):
    """`interpolate_values` with a leaf `barycentrics` that requires grad (None before this feature)."""
    b = _batch(tn, scenes, device, SMALL)
    torch.manual_seed(5)
    field = torch.randn(64, b["V"], device=device, requires_grad=True)
    bc = b["bc"].clone().requires_grad_(True)
    feats = tn.interpolate_values(b["vi"], bc, field)
    G = torch.randn_like(feats)
    (feats * G).sum().backward()
    assert bc.grad is not None and bc.grad.shape == bc.shape
    assert field.grad is not None
    _check_bary_adjoint(geometry, bc.grad.reshape(-1, 3), b["vi"].reshape(-1, 4), field.detach().t().contiguous(),
                        G.reshape(-1, 64).contiguous(), "interpolate_values autograd")
    # barycentrics alone
    bc2 = b["bc"].clone().requires_grad_(True)
    (tn.interpolate_values(b["vi"], bc2, field.detach()) * G).sum().backward()
    assert torch.equal(bc2.grad, bc.grad)


@pytest.mark.parametrize("spec", [BIG, SMALL])
def test_sample_positions_backward(tn, device, scenes, geometry, spec):
    """(B): grad_points per sample, then the vertex / origin / direction sums, atomic and deterministic."""
    b = _batch(tn, scenes, device, spec)
    R, S, V = b["R"], b["S"], b["V"]
    g = torch.Generator(device=device).manual_seed(7)
    gb = torch.randn(R, S, 3, device=device, generator=g)
    cpp = tn.cpp
    pts, go, gd, gv = cpp.sample_positions_backward(b["vi"], b["bc"], gb, b["verts"], b["dist"], want_points=True,
                                                    want_origins=True, want_directions=True, want_vertices=True)
    # -- grad_points
    m64, cond, present = pgc.m64_and_cond(b["vi"], b["verts"], gb)
    assert torch.equal(present, b["mask"].reshape(-1))
    m32 = pts.reshape(-1, 3)
    assert bool(torch.isfinite(m32).all())
    assert bool((m32[~present] == 0).all())
    bound_s = pgc.sample_bound(cond, m64)                           # [n]
    err_s = (m32.double() - m64).norm(dim=-1)
    ratio = float((err_s[present] / bound_s[present]).max())
    print(f"(B) {spec}: cond max {float(cond.max()):.3g}, worst ||m32 - m64|| / (8 u cond ||m64||) = {ratio:.3f}")
    assert bool((err_s <= bound_s).all()), (ratio, int((err_s > bound_s).sum()))
    # only some outputs asked for: the same bits
    p2, o2, d2, v2 = cpp.sample_positions_backward(b["vi"], b["bc"], gb, b["verts"], None, want_origins=True)
    assert p2 is None and d2 is None and v2 is None and torch.equal(o2, go)

    # -- sums: float64 over w32_k m64, m64 and t m64 (the forward's own weights)
    sums = pgc.sums_and_bounds(b["vi"], geometry.gather_weights(b["bc"].reshape(-1, 3)), m64, bound_s, present, b["dist"], R, S, V)
    want_v, bound_v, want_o, bound_o, want_d, bound_d = (sums[k] for k in ("want_v", "bound_v", "want_o", "bound_o", "want_d", "bound_d"))

    def check(name, got, want, bound):
        err = (got.double() - want).abs()
        print(f"(B) {spec} {name}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool(torch.isfinite(got).all()), name
        assert bool((err <= bound).all()), (name, int((err > bound).sum()), float(err.max()))
        assert bool((got[bound == 0] == 0).all()), name        # nothing lands where no live sample points

    check("origins", go, want_o, bound_o)
    check("directions", gd, want_d, bound_d)
    check("vertices (atomic)", gv, want_v, bound_v)
    # the deterministic vertex path: within the same bound, and bit-identical across two runs
    before = cpp.DETERMINISTIC_FIELD_GRADIENT
    cpp.DETERMINISTIC_FIELD_GRADIENT = True
    try:
        det = [cpp.sample_positions_backward(b["vi"], b["bc"], gb, b["verts"], b["dist"], want_vertices=True)[3] for _ in range(2)]
    finally:
        cpp.DETERMINISTIC_FIELD_GRADIENT = before
    check("vertices (deterministic)", det[0], want_v, bound_v)
    assert torch.equal(det[0], det[1])
    assert bool(((det[0].double() - gv.double()).abs() <= 2 * bound_v).all())


@pytest.mark.parametrize("spec", [BIG, SMALL])
def test_matcher_barycentrics_follow_the_stated_convention(tn, device, scenes, geometry, spec):
    """Convention pin: for matched samples in tets with cond2(T) <= 200 the matcher's barycentrics equal
    solve(T^T, o + t d - x0) in float64 within 1e-2 (a wrong vertex order or ray parameter gives errors of order 1; the
    fp32 estimate at this conditioning is below 1e-3).  At most 10 % of the matched samples may fall to the cond cut."""
    b = _batch(tn, scenes, device, spec)
    R, S = b["R"], b["S"]
    _, cond, present = pgc.m64_and_cond(b["vi"], b["verts"], torch.zeros(R, S, 3, device=device))
    keep = present & (cond <= 200)
    assert int(keep.sum()) >= 0.9 * int(present.sum()), (int(keep.sum()), int(present.sum()))
    p = (b["o"].double()[:, None, :] + b["dist"].double()[..., None] * b["d"].double()[:, None, :]).reshape(-1, 3)[keep]
    x = b["verts"].double()[b["vi"].reshape(-1, 4)[keep].long()]
    b64 = geometry.barycentrics_of(p.cpu(), x.cpu()).to(device)
    err = (b["bc"].reshape(-1, 3)[keep].double() - b64).abs()
    print(f"convention {spec}: {int(keep.sum())} of {int(present.sum())} matched samples, max |b - b64| = {float(err.max()):.3g}")
    assert float(err.max()) <= 1e-2


def _view_term64(render, dirs, g_enc):
    """J(dirs)^T g_enc with the Jacobian of render.direction_encoding in float64"""
    d = dirs.detach().double().requires_grad_(True)
    (out,) = torch.autograd.grad(render.direction_encoding(d), d, g_enc.double())
    return out


@pytest.mark.parametrize("fused", [True, False])
def test_render_train_position_gradients_wiring(tn, device, scenes, geometry, render, fused):
    """The leaf gradients of origins, directions and vertices equal geometry.py in float64 applied to the barycentric
    gradient of the same backward (hooked at capture["barycentric_positions"]), within the bounds of the sums.  The view
    term of `directions`: fused -- rebuilt from ray_head_bias.grad @ Wh[:, :27] through the float64 Jacobian of the encoding,
    allowed 500 u (|h| @ |Wh[:, :27]|) @ A with A the amplitude of each encoding column's derivative (2 pi f, or 1): 128 + 27
    terms of two fp32 dot products, plus <= 3 u |argument| <= 306 u of an amplitude for the fp32 argument of a cosine;
    unfused -- the `directions` gradient of the same call with the switch off (the same operators on the same bits)."""
    pts, cells = scenes.random_mesh(4000, 5)
    tr = tn.TetrahedraTracer(device)
    table = torch.from_numpy(pts).to(device)
    tr.load_tetrahedra(table, torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(300, 6)
    o[::29] = o[::29] + 10.0 * (o[::29] - 0.5)        # moved far out ...
    d[::29] = -d[::29]                                # ... and turned away: these rays miss the mesh
    S, S_fine, M = 32, 32, 256
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(device)
    field = ((torch.rand(64, len(pts), device=device) * 2 - 1) * 0.5).requires_grad_(True)
    rd = render.TetraRenderer(tr, field, mlp, S, M, fused=True, num_fine_samples=S_fine)
    to = torch.from_numpy(o).to(device).requires_grad_(True)
    td = torch.from_numpy(d).to(device).requires_grad_(True)
    verts = table.clone().requires_grad_(True)
    nv = tr.trace_rays(to.detach(), td.detach(), M)["num_visited_cells"]
    hit = int((nv > 0).sum())
    R = len(o)
    assert 0 < hit < R
    rand = {"coarse": torch.rand(hit, S + 1, device=device), "fine": torch.rand(hit, S_fine + 1, device=device)}
    target = torch.rand(R, 3, device=device)
    hb = torch.zeros(R, 128, device=device, requires_grad=True) if fused else None

    def loss_of(out):
        return ((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()

    cap, seen = {}, []
    out = rd.render_train(to, td, rand=rand, fused=fused, capture=cap, ray_head_bias=hb, position_gradients=True, vertices=verts)
    cap["barycentric_positions"].register_hook(lambda g: seen.append(g.detach().clone()))
    loss_of(out).backward()
    assert len(seen) == 1
    idx, vi, bc, S2 = cap["idx"], cap["vertex_indices"], cap["barycentric_coordinates"], cap["samples_per_ray"]
    r = idx.numel()
    assert r == hit and S2 == S + S_fine + 1
    dist = ((cap["edges"][:, 1:] + cap["edges"][:, :-1]) / 2)
    gb = seen[0].reshape(-1, 3)
    assert float(gb.abs().max()) > 0
    m64, cond, present = pgc.m64_and_cond(vi, table, gb)
    want = geometry.sample_positions_backward(vi.reshape(-1, 4), bc.reshape(-1, 3).double(), gb.double(), table.double(),
                                              dist.reshape(-1).double(), S2, weights=geometry.gather_weights(bc.reshape(-1, 3)).double())
    # bounds of the sums (see the module docstring)
    bound_s = 8 * U * cond * m64.norm(dim=-1)
    live = want["live"].double()
    w = geometry.gather_weights(bc.reshape(-1, 3)).double().abs() * live[:, None]
    ids = vi.reshape(-1, 4).long().clamp_min(0).reshape(-1)
    V = len(pts)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)     # noqa: E731
    abs_v = z(V, 3).index_add_(0, ids, (w[:, :, None] * want["points"].abs()[:, None, :]).reshape(-1, 3))
    cnt_v = z(V).index_add_(0, ids, live[:, None].expand(-1, 4).reshape(-1))
    bound_v = z(V).index_add_(0, ids, (w * bound_s[:, None]).reshape(-1))[:, None] + cnt_v[:, None] * U * abs_v
    t = dist.reshape(-1).double()
    n_live = live.reshape(r, S2).sum(1)[:, None]
    bound_o = bound_s.reshape(r, S2).sum(1)[:, None] + n_live * U * want["points"].abs().reshape(r, S2, 3).sum(1)
    bound_d = (t * bound_s).reshape(r, S2).sum(1)[:, None] + n_live * U * (t[:, None] * want["points"]).abs().reshape(r, S2, 3).sum(1)

    def check(name, got, expect, bound):
        err = (got.double() - expect).abs()
        print(f"wiring fused={fused} {name}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
              f"max |gradient| = {float(expect.abs().max()):.3g}")
        assert bool((err <= bound).all()), (name, int((err > bound).sum()), float(err.max()))

    check("vertices", verts.grad, want["vertices"], bound_v)
    check("origins", to.grad[idx], want["origins"], bound_o)
    missing = torch.ones(R, dtype=torch.bool, device=device)
    missing[idx] = False
    assert int(missing.sum()) == R - hit
    assert bool((to.grad[missing] == 0).all()) and bool((td.grad[missing] == 0).all())      # missing rays: exact zeros
    dirs = td.detach()[idx]
    if fused:
        Wh = render.mlp_weights(mlp)[8].detach()[:, :render.DIR_ENC]
        h = hb.grad[idx]
        view = _view_term64(render, dirs, h.double() @ Wh.double())
        freqs = 2.0 ** torch.linspace(0.0, 4.0, 4, dtype=torch.float64, device=device)
        amp = torch.zeros(render.DIR_ENC, 3, dtype=torch.float64, device=device)       # |d enc_j / d dir_c| <= amp[j, c]
        for c in range(3):
            amp[4 * c:4 * c + 4, c] = 2 * np.pi * freqs
            amp[12 + 4 * c:12 + 4 * c + 4, c] = 2 * np.pi * freqs
            amp[24 + c, c] = 1.0
        bound_view = 500 * U * ((h.double().abs() @ Wh.double().abs()) @ amp)
    else:
        td0 = td.detach().clone().requires_grad_(True)
        loss_of(rd.render_train(to.detach(), td0, rand=rand, fused=False)).backward()
        view = td0.grad[idx].double()
        bound_view = torch.zeros_like(view)
    expect = want["directions"] + view
    check("directions", td.grad[idx], expect, bound_d + bound_view + U * (want["directions"].abs() + view.abs()))
    assert float(view.abs().max()) > 0 and float(want["directions"].abs().max()) > 0

    if fused:
        # the sync-free form (no capture, no rand): padded rows and missing rays contribute exact zeros, nothing is non-finite
        to2 = to.detach().clone().requires_grad_(True)
        td2 = td.detach().clone().requires_grad_(True)
        v2 = table.clone().requires_grad_(True)
        torch.manual_seed(1)
        loss_of(rd.render_train(to2, td2, position_gradients=True, vertices=v2)).backward()
        for gname, gten in (("origins", to2.grad), ("directions", td2.grad), ("vertices", v2.grad)):
            assert bool(torch.isfinite(gten).all()), gname
        assert bool((to2.grad[missing] == 0).all()) and bool((td2.grad[missing] == 0).all())
        assert float(to2.grad.abs().max()) > 0 and float(v2.grad.abs().max()) > 0
        # the same batch through the compacting form with the SAME draws (the first `hit` rows of the [R, .] draws the
        # sync-free form makes): per ray the same kernels see the same samples, so the padded rows -- copies of the first
        # hitting ray, whose outputs are masked -- must have added exact zeros to that ray's gradient
        torch.manual_seed(1)
        full = {"coarse": torch.rand(R, S + 1, device=device), "fine": torch.rand(R, S_fine + 1, device=device)}
        rand3 = {k: v[:hit].contiguous() for k, v in full.items()}
        to3 = to.detach().clone().requires_grad_(True)
        loss_of(rd.render_train(to3, td.detach(), rand=rand3, position_gradients=True)).backward()
        first = int(idx[0])
        print(f"sync-free vs compacting: max |difference| of the origin gradients = {float((to3.grad - to2.grad).abs().max()):.3g}")
        assert torch.equal(to3.grad[first], to2.grad[first])


def test_off_is_off(tn, device, scenes, render):
    """position_gradients=False (the default): outputs and all thirteen gradients are bit-identical between a call made
    before and one made after a position-gradient call on the same renderer (deterministic mode, fixed draws)."""
    pts, cells = scenes.random_mesh(4000, 5)
    tr = tn.TetrahedraTracer(device)
    table = torch.from_numpy(pts).to(device)
    tr.load_tetrahedra(table, torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(256, 6)
    to, td = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    S, S_fine, M = 32, 32, 256
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(device)
    field = ((torch.rand(64, len(pts), device=device) * 2 - 1) * 0.5).requires_grad_(True)
    rd = render.TetraRenderer(tr, field, mlp, S, M, fused=True, num_fine_samples=S_fine)
    hit = int((tr.trace_rays(to, td, M)["num_visited_cells"] > 0).sum())
    rand = {"coarse": torch.rand(hit, S + 1, device=device), "fine": torch.rand(hit, S_fine + 1, device=device)}
    target = torch.rand(len(o), 3, device=device)
    params = [field] + list(render.mlp_weights(mlp))
    assert len(params) == 13

    def run(**kw):
        for p in params:
            p.grad = None
        out = rd.render_train(kw.pop("o", to), kw.pop("d", td), rand=rand, **kw)
        (((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()).backward()
        return [out[k].detach().clone() for k in ("rgb", "accumulation", "depth")] + [p.grad.clone() for p in params]

    before = tn.cpp.DETERMINISTIC_FIELD_GRADIENT
    tn.cpp.DETERMINISTIC_FIELD_GRADIENT = True
    try:
        first = run()
        o2, d2, v2 = to.clone().requires_grad_(True), td.clone().requires_grad_(True), table.clone().requires_grad_(True)
        on = run(o=o2, d=d2, position_gradients=True, vertices=v2)
        assert o2.grad is not None and d2.grad is not None and v2.grad is not None
        second = run()
    finally:
        tn.cpp.DETERMINISTIC_FIELD_GRADIENT = before
    for a, c in zip(first, second):
        assert torch.equal(a, c)
    # (the forward does not depend on the switch either)
    for a, c in zip(first[:3], on[:3]):
        assert torch.equal(a, c)
