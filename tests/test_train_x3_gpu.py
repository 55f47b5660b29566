"""The bf16x3 TRAINING forward (tn_mlp_forward_gather_train_ex mode 1, csrc/tn_mlp_x3_train.hip) on the GPU, and its way up to
render_train(mlp_mode="bf16x3") and the nerfstudio adapter (config.train_mlp_mode).

The kernel is k_mlp_forward_x3's arithmetic plus the saves of the fp32 training forward, so it is held to both: the outputs are
the inference kernel's BITS, the saved tensors have the fp32 training forward's LAYOUT (x0 even its bits: the gather is the same
statement), every saved layer follows from the one before it within the per-layer bound this arithmetic is already held to
(tests/test_render_gpu.py::test_bf16x3_error_bound_per_layer), and the unchanged fp32 adjoints give, on what it saved, the
float64 gradient under the saved ReLU decisions within that test's own bound (tests/test_train_gpu.py).

Shapes: the smallest at which the kernel takes each of its paths -- less than one 32-sample wave tile; a partial last 256-sample
group; more groups than the grid has blocks (302 > 256: some blocks run a second group)."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))

SETS = [(3, 7, 200), (300, 97, 5000), (300, 257, 5000)]
NAMES = ["field", "w1", "b1", "w2", "b2", "w3", "b3", "wd", "bd", "wh", "bh", "wr", "br"]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _decode_relu_masks(masks, n):
    """[4, n, 2] int64 -> bool [4, n, 128] in nn.Linear feature order: bit j of word (layer, sample, half h) = accumulator slot j =
    feature 32 (j >> 4) + (j & 3) + 8 ((j & 15) >> 2) + 4 h (the map tests/test_train_gpu.py::_decode_relu_masks states)."""
    import torch

    j = torch.arange(64, device=masks.device)
    bits = ((masks[..., None] >> j) & 1).bool()
    out = torch.empty(4, n, 128, dtype=torch.bool, device=masks.device)
    for h in range(2):
        out[:, :, 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * h] = bits[:, :, h, :]
    return out


def _quad_major(rows, n):
    """[F, n] slice of saved.acts, whose memory is quad-major [F / 4][n][4] (element (feature f, sample s) at ((f / 4) n + s) 4 +
    f % 4, include/tetranerf_hip.h) -> [n, F] in feature order"""
    F = rows.shape[0]
    return rows.reshape(F // 4, n, 4).permute(1, 0, 2).reshape(n, F)


_CACHE = {}


def _case(tn, device, R, S, V, biased):
    """inputs of one sample set (as in test_mlp_backward_matches_autograd) and the three forwards on them, computed once"""
    import torch

    key = (R, S, V, biased)
    if key in _CACHE:
        return _CACHE[key]
    render = importlib.import_module("tetra-nerf_amd.render")
    torch.manual_seed(1)
    n = R * S
    mlp = render.TetraMLP().to(device)
    for p in mlp.parameters():      # larger weights than the default init: every ReLU / softplus / sigmoid branch is live
        p.data.mul_(1.5)
    field = torch.randn(64, V, device=device) * 0.7
    vi = torch.randint(0, V, (n, 4), dtype=torch.int32, device=device)
    vi[::17, 2] = -1                # EMPTY vertices are skipped by the gather
    bc = (torch.rand(n, 3, device=device) / 3).contiguous()
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=device), dim=-1)
    bias = (torch.randn(R, 128, device=device) * 0.7) if biased else None
    w = [x.detach() for x in render.mlp_weights(mlp)]
    c = dict(n=n, S=S, w=w, field=field, vi=vi, bc=bc, dirs=dirs, bias=bias)
    c["plain"] = tn.cpp.mlp_forward_gather(vi, bc, field, dirs, w, S, mode="bf16x3", ray_head_bias=bias)
    c["x3"] = tn.cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, ray_head_bias=bias, mode="bf16x3")
    c["fp32"] = tn.cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, ray_head_bias=bias)
    torch.cuda.synchronize()
    _CACHE[key] = c
    return c


CASES = [(R, S, V, False) for R, S, V in SETS] + [SETS[-1] + (True,)]
IDS = [f"{R}x{S}{'-bias' if b else ''}" for R, S, V, b in CASES]


@pytest.mark.parametrize("R,S,V,biased", CASES, ids=IDS)
def test_same_forward_as_the_inference_kernel(tn, device, R, S, V, biased):
    import torch

    c = _case(tn, device, R, S, V, biased)
    sigma, rgb, saved = c["x3"]
    assert tuple(sigma.shape) == (c["n"],) and tuple(rgb.shape) == (c["n"], 3)
    assert torch.equal(sigma.view(torch.int32), c["plain"][0].view(torch.int32))
    assert torch.equal(rgb.view(torch.int32), c["plain"][1].view(torch.int32))
    assert bool(torch.isfinite(sigma).all()) and float(sigma.max()) > 0
    if biased:     # the bias acts, on the colours only
        nb = _case(tn, device, R, S, V, False)["x3"]
        assert torch.equal(sigma, nb[0]) and float((rgb - nb[1]).abs().max()) > 1e-2


@pytest.mark.parametrize("R,S,V,biased", CASES, ids=IDS)
def test_saved_x0_is_the_fp32_forwards(tn, device, R, S, V, biased):
    import torch

    c = _case(tn, device, R, S, V, biased)
    n = c["n"]
    x0 = _quad_major(c["x3"][2].acts[0:64], n)
    want = _quad_major(c["fp32"][2].acts[0:64], n)
    assert torch.equal(x0.view(torch.int32), want.view(torch.int32))
    # (and it IS the gather, in feature order: against float64)
    f64, b64 = c["field"].double(), c["bc"].double()
    wts = torch.cat([1 - b64.sum(-1, keepdim=True), b64], -1)
    wts = torch.where(c["vi"] < 0, torch.zeros_like(wts), wts)
    g64 = (f64.t()[c["vi"].long().clamp_min(0)] * wts[..., None]).sum(1)
    assert float((x0.double() - g64).abs().max()) < 1e-5


@pytest.mark.parametrize("R,S,V,biased", CASES, ids=IDS)
def test_masks_are_the_saved_activations_signs(tn, device, R, S, V, biased):
    import torch

    c = _case(tn, device, R, S, V, biased)
    n = c["n"]
    saved = c["x3"][2]
    masks = _decode_relu_masks(saved.masks, n)
    for l in range(4):
        h = _quad_major(saved.acts[64 + 128 * l:192 + 128 * l], n)
        assert bool((h >= 0).all()), l
        nz = h.view(torch.int32) != 0                      # mask_of: "positive" = "bit pattern not zero"
        assert torch.equal(masks[l], nz), (l, int((masks[l] != nz).sum()))
        assert 0.05 < float(nz.float().mean()) < 0.95, l     # both branches live


@pytest.mark.parametrize("R,S,V,biased", CASES, ids=IDS)
def test_every_saved_layer_follows_from_the_one_before(tn, device, R, S, V, biased):
    """float64 value of the SAVED input through the layer's (fp32-representable) weights, after ReLU, against the saved output:
    |h - h64| <= 2^-21 (|W| |x| + |b| [+ |bias|]) + 4e-7 |h64| (ReLU is 1-Lipschitz: the pre-activation's bound carries over).
    A layout error anywhere -- a quad in the wrong place, a slot permutation, a stale row of a lane beyond n -- is O(1) here.
    The head layer's first 27 inputs are the fp32 direction encoding (render.direction_encoding in float32: the statement the
    kernel's k_dir_encoding32 evaluates, operation for operation), an INPUT of the layer like the saved h3."""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    c = _case(tn, device, R, S, V, biased)
    n, w = c["n"], [x.double() for x in c["w"]]
    sigma, _, saved = c["x3"]
    acts = [_quad_major(saved.acts[0:64], n).double()] + [_quad_major(saved.acts[64 + 128 * l:192 + 128 * l], n).double() for l in range(4)]

    def check(name, x, W, b, extra, got):
        pre = x @ W.t() + b + (0 if extra is None else extra)
        h64 = pre.clamp_min(0)
        bound = 2.0 ** -21 * (x.abs() @ W.abs().t() + b.abs() + (0 if extra is None else extra.abs())) + 4e-7 * h64.abs()
        err = (got - h64).abs()
        print(f"{name}: max |h - h64| / bound = {float((err / bound).max()):.3f}, max |h - h64| = {float(err.max()):.2e}")
        assert bool((err <= bound).all()), (name, float((err / bound).max()))

    check("layer 1", acts[0], w[0], w[1], None, acts[1])
    check("layer 2", acts[1], w[2], w[3], None, acts[2])
    check("layer 3", acts[2], w[4], w[5], None, acts[3])
    enc = render.direction_encoding(c["dirs"]).double()[:, None, :].expand(-1, S, -1).reshape(n, 27)
    ray_bias = None if c["bias"] is None else c["bias"].double()[:, None, :].expand(-1, S, -1).reshape(n, 128)
    check("head layer", torch.cat([enc, acts[3]], -1), w[8], w[9], ray_bias, acts[4])
    # density head on the saved h3: softplus^-1(sigma), where it is well-conditioned
    y64 = (acts[3] @ w[6].t() + w[7])[:, 0]
    bound = 2.0 ** -21 * ((acts[3].abs() @ w[6].abs().t())[:, 0] + w[7].abs()) + 4e-7 * y64.abs()
    s = sigma.double()
    y = torch.where(s > 20, s, torch.log(torch.expm1(s.clamp_min(1e-30))))
    ok = s > 1e-3
    err = (y - y64).abs()
    print(f"density head: {int(ok.sum())} of {n} samples, max err / bound = {float((err[ok] / bound[ok]).max()):.3f}")
    assert int(ok.sum()) > n // 4
    assert bool((err[ok] <= bound[ok]).all()), float((err[ok] / bound[ok]).max())


@pytest.fixture(scope="module")
def scene(tn, device, scenes):
    """512 rays into the 4000-point mesh (tests/test_train_gpu.py's)"""
    import torch

    pts, cells = scenes.random_mesh(4000, 5)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(512, 6)
    to, td = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    hit = int((tr.trace_rays(to, td, 256)["num_visited_cells"] > 0).sum())
    return dict(pts=pts, tracer=tr, o=to, d=td, hit=hit)


def test_gradients_match_float64_under_the_masks_the_bf16x3_forward_saved(tn, device, scene):
    """tests/test_train_gpu.py::test_training_gradients_match_float64_under_the_saved_relu_masks, configuration (24, 24, True,
    True), with the bf16x3 forward: the float64 statement under the masks THIS forward saved, against the fused gradients =
    the bf16x3 forward followed by the unchanged fp32 adjoints.  Same bound (< max(5 t32, 5e-6) on all 13 tensors), same cap on
    the ReLU decisions that differ from float64's own (32 per layer)."""
    import torch
    from test_train_gpu import _statement

    render = importlib.import_module("tetra-nerf_amd.render")
    cpp = tn.cpp
    tr, to, td, hit = scene["tracer"], scene["o"], scene["d"], scene["hit"]
    torch.manual_seed(123)
    target = torch.rand(len(to), 3, device=device)
    S, S_fine, biased, scaling = 24, 24, True, True
    torch.manual_seed(0)
    mlp = render.TetraMLP().to(device)
    field = ((torch.rand(64, len(scene["pts"]), device=device) * 2 - 1) * 0.5)
    rd = render.TetraRenderer(tr, field, mlp, S, 256, fused=True, num_fine_samples=S_fine, biased=biased)
    rand = {"coarse": torch.rand(hit, S + 1, device=device), "fine": torch.rand(hit, S_fine + 1, device=device)}
    cap = {}
    with torch.no_grad():
        rd.render_train(to, td, gradient_scaling=scaling, rand=rand, fused=True, capture=cap, mlp_mode="bf16x3")
    vi, bc, edges, S2, dirs = cap["vertex_indices"], cap["barycentric_coordinates"], cap["edges"], cap["samples_per_ray"], cap["dirs"]
    n = vi.numel() // 4
    w = [x.detach() for x in render.mlp_weights(mlp)]
    sigma, rgb, saved = cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S2, mode="bf16x3")
    masks = _decode_relu_masks(saved.masks.clone(), n)
    # upstream gradients: the float64 composite + loss at the fused forward's outputs
    dt = torch.float64
    sg = sigma.detach().to(dt).view(-1, S2, 1).requires_grad_(True)
    cl = rgb.detach().to(dt).view(-1, S2, 3).requires_grad_(True)
    e64 = edges.to(dt)
    spacing = (e64 - cap["near"].to(dt)) / (cap["far"].to(dt) - cap["near"].to(dt))
    cl2, sg2, _ = render.GradientScaler.apply(cl, sg, (spacing[:, 1:] + spacing[:, :-1])[..., None])
    rgb_r, acc_r, _, _ = render.composite(sg2, cl2, e64[:, :-1, None], e64[:, 1:, None])
    full_rgb = torch.ones(len(to), 3, dtype=dt, device=device).index_copy(0, cap["idx"], rgb_r)
    full_acc = torch.zeros(len(to), 1, dtype=dt, device=device).index_copy(0, cap["idx"], acc_r)
    (((full_rgb - target.to(dt)) ** 2).mean() + 0.1 * full_acc.mean()).backward()
    d_sigma, d_rgb = sg.grad.reshape(-1), cl.grad.reshape(-1, 3)
    gf, gw = cpp.mlp_backward(saved, vi, bc, field, dirs, w, sigma, rgb, d_sigma.float().contiguous(), d_rgb.float().contiguous())
    fused = [gf] + list(gw)
    assert len(fused) == 13
    res = {}
    for label, dtype, mk in (("f64 masked", torch.float64, masks), ("f32 masked", torch.float32, masks), ("f64 own", torch.float64, None)):
        s_, c_, leaves, natural = _statement(render, device, mlp, field, vi.reshape(n, 4), bc.reshape(n, 3), dirs, S2, mk, dtype)
        ((s_ * d_sigma.to(dtype)).sum() + (c_ * d_rgb.to(dtype)).sum()).backward()
        res[label] = ([x.grad for x in leaves], natural)
    flipped = (masks != res["f64 own"][1]).sum(dim=(1, 2)).tolist()
    print(f"bf16x3 forward, config {(S, S_fine, biased, scaling)}: {n} samples, ReLU decisions differing from float64's own per layer "
          f"(of {n * 128}): {flipped}")
    assert max(flipped) <= 32, flipped
    for k, name in enumerate(NAMES):
        ours, t32 = _rel(fused[k], res["f64 masked"][0][k]), _rel(res["f32 masked"][0][k], res["f64 masked"][0][k])
        print(f"  {name}: fused {ours:.2e}, float32 autograd {t32:.2e}")
        assert ours < max(5.0 * t32, 5e-6), (name, ours, t32)


def _train_setup(render, device, scene, seed=0, **kw):
    import torch

    torch.manual_seed(seed)
    mlp = render.TetraMLP().to(device)
    field = ((torch.rand(64, len(scene["pts"]), device=device) * 2 - 1) * 0.5).requires_grad_(True)
    S, S_fine = 24, 24
    rd = render.TetraRenderer(scene["tracer"], field, mlp, S, 256, fused=True, num_fine_samples=S_fine, biased=True, **kw)
    hit = scene["hit"]
    rand = {"coarse": torch.rand(hit, S + 1, device=device), "fine": torch.rand(hit, S_fine + 1, device=device)}
    target = torch.rand(len(scene["o"]), 3, device=device)
    params = [field] + list(render.mlp_weights(mlp))
    assert len(params) == 13

    def run(**call_kw):
        for p in params:
            p.grad = None
        out = rd.render_train(scene["o"], scene["d"], gradient_scaling=True, rand=rand, **call_kw)
        (((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()).backward()
        return {k: out[k].detach().clone() for k in ("rgb", "accumulation", "depth", "ray_mask")}, [p.grad.clone() for p in params]

    run.rand = rand
    return rd, run


def test_render_train_bf16x3_against_fp32(tn, device, scene):
    """End to end: the coarse density pass and the recorded fine node in bf16x3 against the default call, same draws: 1e-5, the
    bar of every bf16x3-versus-fp32 comparison here."""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    rd, run = _train_setup(render, device, scene)
    want, _ = run()
    got, grads = run(mlp_mode="bf16x3")
    assert torch.equal(got["ray_mask"], want["ray_mask"]) and int(want["ray_mask"].sum()) > 300
    for k in ("rgb", "accumulation"):
        err = float((got[k] - want[k]).abs().max())
        print(f"{k}: max |bf16x3 - fp32| = {err:.2e}")
        assert err <= 1e-5, (k, err)
    assert float(want["accumulation"].max()) > 0.5
    assert not torch.equal(got["rgb"], want["rgb"])          # (another arithmetic did run)
    for name, g in zip(NAMES, grads):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    # a renderer whose train_mlp_mode is bf16x3 takes the same path as the per-call override, and "fp32" per call overrides it
    rd.train_mlp_mode = "bf16x3"
    again, _ = run()
    back, _ = run(mlp_mode="fp32")
    rd.train_mlp_mode = "fp32"
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(again[k], got[k]) and torch.equal(back[k], want[k]), k
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        run(mlp_mode="tf32")


def test_no_graph_training_forward_in_bf16x3(tn, device, scene):
    """render_train under no_grad runs the non-saving kernels; in bf16x3 they are the same arithmetic as the recorded node, so
    the outputs are its bits"""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    rd, run = _train_setup(render, device, scene)
    recorded, _ = run(mlp_mode="bf16x3")
    with torch.no_grad():
        out = rd.render_train(scene["o"], scene["d"], gradient_scaling=True, rand=run.rand, mlp_mode="bf16x3")
    assert not out["rgb"].requires_grad
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(out[k], recorded[k]), k


def test_off_is_off(tn, device, scene):
    """The default (fp32) training call gives the same bits -- outputs and all thirteen gradients, deterministic mode, fixed draws
    -- before and after a bf16x3 call on the same renderer; and mlp_mode="bf16x3" (render()'s switch) without train_mlp_mode
    trains bit-identically to mlp_mode="fp32"."""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    before = tn.cpp.DETERMINISTIC_FIELD_GRADIENT
    tn.cpp.DETERMINISTIC_FIELD_GRADIENT = True
    try:
        rd, run = _train_setup(render, device, scene)
        first = run()
        run(mlp_mode="bf16x3")
        second = run()
        rd3, run3 = _train_setup(render, device, scene, mlp_mode="bf16x3")
        assert rd3.mlp_mode == "bf16x3" and rd3.train_mlp_mode == "fp32"
        third = run3()
    finally:
        tn.cpp.DETERMINISTIC_FIELD_GRADIENT = before
    for other in (second, third):
        for k in ("rgb", "accumulation", "depth"):
            assert torch.equal(first[0][k], other[0][k]), k
        for name, a, c in zip(NAMES, first[1], other[1]):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), name


def test_adapter_trains_in_bf16x3_when_the_config_says_so(tn, device, scenes):
    """nerfstudio adapter: a reference TetrahedraNerf (tests/golden/reference_model.py) whose config carries train_mlp_mode =
    "bf16x3", in training mode, against the same model without the field under the same seed: 1e-5, gradients on every parameter."""
    import torch
    import reference_model as rm

    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    plugin.install(ref.TetrahedraNerf)
    try:
        pts, cells = scenes.random_mesh(6000, 31)
        model = rm.build_model(ref, pts, cells, num_samples=48, num_fine_samples=48).to(device).train()
        assert not hasattr(model.config, "train_mlp_mode")
        o, d = scenes.outside_in_rays(1024, 33)
        rb = rm.ray_bundle(ref, o, d, device, camera_indices=np.arange(len(o)) % 3)
        target = torch.rand(len(o), 3, device=device)
        params = [model.tetrahedra_field] + plugin.weights_from_model(model)

        def step():
            for p in params:
                p.grad = None
            torch.manual_seed(7)
            out = model(rb)
            (((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()).backward()
            return {k: out[k].detach().clone() for k in ("rgb", "accumulation")}, [p.grad for p in params]

        want, _ = step()
        model.config.train_mlp_mode = "bf16x3"
        got, grads = step()
        for k in ("rgb", "accumulation"):
            err = float((got[k] - want[k]).abs().max())
            print(f"adapter {k}: max |bf16x3 - fp32| = {err:.2e}")
            assert err <= 1e-5, (k, err)
        assert not torch.equal(got["rgb"], want["rgb"])
        assert float(want["accumulation"].max()) > 0.5
        for name, g in zip(NAMES, grads):
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    finally:
        plugin.uninstall(ref.TetrahedraNerf)
