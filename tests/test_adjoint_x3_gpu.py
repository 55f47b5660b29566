"""The bf16x3 dX chain (tn_mlp_backward_ex mode 1, csrc/tn_mlp_x3_bwd.hip) on the GPU, and its way up to
render_train(adjoint_mode="bf16x3") and the nerfstudio adapter (config.train_adjoint_mode).

The kernel is k_mlp_backward with its four matrix products in the split-operand bf16 arithmetic, so it is held to both: what
the VALU computes (dhead, d4) are the fp32 kernel's BITS, the outputs have its LAYOUTS, and every produced layer follows from
the stored one before it within the per-layer bound this arithmetic is already held to
(tests/test_render_gpu.py::test_bf16x3_error_bound_per_layer, tests/test_train_x3_gpu.py). Mode 0 of the new entry is the old
entry, bit for bit.

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
PARTS = ("d1", "d2", "d3", "d4", "dhead", "dx0")


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
    """[F, n] slice whose memory is quad-major [F / 4][n][4] (element (feature f, sample s) at ((f / 4) n + s) 4 + f % 4,
    include/tetranerf_hip.h) -> [n, F] in feature order"""
    F = rows.shape[0]
    return rows.reshape(F // 4, n, 4).permute(1, 0, 2).reshape(n, F)


def _raw_chain(tn, c, fwd, mode):
    """the dX chain alone through the C entry itself: mode None = tn_mlp_backward, otherwise tn_mlp_backward_ex(mode); the six
    outputs on NaN-filled buffers (a value the kernel failed to write shows)"""
    import ctypes as C

    import torch

    cpp = tn.cpp
    lib = cpp._lib.load()
    sigma, rgb, saved = fwd
    n = c["n"]
    dev = sigma.device
    buf = torch.full((4 * 128 + 4, n), float("nan"), dtype=torch.float32, device=dev)
    rows = torch.full((n, 64), float("nan"), dtype=torch.float32, device=dev)
    bs = cpp._backward_buffers(saved.acts, saved.masks, buf, rows)
    mh = cpp.fused_mlp(c["w"])
    head = (mh.handle, n, sigma.data_ptr(), rgb.data_ptr(), c["d_sigma"].data_ptr(), c["d_rgb"].data_ptr(), C.byref(bs))
    stream = cpp._stream(dev)
    if mode is None:
        cpp._lib.check(lib.tn_mlp_backward(*head, stream))
    else:
        cpp._lib.check(lib.tn_mlp_backward_ex(*head, mode, stream))
    torch.cuda.synchronize()
    return dict(d1=buf[0:128], d2=buf[128:256], d3=buf[256:384], d4=buf[384:512], dhead=buf[512:516], dx0=rows)


def _public_chain(tn, c, fwd, adjoint_mode):
    sigma, rgb, saved = fwd
    res = tn.cpp.mlp_backward(saved, c["vi"], c["bc"], c["field"], c["dirs"], c["w"], sigma, rgb, c["d_sigma"], c["d_rgb"],
                              adjoint_mode=adjoint_mode, return_chain=True)
    assert len(res) == 3
    ch = res[2]
    return {k: getattr(ch, k).clone() for k in PARTS}


_CACHE = {}


def _case(tn, device, R, S, V, biased, forward):
    """inputs of one sample set (as in tests/test_train_x3_gpu.py::_case), the training forward on them in `forward`'s arithmetic,
    seeded upstream gradients at a realistic loss scale, and the chains every test below reads -- computed once"""
    import torch

    key = (R, S, V, biased, forward)
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
    torch.manual_seed(2)
    d_sigma = (torch.randn(n, device=device) * 1e-3).contiguous()
    d_rgb = (torch.randn(n, 3, device=device) * 1e-3).contiguous()
    c = dict(n=n, S=S, w=w, field=field, vi=vi, bc=bc, dirs=dirs, bias=bias, d_sigma=d_sigma, d_rgb=d_rgb)
    fwd = tn.cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S, ray_head_bias=bias, mode=forward)
    c["fwd"] = fwd
    c["old"] = _raw_chain(tn, c, fwd, None)
    c["ex0"] = _raw_chain(tn, c, fwd, 0)
    c["x3"] = _raw_chain(tn, c, fwd, 1)
    c["x3 again"] = _raw_chain(tn, c, fwd, 1)
    c["public fp32"] = _public_chain(tn, c, fwd, "fp32")
    c["public x3"] = _public_chain(tn, c, fwd, "bf16x3")
    torch.cuda.synchronize()
    _CACHE[key] = c
    return c


CASES = [(R, S, V, False, "fp32") for R, S, V in SETS] + [SETS[-1] + (True, "fp32"), SETS[1] + (False, "bf16x3")]
IDS = [f"{R}x{S}{'-bias' if b else ''}-{f}" for R, S, V, b, f in CASES]


def _same_bits(a, b):
    import torch

    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("R,S,V,biased,forward", CASES, ids=IDS)
def test_mode_0_is_the_old_entry(tn, device, R, S, V, biased, forward):
    import torch

    c = _case(tn, device, R, S, V, biased, forward)
    for k in PARTS:
        assert bool(torch.isfinite(c["old"][k]).all()), k          # (every value was written)
        assert _same_bits(c["ex0"][k], c["old"][k]), k
        assert _same_bits(c["public fp32"][k], c["old"][k]), k     # mlp_backward's default goes there too
        assert _same_bits(c["public x3"][k], c["x3"][k]), k        # and adjoint_mode="bf16x3" is mode 1
    assert float(c["old"]["dx0"].abs().max()) > 0


def test_other_modes_are_refused(tn, device):
    c = _case(tn, device, *CASES[0])
    for mode in (2, 3, -1):
        with pytest.raises(RuntimeError, match="mlp mode must be"):
            _raw_chain(tn, c, c["fwd"], mode)
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        _public_chain(tn, c, c["fwd"], "bf16")


@pytest.mark.parametrize("R,S,V,biased,forward", CASES, ids=IDS)
def test_what_the_valu_computes_did_not_move(tn, device, R, S, V, biased, forward):
    c = _case(tn, device, R, S, V, biased, forward)
    assert _same_bits(c["x3"]["dhead"], c["old"]["dhead"])
    assert _same_bits(c["x3"]["d4"], c["old"]["d4"])
    # (and another arithmetic did run behind them)
    assert not _same_bits(c["x3"]["d3"], c["old"]["d3"])
    assert not _same_bits(c["x3"]["dx0"], c["old"]["dx0"])


@pytest.mark.parametrize("R,S,V,biased,forward", CASES, ids=IDS)
def test_every_produced_layer_follows_from_the_one_before(tn, device, R, S, V, biased, forward):
    """float64 product of the chain's own STORED d_{l+1} with the (fp32-representable) weights, masked by the saved ReLU mask,
    against the stored d_l: |d - d64| <= 2^-21 (|d_{l+1}| @ |W| [+ |d sigma_raw| |wd|]) + 4e-7 |d64|, and exactly 0 where the mask
    bit is clear.  A misplaced quad, a wrong K permutation in the transposed pack or a stale lane beyond n is O(1) here."""
    import torch

    c = _case(tn, device, R, S, V, biased, forward)
    n, w = c["n"], [x.double() for x in c["w"]]
    ch = c["x3"]
    masks = _decode_relu_masks(c["fwd"][2].masks, n)
    d4, d3, d2, d1 = (_quad_major(ch[k], n).double() for k in ("d4", "d3", "d2", "d1"))
    dx0 = ch["dx0"].double()
    dsr = ch["dhead"][0].double()[:, None]

    def check(name, d_in, W, mask, got, extra=None, extra_abs=None):
        d64 = d_in @ W + (0 if extra is None else extra)
        bound = 2.0 ** -21 * (d_in.abs() @ W.abs() + (0 if extra_abs is None else extra_abs))
        if mask is not None:
            d64 = d64 * mask
            assert bool((got[~mask] == 0).all()), name
        bound = bound + 4e-7 * d64.abs()
        err = (got - d64).abs()
        if mask is not None:
            err, bound = err[mask], bound[mask]
        print(f"{name}: max |d - d64| / bound = {float((err / bound).max()):.3f}, max |d - d64| = {float(err.max()):.2e}, "
              f"max |d64| = {float(d64.abs().max()):.2e}")
        assert float(d64.abs().max()) > 0
        assert bool((err <= bound).all()), (name, float((err / bound).max()))

    wd = w[6]                                     # [1, 128]
    check("d3", d4, w[8][:, 27:], masks[2], d3, extra=dsr * wd, extra_abs=dsr.abs() * wd.abs())
    check("d2", d3, w[4], masks[1], d2)
    check("d1", d2, w[2], masks[0], d1)
    check("dx0", d1, w[0], None, dx0)
    # d4 itself, the fp32 VALU statement: ReLU'(h4) Wr^T d rgb_raw (three products per value: a few fp32 roundings)
    drr = ch["dhead"][1:4].double().t()
    d4_64 = (drr @ w[10]) * masks[3]
    assert bool((d4[~masks[3]] == 0).all())
    assert float((d4 - d4_64).abs().max()) <= 4e-7 * float((drr.abs() @ w[10].abs()).max())


@pytest.mark.parametrize("R,S,V,biased,forward", CASES, ids=IDS)
def test_deterministic(tn, device, R, S, V, biased, forward):
    c = _case(tn, device, R, S, V, biased, forward)
    for k in PARTS:
        assert _same_bits(c["x3 again"][k], c["x3"][k]), k


@pytest.fixture(scope="module")
def scene(tn, device, scenes):
    """512 rays into the 4000-point mesh (tests/test_train_gpu.py's)"""
    import torch

    pts, cells = scenes.random_mesh(4000, 5)
    tr = tn.TetrahedraTracer(device)
    table = torch.from_numpy(pts).to(device)
    tr.load_tetrahedra(table, torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(512, 6)
    to, td = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    hit = int((tr.trace_rays(to, td, 256)["num_visited_cells"] > 0).sum())
    return dict(pts=pts, table=table, tracer=tr, o=to, d=td, hit=hit)


@pytest.mark.parametrize("forward", ["fp32", "bf16x3"])
def test_gradients_match_float64_under_the_saved_masks(tn, device, scene, forward):
    """tests/test_train_x3_gpu.py::test_gradients_match_float64_under_the_masks_the_bf16x3_forward_saved with the bf16x3 dX
    chain: same scene, configuration (24, 24, True, True), same float64 statement under the masks the forward saved.  Same
    bound: all 13 gradients < max(5 x float32 autograd, 5e-6) of the float64 statement."""
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
        rd.render_train(to, td, gradient_scaling=scaling, rand=rand, fused=True, capture=cap, mlp_mode=forward)
    vi, bc, edges, S2, dirs = cap["vertex_indices"], cap["barycentric_coordinates"], cap["edges"], cap["samples_per_ray"], cap["dirs"]
    n = vi.numel() // 4
    w = [x.detach() for x in render.mlp_weights(mlp)]
    sigma, rgb, saved = cpp.mlp_forward_gather_train(vi, bc, field, dirs, w, S2, mode=forward)
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
    gf, gw = cpp.mlp_backward(saved, vi, bc, field, dirs, w, sigma, rgb, d_sigma.float().contiguous(), d_rgb.float().contiguous(),
                              adjoint_mode="bf16x3")
    fused = [gf] + list(gw)
    assert len(fused) == 13
    res = {}
    for label, dtype in (("f64 masked", torch.float64), ("f32 masked", torch.float32)):
        s_, c_, leaves, _ = _statement(render, device, mlp, field, vi.reshape(n, 4), bc.reshape(n, 3), dirs, S2, masks, dtype)
        ((s_ * d_sigma.to(dtype)).sum() + (c_ * d_rgb.to(dtype)).sum()).backward()
        res[label] = [x.grad for x in leaves]
    print(f"{forward} forward, bf16x3 dX chain, config {(S, S_fine, biased, scaling)}: {n} samples")
    ratios = []
    for k, name in enumerate(NAMES):
        ours, t32 = _rel(fused[k], res["f64 masked"][k]), _rel(res["f32 masked"][k], res["f64 masked"][k])
        ratios.append((name, ours, t32))
        print(f"  {name}: fused {ours:.2e}, float32 autograd {t32:.2e}")
    for name, ours, t32 in ratios:
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

    def run(o=None, d=None, **call_kw):
        for p in params:
            p.grad = None
        out = rd.render_train(scene["o"] if o is None else o, scene["d"] if d is None else d, gradient_scaling=True, rand=rand, **call_kw)
        (((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()).backward()
        return {k: out[k].detach().clone() for k in ("rgb", "accumulation", "depth", "ray_mask")}, [p.grad.clone() for p in params]

    return rd, run


def _tensor_rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def test_render_train_end_to_end_and_off_is_off(tn, device, scene):
    """render_train(adjoint_mode="bf16x3") against the default call on the same draws (deterministic field gradient): the outputs
    are the default's BITS (the adjoint mode does not touch the forward); the 13 gradients are finite, nonzero, not bit-equal, and
    within 1e-5 of the default's relative to each tensor's max -- twice the 5e-6 floor of the float64 test above, both adjoints
    seeing the same masks.  The renderer's train_adjoint_mode takes the same path, "fp32" per call overrides it, and a default
    call afterwards gives the default's bits again."""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    before = tn.cpp.DETERMINISTIC_FIELD_GRADIENT
    tn.cpp.DETERMINISTIC_FIELD_GRADIENT = True
    try:
        rd, run = _train_setup(render, device, scene)
        assert rd.train_adjoint_mode == "fp32"
        want, want_g = run()
        got, got_g = run(adjoint_mode="bf16x3")
        rd.train_adjoint_mode = "bf16x3"
        again, again_g = run()
        back, back_g = run(adjoint_mode="fp32")
        rd.train_adjoint_mode = "fp32"
        after, after_g = run()
        rd2, run2 = _train_setup(render, device, scene, train_adjoint_mode="bf16x3")
        assert rd2.train_adjoint_mode == "bf16x3" and rd2.train_mlp_mode == "fp32"
        built, built_g = run2()
        # independent of the forward's mode: both in bf16x3
        both, both_g = run(mlp_mode="bf16x3", adjoint_mode="bf16x3")
        x3fwd, x3fwd_g = run(mlp_mode="bf16x3")
        with pytest.raises(RuntimeError, match="mlp mode must be"):
            run(adjoint_mode="bf16")
    finally:
        tn.cpp.DETERMINISTIC_FIELD_GRADIENT = before
    assert int(want["ray_mask"].sum()) > 300 and float(want["accumulation"].max()) > 0.5
    for k in ("rgb", "accumulation", "depth", "ray_mask"):
        for other in (got, again, back, after, built):
            assert torch.equal(other[k], want[k]), k
        assert torch.equal(both[k], x3fwd[k]), k
    differ = 0
    for name, g, wg, ag, bg_, fg, ug in zip(NAMES, got_g, want_g, again_g, back_g, after_g, built_g):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        rel = _tensor_rel(g, wg)
        print(f"{name}: max |bf16x3 adjoint - fp32 adjoint| / max |fp32| = {rel:.2e}")
        assert rel <= 1e-5, (name, rel)
        differ += int(not _same_bits(g, wg))
        assert _same_bits(ag, g) and _same_bits(ug, g), name            # the renderer's switch = the per-call override
        assert _same_bits(bg_, wg) and _same_bits(fg, wg), name        # off is off
    # (dhead and d4 are the fp32 kernel's bits, so wr / br / bh and the like may coincide; the tensors behind a bf16x3 product do not)
    assert differ >= 7 and not _same_bits(got_g[0], want_g[0]), differ
    for name, g, wg in zip(NAMES, both_g, x3fwd_g):
        rel = _tensor_rel(g, wg)
        assert bool(torch.isfinite(g).all()) and rel <= 1e-5, (name, rel)
    assert not _same_bits(both_g[0], x3fwd_g[0])


def test_position_gradients_with_the_bf16x3_adjoint(tn, device, scene):
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    rd, run = _train_setup(render, device, scene)
    grads = {}
    for mode in ("fp32", "bf16x3"):
        o2, d2 = scene["o"].clone().requires_grad_(True), scene["d"].clone().requires_grad_(True)
        v2 = scene["table"].clone().requires_grad_(True)
        run(o=o2, d=d2, position_gradients=True, vertices=v2, adjoint_mode=mode)
        assert o2.grad is not None and d2.grad is not None and v2.grad is not None
        grads[mode] = (o2.grad.clone(), d2.grad.clone())
    for name, g, wg in zip(("origins", "directions"), grads["bf16x3"], grads["fp32"]):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        rel = _tensor_rel(g, wg)
        print(f"{name}: max |bf16x3 adjoint - fp32 adjoint| / max |fp32| = {rel:.2e}")
        assert rel <= 1e-5, (name, rel)


def test_adapter_trains_with_the_bf16x3_adjoint_when_the_config_says_so(tn, device, scenes):
    """nerfstudio adapter: a reference TetrahedraNerf (tests/golden/reference_model.py) whose config carries train_adjoint_mode =
    "bf16x3", in training mode, against the same model without the field under the same seed: the same outputs, gradients on
    every parameter within 1e-5 of the default's relative to each tensor's max (both adjoints see the same forward and masks;
    what differs is four matrix products held to 2^-21 of their magnitude sums) and not bit-equal to them."""
    import torch
    import reference_model as rm

    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    plugin.install(ref.TetrahedraNerf)
    try:
        pts, cells = scenes.random_mesh(6000, 31)
        model = rm.build_model(ref, pts, cells, num_samples=48, num_fine_samples=48).to(device).train()
        assert not hasattr(model.config, "train_adjoint_mode")
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
            return {k: out[k].detach().clone() for k in ("rgb", "accumulation")}, [p.grad.clone() for p in params]

        want, want_g = step()
        model.config.train_adjoint_mode = "bf16x3"
        got, grads = step()
        for k in ("rgb", "accumulation"):
            assert torch.equal(got[k], want[k]), k
        assert float(want["accumulation"].max()) > 0.5
        for name, g, wg in zip(NAMES, grads, want_g):
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
            rel = _tensor_rel(g, wg)
            print(f"adapter {name}: max |bf16x3 adjoint - fp32 adjoint| / max |fp32| = {rel:.2e}")
            assert rel <= 1e-5, (name, rel)      # (a wrongly routed mode, or none, does not pass: see the last line)
        assert not _same_bits(grads[0], want_g[0])
    finally:
        plugin.uninstall(ref.TetrahedraNerf)
