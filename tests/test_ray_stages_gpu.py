"""The per-ray stages (csrc/tn_ray_ops.h: coarse sampler, PDF sampler, composite) and the composite adjoint
(k_composite_backward, csrc/tn_mlp_bwd.hip) against the plain statements of render.py evaluated in FLOAT64 on the same fp32
inputs, at every size at which the kernels change form and on rays that end in an opaque surface.  The inputs come from
tests/ray_stage_lib.py; tests/test_ray_stages.py checks, without a GPU, that they are well scaled and that the fp32
statements meet the same bars -- so a failure here is the kernel's.

Every bound is either the bar the suite already holds the kernel to, or a multiple of the error `y` of the fp32 statement on
the device in the same test: two correct fp32 evaluations differ in summation order, and the factor (4 for one ray-wise
figure, 8 for a maximum over 64 rays of a sampler) is the room for that.  Each test prints its figures before it asserts."""
import importlib

import pytest

import ray_stage_lib as lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def render():
    return importlib.import_module("tetra-nerf_amd.render")


def _report(*parts):
    print("ray-stages:", *parts, flush=True)


# ---- B1 / B2: the composite adjoint ------------------------------------------------------------------------------------------

def _adjoint_case(tn, device, render, S, bg, use_rgb, use_acc, through_node):
    """(errors of the kernel, errors of fp32 autograd on the device), each (d sigma [R], d rgb [R]) per ray."""
    import torch

    cpu = lib.composite_inputs(S)
    scales = lib.composite_scales(cpu, bg, use_rgb, use_acc)
    assert float(scales[0].min()) > lib.MIN_SCALE and (not use_rgb or float(scales[1].min()) > lib.MIN_SCALE)   # (inputs)
    want = lib.composite_gradients(cpu, bg, torch.float64, use_rgb, use_acc)
    inp = lib.to_device(cpu, device)
    y = lib.composite_errors([g.cpu() for g in lib.composite_gradients(inp, bg, torch.float32, use_rgb, use_acc)], want, scales)
    g_rgb, g_acc = (inp["g_rgb"] if use_rgb else None), (inp["g_acc"] if use_acc else None)
    if through_node:
        sigma, rgb = inp["sigma"].clone().requires_grad_(True), inp["rgb"].clone().requires_grad_(True)
        o, a, _ = render._FusedCompositeFunction.apply(sigma, rgb, inp["edges"], bg)
        loss = 0
        if use_rgb:
            loss = loss + (o * g_rgb).sum()
        if use_acc:
            loss = loss + (a.reshape(-1) * g_acc).sum()
        loss.backward()
        got = (sigma.grad, rgb.grad)
    else:
        got = tn.cpp.composite_backward(inp["sigma"], inp["rgb"], inp["edges"], g_rgb, g_acc, bg)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    if not use_rgb:
        assert float(got[1].abs().max()) == 0
    return lib.composite_errors([g.cpu() for g in got], want, scales), y


@pytest.mark.parametrize("through_node", [False, True], ids=["op", "autograd-node"])
@pytest.mark.parametrize("S", lib.COMPOSITE_S)
def test_composite_adjoint_vs_float64_autograd(tn, device, render, S, through_node):
    """d sigma and d rgb of tn_composite_backward (and of the autograd node around it) against float64 autograd of
    render.composite, per ray and scaled by the ray's inputs (ray_stage_lib.composite_scales), on thin rays, rays with an opaque
    surface at sample 0 / 1 / 3 / S // 2 (the sum of delta sigma in the hundreds: where a prefix formed as total minus suffix
    loses the transmittance) and empty rays; three backgrounds, and once each without g_acc and without g_rgb.
    Bound per case and tensor: max(4 y, 2^-20), y = the same figure of fp32 torch autograd on the device."""
    failures = []
    for s, bg, use_rgb, use_acc in lib.composite_cases():
        if s != S:
            continue
        (es, ec), (ys, yc) = _adjoint_case(tn, device, render, S, bg, use_rgb, use_acc, through_node)
        for name, e, y in (("d_sigma", es, ys), ("d_rgb", ec, yc)):
            bound = max(4 * float(y.max()), lib.FLOOR)
            _report(f"adjoint S={S} bg={bg} g_rgb={use_rgb} g_acc={use_acc} node={through_node} {name}: err {float(e.max()):.3e} "
                    f"y {float(y.max()):.3e} ratio {float(e.max()) / max(float(y.max()), 1e-30):.2f} bound {bound:.3e} per class "
                    + ", ".join(f"{k} {v:.2e}" for k, v in lib.per_class(e, S).items()))
            if not float(e.max()) <= bound:
                failures.append((bg, use_rgb, use_acc, name, float(e.max()), bound))
    assert not failures, failures


@pytest.mark.parametrize("S", lib.COMPOSITE_S)
def test_composite_adjoint_weights_are_the_forwards(tn, device, S):
    """With g_rgb = 1 and no g_acc, d rgb[..., 0] IS the weight the adjoint differentiates: the forward's, bit for bit."""
    import torch

    inp = lib.to_device(lib.composite_inputs(S), device)
    R = inp["sigma"].shape[0]
    w_fwd = tn.cpp.composite(inp["sigma"], inp["rgb"], inp["edges"], return_weights=True)[3]
    w_adj = tn.cpp.composite_backward(inp["sigma"], inp["rgb"], inp["edges"], torch.ones(R, 3, device=device), None)[1][..., 0].contiguous()
    diff = (w_adj.double() - w_fwd.double()).abs() / w_fwd.double().clamp_min(1e-300)
    differ = w_adj.view(torch.int32) != w_fwd.view(torch.int32)
    _report(f"weights S={S}: {int(differ.sum())} of {differ.numel()} differ, largest relative difference {float(diff[differ].max()) if bool(differ.any()) else 0.0:.3e}; "
            "classes with a differing ray (1) " + ", ".join(f"{k} {int(v)}" for k, v in lib.per_class(differ.any(-1).float().cpu(), S).items()))
    assert float(w_fwd.max()) > 0.5
    assert torch.equal(w_adj.view(torch.int32), w_fwd.view(torch.int32))


def test_composite_backward_rejects_mismatched_inputs(tn, device):
    """Every mismatch raises before the launch: the kernel indexes all five tensors by the R and S of sigma."""
    import torch

    R, S = 5, 7
    ok = dict(sigma=torch.rand(R, S, device=device), rgb=torch.rand(R, S, 3, device=device), edges=torch.rand(R, S + 1, device=device),
              d_out_rgb=torch.rand(R, 3, device=device), d_out_acc=torch.rand(R, device=device))
    tn.cpp.composite_backward(**ok)
    bad = dict(sigma=[torch.rand(R, S + 1, device=device), torch.rand(R * S, device=device), ok["sigma"].double(), ok["sigma"].cpu(), ok["sigma"].t()],
               rgb=[torch.rand(R, S - 1, 3, device=device), torch.rand(R, S, device=device), ok["rgb"].double(), ok["rgb"].cpu()],
               edges=[torch.rand(R, S, device=device), torch.rand(R - 1, S + 1, device=device), ok["edges"].double(),
                      torch.rand(R, 2 * (S + 1), device=device)[:, ::2]],
               d_out_rgb=[torch.rand(R, device=device), torch.rand(R - 1, 3, device=device), ok["d_out_rgb"].double(), ok["d_out_rgb"].cpu()],
               d_out_acc=[torch.rand(R, 1, device=device), torch.rand(R - 1, device=device), ok["d_out_acc"].double(),
                          torch.rand(2 * R, device=device)[::2]])
    for name, values in bad.items():
        for v in values:
            with pytest.raises(RuntimeError):
                tn.cpp.composite_backward(**{**ok, name: v})


# ---- B3: the PDF sampler -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("S,num_fine", lib.PDF_SHAPES)
def test_sample_pdf_vs_float64_statement(tn, device, S, num_fine, train):
    """tn_sample_pdf against render.pdf_sample_bins in float64 at both edges of both chunk forms (S + 1 or num_fine + 1 of 192 /
    193 and 320 / 321), in the plain-loop form reached through either argument, with S != num_fine, and with 1 and 2 samples."""
    import torch

    cpu = lib.pdf_inputs(S, num_fine, train)
    want = lib.pdf_statement(cpu, num_fine, torch.float64)
    inp = lib.to_device(cpu, device)
    y32 = lib.pdf_error(lib.pdf_statement(inp, num_fine, torch.float32).cpu(), want, cpu)
    # an unwritten slot should show as NaN, not as an earlier call's correct value in a recycled block
    poison = torch.full((lib.PDF_RAYS, S + num_fine + 2), float("nan"), device=device)
    del poison
    got = tn.cpp.sample_pdf(inp["edges"], inp["weights"], inp["near_far"], num_fine, u_rand=inp["u_rand"])
    assert got.shape == (lib.PDF_RAYS, S + num_fine + 2) and not bool(torch.isnan(got).any())
    far = inp["near_far"][:, 1:2]
    assert bool((got[:, 1:] >= got[:, :-1] - 1e-6 * far).all())
    err = lib.pdf_error(got.cpu(), want, cpu)
    e, y = float(err.max()), float(y32.max())
    _report(f"pdf S={S} num_fine={num_fine} train={train}: err {e:.3e} y32 {y:.3e} ratio {e / max(y, 1e-30):.2f}")
    assert e <= 2e-5, e
    assert e <= 8 * y, (e, y)


# ---- B4: the coarse sampler --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("biased", [False, True], ids=["uniform", "biased"])
@pytest.mark.parametrize("S", lib.COARSE_S)
def test_sample_coarse_on_crafted_rows_vs_float64_statement(tn, device, render, S, biased, train):
    """tn_sample_coarse on rows made by hand -- 0, 1, 2, 63, 64, 65, 129, 255 and M = 256 segments, a zero-length segment and a
    segment with t_out < t_in at known interior slots, 1e30 behind the last segment -- against render.biased_sample_bins /
    uniform_sample_bins in float64.  A row without a segment (the sync-free training path names such rays) gets near / far =
    (0, 1) and, biased or not, the plain spacing bins: ray_sample_coarse_nf skips the biased mapping when nb == 0."""
    import torch

    cpu = lib.coarse_rows()
    t_cpu = lib.coarse_draws(S) if train else None
    idx, want = lib.coarse_statement(cpu, S, biased, t_cpu, torch.float64)
    rows = lib.to_device(cpu, device)
    t_rand = None if t_cpu is None else t_cpu.to(device)
    _, y_edges = lib.coarse_statement(rows, S, biased, t_rand, torch.float32)
    y32 = lib.coarse_error(y_edges.cpu(), want, cpu, idx)
    R = len(cpu["num_visited"])
    poison = torch.full((R, S + 1), float("nan"), device=device)
    del poison
    edges, nf = tn.cpp.sample_coarse(rows["num_visited"], rows["hit_distances"], torch.arange(R, dtype=torch.int32, device=device), S,
                                     biased=biased, t_rand=t_rand)
    assert edges.shape == (R, S + 1) and nf.shape == (R, 2) and bool(torch.isfinite(edges).all())
    near, far = lib.coarse_near_far(cpu)
    assert torch.equal(nf.cpu(), torch.stack([near, far], 1))           # first t_in, last t_out; (0, 1) without a segment
    miss = torch.nonzero(cpu["num_visited"] == 0)[:, 0]
    assert len(miss) == lib.COARSE_RAYS_PER_NV
    miss = miss.to(device)
    bins = render.uniform_sample_bins(torch.zeros(len(miss), 1, device=device), torch.ones(len(miss), 1, device=device), S,
                                      None if t_rand is None else t_rand[miss])
    assert torch.equal(edges[miss], bins.expand(len(miss), S + 1))
    err = lib.coarse_error(edges.cpu()[idx], want, cpu, idx)
    e, y = float(err.max()), float(y32.max())
    _report(f"coarse S={S} biased={biased} train={train}: err {e:.3e} y32 {y:.3e} ratio {e / max(y, 1e-30):.2f}")
    assert e <= 4e-7, e
    assert e <= 8 * y, (e, y)
