"""Inputs, float64 references and error measures of the expected-depth / distortion tests: tests/test_ray_aux.py (CPU: the
statements alone) and tests/test_ray_aux_gpu.py (k_composite_aux and k_composite_backward_aux, csrc/tn_ray_aux.hip) take the SAME
tensors from here.  The rays are ray_stage_lib.composite_inputs(S) as they are (48 rays: thin, opaque surfaces at sample 0 / 1 / 3 /
S // 2, empty; edges from 1.0 on, a span of about 0.01 S); the two new cotangents are drawn here.  Everything is made on the CPU;
every reference is render.composite + render.composite_aux_statement (the literal pairwise form) in float64."""
import functools

import torch

import ray_stage_lib as lib

render = lib.render

# ray_stage_lib's sizes plus both sides of every size at which the kernels of tn_ray_aux.hip change form: the forward groups its
# chunks of 64 samples by 2 / 5 / 9 (S <= 128, <= 320, beyond: 128 | 129 are in the list already, 320 | 321 are added) and takes a
# second trip of the largest group from 577 on (576 | 577); the adjoint works chunk by chunk (64 | 65)
AUX_S = tuple(sorted(set(lib.COMPOSITE_S) | {320, 321, 576}))
CASES = ("depth", "distortion", "all")      # g_depth only, g_dist only, both together with g_rgb and g_acc
FLOOR, MIN_SCALE = lib.FLOOR, lib.MIN_SCALE
# background of the sweep over the sizes (black: a_i has no background term; at S = 2 the four terms of one empty ray's a_i cancel to
# a hundredth under a white one, and no fp32 evaluation has the digits then -- ray_stage_lib.composite_inputs' remark); the three
# backgrounds are compared at BACKGROUNDS_S
BACKGROUND, BACKGROUNDS_S = 0.0, 129


def _draw_cotangents(S, attempt):
    g = torch.Generator().manual_seed(S + 100003 * attempt)
    g_depth = torch.randn(48, generator=g)
    return g_depth, torch.randn(48, generator=g)


def _case_cotangents(inp, cot, case):
    """(g_rgb, g_acc, g_depth, g_dist) of a case, None where the case has none."""
    if case == "depth":
        return None, None, cot[0], None
    if case == "distortion":
        return None, None, None, cot[1]
    return inp["g_rgb"], inp["g_acc"], cot[0], cot[1]


def statement(inp, dtype):
    """(depth_moment [R], distortion_raw [R]) of render.composite_aux_statement in `dtype`, on the device the inputs are on."""
    return render.composite_aux_statement(inp["sigma"].to(dtype), inp["edges"].to(dtype))


def gradients(inp, cot, background, dtype, case):
    """(d sigma [R,S], d rgb [R,S,3]) of sum(out_rgb g_rgb) + sum(acc g_acc) + sum(depth_moment g_depth) + sum(distortion_raw g_dist)
    -- the terms the case has -- by autograd of render.composite + render.composite_aux_statement in `dtype`."""
    g_rgb, g_acc, g_depth, g_dist = _case_cotangents(inp, cot, case)
    sigma = inp["sigma"].detach().to(dtype, copy=True).requires_grad_(True)
    rgb = inp["rgb"].detach().to(dtype, copy=True).requires_grad_(True)
    e = inp["edges"].to(dtype)
    out_rgb, acc, _, _ = render.composite(sigma[..., None], rgb, e[:, :-1, None], e[:, 1:, None], background=background)
    moment, dist = render.composite_aux_statement(sigma, e)
    loss = out_rgb.sum() * 0
    for out, g in ((out_rgb, g_rgb), (acc[:, 0], g_acc), (moment, g_depth), (dist, g_dist)):
        if g is not None:
            loss = loss + (out * g.to(device=out.device, dtype=dtype)).sum()
    loss.backward()
    return sigma.grad.detach(), rgb.grad.detach()


def dw_closed_form(w, edges):
    """(d depth_moment / dw [R,S], d distortion_raw / dw [R,S]) in the linear-time form the kernels use, in the dtype of the inputs:
    (e_k + e_{k+1}) / 2 and 2 (u'_k W_k - WU_k + WU>_k - u'_k W>_k) + (2/3) w_k delta_k."""
    e0 = edges[:, :1]
    u = ((edges[:, :-1] - e0) + (edges[:, 1:] - e0)) / 2
    delta = edges[:, 1:] - edges[:, :-1]
    W_incl, WU_incl = torch.cumsum(w, -1), torch.cumsum(w * u, -1)
    W, WU = W_incl - w, WU_incl - w * u
    W_suf, WU_suf = W_incl[:, -1:] - W_incl, WU_incl[:, -1:] - WU_incl
    return (edges[:, :-1] + edges[:, 1:]) / 2, 2 * (u * W - WU + WU_suf - u * W_suf) + (2.0 / 3.0) * w * delta


def scales(inp, cot, background, case):
    """Per ray, in float64: (max_i delta_i * max_i |a_i|, max |g_rgb|) with the FULL a_i = dL/dw_i of the case: g_rgb . c_i -
    bg . g_rgb + g_acc + g_depth d depth_moment / dw_i + g_dist d distortion_raw / dw_i (ray_stage_lib.composite_scales with the two
    new terms)."""
    g_rgb, g_acc, g_depth, g_dist = _case_cotangents(inp, cot, case)
    e, c = inp["edges"].double().cpu(), inp["rgb"].double().cpu()
    R = e.shape[0]
    g = torch.zeros(R, 3, dtype=torch.float64) if g_rgb is None else g_rgb.double().cpu()
    a = (c * g[:, None, :]).sum(-1) - (render.background_tensor(background).double() * g).sum(-1)[:, None]
    if g_acc is not None:
        a = a + g_acc.double().cpu()[:, None]
    dm, dd = dw_closed_form(render.ray_weights(inp["sigma"].double().cpu(), e), e)
    if g_depth is not None:
        a = a + g_depth.double().cpu()[:, None] * dm
    if g_dist is not None:
        a = a + g_dist.double().cpu()[:, None] * dd
    return (e[:, 1:] - e[:, :-1]).max(-1).values * a.abs().max(-1).values, g.abs().max(-1).values


def value_errors(got, want64, inp):
    """Per ray: (|d depth_moment| / e_S, |d distortion_raw| / (e_S - e_0)) of `got` against the float64 values."""
    e = inp["edges"].double().cpu()
    return ((got[0].double().cpu() - want64[0].cpu()).abs() / e[:, -1], (got[1].double().cpu() - want64[1].cpu()).abs() / (e[:, -1] - e[:, 0]))


def gradient_errors(got, want64, sc):
    """ray_stage_lib.composite_errors: per-ray (d sigma, d rgb) errors under the scales above.  A ray whose a_i are all 0 (an empty
    ray under g_dist alone: every term of d distortion_raw / dw carries a weight) reports the plain absolute error of its d sigma,
    which must then be 0 -- the rule composite_errors has for d rgb without g_rgb."""
    sc = (torch.where(sc[0] > 0, sc[0], torch.ones_like(sc[0])), sc[1])
    return lib.composite_errors([g.detach().cpu() for g in got], [g.cpu() for g in want64], sc)


@functools.lru_cache(maxsize=None)
def reference_values(S):
    return statement(lib.composite_inputs(S), torch.float64)


@functools.lru_cache(maxsize=None)
def _reference_gradients(S, background, case, attempt):
    inp = lib.composite_inputs(S)
    return gradients(inp, _draw_cotangents(S, attempt), background, torch.float64, case)


def _usable(S, attempt):
    """Neither condition involves a kernel: with all four cotangents (the full a_i) every ray's scale exceeds MIN_SCALE and the
    fp32 statement under fp32 autograd on the CPU is within FLOOR of float64.  (The cases with one cotangent have a single term in
    a_i: nothing cancels, and their bound comes from the fp32 statement measured beside the kernel.)"""
    inp, cot = lib.composite_inputs(S), _draw_cotangents(S, attempt)
    if not float(scales(inp, cot, BACKGROUND, "all")[0].min()) > MIN_SCALE:
        return False
    es, _ = gradient_errors(gradients(inp, cot, BACKGROUND, torch.float32, "all"), _reference_gradients(S, BACKGROUND, "all", attempt),
                            scales(inp, cot, BACKGROUND, "all"))
    return float(es.max()) <= FLOOR


@functools.lru_cache(maxsize=None)
def _attempt(S):
    for attempt in range(100):
        if _usable(S, attempt):
            return attempt
    raise AssertionError(f"no usable cotangents for S = {S}")


def cotangents(S):
    """(g_depth [48], g_dist [48]) = randn, randn from torch.Generator().manual_seed(S), in that order.  Should a size fail the two
    conditions of _usable, the next draw of a seeded sequence is taken, as ray_stage_lib.composite_inputs does for its batches;
    tests/test_ray_aux.py asserts that the nine sizes of ray_stage_lib.COMPOSITE_S take the first."""
    return _draw_cotangents(S, _attempt(S))


def cotangent_attempt(S):
    return _attempt(S)


def reference_gradients(S, background, case):
    """float64 autograd gradients of a case, computed once per process."""
    return _reference_gradients(S, background, case, _attempt(S))
