"""Inputs, float64 references and error measures of the per-ray stage tests: tests/test_ray_stages.py (CPU: the references
alone) and tests/test_ray_stages_gpu.py (the kernels of csrc/tn_ray_ops.h and k_composite_backward) draw the SAME tensors from
here.  Everything is made on the CPU from a seeded generator and returned as fp32 (int32 for counts and indices); every
reference is the plain statement of render.py evaluated in float64 on those fp32 values cast up."""
import functools
import importlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
render = importlib.import_module("tetra-nerf_amd.render")

# ---- composite adjoint ------------------------------------------------------------------------------------------------------
COMPOSITE_S = (1, 2, 63, 64, 65, 128, 129, 513, 577)
BACKGROUNDS = (1.0, 0.0, (0.2, 0.5, 0.9))
RAYS_PER_CLASS = 8
FLOOR = 2.0 ** -20          # 16 fp32 ulps: the least bound a test derives from the fp32 statement's own error
MIN_SCALE = 1e-4


def composite_classes(S):
    """(name, first opaque sample or None) of the ray classes, RAYS_PER_CLASS consecutive rays each, in row order."""
    return [("thin", None)] + [(f"surface at {k}", min(k, S - 1)) for k in (0, 1, 3, S // 2)] + [("empty", None)]


def composite_cases():
    """(S, background, with g_rgb, with g_acc) of every comparison: all sizes x all backgrounds, and one case each without the
    gradient of the accumulation and without that of the colour."""
    return [(S, bg, True, True) for S in COMPOSITE_S for bg in BACKGROUNDS] + [(129, BACKGROUNDS[2], True, False), (129, BACKGROUNDS[2], False, True)]


def _draw_composite_inputs(S, seed):
    g = torch.Generator().manual_seed(1000 * S + seed)
    n = RAYS_PER_CLASS
    rows = []
    for name, k in composite_classes(S):
        if name == "thin":
            s = torch.rand(n, S, generator=g) * 4
        elif name == "empty":
            s = torch.zeros(n, S)
        else:
            s = torch.rand(n, S, generator=g)
            s[:, k:] = 100 + torch.rand(n, S - k, generator=g) * 400
        rows.append(s)
    sigma = torch.cat(rows).contiguous()
    R = sigma.shape[0]
    edges = (1 + torch.cumsum(torch.rand(R, S + 1, generator=g) * 0.02, -1)).contiguous()
    rgb = torch.rand(R, S, 3, generator=g)
    return {"sigma": sigma, "rgb": rgb, "edges": edges, "g_rgb": torch.randn(R, 3, generator=g), "g_acc": torch.randn(R, generator=g)}


def _usable(inp, S):
    for s, bg, ur, ua in composite_cases():
        if s != S:
            continue
        scales = composite_scales(inp, bg, ur, ua)
        if not (float(scales[0].min()) > MIN_SCALE and (not ur or float(scales[1].min()) > MIN_SCALE)):
            return False
        errs = composite_errors(composite_gradients(inp, bg, torch.float32, ur, ua), composite_gradients(inp, bg, torch.float64, ur, ua), scales)
        if not max(float(errs[0].max()), float(errs[1].max())) <= FLOOR:
            return False
    return True


@functools.lru_cache(maxsize=None)
def _composite_inputs(S):
    for seed in range(1000):
        inp = _draw_composite_inputs(S, seed)
        if _usable(inp, S):
            return inp
    raise AssertionError(f"no usable batch for S = {S}")


def composite_inputs(S):
    """sigma [48,S], rgb [48,S,3], edges [48,S+1], g_rgb [48,3], g_acc [48]: thin rays (sigma < 4), rays that end in a surface
    (sigma < 1 in front of sample k, 100 ... 500 from k on: the sum of delta sigma reaches hundreds) and empty rays.
    The batch is the first of a seeded sequence that meets two conditions, neither of which involves a kernel, in every case of
    its S: every ray's scale (composite_scales) exceeds MIN_SCALE, and fp32 autograd of render.composite on the CPU is within
    FLOOR of float64 autograd.  With one or two samples a batch fails them now and then: the largest delta of a ray is almost
    0, or the three terms of its a_i nearly cancel (|a| a hundredth of them), and then NO fp32 evaluation has the digits
    the measure asks for -- such a ray tests the order of three additions, not the adjoint.  From S = 63 on the first batch
    is taken.  tests/test_ray_stages.py asserts both conditions on what this returns."""
    return dict(_composite_inputs(S))


def composite_gradients(inp, background, dtype, use_rgb=True, use_acc=True):
    """(d sigma [R,S], d rgb [R,S,3]) of sum(out_rgb g_rgb) + sum(acc g_acc) by autograd of render.composite in `dtype`, on the
    device the inputs are on."""
    sigma = inp["sigma"].detach().to(dtype, copy=True).requires_grad_(True)
    rgb = inp["rgb"].detach().to(dtype, copy=True).requires_grad_(True)
    e = inp["edges"].to(dtype)
    out_rgb, acc, _, _ = render.composite(sigma[..., None], rgb, e[:, :-1, None], e[:, 1:, None], background=background)
    loss = out_rgb.sum() * 0
    if use_rgb:
        loss = loss + (out_rgb * inp["g_rgb"].to(dtype)).sum()
    if use_acc:
        loss = loss + (acc[:, 0] * inp["g_acc"].to(dtype)).sum()
    loss.backward()
    return sigma.grad.detach(), rgb.grad.detach()


def composite_scales(inp, background, use_rgb=True, use_acc=True):
    """Per ray, in float64: (max_i delta_i * max_i |a_i|, max |g_rgb|) with a_i = dL/dw_i = g_rgb . c_i - bg . g_rgb + g_acc --
    the size of a ray's INPUTS, so that a ray whose gradients are all ~ e^-10 is not held to digits fp32 does not have."""
    e, c = inp["edges"].double(), inp["rgb"].double()
    g = inp["g_rgb"].double() if use_rgb else torch.zeros_like(inp["g_rgb"], dtype=torch.float64)
    ga = inp["g_acc"].double() if use_acc else torch.zeros_like(inp["g_acc"], dtype=torch.float64)
    bg = render.background_tensor(background, e.device).double()
    a = (c * g[:, None, :]).sum(-1) - (bg * g).sum(-1)[:, None] + ga[:, None]
    return (e[:, 1:] - e[:, :-1]).max(-1).values * a.abs().max(-1).values, g.abs().max(-1).values


def composite_errors(got, want, scales):
    """Per-ray errors (d sigma, d rgb) of the gradients `got` against the float64 ones under the scales above; a ray whose
    colour scale is 0 (no g_rgb) reports the plain absolute error of its d rgb, which must then be 0."""
    es = (got[0].double() - want[0]).abs().max(-1).values / scales[0]
    ec = (got[1].double() - want[1]).abs().flatten(1).max(-1).values / torch.where(scales[1] > 0, scales[1], torch.ones_like(scales[1]))
    return es, ec


def per_class(err, S):
    """{class name: max error} of a per-ray error vector in the row order of composite_inputs."""
    return {name: float(err[i * RAYS_PER_CLASS:(i + 1) * RAYS_PER_CLASS].max()) for i, (name, _) in enumerate(composite_classes(S))}


# ---- PDF sampler ------------------------------------------------------------------------------------------------------------
# both edges of both chunk forms (192 / 193, 320 / 321 entries) in each argument, the loop form through S and through num_fine,
# several chunks per list, one chunk, one sample
PDF_SHAPES = ((1, 1), (2, 5), (63, 63), (190, 191), (191, 100), (192, 10), (10, 192), (319, 319), (320, 64), (64, 330), (513, 128))
PDF_RAYS = 64


def pdf_inputs(S, num_fine, train, seed=0):
    """edges [64,S+1] euclidean, weights [64,S], near_far [64,2], u_rand [64,num_fine+1] or None.  Spacing edges: a linspace for
    the even rays, normalised cumsum(U[0.05,1)) for the odd ones; weights: peaky (rand^8), every 5th ray all zero (the
    padding path), every 5th + 1 flat, divided by max(sum, 1)."""
    g = torch.Generator().manual_seed(100000 * S + 10 * num_fine + seed)
    r = PDF_RAYS
    near = torch.rand(r, 1, generator=g) + 0.5
    far = near + 0.5 + torch.rand(r, 1, generator=g) * 2.5
    spacing = torch.linspace(0.0, 1.0, S + 1)[None].repeat(r, 1)
    steps = torch.cumsum(0.05 + 0.95 * torch.rand(r, S, generator=g), -1)
    spacing[1::2, 1:] = (steps / steps[:, -1:])[1::2]
    edges = (spacing * far + (1.0 - spacing) * near).contiguous()
    w = torch.rand(r, S, generator=g) ** 8
    w[::5] = 0.0
    w[1::5] = 0.3 / S
    w = (w / w.sum(-1, keepdim=True).clamp_min(1.0)).contiguous()
    u_rand = torch.rand(r, num_fine + 1, generator=g) if train else None
    return {"edges": edges, "weights": w, "near_far": torch.cat([near, far], 1).contiguous(), "u_rand": u_rand}


def pdf_statement(inp, num_fine, dtype):
    """render.pdf_sample_bins in `dtype` on the inputs as the kernel gets them (the spacing edges re-derived from the euclidean
    ones, as the renderer does)."""
    e, w, nf = inp["edges"].to(dtype), inp["weights"].to(dtype), inp["near_far"].to(dtype)
    near, far = nf[:, 0:1], nf[:, 1:2]
    u = None if inp["u_rand"] is None else inp["u_rand"].to(dtype)
    return render.pdf_sample_bins((e - near) / (far - near), w, num_fine, near, far, u_rand=u)


def pdf_error(got, want64, inp):
    """Per ray: max |got - want| / (far - near)."""
    nf = inp["near_far"].to(want64.device).double()
    return (got.double() - want64).abs().max(-1).values / (nf[:, 1] - nf[:, 0])


# ---- coarse sampler ---------------------------------------------------------------------------------------------------------
COARSE_M = 256
COARSE_NV = (0, 1, 2, 63, 64, 65, 129, 255, 256)
COARSE_RAYS_PER_NV = 6
COARSE_S = (1, 63, 64, 65, 200)
FILL = 1e30                 # what the slots beyond a row's segments hold


def coarse_rows(seed=0):
    """Trace rows built by hand: num_visited i32 [54], hit_distances f32 [54,256,2] (6 rays per segment count of COARSE_NV;
    contiguous segments of length U[0.001,0.05) from a start in [0.5,1.5); slots beyond the count hold 1e30) and, per ray,
    the slots of its zero-length segment and of its segment with t_out < t_in (rays with 4 segments or more: slot 1 and slot
    nv - 2, both interior so that near / far stay the first entry and the last exit; -1 otherwise)."""
    g = torch.Generator().manual_seed(77 + seed)
    M = COARSE_M
    nvs, rows, zero_slot, neg_slot = [], [], [], []
    for nv in COARSE_NV:
        for _ in range(COARSE_RAYS_PER_NV):
            hd = torch.full((M, 2), FILL)
            start = float(torch.rand(1, generator=g)) + 0.5
            length = 0.001 + 0.049 * torch.rand(nv, generator=g)
            z, n = (1, nv - 2) if nv >= 4 else (-1, -1)
            back = torch.zeros(nv)
            if nv >= 4:
                length[z] = 0.0
                length[n] = 0.0         # the segment contributes nothing; its exit lies before its entry
                back[n] = 0.01
            t_in = start + torch.cat([torch.zeros(1), torch.cumsum(length, 0)[:-1]]) if nv else torch.zeros(0)
            hd[:nv, 0] = t_in
            hd[:nv, 1] = t_in + length - back
            nvs.append(nv); rows.append(hd); zero_slot.append(z); neg_slot.append(n)
    return {"num_visited": torch.tensor(nvs, dtype=torch.int32), "hit_distances": torch.stack(rows).contiguous(),
            "zero_slot": torch.tensor(zero_slot), "neg_slot": torch.tensor(neg_slot)}


def coarse_draws(S, seed=0):
    g = torch.Generator().manual_seed(31 * S + seed)
    return torch.rand(len(COARSE_NV) * COARSE_RAYS_PER_NV, S + 1, generator=g)


def coarse_near_far(rows):
    """(near [R], far [R]) = first t_in and last t_out of every row, (0, 1) for the rows without a segment."""
    nv, hd = rows["num_visited"].long(), rows["hit_distances"]
    hit = nv > 0
    near = torch.where(hit, hd[:, 0, 0], torch.zeros_like(hd[:, 0, 0]))
    far = torch.where(hit, hd[torch.arange(len(nv), device=nv.device), (nv - 1).clamp_min(0), 1], torch.ones_like(near))
    return near, far


def coarse_statement(rows, S, biased, t_rand, dtype):
    """render.biased_sample_bins / uniform_sample_bins in `dtype` on the rays with a segment: (their indices, edges [r,S+1])."""
    idx = torch.nonzero(rows["num_visited"] > 0)[:, 0]
    near, far = coarse_near_far(rows)
    near, far = near[idx, None].to(dtype), far[idx, None].to(dtype)
    t = None if t_rand is None else t_rand[idx].to(dtype)
    if biased:
        return idx, render.biased_sample_bins(near, far, S, rows["num_visited"][idx], rows["hit_distances"][idx].to(dtype), t)
    return idx, render.uniform_sample_bins(near, far, S, t)


def coarse_error(got, want64, rows, idx):
    """Per ray: max |edges - want| / (|far - near| + |far|)."""
    near, far = coarse_near_far(rows)
    near, far = near[idx].double(), far[idx].double()
    return (got.double() - want64).abs().max(-1).values / ((far - near).abs() + far.abs())


def to_device(d, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
