"""Inputs and references of the RAdam tests (tests/test_radam.py on the CPU, tests/test_radam_gpu.py on the device).

A case is a parameter p, and per step a gradient g with |g| in {0} U [1e-6, 1] (log-uniform magnitudes, random signs, one element
in 16 exactly 0), so that no fp32 denormal arises in g, exp_avg, exp_avg_sq or their products.  Everything is made on the CPU from
a seed; the GPU tests upload it."""
import importlib

import torch

STEPS = 12
N = 4096
LR = 1e-3
EPS = 1e-8
BETAS = (0.9, 0.999)
# (name, weight_decay, decoupled)
DECAYS = (("none", 0.0, False), ("coupled", 1e-2, False), ("decoupled", 1e-2, True))


def optim():
    return importlib.import_module("tetra-nerf_amd.optim")


def parameter(shape, seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(shape, generator=gen) * 0.5).float()


def gradient(shape, seed, step):
    gen = torch.Generator().manual_seed(7919 * seed + step)
    mag = (10.0 ** (-6.0 * torch.rand(shape, generator=gen, dtype=torch.float64))).clamp(1e-6, 1.0).float().clamp(1e-6, 1.0)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    zero = torch.rand(shape, generator=gen) < 1.0 / 16
    return torch.where(zero, torch.zeros(()), mag * sign).float()


def moments(shape, seed):
    """A plausible mid-training state (exp_avg, exp_avg_sq >= 0), for single steps that do not start from zeros."""
    gen = torch.Generator().manual_seed(31 + seed)
    g = gradient(shape, seed + 17, 0)
    return (g * torch.rand(shape, generator=gen)).float(), (g * g * torch.rand(shape, generator=gen)).float()


def statement_step(p, g, m, v, step, decay=DECAYS[0], lr=LR, betas=BETAS, eps=EPS):
    return optim().radam_statement(p, g, m, v, step, lr, betas, eps, decay[1], decay[2])


def torch_trajectory(p0, grads, dtype, decay, lr=LR, betas=BETAS, eps=EPS):
    """[(p, exp_avg, exp_avg_sq) after each step] of torch.optim.RAdam(foreach=False) in `dtype` on the CPU."""
    p = p0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.RAdam([p], lr=lr, betas=betas, eps=eps, weight_decay=decay[1], decoupled_weight_decay=decay[2], foreach=False)
    out = []
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


def statement_trajectory(p0, grads, decay, lr=LR, betas=BETAS, eps=EPS):
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    out = []
    for t, g in enumerate(grads, 1):
        p, m, v = statement_step(p, g, m, v, t, decay, lr, betas, eps)
        out.append((p, m, v))
    return out


def error(x, ref):
    """max |x - ref| / max |ref|, in float64"""
    ref = ref.double()
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(torch.finfo(torch.float64).tiny))
