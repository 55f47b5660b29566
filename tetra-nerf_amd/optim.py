"""The optimiser step of a training iteration on HIP: `FusedRAdam`, a drop-in for `torch.optim.RAdam`.

The reference trains its one parameter group "fields" -- the vertex field and the MLP -- with RAdam
(tetranerf/nerfstudio/registration.py:37-45).  torch.optim.RAdam runs the update as a chain of element-wise launches over whole
tensors, and its in-place step on the field makes the next gather re-transpose the [64, V] field into its vertex-major shadow.
Here the step is one kernel per registered field (tn_radam_step_field: parameter, both moments AND the shadow in one pass) and
one kernel per 32 other tensors (tn_radam_step).

THE STATEMENT (`radam_statement`, plain torch, runs on the CPU) is torch's single-tensor RAdam (torch/optim/radam.py) with its
scalar factors folded into one step size `a` (`radam_scalars`, float64 on the host).  Every line is one fp32 operation and one
rounding, every scalar is rounded to fp32 once; the kernels are the same text (csrc/tn_optim.hip) and are bit-equal to it.
The one operation torch does not round correctly on the CPU, the square root, is numpy's (`_sqrt_rn`).

Outside the contract: fp32 denormals (kept by the kernels; the CPU statement keeps them too unless flush-to-zero is set) and
non-finite gradients (they propagate into exp_avg, exp_avg_sq and the parameter as in torch; nerfstudio's GradScaler skips such
steps).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Tuple

import numpy as np
import torch

from . import _lib
from . import tetranerf_cpp_extension as cpp

RHO_THRESHOLD = 5.0
TABLE_SIZE = 32          # tensors per launch of k_radam_flat (csrc/tn_kernels.h: RADAM_TABLE)
FIELD_GRID_CAP = None    # launch_radam_field does not cap its grid: one block per 64-vertex tile, no block strides
FIELD_ROWS = 64          # the field kernel's feature count


def radam_scalars(step: int, lr: float, betas: Tuple[float, float]) -> Tuple[float, bool]:
    """(a, adaptive) of step count `step` >= 1, in float64: the bias corrections and the variance rectification of
    torch/optim/radam.py folded into the one factor the element-wise statement multiplies exp_avg with."""
    if step < 1:
        raise ValueError(f"radam_scalars: step must be >= 1, got {step}")
    b1, b2 = float(betas[0]), float(betas[1])
    t = float(step)
    bc1 = 1 - b1 ** t
    bc2 = 1 - b2 ** t
    rho_inf = 2 / (1 - b2) - 1
    rho_t = rho_inf - 2 * t * (b2 ** t) / bc2
    if rho_t > RHO_THRESHOLD:
        rect = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t))
        return float(lr) * rect * math.sqrt(bc2) / bc1, True
    return float(lr) / bc1, False


def _f32(x: float) -> torch.Tensor:
    return torch.tensor(float(x), dtype=torch.float32)


def _sqrt_rn(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root of a CPU tensor.  torch.sqrt on the CPU is NOT one: it goes through a vector
    math library whose result is off by one ulp for about 0.65 % of inputs (measured against float64 on 2^20 values; which
    inputs depends on the processor), so the statement would differ from machine to machine.  numpy's sqrt is the processor's
    IEEE instruction (0 of the same 2^20 off), as is the kernels' sqrtf sequence."""
    return torch.from_numpy(np.sqrt(x.detach().numpy()))


def hyper_scalars(lr, betas, eps, weight_decay, decoupled):
    """The group's scalars as the kernels take them: (1 - b1, b2, 1 - b2, eps, decay, decay_mode), in float64; decay_mode 0 none,
    1 coupled (decay = wd), 2 decoupled (decay = 1 - lr wd).  Each becomes fp32 once: here through torch.tensor, in step()
    through ctypes' c_float -- the same round-to-nearest conversion of the same double."""
    b1, b2 = float(betas[0]), float(betas[1])
    if weight_decay != 0:
        mode, decay = (2, 1 - float(lr) * float(weight_decay)) if decoupled else (1, float(weight_decay))
    else:
        mode, decay = 0, 0.0
    return 1 - b1, b2, 1 - b2, float(eps), decay, mode


def radam_statement(p, g, m, v, step, lr, betas, eps=1e-8, weight_decay=0.0, decoupled=False):
    """One RAdam step on fp32 tensors: returns the new (p, m, v); the inputs are not written.  `step` is the count AFTER the
    increment (1 for the first step)."""
    for x in (p, g, m, v):
        if x.dtype != torch.float32:
            raise ValueError("radam_statement: fp32 tensors only")
    a, adaptive = radam_scalars(int(step), lr, betas)
    omb1, b2, omb2, eps_, decay, mode = hyper_scalars(lr, betas, eps, weight_decay, decoupled)
    a, omb1, b2, omb2, eps_, decay = (_f32(x) for x in (a, omb1, b2, omb2, eps_, decay))
    if mode == 1:
        g = torch.add(g, torch.mul(decay, p))
    elif mode == 2:
        p = torch.mul(p, decay)
    m = torch.add(m, torch.mul(omb1, torch.sub(g, m)))
    v = torch.add(torch.mul(b2, v), torch.mul(torch.mul(omb2, g), g))
    if adaptive:
        p = torch.sub(p, torch.div(torch.mul(a, m), torch.add(_sqrt_rn(v), eps_)))
    else:
        p = torch.sub(p, torch.mul(a, m))
    return p, m, v


class _Hyper(C.Structure):      # tn_radam_hyper
    _fields_ = [("one_minus_beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float),
                ("decay", C.c_float), ("decay_mode", C.c_int)]


class _Tensor(C.Structure):     # tn_radam_tensor
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("count", C.c_size_t), ("step_size", C.c_float), ("adaptive", C.c_int)]


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise TypeError("FusedRAdam: parameters must be tensors, got " + torch.typename(p))
    if p.is_sparse or p.dtype != torch.float32:
        raise RuntimeError(f"FusedRAdam: parameters must be dense fp32 tensors, got {p.dtype}")
    if not p.is_contiguous():
        raise RuntimeError("FusedRAdam: parameters must be contiguous")
    if p.device.type != "cuda":
        raise RuntimeError("FusedRAdam: parameters must be on a GPU (there is no CPU fallback; use torch.optim.RAdam there)")


class FusedRAdam(torch.optim.Optimizer):
    """torch.optim.RAdam with the step on HIP: same constructor keywords, defaults, state (`step` a float32 CPU tensor,
    `exp_avg`, `exp_avg_sq` in the parameter's layout) and state_dict, so checkpoints interchange in both directions.

    A parameter that is a field registered with cpp.register_field and shaped [64, V] is stepped by tn_radam_step_field, which
    also writes the field's vertex-major shadow [V, 64]; the step installs it in the field cache, so the next
    field_vertex_major(field) launches no transposition.  The shadow is ONE buffer per field, overwritten by every step on the
    stepping stream (single-stream contract, as for the fused MLP handle).  Every other parameter goes through tn_radam_step, 32
    tensors per launch.  The kernels write through raw pointers; step() bumps the version counter of every tensor it wrote, so
    the caches keyed by tensor version (field shadow, packed MLP weights) see the step.

    step() reads group["lr"] on the host at every call (schedulers write it there), never synchronises with the device and
    allocates nothing after a parameter's first step.  Refused: maximize, capturable, differentiable, a tensor lr, sparse
    gradients, parameters that are not dense contiguous fp32 on a GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedRAdam: lr must be a Python number (the step size is computed on the host); a tensor lr is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys of torch.optim.RAdam's groups, so that a state_dict of either loads into the other
        defaults = {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay, "maximize": maximize, "foreach": foreach,
                    "capturable": capturable, "decoupled_weight_decay": decoupled_weight_decay, "differentiable": differentiable}
        self._shadows = {}      # id(field) -> (weakref, shadow [V, 64], event): the buffer tn_radam_step_field writes
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group):
        for key in ("maximize", "capturable", "differentiable"):
            if group.get(key, False):
                raise ValueError(f"FusedRAdam: {key}=True is not supported")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("FusedRAdam: lr must be a Python number (the step size is computed on the host); a tensor lr is not supported")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group["params"]:
                _check_param(p)
        except Exception:
            self.param_groups.pop()
            raise

    def _shadow_of(self, field):
        import weakref

        if not hasattr(self, "_shadows"):      # (an unpickled optimiser: __setstate__ restores torch's attributes only)
            self._shadows = {}
        hit = self._shadows.get(id(field))
        if hit is None or hit[0]() is not field or tuple(hit[1].shape) != (field.shape[1], field.shape[0]):
            key = id(field)

            def _drop(ref, key=key, table=self._shadows):
                cur = table.get(key)
                if cur is not None and cur[0] is ref:
                    del table[key]

            hit = self._shadows[key] = (weakref.ref(field, _drop), torch.empty((field.shape[1], field.shape[0]), dtype=torch.float32,
                                                                               device=field.device), torch.cuda.Event())
        return hit[1], hit[2]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for group in self.param_groups:
            self._check_group(group)
            lr, betas = float(group["lr"]), group["betas"]
            omb1, b2, omb2, eps, decay, mode = hyper_scalars(lr, betas, group["eps"], group["weight_decay"],
                                                             group.get("decoupled_weight_decay", False))
            hyper = _Hyper(omb1, b2, omb2, eps, decay, mode)
            flat = {}        # device -> [(p, grad, exp_avg, exp_avg_sq, a, adaptive)]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("FusedRAdam does not support sparse gradients")
                _check_param(p)
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                    raise RuntimeError("FusedRAdam: a gradient must be a contiguous fp32 tensor of its parameter's shape and device")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for s in (m, v):
                    if s.dtype != torch.float32 or s.device != p.device or s.shape != p.shape or not s.is_contiguous():
                        raise RuntimeError("FusedRAdam: exp_avg / exp_avg_sq must be contiguous fp32 tensors of the parameter's shape and device")
                state["step"] += 1
                a, adaptive = radam_scalars(int(state["step"].item()), lr, betas)
                if p.dim() == 2 and p.shape[0] == FIELD_ROWS and cpp.field_is_registered(p):
                    shadow, event = self._shadow_of(p)
                    with cpp._on(p.device):
                        _lib.check(lib.tn_radam_step_field(p.shape[1], p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                           shadow.data_ptr(), a, int(adaptive), C.addressof(hyper), cpp._stream(p.device)))
                        torch.autograd.graph.increment_version(p)
                        cpp.install_field_shadow(p, shadow, event)
                    torch.autograd.graph.increment_version(m)
                    torch.autograd.graph.increment_version(v)
                else:
                    flat.setdefault(p.device, []).append((p, g, m, v, a, adaptive))
            for dev, items in flat.items():
                table = (_Tensor * len(items))()
                for slot, (p, g, m, v, a, adaptive) in zip(table, items):
                    slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                    slot.count, slot.step_size, slot.adaptive = p.numel(), a, int(adaptive)
                with cpp._on(dev):
                    _lib.check(lib.tn_radam_step(len(items), C.addressof(table), C.addressof(hyper), cpp._stream(dev)))
                for p, _, m, v, _, _ in items:
                    torch.autograd.graph.increment_version(p)
                    torch.autograd.graph.increment_version(m)
                    torch.autograd.graph.increment_version(v)
        return loss


def grow_parameter(optimizer, old, new, exp_avg=None, exp_avg_sq=None):
    """Replace the parameter `old` of `optimizer` by `new` -- the same quantity on a mesh with other vertices, more after a split
    (cpp.split_vertex_rows), fewer after a prune (cpp.prune_vertex_rows); any shape -- in its parameter group, and move its
    state: `step` is kept (the bias corrections and the rectification go on where they were), `exp_avg` / `exp_avg_sq` are the
    tensors given (the old moments carried to the new vertices) or zeros of the new shape.  A parameter that has not been stepped yet has no state, and gets none.  Works on torch.optim.RAdam and on FusedRAdam,
    whose state layouts are the same: the state_dict of either still loads into the other.  Raises ValueError if `old` is not a
    parameter of the optimiser, or a moment has not the new parameter's shape, dtype and device.  Returns `new`."""
    group = next((g for g in optimizer.param_groups if any(p is old for p in g["params"])), None)
    if group is None:
        raise ValueError("grow_parameter: `old` is not a parameter of this optimiser")
    if any(p is new for g in optimizer.param_groups for p in g["params"]):
        raise ValueError("grow_parameter: `new` is already a parameter of this optimiser")
    for name, m in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if m is not None and (m.shape != new.shape or m.dtype != new.dtype or m.device != new.device):
            raise ValueError(f"grow_parameter: {name} must have the shape, dtype and device of the new parameter")
    if isinstance(optimizer, FusedRAdam):
        _check_param(new)
    state = optimizer.state.pop(old, None)
    group["params"] = [new if p is old else p for p in group["params"]]
    if state:
        moved = dict(state)                                                    # `step` and whatever else the class keeps
        with torch.no_grad():
            for name, m in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
                if name in state:
                    moved[name] = torch.zeros_like(new, memory_format=torch.preserve_format) if m is None else m.detach().contiguous()
        optimizer.state[new] = moved
    shadows = getattr(optimizer, "_shadows", None)
    if shadows is not None:
        shadows.pop(id(old), None)                                             # the [V, 64] buffer of the old field goes with it
    return new
