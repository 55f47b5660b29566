"""tetra-nerf_amd: the ray -> tetrahedra hot path of Tetra-NeRF on AMD MI355X (gfx950).

Python surface = what `tetranerf.utils.extension` exposes in the reference
(/root/reference/tetranerf/utils/extension/__init__.py:23-26,67-73): `TetrahedraTracer`,
`triangulate`, `gather_uint32`, `scatter_ema_uint32_`, `interpolate_values`
(differentiable w.r.t. the field), `add_barycentrics_grad`; the raw module is `cpp`
(same role as `tetranerf.cpp`, tetranerf/__init__.py:1).

The directory name contains a hyphen, so import it with
    importlib.import_module("tetra-nerf_amd")
or through the alias module `tetranerf_amd` at the repository root.
"""
from __future__ import annotations

import torch

from . import tetranerf_cpp_extension as cpp

__version__ = "0.1.0"

TetrahedraTracer = cpp.TetrahedraTracer
triangulate = cpp.triangulate
gather_uint32 = cpp.gather_uint32
scatter_ema_uint32_ = cpp.scatter_ema_uint32


class _GatherField(torch.autograd.Function):
    """field[64,V] -> per-sample features; gradient flows to the field like
    _InterpolateValuesFunction (extension/__init__.py:29-42) and, when they require it, to the
    barycentrics (py_binding.cpp:354 leaves that as a TODO; tn_interpolate_values_backward_bary_vm).
    The vertex indices -- tet membership -- are constants of the gradient."""

    @staticmethod
    def forward(ctx, vertex_indices, barycentric_coordinates, field):
        ctx.save_for_backward(vertex_indices, barycentric_coordinates, field)
        return cpp.interpolate_values(vertex_indices, barycentric_coordinates, field)

    @staticmethod
    def backward(ctx, grad_out):
        vertex_indices, barycentric_coordinates, field = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        grad_field = grad_bary = None
        if ctx.needs_input_grad[2]:
            grad_field = cpp.interpolate_values_backward(vertex_indices, barycentric_coordinates, field, grad_out)
        if ctx.needs_input_grad[1]:
            grad_bary = cpp.interpolate_values_backward_barycentrics(vertex_indices, field, grad_out)
        return None, grad_bary, grad_field


def interpolate_values(vertex_indices, barycentric_coordinates, field):
    return _GatherField.apply(vertex_indices, barycentric_coordinates, field)


class _BarycentricsGrad(torch.autograd.Function):
    """Identity on the barycentrics that routes their gradient to the tetrahedron vertices and
    the query points (role of _BarycentricsGradFunction, extension/__init__.py:45-68; unused
    by the model).  With lambda_1..3 the non-leading barycentrics of p in (v0..v3):
        p - v0 = T^T lambda,  T = rows (v_k - v0)   =>   d lambda = T^-T (dp - sum_k w_k dv_k)
    with w = (1 - sum lambda, lambda)."""

    @staticmethod
    def forward(ctx, barycentrics, vertices, points):
        ctx.save_for_backward(barycentrics, vertices)
        return barycentrics

    @staticmethod
    def backward(ctx, grad_bary):
        barycentrics, vertices = ctx.saved_tensors
        need_v, need_p = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_v = grad_p = None
        if need_v or need_p:
            edges = vertices[..., 1:, :] - vertices[..., :1, :]
            m = torch.linalg.solve(edges, grad_bary)
            if need_p:
                grad_p = m
            if need_v:
                w = torch.cat([1.0 - barycentrics.sum(-1, keepdim=True), barycentrics], -1)
                grad_v = -(w.unsqueeze(-1) * m.unsqueeze(-2))
        return grad_bary, grad_v, grad_p


def add_barycentrics_grad(barycentrics, vertices, points):
    return _BarycentricsGrad.apply(barycentrics, vertices, points)


class _SamplePositionsGrad(torch.autograd.Function):
    """Identity on the barycentrics of ray samples whose backward is tn_sample_positions_backward: the barycentric
    gradient passes through unchanged and is also routed to the mesh vertices and to the rays the samples sit on
    (the statement: geometry.sample_positions_backward)."""

    @staticmethod
    def forward(ctx, barycentrics, vertex_indices, vertices, origins, directions, distances):
        ctx.save_for_backward(barycentrics, vertex_indices, vertices, distances)
        return barycentrics.view_as(barycentrics)

    @staticmethod
    def backward(ctx, grad_bary):
        barycentrics, vertex_indices, vertices, distances = ctx.saved_tensors
        _, need_v, need_o, need_d = ctx.needs_input_grad[1:5]
        grad_v = grad_o = grad_d = None
        if need_v or need_o or need_d:
            _, grad_o, grad_d, grad_v = cpp.sample_positions_backward(
                vertex_indices, barycentrics, grad_bary.contiguous(), vertices.detach(), distances,
                want_origins=need_o, want_directions=need_d, want_vertices=need_v)
        return grad_bary, None, grad_v, grad_o, grad_d, None


def sample_positions_grad(barycentrics, vertex_indices, vertices, origins, directions, distances):
    """Identity on `barycentrics` f32 [R, S, 3] that makes them differentiable w.r.t. where the samples sit: in the
    backward pass the barycentric gradient g of a sample becomes m = T^-1 g (T = rows x_k - x_0 of its tetrahedron
    `vertex_indices` i32 [R, S, 4] in `vertices` f32 [V, 3]), the gradient w.r.t. the sample point p = o + t d, and
        vertices [V,3] receive -w_k m (w = (1 - sum b, b0, b1, b2)),  origins [R,3] sum_s m,  directions [R,3] sum_s t_s m
    with t = `distances` f32 [R, S], the sample distances handed to find_visited_cells.  One HIP kernel
    (tn_sample_positions_backward); the role of add_barycentrics_grad for whole ray batches.  Tet membership, t, near / far
    and the sampler draws are CONSTANTS of the gradient; after the vertices moved the tracer must follow them
    (TetrahedraTracer.update_vertices while the cells stay, load_tetrahedra otherwise).  Under cpp.deterministic_gradients() the vertex sum is taken without float atomics."""
    return _SamplePositionsGrad.apply(barycentrics, vertex_indices, vertices, origins, directions, distances)


__all__ = ["TetrahedraTracer", "triangulate", "gather_uint32", "scatter_ema_uint32_",
           "interpolate_values", "add_barycentrics_grad", "sample_positions_grad", "cpp"]
