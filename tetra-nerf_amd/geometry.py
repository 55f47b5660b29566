"""The position gradients, stated once in plain torch (any device, any floating dtype).

What csrc/tn_position_grad.hip computes on the device, as the definition the tests hold it to -- the way ray_order.py
states the binning key.  Nothing here needs a GPU or the library.

A sample has vertex ids v0..v3 (`vertex_indices` [n, 4]; `EMPTY` = 0xFFFFFFFF, -1 as int32, marks a missing vertex) and
barycentrics b = (b0, b1, b2) [n, 3].  The forward statement is

    p   = o + t d                                  the sample point on its ray (t: the sample distance)
    b   = solve(T^T, p - x0)                       T = rows (x1 - x0, x2 - x0, x3 - x0), x_k the position of v_k
    phi = b0 F[v1] + b1 F[v2] + b2 F[v3] + (1 - (b0 + b1 + b2)) F[v0]

(A) `gather_backward_barycentrics`: g_k = sum_c G[c] (F[v_{k+1}, c] - F[v_0, c]) with G = dL/dphi, for any D; the row of an
    EMPTY id is a zero row.
(B) `sample_positions_backward`: dL/dp = m with T m = g, in closed form
        m = (g0 (e2 x e3) + g1 (e3 x e1) + g2 (e1 x e2)) / (e1 . (e2 x e3)),   e_k = x_k - x_0;
    vertex v_k receives -w_k m with w = (1 - (b0+b1+b2), b0, b1, b2); a ray receives dL/do = sum_s m, dL/dd = sum_s t_s m.
    A sample with an EMPTY id, a zero determinant or a non-finite m contributes exact zeros everywhere.

Tet membership (the vertex ids), t, near / far and the sampler draws are CONSTANTS of these gradients.
"""
from __future__ import annotations

from typing import Optional

import torch

EMPTY = 0xFFFFFFFF


def _ids(vertex_indices: torch.Tensor, num_vertices: int):
    """(int64 ids clamped into the table, bool `present`): EMPTY (-1 as int32) and out-of-range ids are not present"""
    v = vertex_indices.long()
    v = torch.where(v < 0, v + (1 << 32), v)        # int32 view of a uint32 id
    present = v < num_vertices
    return torch.where(present, v, torch.zeros_like(v)), present


def gather_backward_barycentrics(vertex_indices: torch.Tensor, field_vm: torch.Tensor, grad_rows: torch.Tensor) -> torch.Tensor:
    """(A).  vertex_indices [n, D] integer, field_vm [V, F] the VERTEX-major field, grad_rows [n, F] -> [n, D - 1]."""
    ids, present = _ids(vertex_indices, field_vm.shape[0])
    rows = field_vm[ids] * present[..., None].to(field_vm.dtype)            # [n, D, F], zero rows for EMPTY ids
    return torch.einsum("nc,nkc->nk", grad_rows, rows[:, 1:] - rows[:, :1])


def sample_point_gradient(vertex_indices: torch.Tensor, grad_bary: torch.Tensor, vertices: torch.Tensor):
    """m = T^-1 g per sample in closed form.  vertex_indices [n, 4], grad_bary [n, 3], vertices [V, 3] ->
    (m [n, 3] with exact zeros where the sample is not `live`, live bool [n])."""
    ids, present = _ids(vertex_indices, vertices.shape[0])
    x = vertices[ids]                                                        # [n, 4, 3]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = torch.linalg.cross(e2, e3), torch.linalg.cross(e3, e1), torch.linalg.cross(e1, e2)
    det = (e1 * c23).sum(-1, keepdim=True)
    g = grad_bary
    m = (g[:, 0:1] * c23 + g[:, 1:2] * c31 + g[:, 2:3] * c12) / det
    live = present.all(-1) & (det[:, 0] != 0) & torch.isfinite(m).all(-1)
    return torch.where(live[:, None], m, torch.zeros_like(m)), live


def gather_weights(barycentrics: torch.Tensor) -> torch.Tensor:
    """w = (1 - ((b0 + b1) + b2), b0, b1, b2) [n, 4]: the weights of (v0, v1, v2, v3), summed in the order the gather kernels
    use (in float32 these are, bit for bit, the weights the forward applied)."""
    b = barycentrics
    return torch.cat([1.0 - ((b[:, 0:1] + b[:, 1:2]) + b[:, 2:3]), b], -1)


def sample_positions_backward(vertex_indices: torch.Tensor, barycentrics: torch.Tensor, grad_bary: torch.Tensor,
                              vertices: torch.Tensor, distances: Optional[torch.Tensor] = None, samples_per_ray: Optional[int] = None,
                              weights: Optional[torch.Tensor] = None):
    """(B).  vertex_indices [n, 4], barycentrics / grad_bary [n, 3], vertices [V, 3], distances [n] (t per sample),
    samples_per_ray S (n = R S; None: no per-ray sums).  weights [n, 4]: the gather's weights if they are not to be formed
    from `barycentrics` in this dtype (a float64 check of the float32 kernels passes gather_weights(b_float32)).
    Returns a dict: points [n, 3] = m; vertices [V, 3]; origins [R, 3] = sum_s m; directions [R, 3] = sum_s t_s m
    (the last two only with samples_per_ray, the last only with distances)."""
    m, live = sample_point_gradient(vertex_indices, grad_bary, vertices)
    w = gather_weights(barycentrics) if weights is None else weights
    ids, _ = _ids(vertex_indices, vertices.shape[0])
    terms = -(w[:, :, None] * m[:, None, :]) * live[:, None, None].to(m.dtype)          # [n, 4, 3]
    out = {"points": m, "live": live,
           "vertices": torch.zeros_like(vertices).index_add_(0, ids.reshape(-1), terms.reshape(-1, 3))}
    if samples_per_ray is not None:
        out["origins"] = m.reshape(-1, int(samples_per_ray), 3).sum(1)
        if distances is not None:
            out["directions"] = (distances.reshape(-1, 1) * m).reshape(-1, int(samples_per_ray), 3).sum(1)
    return out


def barycentrics_of(points: torch.Tensor, tet_vertices: torch.Tensor) -> torch.Tensor:
    """The forward statement b = solve(T^T, p - x0).  points [n, 3], tet_vertices [n, 4, 3] -> [n, 3]."""
    T = tet_vertices[:, 1:] - tet_vertices[:, :1]
    return torch.linalg.solve(T.transpose(-1, -2), (points - tet_vertices[:, 0]).unsqueeze(-1)).squeeze(-1)
