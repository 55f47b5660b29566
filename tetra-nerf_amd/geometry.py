"""The position gradients, the vertex step limiter, the Delaunay monitor with its state transfer and (at the end of the file) the
isosurface extraction, stated once in plain torch / numpy (any device).

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
    A sample with an EMPTY (or out-of-range) id, a zero determinant or a non-finite m contributes exact zeros everywhere; an
    id-dead sample does so whatever its barycentrics, distance and gradient hold.

Tet membership (the vertex ids), t, near / far and the sampler draws are CONSTANTS of these gradients.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
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
    (the last two only with samples_per_ray, the last only with distances).
    A sample that is not `live` contributes exact zeros whatever its barycentrics, distance and gradient hold (a row the
    matcher never wrote may hold NaN): its terms are SELECTED away, not multiplied by zero."""
    m, live = sample_point_gradient(vertex_indices, grad_bary, vertices)
    w = gather_weights(barycentrics) if weights is None else weights
    ids, _ = _ids(vertex_indices, vertices.shape[0])
    terms = -(w[:, :, None] * m[:, None, :])                                            # [n, 4, 3]
    terms = torch.where(live[:, None, None], terms, torch.zeros_like(terms))
    out = {"points": m, "live": live,
           "vertices": torch.zeros_like(vertices).index_add_(0, ids.reshape(-1), terms.reshape(-1, 3))}
    if samples_per_ray is not None:
        out["origins"] = m.reshape(-1, int(samples_per_ray), 3).sum(1)
        if distances is not None:
            tm = distances.reshape(-1, 1) * m
            out["directions"] = torch.where(live[:, None], tm, torch.zeros_like(tm)).reshape(-1, int(samples_per_ray), 3).sum(1)
    return out


def barycentrics_of(points: torch.Tensor, tet_vertices: torch.Tensor) -> torch.Tensor:
    """The forward statement b = solve(T^T, p - x0).  points [n, 3], tet_vertices [n, 4, 3] -> [n, 3]."""
    T = tet_vertices[:, 1:] - tet_vertices[:, :1]
    return torch.linalg.solve(T.transpose(-1, -2), (points - tet_vertices[:, 0]).unsqueeze(-1)).squeeze(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# The vertex step limiter (csrc/tn_vertex_guard_core.h, csrc/tn_vertex_guard.hip), stated in torch.
#
# The WIDTH w of a tetrahedron is its smallest extent over all directions.  It is attained on one of seven slabs: the four
# heights and the three distances between opposite edges, |vol6| / |a x b| with a, b two edges of a face or two opposite edges.
# If every vertex of a tetrahedron moves by less than w / 2 the four points are coplanar at no fraction of the straight move, so
# the signed volume keeps its sign.  Widths are float64 on the float32 coordinates, one rounding per operation in the order
# written here (no fused multiply-add: every product is a statement of its own); the clamp is float32 in the order written.
# With float32 inputs the results are, bit for bit, what the kernels give.

MAX_STEP_FRACTION = 0.45         # 0.45 (1 + 2^-20) + 1/32 < 1/2
FREEZE_RATIO = 2.0 ** -17        # star width below this part of the vertex's largest |coordinate|: the vertex does not move

_SLABS = ((1, 2, 1, 3), (0, 2, 0, 3), (0, 1, 0, 3), (0, 1, 0, 2),      # faces: two edges out of one corner
          (0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2))                    # pairs of opposite edges


def _cross3(u, v):
    return (u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])


def _vol6(p):
    """signed ((p1-p0) x (p2-p0)) . (p3-p0) of p float64 [T, 4, 3]"""
    n0, n1, n2 = _cross3(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    e3 = p[:, 3] - p[:, 0]
    return (n0 * e3[:, 0] + n1 * e3[:, 1]) + n2 * e3[:, 2]


def tet_orient(vertices: torch.Tensor, cells: torch.Tensor) -> torch.Tensor:
    """int8 [T]: the sign of the signed volume of every tetrahedron (0 also where it is NaN)"""
    v = _vol6(vertices.double()[cells.long()])
    return (v > 0).to(torch.int8) - (v < 0).to(torch.int8)


def tet_slabs(p: torch.Tensor):
    """p float64 [T, 4, 3] -> (vol6 [T] signed, norms [T, 7]): slab k has thickness |vol6| / norms[:, k] and the unit normal of
    its cross product; the width is the thinnest of the seven.  (torch's float64 square root on the CPU may be a vector-library
    call that is off in the last bit; the float32 rounding of the width absorbs that except about once in 1e8 tetrahedra.)"""
    norms = []
    for a, b, c, d in _SLABS:
        w0, w1, w2 = _cross3(p[:, b] - p[:, a], p[:, d] - p[:, c])
        norms.append(torch.sqrt((w0 * w0 + w1 * w1) + w2 * w2))
    return _vol6(p), torch.stack(norms, -1)


def tet_width64(p: torch.Tensor) -> torch.Tensor:
    """float64 [T]: |vol6| / den with den the largest of the seven norms (taken with `>`, so a NaN norm is passed over), 0 where den is 0"""
    vol6, norms = tet_slabs(p)
    den = torch.zeros_like(vol6)
    for k in range(7):
        den = torch.where(norms[:, k] > den, norms[:, k], den)
    return torch.where(den > 0, vol6.abs() / den, torch.zeros_like(den))


def tet_width_orient(vertices: torch.Tensor, cells: torch.Tensor):
    """vertices [V, 3], cells integer [T, 4] -> (width float32 [T], orient int8 [T]).  width = fl32(tet_width64); anything that is
    not 0 <= width < inf counts as 0."""
    p = vertices.double()[cells.long()]
    w = tet_width64(p).to(torch.float32)
    w = torch.where((w >= 0) & (w < float("inf")), w, torch.zeros_like(w))
    vol6 = _vol6(p)
    return w, (vol6 > 0).to(torch.int8) - (vol6 < 0).to(torch.int8)


def star_width(vertices: torch.Tensor, cells: torch.Tensor, width: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [V]: the smallest width over the tetrahedra around each vertex; +inf where no tetrahedron names it"""
    if width is None:
        width = tet_width_orient(vertices, cells)[0]
    out = torch.full((vertices.shape[0],), float("inf"), dtype=torch.float32, device=vertices.device)
    return out.scatter_reduce_(0, cells.long().reshape(-1), width.repeat_interleave(4), "amin", include_self=True)


def _sqrt_f32(x: torch.Tensor) -> torch.Tensor:
    """the correctly rounded float32 square root (what sqrtf is on the device and in C).  torch.sqrt on a float32 CPU tensor
    is not that: above a few hundred elements it is a vector-library call whose last bit depends on the machine.  Through float64
    it is: the root of a float32 is never close enough to the middle of two float32 for the float64 rounding to matter."""
    return torch.sqrt(x.double()).to(torch.float32)


def limit_vertex_step_statement(xyz_old: torch.Tensor, xyz_new: torch.Tensor, cells: torch.Tensor, fraction: float = 0.25,
                                _check_range: bool = True):
    """What tn_limit_vertex_step computes.  xyz_old / xyz_new float32 [V, 3] (xyz_new is NOT modified), cells integer [T, 4].
    Returns a dict: "xyz" float32 [V, 3] the limited positions, "star_width" float32 [V] (of xyz_old), "frozen" / "clamped" bool
    [V], "counters" int64 [4] = clamped, frozen but asked to move, flipped, collapsed (tetrahedra, xyz_old against "xyz").
    `_check_range=False` (tests only) lifts both the range of `fraction` and the freeze rule: it shows what the same step does
    when it is clamped to more than the bound allows."""
    if _check_range and not 0.0 < fraction <= MAX_STEP_FRACTION:
        raise ValueError("fraction must be in (0, 0.45]")
    old, new = xyz_old.to(torch.float32), xyz_new.to(torch.float32)
    star = star_width(old, cells)
    a = old.abs()
    m = a[:, 0]
    m = torch.where(a[:, 1] > m, a[:, 1], m)
    m = torch.where(a[:, 2] > m, a[:, 2], m)
    frozen = ~(star >= torch.tensor(FREEZE_RATIO, dtype=torch.float32, device=old.device) * m)
    if not _check_range:
        frozen = torch.zeros_like(frozen)
    d = new - old
    n = _sqrt_f32((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    lim = torch.tensor(fraction, dtype=torch.float32, device=old.device) * star
    finite = n < float("inf")
    kept = finite & (n <= lim)
    s = lim / n
    shortened = old + d * s[:, None]
    out = torch.where(frozen[:, None], old, torch.where(kept[:, None], new, torch.where(finite[:, None], shortened, old)))
    clamped = ~frozen & ~kept
    before, after = tet_orient(old, cells).long(), tet_orient(out, cells).long()
    counters = torch.stack([clamped.sum(), (frozen & (new != old).any(-1)).sum(), (before * after < 0).sum(),
                            ((before != 0) & (after == 0)).sum()])
    return {"xyz": out, "star_width": star, "frozen": frozen, "clamped": clamped, "counters": counters}


# ---------------------------------------------------------------------------------------------------------------------------
# The Delaunay monitor and the per-tetrahedron state transfer (csrc/tn_delaunay_core.h, csrc/tn_delaunay.hip; DESIGN.md
# section 4.16), stated in float64 on numpy arrays -- or on torch tensors of any device, through the same text: the expressions
# use nothing but + - * abs and comparisons, one rounding per operation in the order written here, which is the order of the
# element functions.  IEEE double + - * are correctly rounded everywhere, so the results are, bit for bit, what the kernels give.

DELAUNAY_EPS = 2.0 ** -53
INSPHERE_BOUND = (16.0 + 224.0 * DELAUNAY_EPS) * DELAUNAY_EPS      # Shewchuk's stage-A bound of the in-sphere determinant
ORIENT_BOUND = (7.0 + 56.0 * DELAUNAY_EPS) * DELAUNAY_EPS          # ... and of the orientation determinant
FACE_HULL, FACE_REGULAR, FACE_VIOLATED, FACE_UNCERTAIN = 0, 1, 2, 3


def orient_det(p):
    """p float64 [n, 4, 3] -> (det, permanent) of the 3 x 3 orientation determinant translated by p3 (its sign is the opposite
    of tet_orient's)"""
    adx, ady, adz = p[:, 0, 0] - p[:, 3, 0], p[:, 0, 1] - p[:, 3, 1], p[:, 0, 2] - p[:, 3, 2]
    bdx, bdy, bdz = p[:, 1, 0] - p[:, 3, 0], p[:, 1, 1] - p[:, 3, 1], p[:, 1, 2] - p[:, 3, 2]
    cdx, cdy, cdz = p[:, 2, 0] - p[:, 3, 0], p[:, 2, 1] - p[:, 3, 1], p[:, 2, 2] - p[:, 3, 2]
    bdxcdy, cdxbdy = bdx * cdy, cdx * bdy
    cdxady, adxcdy = cdx * ady, adx * cdy
    adxbdy, bdxady = adx * bdy, bdx * ady
    det = (adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy)) + cdz * (adxbdy - bdxady)
    perm = ((abs(bdxcdy) + abs(cdxbdy)) * abs(adz) + (abs(cdxady) + abs(adxcdy)) * abs(bdz)) + (abs(adxbdy) + abs(bdxady)) * abs(cdz)
    return det, perm


def insphere_det(p, e):
    """p float64 [n, 4, 3], e float64 [n, 3] -> (det, permanent) of the 4 x 4 in-sphere determinant translated by e"""
    aex, aey, aez = p[:, 0, 0] - e[:, 0], p[:, 0, 1] - e[:, 1], p[:, 0, 2] - e[:, 2]
    bex, bey, bez = p[:, 1, 0] - e[:, 0], p[:, 1, 1] - e[:, 1], p[:, 1, 2] - e[:, 2]
    cex, cey, cez = p[:, 2, 0] - e[:, 0], p[:, 2, 1] - e[:, 1], p[:, 2, 2] - e[:, 2]
    dex, dey, dez = p[:, 3, 0] - e[:, 0], p[:, 3, 1] - e[:, 1], p[:, 3, 2] - e[:, 2]
    aexbey, bexaey = aex * bey, bex * aey
    ab = aexbey - bexaey
    bexcey, cexbey = bex * cey, cex * bey
    bc = bexcey - cexbey
    cexdey, dexcey = cex * dey, dex * cey
    cd = cexdey - dexcey
    dexaey, aexdey = dex * aey, aex * dey
    da = dexaey - aexdey
    aexcey, cexaey = aex * cey, cex * aey
    ac = aexcey - cexaey
    bexdey, dexbey = bex * dey, dex * bey
    bd = bexdey - dexbey
    abc = (aez * bc - bez * ac) + cez * ab
    bcd = (bez * cd - cez * bd) + dez * bc
    cda = (cez * da + dez * ac) + aez * cd
    dab = (dez * ab + aez * bd) + bez * da
    alift = (aex * aex + aey * aey) + aez * aez
    blift = (bex * bex + bey * bey) + bez * bez
    clift = (cex * cex + cey * cey) + cez * cez
    dlift = (dex * dex + dey * dey) + dez * dez
    det = (dlift * abc - clift * dab) + (blift * cda - alift * bcd)
    aezp, bezp, cezp, dezp = abs(aez), abs(bez), abs(cez), abs(dez)
    abp, bcp, cdp = abs(aexbey) + abs(bexaey), abs(bexcey) + abs(cexbey), abs(cexdey) + abs(dexcey)
    dap, acp, bdp = abs(dexaey) + abs(aexdey), abs(aexcey) + abs(cexaey), abs(bexdey) + abs(dexbey)
    perm = ((((cdp * bezp + bdp * cezp) + bcp * dezp) * alift + ((dap * cezp + acp * dezp) + cdp * aezp) * blift) +
            (((abp * dezp + bdp * aezp) + dap * bezp) * clift + ((bcp * aezp + acp * bezp) + abp * cezp) * dlift))
    return det, perm


def _as_index(x):
    """int64 ids of an integer array or tensor; the int32 view of a uint32 id (EMPTY = -1) comes back as the uint32"""
    if isinstance(x, torch.Tensor):
        v = x.long()
        return torch.where(v < 0, v + (1 << 32), v)
    v = np.asarray(x).astype(np.int64)
    return np.where(v < 0, v + (1 << 32), v)


def delaunay_faces(cells, face_tets):
    """The gather of the monitor.  cells integer [T, 4], face_tets integer [F, 2] (TetrahedraTracer.face_tables) ->
    (interior bool [F], t0 [n], t1 [n], e [n]) over the n interior faces: e = the first vertex of cells[t1] that cells[t0] does not
    name (the last one where it names all four)."""
    xp = torch if isinstance(cells, torch.Tensor) else np
    c, ft = _as_index(cells), _as_index(face_tets)
    interior = ft[:, 1] != EMPTY
    t0, t1 = ft[:, 0][interior], ft[:, 1][interior]
    c0, c1 = c[t0], c[t1]
    new = (c1[:, :, None] != c0[:, None, :]).all(-1)
    e = c1[:, 3]
    for k in (2, 1, 0):
        e = xp.where(new[:, k], c1[:, k], e)
    return interior, t0, t1, e


def delaunay_face_statement(cells, face_tets, xyz):
    """What tn_delaunay_check computes.  cells integer [T, 4], face_tets integer [F, 2], xyz float32 [V, 3]: numpy arrays, or
    torch tensors of one device (the result is of the same kind).  Returns a dict: "face_state" int8 [F] (0 hull, 1 regular,
    2 violated, 3 uncertain), "tet_violations" uint8 [T], "counters" int64 [4] = interior faces, violated, uncertain, violated
    with t0 certainly of negative orientation as stored; and, over the interior faces only, "interior" bool [F], "insphere" /
    "orient" = (det, permanent) of the two determinants."""
    as_torch = isinstance(xyz, torch.Tensor)
    xp = torch if as_torch else np
    if not as_torch:
        cells, face_tets, xyz = np.asarray(cells), np.asarray(face_tets), np.asarray(xyz)
    interior, t0, t1, e = delaunay_faces(cells, face_tets)
    x = xyz.double() if as_torch else xyz.astype(np.float64)
    p = x[_as_index(cells)[t0]]
    ins, ori = insphere_det(p, x[e]), orient_det(p)
    certain = (abs(ins[0]) > INSPHERE_BOUND * ins[1]) & (abs(ori[0]) > ORIENT_BOUND * ori[1])
    inside = (ins[0] > 0) == (ori[0] > 0)
    violated = certain & inside
    inverted = violated & (ori[0] > 0)
    T, F = len(cells), len(face_tets)
    if as_torch:
        state = torch.where(certain, torch.where(inside, FACE_VIOLATED, FACE_REGULAR), FACE_UNCERTAIN).to(torch.int8)
        face_state = torch.zeros(F, dtype=torch.int8, device=xyz.device)
        face_state[interior] = state
        per_tet = torch.bincount(torch.cat([t0[violated], t1[violated]]), minlength=T).to(torch.uint8)
        counters = torch.stack([interior.sum(), violated.sum(), (~certain).sum(), inverted.sum()])
    else:
        state = np.where(certain, np.where(inside, FACE_VIOLATED, FACE_REGULAR), FACE_UNCERTAIN).astype(np.int8)
        face_state = np.zeros(F, np.int8)
        face_state[interior] = state
        per_tet = np.bincount(np.concatenate([t0[violated], t1[violated]]), minlength=T).astype(np.uint8)
        counters = np.array([interior.sum(), violated.sum(), (~certain).sum(), inverted.sum()], np.int64)
    return {"face_state": face_state, "tet_violations": per_tet, "counters": counters, "interior": interior, "insphere": ins,
            "orient": ori}


def remap_tet_values_statement(old_cells, new_cells, values, num_vertices: int):
    """What tn_remap_tet_values computes.  old_cells integer [T, 4], values float32 [T], new_cells integer [T', 4]: numpy arrays, or
    torch tensors of one device.  star_max[v] = the largest value over the old cells that name v (0 where none does), new value
    = the largest star_max of the new cell's four vertices -- "largest" by the values' BIT PATTERNS as unsigned integers, which is
    the larger float for the non-negative values the transfer is for; NaN and negative values follow that rule unchecked.
    Vertex ids >= num_vertices are passed over.  Returns {"values": float32 [T'], "star_max": float32 [num_vertices]}."""
    V = int(num_vertices)
    if isinstance(values, torch.Tensor):
        co, cn = _as_index(old_cells), _as_index(new_cells)
        bits = values.contiguous().view(torch.int32).long() & 0xFFFFFFFF
        ok = co < V
        star = torch.zeros(V, dtype=torch.int64, device=values.device)
        star.scatter_reduce_(0, co[ok], bits[:, None].expand(-1, 4)[ok], "amax", include_self=True)
        okn = cn < V
        got = torch.where(okn, star[torch.where(okn, cn, torch.zeros_like(cn))], torch.zeros_like(cn)).amax(1) if len(cn) else star[:0]
        f32 = lambda b: torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32).view(torch.float32)   # noqa: E731
        return {"values": f32(got), "star_max": f32(star)}
    co, cn = _as_index(old_cells), _as_index(new_cells)
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    ok = co < V
    star = np.zeros(V, np.uint32)
    np.maximum.at(star, co[ok], np.broadcast_to(bits[:, None], co.shape)[ok])
    okn = cn < V
    got = np.where(okn, star[np.where(okn, cn, 0)], 0).astype(np.uint32).max(1) if len(cn) else star[:0]
    return {"values": got.view(np.float32), "star_max": star.view(np.float32)}


# ---------------------------------------------------------------------------------------------------------------------------
# The isosurface extraction (csrc/tn_isosurface_core.h, csrc/tn_isosurface.hip), stated in numpy: marching
# tetrahedra on the mesh itself.  The positions are float32 + - * / on float32 arrays -- numpy rounds every operation once and
# fuses nothing, which is the arithmetic of the element functions -- and the orientation is _vol6 in float64, the expression of
# tn::guard::tet_orient.  Every array is, bit for bit, what the kernels give.

ISO_VALUE_LIMIT = 2.0 ** 126           # values and level must be below it in magnitude
ISO_MAX_TETS = 1 << 30
ISO_EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# ISO_TRI_TABLE[code][row] = the three tet edges of triangle `row` for the inside code (bit c = corner c is inside), -1 = none;
# written for a tetrahedron of non-negative orientation so that (q1-q0) x (q2-q0) points towards values < level
ISO_TRI_TABLE = (
    ((-1, -1, -1), (-1, -1, -1)),
    ((0, 1, 2), (-1, -1, -1)),
    ((0, 4, 3), (-1, -1, -1)),
    ((1, 2, 4), (1, 4, 3)),
    ((1, 3, 5), (-1, -1, -1)),
    ((0, 3, 5), (0, 5, 2)),
    ((0, 4, 5), (0, 5, 1)),
    ((2, 4, 5), (-1, -1, -1)),
    ((2, 5, 4), (-1, -1, -1)),
    ((0, 1, 5), (0, 5, 4)),
    ((0, 2, 5), (0, 5, 3)),
    ((1, 5, 3), (-1, -1, -1)),
    ((1, 3, 4), (1, 4, 2)),
    ((0, 3, 4), (-1, -1, -1)),
    ((0, 2, 1), (-1, -1, -1)),
    ((-1, -1, -1), (-1, -1, -1)),
)


def _to_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def isosurface_statement(xyz, cells, values, level, tet_mask=None):
    """What tn_isosurface_count + tn_isosurface_emit compute.  xyz float32 [V, 3], cells integer [T, 4] (any tetrahedron soup),
    values float32 [V], level a float (finite, |level| < 2^126: ValueError otherwise), tet_mask [T] or None (0 = skip): numpy
    arrays, or torch tensors (copied to the host).

    inside(v) = values[v] >= level.  A tetrahedron is skipped if its mask is 0, an id is >= V, or one of its four values is not
    finite or is >= 2^126 in magnitude.  Tet edges 0..5 = ISO_EDGE_CORNERS in stored corner order; an edge crosses if its ends
    differ in `inside`; ISO_TRI_TABLE names the edges of the one or two triangles, corners 1 and 2 swapped where tet_orient is
    negative.  A surface vertex belongs to a mesh edge (a, b), a < b, and is xyz[a] + t (xyz[b] - xyz[a]) with
    t = (level - values[a]) / (values[b] - values[a]), all in float32, one rounding per operation.  Vertices ascend by
    (a << 32 | b), triangles by tetrahedron and then by table row.

    Returns a dict of numpy arrays: "positions" float32 [N, 3], "triangles" int32 [M, 3] (vertex ids), "triangle_tets" int32 [M],
    "edge_vertices" int32 [N, 2] = (a, b), "edge_t" float32 [N]; "tri_offsets" / "ref_offsets" uint32 [T + 1] (exclusive sums of
    the triangles / crossing edges per tetrahedron) and the ints "num_triangles" = M, "num_refs" (edge references before welding)."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    values = np.ascontiguousarray(_to_numpy(values), np.float32).reshape(-1)
    c = _as_index(_to_numpy(cells)).reshape(-1, 4)
    with np.errstate(over="ignore"):
        level = np.float32(level)                                             # the entries take a float
    if not abs(float(level)) < ISO_VALUE_LIMIT:
        raise ValueError("level must be finite and below 2^126 in magnitude")
    V, T = len(values), len(c)
    if T >= ISO_MAX_TETS:
        raise ValueError("num_cells must be below 2^30")
    ok = np.ones(T, bool) if tet_mask is None else _to_numpy(tet_mask).reshape(-1) != 0
    ok = ok & (c < V).all(1)
    safe = np.where(ok[:, None], c, 0)
    v = values[safe] if V else np.zeros((T, 4), np.float32)
    with np.errstate(invalid="ignore"):
        ok = ok & (np.abs(v) < np.float32(ISO_VALUE_LIMIT)).all(1)
        code = np.where(ok, ((v >= level) * np.array([1, 2, 4, 8])).sum(1), 0)
    table = np.asarray(ISO_TRI_TABLE, np.int64)
    ec = np.asarray(ISO_EDGE_CORNERS, np.int64)
    ntri = (table[code, :, 0] >= 0).sum(1)
    cross = (((code[:, None] >> ec[None, :, 0]) ^ (code[:, None] >> ec[None, :, 1])) & 1).astype(bool)       # [T, 6]
    nref = cross.sum(1)
    tri_offsets = np.concatenate([[0], np.cumsum(ntri)]).astype(np.uint32)
    ref_offsets = np.concatenate([[0], np.cumsum(nref)]).astype(np.uint32)
    # the edge references in slot order: by tetrahedron, then by tet edge
    tt, ee = np.nonzero(cross)
    u, w = c[tt, ec[ee, 0]], c[tt, ec[ee, 1]]
    key = (np.minimum(u, w).astype(np.uint64) << np.uint64(32)) | np.maximum(u, w).astype(np.uint64)
    ukey, slot_id = np.unique(key, return_inverse=True)
    slot_id = slot_id.reshape(-1)
    a, b = (ukey >> np.uint64(32)).astype(np.int64), (ukey & np.uint64(0xFFFFFFFF)).astype(np.int64)
    va, vb = values[a], values[b]
    t = (level - va) / (vb - va)
    positions = xyz[a] + t[:, None] * (xyz[b] - xyz[a])
    # the triangles
    M = int(tri_offsets[-1])
    triangles, triangle_tets = np.zeros((M, 3), np.int64), np.zeros(M, np.int64)
    rank = np.cumsum(cross, 1) - cross                                        # position of edge e among the crossing edges
    emitting = np.nonzero(ntri > 0)[0]
    negative = np.zeros(T, bool)
    negative[emitting] = _vol6(xyz.astype(np.float64)[c[emitting]]) < 0
    for row in (0, 1):
        tets = np.nonzero(ntri > row)[0]
        edges = table[code[tets], row]                                        # [n, 3]
        edges = np.where(negative[tets, None], edges[:, [0, 2, 1]], edges)
        slots = ref_offsets[tets].astype(np.int64)[:, None] + rank[tets[:, None], edges]
        index = tri_offsets[tets].astype(np.int64) + row
        triangles[index] = slot_id[slots]
        triangle_tets[index] = tets
    return {"positions": positions.astype(np.float32), "triangles": triangles.astype(np.int32),
            "triangle_tets": triangle_tets.astype(np.int32),
            "edge_vertices": np.stack([a, b], 1).astype(np.uint32).view(np.int32).reshape(-1, 2), "edge_t": t.astype(np.float32),
            "tri_offsets": tri_offsets, "ref_offsets": ref_offsets, "num_triangles": M, "num_refs": int(ref_offsets[-1])}


# The refinement of the surface vertices (csrc/tn_isosurface_core.h: refine_begin / refine_candidate / refine_select /
# refine_vertex; csrc/tn_isosurface_refine.hip), stated in numpy with the same float32 operations.

ISO_REFINE_CANDIDATES = 7
ISO_REFINE_MAX_ROUNDS = 8
ISO_REFINE_FROZEN, ISO_REFINE_BAD_IDS = 1, 2


def isosurface_refine_candidates(t_lo, t_hi):
    """The 7 candidates of every bracket, float32 [N, 7]: t_j = t_lo + (j / 8) * (t_hi - t_lo), j = 1..7, one rounding per
    operation; t_lo <= t_1 <= ... <= t_7 <= t_hi for 0 <= t_lo <= t_hi <= 1 (the proof: tn_isosurface_core.h)."""
    t_lo, t_hi = np.asarray(t_lo, np.float32).reshape(-1, 1), np.asarray(t_hi, np.float32).reshape(-1, 1)
    j = (np.arange(1, ISO_REFINE_CANDIDATES + 1, dtype=np.float32) * np.float32(0.125))[None]
    return (t_lo + j * (t_hi - t_lo)).astype(np.float32)


def isosurface_refine_select(bracket, flags, densities, level):
    """One round on the brackets float32 [N, 4] = (t_lo, t_hi, s_lo, s_hi) and flags uint8 [N], given the densities float32
    [N, 7] at isosurface_refine_candidates: returns the new (bracket, flags).  The first interval from t_lo whose ends differ in
    inside(s) = s >= level; a candidate that is not finite or is >= 2^126 in magnitude freezes its edge; a flagged edge stays."""
    bracket, flags = np.array(bracket, np.float32).reshape(-1, 4), np.array(flags, np.uint8).reshape(-1)
    s = np.asarray(densities, np.float32).reshape(-1, ISO_REFINE_CANDIDATES)
    level = np.float32(level)
    t = isosurface_refine_candidates(bracket[:, 0], bracket[:, 1])
    ts = np.concatenate([bracket[:, 0:1], t, bracket[:, 1:2]], 1)                 # [N, 9]
    ss = np.concatenate([bracket[:, 2:3], s, bracket[:, 3:4]], 1)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(s) < np.float32(ISO_VALUE_LIMIT)).all(1)
        inside = ss >= level
    differ = inside[:, :-1] != inside[:, 1:]                                      # [N, 8]
    first = differ.argmax(1)
    live = flags == 0
    frozen_now = live & (bad | ~differ.any(1))
    move = live & ~frozen_now
    rows = np.nonzero(move)[0]
    bracket[rows] = np.stack([ts[rows, first[rows]], ts[rows, first[rows] + 1], ss[rows, first[rows]], ss[rows, first[rows] + 1]], 1)
    flags[frozen_now] = ISO_REFINE_FROZEN
    return bracket, flags


def isosurface_refine_vertices(xyz, edge_vertices, bracket, level):
    """(edge_t float32 [N], positions float32 [N, 3]) of the brackets: q = (level - s_lo) / (s_hi - s_lo),
    t = t_lo + q (t_hi - t_lo) put back into [t_lo, t_hi] (t = q (t_hi - t_lo) where t_lo == 0: the sign of a zero stays),
    p = xyz[a] + t (xyz[b] - xyz[a]); an edge with an id >= V gives t = 0, p = 0."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    ev = _as_index(_to_numpy(edge_vertices)).reshape(-1, 2)
    br = np.asarray(bracket, np.float32).reshape(-1, 4)
    level = np.float32(level)
    ok = (ev < len(xyz)).all(1)
    a, b = np.where(ok, ev[:, 0], 0), np.where(ok, ev[:, 1], 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (level - br[:, 2]) / (br[:, 3] - br[:, 2])
        m = q * (br[:, 1] - br[:, 0])
        t = np.where(br[:, 0] == 0, m, br[:, 0] + m)
        t = np.where(~(t >= br[:, 0]), br[:, 0], np.where(t > br[:, 1], br[:, 1], t)).astype(np.float32)
        xa, xb = (xyz[a], xyz[b]) if len(xyz) else (np.zeros((len(ev), 3), np.float32),) * 2
        p = xa + t[:, None] * (xb - xa)
    t = np.where(ok, t, np.float32(0)).astype(np.float32)
    return t, np.where(ok[:, None], p, np.float32(0)).astype(np.float32)


def isosurface_refine_statement(xyz, edge_vertices, values, level, density_fn, rounds):
    """What tn_isosurface_refine_begin, `rounds` x (tn_isosurface_refine_points, density_fn, tn_isosurface_refine_select) and
    tn_isosurface_refine_vertices compute: every welded vertex of isosurface_statement moves along its own mesh edge (a, b) onto a
    crossing of density_fn, the topology untouched.  xyz float32 [V, 3], edge_vertices integer [N, 2] (a < b, as emitted), values
    float32 [V], level a float (finite, |level| < 2^126), rounds in 0..8 (ValueError otherwise).
    density_fn(a_ids int64 [n], b_ids int64 [n], t float32 [n]) -> float32 [n]: the density at xyz[a] + t (xyz[b] - xyz[a]); it is
    asked for all 7 N candidates of a round at once, in [N, 7] order.  rounds = 0 never calls it and returns
    isosurface_statement's edge_t and positions bit for bit.
    NOT covered: a tetrahedron whose four vertex values lie on one side is never visited (thin features between vertices stay
    missing); the triangles are chords of the surface, so the enclosed volume can shrink; of several crossings on one edge the one
    nearest a is taken; zero-area triangles are kept.
    Returns {"edge_t": float32 [N], "positions": float32 [N, 3], "edge_bracket": float32 [N, 4] = (t_lo, t_hi, s_lo, s_hi),
    "edge_frozen": uint8 [N] (0; 1 = frozen: a density or a value out of range, or values on one side; 2 = an id >= V),
    "brackets": the list of the rounds + 1 bracket arrays from the start on}."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    values = np.ascontiguousarray(_to_numpy(values), np.float32).reshape(-1)
    ev = _as_index(_to_numpy(edge_vertices)).reshape(-1, 2)
    with np.errstate(over="ignore"):
        level = np.float32(level)
    if not abs(float(level)) < ISO_VALUE_LIMIT:
        raise ValueError("level must be finite and below 2^126 in magnitude")
    rounds = int(rounds)
    if not 0 <= rounds <= ISO_REFINE_MAX_ROUNDS:
        raise ValueError("rounds must be in 0..8")
    if len(xyz) != len(values):
        raise ValueError("xyz and values must have one row per vertex")
    V, N = len(values), len(ev)
    ok = (ev < V).all(1)
    a, b = np.where(ok, ev[:, 0], 0), np.where(ok, ev[:, 1], 0)
    va, vb = (values[a], values[b]) if V else (np.zeros(N, np.float32),) * 2
    bracket = np.stack([np.zeros(N, np.float32), np.ones(N, np.float32), np.where(ok, va, 0), np.where(ok, vb, 0)], 1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        fine = (np.abs(va) < np.float32(ISO_VALUE_LIMIT)) & (np.abs(vb) < np.float32(ISO_VALUE_LIMIT)) & ((va >= level) != (vb >= level))
    flags = np.where(ok, np.where(fine, 0, ISO_REFINE_FROZEN), ISO_REFINE_BAD_IDS).astype(np.uint8)
    history = [bracket.copy()]
    for _ in range(rounds):
        t = isosurface_refine_candidates(bracket[:, 0], bracket[:, 1])
        s = np.asarray(density_fn(np.repeat(a, ISO_REFINE_CANDIDATES), np.repeat(b, ISO_REFINE_CANDIDATES), t.reshape(-1)), np.float32)
        bracket, flags = isosurface_refine_select(bracket, flags, s.reshape(N, ISO_REFINE_CANDIDATES), level)
        history.append(bracket.copy())
    edge_t, positions = isosurface_refine_vertices(xyz, ev, bracket, level)
    return {"edge_t": edge_t, "positions": positions, "edge_bracket": bracket, "edge_frozen": flags, "brackets": history}


# ---------------------------------------------------------------------------------------------------------------------------
# The tetrahedron split (csrc/tn_split_core.h, csrc/tn_split.hip), stated in numpy: selected tetrahedra
# are split 1 -> 4 at their centroids.  The centroid and the new per-vertex values are float32 + and * on float32 arrays, one
# rounding per operation in the order written; the orientations are _vol6 in float64, the expression of tn::guard::tet_orient.
# Every array is, bit for bit, what the kernels give.

SPLIT_MAX_CELLS = 1 << 30


def _sign64(v):
    return (v > 0).astype(np.int8) - (v < 0).astype(np.int8)                  # 0 also for NaN


def _mean4_f32(a, b, c, d):
    """((a + b) + (c + d)) * 0.25f on float32 arrays: split::mean4"""
    with np.errstate(over="ignore", invalid="ignore"):
        return ((a + b) + (c + d)) * np.float32(0.25)


def split_tetrahedra_statement(xyz, cells, select):
    """What tn_split_count + tn_split_emit compute.  xyz float32 [V, 3], cells integer [T, 4] (any tetrahedron soup), select [T]
    (non-zero = asked): numpy arrays, or torch tensors (copied to the host).

    Tetrahedron t is accepted iff it is asked, its four ids are < V, the orientation s of its stored row (the sign of _vol6 in
    float64 on the float32 coordinates, 0 also for NaN) is not 0, and each of its four children has that orientation s.  Child i is
    the stored row with slot i replaced by the centroid c = ((p0 + p1) + (p2 + p3)) * 0.25f per coordinate in float32.  With k =
    the accepted tetrahedra below t and K their total, the new vertex is V + k, child 0 overwrites row t, children 1, 2, 3 are
    rows T + 3k, T + 3k + 1, T + 3k + 2.

    Returns a dict of numpy arrays: "vertices" float32 [V + K, 3], "cells" int32 [T + 3K, 4], "cell_parent" int32 [T + 3K] (the
    row itself below T, the parent for an appended row), "vertex_parents" int32 [K, 4] (the parent's row as stored), "offsets"
    uint32 [T + 1] (exclusive sums of the accepted flags), "counters" uint32 [4] = asked, accepted, refused for a flat or inverted
    parent or child, refused for an id >= V; and the int "num_new" = K."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    c = _as_index(_to_numpy(cells)).reshape(-1, 4)
    asked = _to_numpy(select).reshape(-1) != 0
    V, T = len(xyz), len(c)
    if len(asked) != T:
        raise ValueError("select must have one entry per row of cells")
    ids_ok = (c < V).all(1)
    judged = np.nonzero(asked & ids_ok)[0]
    p = xyz[c[judged]]                                                        # float32 [n, 4, 3]
    cen = _mean4_f32(p[:, 0], p[:, 1], p[:, 2], p[:, 3])                      # float32 [n, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        s = _sign64(_vol6(p.astype(np.float64)))
        fine = s != 0
        for i in range(4):
            q = p.copy()
            q[:, i] = cen
            fine &= _sign64(_vol6(q.astype(np.float64))) == s
    accepted = np.zeros(T, bool)
    accepted[judged] = fine
    offsets = np.concatenate([[0], np.cumsum(accepted)]).astype(np.uint32)
    K = int(offsets[-1])
    if T + 3 * K >= SPLIT_MAX_CELLS or V + K >= 0xFFFFFFFF:
        raise ValueError("num_cells + 3 num_new must be below 2^30 and num_vertices + num_new below 2^32 - 1")
    parents = np.nonzero(accepted)[0]
    new_id = V + np.arange(K, dtype=np.int64)
    vertices = np.concatenate([xyz, cen[fine]], 0).astype(np.float32)
    out = np.concatenate([c, np.zeros((3 * K, 4), np.int64)], 0)
    cell_parent = np.concatenate([np.arange(T, dtype=np.int64), np.repeat(parents, 3)])
    for i in range(4):
        child = c[parents].copy()
        child[:, i] = new_id
        rows = parents if i == 0 else T + 3 * np.arange(K, dtype=np.int64) + (i - 1)
        out[rows] = child
    counters = np.array([asked.sum(), K, (asked & ids_ok).sum() - K, (asked & ~ids_ok).sum()], np.uint32)
    return {"vertices": vertices, "cells": out.astype(np.uint32).view(np.int32).reshape(-1, 4),
            "cell_parent": cell_parent.astype(np.int32), "vertex_parents": c[parents].astype(np.uint32).view(np.int32).reshape(-1, 4),
            "offsets": offsets, "counters": counters, "num_new": K}


def split_vertex_rows_statement(values, vertex_parents, new="mean"):
    """What tn_split_vertex_rows computes.  values float32 [rows, V], vertex_parents integer [K, 4] -> float32 [rows, V + K]: the
    old columns, then for new vertex k either ((x[a] + x[b]) + (x[c] + x[d])) * 0.25f in float32 with (a, b, c, d) =
    vertex_parents[k] (new = "mean": the centroid's form, so an affine function of the position is carried exactly up to these
    three roundings) or 0 (new = "zero").  A row of vertex_parents with an id >= V gives 0."""
    if new not in ("mean", "zero"):
        raise ValueError('new must be "mean" or "zero"')
    values = np.ascontiguousarray(_to_numpy(values), np.float32)
    if values.ndim != 2 or values.shape[0] == 0:
        raise ValueError("values must be [rows, V] with rows > 0")
    vp = _as_index(_to_numpy(vertex_parents)).reshape(-1, 4)
    rows, V = values.shape
    fresh = np.zeros((rows, len(vp)), np.float32)
    ok = (vp < V).all(1)
    if new == "mean" and ok.any():
        a, b, c, d = (values[:, vp[ok, j]] for j in range(4))
        fresh[:, ok] = _mean4_f32(a, b, c, d)
    return np.concatenate([values, fresh], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# The edge split (csrc/tn_edge_split_core.h, csrc/tn_edge_split.hip), stated in numpy and vectorised:
# selected edges are bisected at their midpoints together with every tetrahedron around them.  Every array is, bit for bit, what
# the kernels give.

EDGE_SPLIT_COUNTER_NAMES = ("asked", "asked_refused_id", "asked_refused_flat", "candidates", "refused_id", "refused_hull",
                            "refused_lost", "refused_flat", "accepted", "bisected")
_EDGE_CORNERS = np.array(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)))   # iso::EDGE_CORNERS
_ES_ID, _ES_HULL, _ES_LOST, _ES_FLAT = 1, 2, 4, 8


def _len2_f32(lo, hi):
    """(dx dx + dy dy) + dz dz of d = hi - lo on float32 [n, 3]: esplit::len2"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = hi - lo
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _beats(len_e, key_e, len_f, key_f):
    with np.errstate(invalid="ignore"):
        return (len_e > len_f) | ((len_e == len_f) & (key_e < key_f))


def _row_edges(c, p):
    """(key uint64 [n, 6], len2 float32 [n, 6], slot_lo [n, 6], slot_hi [n, 6]) of rows c int64 [n, 4] with positions p f32 [n, 4, 3]"""
    n = len(c)
    a, b = _EDGE_CORNERS[:, 0], _EDGE_CORNERS[:, 1]
    a_low = c[:, a] < c[:, b]
    slot_lo, slot_hi = np.where(a_low, a[None], b[None]), np.where(a_low, b[None], a[None])
    r = np.arange(n)[:, None]
    key = (c[r, slot_lo].astype(np.uint64) << np.uint64(32)) | c[r, slot_hi].astype(np.uint64)
    len2 = np.zeros((n, 6), np.float32)
    if p is not None:
        for e in range(6):
            len2[:, e] = _len2_f32(p[np.arange(n), slot_lo[:, e]], p[np.arange(n), slot_hi[:, e]])
    return key, len2, slot_lo, slot_hi


def split_edges_statement(xyz, cells, select, faces, face_tets):
    """What tn_edge_split_count(_tables) + tn_edge_split_emit compute.  xyz float32 [V, 3], cells integer [T, 4] (any tetrahedron
    soup), select [T] (non-zero = asked), faces integer [F, 3] and face_tets integer [F, 2] (the face table of the cells:
    oracle.build_faces, TetrahedraTracer.face_tables; a hull face has no second tetrahedron, -1): numpy arrays, or torch tensors
    (copied to the host).

    An edge is the sorted id pair (lo, hi), key = lo << 32 | hi, its squared length (dx dx + dy dy) + dz dz of d = p[hi] - p[lo] in
    float32.  Edge e beats f iff len2(e) > len2(f), or they are equal and key(e) < key(f); the best of a list is the first, replaced
    by every later one that beats it.  An asked tetrahedron whose ids are < V and whose stored orientation s is not 0 nominates the
    best of its six edges, in the order (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) of its slots; the candidates are the distinct
    nominated keys.  The winner of ANY row is the best candidate among its six edges.  A candidate is refused, in this precedence,
    because a row that holds it has an id >= V; because it is an edge of a hull face; because the winner of a row that holds it is
    another edge; because a row that holds it has orientation 0, or one of the row's two children has not the row's orientation
    (child 0: the slot of hi replaced by the midpoint ((p_lo + p_hi) + (p_lo + p_hi)) * 0.25f, child 1: the slot of lo).  The
    accepted edges are ranked j in ascending key order, the new vertex is V + j; a bisected row t with k bisected rows below it
    keeps child 0 and appends child 1 as row T + k.

    Returns a dict of numpy arrays: "vertices" float32 [V + K_v, 3], "cells" int32 [T + K_t, 4], "cell_parent" int32 [T + K_t],
    "vertex_parents" int32 [K_v, 4] = (lo, hi, lo, hi), "edge_vertices" int32 [K_v, 2], "bisected" uint8 [T], "tet_edge" int32 [T]
    (the rank of the row's accepted edge, -1 where it is not bisected), "tet_offsets" uint32 [T + 1], "counters" uint32 [10]
    (EDGE_SPLIT_COUNTER_NAMES); and the ints "num_new" = K_v, "num_rows" = K_t, "num_cells" = T + K_t."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    c = _as_index(_to_numpy(cells)).reshape(-1, 4)
    asked = _to_numpy(select).reshape(-1) != 0
    f = _as_index(_to_numpy(faces)).reshape(-1, 3)
    ft = _as_index(_to_numpy(face_tets)).reshape(-1, 2)
    V, T = len(xyz), len(c)
    if len(asked) != T:
        raise ValueError("select must have one entry per row of cells")
    if len(f) != len(ft):
        raise ValueError("faces and face_tets must have one row per face")
    ids_ok = (c < V).all(1)
    good = np.nonzero(ids_ok)[0]
    cg = c[good]
    p = xyz[cg]                                                               # float32 [n, 4, 3]
    n, rows = len(good), np.arange(len(good))
    with np.errstate(invalid="ignore", over="ignore"):
        s = _sign64(_vol6(p.astype(np.float64)))
    key, len2, slot_lo, slot_hi = _row_edges(cg, p)

    # candidates: the best edge of every asked, well-formed row that is not flat
    best = np.zeros(n, np.int64)
    for e in range(1, 6):
        better = _beats(len2[:, e], key[:, e], len2[rows, best], key[rows, best])
        best = np.where(better, e, best)
    nominates = asked[good] & (s != 0)
    cand = np.unique(key[rows, best][nominates])                              # ascending uint64 [C]
    C = len(cand)
    flags = np.zeros(C, np.uint32)

    def find(k):
        at = np.searchsorted(cand, k)
        ok = (at < C) & (cand[np.minimum(at, max(C - 1, 0))] == k) if C else np.zeros(k.shape, bool)
        return np.where(ok, at, -1)

    # every well-formed row: its winner, what it says of the candidates it holds
    winner = np.full(T, -1, np.int64)
    if C:
        found = find(key)                                                     # [n, 6]
        w = np.full(n, -1, np.int64)                                          # the winning tet edge
        for e in range(6):
            has = found[:, e] >= 0
            wc = np.maximum(w, 0)
            better = has & ((w < 0) | _beats(len2[:, e], key[:, e], len2[rows, wc], key[rows, wc]))
            w = np.where(better, e, w)
        has_w = w >= 0
        wc = np.maximum(w, 0)
        lo_p, hi_p = p[rows, slot_lo[rows, wc]], p[rows, slot_hi[rows, wc]]
        mid = _mean4_f32(lo_p, hi_p, lo_p, hi_p)
        flat = s == 0
        with np.errstate(invalid="ignore", over="ignore"):
            for replaced in (slot_hi[rows, wc], slot_lo[rows, wc]):
                q = p.copy()
                q[rows, replaced] = mid
                flat = flat | (_sign64(_vol6(q.astype(np.float64))) != s)
        win_cand = np.where(has_w, found[rows, wc], -1)
        for e in range(6):
            has = found[:, e] >= 0
            lost = has & (found[:, e] != win_cand)
            np.bitwise_or.at(flags, found[lost, e], np.uint32(_ES_LOST))
        np.bitwise_or.at(flags, win_cand[has_w & flat], np.uint32(_ES_FLAT))
        winner[good] = win_cand
        # rows with an id >= V: every candidate among their edges is refused for the id
        bad = c[~ids_ok]
        if len(bad):
            bkey, _, _, _ = _row_edges(bad, None)
            at = find(bkey)
            np.bitwise_or.at(flags, at[at >= 0], np.uint32(_ES_ID))
        # hull faces
        hull = f[ft[:, 1] == EMPTY]
        for k in range(3):
            u, v = hull[:, k], hull[:, (k + 1) % 3]
            hk = (np.minimum(u, v).astype(np.uint64) << np.uint64(32)) | np.maximum(u, v).astype(np.uint64)
            at = find(hk)
            np.bitwise_or.at(flags, at[at >= 0], np.uint32(_ES_HULL))

    r_id = (flags & _ES_ID) != 0
    r_hull = ~r_id & ((flags & _ES_HULL) != 0)
    r_lost = ~r_id & ~r_hull & ((flags & _ES_LOST) != 0)
    r_flat = ~r_id & ~r_hull & ~r_lost & ((flags & _ES_FLAT) != 0)
    accepted = flags == 0
    rank = np.concatenate([[0], np.cumsum(accepted)]).astype(np.int64)
    K_v = int(rank[-1])
    bisected = (winner >= 0) & accepted[np.maximum(winner, 0)] if C else np.zeros(T, bool)
    tet_edge = np.where(bisected, rank[np.maximum(winner, 0)] if C else 0, -1)
    tet_offsets = np.concatenate([[0], np.cumsum(bisected)]).astype(np.uint32)
    K_t = int(tet_offsets[-1])
    if T + K_t >= SPLIT_MAX_CELLS or V + K_v >= 0xFFFFFFFF:
        raise ValueError("num_cells + bisected rows must be below 2^30 and num_vertices + num_new below 2^32 - 1")
    acc_keys = cand[accepted]
    lo, hi = (acc_keys >> np.uint64(32)).astype(np.int64), (acc_keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    edge_vertices = np.stack([lo, hi], 1).reshape(-1, 2)
    mid = _mean4_f32(xyz[lo], xyz[hi], xyz[lo], xyz[hi]).reshape(-1, 3)
    vertices = np.concatenate([xyz, mid], 0).astype(np.float32)
    parents = np.nonzero(bisected)[0]
    j = tet_edge[parents]
    child0, child1 = c[parents].copy(), c[parents].copy()
    is_hi, is_lo = child0 == hi[j][:, None], child1 == lo[j][:, None]
    child0[np.arange(len(parents)), is_hi.argmax(1)] = V + j                  # the first slot that holds the id
    child1[np.arange(len(parents)), is_lo.argmax(1)] = V + j
    out = np.concatenate([c, child1], 0)
    out[parents] = child0
    cell_parent = np.concatenate([np.arange(T, dtype=np.int64), parents])
    counters = np.array([asked.sum(), (asked & ~ids_ok).sum(), (asked[good] & (s == 0)).sum(), C, r_id.sum(), r_hull.sum(),
                         r_lost.sum(), r_flat.sum(), K_v, K_t], np.uint32)
    as_i32 = lambda a, shape: np.ascontiguousarray(a.astype(np.int64).astype(np.uint32)).view(np.int32).reshape(shape)
    return {"vertices": vertices, "cells": as_i32(out, (-1, 4)), "cell_parent": cell_parent.astype(np.int32),
            "vertex_parents": as_i32(np.stack([lo, hi, lo, hi], 1), (-1, 4)), "edge_vertices": as_i32(edge_vertices, (-1, 2)),
            "bisected": bisected.astype(np.uint8), "tet_edge": as_i32(np.where(tet_edge < 0, 0xFFFFFFFF, tet_edge), (-1,)),
            "tet_offsets": tet_offsets, "counters": counters, "num_new": K_v, "num_rows": K_t, "num_cells": T + K_t}


# ---------------------------------------------------------------------------------------------------------------------------
# The Delaunay repair by bistellar flips (csrc/tn_flip_core.h, csrc/tn_flip.hip), stated in numpy and
# vectorised: a certainly violated interior face is removed by a 2-3 or a 3-2 flip.  The signs are those of orient_det /
# insphere_det above with their stage-A bounds; every array is, bit for bit, what the kernels give.

FLIP_COUNTER_NAMES = ("interior", "violated", "verdict_uncertain", "refused_id", "refused_invalid", "refused_uncertain",
                      "refused_unflippable", "refused_lost", "accepted_23", "accepted_32")
FLIP_NONE, FLIP_23, FLIP_32 = 0, 1, 2                      # face_flip's codes: FLIP_32 + the bad k
(FLIP_K_HULL, FLIP_K_REGULAR, FLIP_K_VERDICT_UNCERTAIN, FLIP_K_ID, FLIP_K_INVALID, FLIP_K_UNCERTAIN,
 FLIP_K_UNFLIPPABLE) = 8, 9, 10, 11, 12, 13, 14           # flip::Kind: what a face that is no flippable candidate is


def _orient_sign(q0, q1, q2, q3):
    """+1 / -1 where the sign of orient_det of the rows (q0, q1, q2, q3) float64 [n, 3] is certain, 0 where it is not"""
    det, perm = orient_det(np.stack([q0, q1, q2, q3], 1))
    return np.where(abs(det) > ORIENT_BOUND * perm, np.where(det > 0, 1, -1), 0)


def _apex_slot(c, f):
    """the first slot of each row c [n, 4] whose id is not one of f [n, 3]; -1 where every slot is"""
    free = (c[:, :, None] != f[:, None, :]).all(-1)
    return np.where(free.any(1), free.argmax(1), -1)


def flip_faces_statement(xyz, cells, faces, face_tets):
    """What tn_flip_count(_tables) + tn_flip_emit compute: ONE round of flips.  xyz float32 [V, 3], cells integer [T, 4], faces
    integer [F, 3] and face_tets integer [F, 2] (the face table of the cells; a hull face has no second tetrahedron, -1): numpy
    arrays, or torch tensors (copied to the host).

    For an interior face f: (a, b, c) = faces[f] as stored, t0, t1 = face_tets[f], d / e = the id in the first slot of row t0 / t1
    that is not one of a, b, c.  O(p, q, r, s) is the sign of orient_det, certain iff |det| > ORIENT_BOUND * permanent.  The face
    is refused for the first of: ID (t0 or t1 >= T, an id >= V among a, b, c and the two rows, or a row without such a slot: no
    position is read and the face has no verdict); -- then the verdict of delaunay_face_statement decides whether it is a
    candidate at all: only VIOLATED faces are --; INVALID (O(a,b,c,d) or O(a,b,c,e) uncertain, or equal); UNCERTAIN (one of o_k =
    O(x_k, y_k, d, e), (x_k, y_k) = (a,b), (b,c), (c,a), uncertain); UNFLIPPABLE (o_k is good iff it equals O(a,b,c,e); three good:
    a 2-3 flip of {t0, t1}; two good and the bad k: a 3-2 flip iff one row t2 is the neighbour of t0 and of t1 across their faces
    opposite the id of (a, b, c) that is not x_k, y_k -- through tet_faces and face_tets -- and holds x_k, y_k, d, e; anything
    else); LOST (a row it needs is claimed by a flippable candidate with a smaller face id).  Otherwise it is accepted.  Children:
    (x_k, y_k, d, e) for every good k ascending; child 0 takes t0's place, child 1 t1's, t2's place is deleted, child 2 of a 2-3
    flip is appended at (T - K32) + its rank among the accepted 2-3 flips in ascending face id.

    Returns a dict of numpy arrays: "cells" int32 [T', 4], "cell_sources" int32 [T', 3] (the old rows whose union holds the new
    one, -1 = none), "flipped" uint8 [T], "tet_flip" int32 [T] (the accepted face that takes the row, -1), "tet_offsets" uint32
    [T + 1], "face_flip" int32 [F, 3] = (code, t2, rank), "counters" uint32 [10] (FLIP_COUNTER_NAMES), "face_kind" int64 [F]
    (FLIP_K_* or the code of a flippable candidate, accepted or lost), "tet_faces" int64 [T, 4]; and the ints "num_23", "num_32",
    "num_cells" = T' = T + K23 - K32."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    c = _as_index(_to_numpy(cells)).reshape(-1, 4)
    f = _as_index(_to_numpy(faces)).reshape(-1, 3)
    ft = _as_index(_to_numpy(face_tets)).reshape(-1, 2)
    V, T, F = len(xyz), len(c), len(f)
    if len(ft) != F:
        raise ValueError("faces and face_tets must have one row per face")
    ids = np.arange(F)

    tet_faces = np.full((T, 4), EMPTY, np.int64)
    for side in (0, 1):
        at = ids[ft[:, side] < T]
        t = ft[at, side]
        slot = _apex_slot(c[t], f[at])
        tet_faces[t[slot >= 0], slot[slot >= 0]] = at[slot >= 0]

    interior = ft[:, 1] != EMPTY
    kind = np.where(interior, FLIP_K_ID, FLIP_K_HULL).astype(np.int64)
    third = np.full(F, EMPTY, np.int64)
    g = ids[interior & (ft[:, 0] < T) & (ft[:, 1] < T)]
    c0, c1, fg = c[ft[g, 0]], c[ft[g, 1]], f[g]
    s0, s1 = _apex_slot(c0, fg), _apex_slot(c1, fg)
    ok = (s0 >= 0) & (s1 >= 0) & (fg < V).all(1) & (c0 < V).all(1) & (c1 < V).all(1)
    g, c0, c1, fg, s0, s1 = g[ok], c0[ok], c1[ok], fg[ok], s0[ok], s1[ok]
    n, r = len(g), np.arange(len(g))
    t0, t1 = ft[g, 0], ft[g, 1]
    d, e = c0[r, s0], c1[r, s1]
    x = xyz.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        new = (c1[:, :, None] != c0[:, None, :]).all(-1)
        ev = c1[:, 3]
        for k in (2, 1, 0):
            ev = np.where(new[:, k], c1[:, k], ev)
        p = x[c0]
        ins, ori = insphere_det(p, x[ev]), orient_det(p)
        certain = (abs(ins[0]) > INSPHERE_BOUND * ins[1]) & (abs(ori[0]) > ORIENT_BOUND * ori[1])
        inside = (ins[0] > 0) == (ori[0] > 0)
        pa, pb, pc, pd, pe = x[fg[:, 0]], x[fg[:, 1]], x[fg[:, 2]], x[d], x[e]
        sd, se = _orient_sign(pa, pb, pc, pd), _orient_sign(pa, pb, pc, pe)
        o = np.stack([_orient_sign(pa, pb, pd, pe), _orient_sign(pb, pc, pd, pe), _orient_sign(pc, pa, pd, pe)], 1).reshape(n, 3)
    good = o == se[:, None]
    flippable = np.where(good.sum(1) == 3, FLIP_23, np.where(good.sum(1) == 2, FLIP_32 + (~good).argmax(1), FLIP_K_UNFLIPPABLE))
    kg = np.where(~certain, FLIP_K_VERDICT_UNCERTAIN, np.where(~inside, FLIP_K_REGULAR,
                  np.where((sd == 0) | (se == 0) | (sd == se), FLIP_K_INVALID, np.where((o == 0).any(1), FLIP_K_UNCERTAIN, flippable))))

    # the third row of the 3-2 candidates
    m = np.nonzero((kg >= FLIP_32) & (kg < FLIP_32 + 3))[0]
    if len(m):
        kb = kg[m] - FLIP_32
        xx, yy, zz = fg[m, kb], fg[m, (kb + 1) % 3], fg[m, (kb + 2) % 3]
        nb = []
        for cc, tt in ((c0[m], t0[m]), (c1[m], t1[m])):
            is_z = cc == zz[:, None]
            gf = tet_faces[tt, is_z.argmax(1)]
            okf = is_z.any(1) & (gf < F)
            gf = np.where(okf, gf, 0)
            u, w = ft[gf, 0], ft[gf, 1]
            nb.append(np.where(okf, np.where(u == tt, w, np.where(w == tt, u, EMPTY)), EMPTY))
        t2 = np.where((nb[0] == nb[1]) & (nb[0] < T) & (nb[0] != t0[m]) & (nb[0] != t1[m]), nb[0], EMPTY)
        c2 = c[np.where(t2 < T, t2, 0)] if T else np.zeros((len(m), 4), np.int64)
        have = np.ones(len(m), bool)
        for want in (xx, yy, d[m], e[m]):
            have &= (c2 == want[:, None]).any(1)
        t2 = np.where((t2 != EMPTY) & have, t2, EMPTY)
        kg[m] = np.where(t2 == EMPTY, FLIP_K_UNFLIPPABLE, kg[m])
        third[g[m]] = t2
    kind[g] = kg

    # the claims and the precedence
    claim = np.full(T, EMPTY, np.int64)
    cand = ids[kind < FLIP_K_HULL]
    ct0, ct1, ct2 = ft[cand, 0], ft[cand, 1], third[cand]
    has2 = ct2 != EMPTY
    np.minimum.at(claim, ct0, cand)
    np.minimum.at(claim, ct1, cand)
    np.minimum.at(claim, ct2[has2], cand[has2])
    won = (claim[ct0] == cand) & (claim[ct1] == cand) & (~has2 | (claim[np.where(has2, ct2, 0)] == cand)) if len(cand) else np.zeros(0, bool)
    acc = cand[won]
    code = np.zeros(F, np.int64)
    code[acc] = kind[acc]
    is23 = code == FLIP_23
    rank = np.concatenate([[0], np.cumsum(is23)]).astype(np.int64)
    K23, K32 = int(is23.sum()), int((code >= FLIP_32).sum())
    if T + K23 >= SPLIT_MAX_CELLS:
        raise ValueError("num_cells + accepted 2-3 flips must be below 2^30")
    face_flip = np.stack([code, np.where(code >= FLIP_32, third, EMPTY), np.where(is23, rank[:-1], EMPTY)], 1).reshape(F, 3)

    taken = (claim < F) & (code[np.where(claim < F, claim, 0)] != FLIP_NONE) if F else np.zeros(T, bool)
    owner = np.where(taken, claim, 0)
    rows = np.arange(T)
    kept = ~taken | (ft[owner, 0] == rows) | (ft[owner, 1] == rows) if F else np.ones(T, bool)
    tet_offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint32)
    T_new = T + K23 - K32
    out = np.zeros((T_new, 4), np.int64)
    src = np.full((T_new, 3), EMPTY, np.int64)
    plain = rows[~taken]
    out[tet_offsets[plain]] = c[plain]
    src[tet_offsets[plain], 0] = plain
    if len(acc):
        where_g = np.full(F, -1, np.int64)
        where_g[g] = r
        ag = where_g[acc]                                                     # accepted faces as rows of the judged arrays
        fa, da, ea, ka = fg[ag], d[ag], e[ag], code[acc]
        bad, ra = np.where(ka >= FLIP_32, ka - FLIP_32, 3), np.arange(len(acc))
        for j in range(3):                                                    # child j: the j-th good k in ascending order
            k = np.minimum(j + (bad <= j), 2)
            use = (ka == FLIP_23) if j == 2 else np.ones(len(acc), bool)      # (a 3-2 flip has no third child)
            row = np.stack([fa[ra, k], fa[ra, (k + 1) % 3], da, ea], 1)
            pos = (tet_offsets[ft[acc, 0]], tet_offsets[ft[acc, 1]], (T - K32) + rank[acc])[j].astype(np.int64)
            out[pos[use]] = row[use]
            src[pos[use], 0], src[pos[use], 1] = ft[acc[use], 0], ft[acc[use], 1]
            src[pos[use], 2] = np.where(ka[use] >= FLIP_32, third[acc[use]], EMPTY)
    viol = (kind < FLIP_K_HULL) | (kind >= FLIP_K_INVALID)
    counters = np.array([interior.sum(), viol.sum(), (kind == FLIP_K_VERDICT_UNCERTAIN).sum(), (kind == FLIP_K_ID).sum(),
                         (kind == FLIP_K_INVALID).sum(), (kind == FLIP_K_UNCERTAIN).sum(), (kind == FLIP_K_UNFLIPPABLE).sum(),
                         len(cand) - len(acc), K23, K32], np.uint32)
    as_i32 = lambda a, shape: np.ascontiguousarray(a.astype(np.int64).astype(np.uint32)).view(np.int32).reshape(shape)   # noqa: E731
    return {"cells": as_i32(out, (-1, 4)), "cell_sources": as_i32(src, (-1, 3)), "flipped": taken.astype(np.uint8),
            "tet_flip": as_i32(np.where(taken, claim, EMPTY), (-1,)), "tet_offsets": tet_offsets, "face_flip": as_i32(face_flip, (-1, 3)),
            "counters": counters, "face_kind": kind, "tet_faces": tet_faces, "num_23": K23, "num_32": K32, "num_cells": T_new}


def flip_tet_values_statement(values, cell_sources):
    """What flip_tet_values computes: per new row the largest value over its sources, by the values' bit patterns as unsigned
    integers (remap_tet_values_statement's rule).  values float32 [T], cell_sources integer [T', 3] (-1 = none) -> float32 [T']."""
    bits = np.ascontiguousarray(_to_numpy(values), np.float32).view(np.uint32)
    s = _as_index(_to_numpy(cell_sources)).reshape(-1, 3)
    got = np.where(s != EMPTY, bits[np.where(s != EMPTY, s, 0)], 0) if len(bits) else np.zeros(s.shape, np.uint32)
    return got.astype(np.uint32).max(1).view(np.float32) if len(s) else np.zeros(0, np.float32)


def flip_to_delaunay_statement(xyz, cells, face_table, max_rounds=32):
    """What TetrahedraTracer.flip_to_delaunay computes: rounds of flip_faces_statement until one accepts nothing or max_rounds is
    reached.  face_table(cells) -> (faces, face_tets) of the cells of every round.  Returns {"cells", "cell_sources" (composed:
    int64 [T', S] padded with EMPTY, the input rows whose union holds the row), "rounds" (the counters of every round run),
    "violated", "unflippable" (of the last round run: what is left), "num_rounds" (the rounds that accepted something)}."""
    cells = np.ascontiguousarray(_to_numpy(cells)).reshape(-1, 4)
    sources = np.arange(len(cells), dtype=np.int64)[:, None]
    rounds = []
    for _ in range(max(int(max_rounds), 0) + 1):
        faces, face_tets = face_table(cells)
        out = flip_faces_statement(xyz, cells, faces, face_tets)
        rounds.append(out["counters"])
        if out["num_23"] + out["num_32"] == 0 or len(rounds) > max_rounds:
            break
        cells = out["cells"]
        sources = compose_cell_sources(sources, out["cell_sources"])
    last = rounds[-1]
    return {"cells": cells, "cell_sources": sources, "rounds": rounds, "violated": int(last[1]), "unflippable": int(last[6]),
            "num_rounds": len(rounds) - 1}


def compose_cell_sources(sources, step):
    """sources integer [T, S] (EMPTY-padded input rows of every current row), step integer [T', 3] (flip_faces' cell_sources of
    one round) -> int64 [T', S'] the input rows of every new row: the union over its up to three sources, ascending, without
    repeats, padded with EMPTY and trimmed to the longest."""
    s = _as_index(np.asarray(step)).reshape(-1, 3)
    src = _as_index(np.asarray(sources))
    got = np.where((s != EMPTY)[:, :, None], src[np.where(s != EMPTY, s, 0)], EMPTY).reshape(len(s), -1)
    got = np.sort(got, 1)
    got[:, 1:][got[:, 1:] == got[:, :-1]] = EMPTY
    got = np.sort(got, 1)
    width = max(int((got != EMPTY).sum(1).max()) if len(got) else 1, 1)
    return got[:, :width]


# ---------------------------------------------------------------------------------------------------------------------------
# The face table of any cell rows (csrc/tn_build_core.h: face_hash_insert / face_is_first / face_emit; csrc/tn_build.hip:
# tn_face_table_count / tn_face_table_emit), stated in numpy.  No arithmetic: every array is, byte for
# byte, what the entries and a load of the same cells give.

FACE_TABLE_COUNTER_NAMES = ("faces", "hull_faces", "flags", "reserved")
FACE_TABLE_FLAG_CELL_OOB, FACE_TABLE_FLAG_TRIPLE_FACE = 1, 2     # tn_build_core.h: FLAG_CELL_OOB, FLAG_TRIPLE_FACE


def face_sightings_statement(cells):
    """The first half of the face table (tn_face_table_count).  Sighting i = 4 t + j is local face j of row t, the ids
    cells[t, (j+1)&3], cells[t, (j+2)&3], cells[t, (j+3)&3] (face_of_tet).  Sightings are keyed by their sorted id triple: a key seen
    once is a hull face, a key seen twice pairs its two sightings, a key seen three times or more is the build's "shared by more
    than two tetrahedra" (then the two smallest sightings are paired here and the others stand alone; the device leaves it open
    which two pair).  Rows need not be tetrahedra of a mesh: a row that repeats an id pairs its own sightings by the same rule.
    Returns (triples uint32 [4T, 3], partner uint32 [4T] -- the other sighting of the face, EMPTY for none --, face_index uint32
    [4T + 1] -- exclusive sums of "sighting i is the first of its face", the total F last --, triple: bool)."""
    c = _as_index(_to_numpy(cells)).reshape(-1, 4)
    n4, j = 4 * len(c), np.arange(4)
    tri = np.stack([c[:, (j + 1) & 3], c[:, (j + 2) & 3], c[:, (j + 3) & 3]], -1).reshape(n4, 3)
    key = np.sort(tri, 1)
    order = np.lexsort((np.arange(n4), key[:, 2], key[:, 1], key[:, 0]))        # by key, then by sighting
    sk = key[order]
    new = np.ones(n4, bool)
    new[1:] = (sk[1:] != sk[:-1]).any(1)
    start = np.flatnonzero(new)
    size = np.diff(np.append(start, n4))
    partner = np.full(n4, EMPTY, np.int64)
    a, b = order[start[size >= 2]], order[start[size >= 2] + 1]
    partner[a], partner[b] = b, a
    first = (partner == EMPTY) | (np.arange(n4) < partner)
    face_index = np.zeros(n4 + 1, np.uint32)
    face_index[1:] = np.cumsum(first)
    return tri.astype(np.uint32), partner.astype(np.uint32), face_index, bool((size >= 3).any())


def face_table_statement(cells, num_vertices=None):
    """What tn_face_table_count + tn_face_table_emit compute, and what load_tetrahedra builds: the face table of cells integer
    [T, 4] (numpy, or a torch tensor copied to the host; int32 ids are read as the uint32 they stand for).  With
    face_sightings_statement's pairs: a face is a pair or a lone sighting; its id is the rank of its first (smaller) sighting among
    the first sightings, so faces come in order of first sighting 4 t + j; its stored ids are its first sighting's, as face_of_tet
    orders them.
    Returns (faces uint32 [F, 3], face_tets uint32 [F, 2] = (row of the first sighting, row of its partner or EMPTY: a hull
    face), tet_faces uint32 [T, 4] = the face id of every sighting, counters uint32 [4] = F, hull faces, flag bits
    (FACE_TABLE_FLAG_CELL_OOB: an id >= num_vertices, never set with num_vertices None; FACE_TABLE_FLAG_TRIPLE_FACE: the table is
    then unspecified on the device), 0)."""
    tri, partner, face_index, triple = face_sightings_statement(cells)
    n4, F = len(partner), int(face_index[-1])
    fs = np.flatnonzero(face_index[1:] != face_index[:-1])                     # the first sightings, ascending
    p = partner[fs]
    faces = tri[fs].reshape(F, 3)
    face_tets = np.stack([fs >> 2, np.where(p == EMPTY, EMPTY, p >> 2)], 1).astype(np.uint32).reshape(F, 2)
    tet_faces = np.zeros(n4, np.uint32)
    ids = np.arange(F, dtype=np.uint32)
    tet_faces[fs] = ids
    tet_faces[p[p != EMPTY]] = ids[p != EMPTY]
    flags = FACE_TABLE_FLAG_TRIPLE_FACE if triple else 0
    if num_vertices is not None and n4 and int(tri.max()) >= int(num_vertices):
        flags |= FACE_TABLE_FLAG_CELL_OOB
    counters = np.array([F, int((partner == EMPTY).sum()), flags, 0], np.uint32)
    return faces, face_tets, tet_faces.reshape(-1, 4), counters


# ---------------------------------------------------------------------------------------------------------------------------
# Vertex pruning (csrc/tn_prune_core.h, csrc/tn_prune.hip), stated in numpy: asked vertices whose every
# tetrahedron is dead, and which lie on no hull face, are removed, and every per-vertex array is compacted.  No arithmetic: every
# array is, bit for bit, what the kernels give.

PRUNE_COUNTER_NAMES = ("asked", "removed", "kept_live", "kept_hull", "kept_unreferenced")


def prune_vertices_statement(xyz, cells, dead, faces, face_tets, vertex_select=None):
    """What tn_prune_count(_tables) + tn_prune_emit compute.  xyz float32 [V, 3], cells integer [T, 4] (any tetrahedron soup),
    dead [T] (non-zero = dead), faces integer [F, 3] and face_tets integer [F, 2] (a face table of the cells: oracle.build_faces,
    TetrahedraTracer.face_tables), vertex_select [V] or None (non-zero = asked; None: every vertex): numpy arrays, or torch
    tensors (copied to the host).  int32 ids are read as the uint32 they stand for (-1 = 0xFFFFFFFF).

    named[v]: some row of cells contains v.  live[v]: a row that is not dead, or that has an id >= V, contains v.  hull[v]: v is a
    vertex of a face with face_tets[f, 1] == 0xFFFFFFFF.  Ids >= V are skipped in every table.  An asked vertex is kept because
    live, else because hull, else because it is not named, else removed; a vertex that is not asked is kept.

    Returns a dict of numpy arrays: "vertices" float32 [V', 3] = xyz[kept_ids], "new_id" int32 [V] (the new id, -1 where
    removed), "kept_ids" int32 [V'] (ascending), "offsets" uint32 [V + 1] (exclusive sums of the keep flags), "counters" uint32
    [5] = asked, removed, kept live, kept hull, kept unreferenced (PRUNE_COUNTER_NAMES); and the ints "num_kept" = V',
    "num_removed"."""
    xyz = np.ascontiguousarray(_to_numpy(xyz), np.float32).reshape(-1, 3)
    c = _as_index(_to_numpy(cells)).reshape(-1, 4)
    is_dead = _to_numpy(dead).reshape(-1) != 0
    f = _as_index(_to_numpy(faces)).reshape(-1, 3)
    ft = _as_index(_to_numpy(face_tets)).reshape(-1, 2)
    V, T = len(xyz), len(c)
    if len(is_dead) != T:
        raise ValueError("dead must have one entry per row of cells")
    if len(f) != len(ft):
        raise ValueError("faces and face_tets must have one row per face")
    asked = np.ones(V, bool) if vertex_select is None else _to_numpy(vertex_select).reshape(-1) != 0
    if len(asked) != V:
        raise ValueError("vertex_select must have one entry per vertex")

    def mark(ids):
        m = np.zeros(V, bool)
        ids = ids.reshape(-1)
        m[ids[ids < V]] = True
        return m

    named = mark(c)
    live = mark(c[~is_dead | (c >= V).any(1)])
    hull = mark(f[ft[:, 1] == EMPTY])
    removed = asked & ~live & ~hull & named
    keep = ~removed
    offsets = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint32)
    kept_ids = np.nonzero(keep)[0]
    new_id = np.full(V, -1, np.int64)
    new_id[kept_ids] = np.arange(len(kept_ids))
    counters = np.array([asked.sum(), removed.sum(), (asked & live).sum(), (asked & ~live & hull).sum(),
                         (asked & ~live & ~hull & ~named).sum()], np.uint32)
    return {"vertices": np.ascontiguousarray(xyz[kept_ids]), "new_id": new_id.astype(np.int32), "kept_ids": kept_ids.astype(np.int32),
            "offsets": offsets, "counters": counters, "num_kept": len(kept_ids), "num_removed": int(removed.sum())}


def prune_vertex_rows_statement(values, kept_ids):
    """What tn_prune_vertex_rows computes.  values float32 [rows, V], kept_ids integer [V'] -> float32 [rows, V']:
    out[r, j] = values[r, kept_ids[j]], 0 where kept_ids[j] >= V."""
    values = np.ascontiguousarray(_to_numpy(values), np.float32)
    if values.ndim != 2 or values.shape[0] == 0:
        raise ValueError("values must be [rows, V] with rows > 0")
    ids = _as_index(_to_numpy(kept_ids)).reshape(-1)
    ok = ids < values.shape[1]
    out = np.zeros((values.shape[0], len(ids)), np.float32)
    out[:, ok] = values[:, ids[ok]]
    return out
