"""The sort key of the tracer's opt-in ray binning (TN_TRACE_BIN_RAYS / option "bin_rays"), stated once.

`ray_keys` is, float32 operation for float32 operation, what k_ray_keys (csrc/tn_ray_order.hip) computes on the device;
the library is built with -ffp-contract=off and correctly rounded division, so the two agree bit for bit and a binned
call walks its rays in the order `np.argsort(ray_keys(...), kind="stable")` (TetrahedraTracer.ray_order()).  numpy
only: nothing here needs a GPU or the library.

The key has KEY_BITS = 30 bits, from (origin, direction, mesh box) alone:
  bits 18..29  Morton code of the ORIGIN, 4 bits per axis, in the box [c - 3h, c + 3h]
  bits  0..17  Morton code of the point of the ray's LINE closest to c, 6 bits per axis, in the box [c - r, c + r]
with c the centre of the mesh box, h its half extent and r = |h|.  Rays that start in the same cell and pass the centre
on the same side cross the same tetrahedra.  The key is total: every quantisation clamps before it converts to an
integer, and a NaN compares false and lands in cell 0.
"""
from __future__ import annotations

import numpy as np

ORIGIN_BITS = 4          # per axis
POINT_BITS = 6           # per axis
KEY_BITS = 3 * (ORIGIN_BITS + POINT_BITS)

_f = np.float32


def _cell(x, cells):
    """float32 -> integer cell 0 .. cells - 1; NaN and everything below 0 -> 0, everything above (+inf too) -> cells - 1."""
    x = np.where(x > _f(0.0), x, _f(0.0))
    x = np.where(x < _f(cells - 1), x, _f(cells - 1))
    return x.astype(np.uint32)


def _morton(cx, cy, cz, bits):
    key = np.zeros(cx.shape, np.uint32)
    for i in range(bits):
        key |= ((cx >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i)
        key |= ((cy >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + 1)
        key |= ((cz >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + 2)
    return key


def box_constants(mesh_lo, mesh_hi):
    """(c [3], e [3], r): centre, three half extents and the half diagonal of the mesh box, in float32 as the library holds them."""
    lo = np.asarray(mesh_lo, _f).reshape(3)
    hi = np.asarray(mesh_hi, _f).reshape(3)
    with np.errstate(all="ignore"):
        c = (lo + hi) * _f(0.5)
        h = (hi - lo) * _f(0.5)
        e = h * _f(3.0)
        r = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    return c, e, _f(r)


def closest_points(origins, directions, mesh_lo, mesh_hi):
    """float32 [R,3]: the point of each ray's line that is closest to the centre of the mesh box (what the low key bits quantise)."""
    o = np.ascontiguousarray(origins, _f).reshape(-1, 3)
    d = np.ascontiguousarray(directions, _f).reshape(-1, 3)
    c, _, _ = box_constants(mesh_lo, mesh_hi)
    with np.errstate(all="ignore"):
        ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        wx, wy, wz = c[0] - ox, c[1] - oy, c[2] - oz
        dd = (dx * dx + dy * dy) + dz * dz
        t = ((wx * dx + wy * dy) + wz * dz) / dd
        return np.stack([ox + dx * t, oy + dy * t, oz + dz * t], -1)


def ray_keys(origins, directions, mesh_lo, mesh_hi) -> np.ndarray:
    """uint32 [R] sort keys of the rays (origins, directions: [R,3]) for a mesh whose referenced vertices span [mesh_lo, mesh_hi]."""
    o = np.ascontiguousarray(origins, _f).reshape(-1, 3)
    c, e, r = box_constants(mesh_lo, mesh_hi)
    p = closest_points(o, directions, mesh_lo, mesh_hi)
    no, npnt = _f(1 << (ORIGIN_BITS - 1)), _f(1 << (POINT_BITS - 1))
    with np.errstate(all="ignore"):
        co = [_cell(((o[:, k] - c[k]) / e[k]) * no + no, 1 << ORIGIN_BITS) for k in range(3)]
        cp = [_cell(((p[:, k] - c[k]) / r) * npnt + npnt, 1 << POINT_BITS) for k in range(3)]
    return (_morton(*co, ORIGIN_BITS) << np.uint32(3 * POINT_BITS)) | _morton(*cp, POINT_BITS)
