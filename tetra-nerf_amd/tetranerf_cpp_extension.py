"""Drop-in for the reference's pybind11 module `tetranerf_cpp_extension`
(/root/reference/src/py_binding.cpp:433-449), backed by libtetranerf_hip.so on MI355X.

Same names, argument meaning, result dictionaries, dtypes/shapes and error behaviour:

    TetrahedraTracer(device)                      py_binding.cpp:28-40
      .device                                     :218-220, 436
      .load_tetrahedra(xyz, cells)                :144-161
      .trace_rays(origins, directions, M)         :41-76
      .find_visited_cells(...)                    :163-216
    interpolate_values(vi, bc, field)             :298-330
    interpolate_values_backward(vi, bc, field, g) :341-372
    triangulate(points), find_average_spacing(points)   :229-256 (CGAL there; scipy here, CPU, offline)
    gather_uint32 / scatter_ema_uint32            :374-431 (not on the model path)

Host code is PyTorch plumbing only: tensor checks, output allocation (torch.empty -- the
kernels write every byte, so the reference's torch::zeros memset pass is not needed) and raw
pointers + the current HIP stream handed to the C-ABI.  Nothing here computes on the CPU and
nothing imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib


_POISON = os.environ.get("TETRANERF_HIP_POISON", "") not in ("", "0")


def _empty(*shape, dtype=torch.float32, device=None):
    """torch.empty for outputs and scratch (every kernel writes each byte it owns).  TETRANERF_HIP_POISON=1 (tests,
    debugging) pre-fills them with NaN / 0x7f7f7f7f so that a byte a kernel failed to write, or read before writing,
    shows up instead of inheriting whatever the allocator's block held."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    if _POISON and t.numel():
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(0x7F7F7F7F if t.dtype in (torch.int32, torch.int64) else 0x7F)
    return t


def _check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _check_input(x, name):
    _check(isinstance(x, torch.Tensor), f"{name} must be a tensor")
    _check(x.device.type == "cuda", f"{name} must be a CUDA tensor")
    _check(x.is_contiguous(), f"{name} must be contiguous")


# The wrappers below are on the path of every op call: at 4096 x 513 samples find_visited_cells is an 18 us kernel behind what
# used to be 21-27 us of Python per call (profiles/r06av_ops_host.txt), so the helpers avoid object construction: the raw
# stream handle instead of a torch Stream object, plain ints for pointers (every entry point has ctypes argtypes, which
# convert an int to a void pointer), and a device context only when the tracer's device is not the current one.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device) -> int:
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(device):
    """`with _on(dev):` = torch.cuda.device(dev) when another device is current, nothing otherwise."""
    if device.index is None or torch.cuda.current_device() == device.index:
        return _NO_GUARD
    return torch.cuda.device(device)


def _trace_rows(R, M, dev):
    """The five unwritten arrays of a trace over R rays with M slots each, under trace_rays' keys and in the order the C entries
    take them (`*map(_ptr, rows.values())`)."""
    return {
        "num_visited_cells": _empty((R,), dtype=torch.int32, device=dev),
        "visited_cells": _empty((R, M), dtype=torch.int32, device=dev),
        "barycentric_coordinates": _empty((R, M, 2, 3), dtype=torch.float32, device=dev),
        "hit_distances": _empty((R, M, 2), dtype=torch.float32, device=dev),
        "vertex_indices": _empty((R, M, 4), dtype=torch.int32, device=dev),
    }


class TetrahedraTracer:
    """OptiX-free tetrahedra tracer; API of PyTetrahedraTracer (py_binding.cpp:28-227)."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("The device argument must be a CUDA device.")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.tn_tracer_create(int(device.index), C.byref(h)))
        self._h = h
        self.tetrahedra_vertices = None
        self.tetrahedra_cells = None

    # read-only property, compared by the model to decide re-creation (model.py:398-402)
    @property
    def device(self):
        return self._device

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.tn_tracer_destroy(h)
        self.tetrahedra_vertices = None
        self.tetrahedra_cells = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_float_dim3(self, x, name):
        _check_input(x, name)
        _check(x.device == self._device, f"{name} must be on the same device")
        _check(x.dtype == torch.float32, f"{name} must have float32 type")
        _check(x.dim() >= 1 and x.size(-1) == 3, f"{name} must have last dimension with size 3")

    def load_tetrahedra(self, xyz, cells, refittable: bool = False):
        """PyTetrahedraTracer::load_tetrahedra (py_binding.cpp:144-161).  refittable (no reference counterpart; keyword; for THIS
        load): the tracer keeps what update_vertices needs (option "refit_tables"; tn_refit_table_bytes tells how much)."""
        self._check_float_dim3(xyz, "xyz")
        _check_input(cells, "cells")
        _check(cells.device == self._device, "cells must be on the same device")
        _check(cells.dim() >= 1 and cells.size(-1) == 4, "indices must have last dimension with size 4")
        _check(cells.dtype == torch.int32, "indices must have int32 type")
        # borrowed, not copied (tetrahedra_tracer.h:300-303): keep them alive
        self.tetrahedra_cells = cells
        self.tetrahedra_vertices = xyz
        invalidate_field_cache()   # a new mesh comes with a (re-)initialised field (model.py:349-392 writes it through .data)
        if refittable or self._refittable:
            self.set_option("refit_tables", int(bool(refittable)))
            self._refittable = bool(refittable)
        _lib.check(self._lib.tn_load_tetrahedra(
            self._h, xyz.numel() // 3, cells.numel() // 4, _ptr(xyz), _ptr(cells), _stream(self._device)))

    _refittable = False          # what the last load_tetrahedra(refittable=...) set the option to
    supports_refit = True

    def update_vertices(self, xyz):
        """The vertices moved, the cells did not (no reference counterpart: the reference reloads): tn_update_vertices recomputes
        what the tracer's tables hold of the positions and keeps everything topological, so every query answers as a tracer
        freshly loaded on `xyz` would, at a fraction of the load's cost.  xyz: float32 [V, 3] on the tracer's device with the
        loaded V -- the loaded tensor after an in-place update, or another one; borrowed from now on, like load_tetrahedra's.
        Needs load_tetrahedra(..., refittable=True) and the device build.  The field cache is NOT invalidated (the field did not
        change).  Records and BVH leaves keep the order the LOADED positions gave them: after large deformation, or when the
        cells change, load again.  A move after which tetrahedra overlap leaves a mesh the walk's certification does not cover,
        refitted or freshly loaded: limit_vertex_step(old, xyz) before this call shortens a move so that no tetrahedron inverts."""
        self._check_float_dim3(xyz, "xyz")
        _lib.check(self._lib.tn_update_vertices(self._h, xyz.numel() // 3, _ptr(xyz), _stream(self._device)))
        self.tetrahedra_vertices = xyz

    def refit_table_bytes(self) -> int:
        """device bytes kept for update_vertices beyond the tracer's tables (0 after a load without refittable=True)"""
        return int(self._lib.tn_refit_table_bytes(self._h))

    supports_vertex_step_limit = True
    VERTEX_GUARD_GRID_LANES = 1024 * 256     # lanes of the limiter's kernels at their grid cap (tn_vertex_guard.hip: GUARD_BLOCKS * BT)

    def _check_loaded_vertices(self, x, name):
        self._check_float_dim3(x, name)
        _check(self.tetrahedra_vertices is not None, "no mesh is loaded; call load_tetrahedra first")
        _check(x.dim() == 2 and x.size(0) == self.tetrahedra_vertices.numel() // 3,
               f"{name} must have shape [V, 3] with the V of the loaded mesh")

    def _xyz_or_loaded(self, xyz):
        """`xyz`, or the loaded vertices where it is None; checked against the loaded mesh"""
        if xyz is None:
            xyz = self.tetrahedra_vertices
            _check(xyz is not None, "no mesh is loaded; call load_tetrahedra first")
        self._check_loaded_vertices(xyz, "xyz")
        return xyz

    def _check_tet_values(self, tet_values, flat):
        """`tet_values` as a tuple of arrays over the loaded cells on the tracer's device: [T, ...], or float32 [T] where flat"""
        tet_values, T = tuple(tet_values), self.tetrahedra_cells.numel() // 4
        for t in tet_values:
            _check_input(t, "tet_values")
            ok = t.dim() >= 1 and t.size(0) == T and t.device == self._device
            _check(ok and (not flat or (t.dtype == torch.float32 and t.dim() == 1)),
                   f"tet_values must be {'float32 [T]' if flat else '[T, ...]'} arrays over the loaded cells, on the tracer's device")
        return tet_values

    def _check_rays(self, ray_origins, ray_directions, max_ray_triangles):
        """(R, M) of a trace: M = max_ray_triangles a power of 2, both ray arrays float32 [..., 3] on the device, as many of each"""
        M = int(max_ray_triangles)
        if M <= 0 or (M & (M - 1)) != 0:
            raise RuntimeError("max_ray_triangles must be a power of 2.")
        self._check_float_dim3(ray_origins, "ray_origins")
        self._check_float_dim3(ray_directions, "ray_directions")
        R = ray_origins.numel() // 3
        _check(ray_directions.numel() // 3 == R, "ray_origins and ray_directions must have the same number of rays")
        return R, M

    def tet_quality(self, xyz=None):
        """Width and orientation of every loaded tetrahedron on `xyz` (None: the loaded vertices), and the star width of every
        vertex (no reference counterpart; tn_tet_quality, geometry.tet_width_orient / star_width).  xyz: float32 [V, 3] on the
        tracer's device, any positions of the loaded mesh's vertices.  Returns {"width": f32 [T] -- the smallest extent of the
        tetrahedron over all directions, "orient": int8 [T] -- sign of its signed volume, "star_width": f32 [V] -- the smallest
        width around the vertex, +inf where no tetrahedron names it}.  No synchronisation."""
        with torch.no_grad():
            xyz = self._xyz_or_loaded(xyz)
            V, T, dev = xyz.size(0), self.tetrahedra_cells.numel() // 4, self._device
            width = _empty((T,), dtype=torch.float32, device=dev)
            orient = _empty((T,), dtype=torch.int8, device=dev)
            star = _empty((V,), dtype=torch.float32, device=dev)
            with _on(dev):
                _lib.check(self._lib.tn_tet_quality(self._h, V, _ptr(xyz), _ptr(width), _ptr(orient), _ptr(star), _stream(dev)))
            return {"width": width, "orient": orient, "star_width": star}

    def limit_vertex_step(self, xyz_old, xyz_new, fraction: float = 0.25, verify: bool = True):
        """Shorten the move xyz_old -> xyz_new per vertex so that no tetrahedron of the loaded mesh turns inside out (no
        reference counterpart; tn_limit_vertex_step, geometry.limit_vertex_step_statement; the rule and its proof: DESIGN.md
        section 4.11).  xyz_old: float32 [V, 3], the positions the mesh is valid on (the tracer's, at the last load or refit);
        xyz_new: float32 [V, 3], WRITTEN IN PLACE (pass `param.data` of an optimised tensor: the call runs under no_grad and bumps
        no version counter).  A vertex moves by at most fraction * its star width (fraction in (0, 0.45]); vertices whose star
        width is below 2^-17 of their largest |coordinate| stay where they were.  verify: also count the tetrahedra that flipped
        or collapsed all the same (one more pass; both 0 whenever the bound applies).
        Returns (counters int32 [4] on the device: clamped, frozen but asked to move, flipped, collapsed; star_width f32 [V]).
        Nothing is read back: look at the counters when you would synchronise anyway.  The tracer's tables are not touched --
        update_vertices(xyz_new) makes it follow.  Not covered: far-apart parts of the hull moving into each other."""
        with torch.no_grad():
            self._check_loaded_vertices(xyz_old, "xyz_old")
            self._check_loaded_vertices(xyz_new, "xyz_new")
            V, dev = xyz_old.size(0), self._device
            star = _empty((V,), dtype=torch.float32, device=dev)
            counters = _empty((4,), dtype=torch.int32, device=dev)
            with _on(dev):
                _lib.check(self._lib.tn_limit_vertex_step(self._h, V, _ptr(xyz_old), _ptr(xyz_new), float(fraction), _ptr(star),
                                                          _ptr(counters), 0 if verify else 1, _stream(dev)))
            return counters, star

    supports_delaunay_check = True
    DELAUNAY_GRID_LANES = 1024 * 256         # lanes of the monitor's kernels at their grid cap (tn_delaunay.hip: DELAUNAY_BLOCKS * BT)

    def delaunay_check(self, xyz=None, face_state: bool = False, tet_violations: bool = False):
        """Is the loaded mesh still Delaunay on `xyz` (None: the loaded vertices)?  (No reference counterpart; tn_delaunay_check,
        geometry.delaunay_face_statement; the predicate and its bound: DESIGN.md section 4.16.)  Every interior face is tested
        once: it is violated iff the vertex behind it lies strictly inside the circumsphere of the tetrahedron in front of it, in
        double with a proven error bound; a face the bound cannot decide (cospherical points, zero-volume tetrahedra) is uncertain.
        Returns {"counters": int32 [4] on the device -- interior faces, violated, uncertain, violated with a first tetrahedron of
        negative orientation as stored; "face_state": int8 [F] (0 hull, 1 regular, 2 violated, 3 uncertain; rows as
        face_tables()) or None; "tet_violations": uint8 [T], the violated faces of each tetrahedron, or None}.
        Nothing is read back: look at the counters when you would synchronise anyway.  The tracer is not touched."""
        with torch.no_grad():
            xyz = self._xyz_or_loaded(xyz)
            V, T, dev = xyz.size(0), self.tetrahedra_cells.numel() // 4, self._device
            counters = _empty((4,), dtype=torch.int32, device=dev)
            state = _empty((int(self._lib.tn_num_faces(self._h)),), dtype=torch.int8, device=dev) if face_state else None
            # counted through 32-bit atomics: whole words of storage behind the T bytes that are returned
            per_tet = _empty((4 * ((T + 3) // 4),), dtype=torch.uint8, device=dev) if tet_violations else None
            with _on(dev):
                _lib.check(self._lib.tn_delaunay_check(self._h, V, _ptr(xyz), _ptr(counters), _ptr(state), _ptr(per_tet), _stream(dev)))
            return {"counters": counters, "face_state": state, "tet_violations": None if per_tet is None else per_tet[:T]}

    def retriangulate(self, xyz, tet_values=()):
        """Give the vertices `xyz` (float32 [V, 3] on the tracer's device, the loaded V) new cells and load them: cells =
        triangulate(xyz) -- Qhull, on the CPU --, every array of `tet_values` (float32 [T] of values >= 0 on the loaded cells: the
        occupancy field) carried to the new cells by remap_tet_values, then load_tetrahedra(xyz, cells, refittable=what this tracer
        was loaded with).  Returns {"cells": int32 [T', 4] (borrowed by the tracer from now on), "tet_values": the carried arrays
        in the order given, "num_tetrahedra": T'}.  BLOCKING: a copy of the vertices to the host, the triangulation, and the load.
        If the triangulation fails the tracer stays as it was.  The field cache is invalidated, as by every load."""
        with torch.no_grad():
            self._check_loaded_vertices(xyz, "xyz")
            old_cells, V = self.tetrahedra_cells, xyz.size(0)
            tet_values = self._check_tet_values(tet_values, flat=True)
            cells = triangulate(xyz).to(torch.int32).contiguous()         # raises on a Qhull failure: nothing touched so far
            carried = [remap_tet_values(old_cells, cells, t, V) for t in tet_values]
            self.load_tetrahedra(xyz, cells, refittable=self._refittable)
            return {"cells": cells, "tet_values": carried, "num_tetrahedra": cells.size(0)}

    supports_isosurface = True
    ISOSURFACE_GRID_LANES = 1024 * 256       # lanes of the extraction's kernels at their grid cap (tn_isosurface.hip: ISO_BLOCKS * BT)

    def isosurface(self, values, level, tet_mask=None, xyz=None, refine=None):
        """The level set { values = level } of a per-vertex scalar on the LOADED cells, as a triangle mesh: `isosurface` (below)
        on the tracer's own tables.  values f32 [V]; tet_mask uint8 / bool [T] or None; xyz (None: the loaded vertices) f32 [V, 3],
        any positions of the loaded mesh's vertices.  Blocks on two small read-backs.  The tracer is not touched.
        refine (None: the extraction alone, nothing else runs): a dict with "rounds" (0..8) and either "field" f32 [64, V] and
        "weights" (optionally "mode") -- isosurface_refine on the network whose vertex densities `values` are -- or "density_fn",
        the callback of isosurface_refine_with; the vertices then move along their edges onto that density's level set."""
        xyz = self._xyz_or_loaded(xyz)
        surface = isosurface(xyz.detach(), self.tetrahedra_cells.reshape(-1, 4), values, level, tet_mask)
        if refine is None:
            return surface
        _check(isinstance(refine, dict) and "rounds" in refine and (("density_fn" in refine) != ("field" in refine and "weights" in refine)),
               'refine must be a dict with "rounds" and either "density_fn" or "field" and "weights"')
        if "density_fn" in refine:
            return isosurface_refine_with(surface, xyz.detach(), values, level, refine["density_fn"], refine["rounds"])
        return isosurface_refine(surface, xyz.detach(), values, level, refine["field"], refine["weights"], refine["rounds"],
                                 mode=refine.get("mode", "fp32"))

    supports_split = True
    SPLIT_GRID_LANES = 1024 * 256            # lanes of the split's kernels at their grid cap (tn_split.hip: SPLIT_BLOCKS * BT)

    def split_tetrahedra(self, select, vertex_rows=(), tet_values=()):
        """Split the selected tetrahedra of the LOADED mesh 1 -> 4 at their centroids and load the result: `split_tetrahedra`
        (below) on the tracer's own tables, every array of `vertex_rows` (f32 [rows, V]: the field, its optimiser's moments)
        carried by split_vertex_rows(new="mean"), every array of `tet_values` ([T, ...] on the loaded cells: the occupancy)
        carried as values[cell_parent] -- a child lies inside its parent, so this is exact --, then load_tetrahedra(new vertices,
        new cells, refittable=what this tracer was loaded with).  select: uint8 / bool [T].
        Returns split_tetrahedra's dict with "vertex_rows" and "tet_values" (the carried arrays in the order given) added; the
        tracer borrows "vertices" and "cells" from now on.  With K == 0 (nothing asked, or everything refused) the tracer is not
        touched and the inputs come back as they are.  BLOCKS on the one read-back of K, and on what load_tetrahedra reads back.
        The field cache is invalidated, as by every load."""
        with torch.no_grad():
            xyz, cells = self.tetrahedra_vertices, self.tetrahedra_cells
            _check(xyz is not None, "no mesh is loaded; call load_tetrahedra first")
            xyz, cells = xyz.detach().reshape(-1, 3), cells.reshape(-1, 4)
            V, T = xyz.size(0), cells.size(0)
            vertex_rows = tuple(vertex_rows)
            for v in vertex_rows:
                _check_input(v, "vertex_rows")
                _check(v.dtype == torch.float32 and v.dim() == 2 and v.size(1) == V and v.device == self._device,
                       "vertex_rows must be float32 [rows, V] arrays over the loaded vertices, on the tracer's device")
            tet_values = self._check_tet_values(tet_values, flat=False)
            out = split_tetrahedra(xyz, cells, select)
            if out["num_new"] == 0:
                out.update(vertices=self.tetrahedra_vertices, cells=self.tetrahedra_cells, vertex_rows=list(vertex_rows),
                           tet_values=list(tet_values))
                return out
            out["vertex_rows"] = [split_vertex_rows(v.detach(), out["vertex_parents"]) for v in vertex_rows]
            parent = out["cell_parent"].long()
            out["tet_values"] = [t.detach()[parent] for t in tet_values]
            self.load_tetrahedra(out["vertices"], out["cells"], refittable=self._refittable)
            return out

    supports_edge_split = True
    EDGE_SPLIT_GRID_LANES = 1024 * 256       # lanes of the edge split's kernels at their grid cap (tn_edge_split.hip: ESPLIT_BLOCKS * BT)

    def edge_split_count(self, select, xyz=None):
        """The first half of split_edges, alone: tn_edge_split_count on the tracer's own cells and face tables (split_edges' rule).
        select: uint8 / bool [T]; xyz (None: the loaded vertices) f32 [V, 3].  Returns the dict of device arrays "tet_offsets" i32
        [T + 1], "tet_edge" i32 [T], "bisected" uint8 [T], "edge_vertices" i32 [T, 2] (the first K_v rows are written), "counters"
        i32 [10].  No synchronisation; the tracer is not touched."""
        with torch.no_grad():
            xyz = self._xyz_or_loaded(xyz)
            V, T, dev = xyz.size(0), self.tetrahedra_cells.numel() // 4, self._device
            _check_input(select, "select")
            _check(select.dtype in (torch.uint8, torch.bool) and select.numel() == T and select.device == dev,
                   "select must be uint8 or bool [num_cells] on the tracer's device")
            with _on(dev):
                out = _edge_split_buffers(T, dev)
                _lib.check(self._lib.tn_edge_split_count(self._h, V, _ptr(xyz), _ptr(select), _ptr(out["tet_offsets"]), _ptr(out["tet_edge"]),
                                                         _ptr(out["bisected"]), _ptr(out["edge_vertices"]), _ptr(out["counters"]),
                                                         _stream(dev)))
            return out

    def split_edges(self, select, vertex_rows=(), tet_values=()):
        """Bisect the best edge of every selected tetrahedron of the LOADED mesh at its midpoint, together with every tetrahedron
        around it, and load the result: `split_edges` (below) on the tracer's own cells and face tables, every array of
        `vertex_rows` (f32 [rows, V]: the field, its optimiser's moments) carried by split_vertex_rows(new="mean") -- the new
        vertex's parents are (lo, hi, lo, hi) --, every array of `tet_values` ([T, ...] on the loaded cells: the occupancy) carried
        as values[cell_parent] -- the two children tile their parent, so this is exact --, then load_tetrahedra(new vertices, new
        cells, refittable=what this tracer was loaded with).  select: uint8 / bool [T].
        Returns split_edges' dict with "vertex_rows" and "tet_values" (the carried arrays in the order given) added; the tracer
        borrows "vertices" and "cells" from now on.  With K_v == 0 (nothing asked, or everything refused) the tracer is not touched
        and the inputs come back as they are.  BLOCKS on the one read-back of the counters, and on what load_tetrahedra reads
        back.  The field cache is invalidated, as by every load."""
        with torch.no_grad():
            xyz, cells = self.tetrahedra_vertices, self.tetrahedra_cells
            _check(xyz is not None, "no mesh is loaded; call load_tetrahedra first")
            xyz, cells = xyz.detach().reshape(-1, 3), cells.reshape(-1, 4)
            V = xyz.size(0)
            vertex_rows = tuple(vertex_rows)
            for v in vertex_rows:
                _check_input(v, "vertex_rows")
                _check(v.dtype == torch.float32 and v.dim() == 2 and v.size(1) == V and v.device == self._device,
                       "vertex_rows must be float32 [rows, V] arrays over the loaded vertices, on the tracer's device")
            tet_values = self._check_tet_values(tet_values, flat=False)
            with _on(self._device):
                out = _edge_split_emit(xyz, cells, self.edge_split_count(select, xyz))
            if out["num_new"] == 0:
                out.update(vertices=self.tetrahedra_vertices, cells=self.tetrahedra_cells, vertex_rows=list(vertex_rows),
                           tet_values=list(tet_values))
                return out
            out["vertex_rows"] = [split_vertex_rows(v.detach(), out["vertex_parents"]) for v in vertex_rows]
            parent = out["cell_parent"].long()
            out["tet_values"] = [t.detach()[parent] for t in tet_values]
            self.load_tetrahedra(out["vertices"], out["cells"], refittable=self._refittable)
            return out

    supports_flip = True
    FLIP_GRID_LANES = 1024 * 256             # lanes of the flip's kernels at their grid cap (tn_flip.hip: FLIP_BLOCKS * BT)

    def flip_count(self, xyz=None):
        """The first half of a round of flips, alone: tn_flip_count on the tracer's own cells and face tables (flip_faces' rule).
        xyz (None: the loaded vertices) f32 [V, 3].  Returns the dict of device arrays "tet_offsets" i32 [T + 1], "tet_flip" i32 [T],
        "flipped" uint8 [T], "face_flip" i32 [F, 3], "counters" i32 [10].  No synchronisation; the tracer is not touched."""
        with torch.no_grad():
            xyz = self._xyz_or_loaded(xyz)
            V, T, dev = xyz.size(0), self.tetrahedra_cells.numel() // 4, self._device
            with _on(dev):
                out = _flip_buffers(T, int(self._lib.tn_num_faces(self._h)), dev)
                _lib.check(self._lib.tn_flip_count(self._h, V, _ptr(xyz), _ptr(out["tet_offsets"]), _ptr(out["tet_flip"]),
                                                   _ptr(out["flipped"]), _ptr(out["face_flip"]), _ptr(out["counters"]), _stream(dev)))
            return out

    def flip_faces(self, xyz=None):
        """ONE round of flips on the loaded mesh, not loaded: flip_count, the read-back of the counters, tn_flip_emit_loaded.
        Returns flip_faces' dict (below); with nothing accepted "cells" is the loaded tensor itself.  The tracer is not touched."""
        with torch.no_grad():
            count = self.flip_count(xyz)
            cells = self.tetrahedra_cells.reshape(-1, 4)

            def emit(K23, K32, new_cells, sources):
                _lib.check(self._lib.tn_flip_emit_loaded(self._h, _ptr(count["tet_offsets"]), _ptr(count["tet_flip"]), _ptr(count["face_flip"]),
                                                         K23, K32, _ptr(new_cells), _ptr(sources), _stream(self._device)))
            with _on(self._device):
                return _flip_emit(cells, count, emit)

    supports_face_table = True               # flip_to_delaunay(reload="once"), cpp.face_table, cpp.flip_to_delaunay

    def flip_to_delaunay(self, xyz=None, tet_values=(), max_rounds=32, reload="round"):
        """Repair the Delaunay property of the LOADED mesh on `xyz` (None: the loaded vertices) by bistellar flips, on the device (no
        reference counterpart).  Rounds of flip_faces -- every certainly violated face that is flippable
        and wins its rows is removed by a 2-3 or a 3-2 flip -- until a round accepts nothing or max_rounds rounds have flipped.  No
        vertex is added or moved: per-vertex arrays (the field, its optimiser's moments) stay as they are.  Every array of
        `tet_values` (float32 [T] of values >= 0 on the loaded cells: the occupancy) is carried by flip_tet_values: a new row lies
        inside the union of its sources and takes the largest of their values.  The tracer is loaded with the cells of every round
        (the next round reads its face table) with refittable = what it was loaded with; when the first round accepts nothing it
        is not touched.  The precondition is a mesh without inverted tetrahedra (limit_vertex_step keeps it so).
        Returns {"cells": int32 [T', 4] (borrowed by the tracer from now on), "tet_values": the carried arrays, "cell_sources":
        int64 [T', S] (the input rows whose union holds the row, ascending, padded with -1), "rounds": the ten counters of every
        round run, as lists (geometry.FLIP_COUNTER_NAMES; the last round is the one that accepted nothing, or the first not run
        for max_rounds), "violated" and "unflippable": what that last round counted, "num_rounds": rounds that flipped,
        "num_tetrahedra": T'}.  BLOCKS per round on two small read-backs -- the counters between the two entries, and the width of
        the composed sources (compose_cell_sources) -- and on the loads.
        reload (keyword): "round" -- the above.  "once" -- the first round reads the tracer's own tables, every later round a face
        table built from that round's cells alone (tn_face_table_count / tn_face_table_emit; the free
        function flip_to_delaunay's loop), and the tracer is loaded exactly once, at the end, iff a round flipped: the same
        returned dict and borrow rules, the same two read-backs per round, one load's worth of Morton sort, walk records, hull
        tree and face BVH instead of one per round.  While the rounds run, and if one raises, the tracer holds the mesh it was
        called with."""
        _check(reload in ("round", "once"), 'reload must be "round" or "once"')
        with torch.no_grad():
            xyz = self._xyz_or_loaded(xyz)
            tet_values = list(self._check_tet_values(tet_values, flat=True))
            if reload == "once":
                loaded = self.tetrahedra_cells
                with _on(self._device):
                    count = self.flip_count(xyz)

                    def emit(K23, K32, new_cells, sources):
                        _lib.check(self._lib.tn_flip_emit_loaded(self._h, _ptr(count["tet_offsets"]), _ptr(count["tet_flip"]),
                                                                 _ptr(count["face_flip"]), K23, K32, _ptr(new_cells), _ptr(sources),
                                                                 _stream(self._device)))
                    out = _flip_rounds(xyz, loaded.reshape(-1, 4), int(self._lib.tn_num_faces(self._h)), count, emit, tet_values,
                                       max_rounds)
                if out["num_rounds"] == 0:
                    out["cells"] = loaded                                       # (returned as it is where nothing flips)
                else:
                    self.load_tetrahedra(xyz, out["cells"], refittable=self._refittable)
                return out
            cells = self.tetrahedra_cells                                       # (returned as it is where nothing flips)
            sources, rounds = torch.arange(cells.numel() // 4, dtype=torch.int64, device=self._device)[:, None], []
            while True:
                if len(rounds) >= int(max_rounds):                            # the round that is not run: counted, not emitted
                    rounds.append(self.flip_count(xyz)["counters"].tolist())
                    break
                out = self.flip_faces(xyz)
                rounds.append(out["counters"].tolist())
                if out["num_23"] + out["num_32"] == 0:
                    break
                cells = out["cells"]
                tet_values = [flip_tet_values(t.detach(), out["cell_sources"]) for t in tet_values]
                sources = compose_cell_sources(sources, out["cell_sources"])
                self.load_tetrahedra(xyz, cells, refittable=self._refittable)
            return {"cells": cells, "tet_values": tet_values, "cell_sources": sources, "rounds": rounds, "violated": rounds[-1][1],
                    "unflippable": rounds[-1][6], "num_rounds": len(rounds) - 1, "num_tetrahedra": cells.numel() // 4}

    supports_prune = True
    PRUNE_GRID_LANES = 1024 * 256            # lanes of the prune's kernels at their grid cap (tn_prune.hip: PRUNE_BLOCKS * BT)

    def prune_count(self, dead, vertex_select=None):
        """The first half of remove_vertices, alone: tn_prune_count on the tracer's own cells and face tables (prune_vertices'
        rule).  dead: uint8 / bool [T]; vertex_select: uint8 / bool [V] or None.  Returns (offsets i32 [V + 1] -- vertex v is
        removed iff offsets[v + 1] == offsets[v], V' = offsets[V] --, counters i32 [5]: asked, removed, kept live, kept hull,
        kept unreferenced), both on the device.  No synchronisation; the tracer is not touched."""
        with torch.no_grad():
            xyz = self.tetrahedra_vertices
            _check(xyz is not None, "no mesh is loaded; call load_tetrahedra first")
            V, T, dev = xyz.numel() // 3, self.tetrahedra_cells.numel() // 4, self._device
            _check_prune_masks(dead, vertex_select, T, V, dev)
            with _on(dev):
                offsets = _empty((V + 1,), dtype=torch.int32, device=dev)
                counters = _empty((5,), dtype=torch.int32, device=dev)
                _lib.check(self._lib.tn_prune_count(self._h, V, _ptr(dead), _ptr(vertex_select), _ptr(offsets), _ptr(counters),
                                                    _stream(dev)))
            return offsets, counters

    def remove_vertices(self, dead, vertex_select=None, vertex_rows=(), tet_values=()):
        """Remove the vertices of the LOADED mesh that only dead tetrahedra name and that lie on no hull face, and load the
        Delaunay cells of the rest: tn_prune_count on the tracer's own cells and face tables, tn_prune_emit (prune_vertices'
        rule), cells = triangulate(kept points) -- Qhull, on the CPU --, every array of `vertex_rows` (f32 [rows, V]: the field,
        its optimiser's moments) carried by prune_vertex_rows, every array of `tet_values` (float32 [T] of values >= 0 on the
        loaded cells: the occupancy) carried by remap_tet_values(old cells, kept_ids[new cells]), then load_tetrahedra(kept
        points, new cells, refittable=what this tracer was loaded with).  dead: uint8 / bool [T]; vertex_select: uint8 / bool [V]
        or None.  Every hull-face vertex is kept, so the convex hull -- and with it the traced domain -- is unchanged wherever
        the loaded cells triangulate the convex hull of their points, as the reference's meshes do; it is not once moved
        vertices have bent the hull.
        Returns {"vertices": f32 [V', 3], "cells": i32 [T', 4] (both borrowed by the tracer from now on), "new_id", "kept_ids",
        "counters", "num_removed", "vertex_rows", "tet_values" (the carried arrays in the order given), "num_tetrahedra": T'}.
        With nothing removed the tracer is not touched and the inputs come back as they are; if the triangulation fails the
        tracer stays as it was.  BLOCKS on the read-back of V', the triangulation and the load.  The field cache is
        invalidated, as by every load."""
        with torch.no_grad():
            xyz, cells = self.tetrahedra_vertices, self.tetrahedra_cells
            _check(xyz is not None, "no mesh is loaded; call load_tetrahedra first")
            xyz, old_cells = xyz.detach().reshape(-1, 3), cells.reshape(-1, 4)
            V, T, dev = xyz.size(0), old_cells.size(0), self._device
            vertex_rows = tuple(vertex_rows)
            for v in vertex_rows:
                _check_input(v, "vertex_rows")
                _check(v.dtype == torch.float32 and v.dim() == 2 and v.size(1) == V and v.device == dev,
                       "vertex_rows must be float32 [rows, V] arrays over the loaded vertices, on the tracer's device")
            tet_values = self._check_tet_values(tet_values, flat=True)
            offsets, counters = self.prune_count(dead, vertex_select)
            with _on(dev):
                out = _prune_emit(xyz, offsets, counters)
            if out["num_removed"] == 0:
                out.update(vertices=self.tetrahedra_vertices, cells=self.tetrahedra_cells, vertex_rows=list(vertex_rows),
                           tet_values=list(tet_values), num_tetrahedra=T)
                return out
            new_cells = triangulate(out["vertices"]).to(torch.int32).contiguous()   # raises on a Qhull failure: nothing touched so far
            in_old_ids = out["kept_ids"][new_cells.long()].contiguous()
            out["vertex_rows"] = [prune_vertex_rows(v.detach(), out["kept_ids"]) for v in vertex_rows]
            out["tet_values"] = [remap_tet_values(old_cells, in_old_ids, t.detach(), V) for t in tet_values]
            self.load_tetrahedra(out["vertices"], new_cells, refittable=self._refittable)
            out.update(cells=new_cells, num_tetrahedra=new_cells.size(0))
            return out

    supports_compact_rows = True
    supports_bin_rays = True

    def trace_rays(self, ray_origins, ray_directions, max_ray_triangles, compact_rows: bool = False, bin_rays: bool = False):
        """PyTetrahedraTracer::trace_rays (py_binding.cpp:41-76).  compact_rows (no reference counterpart; per call):
        slots >= num_visited_cells are left unwritten (tn_trace_rays_ex + TN_TRACE_COMPACT_ROWS) for consumers that read
        the rows only through num_visited_cells (the samplers, find_visited_cells(ray_index=...), render_rays).
        bin_rays (no reference counterpart; per call; for INCOHERENT batches): the library walks the rays in a locality
        order of its own (TN_TRACE_BIN_RAYS; the key is ray_order.ray_keys) and writes every row at the caller's index:
        the same five arrays, bit for bit.  Small batches on the BVH path and chunked calls ignore it (ray_order())."""
        with torch.no_grad():
            R, M = self._check_rays(ray_origins, ray_directions, max_ray_triangles)
            out = _trace_rows(R, M, self._device)
            _lib.check(self._lib.tn_trace_rays_ex(
                self._h, R, M, _ptr(ray_origins), _ptr(ray_directions), *map(_ptr, out.values()),
                (1 if compact_rows else 0) | (2 if bin_rays else 0), _stream(self._device)))
        return out

    def trace_rays_triangles(self, ray_origins, ray_directions, max_ray_triangles):
        """PyTetrahedraTracer::trace_rays_triangles (py_binding.cpp:78-113): the sorted all-hits list."""
        with torch.no_grad():
            R, M = self._check_rays(ray_origins, ray_directions, max_ray_triangles)
            dev = self._device
            num = _empty((R,), dtype=torch.int32, device=dev)
            vis = _empty((R, M), dtype=torch.int32, device=dev)
            bary = _empty((R, M, 2), dtype=torch.float32, device=dev)
            dist = _empty((R, M), dtype=torch.float32, device=dev)
            verts = _empty((R, M, 3), dtype=torch.int32, device=dev)
            _lib.check(self._lib.tn_trace_rays_triangles(self._h, R, M, _ptr(ray_origins), _ptr(ray_directions), _ptr(num),
                                                         _ptr(vis), _ptr(bary), _ptr(dist), _ptr(verts), _stream(dev)))
        return {"num_visited_triangles": num, "visited_triangles": vis, "barycentric_coordinates": bary,
                "vertex_indices": verts, "hit_distances": dist}

    def find_tetrahedra(self, positions):
        """PyTetrahedraTracer::find_tetrahedra (py_binding.cpp:115-142): point location."""
        with torch.no_grad():
            self._check_float_dim3(positions, "positions")
            shape = tuple(positions.shape[:-1])
            N = positions.numel() // 3
            dev = self._device
            bary = _empty(shape + (3,), dtype=torch.float32, device=dev)
            verts = _empty(shape + (4,), dtype=torch.int32, device=dev)
            tets = _empty(shape, dtype=torch.int32, device=dev)
            _lib.check(self._lib.tn_find_tetrahedra(self._h, N, _ptr(positions), _ptr(tets), _ptr(bary), _ptr(verts),
                                                    _stream(dev)))
        return {"tetrahedra": tets, "barycentric_coordinates": bary, "vertex_indices": verts, "valid_mask": tets != -1}

    def find_visited_cells(self, num_visited_cells, visited_cells, barycentric_coordinates,
                           hit_distances, vertex_indices, distances, ray_index=None, count=None):
        """py_binding.cpp:163-216.  Addition: `ray_index` (int32 [r]) matches a SUBSET of the traced rays without
        compacting their rows first -- `distances` and the results are [r, S...], the trace tensors stay [R, M...];
        `count` (int32 [1] device tensor, with ray_index): only the first count[0] rows are matched (compact_hits)."""
        sdev = self._device
        for x, name in ((num_visited_cells, "num_visited_cells"), (visited_cells, "visited_cells"),
                        (barycentric_coordinates, "barycentric_coordinates"),
                        (hit_distances, "hit_distances"), (distances, "distances"),
                        (vertex_indices, "vertex_indices")):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous() and x.device == sdev):
                _check_input(x, name)                                   # (raises with the reference's messages)
                _check(x.device == sdev, f"{name} must be on the same device")
        _check(distances.dtype == torch.float32, "distances must have float32 type")
        R = num_visited_cells.size(0)
        _check(count is None or ray_index is not None, "find_visited_cells: `count` needs `ray_index` (it counts rows of that list)")
        if ray_index is not None:
            _check_input(ray_index, "ray_index")
            _check(ray_index.dtype == torch.int32 and ray_index.dim() == 1, "ray_index must be int32 [r]")
            _check(ray_index.device == self._device, "ray_index must be on the same device")
            R = ray_index.size(0)
        _check(distances.dim() == 2 and distances.size(0) == R,
               "distances must be of [num_rays, num_samples_per_ray] shape")
        _check(vertex_indices.size(-1) == 4, "vertex_indices must have last dimension with size 4")
        _check(self.tetrahedra_vertices is not None, "load_tetrahedra must be called first")
        _check(num_visited_cells.dtype == torch.int32 and visited_cells.dtype == torch.int32
               and vertex_indices.dtype == torch.int32, "index tensors must have int32 type")
        _check(hit_distances.dtype == torch.float32 and barycentric_coordinates.dtype == torch.float32,
               "hit_distances / barycentric_coordinates must have float32 type")
        S = distances.size(-1)
        M = visited_cells.size(1)
        dev = self._device
        mask = _empty((R, S), dtype=torch.bool, device=dev)
        matched_cells = _empty((R, S), dtype=torch.int32, device=dev)
        barycentric_coordinates_out = _empty((R, S, 3), dtype=torch.float32, device=dev)
        vertex_indices_out = _empty((R, S, 4), dtype=torch.int32, device=dev)
        # the C entry points take no device argument: launch with the tracer's device current (its stream, its pointers)
        with _on(dev):
            if ray_index is None:
                _lib.check(self._lib.tn_find_matched_cells(
                    R, S, M, _ptr(num_visited_cells), _ptr(visited_cells), _ptr(hit_distances),
                    _ptr(barycentric_coordinates), _ptr(distances), _ptr(vertex_indices), _ptr(matched_cells),
                    _ptr(vertex_indices_out), _ptr(mask), _ptr(barycentric_coordinates_out), _stream(dev)))
            else:
                _lib.check(self._lib.tn_find_matched_cells_indexed(
                    R, S, M, _ptr(ray_index), _ptr(num_visited_cells), _ptr(visited_cells), _ptr(hit_distances),
                    _ptr(barycentric_coordinates), _ptr(distances), _ptr(vertex_indices), _ptr(matched_cells),
                    _ptr(vertex_indices_out), _ptr(mask), _ptr(barycentric_coordinates_out), _ptr(count), _stream(dev)))
        return {
            "cell_indices": matched_cells,
            "vertex_indices": vertex_indices_out,
            "mask": mask,
            "barycentric_coordinates": barycentric_coordinates_out,
        }

    # -- additions (not in the reference surface) ------------------------------------------
    def trace_stats(self):
        """Counters of the last trace_rays call: rays certified by the walk / all others (literal pairing of the log +
        BVH re-trace) / rays whose pairing ran the serial literal branch / rays that overflowed M-1 hits."""
        arr = (C.c_uint64 * 4)()
        _lib.check(self._lib.tn_trace_stats(self._h, C.byref(arr)))
        return {"walk": arr[0], "general": arr[1], "serial": arr[2], "overflow": arr[3]}

    def flag_reasons(self):
        """Why the walk did not certify rays of the last trace_rays (reason code 1..12 -> count; include/tetranerf_hip.h);
        7 = sound chain with a gap below eps / a tie / an inversion, 13 = such rays whose logged hits went through the
        literal sort + pairing (the others were re-traced through the BVH); with option verify_stride: 15 = certified rays
        cross-checked against a count-only BVH traversal, 14 = those whose face count differed (handed to the BVH path)."""
        arr = (C.c_uint64 * 16)()
        _lib.check(self._lib.tn_trace_flag_reasons(self._h, C.byref(arr)))
        return {k: int(arr[k]) for k in range(1, 16) if arr[k]}

    def set_option(self, name: str, value: int):
        _lib.check(self._lib.tn_set_option(self._h, name.encode(), int(value)))

    def cross_check(self):
        """The cross-check of the walk's certification in the last trace_rays call (tn_trace_cross_check): the blind sample
        (every stride-th certified ray) and the risk classes (EVERY certified ray inside the wide band of a guard)."""
        arr = (C.c_uint64 * 8)()
        _lib.check(self._lib.tn_trace_cross_check(self._h, C.byref(arr)))
        return {"stride": int(arr[0]), "checked": int(arr[1]), "mismatches": int(arr[2]),
                "risk": {"hull_near_miss_rays": int(arr[3]), "thin_neighbourhood_rays": int(arr[4]), "checked": int(arr[5]),
                         "mismatches": int(arr[6])}}

    def ray_order(self):
        """The order in which the last trace_rays call walked its rays (tn_trace_ray_order): int64 numpy array, entry i =
        caller index of the i-th walked ray; empty when that call was not binned.  Test / diagnostic aid (synchronises)."""
        import numpy as np

        n = C.c_size_t(0)
        _lib.check(self._lib.tn_trace_ray_order(self._h, None, C.byref(n)))
        out = np.empty(n.value, np.uint32)
        if n.value:
            _lib.check(self._lib.tn_trace_ray_order(self._h, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out.astype(np.int64)

    TIMING_KEYS = ("speculative_fill", "walk", "bvh_fallback", "cross_check", "segment_writer", "literal_pairing", "tail_fill",
                   "cross_check_retrace")

    def trace_timings(self):
        """Per-kernel milliseconds of the last one-chunk walk call traced with set_option("timing", 1) (the kernels then run
        serialised on the caller's stream; tn_trace_timings)."""
        arr = (C.c_float * 8)()
        _lib.check(self._lib.tn_trace_timings(self._h, C.byref(arr)))
        return {k: float(arr[i]) for i, k in enumerate(self.TIMING_KEYS)}

    def face_tables(self):
        """(faces [F,3], face_tets [F,2]) int64 CPU tensors of the loaded mesh (debug aid)."""
        F = self._lib.tn_num_faces(self._h)
        faces = _empty((F, 3), dtype=torch.int32)
        ft = _empty((F, 2), dtype=torch.int32)
        _lib.check(self._lib.tn_get_faces(self._h, _ptr(faces), _ptr(ft)))
        return faces, ft

    def build_table(self, which: int):
        """One of the structures load_tetrahedra built, as a uint8 CPU tensor (test aid; see tn_get_build_table)."""
        n = C.c_size_t(0)
        _lib.check(self._lib.tn_get_build_table(self._h, int(which), None, C.byref(n)))
        out = _empty((n.value,), dtype=torch.uint8)
        if n.value:
            _lib.check(self._lib.tn_get_build_table(self._h, int(which), _ptr(out), C.byref(n)))
        return out

    def postprocess_hits(self, hit_count, hit_ids, hit_t, hit_uv, faces=None, face_tets=None):
        """Run only the dedupe/pairing stage on sorted hit rows (test aid); with `faces` [F,3] / `face_tets` [F,2]
        (int32) on those tables instead of the loaded mesh's."""
        R, M = hit_ids.shape
        dev = self._device
        out = _trace_rows(R, M, dev)
        hits = (_ptr(hit_count), _ptr(hit_ids), _ptr(hit_t), _ptr(hit_uv))
        if faces is not None:
            _check(face_tets is not None and faces.dtype == torch.int32 and face_tets.dtype == torch.int32
                   and faces.is_contiguous() and face_tets.is_contiguous(), "faces / face_tets must be contiguous int32")
            _lib.check(self._lib.tn_postprocess_hits_tables(dev.index or 0, R, M, _ptr(faces), _ptr(face_tets), *hits,
                                                            *map(_ptr, out.values()), _stream(dev)))
            return out
        _lib.check(self._lib.tn_postprocess_hits(self._h, R, M, *hits, *map(_ptr, out.values()), _stream(dev)))
        return out


def fill_rows(visited_cells, barycentric_coordinates, hit_distances, vertex_indices=None, first_slot=0):
    """The constant tails of trace_rays' dense rows (tn_fill_rows) from slot `first_slot` (a multiple of 32: a 128-byte line
    boundary of all four arrays; anything else raises) on, in place, for every row."""
    for x, name in ((visited_cells, "visited_cells"), (barycentric_coordinates, "barycentric_coordinates"),
                    (hit_distances, "hit_distances")) + (() if vertex_indices is None else ((vertex_indices, "vertex_indices"),)):
        _check_input(x, name)
    R, M = visited_cells.shape
    dev = visited_cells.device
    with _on(dev):
        _lib.check(_lib.load().tn_fill_rows(R, M, int(first_slot), _ptr(visited_cells), _ptr(barycentric_coordinates),
                                            _ptr(hit_distances), _ptr(vertex_indices), _stream(dev)))


# Vertex-major shadow copies [V, F] of feature-major fields [F, V] (the checkpoint layout, model.py:269-271).
#
# The gather kernels want one 256-byte row per vertex, the model keeps `tetrahedra_field` feature-major.  By default the
# shadow is made PER CALL (tn_transpose_f32: 23 MB of traffic at V = 45k, ~10 us) -- always correct.  A caller that owns
# the field can opt in to a cached shadow with `register_field(t)`: the copy is then refreshed only when the tensor's
# version counter or storage pointer moves (every in-place optimiser step, copy_ and load_state_dict bump the counter).
# What does NOT bump it are writes through `.data` (the reference model initialises the field that way,
# model.py:336-343,379-386: `self.tetrahedra_field.data[1:4, :] = ...`), so the owner of a registered field must call
# `invalidate_field_cache()` after any such write.  TetraRenderer and the nerfstudio adapter register their field and
# invalidate it from the model's initialisation hook; `TetrahedraTracer.load_tetrahedra` invalidates everything.
# A cached shadow remembers the event that ends its transposition: a consumer on another stream waits for it.
_FIELD_VM = {}        # id(tensor) -> (weakref, version, data_ptr, shadow, event)
# TETRANERF_HIP_CHECK_CACHES=1 (debug): every use of a cached field shadow compares it with the field (a device-wide
# comparison + synchronisation per call: for hunting stale caches, not for production)
_CHECK_CACHES = os.environ.get("TETRANERF_HIP_CHECK_CACHES", "0") == "1"


def register_field(field):
    """Opt in to a cached vertex-major shadow of `field` (see above).  Returns `field`."""
    import weakref

    hit = _FIELD_VM.get(id(field))
    if hit is None or hit[0]() is not field:      # (a dead entry whose id() was reused is replaced)
        key = id(field)

        def _drop(ref, key=key):                  # the field died: its [V,64] shadow (V * 256 bytes of HBM) goes with it
            cur = _FIELD_VM.get(key)
            if cur is not None and cur[0] is ref:
                del _FIELD_VM[key]

        _FIELD_VM[key] = (weakref.ref(field, _drop), None, None, None, None)
    return field


def field_is_registered(field) -> bool:
    hit = _FIELD_VM.get(id(field))
    return hit is not None and hit[0]() is field


def install_field_shadow(field, shadow, event=None):
    """Hand the cache of a registered `field` [F, V] a vertex-major `shadow` [V, F] that a kernel on the current stream has just
    written for the field's CURRENT version (optim.FusedRAdam: the step stores it in the pass that updates the field): the next
    field_vertex_major(field) returns it without a transposition.  `event` (a torch.cuda.Event to reuse; default a new one) is
    recorded on the current stream, as after a transposition.  The caller owns the claim that the two agree
    (TETRANERF_HIP_CHECK_CACHES=1 compares them at every use)."""
    hit = _FIELD_VM.get(id(field))
    _check(hit is not None and hit[0]() is field, "install_field_shadow: the field is not registered (cpp.register_field)")
    _check(shadow.dtype == torch.float32 and shadow.is_contiguous() and shadow.device == field.device
           and tuple(shadow.shape) == (field.shape[1], field.shape[0]), "install_field_shadow: shadow must be f32 [V, F] on the field's device")
    ev = torch.cuda.Event() if event is None else event
    ev.record(torch.cuda.current_stream(field.device))
    _FIELD_VM[id(field)] = (hit[0], field._version, field.data_ptr(), shadow, ev)
    return ev


def unregister_field(field):
    _FIELD_VM.pop(id(field), None)


def invalidate_field_cache(field=None):
    """Forget the cached shadow of `field` (all registered fields if None): required after a write through `.data`
    or a raw pointer; the registration itself stays."""
    for k, v in list(_FIELD_VM.items()):
        if v[0]() is None:
            del _FIELD_VM[k]
        elif field is None or v[0]() is field:
            _FIELD_VM[k] = (v[0], None, None, None, None)


def _transpose_field(field):
    Fd, V = field.shape
    ft = _empty((V, Fd), dtype=torch.float32, device=field.device)
    with _on(field.device):
        _lib.check(_lib.load().tn_transpose_f32(Fd, V, _ptr(field), _ptr(ft), _stream(field.device)))
    return ft


def field_vertex_major(field):
    """[V, F] copy of `field` [F, V]: per call, or cached per (tensor object, version, pointer) for registered fields."""
    hit = _FIELD_VM.get(id(field))
    if hit is None or hit[0]() is not field:
        # a detach()-ed alias of a registered field (autograd hands those to Function.backward): same storage, same
        # version counter
        hit = next((v for v in _FIELD_VM.values() if v[0]() is not None and v[2] == field.data_ptr()
                    and v[0]().shape == field.shape and v[0]()._version == field._version), None)
        if hit is None:
            return _transpose_field(field)
        field = hit[0]()
    if hit[1] == field._version and hit[2] == field.data_ptr() and hit[3] is not None:
        cur = torch.cuda.current_stream(field.device)
        cur.wait_event(hit[4])   # no-op on the producing stream; orders a consumer on another stream
        if _CHECK_CACHES and not torch.equal(hit[3], field.detach().t()):
            # (debug aid, TETRANERF_HIP_CHECK_CACHES=1: a write through `.data` / a raw pointer bumps no version counter)
            raise RuntimeError("the cached vertex-major shadow of a registered field is STALE: the field was written through "
                               ".data or a raw pointer without cpp.invalidate_field_cache(field)")
        return hit[3]
    ft = _transpose_field(field)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(field.device))
    _FIELD_VM[id(field)] = (hit[0], field._version, field.data_ptr(), ft, ev)
    return ft


def interpolate_values(vertex_indices, barycentric_coordinates, field):
    """py_interpolate_values (py_binding.cpp:298-330): returns [..., field_dim] as a
    moveaxis(0,-1) view of a contiguous [field_dim, n] buffer."""
    for x, name in ((vertex_indices, "vertex_indices"), (barycentric_coordinates, "barycentric_coordinates"),
                    (field, "field")):
        _check_input(x, name)
    _check(vertex_indices.dtype == torch.int32, "vertex_indices must be a tensor of type int32")
    _check(barycentric_coordinates.dtype == torch.float32, "barycentric_coordinates must be a tensor of type float32")
    _check(barycentric_coordinates.size(-1) + 1 == vertex_indices.size(-1),
           "barycentric_coordinates must have the same last dimension as vertex_indices - 1")
    _check(field.dtype == torch.float32, "field must be a tensor of type float32")
    D = vertex_indices.size(-1)
    _check(D in (2, 3, 4, 6), f"Unsupported interpolation dimension with value {D}")
    n = vertex_indices.numel() // D
    Fd = field.size(0)
    result = _empty((Fd,) + tuple(vertex_indices.shape[:-1]), dtype=field.dtype, device=field.device)
    ft = field_vertex_major(field)
    with _on(field.device):
        _lib.check(_lib.load().tn_interpolate_values_vm(
            D, n, Fd, _ptr(vertex_indices), _ptr(barycentric_coordinates), _ptr(ft), _ptr(result), _stream(field.device)))
    return result.moveaxis(0, -1)


def deterministic_gradients() -> bool:
    """Whether the field gradient (the gather's adjoint) is summed without float atomics: bit-identical from run to run, 3-5x
    the time of the atomic kernel (the twelve weight gradients are bit-reproducible either way).  On when the caller asked
    PyTorch for deterministic algorithms (`torch.use_deterministic_algorithms(True)`) or set DETERMINISTIC_FIELD_GRADIENT."""
    return bool(DETERMINISTIC_FIELD_GRADIENT) or torch.are_deterministic_algorithms_enabled()


DETERMINISTIC_FIELD_GRADIENT = False


def _gather_adjoint_vm(lib, D, V, n, Fd, vi, bc, rows, grad_vm, stream):
    if deterministic_gradients():
        _lib.check(lib.tn_interpolate_values_backward_vm_det(D, V, n, Fd, _ptr(vi), _ptr(bc), _ptr(rows), _ptr(grad_vm), stream))
    else:
        _lib.check(lib.tn_interpolate_values_backward_vm(D, n, Fd, _ptr(vi), _ptr(bc), _ptr(rows), _ptr(grad_vm), stream))


def interpolate_values_backward(vertex_indices, barycentric_coordinates, field, grad_in):
    """py_interpolate_values_backward (py_binding.cpp:341-372)."""
    for x, name in ((vertex_indices, "vertex_indices"), (barycentric_coordinates, "barycentric_coordinates"),
                    (field, "field"), (grad_in, "grad_in")):
        _check_input(x, name)
    _check(vertex_indices.dtype == torch.int32, "vertex_indices must be a tensor of type int32")
    _check(barycentric_coordinates.dtype == torch.float32, "barycentric_coordinates must be a tensor of type float32")
    _check(field.dtype == torch.float32, "field must be a tensor of type float32")
    _check(grad_in.dtype == torch.float32, "grad_in must be a tensor of type float32")
    _check(barycentric_coordinates.size(-1) + 1 == vertex_indices.size(-1),
           "barycentric_coordinates must have the same last dimension as vertex_indices - 1")
    D = vertex_indices.size(-1)
    _check(D in (2, 3, 4, 6), f"Unsupported interpolation dimension with value {D}")
    n = vertex_indices.numel() // D
    Fd, V = field.size(0), field.size(-1)
    _check(grad_in.size(-1) == Fd, "grad_in must have shape [..., field_dim]")
    grad_field_out = _empty((Fd, V), dtype=grad_in.dtype, device=grad_in.device)
    lib = _lib.load()
    if grad_in.moveaxis(-1, 0).is_contiguous() and Fd > 1 and not deterministic_gradients():
        # the reference's layout: a [Fd, n] buffer viewed as [..., Fd] (what py_binding.cpp:369 produces)
        with _on(field.device):
            _lib.check(lib.tn_interpolate_values_backward(D, V, n, Fd, _ptr(vertex_indices), _ptr(barycentric_coordinates),
                                                          _ptr(grad_in.moveaxis(-1, 0)), _ptr(grad_field_out),
                                                          _stream(field.device)))
        return grad_field_out
    # sample-major rows, the usual autograd gradient: consumed as is, accumulated vertex-major, transposed back once
    g = grad_in.contiguous()
    grad_vm = torch.zeros((V, Fd), dtype=torch.float32, device=grad_in.device)
    with _on(field.device):
        _gather_adjoint_vm(lib, D, V, n, Fd, vertex_indices, barycentric_coordinates, g, grad_vm, _stream(field.device))
        _lib.check(lib.tn_transpose_f32(V, Fd, _ptr(grad_vm), _ptr(grad_field_out), _stream(field.device)))
    return grad_field_out


def _bary_adjoint_vm(lib, D, n, Fd, vi, rows, field_vm, stream):
    """tn_interpolate_values_backward_bary_vm on checked arguments -> grad_bary f32 [n, D-1]"""
    grad_bary = _empty((n, D - 1), dtype=torch.float32, device=rows.device)
    _lib.check(lib.tn_interpolate_values_backward_bary_vm(D, n, Fd, _ptr(vi), _ptr(rows), _ptr(field_vm), _ptr(grad_bary), stream))
    return grad_bary


def interpolate_values_backward_barycentrics(vertex_indices, field, grad_in):
    """The gather's adjoint w.r.t. the barycentrics (tn_interpolate_values_backward_bary_vm; the gradient py_binding.cpp:354
    leaves as a TODO): grad_bary[..., k] = sum_c grad_in[..., c] (field[c, v_{k+1}] - field[c, v_0]), f32 [..., D-1]; the
    row of an EMPTY id is a zero row.  vertex_indices i32 [..., D], field f32 [F, V], grad_in f32 [..., F].  The vertex ids
    (tet membership) are constants of this gradient."""
    for x, name in ((vertex_indices, "vertex_indices"), (field, "field"), (grad_in, "grad_in")):
        _check_input(x, name)
    _check(vertex_indices.dtype == torch.int32, "vertex_indices must be a tensor of type int32")
    _check(field.dtype == torch.float32, "field must be a tensor of type float32")
    _check(grad_in.dtype == torch.float32, "grad_in must be a tensor of type float32")
    D = vertex_indices.size(-1)
    _check(D in (2, 3, 4, 6), f"Unsupported interpolation dimension with value {D}")
    n = vertex_indices.numel() // D
    Fd = field.size(0)
    _check(grad_in.size(-1) == Fd and grad_in.numel() == n * Fd, "grad_in must have shape [..., field_dim]")
    ft = field_vertex_major(field)
    with _on(field.device):
        grad_bary = _bary_adjoint_vm(_lib.load(), D, n, Fd, vertex_indices, grad_in, ft, _stream(field.device))
    return grad_bary.view(tuple(vertex_indices.shape[:-1]) + (D - 1,))


def sample_positions_backward(vertex_indices, barycentric_coordinates, grad_bary, vertices, distances=None, want_points=False,
                              want_origins=False, want_directions=False, want_vertices=False):
    """The adjoint of the sample position (tn_sample_positions_backward; completes add_barycentrics_grad,
    extension/__init__.py:45-68, as one kernel).  vertex_indices i32 [R, S, 4], barycentric_coordinates / grad_bary
    f32 [R, S, 3], vertices f32 [V, 3], distances f32 [R, S] (the sample distances t handed to find_visited_cells; needed
    for want_directions).  With T = rows (x_k - x_0) of the sample's tetrahedron, m = T^-1 grad_bary is dL/d(sample point):
        points [R,S,3] = m;  origins [R,3] = sum_s m;  directions [R,3] = sum_s t_s m   (p = o + t d, t held constant);
        vertices [V,3]: vertex v_k receives -w_k m, w = (1 - (b0+b1+b2), b0, b1, b2)
    -- summed with float atomics, or, under deterministic_gradients(), by one writer per element in a fixed order (-m
    through tn_interpolate_values_backward_vm_det with field_dim = 3).  Samples with an EMPTY id, a zero determinant or a
    non-finite m contribute exact zeros; an id-dead sample (an id that is EMPTY or >= V) does so whatever its barycentrics,
    distance and gradient hold, on the atomic and on the deterministic path.  Tet membership, t, near / far and the sampler
    draws are constants of the gradient.  Returns (points, origins, directions, vertices), None where not asked for."""
    for x, name in ((vertex_indices, "vertex_indices"), (barycentric_coordinates, "barycentric_coordinates"),
                    (grad_bary, "grad_bary"), (vertices, "vertices")) + (() if distances is None else ((distances, "distances"),)):
        _check_input(x, name)
    _check(vertex_indices.dtype == torch.int32 and vertex_indices.dim() == 3 and vertex_indices.size(-1) == 4,
           "vertex_indices must be i32 [R,S,4]")
    R, S = vertex_indices.size(0), vertex_indices.size(1)
    for x, name in ((barycentric_coordinates, "barycentric_coordinates"), (grad_bary, "grad_bary")):
        _check(x.dtype == torch.float32 and tuple(x.shape) == (R, S, 3), f"{name} must be f32 [R,S,3]")
    _check(vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.size(1) == 3, "vertices must be f32 [V,3]")
    _check(distances is None or (distances.dtype == torch.float32 and tuple(distances.shape) == (R, S)), "distances must be f32 [R,S]")
    _check(distances is not None or not want_directions, "want_directions needs the sample distances")
    dev, V = vertices.device, vertices.size(0)
    det = want_vertices and deterministic_gradients()
    points = _empty((R, S, 3), dtype=torch.float32, device=dev) if (want_points or det) else None
    origins = _empty((R, 3), dtype=torch.float32, device=dev) if want_origins else None
    directions = _empty((R, 3), dtype=torch.float32, device=dev) if want_directions else None
    grad_v = torch.zeros((V, 3), dtype=torch.float32, device=dev) if want_vertices else None
    lib = _lib.load()
    with _on(dev):
        stream = _stream(dev)
        _lib.check(lib.tn_sample_positions_backward(R, S, V, _ptr(vertex_indices), _ptr(barycentric_coordinates), _ptr(grad_bary),
                                                    _ptr(distances), _ptr(vertices), _ptr(points), _ptr(origins), _ptr(directions),
                                                    None if det else _ptr(grad_v), stream))
        if det and R * S:
            # the gather's adjoint skips an id >= V but still adds w * (-0) through the other three ids of that sample, which
            # is NaN for a non-finite w: a sample with any id that is EMPTY or >= V hands it four EMPTY ids
            absent = ((vertex_indices < 0) | (vertex_indices >= V)).any(-1, keepdim=True)
            ids = torch.where(absent, torch.full_like(vertex_indices, -1), vertex_indices)
            _lib.check(lib.tn_interpolate_values_backward_vm_det(4, V, R * S, 3, _ptr(ids), _ptr(barycentric_coordinates),
                                                                 _ptr(points.neg()), _ptr(grad_v), stream))
    return (points if want_points else None), origins, directions, grad_v


class _MlpWeightsStruct(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "wd", "bd", "wh", "bh", "wr", "br")]


_WEIGHT_SHAPES = [(128, 64), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,), (128, 155), (128,), (3, 128), (3,)]
_MODES = {"fp32": 0, "bf16x3": 1, "bf16": 2, 0: 0, 1: 1, 2: 2}


def _mode(mode, inference=True):
    """C-ABI value of an arithmetic of the fused MLP kernels.  "bf16" (plain bf16 products, fp32 accumulation: render.py,
    mlp_forward_bf16_statement) is an arithmetic of the evaluation forwards only: inference=False -- the training forward and
    the one-launch render -- refuses it."""
    m = _MODES.get(mode)
    _check(m is not None, 'mlp mode must be "fp32", "bf16x3" or (evaluation forwards only) "bf16"')
    _check(inference or m != 2, 'mlp mode must be "fp32" or "bf16x3" here: "bf16" is an arithmetic of the evaluation forwards '
                                '(mlp_forward, mlp_forward_gather, TetraRenderer.render) only')
    return m


class FusedMLP:
    """Handle of the fused MLP kernels (tn_mlp_*): holds the packed forms of ONE set of weights on the device.
    `sync(weights)` packs them when they changed since the last call -- detected through the tensors' identity, version
    counter and storage pointer, i.e. every in-place optimiser step / copy_ / load_state_dict is seen; a write through
    `.data` is not (call `sync(weights, force=True)` or `invalidate()` then).  weights = the 12 tensors
    (w1,b1,w2,b2,w3,b3,wd,bd,wh,bh,wr,br) in nn.Linear layout, contiguous fp32 on the handle's device."""

    def __init__(self, device):
        device = torch.device(device)
        _check(device.type == "cuda", "The device argument must be a CUDA device.")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.tn_mlp_create(int(device.index), C.byref(h)))
        self._h = h
        self._key = None

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.tn_mlp_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def invalidate(self):
        self._key = None

    def sync(self, weights, force=False):
        _check(len(weights) == 12, "weights must hold 12 tensors")
        import weakref

        # identity through weak references: id() of a collected tensor can be reused by a new one at the same address
        key = tuple((w._version, w.data_ptr()) for w in weights)
        if (not force and self._key is not None and key == self._key[0]
                and all(r() is w for r, w in zip(self._key[1], weights))):
            # the packs were made on the stream that was current then: a consumer on another stream waits for them
            torch.cuda.current_stream(self.device).wait_event(self._packed)
            return self
        st = _MlpWeightsStruct()
        keep = []
        for (name, _), w, shp in zip(_MlpWeightsStruct._fields_, weights, _WEIGHT_SHAPES):
            w = w.detach()
            _check_input(w, name)
            _check(w.device == self.device, f"{name} must be on the handle's device")
            _check(w.dtype == torch.float32 and tuple(w.shape) == shp, f"{name} must be f32 {shp}")
            keep.append(w)
            setattr(st, name, w.data_ptr())
        with _on(self.device):
            _lib.check(self._lib.tn_mlp_set_weights(self._h, C.byref(st), _stream(self.device)))
        del keep
        self._packed = torch.cuda.Event()
        self._packed.record(torch.cuda.current_stream(self.device))
        self._key = (key, [weakref.ref(w) for w in weights])
        return self

    @property
    def handle(self):
        return self._h


_DEFAULT_MLP = {}    # id(first weight tensor) -> (weakref to it, FusedMLP): one handle (packed weights + scratch) per MODEL
_MAX_HANDLES = 8     # (each holds ~1.5 MB of packs + 42 MB of gradient scratch once it has been trained with)


def fused_mlp(weights) -> FusedMLP:
    """The handle of this weight set, synchronised with `weights` (re-packed only when they changed).  Handles are keyed
    by the identity of the first weight tensor, so two models alternating on a device each keep their packs (a single
    per-device handle re-packed four weight forms on every switch); a handle dies with its model, the oldest one is
    dropped beyond _MAX_HANDLES.  Single-stream contract per handle: set_weights and the kernels are enqueued on the
    caller's current stream; a call from another stream waits for the packing event (FusedMLP.sync), but two streams
    must not run kernels of ONE handle concurrently (they share its per-call scratch)."""
    import weakref

    w0 = weights[0]
    key = id(w0)
    hit = _DEFAULT_MLP.get(key)
    if hit is None or hit[0]() is not w0:
        def _drop(ref, key=key):
            cur = _DEFAULT_MLP.get(key)
            if cur is not None and cur[0] is ref:
                del _DEFAULT_MLP[key]

        while len(_DEFAULT_MLP) >= _MAX_HANDLES:
            _DEFAULT_MLP.pop(next(iter(_DEFAULT_MLP)))
        hit = _DEFAULT_MLP[key] = (weakref.ref(w0, _drop), FusedMLP(w0.device))
    return hit[1].sync(weights)


def invalidate_weight_cache():
    """Needed only after writing MLP parameters through `.data` / a raw pointer."""
    for _, m in _DEFAULT_MLP.values():
        m.invalidate()


def mlp_forward(feats_fm, dirs, weights, samples_per_ray, mode="fp32"):
    """Fused MFMA forward of mlp_base + density head + mlp_head + rgb head (addition to the
    reference surface; the reference runs these through nerfstudio/PyTorch, model.py:602-621).
    feats_fm f32 [64, n] feature-major (interpolate_values(...).moveaxis(-1, 0) is that buffer),
    dirs f32 [n // samples_per_ray, 3], weights: 12 contiguous fp32 CUDA tensors in nn.Linear layout
    (w1,b1,w2,b2,w3,b3,wd,bd,wh,bh,wr,br).  mode: "fp32" (exact fp32 MFMA chain), "bf16x3" (bf16 MFMA on 3-way
    split operands; opt-in) or "bf16" (one bf16 MFMA per product, fp32 accumulation; opt-in, NOT at the 1e-5 parity bar of the
    other two: render.mlp_forward_bf16_statement states it).  Returns sigma [n], rgb [n,3].
    dirs=None: density only (mlp_base + density head; the entry's rgb == NULL) -> sigma [n].  The field itself, [64, V] as stored,
    is such a buffer: its columns are the features AT the vertices."""
    _check_input(feats_fm, "feats")
    _check(feats_fm.dtype == torch.float32 and feats_fm.dim() == 2 and feats_fm.size(0) == 64, "feats must be f32 [64, n]")
    n = feats_fm.size(1)
    S = int(samples_per_ray)
    _check(S > 0 and n % S == 0, "n must be a multiple of samples_per_ray")
    if dirs is not None:
        _check_input(dirs, "dirs")
        _check(dirs.dtype == torch.float32 and tuple(dirs.shape) == (n // S, 3), "dirs must be f32 [n/samples_per_ray, 3]")
    m = fused_mlp(weights)
    dev = feats_fm.device
    sigma = _empty((n,), dtype=torch.float32, device=dev)
    rgb = None if dirs is None else _empty((n, 3), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().tn_mlp_forward(m.handle, n, S, _ptr(feats_fm), _ptr(dirs), _mode(mode), _ptr(sigma), _ptr(rgb),
                                              _stream(dev)))
    return sigma if dirs is None else (sigma, rgb)


def _ray_bias(ray_head_bias, rays, dev):
    """f32 [rays, 128] per-ray bias of the head layer (appearance embedding: include/tetranerf_hip.h) or None"""
    if ray_head_bias is None:
        return None
    _check_input(ray_head_bias, "ray_head_bias")
    _check(ray_head_bias.dtype == torch.float32 and tuple(ray_head_bias.shape) == (rays, 128) and ray_head_bias.device == dev,
           "ray_head_bias must be f32 [rays, 128] on the field's device")
    return ray_head_bias


def _check_gather_args(field, dirs, samples=None, rays=None):
    """Argument checks of the calls that gather from `field`.  The gathering forwards pass samples = (vertex_indices,
    barycentric_coordinates, samples_per_ray) and get (n, S) back; dirs f32 [n / S, 3], or None: density only.  render_rays
    passes rays = R instead: its `directions` cover ALL rays (and it has checked the tensors themselves)."""
    if samples is None:
        _check(dirs.dtype == torch.float32 and tuple(dirs.shape) == (rays, 3), "directions must be f32 [R, 3]")
        _check(field.dtype == torch.float32 and field.dim() == 2 and field.size(0) == 64, "field must be f32 [64, V]")
        return None
    vertex_indices, barycentric_coordinates, samples_per_ray = samples
    for x, name in ((vertex_indices, "vertex_indices"), (barycentric_coordinates, "barycentric_coordinates"),
                    (field, "field")) + (() if dirs is None else ((dirs, "dirs"),)):
        _check_input(x, name)
    _check(vertex_indices.dtype == torch.int32 and vertex_indices.size(-1) == 4, "vertex_indices must be i32 [...,4]")
    _check(barycentric_coordinates.dtype == torch.float32 and barycentric_coordinates.size(-1) == 3,
           "barycentric_coordinates must be f32 [...,3]")
    _check(field.dtype == torch.float32 and field.dim() == 2 and field.size(0) == 64, "field must be f32 [64, V]")
    n = vertex_indices.numel() // 4
    S = int(samples_per_ray)
    _check(S > 0 and n % S == 0, "n must be a multiple of samples_per_ray")
    _check(dirs is None or (dirs.dtype == torch.float32 and tuple(dirs.shape) == (n // S, 3)),
           "dirs must be f32 [n/samples_per_ray, 3]")
    return n, S


def _given_or_fresh(t, name, shape, dev, wording):
    """The f32 output tensor of `shape` a caller handed in to be stored into, checked (`wording`: the caller's own), or a fresh
    unwritten one."""
    if t is None:
        return _empty(shape, dtype=torch.float32, device=dev)
    _check_input(t, name)
    _check(t.dtype == torch.float32 and t.numel() == math.prod(shape) and t.device == dev, wording)
    return t


def _forward_gather(listed, live, live_count, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray, mode,
                    ray_head_bias, count, sigma, rgb):
    """mlp_forward_gather (listed=False: tn_mlp_forward_gather, fresh outputs) and mlp_forward_gather_indexed (listed=True:
    tn_mlp_forward_gather_indexed over live / live_count, outputs given or fresh)."""
    density_only = dirs is None
    n, S = _check_gather_args(field, dirs, samples=(vertex_indices, barycentric_coordinates, samples_per_ray))
    dev = field.device
    if listed:
        _check(_MODES.get(mode) != 2, 'mlp_forward_gather_indexed: mlp mode must be "fp32" or "bf16x3": the plain-bf16 kernel has no '
                                      'indexed form')
        for x, name in ((live, "live"), (live_count, "live_count")):
            _check_input(x, name)
            _check(x.dtype == torch.int32 and x.device == dev, f"{name} must be an int32 tensor on the field's device")
        _check(live.numel() >= n and live_count.numel() >= 1, "live must hold n entries, live_count one")
        _check_count(count, S, n, "mlp_forward_gather_indexed")
    m = fused_mlp(weights)
    field_vm = field_vertex_major(field)
    sigma = _given_or_fresh(sigma, "sigma", (n,), dev, "sigma must be f32 [n]")
    rgb = None if density_only else _given_or_fresh(rgb, "rgb", (n, 3), dev, "rgb must be f32 [n, 3]")
    lib = _lib.load()
    with _on(dev):
        args = (_ptr(vertex_indices), _ptr(barycentric_coordinates), _ptr(field_vm), _ptr(dirs), _mode(mode), _ptr(sigma), _ptr(rgb),
                _ptr(None if density_only else _ray_bias(ray_head_bias, n // S, dev)), _ptr(count), _stream(dev))
        if listed:
            _lib.check(lib.tn_mlp_forward_gather_indexed(m.handle, n, S, _ptr(live), _ptr(live_count), *args))
        else:
            _lib.check(lib.tn_mlp_forward_gather(m.handle, n, S, *args))
    return sigma if density_only else (sigma, rgb)


def mlp_forward_gather(vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray, mode="fp32",
                       ray_head_bias=None, count=None):
    """interpolate_values + mlp_forward in ONE kernel: the wave gathers its samples' features from the
    (vertex-major shadow of the) field straight into MFMA operand registers; the [64, n] feature buffer is never
    written.  vertex_indices i32 [..., 4], barycentric_coordinates f32 [..., 3], field f32 [64, V].
    dirs=None: density only (the coarse pass of the model, model.py:577-581) -> sigma [n]."""
    return _forward_gather(False, None, None, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray, mode,
                           ray_head_bias, count, None, None)


# ---- per-tetrahedron occupancy field (the reference registers `tetrahedra_occupancy`, model.py:98-99,256-265, and never uses it)

def _check_cells(cells, name="cells"):
    _check_input(cells, name)
    _check(cells.dtype == torch.int32, f"{name} must be an int32 tensor (find_visited_cells' cell_indices; -1 = unmatched)")


def _check_occupancy(occupancy, dev):
    _check_input(occupancy, "occupancy")
    _check(occupancy.dtype == torch.float32 and occupancy.dim() == 1 and occupancy.device == dev,
           "occupancy must be f32 [num_cells] on the samples' device")


def _check_count(count, samples_per_ray, n, what):
    if count is None:
        return
    _check(count.dtype == torch.int32 and count.numel() >= 1 and count.is_cuda, "count must be an i32 device tensor")
    _check(samples_per_ray is not None and int(samples_per_ray) > 0 and n % int(samples_per_ray) == 0,
           f"{what}: `count` counts rays: it needs samples_per_ray, a divisor of the number of samples")


def occupancy_update(occupancy, cells, sigma, decay, samples_per_ray=None, count=None):
    """IN PLACE update of the per-tetrahedron occupancy field (tn_occupancy_update; statement: render.occupancy_update_statement):
        occupancy[t] = max(decay * occupancy[t], max{ sigma[i] : cells[i] == t })
    occupancy f32 [T]; cells i32 [...] = the matched tetrahedron of every sample (find_visited_cells' "cell_indices", -1 =
    unmatched); sigma f32, as many values.  Unmatched samples, ids >= T and sigmas that are not >= 0 contribute nothing; every
    tetrahedron decays.  count (i32 [1] on the device, with samples_per_ray): only the samples of the first count[0] rays are
    read.  Caller's stream, no host synchronisation; bit-identical from run to run.  Returns `occupancy`."""
    _check_cells(cells)
    _check_input(sigma, "sigma")
    dev = cells.device
    _check_occupancy(occupancy, dev)
    _check(sigma.dtype == torch.float32 and sigma.numel() == cells.numel() and sigma.device == dev,
           "sigma must be f32 with one value per entry of cells")
    n = cells.numel()
    if samples_per_ray is None and count is not None and cells.dim() >= 2:
        samples_per_ray = cells.size(-1)
    _check_count(count, samples_per_ray, n, "occupancy_update")
    with _on(dev):
        _lib.check(_lib.load().tn_occupancy_update(occupancy.numel(), n, _ptr(cells), _ptr(sigma), float(decay), _ptr(occupancy),
                                                   int(samples_per_ray or 0), _ptr(count), _stream(dev)))
    return occupancy


# ---- per-tetrahedron training statistics (no reference counterpart: the reference never changes its mesh)

TET_STATS_MAX_SAMPLES = 8192   # samples per ray tn_tet_stats_accumulate supports (a row's weights live in the wave's LDS)


def tet_stats_new(num_cells, device):
    """Zeroed statistics i64 [num_cells, 3] for tet_stats_accumulate: per tetrahedron (hits, sum of weights, sum of weight x
    ray value), the last two in fixed point with 32 fractional bits (render.tet_stats_scores turns them into floats)."""
    return torch.zeros((int(num_cells), 3), dtype=torch.int64, device=device)


def tet_stats_accumulate(stats, cells, sigma, edges, ray_value=None, ray_index=None, count=None):
    """IN PLACE accumulation of per-tetrahedron training statistics (tn_tet_stats_accumulate; statement:
    render.tet_stats_statement, byte for byte).  stats i64 [T, 3]; cells i32 [rows, S] = the matched tetrahedron of every sample
    (find_visited_cells' "cell_indices", -1 = unmatched); sigma f32 [rows, S] and edges f32 [rows, S + 1] = what the composite
    of these rows takes -- the kernel forms the composite's own weights w from them and adds, for every sample with a cell < T,
        stats[cell] += (1, rint(w^ * 2^32), rint(fl32(w^ * v^) * 2^32)),   w^ = clamp(w, 0, 1), v^ = clamp(v, 0, 256), NaN -> 0
    with v = ray_value[ray_index[row]] (ray_value f32 [rays], None: 1; ray_index i32 [rows], None: the row itself; its entries
    must be valid indices of ray_value).  count (i32 [1] on the device): only the first count[0] rows are read -- the padded
    rows of compact_hits(want_padded=True) repeat a real ray and must not be counted.  Integer sums: independent of any order,
    identical from run to run.  Caller's stream, no host synchronisation.  Returns `stats`."""
    _check_cells(cells)
    dev = cells.device
    _check_input(stats, "stats")
    _check(stats.dtype == torch.int64 and stats.dim() == 2 and stats.size(1) == 3 and stats.device == dev,
           "stats must be i64 [num_cells, 3] on the samples' device (tet_stats_new)")
    _check(stats.size(0) < 2 ** 32, "stats: too many tetrahedra")
    _check(cells.dim() == 2, "cells must be i32 [rows, samples_per_ray]")
    rows, S = cells.shape
    for x, name, shape in ((sigma, "sigma", (rows, S)), (edges, "edges", (rows, S + 1))):
        _check_input(x, name)
        _check(x.dtype == torch.float32 and tuple(x.shape) == shape and x.device == dev,
               f"{name} must be f32 {list(shape)} on the samples' device")
    if ray_value is not None:
        _check_input(ray_value, "ray_value")
        _check(ray_value.dtype == torch.float32 and ray_value.dim() == 1 and ray_value.device == dev,
               "ray_value must be f32 [rays] on the samples' device")
        _check(ray_index is not None or ray_value.numel() >= rows, "ray_value must hold one value per row (or pass ray_index)")
    if ray_index is not None:
        _check_input(ray_index, "ray_index")
        _check(ray_index.dtype == torch.int32 and ray_index.numel() == rows and ray_index.device == dev,
               "ray_index must be i32 [rows] on the samples' device")
        _check(ray_value is not None, "ray_index names entries of ray_value: pass ray_value")
    if count is not None:
        _check(count.dtype == torch.int32 and count.numel() >= 1 and count.device == dev, "count must be an i32 tensor on the samples' device")
    with _on(dev):
        _lib.check(_lib.load().tn_tet_stats_accumulate(stats.size(0), rows, S, _ptr(cells), _ptr(sigma), _ptr(edges), _ptr(ray_value),
                                                       _ptr(ray_index), _ptr(count), _ptr(stats), _stream(dev)))
    return stats


def remap_tet_values(old_cells, new_cells, values, num_vertices, return_star_max=False):
    """Per-tetrahedron values (>= 0: the occupancy field) carried from `old_cells` to `new_cells` over the same vertices, without
    point location (tn_remap_tet_values; statement: geometry.remap_tet_values_statement):
        star_max[v] = max{ values[t] : old_cells[t] names v },  new[t'] = max of star_max over the four vertices of new_cells[t'].
    Conservative -- a new tetrahedron is at least as live as every old one around each of its vertices -- at the price of a
    dilation by one ring, which the next occupancy_update decays.  old_cells i32 [T, 4], values f32 [T], new_cells i32 [T', 4] on one
    device.  NaN and negative values are not checked: the kernels take the maximum of the BIT PATTERNS as unsigned integers.
    Caller's stream, no host synchronisation.  Returns f32 [T'] (with return_star_max: also star_max f32 [num_vertices])."""
    for c, name in ((old_cells, "old_cells"), (new_cells, "new_cells")):
        _check_input(c, name)
        _check(c.dtype == torch.int32 and c.dim() == 2 and c.size(1) == 4, f"{name} must be int32 [num_cells, 4]")
    _check_input(values, "values")
    dev = values.device
    _check(values.dtype == torch.float32 and values.dim() == 1 and values.numel() == old_cells.size(0),
           "values must be f32 with one value per row of old_cells")
    _check(old_cells.device == dev and new_cells.device == dev, "old_cells, new_cells and values must be on the same device")
    V = int(num_vertices)
    _check(V >= 0, "num_vertices must not be negative")
    with torch.no_grad():
        out = _empty((new_cells.size(0),), dtype=torch.float32, device=dev)
        star = _empty((V,), dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.check(_lib.load().tn_remap_tet_values(V, old_cells.size(0), _ptr(old_cells), _ptr(values), new_cells.size(0),
                                                       _ptr(new_cells), _ptr(out), _ptr(star), _stream(dev)))
    return (out, star) if return_star_max else out


def isosurface(xyz, cells, values, level, tet_mask=None):
    """Marching tetrahedra on the mesh itself (no reference counterpart; tn_isosurface_count + tn_isosurface_emit; statement:
    geometry.isosurface_statement, bit for bit; the rule: DESIGN.md section 4.17): the level set { values = level } of the
    piecewise-linear interpolant of a per-vertex scalar, welded, consistently oriented -- (q1-q0) x (q2-q0) points towards
    values < level -- and in a deterministic order.  xyz f32 [V, 3], cells i32 [T, 4] (any tetrahedron soup; a row with an id
    outside [0, V) is skipped), values f32 [V], tet_mask uint8 / bool [T] or None (0 = skip the tetrahedron), all on one device;
    level: finite, below 2^126 in magnitude.  A tetrahedron with a non-finite value is skipped; a value equal to `level` counts as
    inside, and the zero-area triangles that makes are kept.
    Returns {"positions": f32 [N, 3], "triangles": i32 [M, 3] (rows of positions), "triangle_tets": i32 [M] (the source
    tetrahedron), "edge_vertices": i32 [N, 2] = the mesh edge (a, b), a < b, each vertex lies on, "edge_t": f32 [N] with
    positions = xyz[a] + edge_t (xyz[b] - xyz[a]), "num_triangles": M, "num_refs": the edge references before welding,
    "tri_offsets" / "ref_offsets": i32 [T + 1], the triangles / edge references in front of every tetrahedron: the triangles of
    tetrahedron t are rows tri_offsets[t] .. tri_offsets[t + 1]}.
    BLOCKS on two small read-backs: the two totals between the entries (they size the outputs), and the welded vertex count."""
    for x, name in ((xyz, "xyz"), (cells, "cells"), (values, "values")):
        _check_input(x, name)
    dev = values.device
    _check(values.dtype == torch.float32 and values.dim() == 1, "values must be f32 [V]")
    V = values.numel()
    _check(xyz.dtype == torch.float32 and tuple(xyz.shape) == (V, 3) and xyz.device == dev, "xyz must be f32 [V, 3] on the device of values")
    _check(cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4 and cells.device == dev,
           "cells must be int32 [num_cells, 4] on the device of values")
    T = cells.size(0)
    if tet_mask is not None:
        _check_input(tet_mask, "tet_mask")
        _check(tet_mask.dtype in (torch.uint8, torch.bool) and tet_mask.numel() == T and tet_mask.device == dev,
               "tet_mask must be uint8 or bool [num_cells] on the device of values")
    lib, level = _lib.load(), float(level)
    with torch.no_grad(), _on(dev):
        offsets = _empty((2, T + 1), dtype=torch.int32, device=dev)
        _lib.check(lib.tn_isosurface_count(V, T, _ptr(cells), _ptr(values), level, _ptr(tet_mask), _ptr(offsets[0]), _ptr(offsets[1]),
                                           _stream(dev)))
        num_triangles, num_refs = offsets[:, T].tolist()                       # read-back 1
        triangles = _empty((num_triangles, 3), dtype=torch.int32, device=dev)
        triangle_tets = _empty((num_triangles,), dtype=torch.int32, device=dev)
        edge_vertices = _empty((num_refs, 2), dtype=torch.int32, device=dev)
        edge_t = _empty((num_refs,), dtype=torch.float32, device=dev)
        positions = _empty((num_refs, 3), dtype=torch.float32, device=dev)
        count = _empty((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.tn_isosurface_emit(V, T, _ptr(xyz), _ptr(cells), _ptr(values), level, _ptr(tet_mask), _ptr(offsets[0]),
                                          _ptr(offsets[1]), num_triangles, num_refs, _ptr(triangles), _ptr(triangle_tets),
                                          _ptr(edge_vertices), _ptr(edge_t), _ptr(positions), _ptr(count), _stream(dev)))
        N = int(count.item())                                                  # read-back 2
    return {"positions": positions[:N], "triangles": triangles, "triangle_tets": triangle_tets, "edge_vertices": edge_vertices[:N],
            "edge_t": edge_t[:N], "num_triangles": num_triangles, "num_refs": num_refs, "tri_offsets": offsets[0],
            "ref_offsets": offsets[1]}


ISOSURFACE_REFINE_MAX_ROUNDS = 8     # tn_isosurface_core.h: REFINE_MAX_ROUNDS (8^-8 = one ulp of t = 1)
ISOSURFACE_REFINE_CANDIDATES = 7     # tn_isosurface_core.h: REFINE_CANDIDATES


def isosurface_refine_with(surface, xyz, values, level, density_fn, rounds):
    """The refinement of `isosurface`'s vertices with the densities of a CALLBACK (no reference counterpart; the four
    tn_isosurface_refine_* entries; statement: geometry.isosurface_refine_statement, bit for bit on the same densities; the rule:
    DESIGN.md section 4.17).  surface: isosurface's dict; xyz f32 [V, 3], values f32 [V] as passed to it; rounds in 0..8.
    density_fn(vertex_indices i32 [7 N, 4], barycentric f32 [7 N, 3]) -> f32 [7 N] on the same device: the density at the 7
    candidates of every vertex -- the inputs are those of mlp_forward_gather, (a, b, a, a) and (t, 0, 0), vertex-major.  It is
    called once per round, on the caller's stream; nothing is read back here and the host never waits.
    Every welded vertex moves along its own mesh edge to the crossing of the density nearest a, bracketed to 8^-rounds of the edge;
    triangles, welding and order are untouched.  rounds = 0 never calls density_fn and returns isosurface's positions and edge_t
    bit for bit (in new arrays: the first and the last kernel still run).
    Returns a new dict: "positions" and "edge_t" replaced, "edge_bracket" f32 [N, 4] = (t_lo, t_hi, s_lo, s_hi) and "edge_frozen"
    u8 [N] (1: a density out of range froze the edge; 2: an id >= V) added; every other entry is the same object.  NOT covered: tetrahedra whose four vertex values lie on one side are never visited; the triangles are chords of
    the surface, so the enclosed volume can shrink; of several crossings on one edge the one nearest a is taken; zero-area
    triangles are kept."""
    rounds = int(rounds)
    _check(0 <= rounds <= ISOSURFACE_REFINE_MAX_ROUNDS, "isosurface_refine: rounds must be in 0..8")
    out = dict(surface)
    ev = surface["edge_vertices"]
    for x, name in ((xyz, "xyz"), (values, "values"), (ev, "edge_vertices")):
        _check_input(x, name)
    dev = values.device
    _check(values.dtype == torch.float32 and values.dim() == 1, "values must be f32 [V]")
    V = values.numel()
    _check(xyz.dtype == torch.float32 and tuple(xyz.shape) == (V, 3) and xyz.device == dev, "xyz must be f32 [V, 3] on the device of values")
    _check(ev.dtype == torch.int32 and ev.dim() == 2 and ev.size(1) == 2 and ev.device == dev,
           "surface['edge_vertices'] must be int32 [N, 2] on the device of values")
    N, C = ev.size(0), ISOSURFACE_REFINE_CANDIDATES
    lib, level = _lib.load(), float(level)
    with torch.no_grad(), _on(dev):
        bracket = _empty((N, 4), dtype=torch.float32, device=dev)
        frozen = _empty((N,), dtype=torch.uint8, device=dev)
        vi = _empty((N * C, 4), dtype=torch.int32, device=dev)
        bc = _empty((N * C, 3), dtype=torch.float32, device=dev)
        edge_t = _empty((N,), dtype=torch.float32, device=dev)
        positions = _empty((N, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.tn_isosurface_refine_begin(V, N, _ptr(ev), _ptr(values), level, _ptr(bracket), _ptr(frozen), _stream(dev)))
        for r in range(rounds):
            _lib.check(lib.tn_isosurface_refine_points(V, N, r, _ptr(ev), _ptr(bracket), _ptr(frozen), _ptr(vi), _ptr(bc), _stream(dev)))
            s = density_fn(vi, bc) if N else _empty((0,), dtype=torch.float32, device=dev)
            _check(isinstance(s, torch.Tensor) and s.dtype == torch.float32 and s.numel() == N * C and s.device == dev and s.is_contiguous(),
                   "isosurface_refine: density_fn must return a contiguous f32 tensor with one value per candidate, on the same device")
            _lib.check(lib.tn_isosurface_refine_select(N, r, level, _ptr(s), _ptr(bracket), _ptr(frozen), _stream(dev)))
        _lib.check(lib.tn_isosurface_refine_vertices(V, N, _ptr(xyz), _ptr(ev), _ptr(bracket), level, _ptr(edge_t), _ptr(positions),
                                                     _stream(dev)))
    out.update(positions=positions, edge_t=edge_t, edge_bracket=bracket, edge_frozen=frozen)
    return out


def isosurface_refine(surface, xyz, values, level, field, weights, rounds, mode="fp32"):
    """isosurface_refine_with on the NETWORK's density: every round's 7 N candidates go through the density-only gathering
    forward (mlp_forward_gather(dirs=None), one sample per ray) on field f32 [64, V] and `weights` in `mode` ("fp32", "bf16x3",
    "bf16": whatever that forward accepts).  `values` should be that network's density at the vertices in the same mode
    (mlp_forward(field, None, weights, 1, mode)), as render.extract_mesh passes it.  The mesh `isosurface` gives is the level set of
    the linear interpolant of the vertex densities; this moves its vertices onto the level set of the network along their edges.
    What it returns, and what it does not cover: isosurface_refine_with."""
    def density(vi, bc):
        return mlp_forward_gather(vi, bc, field, None, weights, 1, mode=mode)

    if int(rounds) > 0:
        _check_input(field, "field")
        _check(field.dtype == torch.float32 and field.dim() == 2 and field.size(0) == 64 and field.size(1) == values.numel(),
               "field must be f32 [64, V], one column per entry of values")
    return isosurface_refine_with(surface, xyz, values, level, density, rounds)


def split_tetrahedra(xyz, cells, select):
    """Split the selected tetrahedra 1 -> 4 at their centroids (no reference counterpart: the reference's mesh is its input point
    cloud for the whole run; tn_split_count + tn_split_emit; statement: geometry.split_tetrahedra_statement, bit for bit; the
    rule: DESIGN.md section 4.18).  xyz f32 [V, 3], cells i32 [T, 4] (any tetrahedron soup), select uint8 / bool [T] (non-zero =
    asked), all on one device.  A tetrahedron is ACCEPTED iff it is asked, its ids are in [0, V), its stored row is not flat
    (orientation 0, also for NaN) and each of its four children -- the row with one slot replaced by the fp32 centroid
    ((p0 + p1) + (p2 + p3)) * 0.25f -- has the parent's orientation.  The four outer faces stay: the mesh stays conforming.
    Returns {"vertices": f32 [V + K, 3] (the old rows, then the centroids), "cells": i32 [T + 3K, 4] (child 0 in the parent's row,
    children 1..3 appended, three rows per accepted tetrahedron in ascending order), "cell_parent": i32 [T + 3K] (the row itself
    below T, the parent for an appended row: values[cell_parent] carries a per-tetrahedron array), "vertex_parents": i32 [K, 4]
    (the parent's row as stored: split_vertex_rows carries a per-vertex array), "counters": i32 [4] on the device -- asked,
    accepted, refused for a flat or inverted parent or child, refused for an id outside [0, V) --, "num_new": K}.
    BLOCKS on one small read-back: K between the two entries (it sizes the outputs).  With K == 0 the second entry is not called:
    "vertices" and "cells" are the inputs themselves."""
    for x, name in ((xyz, "xyz"), (cells, "cells"), (select, "select")):
        _check_input(x, name)
    dev = xyz.device
    _check(xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.size(1) == 3, "xyz must be f32 [V, 3]")
    _check(cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4 and cells.device == dev,
           "cells must be int32 [num_cells, 4] on the device of xyz")
    V, T = xyz.size(0), cells.size(0)
    _check(select.dtype in (torch.uint8, torch.bool) and select.numel() == T and select.device == dev,
           "select must be uint8 or bool [num_cells] on the device of xyz")
    lib = _lib.load()
    with torch.no_grad(), _on(dev):
        offsets = _empty((T + 1,), dtype=torch.int32, device=dev)
        counters = _empty((4,), dtype=torch.int32, device=dev)
        _lib.check(lib.tn_split_count(V, T, _ptr(xyz), _ptr(cells), _ptr(select), _ptr(offsets), _ptr(counters), _stream(dev)))
        K = int(offsets[T].item())                                             # the read-back
        if K == 0:
            return {"vertices": xyz, "cells": cells, "cell_parent": torch.arange(T, dtype=torch.int32, device=dev),
                    "vertex_parents": _empty((0, 4), dtype=torch.int32, device=dev), "counters": counters, "num_new": 0}
        vertices = _empty((V + K, 3), dtype=torch.float32, device=dev)
        new_cells = _empty((T + 3 * K, 4), dtype=torch.int32, device=dev)
        cell_parent = _empty((T + 3 * K,), dtype=torch.int32, device=dev)
        vertex_parents = _empty((K, 4), dtype=torch.int32, device=dev)
        _lib.check(lib.tn_split_emit(V, T, _ptr(xyz), _ptr(cells), _ptr(offsets), K, _ptr(vertices), _ptr(new_cells), _ptr(cell_parent),
                                     _ptr(vertex_parents), _stream(dev)))
    return {"vertices": vertices, "cells": new_cells, "cell_parent": cell_parent, "vertex_parents": vertex_parents,
            "counters": counters, "num_new": K}


SPLIT_NEW_MODES = {"mean": 0, "zero": 1}     # tn_split_core.h: MODE_MEAN, MODE_ZERO


def split_vertex_rows(values, vertex_parents, new="mean", values_vm=None, want_vertex_major=False):
    """A per-vertex array grown by the vertices of a split (tn_split_vertex_rows; statement: geometry.split_vertex_rows_statement,
    bit for bit).  values f32 [rows, V] (the [64, V] field, a moment of its optimiser), vertex_parents i32 [K, 4]
    (split_tetrahedra's) -> f32 [rows, V + K]: the old columns, then per new vertex ((x[a] + x[b]) + (x[c] + x[d])) * 0.25f of its
    four parents' columns (new="mean": the centroid's own form, so the piecewise-linear field stays the function it was, up to
    rounding) or 0 (new="zero").  values_vm f32 [V, rows] (optional): the caller's vertex-major shadow of `values`
    (field_vertex_major); the parent columns are then read from it as whole rows.  want_vertex_major: also return the shadow
    f32 [V + K, rows] of the result, written in the same pass and bit-equal to its transposition: (out, out_vm).
    Caller's stream, no host synchronisation."""
    _check(new in SPLIT_NEW_MODES, 'split_vertex_rows: new must be "mean" or "zero"')
    for x, name in ((values, "values"), (vertex_parents, "vertex_parents")):
        _check_input(x, name)
    dev = values.device
    _check(values.dtype == torch.float32 and values.dim() == 2 and values.size(0) > 0, "values must be f32 [rows, V] with rows > 0")
    _check(vertex_parents.dtype == torch.int32 and vertex_parents.dim() == 2 and vertex_parents.size(1) == 4 and vertex_parents.device == dev,
           "vertex_parents must be int32 [K, 4] on the device of values")
    rows, V, K = values.size(0), values.size(1), vertex_parents.size(0)
    if values_vm is not None:
        _check_input(values_vm, "values_vm")
        _check(values_vm.dtype == torch.float32 and tuple(values_vm.shape) == (V, rows) and values_vm.device == dev,
               "values_vm must be f32 [V, rows] on the device of values")
    with torch.no_grad(), _on(dev):
        out = _empty((rows, V + K), dtype=torch.float32, device=dev)
        out_vm = _empty((V + K, rows), dtype=torch.float32, device=dev) if want_vertex_major else None
        _lib.check(_lib.load().tn_split_vertex_rows(rows, V, K, _ptr(values), _ptr(values_vm), _ptr(vertex_parents), SPLIT_NEW_MODES[new],
                                                    _ptr(out), _ptr(out_vm), _stream(dev)))
    return (out, out_vm) if want_vertex_major else out


def _edge_split_buffers(T, dev):
    """the outputs of the edge split's count entries"""
    return {"tet_offsets": _empty((T + 1,), dtype=torch.int32, device=dev), "tet_edge": _empty((T,), dtype=torch.int32, device=dev),
            "bisected": _empty((T,), dtype=torch.uint8, device=dev), "edge_vertices": _empty((T, 2), dtype=torch.int32, device=dev),
            "counters": _empty((10,), dtype=torch.int32, device=dev)}


EDGE_SPLIT_MAX_CELLS = 1 << 30               # tn_edge_split_core.h: MAX_CELLS


def _edge_split_emit(xyz, cells, count):
    """The read-back of the counters and tn_edge_split_emit: split_edges' dict (the inputs themselves where nothing is accepted)"""
    V, T, dev = xyz.size(0), cells.size(0), xyz.device
    counters = count["counters"]
    host = counters.tolist()                                                   # the read-back
    Kv, Kt = int(host[8]), int(host[9])
    _check(T + Kt < EDGE_SPLIT_MAX_CELLS and V + Kv < 0xFFFFFFFF,
           "split_edges: num_cells + bisected rows must be below 2^30 and num_vertices + num_new below 2^32 - 1")
    out = {"counters": counters, "bisected": count["bisected"], "tet_edge": count["tet_edge"], "tet_offsets": count["tet_offsets"],
           "edge_vertices": count["edge_vertices"][:Kv], "num_new": Kv, "num_rows": Kt, "num_cells": T + Kt}
    if Kv == 0:
        out.update(vertices=xyz, cells=cells, cell_parent=torch.arange(T, dtype=torch.int32, device=dev),
                   vertex_parents=_empty((0, 4), dtype=torch.int32, device=dev))
        return out
    vertices = _empty((V + Kv, 3), dtype=torch.float32, device=dev)
    new_cells = _empty((T + Kt, 4), dtype=torch.int32, device=dev)
    cell_parent = _empty((T + Kt,), dtype=torch.int32, device=dev)
    vertex_parents = _empty((Kv, 4), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tn_edge_split_emit(V, T, _ptr(xyz), _ptr(cells), _ptr(count["tet_offsets"]), _ptr(count["tet_edge"]),
                                              _ptr(count["edge_vertices"]), Kv, Kt, _ptr(vertices), _ptr(new_cells), _ptr(cell_parent),
                                              _ptr(vertex_parents), _stream(dev)))
    out.update(vertices=vertices, cells=new_cells, cell_parent=cell_parent, vertex_parents=vertex_parents)
    return out


def split_edges(xyz, cells, select, faces, face_tets):
    """Bisect the best edge of every selected tetrahedron at its midpoint, together with every tetrahedron around it (no reference
    counterpart: the reference's mesh is its input point cloud for the whole run; tn_edge_split_count_tables + tn_edge_split_emit;
    statement: geometry.split_edges_statement, bit for bit; the rule: DESIGN.md section 4.22).  xyz f32 [V, 3], cells i32 [T, 4]
    (any tetrahedron soup), select uint8 / bool [T] (non-zero = asked), faces i32 [F, 3] and face_tets i32 [F, 2] (the cells' face
    table, -1 = no second tetrahedron: a hull face), all on one device.  An asked tetrahedron that is well-formed and not flat
    nominates its longest edge (ties: the smaller key lo << 32 | hi); a nominated edge is bisected unless a row around it has an id
    outside [0, V), it lies on a hull face, a row around it holds a longer nominated edge, or a row around it or one of that row's
    two children is flat.  The bisected edges share no tetrahedron: an independent set, not a maximal one -- call again for more.
    Returns {"vertices": f32 [V + K_v, 3] (the old rows, then the midpoints in ascending edge order), "cells": i32 [T + K_t, 4]
    (child 0 in the parent's row, child 1 appended, in ascending parent order), "cell_parent": i32 [T + K_t] (values[cell_parent]
    carries a per-tetrahedron array), "vertex_parents": i32 [K_v, 4] = (lo, hi, lo, hi) (split_vertex_rows carries a per-vertex
    array), "edge_vertices": i32 [K_v, 2], "bisected": uint8 [T] (carry your own selection as cat(select & ~bisected,
    zeros(K_t))), "tet_edge": i32 [T], "tet_offsets": i32 [T + 1], "counters": i32 [10] on the device
    (geometry.EDGE_SPLIT_COUNTER_NAMES), "num_new": K_v, "num_rows": K_t, "num_cells": T + K_t}.
    BLOCKS on one small read-back: the counters between the two entries (they size the outputs).  With K_v == 0 the second entry
    is not called: "vertices" and "cells" are the inputs themselves."""
    for x, name in ((xyz, "xyz"), (cells, "cells"), (select, "select"), (faces, "faces"), (face_tets, "face_tets")):
        _check_input(x, name)
    dev = xyz.device
    _check(xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.size(1) == 3, "xyz must be f32 [V, 3]")
    _check(cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4 and cells.device == dev,
           "cells must be int32 [num_cells, 4] on the device of xyz")
    V, T, F = xyz.size(0), cells.size(0), faces.size(0)
    _check(select.dtype in (torch.uint8, torch.bool) and select.numel() == T and select.device == dev,
           "select must be uint8 or bool [num_cells] on the device of xyz")
    _check(faces.dtype == torch.int32 and faces.dim() == 2 and faces.size(1) == 3 and faces.device == dev,
           "faces must be int32 [num_faces, 3] on the device of xyz")
    _check(face_tets.dtype == torch.int32 and tuple(face_tets.shape) == (F, 2) and face_tets.device == dev,
           "face_tets must be int32 [num_faces, 2] on the device of xyz")
    with torch.no_grad(), _on(dev):
        count = _edge_split_buffers(T, dev)
        _lib.check(_lib.load().tn_edge_split_count_tables(dev.index or 0, V, T, _ptr(xyz), _ptr(cells), _ptr(select), F, _ptr(faces),
                                                          _ptr(face_tets), _ptr(count["tet_offsets"]), _ptr(count["tet_edge"]),
                                                          _ptr(count["bisected"]), _ptr(count["edge_vertices"]), _ptr(count["counters"]),
                                                          _stream(dev)))
        return _edge_split_emit(xyz, cells, count)


def _flip_buffers(T, F, dev):
    """the outputs of the flip's count entries"""
    return {"tet_offsets": _empty((T + 1,), dtype=torch.int32, device=dev), "tet_flip": _empty((T,), dtype=torch.int32, device=dev),
            "flipped": _empty((T,), dtype=torch.uint8, device=dev), "face_flip": _empty((F, 3), dtype=torch.int32, device=dev),
            "counters": _empty((10,), dtype=torch.int32, device=dev)}


FLIP_MAX_CELLS = 1 << 30                     # tn_flip_core.h: MAX_CELLS


def _flip_emit(cells, count, emit):
    """The read-back of the counters and the emit entry `emit(K23, K32, cells_out, cell_sources)`: flip_faces' dict (the input
    cells themselves where nothing is accepted)"""
    T, dev = cells.size(0), cells.device
    host = count["counters"].tolist()                                          # the read-back
    K23, K32 = int(host[8]), int(host[9])
    _check(T + K23 < FLIP_MAX_CELLS, "flip_faces: num_cells + accepted 2-3 flips must be below 2^30")
    out = {"counters": count["counters"], "flipped": count["flipped"], "tet_flip": count["tet_flip"], "tet_offsets": count["tet_offsets"],
           "face_flip": count["face_flip"], "num_23": K23, "num_32": K32, "num_cells": T + K23 - K32}
    if K23 + K32 == 0:
        src = torch.full((T, 3), -1, dtype=torch.int32, device=dev)
        src[:, 0] = torch.arange(T, dtype=torch.int32, device=dev)
        out.update(cells=cells, cell_sources=src)
        return out
    new_cells = _empty((T + K23 - K32, 4), dtype=torch.int32, device=dev)
    sources = _empty((T + K23 - K32, 3), dtype=torch.int32, device=dev)
    emit(K23, K32, new_cells, sources)
    out.update(cells=new_cells, cell_sources=sources)
    return out


def flip_faces(xyz, cells, faces, face_tets):
    """ONE round of the Delaunay repair by bistellar flips (no reference counterpart; tn_flip_count_tables + tn_flip_emit;
    statement: geometry.flip_faces_statement, bit for bit; the rule: DESIGN.md section 4.23).  xyz f32 [V, 3], cells i32 [T, 4],
    faces i32 [F, 3] and face_tets i32 [F, 2] (the cells' face table, -1 = no second tetrahedron: a hull face), all on one device.
    Every interior face that is CERTAINLY violated (delaunay_check's verdict) is a candidate: for a 2-3 flip where the edge
    between the two opposite vertices crosses the face, for a 3-2 flip where it passes one edge of the face and a third
    tetrahedron closes the ring around that edge.  A candidate is refused for an id outside [0, V), for opposite vertices that are
    not certainly on opposite sides, for an uncertain orientation around the new edge, for an unflippable configuration, or
    because a tetrahedron it needs goes to a candidate with a smaller face id.  The accepted flips share no tetrahedron: an
    independent set, not a maximal one -- call again for more.  No vertex is added or moved.
    Returns {"cells": i32 [T', 4], "cell_sources": i32 [T', 3] (the old rows whose union holds the new row, -1 = none:
    flip_tet_values carries a per-tetrahedron array), "flipped": uint8 [T], "tet_flip": i32 [T], "tet_offsets": i32 [T + 1],
    "face_flip": i32 [F, 3] = (code, t2, rank), "counters": i32 [10] on the device (geometry.FLIP_COUNTER_NAMES), "num_23",
    "num_32", "num_cells": T' = T + num_23 - num_32}.
    BLOCKS on one small read-back: the counters between the two entries (they size the outputs).  With nothing accepted the
    second entry is not called: "cells" is the input itself."""
    for x, name in ((xyz, "xyz"), (cells, "cells"), (faces, "faces"), (face_tets, "face_tets")):
        _check_input(x, name)
    dev = xyz.device
    _check(xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.size(1) == 3, "xyz must be f32 [V, 3]")
    _check(cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4 and cells.device == dev,
           "cells must be int32 [num_cells, 4] on the device of xyz")
    V, T, F = xyz.size(0), cells.size(0), faces.size(0)
    _check(faces.dtype == torch.int32 and faces.dim() == 2 and faces.size(1) == 3 and faces.device == dev,
           "faces must be int32 [num_faces, 3] on the device of xyz")
    _check(face_tets.dtype == torch.int32 and tuple(face_tets.shape) == (F, 2) and face_tets.device == dev,
           "face_tets must be int32 [num_faces, 2] on the device of xyz")
    lib = _lib.load()
    with torch.no_grad(), _on(dev):
        count = _flip_buffers(T, F, dev)
        _lib.check(lib.tn_flip_count_tables(dev.index or 0, V, T, _ptr(xyz), _ptr(cells), F, _ptr(faces), _ptr(face_tets),
                                            _ptr(count["tet_offsets"]), _ptr(count["tet_flip"]), _ptr(count["flipped"]),
                                            _ptr(count["face_flip"]), _ptr(count["counters"]), _stream(dev)))

        def emit(K23, K32, new_cells, sources):
            _lib.check(lib.tn_flip_emit(T, _ptr(cells), F, _ptr(faces), _ptr(face_tets), _ptr(count["tet_offsets"]), _ptr(count["tet_flip"]),
                                        _ptr(count["face_flip"]), K23, K32, _ptr(new_cells), _ptr(sources), _stream(dev)))
        return _flip_emit(cells, count, emit)


def flip_tet_values(values, cell_sources):
    """Carry a per-tetrahedron array through a round of flips: values f32 [T] (>= 0: the occupancy), cell_sources i32 [T', 3]
    (flip_faces; -1 = none) -> f32 [T']: per new row the largest value over its sources, by remap_tet_values' rule (the values'
    bit patterns as unsigned integers; geometry.flip_tet_values_statement).  A new row lies inside the union of its sources, so
    this is conservative in space, not only over vertex stars.  Plain torch; no synchronisation."""
    _check(values.dtype == torch.float32 and values.dim() == 1, "values must be float32 [T]")
    _check(cell_sources.dim() == 2 and cell_sources.size(1) == 3 and cell_sources.device == values.device,
           "cell_sources must be [T', 3] on the device of values")
    with torch.no_grad():
        bits = values.contiguous().view(torch.int32).long() & 0xFFFFFFFF
        s = cell_sources.long()
        if bits.numel() == 0:
            return torch.zeros(s.size(0), dtype=torch.float32, device=values.device)
        got = torch.where(s >= 0, bits[s.clamp_min(0)], torch.zeros_like(s)).amax(1)
        return torch.where(got >= (1 << 31), got - (1 << 32), got).to(torch.int32).view(torch.float32)


def compose_cell_sources(sources, step):
    """sources int64 [T, S] (-1-padded input rows of every current row; None: every row is its own source), step i32 [T', 3]
    (flip_faces' cell_sources of one round) -> int64 [T', S'] the input rows of every new row: the union over its sources,
    ascending, without repeats, padded with -1 and trimmed to the longest (geometry.compose_cell_sources).  One read-back."""
    s = step.long()
    if sources is None:
        sources = torch.arange(int(s.max().item()) + 1 if s.numel() else 0, dtype=torch.int64, device=s.device)[:, None]
    big = 1 << 32
    src = torch.where(sources < 0, torch.full_like(sources, big), sources)
    got = torch.where((s >= 0)[:, :, None], src[s.clamp_min(0)], torch.full((1, 1, 1), big, dtype=torch.int64, device=s.device))
    got = got.reshape(s.size(0), -1).sort(1).values
    got[:, 1:][got[:, 1:] == got[:, :-1]] = big
    got = got.sort(1).values
    width = max(int((got != big).sum(1).max().item()) if got.numel() else 1, 1)
    got = got[:, :width]
    return torch.where(got == big, torch.full_like(got, -1), got)


FACE_TABLE_MAX_CELLS = 1 << 30               # tn_face_table_count: num_cells must be below 2^30
FACE_TABLE_FLAG_CELL_OOB, FACE_TABLE_FLAG_TRIPLE_FACE = 1, 2   # tn_build_core.h: FLAG_CELL_OOB, FLAG_TRIPLE_FACE (geometry.py has them too)


def _check_cell_rows(cells):
    _check_input(cells, "cells")
    _check(cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4, "cells must be int32 [num_cells, 4]")
    _check(cells.size(0) < FACE_TABLE_MAX_CELLS, "face_table: num_cells must be below 2^30")


def _face_table_count(cells, V):
    """tn_face_table_count on checked cells: (partner i32 [4T], face_index i32 [4T + 1], counters i32 [4]); no synchronisation"""
    T, dev = cells.size(0), cells.device
    partner = _empty((4 * T,), dtype=torch.int32, device=dev)
    face_index = _empty((4 * T + 1,), dtype=torch.int32, device=dev)
    counters = _empty((4,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tn_face_table_count(dev.index or 0, V, T, _ptr(cells), _ptr(partner), _ptr(face_index), _ptr(counters),
                                               _stream(dev)))
    return partner, face_index, counters


def _face_table_emit(cells, partner, face_index, F, tet_faces=True, exact=True):
    """tn_face_table_emit for the host value F: (faces i32 [F, 3], face_tets i32 [F, 2], tet_faces i32 [T, 4] or None).  exact: F
    is the count's own total, read back; otherwise face_tets starts as -1, so that rows a smaller total leaves out are hull faces
    (which no mesh operation reads further), never unwritten memory."""
    T, dev = cells.size(0), cells.device
    faces = _empty((F, 3), dtype=torch.int32, device=dev)
    face_tets = _empty((F, 2), dtype=torch.int32, device=dev) if exact else torch.full((F, 2), -1, dtype=torch.int32, device=dev)
    tf = _empty((T, 4), dtype=torch.int32, device=dev) if tet_faces else None
    _lib.check(_lib.load().tn_face_table_emit(T, _ptr(cells), _ptr(partner), _ptr(face_index), F, _ptr(faces), _ptr(face_tets), _ptr(tf),
                                              _stream(dev)))
    return faces, face_tets, tf


def _check_face_table_counters(host, num_faces=None):
    """the build's own errors for the flag bits of a read-back [F, hull faces, flags, 0]; num_faces: the F the caller emitted with"""
    _check(not host[2] & FACE_TABLE_FLAG_CELL_OOB, "cells contains a vertex index that is out of bounds")
    _check(not host[2] & FACE_TABLE_FLAG_TRIPLE_FACE, "A triangle is shared by more than two tetrahedra!")
    _check(num_faces is None or host[0] == num_faces,
           f"internal: the face table has {host[0]} faces where the flips of the last round leave {num_faces}")


def face_table(cells, num_vertices=None):
    """The face table of any cell rows on the device, without a tracer (tn_face_table_count + tn_face_table_emit: the face-table
    stage of load_tetrahedra's device build as an entry of its own; statement: geometry.face_table_statement, byte for byte; the
    rule: DESIGN.md section 4.24).  cells i32 [T, 4]; num_vertices: None, or V -- then an id outside [0, V) raises the load's own
    error.  Returns {"faces": i32 [F, 3] (in order of first sighting 4 t + local face, ids as the first sighting's row orders
    them), "face_tets": i32 [F, 2] (-1 = no second tetrahedron: a hull face), "tet_faces": i32 [T, 4] (the face of every local
    face), "counters": i32 [4] on the device (geometry.FACE_TABLE_COUNTER_NAMES), "num_faces": F, "num_hull_faces"}: what
    flip_faces, split_edges and prune_vertices take as `faces` / `face_tets`, and what TetrahedraTracer.face_tables() reports after
    a load of the same cells.  Raises "A triangle is shared by more than two tetrahedra!" like the load.
    BLOCKS on one small read-back: the counters between the two entries (they size the outputs)."""
    _check_cell_rows(cells)
    dev = cells.device
    with torch.no_grad(), _on(dev):
        # without V no id is out of bounds: every uint32 id is below 2^32
        partner, face_index, counters = _face_table_count(cells, 1 << 32 if num_vertices is None else int(num_vertices))
        host = [h & 0xFFFFFFFF for h in counters.tolist()]                      # the read-back
        _check_face_table_counters(host)
        faces, face_tets, tet_faces = _face_table_emit(cells, partner, face_index, host[0])
    return {"faces": faces, "face_tets": face_tets, "tet_faces": tet_faces, "counters": counters, "num_faces": host[0],
            "num_hull_faces": host[1]}


def _flip_count_tables(xyz, cells, faces, face_tets):
    """tn_flip_count_tables on checked arrays -> (the count buffers, flip_faces' emit closure); no synchronisation"""
    lib, dev = _lib.load(), xyz.device
    V, T, F = xyz.size(0), cells.size(0), faces.size(0)
    count = _flip_buffers(T, F, dev)
    _lib.check(lib.tn_flip_count_tables(dev.index or 0, V, T, _ptr(xyz), _ptr(cells), F, _ptr(faces), _ptr(face_tets),
                                        _ptr(count["tet_offsets"]), _ptr(count["tet_flip"]), _ptr(count["flipped"]),
                                        _ptr(count["face_flip"]), _ptr(count["counters"]), _stream(dev)))

    def emit(K23, K32, new_cells, sources):
        _lib.check(lib.tn_flip_emit(T, _ptr(cells), F, _ptr(faces), _ptr(face_tets), _ptr(count["tet_offsets"]), _ptr(count["tet_flip"]),
                                    _ptr(count["face_flip"]), K23, K32, _ptr(new_cells), _ptr(sources), _stream(dev)))
    return count, emit


def _flip_rounds(xyz, cells, F, count, emit, tet_values, max_rounds):
    """The loop of flip_to_delaunay on face tables built by tn_face_table_count / tn_face_table_emit.
    (count, emit): the first round's count buffers on `cells` and its emit closure (_flip_emit's), F the face count of that round's
    table.  After a round's read-back K23 and K32 are host values, so the next table's F' = F + 2 K23 - 2 K32 is known without
    another one (a 2-3 flip removes one face and adds three, a 3-2 flip removes three and adds one): the next round's table is
    emitted with F', its flips are counted on it, and its counters (F, flag bits) come back in the SAME read-back as that round's
    flip counters, before anything is emitted from that table.  Two small read-backs per round, like the loop that reloads: this
    one, and the width of the composed sources.  Returns TetrahedraTracer.flip_to_delaunay's dict."""
    dev, V = xyz.device, xyz.size(0)
    tet_values = list(tet_values)
    sources, rounds, table_counters = torch.arange(cells.size(0), dtype=torch.int64, device=dev)[:, None], [], None
    while True:
        if table_counters is None:
            host = count["counters"].tolist()                                   # the read-back
        else:
            host = torch.cat((count["counters"], table_counters)).tolist()      # the read-back, with the table's counters
            _check_face_table_counters([h & 0xFFFFFFFF for h in host[10:]], F)
        rounds.append(host[:10])
        K23, K32 = int(host[8]), int(host[9])
        if K23 + K32 == 0 or len(rounds) > int(max_rounds):                     # nothing accepted, or the round that is not run
            break
        T = cells.size(0)
        _check(T + K23 < FLIP_MAX_CELLS, "flip_faces: num_cells + accepted 2-3 flips must be below 2^30")
        new_cells = _empty((T + K23 - K32, 4), dtype=torch.int32, device=dev)
        step = _empty((T + K23 - K32, 3), dtype=torch.int32, device=dev)
        emit(K23, K32, new_cells, step)
        cells, F = new_cells, F + 2 * K23 - 2 * K32
        tet_values = [flip_tet_values(t.detach(), step) for t in tet_values]
        sources = compose_cell_sources(sources, step)
        partner, face_index, table_counters = _face_table_count(cells, V)
        faces, face_tets, _ = _face_table_emit(cells, partner, face_index, F, tet_faces=False, exact=False)
        count, emit = _flip_count_tables(xyz, cells, faces, face_tets)
    return {"cells": cells, "tet_values": tet_values, "cell_sources": sources, "rounds": rounds, "violated": rounds[-1][1],
            "unflippable": rounds[-1][6], "num_rounds": len(rounds) - 1, "num_tetrahedra": cells.size(0)}


def flip_to_delaunay(xyz, cells, tet_values=(), max_rounds=32):
    """TetrahedraTracer.flip_to_delaunay without a tracer: repair the Delaunay property of `cells` on `xyz` by rounds of bistellar
    flips (flip_faces' rule), every round's face table built on the device by face_table's two entries
    (section 4.24) -- nothing is loaded.  xyz f32 [V, 3], cells i32 [T, 4] on its device (a mesh without inverted tetrahedra,
    ids in [0, V)), tet_values: float32 [T] arrays of values >= 0, carried by flip_tet_values.  Returns the tracer method's dict
    ("cells" is the input itself where nothing flips); its rounds, counters, cell_sources and carried values are the same.
    BLOCKS once on the first table's counters, then per round on two small read-backs: the flip's counters with the next table's,
    and the width of the composed sources."""
    _check_input(xyz, "xyz")
    _check(xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.size(1) == 3, "xyz must be f32 [V, 3]")
    _check_cell_rows(cells)
    _check(cells.device == xyz.device, "cells must be on the device of xyz")
    tet_values = tuple(tet_values)
    for t in tet_values:
        _check_input(t, "tet_values")
        _check(t.dtype == torch.float32 and t.dim() == 1 and t.size(0) == cells.size(0) and t.device == xyz.device,
               "tet_values must be float32 [T] arrays over the cells, on the device of xyz")
    with torch.no_grad(), _on(xyz.device):
        table = face_table(cells, xyz.size(0))
        count, emit = _flip_count_tables(xyz, cells, table["faces"], table["face_tets"])
        return _flip_rounds(xyz, cells, table["num_faces"], count, emit, tet_values, max_rounds)


def _check_prune_masks(dead, vertex_select, T, V, dev):
    _check_input(dead, "dead")
    _check(dead.dtype in (torch.uint8, torch.bool) and dead.numel() == T and dead.device == dev,
           "dead must be uint8 or bool [num_cells] on the device of the mesh")
    if vertex_select is not None:
        _check_input(vertex_select, "vertex_select")
        _check(vertex_select.dtype in (torch.uint8, torch.bool) and vertex_select.numel() == V and vertex_select.device == dev,
               "vertex_select must be uint8 or bool [num_vertices] on the device of the mesh")


def _prune_emit(xyz, offsets, counters):
    """The read-back of V' and tn_prune_emit: prune_vertices' dict (the inputs themselves where nothing is removed)"""
    V, dev = xyz.size(0), xyz.device
    Vp = int(offsets[V].item())                                                 # the read-back
    out = {"offsets": offsets, "counters": counters, "num_kept": Vp, "num_removed": V - Vp}
    if Vp == V:
        ids = torch.arange(V, dtype=torch.int32, device=dev)
        out.update(vertices=xyz, new_id=ids, kept_ids=ids)
        return out
    vertices = _empty((Vp, 3), dtype=torch.float32, device=dev)
    new_id = _empty((V,), dtype=torch.int32, device=dev)
    kept_ids = _empty((Vp,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tn_prune_emit(V, _ptr(xyz), _ptr(offsets), Vp, _ptr(new_id), _ptr(kept_ids), _ptr(vertices), _stream(dev)))
    out.update(vertices=vertices, new_id=new_id, kept_ids=kept_ids)
    return out


def prune_vertices(xyz, cells, dead, faces, face_tets, vertex_select=None):
    """Remove the vertices that only dead tetrahedra name and that lie on no hull face (no reference counterpart: the reference's
    mesh is its input point cloud for the whole run; tn_prune_count_tables + tn_prune_emit; statement:
    geometry.prune_vertices_statement, bit for bit; the rule: DESIGN.md section 4.21).  xyz f32 [V, 3], cells i32 [T, 4] (any
    tetrahedron soup), dead uint8 / bool [T] (non-zero = dead), faces i32 [F, 3] and face_tets i32 [F, 2] (the cells' face table,
    -1 = no second tetrahedron: a hull face), vertex_select uint8 / bool [V] or None (only these vertices are asked), all on one
    device.  An asked vertex is kept because a tetrahedron that is not dead (or that has an id outside [0, V)) names it, else
    because it is on a hull face, else because no tetrahedron names it; otherwise it is removed.
    Returns {"vertices": f32 [V', 3] = xyz[kept_ids], "new_id": i32 [V] (-1 where removed), "kept_ids": i32 [V'] (ascending:
    prune_vertex_rows carries a per-vertex array), "offsets": i32 [V + 1], "counters": i32 [5] on the device -- asked, removed,
    kept live, kept hull, kept unreferenced --, "num_kept": V', "num_removed"}.  The cells of the kept points are the caller's
    (triangulate; TetrahedraTracer.remove_vertices).  BLOCKS on one small read-back: V' between the two entries (it sizes the
    outputs).  With nothing removed the second entry is not called: "vertices" is the input itself."""
    for x, name in ((xyz, "xyz"), (cells, "cells"), (faces, "faces"), (face_tets, "face_tets")):
        _check_input(x, name)
    dev = xyz.device
    _check(xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.size(1) == 3, "xyz must be f32 [V, 3]")
    _check(cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4 and cells.device == dev,
           "cells must be int32 [num_cells, 4] on the device of xyz")
    _check(faces.dtype == torch.int32 and faces.dim() == 2 and faces.size(1) == 3 and faces.device == dev,
           "faces must be int32 [num_faces, 3] on the device of xyz")
    _check(face_tets.dtype == torch.int32 and tuple(face_tets.shape) == (faces.size(0), 2) and face_tets.device == dev,
           "face_tets must be int32 [num_faces, 2] on the device of xyz")
    V, T, F = xyz.size(0), cells.size(0), faces.size(0)
    _check_prune_masks(dead, vertex_select, T, V, dev)
    with torch.no_grad(), _on(dev):
        offsets = _empty((V + 1,), dtype=torch.int32, device=dev)
        counters = _empty((5,), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().tn_prune_count_tables(dev.index or 0, V, T, _ptr(cells), F, _ptr(faces), _ptr(face_tets), _ptr(dead),
                                                     _ptr(vertex_select), _ptr(offsets), _ptr(counters), _stream(dev)))
        return _prune_emit(xyz, offsets, counters)


def prune_vertex_rows(values, kept_ids, values_vm=None, want_vertex_major=False):
    """A per-vertex array compacted to the kept vertices of a prune (tn_prune_vertex_rows; statement:
    geometry.prune_vertex_rows_statement, bit for bit).  values f32 [rows, V] (the [64, V] field, a moment of its optimiser),
    kept_ids i32 [V'] (prune_vertices') -> f32 [rows, V'] = values[:, kept_ids].  values_vm f32 [V, rows] (optional): the caller's
    vertex-major shadow of `values` (field_vertex_major); the kept columns are then read from it as whole rows.
    want_vertex_major: also return the shadow f32 [V', rows] of the result, written in the same pass and bit-equal to its
    transposition: (out, out_vm).  Caller's stream, no host synchronisation."""
    for x, name in ((values, "values"), (kept_ids, "kept_ids")):
        _check_input(x, name)
    dev = values.device
    _check(values.dtype == torch.float32 and values.dim() == 2 and values.size(0) > 0, "values must be f32 [rows, V] with rows > 0")
    _check(kept_ids.dtype == torch.int32 and kept_ids.dim() == 1 and kept_ids.device == dev, "kept_ids must be int32 [V'] on the device of values")
    rows, V, Vp = values.size(0), values.size(1), kept_ids.size(0)
    _check(Vp <= V, "kept_ids must not be longer than the rows of values")
    if values_vm is not None:
        _check_input(values_vm, "values_vm")
        _check(values_vm.dtype == torch.float32 and tuple(values_vm.shape) == (V, rows) and values_vm.device == dev,
               "values_vm must be f32 [V, rows] on the device of values")
    with torch.no_grad(), _on(dev):
        out = _empty((rows, Vp), dtype=torch.float32, device=dev)
        out_vm = _empty((Vp, rows), dtype=torch.float32, device=dev) if want_vertex_major else None
        _lib.check(_lib.load().tn_prune_vertex_rows(rows, V, Vp, _ptr(values), _ptr(values_vm), _ptr(kept_ids), _ptr(out), _ptr(out_vm),
                                                    _stream(dev)))
    return (out, out_vm) if want_vertex_major else out


_CULL_SCRATCH = {}   # device -> i32 scratch of cull_samples (tile counts), allocated once and grown on demand


def cull_samples(cells, occupancy, threshold, sigma, rgb=None, samples_per_ray=None, count=None):
    """The samples the network still has to run on (tn_cull_samples; statement: render.cull_mask_statement): a sample is culled iff
    its cell is a valid id < T and occupancy[cell] < threshold; unmatched samples and a NaN occupancy stay live, threshold <= 0
    culls nothing.  Writes sigma = 0 (and rgb = 0 when given) at the culled samples, leaves the live positions untouched, and returns
    (live i32 [n], live_count i32 [1] on the device): live[:live_count] = the indices of the live samples, ascending
    (= torch.nonzero of the live mask); the rest of `live` is unwritten.  count (i32 [1] device tensor, with samples_per_ray --
    default: the last dimension of a 2-D `cells`): samples from count[0] * samples_per_ray on are neither listed nor touched.
    Caller's stream, no host synchronisation."""
    _check_cells(cells)
    _check_input(sigma, "sigma")
    dev = cells.device
    _check_occupancy(occupancy, dev)
    n = cells.numel()
    _check(n < 0xFFFFFFFF, "too many samples for one call")
    _check(sigma.dtype == torch.float32 and sigma.numel() == n and sigma.device == dev, "sigma must be f32 with one value per entry of cells")
    if rgb is not None:
        _check_input(rgb, "rgb")
        _check(rgb.dtype == torch.float32 and rgb.numel() == 3 * n and rgb.device == dev, "rgb must be f32 [n, 3]")
    if samples_per_ray is None:
        samples_per_ray = cells.size(-1) if cells.dim() >= 2 else 1
    _check_count(count, samples_per_ray, n, "cull_samples")
    live = _empty((n,), dtype=torch.int32, device=dev)
    live_count = _empty((1,), dtype=torch.int32, device=dev)
    need = (n + 1023) // 1024 + 1
    scratch = _CULL_SCRATCH.get(dev)
    if scratch is None or scratch.numel() < need:
        scratch = _CULL_SCRATCH[dev] = torch.empty((max(need + need // 4, 1024),), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().tn_cull_samples(n, int(samples_per_ray), _ptr(cells), _ptr(occupancy), occupancy.numel(), float(threshold),
                                               _ptr(live), _ptr(live_count), _ptr(sigma), _ptr(rgb), _ptr(scratch), scratch.numel(),
                                               _ptr(count), _stream(dev)))
    return live, live_count


def mlp_forward_gather_indexed(live, live_count, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray,
                               mode="fp32", ray_head_bias=None, count=None, sigma=None, rgb=None):
    """mlp_forward_gather over the listed samples only (tn_mlp_forward_gather_indexed): slot i < live_count[0] computes sample
    live[i] -- gathers there, takes the head term of that sample's ray, stores sigma / rgb there.  live i32 [n], live_count i32 [1]
    on the device (cull_samples); all other arguments as mlp_forward_gather over all n samples.  sigma f32 [n] / rgb f32 [n, 3]: the
    tensors to store into (what cull_samples zeroed at the culled samples); positions that are not listed are NOT written --
    without them fresh (unwritten) tensors are returned.  For every listed sample the result is bit for bit mlp_forward_gather's
    in the same mode; mode "fp32" or "bf16x3" ("bf16" has no indexed kernel).  dirs=None: density only -> sigma."""
    return _forward_gather(True, live, live_count, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray, mode,
                           ray_head_bias, count, sigma, rgb)


class _RgbBackground(C.Structure):   # tn_rgb_background
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("clamp", C.c_int)]


def _background(background, clamp=False):
    """tn_rgb_background from a grey level (float) or an (r, g, b) triple (sequence or HOST tensor; a device tensor would
    force a sync here) + the RGB renderer's evaluation-mode flag."""
    if isinstance(background, torch.Tensor):
        background = background.detach().reshape(-1).tolist()
    if isinstance(background, (int, float)):
        background = (background,) * 3
    r, g, b = (float(x) for x in background)
    return C.byref(_RgbBackground(r, g, b, 1 if clamp else 0))


def render_rays(trace_lists, order, count, field, directions, weights, num_samples, num_fine=0, biased=False, out=None,
                background=1.0, clamp=True, ray_head_bias=None, histogram_padding=0.01, eps=1e-5, mode="fp32"):
    """Everything between trace_rays and the frame as ONE persistent launch (tn_render_rays_ex; mode "fp32" | "bf16x3"): coarse sampler -> match -> gather
    + MLP -> weights -> PDF sampler -> match -> gather + MLP + heads -> composite, for the hitting rays order[:count] (compact_hits)
    whose number stays on the device.  trace_lists as returned by trace_rays; directions f32 [R,3] and ray_head_bias f32 [R,128]
    over ALL rays; out = (rgb [R,3], accumulation [R,1] or [R], depth) pre-filled with the background values."""
    mode = _mode(mode, inference=False)     # (the persistent kernel has no "bf16" phases: TetraRenderer.render takes the chain)
    nv, _cells, bary, dist, verts = trace_lists
    for x, name in ((nv, "num_visited_cells"), (bary, "barycentric_coordinates"), (dist, "hit_distances"), (verts, "vertex_indices"),
                    (order, "order"), (field, "field"), (directions, "directions")):
        _check_input(x, name)
    R, M = dist.size(0), dist.size(1)
    _check(order.dtype == torch.int32 and order.dim() == 1 and order.numel() <= R, "order must be i32 [<= R]")
    _check(count is None or (count.dtype == torch.int32 and count.numel() >= 1 and count.is_cuda), "count must be an i32 device tensor")
    _check_gather_args(field, directions, rays=R)
    S, Sf = int(num_samples), int(num_fine)
    m = fused_mlp(weights)
    dev = field.device
    field_vm = field_vertex_major(field)
    rgb, acc, depth = out
    for x, name in ((rgb, "rgb"), (acc, "accumulation"), (depth, "depth")):
        _check_input(x, name)
        _check(x.dtype == torch.float32 and x.size(0) == R, f"{name} must be f32 over all rays")
    hb = None
    if ray_head_bias is not None:
        hb = _ray_bias(ray_head_bias, R, dev)
    with _on(dev):
        _lib.check(_lib.load().tn_render_rays_ex(
            m.handle, M, _ptr(nv), _ptr(dist), _ptr(bary), _ptr(verts), _ptr(order), _ptr(count), order.numel(), S, Sf, 1 if biased else 0,
            _ptr(_linspace_table(S, dev)), _ptr(_quantile_table(Sf + 1, True, dev)) if Sf else None, float(histogram_padding), float(eps),
            _ptr(field_vm), _ptr(directions), _background(background, clamp), _ptr(rgb), _ptr(acc), _ptr(depth), _ptr(hb), mode, _stream(dev)))


_TABLES = {}    # (kind, n, device) -> small constant tables of the samplers (the values the PyTorch statements use)


def _linspace_table(S, device):
    key = ("lin", S, device)
    if key not in _TABLES:
        _TABLES[key] = torch.linspace(0.0, 1.0, S + 1, dtype=torch.float32, device=device)
    return _TABLES[key]


def _quantile_table(num_bins, centred, device):
    key = ("q", num_bins, centred, device)
    if key not in _TABLES:
        u = torch.linspace(0.0, 1.0 - (1.0 / num_bins), steps=num_bins, dtype=torch.float32, device=device)
        _TABLES[key] = (u + 1.0 / (2 * num_bins)).contiguous() if centred else u
    return _TABLES[key]


def compact_hits(num_visited_cells, want_padded=False):
    """Stable partition of the rays of a trace call by num_visited_cells > 0, on the device (tn_compact_hits; replaces
    torch.nonzero / boolean indexing: no host synchronisation).  Returns (order i32 [R], count i32 [1] on the device[,
    padded i32 [R]]): order[:count] = the hitting rays in ray order, order[count:] = the others; padded = order with the tail
    replaced by order[0]."""
    _check_input(num_visited_cells, "num_visited_cells")
    _check(num_visited_cells.dtype == torch.int32 and num_visited_cells.dim() == 1, "num_visited_cells must be i32 [R]")
    R, dev = num_visited_cells.numel(), num_visited_cells.device
    order = _empty((R,), dtype=torch.int32, device=dev)
    count = _empty((1,), dtype=torch.int32, device=dev)
    padded = _empty((R,), dtype=torch.int32, device=dev) if want_padded else None
    n_scratch = 2 * ((R + 2047) // 2048)
    scratch = _empty((max(n_scratch, 1),), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().tn_compact_hits(R, _ptr(num_visited_cells), _ptr(order), _ptr(count), _ptr(padded), _ptr(scratch),
                                               scratch.numel(), _stream(dev)))
    return (order, count, padded) if want_padded else (order, count)


def sample_coarse(num_visited_cells, hit_distances, ray_index, num_samples, biased=False, t_rand=None, count=None):
    """Coarse sampler as ONE kernel on the trace rows in place (tn_sample_coarse; model.py:531-557, 111-192): returns
    (edges f32 [r, S+1] euclidean bin edges, near_far f32 [r, 2]) for the hitting rays ray_index i32 [r].  t_rand
    [r, S+1]: training-mode stratified bins; biased: the TetrahedraSampler mapping.  Same values as
    render.uniform_sample_bins / biased_sample_bins up to the rounding of one prefix sum."""
    for x, name in ((num_visited_cells, "num_visited_cells"), (hit_distances, "hit_distances"), (ray_index, "ray_index")):
        _check_input(x, name)
    _check(ray_index.dtype == torch.int32 and ray_index.dim() == 1, "ray_index must be i32 [r]")
    _check(hit_distances.dtype == torch.float32 and hit_distances.dim() == 3 and hit_distances.size(2) == 2, "hit_distances must be f32 [R,M,2]")
    r, S, M = ray_index.numel(), int(num_samples), hit_distances.size(1)
    dev = hit_distances.device
    if t_rand is not None:
        _check_input(t_rand, "t_rand")
        _check(t_rand.dtype == torch.float32 and tuple(t_rand.shape) == (r, S + 1), "t_rand must be f32 [r, S+1]")
    edges = _empty((r, S + 1), dtype=torch.float32, device=dev)
    near_far = _empty((r, 2), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().tn_sample_coarse(r, S, M, _ptr(ray_index), _ptr(num_visited_cells), _ptr(hit_distances),
                                                _ptr(_linspace_table(S, dev)), _ptr(t_rand), 1 if biased else 0, _ptr(edges),
                                                _ptr(near_far), _ptr(count), _stream(dev)))
    return edges, near_far


def _check_live_rows(num_visited_cells, visited_cells, hit_distances, ray_index, occupancy, what):
    """the trace rows + occupancy of sample_live / live_to_distance, checked -> (r, M, device)"""
    for x, name in ((num_visited_cells, "num_visited_cells"), (visited_cells, "visited_cells"), (hit_distances, "hit_distances"),
                    (ray_index, "ray_index")):
        _check_input(x, name)
    _check(ray_index.dtype == torch.int32 and ray_index.dim() == 1, "ray_index must be i32 [r]")
    _check(hit_distances.dtype == torch.float32 and hit_distances.dim() == 3 and hit_distances.size(2) == 2, "hit_distances must be f32 [R,M,2]")
    R, M = hit_distances.size(0), hit_distances.size(1)
    dev = hit_distances.device
    _check(num_visited_cells.dtype == torch.int32 and num_visited_cells.dim() == 1 and num_visited_cells.numel() == R
           and num_visited_cells.device == dev, "num_visited_cells must be i32 [R] on the rows' device")
    _check(visited_cells.dtype == torch.int32 and tuple(visited_cells.shape) == (R, M) and visited_cells.device == dev,
           "visited_cells must be i32 [R,M] on the rows' device")
    _check(ray_index.device == dev, "ray_index must be on the rows' device")
    _check(occupancy is not None, f"{what} needs the occupancy field its segments are compared with")
    _check_occupancy(occupancy, dev)
    return ray_index.numel(), M, dev


def _check_ray_count(count):
    _check(count is None or (count.dtype == torch.int32 and count.numel() >= 1 and count.is_cuda), "count must be an i32 device tensor")


def sample_live(num_visited_cells, visited_cells, hit_distances, ray_index, num_samples, occupancy, threshold, t_rand=None, count=None):
    """The occupancy-guided coarse sampler as ONE kernel on the trace rows in place (tn_sample_live; statements:
    render.live_lengths_statement + live_sample_bins): returns (s_edges f32 [r, S+1], near_far_live f32 [r, 2]) for the hitting
    rays ray_index i32 [r].  near_far_live = (near, near + L), L = the summed length of the ray's LIVE segments -- those whose
    cell cull_samples would not cull under (occupancy f32 [T], threshold); s_edges = the uniform sampler's bin edges over that span
    (t_rand [r, S+1]: training-mode stratified bins), in the live-length coordinate: map values of it with live_to_distance.  A ray
    without a live segment counts all its segments live; count (i32 [1] on the device): rows from count[0] on are unwritten."""
    r, M, dev = _check_live_rows(num_visited_cells, visited_cells, hit_distances, ray_index, occupancy, "sample_live")
    S = int(num_samples)
    _check(S >= 1, "num_samples must be positive")
    _check_ray_count(count)
    if t_rand is not None:
        _check_input(t_rand, "t_rand")
        _check(t_rand.dtype == torch.float32 and tuple(t_rand.shape) == (r, S + 1) and t_rand.device == dev, "t_rand must be f32 [r, S+1]")
    edges = _empty((r, S + 1), dtype=torch.float32, device=dev)
    near_far = _empty((r, 2), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().tn_sample_live(r, S, M, _ptr(ray_index), _ptr(num_visited_cells), _ptr(visited_cells), _ptr(hit_distances),
                                              _ptr(occupancy), occupancy.numel(), float(threshold), _ptr(_linspace_table(S, dev)),
                                              _ptr(t_rand), _ptr(edges), _ptr(near_far), _ptr(count), _stream(dev)))
    return edges, near_far


def live_to_distance(values, num_visited_cells, visited_cells, hit_distances, ray_index, occupancy, threshold, count=None, out=None):
    """The inverse map of the live-length coordinate as ONE kernel (tn_live_to_distance; statement:
    render.live_to_distance_statement): values f32 [r, n] (bin centres, edges, one depth per ray) of the rays ray_index i32 [r] ->
    (t f32 [r, n] distances, slot i32 [r, n] = the segment of the trace row each value landed in).  Every t lies inside a live
    segment of its ray: t_in[slot] <= t <= t_out[slot].  out = (t, slot) to store into; count (i32 [1] on the device): rows from
    count[0] on are unwritten."""
    r, M, dev = _check_live_rows(num_visited_cells, visited_cells, hit_distances, ray_index, occupancy, "live_to_distance")
    _check_input(values, "values")
    _check(values.dtype == torch.float32 and values.dim() == 2 and values.size(0) == r and values.device == dev, "values must be f32 [r, n]")
    n = values.size(1)
    _check_ray_count(count)
    if out is None:
        t, slot = _empty((r, n), dtype=torch.float32, device=dev), _empty((r, n), dtype=torch.int32, device=dev)
    else:
        t, slot = out
        for x, name, dt in ((t, "out t", torch.float32), (slot, "out slot", torch.int32)):
            _check_input(x, name)
            _check(x.dtype == dt and tuple(x.shape) == (r, n) and x.device == dev, f"{name} must be [r, n] of the right type")
    with _on(dev):
        _lib.check(_lib.load().tn_live_to_distance(r, n, M, _ptr(ray_index), _ptr(num_visited_cells), _ptr(visited_cells),
                                                   _ptr(hit_distances), _ptr(occupancy), occupancy.numel(), float(threshold), _ptr(values),
                                                   _ptr(t), _ptr(slot), _ptr(count), _stream(dev)))
    return t, slot


def sample_pdf(edges, weights, near_far, num_fine, u_rand=None, histogram_padding=0.01, eps=1e-5, count=None):
    """nerfstudio's PDFSampler (include_original) as ONE kernel (tn_sample_pdf; model.py:582-586): edges f32 [r, S+1]
    euclidean coarse edges, weights f32 [r, S], near_far f32 [r, 2] -> f32 [r, S + num_fine + 2] merged, sorted euclidean
    edges.  u_rand [r, num_fine+1]: training-mode stratified quantiles."""
    for x, name in ((edges, "edges"), (weights, "weights"), (near_far, "near_far")):
        _check_input(x, name)
        _check(x.dtype == torch.float32, f"{name} must have float32 type")
    r, S = weights.shape
    nb = int(num_fine) + 1
    _check(tuple(edges.shape) == (r, S + 1) and tuple(near_far.shape) == (r, 2), "shape mismatch")
    dev = edges.device
    if u_rand is not None:
        _check_input(u_rand, "u_rand")
        _check(u_rand.dtype == torch.float32 and tuple(u_rand.shape) == (r, nb), "u_rand must be f32 [r, num_fine+1]")
    out = _empty((r, S + 1 + nb), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().tn_sample_pdf(r, S, int(num_fine), _ptr(edges), _ptr(weights), _ptr(near_far),
                                             _ptr(_quantile_table(nb, u_rand is None, dev)), _ptr(u_rand), float(histogram_padding),
                                             float(eps), _ptr(out), _ptr(count), _stream(dev)))
    return out


def composite(sigma, rgb, edges, background=1.0, return_weights=False, clamp=False, out=None, ray_index=None, count=None):
    """RaySamples.get_weights + RGB (background blend) / accumulation / median-depth renderers
    (model.py:632-638) in one kernel.  sigma f32 [R,S], rgb f32 [R,S,3], edges f32 [R,S+1].
    rgb=None: only the weights [R,S] are computed and returned (get_weights of the coarse pass, model.py:582).
    out = (rgb [R_all,3], accumulation, depth over ALL rays of the trace call) + ray_index i32 [R]: row q is written at
    ray_index[q] (returns None); count i32 [1] on the device: only the first count[0] rows are processed (compact_hits)."""
    for x, name in ((sigma, "sigma"), (edges, "edges")) + (() if rgb is None else ((rgb, "rgb"),)):
        _check_input(x, name)
        _check(x.dtype == torch.float32, f"{name} must have float32 type")
    R, S = sigma.shape
    _check((rgb is None or tuple(rgb.shape) == (R, S, 3)) and tuple(edges.shape) == (R, S + 1), "shape mismatch")
    dev = sigma.device
    if rgb is None:
        weights = _empty((R, S), dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.check(_lib.load().tn_composite(R, S, _ptr(sigma), None, _ptr(edges), None, None, None, None,
                                                _ptr(weights), None, _ptr(count), _stream(dev)))
        return weights
    if out is not None:
        _check(ray_index is not None and ray_index.dtype == torch.int32 and ray_index.numel() == R, "out= needs ray_index i32 [R]")
        o_rgb, o_acc, o_depth = out
        for x, name in ((o_rgb, "rgb"), (o_acc, "accumulation"), (o_depth, "depth")):
            _check_input(x, name)
            _check(x.dtype == torch.float32, f"{name} must have float32 type")
        with _on(dev):
            _lib.check(_lib.load().tn_composite(R, S, _ptr(sigma), _ptr(rgb), _ptr(edges), _background(background, clamp), _ptr(o_rgb),
                                                _ptr(o_acc), _ptr(o_depth), None, _ptr(ray_index), _ptr(count), _stream(dev)))
        return None
    out_rgb = _empty((R, 3), dtype=torch.float32, device=dev)
    acc = _empty((R, 1), dtype=torch.float32, device=dev)
    depth = _empty((R, 1), dtype=torch.float32, device=dev)
    weights = _empty((R, S), dtype=torch.float32, device=dev) if return_weights else None
    with _on(dev):
        _lib.check(_lib.load().tn_composite(R, S, _ptr(sigma), _ptr(rgb), _ptr(edges), _background(background, clamp), _ptr(out_rgb),
                                            _ptr(acc), _ptr(depth), _ptr(weights), None, _ptr(count), _stream(dev)))
    return (out_rgb, acc, depth, weights) if return_weights else (out_rgb, acc, depth)


class _MlpBackwardBuffers(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("x0", "h1", "h2", "h3", "h4", "masks", "d1", "d2", "d3", "d4", "dhead", "dx0")]


def _backward_buffers(acts, masks, chain=None, dx0=None):
    """tn_mlp_backward_buffers of a training call: acts f32 [576, n] = x0 [64, n] on top of h1..h4 [128, n] each, masks i64
    [4, n, 2], chain f32 [516, n] = d1..d4 [128, n] on top of dhead [4, n], dx0 f32 [n, 64]; None (or without a column): null
    pointers."""
    def rows(t, firsts):
        if t is None or not t.numel():
            return (None,) * len(firsts)
        base, step = t.data_ptr(), t.stride(0) * t.element_size()
        return tuple(base + f * step for f in firsts)

    return _MlpBackwardBuffers(*rows(acts, (0, 64, 192, 320, 448)), _ptr(masks), *rows(chain, (0, 128, 256, 384, 512)), _ptr(dx0))


class MlpSaved:
    """What mlp_forward_gather_train leaves for mlp_backward: the layer inputs x0 [64,n], h1..h4 [128,n] (quad-major
    [F/4][n][4], opaque to the caller: the operands of the weight-gradient GEMMs) and the ReLU masks [4,n,2] (all the dX kernel needs).  (`sigma` / `rgb` are the
    forward's outputs as returned; an autograd node must hold them through save_for_backward, not through this object.)"""
    __slots__ = ("acts", "masks", "sigma", "rgb", "n", "S")


def _forward_gather_train(listed, live, n_live, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray,
                          ray_head_bias, mode, sigma, rgb):
    """mlp_forward_gather_train (listed=False: every sample has a column of the saves) and mlp_forward_gather_train_indexed
    (listed=True: the columns are the n_live listed samples): checks, handle, field shadow, outputs, saves and the call."""
    mode = _mode(mode, inference=False)
    _check_input(dirs, "dirs")   # (no density-only form: the training forward is the full network)
    n, S = _check_gather_args(field, dirs, samples=(vertex_indices, barycentric_coordinates, samples_per_ray))
    dev = field.device
    sv = MlpSavedIndexed() if listed else MlpSaved()
    sv.n, sv.S = n, S
    if listed:
        sv.n, sv.n_samples, sv.live = int(n_live), n, live
        _check_live_list(live, sv.n, dev)
    m = fused_mlp(weights)
    field_vm = field_vertex_major(field)
    sv.sigma = _given_or_fresh(sigma, "sigma", (n,), dev, f"sigma must be f32 with {n} elements")
    sv.rgb = _given_or_fresh(rgb, "rgb", (n, 3), dev, f"rgb must be f32 with {3 * n} elements")
    sv.acts = _empty((64 + 4 * 128, sv.n), dtype=torch.float32, device=dev)
    sv.masks = _empty((4, sv.n, 2), dtype=torch.int64, device=dev)
    lib = _lib.load()
    with _on(dev):
        args = (_ptr(vertex_indices), _ptr(barycentric_coordinates), _ptr(field_vm), _ptr(dirs.contiguous()), mode, _ptr(sv.sigma),
                _ptr(sv.rgb), C.byref(_backward_buffers(sv.acts, sv.masks)), _ptr(_ray_bias(ray_head_bias, n // S, dev)), _stream(dev))
        if listed:
            _lib.check(lib.tn_mlp_forward_gather_train_indexed(m.handle, sv.n, n, S, _ptr(live), *args))
        else:
            _lib.check(lib.tn_mlp_forward_gather_train_ex(m.handle, n, S, *args))
    return sv.sigma, sv.rgb, sv


def mlp_forward_gather_train(vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray, ray_head_bias=None,
                             mode="fp32"):
    """mlp_forward_gather for training: returns (sigma [n], rgb [n,3], saved) -- `saved` holds 2.3 KB per sample for
    mlp_backward, which then recomputes nothing.  mode: "fp32" (default) or "bf16x3" (tn_mlp_forward_gather_train_ex): sigma /
    rgb are then mlp_forward_gather(mode="bf16x3")'s bits and `saved` holds that forward's activations and ReLU masks in the
    same layouts; mlp_backward runs on them in either arithmetic of its own (adjoint_mode), chosen independently."""
    return _forward_gather_train(False, None, None, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray,
                                 ray_head_bias, mode, None, None)


class MlpSavedIndexed(MlpSaved):
    """What mlp_forward_gather_train_indexed leaves for mlp_backward: MlpSaved with COMPACT tensors -- n = n_live columns, column i
    belongs to sample live[i] of the n_samples samples of the call (S per ray)."""
    __slots__ = ("n_samples", "live")


def _check_live_list(live, n_live, dev):
    _check_input(live, "live")
    _check(live.dtype == torch.int32 and live.device == dev, "live must be an int32 tensor on the field's device")
    _check(0 <= n_live <= live.numel(), "n_live must be a host integer in [0, live.numel()]")


def compact_rows(src, live, n_live):
    """dst[i] = src[live[i]] for i < n_live (tn_compact_rows): src a contiguous 32-bit tensor [n] / [n, 3] / [n, 4] (any leading
    shape), live i32 ascending list of rows (cull_samples), n_live a host integer.  Returns [n_live] / [n_live, 3] / [n_live, 4].
    Every listed row must exist in src: the kernel has no bound to check against."""
    _check_input(src, "src")
    _check(src.element_size() == 4, "compact_rows: 32-bit elements")
    W = 1 if src.dim() <= 1 else src.size(-1)
    _check(W in (1, 3, 4), "compact_rows: rows of 1, 3 or 4 elements")
    n_live = int(n_live)
    _check_live_list(live, n_live, src.device)
    dst = _empty((n_live,) if src.dim() <= 1 else (n_live, W), dtype=src.dtype, device=src.device)
    with _on(src.device):
        _lib.check(_lib.load().tn_compact_rows(W, n_live, _ptr(live), _ptr(src), _ptr(dst), _stream(src.device)))
    return dst


def mlp_forward_gather_train_indexed(live, n_live, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray,
                                     ray_head_bias=None, mode="fp32", sigma=None, rgb=None):
    """mlp_forward_gather_train over the listed samples only (tn_mlp_forward_gather_train_indexed): slot i < n_live computes sample
    live[i] -- gathers there, takes the head term of that sample's ray, stores sigma / rgb there -- and saves at column i of
    COMPACT buffers (2.3 KB per LISTED sample).  live i32 (ascending: cull_samples), n_live a HOST integer (the caller has read
    cull_samples' live_count back); all other arguments as mlp_forward_gather_train over all n samples.  sigma f32 [n] / rgb f32
    [n, 3]: the tensors to store into (what cull_samples zeroed at the culled samples); positions that are not listed are NOT
    written -- without them fresh (unwritten) tensors are returned.  For every listed sample the outputs and the saved column
    are bit for bit mlp_forward_gather_train's in the same mode.  Returns (sigma, rgb, saved: MlpSavedIndexed) for mlp_backward.
    The forward itself tolerates a list entry >= n (it stores no output for it); mlp_backward does NOT: it compacts rows by the
    list without a bound (tn_compact_rows), so only a list whose every entry is a sample -- what cull_samples writes -- may go on
    to the backward."""
    return _forward_gather_train(True, live, n_live, vertex_indices, barycentric_coordinates, field, dirs, weights, samples_per_ray,
                                 ray_head_bias, mode, sigma, rgb)


class MlpChain:
    """What the dX chain of one mlp_backward call produced (return_chain=True; for tests that follow the chain layer by layer):
    d1..d4 [128, n] slices of quad-major memory ([F/4][n][4], like MlpSaved.acts), dhead [4, n] (d sigma_raw, d rgb_raw) and
    dx0 [n, 64]."""
    __slots__ = ("d1", "d2", "d3", "d4", "dhead", "dx0")


def mlp_backward(saved, vertex_indices, barycentric_coordinates, field, dirs, weights, sigma, rgb, d_sigma, d_rgb,
                 want_ray_head_grad=False, want_bary_grad=False, return_dx0=False, adjoint_mode="fp32", return_chain=False,
                 dw_mode="fp32"):
    """Adjoint of mlp_forward_gather_train (addition; the reference leaves this to PyTorch autograd, model.py:602-630):
    given the forward's outputs sigma [n] / rgb [n,3], dL/dsigma [n] and dL/drgb [n,3] returns (grad_field [64,V], [12 weight
    gradients in the order of `weights`]).
    tn_mlp_backward -- the dX chain on the fp32 matrix cores from the saved ReLU masks, nothing recomputed -- then
    tn_mlp_param_grads -- the twelve parameter gradients as sample-streaming fp32-MFMA GEMMs over the saved layer inputs,
    summed without atomics (bit-reproducible) -- then the gather's adjoint.  2.1 KB of gradient buffers per sample.
    Appended to the result, in this order: want_ray_head_grad: the per-ray sums of the head pre-activation's gradient [rays, 128];
    want_bary_grad: dL/d barycentric_coordinates [n, 3], the gather's adjoint w.r.t. the barycentrics on the same d x0 rows
    (tn_interpolate_values_backward_bary_vm; tet membership is a constant of it); return_dx0: those rows, d x0 [n, 64];
    return_chain: an MlpChain with views of everything the dX chain wrote.
    adjoint_mode: arithmetic of the dX chain (tn_mlp_backward_ex), independent of the forward's.  "fp32" (default; mode 0 is
    tn_mlp_backward).  "bf16x3" (mode 1): its four matrix products on the bf16 matrix cores, three bf16 pieces per operand; softplus' /
    sigmoid', the head layer's gradient d4, the density term and the masks stay fp32 (dhead and d4 are the default's bits), and
    so does the gather adjoint, which reads the same buffers.  "bf16" is not an adjoint arithmetic.
    dw_mode: arithmetic of the four weight-gradient GEMMs (tn_mlp_param_grads_ex), independent of the other two.  "fp32" (default;
    mode 0 is tn_mlp_param_grads).  "bf16x3" (mode 1): both streamed operands split into three bf16 pieces as they are staged, six
    products per multiply on the bf16 matrix cores, fp32 accumulation; the bias gradients, d wd and the rgb head stay fp32;
    still without atomics, bit-reproducible.  grad_field does not depend on it.  "bf16" is not a training arithmetic.
    saved an MlpSavedIndexed (mlp_forward_gather_train_indexed; occupancy-culled training): every argument still covers all
    n_samples samples of the call.  The rows of the listed samples are compacted (tn_compact_rows), the dX chain and the gather
    adjoints run unchanged on n_live columns, the parameter gradients and the per-ray sums through their indexed entries; the sums
    run over the listed samples only, grad_bary is [n_samples, 3] with zeros at the samples not listed, the per-ray sums cover all
    rays (zeros for a ray without a listed sample), dx0 and the MlpChain stay compact (slot i = sample live[i]).  Every entry
    of the list must be a sample < n_samples (cull_samples' lists are): tn_compact_rows reads src[live[i]] without a bound."""
    amode = _mode(adjoint_mode, inference=False)
    wmode = _mode(dw_mode, inference=False)
    mh = fused_mlp(weights)
    keep = [w.detach() for w in weights]
    n, S = saved.n, saved.S
    # an MlpSavedIndexed (mlp_forward_gather_train_indexed): all arguments cover the nfull samples of the call; the rows of the
    # n listed ones are compacted first, the per-sample kernels then run unchanged on n columns
    live = getattr(saved, "live", None)
    nfull = n if live is None else saved.n_samples
    _check(vertex_indices.numel() == 4 * nfull, "vertex_indices do not belong to the saved forward pass")
    _check(d_sigma.numel() == nfull and d_rgb.numel() == 3 * nfull, "d_sigma / d_rgb must have n / 3n elements")
    dev = field.device
    V = field.size(1)
    vi = vertex_indices.reshape(nfull, 4)
    bc = barycentric_coordinates.reshape(nfull, 3)
    d_sigma = d_sigma.reshape(nfull).contiguous().float()
    d_rgb = d_rgb.reshape(nfull, 3).contiguous().float()
    dirs = dirs.contiguous()
    if live is not None:
        vi, bc = compact_rows(vi.contiguous(), live, n), compact_rows(bc.contiguous(), live, n)
        sigma, rgb = compact_rows(sigma.reshape(nfull).contiguous(), live, n), compact_rows(rgb.reshape(nfull, 3).contiguous(), live, n)
        d_sigma, d_rgb = compact_rows(d_sigma, live, n), compact_rows(d_rgb, live, n)
    lib = _lib.load()
    # the twelve gradients as views of ONE zero-filled buffer (tn_mlp_param_grads accumulates): one fill launch, not twelve
    sizes = [w.numel() for w in keep]
    offs = [0]
    for k in sizes:
        offs.append(offs[-1] + (k + 3) // 4 * 4)       # 16-byte aligned pieces
    flat = torch.zeros((offs[-1],), dtype=torch.float32, device=dev)
    grads = [flat[o:o + k].view(tuple(w.shape)) for o, k, w in zip(offs, sizes, keep)]
    gs = _MlpWeightsStruct(*[g.data_ptr() for g in grads])
    grad_vm = torch.zeros((V, 64), dtype=torch.float32, device=dev)
    buf = _empty((4 * 128 + 4, n), dtype=torch.float32, device=dev)
    rows = _empty((n, 64), dtype=torch.float32, device=dev)     # d x0, sample-major
    bs = _backward_buffers(saved.acts, saved.masks, buf, rows)
    stream = _stream(dev)
    some = n > 0 or live is None      # (an empty list: nothing to launch, every sum is empty)
    with _on(dev):
        if some:
            _lib.check(lib.tn_mlp_backward_ex(mh.handle, n, _ptr(sigma.contiguous()), _ptr(rgb.contiguous()), _ptr(d_sigma), _ptr(d_rgb),
                                              C.byref(bs), amode, stream))
        if live is not None:
            _lib.check(lib.tn_mlp_param_grads_indexed(mh.handle, n, nfull, S, _ptr(live), _ptr(dirs), C.byref(bs), C.byref(gs), wmode,
                                                      stream))
        else:
            _lib.check(lib.tn_mlp_param_grads_ex(mh.handle, n, S, _ptr(dirs), C.byref(bs), C.byref(gs), wmode, stream))
        d_ray_bias = None
        if want_ray_head_grad:      # gradient of the per-ray head bias: per-ray sums of d4
            d_ray_bias = _empty((nfull // S, 128), dtype=torch.float32, device=dev)
            if live is not None:
                _lib.check(lib.tn_mlp_ray_head_grad_indexed(n, nfull, S, _ptr(live), C.byref(bs), _ptr(d_ray_bias), stream))
            else:
                _lib.check(lib.tn_mlp_ray_head_grad(n, S, C.byref(bs), _ptr(d_ray_bias), stream))
        # gradient of the gathered features -> field (vertex-major accumulation)
        if some:
            _gather_adjoint_vm(lib, 4, V, n, 64, vi, bc, rows, grad_vm, stream)
        grad_field = _empty((64, V), dtype=torch.float32, device=dev)
        _lib.check(lib.tn_transpose_f32(V, 64, _ptr(grad_vm), _ptr(grad_field), stream))
        grad_bary = None
        if want_bary_grad and some:
            grad_bary = _bary_adjoint_vm(lib, 4, n, 64, vi, rows, field_vertex_major(field), stream)
        if want_bary_grad and live is not None:      # rows of the listed samples -> [nfull, 3], zeros at the culled ones
            full = torch.zeros((nfull, 3), dtype=torch.float32, device=dev)
            grad_bary = full if n == 0 else full.index_copy_(0, live[:n].long(), grad_bary.view(n, 3))
    res = (grad_field, grads)
    if want_ray_head_grad:
        res += (d_ray_bias,)
    if want_bary_grad:
        res += (grad_bary,)
    if return_dx0:
        res += (rows,)
    if return_chain:
        ch = MlpChain()
        ch.d1, ch.d2, ch.d3, ch.d4, ch.dhead, ch.dx0 = buf[0:128], buf[128:256], buf[256:384], buf[384:512], buf[512:516], rows
        res += (ch,)
    return res


def composite_aux(sigma, edges, want_weights=False):
    """Two more per-ray sums over composite()'s weights, in one kernel (tn_composite_aux; linear time per ray) -- what nerfstudio's
    DepthRenderer(method="expected") and losses.lossfun_distortion compute in PyTorch on the materialised weights:
    depth_moment [R] = sum_i w_i (e_i + e_{i+1}) / 2 and distortion_raw [R] = sum_ij w_i w_j |u_i - u_j| + 1/3 sum_i w_i^2 delta_i
    (render.composite_aux_statement).  sigma f32 [R,S], edges f32 [R,S+1], non-decreasing per ray.
    Returns (depth_moment, distortion_raw), with want_weights also weights [R,S] (composite()'s, bit for bit)."""
    for x, name in ((sigma, "sigma"), (edges, "edges")):
        _check_input(x, name)
        _check(x.dtype == torch.float32, f"{name} must have float32 type")
    _check(sigma.dim() == 2, "sigma must be f32 [R,S]")
    R, S = sigma.shape
    _check(tuple(edges.shape) == (R, S + 1), "edges must be f32 [R,S+1]")
    dev = sigma.device
    _check(edges.device == dev, "all tensors must be on the same device")
    if S == 0:        # (no sample: both sums are empty; the entry point returns before it writes)
        return (torch.zeros(R, device=dev), torch.zeros(R, device=dev)) + ((sigma.clone(),) if want_weights else ())
    moment = _empty((R,), dtype=torch.float32, device=dev)
    dist = _empty((R,), dtype=torch.float32, device=dev)
    weights = _empty((R, S), dtype=torch.float32, device=dev) if want_weights else None
    with _on(dev):
        _lib.check(_lib.load().tn_composite_aux(R, S, _ptr(sigma), _ptr(edges), _ptr(moment), _ptr(dist), _ptr(weights), _stream(dev)))
    return (moment, dist, weights) if want_weights else (moment, dist)


def composite_backward(sigma, rgb, edges, d_out_rgb, d_out_acc, background=1.0, d_depth_moment=None, d_distortion=None):
    """Adjoint of composite() w.r.t. sigma [R,S] and rgb [R,S,3] (the median depth has no gradient).  sigma f32 [R,S], rgb f32
    [R,S,3], edges f32 [R,S+1]; d_out_rgb f32 [R,3] and d_out_acc f32 [R] (either may be None: that output has no gradient).
    d_depth_moment f32 [R], d_distortion f32 [R] (either may be None): the gradients of composite_aux()'s outputs, further terms of
    dL/dw (tn_composite_backward_aux); with both None the call is tn_composite_backward, as before they existed."""
    new = tuple((x, name) for x, name in ((d_depth_moment, "d_depth_moment"), (d_distortion, "d_distortion")) if x is not None)
    given = ((sigma, "sigma"), (rgb, "rgb"), (edges, "edges")) + tuple((x, name) for x, name in ((d_out_rgb, "d_out_rgb"), (d_out_acc, "d_out_acc"))
                                                                      if x is not None) + new
    for x, name in given:
        _check_input(x, name)
        _check(x.dtype == torch.float32, f"{name} must have float32 type")
    _check(sigma.dim() == 2, "sigma must be f32 [R,S]")
    R, S = sigma.shape
    _check(tuple(rgb.shape) == (R, S, 3) and tuple(edges.shape) == (R, S + 1), "shape mismatch")
    _check(d_out_rgb is None or tuple(d_out_rgb.shape) == (R, 3), "d_out_rgb must be f32 [R,3]")
    _check(d_out_acc is None or tuple(d_out_acc.shape) == (R,), "d_out_acc must be f32 [R]")
    for x, name in new:
        _check(tuple(x.shape) == (R,), f"{name} must be f32 [R]")
    dev = sigma.device
    _check(all(x.device == dev for x, _ in given), "all tensors must be on the same device")
    d_sigma = _empty((R, S), dtype=torch.float32, device=dev)
    d_rgb = _empty((R, S, 3), dtype=torch.float32, device=dev)
    if new:
        with _on(dev):
            _lib.check(_lib.load().tn_composite_backward_aux(R, S, _ptr(sigma), _ptr(rgb), _ptr(edges), _background(background),
                                                             _ptr(d_out_rgb), _ptr(d_out_acc), _ptr(d_depth_moment), _ptr(d_distortion),
                                                             _ptr(d_sigma), _ptr(d_rgb), _stream(dev)))
        return d_sigma, d_rgb
    with _on(dev):
        _lib.check(_lib.load().tn_composite_backward(R, S, _ptr(sigma), _ptr(rgb), _ptr(edges), _background(background), _ptr(d_out_rgb),
                                                     _ptr(d_out_acc), _ptr(d_sigma), _ptr(d_rgb), _stream(dev)))
    return d_sigma, d_rgb


def triangulate(points):
    """py_triangulate (py_binding.cpp:239-256).  The reference runs CGAL's Delaunay on the CPU
    (src/triangulation.cpp:34-75); CGAL is not part of this build, Qhull (scipy) stands in.
    Offline preprocessing, not on the hot path."""
    _check(points.dim() == 2 and points.size(1) == 3, "points must have shape [num_points, 3]")
    from .scenes import delaunay_cells

    cells = delaunay_cells(points.detach().cpu().contiguous().numpy())
    return torch.from_numpy(cells).to(points.device)


def find_average_spacing(points):
    """py_find_average_spacing (py_binding.cpp:229-237): mean distance to the 6 nearest
    neighbours (CGAL::compute_average_spacing<6>, src/triangulation.cpp:121-134)."""
    _check(points.is_contiguous(), "points must be contiguous")
    _check(points.device.type == "cpu", "points must be a CPU tensor")
    _check(points.dim() == 2 and points.size(1) == 3, "points must have shape [num_points, 3]")
    from scipy.spatial import cKDTree

    p = points.numpy()
    d, _ = cKDTree(p).query(p, k=7)
    return float(d[:, 1:].mean())


def gather_uint32(self, dim, index):
    """py_gather_uint32 (py_binding.cpp:374-399); not called by the model."""
    _check(index.dtype == torch.int32, "index must be a tensor of type int32")
    _check(self.is_floating_point(), "self must be a tensor of a floating-point type")
    _check(self.device == index.device, "self and index must be on the same device")
    _check(self.is_contiguous(), "self must be contiguous")
    _check(index.is_contiguous(), "index must be contiguous")
    _check(self.device.type == "cuda", "self must be on CUDA")
    _check(index.device.type == "cuda", "index must be on CUDA")
    _check(self.dim() == 1, "self must be 1-dimensional")
    _check(index.dim() == self.dim(), "self and index must have the same number of dimensions")
    _check(dim == 0, "dim must be 0")
    _check(self.dtype in (torch.float32, torch.float64), "self must be float32 or float64")
    result = _empty(index.shape, dtype=self.dtype, device=self.device)
    with _on(self.device):
        _lib.check(_lib.load().tn_gather_uint32(self.element_size(), self.numel(), index.numel(), _ptr(index), _ptr(self),
                                                _ptr(result), _stream(self.device)))
    return result


def scatter_ema_uint32(self, dim, index, decay, values):
    """py_scatter_ema_uint32 (py_binding.cpp:405-431): in-place x[idx] = x[idx]*decay + (1-decay)*v."""
    _check(dim == 0, "dim must be 0")
    _check(self.is_floating_point(), "self must be a tensor of a floating-point type")
    _check(self.is_contiguous(), "self must be contiguous")
    _check(self.dim() == 1, "self must be 1-dimensional")
    _check(self.device.type == "cuda", "self must be on CUDA")
    _check(index.dtype == torch.int32, "index must be a tensor of type int32")
    _check(index.is_contiguous(), "index must be contiguous")
    _check(index.device.type == "cuda", "index must be on CUDA")
    _check(values.is_contiguous(), "values must be contiguous")
    _check(self.device == index.device, "self and index must be on the same device")
    _check(values.device == index.device, "values and index must be on the same device")
    _check(values.dtype == self.dtype, "values and self must have the same dtype")
    _check(index.dim() == self.dim(), "self and index must have the same number of dimensions")
    _check(values.shape == index.shape, "values and index must have the same shape")
    _check(self.dtype in (torch.float32, torch.float64), "self must be float32 or float64")
    with _on(self.device):
        _lib.check(_lib.load().tn_scatter_ema_uint32(self.element_size(), self.numel(), index.numel(), _ptr(index),
                                                     float(decay), _ptr(values), _ptr(self), _stream(self.device)))
