"""The meshes and the raw vertex step every test of the vertex step limiter uses (tests/test_vertex_guard.py,
tests/test_vertex_guard_gpu.py), stated once, with the torch statement's answers (geometry.limit_vertex_step_statement) computed
once per session and never modified.

The raw step: every vertex moves by 3 x its star width (geometry.star_width) in a random direction of its own -- six times what
the bound allows, so an unlimited or a too weakly limited step turns tetrahedra inside out on every one of these meshes.  Vertices
no tetrahedron names (star width +inf) do not move."""
import importlib

import numpy as np
import torch

SEED = 11
RAW_FACTOR = 3.0
CPU_MESHES = ("random_1500", "grid_12_jitter", "grid_16", "cube", "shells", "near_duplicates", "colmap_like")
KERNEL_MESHES = ("cube", "random_1500", "grid_16", "near_duplicates")          # host emulation and GPU kernels
_CACHE = {}


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def mesh(scenes, name):
    """(points float32 [V, 3], cells int32 [T, 4]), made once"""
    if ("mesh", name) not in _CACHE:
        make = {
            "random_1500": lambda: scenes.random_mesh(1500, 1),
            "grid_12_jitter": lambda: scenes.grid_mesh(12, 0.2),
            "grid_16": lambda: scenes.grid_mesh(16),               # thousands of zero-volume tetrahedra: most vertices freeze
            "cube": lambda: scenes.cube_mesh(),                    # T = 12, V = 9
            "shells": lambda: scenes.shells_mesh(),
            "near_duplicates": lambda: scenes.near_duplicates_mesh(),
            "colmap_like": lambda: scenes.colmap_like_mesh(),
        }[name]
        pts, cells = make()
        _CACHE["mesh", name] = (np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(cells).astype(np.int32))
    return _CACHE["mesh", name]


def raw_step(pts, cells, seed=SEED, factor=RAW_FACTOR):
    """float32 [V, 3]: the vertices after the raw step"""
    star = geometry().star_width(torch.from_numpy(pts), torch.from_numpy(cells)).numpy().astype(np.float64)
    star[~np.isfinite(star)] = 0.0
    v = np.random.default_rng(seed).normal(size=pts.shape)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return np.ascontiguousarray((pts.astype(np.float64) + factor * star[:, None] * v).astype(np.float32))


def case(scenes, name):
    """(old, new, cells) of one mesh as numpy arrays, made once"""
    if ("case", name) not in _CACHE:
        pts, cells = mesh(scenes, name)
        _CACHE["case", name] = (pts, raw_step(pts, cells), cells)
    return _CACHE["case", name]


def statement(scenes, name, fraction=0.45, check_range=True):
    """the statement's answer on `case(name)`: a dict of CPU tensors, made once -- do not write into it"""
    key = ("statement", name, fraction, check_range)
    if key not in _CACHE:
        old, new, cells = case(scenes, name)
        _CACHE[key] = geometry().limit_vertex_step_statement(torch.from_numpy(old), torch.from_numpy(new), torch.from_numpy(cells),
                                                             fraction, _check_range=check_range)
    return _CACHE[key]


def quality(scenes, name):
    """(width float32 [T], orient int8 [T], star_width float32 [V]) of the old vertices by the statement, made once"""
    if ("quality", name) not in _CACHE:
        old, _, cells = case(scenes, name)
        g = geometry()
        w, o = g.tet_width_orient(torch.from_numpy(old), torch.from_numpy(cells))
        _CACHE["quality", name] = (w, o, g.star_width(torch.from_numpy(old), torch.from_numpy(cells), w))
    return _CACHE["quality", name]


def bits(x):
    """integer view of a float tensor / array, for bit-for-bit comparisons"""
    if isinstance(x, torch.Tensor):
        return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)
