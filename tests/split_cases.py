"""The meshes and selections every test of the tetrahedron split uses (tests/test_split.py, tests/test_split_gpu.py), stated once,
with the numpy statement's answers (geometry.split_tetrahedra_statement) computed once per session and never modified, and the
float64 references of the preservation tests.  Nothing here needs a GPU or the library.

A case is (xyz float32 [V, 3], cells int32 [T, 4], select uint8 [T]).  The groups: the stock scenes (the cube with everything
asked; a random mesh with 30 % asked; the two grids, whose flat tetrahedra are refused; the near-duplicates mesh, where the fp32
centroid rounds onto or across a face); hand-made rows (an id >= V, a NaN coordinate); nothing asked; no tetrahedra; and soups
tiled from the cube at every wave, block and grid-cap edge of T (the constants are read from the .hip source), each with none,
one, every third and all of its tetrahedra asked."""
import importlib
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_CACHE = {}
U = 2.0 ** -24                       # unit round-off of float32
ARRAYS = ("vertices", "cells", "cell_parent", "vertex_parents", "offsets", "counters")


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def kernel_constants():
    """(threads per block, grid cap in blocks) of tn_split.hip, read from its source"""
    text = (ROOT / "tetra-nerf_amd" / "csrc" / "tn_split.hip").read_text()
    bt = int(re.search(r"constexpr int BT = (\d+);", text).group(1))
    blocks = int(re.search(r"constexpr unsigned SPLIT_BLOCKS = (\d+);", text).group(1))
    return bt, blocks


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _all(cells):
    return np.ones(len(cells), np.uint8)


def _bad_id():
    """five rows over V = 6 vertices: row 1 names vertex 6 (= V), row 3 names 0xFFFFFFFF; the others are fine"""
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1.25, 1.0, 1.5], [-1, -0.5, -0.25]], np.float32)
    cells = np.array([[0, 1, 2, 3], [1, 2, 3, 6], [1, 2, 3, 4], [0, 2, -1, 5], [0, 2, 1, 5]], np.int32)
    return xyz, cells, _all(cells)


def _nan_coordinate():
    """vertex 4 has a NaN coordinate: row 1 names it and is refused as flat (orientation 0); rows 0 and 2 do not"""
    xyz, cells, select = _bad_id()
    xyz[4, 1] = np.nan
    cells = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [0, 2, 1, 5]], np.int32)
    return xyz, cells, _all(cells)


def soup_sizes():
    bt, blocks = kernel_constants()
    return (1, 63, 64, 65, bt - 1, bt, bt + 1, bt * blocks - 1, bt * blocks, bt * blocks + 1)


SELECTIONS = ("none", "one", "third", "all")


def soup(scenes, T):
    """T tetrahedra tiled from the cube mesh: copy n is moved by (2 n mod 7, n mod 5, 0.5 (n mod 3)) so that the roundings differ"""
    key = ("soup", T)
    if key not in _CACHE:
        pts, cells = scenes.cube_mesh()
        pts, cells = np.asarray(pts, np.float32), np.asarray(cells, np.int64)
        copies = (T + len(cells) - 1) // len(cells)
        n = np.arange(copies)
        shift = np.stack([(2 * n) % 7, n % 5, 0.5 * (n % 3)], 1).astype(np.float32)
        xyz = (pts[None] + shift[:, None]).reshape(-1, 3).astype(np.float32)
        all_cells = (cells[None] + (len(pts) * n)[:, None, None]).reshape(-1, 4)[:T]
        _CACHE[key] = (np.ascontiguousarray(xyz), np.ascontiguousarray(all_cells.astype(np.int32)))
    return _CACHE[key]


def _soup_case(scenes, T, selection):
    xyz, cells = soup(scenes, T)
    select = np.zeros(T, np.uint8)
    if selection == "one":
        select[(2 * T) // 3] = 1
    elif selection == "third":
        select[::3] = 1
    elif selection == "all":
        select[:] = 1
    return xyz, cells, select


def _random_30(scenes):
    pts, cells = scenes.random_mesh(300, 3)
    return pts, cells, (np.random.default_rng(30).random(len(cells)) < 0.3).astype(np.uint8)


FIXED = {
    "cube_all": lambda s: (*s.cube_mesh(), _all(s.cube_mesh()[1])),
    "random_300_30pct": _random_30,
    "grid_4_all": lambda s: (*s.grid_mesh(4), _all(s.grid_mesh(4)[1])),
    "grid_6_all": lambda s: (*s.grid_mesh(6), _all(s.grid_mesh(6)[1])),
    "near_duplicates_400_all": lambda s: (*s.near_duplicates_mesh(400), _all(s.near_duplicates_mesh(400)[1])),
    "id_past_V": lambda s: _bad_id(),
    "nan_coordinate": lambda s: _nan_coordinate(),
    "none_asked": lambda s: (*s.random_mesh(300, 3), np.zeros(len(s.random_mesh(300, 3)[1]), np.uint8)),
    "no_tets": lambda s: (np.zeros((3, 3), np.float32), np.zeros((0, 4), np.int32), np.zeros(0, np.uint8)),
}
REFUSED_FLAT = {"grid_4_all": 25, "grid_6_all": 136, "near_duplicates_400_all": 86, "cube_all": 0, "random_300_30pct": 0}


def names(soups=False):
    out = list(FIXED)
    if soups:
        out += [f"soup_{T}_{sel}" for T in soup_sizes() for sel in SELECTIONS]
    return out


def case(scenes, name):
    if name not in _CACHE:
        if name.startswith("soup_"):
            _, T, sel = name.split("_")
            _CACHE[name] = _soup_case(scenes, int(T), sel)
        else:
            xyz, cells, select = FIXED[name](scenes)
            _CACHE[name] = (np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(cells, np.int32), np.ascontiguousarray(select, np.uint8))
        for a in _CACHE[name]:
            a.setflags(write=False)
    return _CACHE[name]


def statement(scenes, name):
    key = ("statement", name)
    if key not in _CACHE:
        _CACHE[key] = geometry().split_tetrahedra_statement(*case(scenes, name))
        for a in _CACHE[key].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _CACHE[key]


def values_for(V, rows, seed=0, integers=False):
    """a per-vertex array f32 [rows, V]: N(0, 1), or small integers (whose sums of four are exact, and so are their quarters)"""
    rng = np.random.default_rng(1000 * rows + seed)
    if integers:
        return rng.integers(-64, 65, (rows, V)).astype(np.float32)
    return rng.normal(size=(rows, V)).astype(np.float32)


def vol6(p):
    """signed ((p1-p0) x (p2-p0)) . (p3-p0) of p float64 [n, 4, 3]"""
    return np.einsum("ni,ni->n", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])


def parent_interpolant(xyz, cells, field):
    """(F0 float64 [n, rows], gradient float64 [n, rows, 3], p0 float64 [n, 3]) of the affine interpolant of field f32 [rows, V] on
    the n (non-flat) tetrahedra `cells`: P(x) = F0 + gradient . (x - p0)"""
    p = xyz.astype(np.float64)[cells]
    F = field.astype(np.float64).T[cells]                                     # [T, 4, rows]
    A = p[:, 1:] - p[:, :1]                                                   # [T, 3, 3]
    grad = np.linalg.solve(A, F[:, 1:] - F[:, :1])                            # [T, 3, rows]
    return F[:, 0], np.swapaxes(grad, 1, 2), p[:, 0]
