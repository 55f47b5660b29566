"""The meshes, fields and levels every test of the isosurface extraction uses (tests/test_isosurface.py,
tests/test_isosurface_gpu.py), stated once, with the numpy statement's answers (geometry.isosurface_statement) computed once per
session and never modified.  Nothing here needs a GPU or the library.

A case is (xyz float32 [V, 3], cells int32 [T, 4], values float32 [V], level float, tet_mask uint8 [T] or None).  The groups:
one tetrahedron through the whole case table in both stored orientations and flat; degenerate values; each skip reason alone;
welding across a shared face; the order of the keys (by `a` first, ids on both sides of 2^16 and 2^20, the last id); T at every
wave, block and grid-cap edge (the constants are read from the .hip source); empty inputs; four closed surfaces; a linear
field, with the a-priori bound on the distance of its vertices from the plane; a masked surface."""
import importlib
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_CACHE = {}
U = 2.0 ** -24                       # unit round-off of float32


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def kernel_constants():
    """(threads per block, grid cap in blocks) of tn_isosurface.hip, read from its source"""
    text = (ROOT / "tetra-nerf_amd" / "csrc" / "tn_isosurface.hip").read_text()
    bt = int(re.search(r"constexpr int BT = (\d+);", text).group(1))
    blocks = int(re.search(r"constexpr unsigned ISO_BLOCKS = (\d+);", text).group(1))
    return bt, blocks


# ---- one tetrahedron: a general one (positive as stored in the order 0 1 2 3) and a flat one
_TET = np.array([[0.125, 0.25, -0.5], [1.5, 0.0, 0.25], [0.25, 1.25, 0.0], [0.5, 0.375, 1.75]], np.float32)
_FLAT = np.array([[0.0, 0.0, 0.5], [1.0, 0.25, 0.5], [0.25, 1.0, 0.5], [0.75, 0.75, 0.5]], np.float32)
ORDERS = {"pos": [0, 1, 2, 3], "neg": [1, 0, 2, 3]}
LEVEL = 0.125


def _code_values(code, order=(0, 1, 2, 3)):
    """values per vertex id such that STORED corner k (vertex order[k]) is inside iff bit k of `code` is set: inside corners above
    LEVEL, the others below it, every value different, so that no two edges share a t"""
    v = np.zeros(4, np.float32)
    v[list(order)] = [LEVEL + 0.5 + 0.25 * k if (code >> k) & 1 else LEVEL - 0.75 - 0.5 * k for k in range(4)]
    return v


def _one_tet(points, order, values, level=LEVEL, mask=None):
    return points.copy(), np.array([order], np.int32), np.asarray(values, np.float32), level, mask


# two tetrahedra sharing the face (1, 2, 3); with vertex 1 alone inside both emit one triangle and share two edges
_PAIR = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1.25, 1.0, 1.5]], np.float32)
_PAIR_CELLS = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int32)
_PAIR_VALUES = np.array([-1.0, 2.0, -0.5, -0.25, -2.0], np.float32)


def _pair(values=_PAIR_VALUES, cells=_PAIR_CELLS, mask=None):
    return _PAIR.copy(), cells.copy(), np.asarray(values, np.float32), 0.0, mask


def _with(values, index, x):
    v = np.array(values, np.float32)
    v[index] = x
    return v


def _key_order_a_first():
    """edges (1, 70000) and (2, 5) in one mesh: vertex 1 alone is inside the first tetrahedron, vertex 2 alone the second"""
    V = 70001
    rng = np.random.default_rng(70)
    xyz = rng.random((V, 3)).astype(np.float32)
    values = np.full(V, -1.0, np.float32)
    values[[1, 2]] = 1.0
    values[[70000, 5, 10, 11, 12, 13]] = [-0.5, -0.25, -2.0, -3.0, -0.75, -1.5]
    cells = np.array([[70000, 1, 11, 10], [13, 2, 5, 12]], np.int32)
    return xyz, cells, values, 0.0, None


def _around(power):
    """V = 2^power + 1; 48 tetrahedra over ids on both sides of 2^power and the last id, random values"""
    V = (1 << power) + 1
    rng = np.random.default_rng(power)
    pool = np.array([0, 1, 2, 3, (1 << power) - 3, (1 << power) - 2, (1 << power) - 1, 1 << power], np.int64)
    xyz = rng.random((V, 3)).astype(np.float32)
    values = np.zeros(V, np.float32)
    values[pool] = rng.normal(size=len(pool)).astype(np.float32)
    cells = np.stack([rng.choice(pool, 4, replace=False) for _ in range(48)]).astype(np.int32)
    cells[0] = [1 << power, (1 << power) - 1, 0, 1]
    return xyz, cells, values, 0.0, None


def sphere_mesh(scenes, n, seed):
    """the 8 corners (+-1)^3 plus n uniform points of the cube, cells from the project's own triangulation"""
    key = ("sphere_mesh", n, seed)
    if key not in _CACHE:
        corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
        pts = np.concatenate([corners, np.random.default_rng(seed).random((n, 3)) * 2 - 1]).astype(np.float32)
        _CACHE[key] = (pts, scenes.delaunay_cells(pts))
    return _CACHE[key]


SPHERES = {"sphere_56": (56, 0), "sphere_120": (120, 1), "sphere_300": (300, 2), "sphere_1000": (1000, 3)}
SPHERE_LEVEL = -0.36


def _sphere(scenes, n, seed, mask=None):
    pts, cells = sphere_mesh(scenes, n, seed)
    values = -(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2])
    return pts, cells, values.astype(np.float32), SPHERE_LEVEL, mask


def _masked_sphere(scenes):
    pts, cells, values, level, _ = _sphere(scenes, *SPHERES["sphere_120"])
    mask = (np.random.default_rng(5).random(len(cells)) < 0.7).astype(np.uint8)
    return pts, cells, values, level, mask


# ---- the linear field
PLANE_N = np.array([0.3, -0.5, 0.8], np.float64)
PLANE_C, PLANE_LEVEL = 0.1, 0.05


def _linear(scenes):
    pts, cells = sphere_mesh(scenes, *SPHERES["sphere_300"])
    values = (pts.astype(np.float64) @ PLANE_N + PLANE_C).astype(np.float32)
    return pts, cells, values, PLANE_LEVEL, None


def plane_bound(xyz, values):
    """An a-priori bound on the distance of every surface vertex of the linear field f(x) = n . x + c from the plane
    { f = L }, L the float32 level.  u = 2^-24.
      values: v~ = fl32(f(x)) with f evaluated in float64:  |v~ - f(x)| <= u F (1 + 2^-20),  F = max |f| over the vertices.
      t: with t^ = (L - v~a) / (v~b - v~a) in [0, 1] exact, the computed t has three roundings: |t - t^| <= 3.01 u.
      p: per coordinate p = fl(xa + fl(t fl(xb - xa))), three more roundings: with D = max |xb - xa| and X = max |x| over the mesh,
         |p - (xa + t^ (xb - xa))| <= 3.01 u D + 2.01 u D + 1.01 u X = e_p.
      f is linear and v~a + t^ (v~b - v~a) = L exactly, so f(xa + t^ (xb - xa)) - L = (1 - t^) (f(xa) - v~a) + t^ (f(xb) - v~b), at
      most the error of one value.  Hence  |f(p) - L| <= u F (1 + 2^-20) + |n|_1 e_p,  and the distance is that over |n|_2."""
    x = np.asarray(xyz, np.float64)
    F = np.abs(x @ PLANE_N + PLANE_C).max()
    D = (x.max(0) - x.min(0)).max()
    X = np.abs(x).max()
    e_p = (5.02 * D + 1.01 * X) * U
    return (U * F * (1 + 2.0 ** -20) + np.abs(PLANE_N).sum() * e_p) / np.linalg.norm(PLANE_N), e_p


def plane_distance(positions):
    """float64 signed distances of float32 positions from the plane { n . x + c = fl32(level) }"""
    return (np.asarray(positions, np.float64) @ PLANE_N + PLANE_C - float(np.float32(PLANE_LEVEL))) / np.linalg.norm(PLANE_N)


# ---- T at the wave, block and grid-cap edges: a soup cut from a mesh of `scenes`
def soup(scenes, T):
    """the first T tetrahedra of scenes.random_mesh (a small mesh for the wave and block edges, one with more tetrahedra than the
    capped grid has lanes for the cap), values a paraboloid about the cube's centre whose level a tenth of them cross"""
    name = "soup_small" if T <= 2500 else "soup_large"
    if name not in _CACHE:
        pts, cells = scenes.random_mesh(400, 3) if name == "soup_small" else scenes.random_mesh(42000, 11)
        d = pts - np.float32(0.5)
        _CACHE[name] = (pts, cells, -(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32))
    pts, cells, values = _CACHE[name]
    assert T <= len(cells), (T, len(cells))
    return pts, np.ascontiguousarray(cells[:T]), values, -0.2, None


def size_edges():
    """T of the size cases: one below, at and above a wave, a block, and the lanes of the capped grid -- and, because the counting
    pass runs one lane more than there are tetrahedra (it writes the scan's last 0), one further below the cap"""
    bt, blocks = kernel_constants()
    lanes = bt * blocks
    return [63, 64, 65, bt - 1, bt, bt + 1, lanes - 2, lanes - 1, lanes, lanes + 1]


def _table_cases():
    out = {}
    for code in range(16):
        for name, order in ORDERS.items():
            out[f"code_{code:02d}_{name}"] = (lambda code=code, order=order: _one_tet(_TET, order, _code_values(code, order)))
    out["flat_1_edge_code"] = lambda: _one_tet(_FLAT, [0, 1, 2, 3], _code_values(1))
    out["flat_2_edge_code"] = lambda: _one_tet(_FLAT, [0, 1, 2, 3], _code_values(6))
    return out


FIXED = {
    **_table_cases(),
    # a value equal to the level is inside: t = 0 on the three edges out of that corner, a zero-area triangle, kept
    "value_at_level": lambda: _one_tet(_TET, [0, 1, 2, 3], [LEVEL, -1.0, -2.0, -0.5]),
    "value_at_level_far_end": lambda: _one_tet(_TET, [3, 1, 2, 0], [-1.0, -2.0, -0.5, LEVEL]),
    "all_at_level": lambda: _one_tet(_TET, [0, 1, 2, 3], [LEVEL] * 4),
    # each skip reason alone, on the pair: the first tetrahedron is silent, the second emits
    "pair": _pair,
    "skip_mask": lambda: _pair(mask=np.array([0, 1], np.uint8)),
    "skip_id_past_V": lambda: _pair(cells=np.array([[0, 1, 2, 5], [1, 2, 3, 4]], np.int32)),
    "skip_id_empty": lambda: _pair(cells=np.array([[-1, 1, 2, 3], [1, 2, 3, 4]], np.int32)),
    "skip_nan": lambda: _pair(_with(_PAIR_VALUES, 0, np.nan)),
    "skip_inf": lambda: _pair(_with(_PAIR_VALUES, 0, np.inf)),
    "skip_2_126": lambda: _pair(_with(_PAIR_VALUES, 0, 2.0 ** 126)),
    "kept_below_2_126": lambda: _pair(_with(_PAIR_VALUES, 0, -np.nextafter(np.float32(2.0 ** 126), np.float32(0)))),
    "key_a_first": _key_order_a_first,
    "ids_around_2_16": lambda: _around(16),
    "ids_around_2_20": lambda: _around(20),
    "no_tets": lambda: (_PAIR.copy(), np.zeros((0, 4), np.int32), _PAIR_VALUES.copy(), 0.0, None),
    "no_crossing": lambda: _pair(np.full(5, -1.0, np.float32)),
}
SCENE = {
    **{name: (lambda scenes, a=args: _sphere(scenes, *a)) for name, args in SPHERES.items()},
    "sphere_120_masked": _masked_sphere,
    "linear": _linear,
}
SKIPPED_FIRST = ["skip_mask", "skip_id_past_V", "skip_id_empty", "skip_nan", "skip_inf", "skip_2_126"]


def names(large=True):
    """every case; large=False leaves out the grid-cap soups (a quarter of a million tetrahedra each)"""
    sizes = [f"soup_{T}" for T in size_edges() if large or T <= 2500]
    return sorted(FIXED) + sorted(SCENE) + sizes


def case(scenes, name):
    if ("case", name) not in _CACHE:
        if name in FIXED:
            c = FIXED[name]()
        elif name in SCENE:
            c = SCENE[name](scenes)
        else:
            c = soup(scenes, int(name[len("soup_"):]))
        xyz, cells, values, level, mask = c
        _CACHE["case", name] = (np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(cells, np.int32),
                                np.ascontiguousarray(values, np.float32), float(level),
                                None if mask is None else np.ascontiguousarray(mask, np.uint8))
    return _CACHE["case", name]


def statement(scenes, name):
    """the numpy statement's answer on case(name), made once -- do not write into it"""
    if ("statement", name) not in _CACHE:
        s = geometry().isosurface_statement(*case(scenes, name))
        if name == "linear":                                                  # the reference itself is held to the bound, in float64
            xyz, _, values, _, _ = case(scenes, name)
            assert np.abs(plane_distance(s["positions"])).max() <= plane_bound(xyz, values)[0]
        _CACHE["statement", name] = s
    return _CACHE["statement", name]


ARRAYS = ("positions", "triangles", "triangle_tets", "edge_vertices", "edge_t")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


# ---- properties of a triangle mesh
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def closed_and_oriented(triangles):
    """every directed edge occurs once and its reverse once"""
    e = directed_edges(triangles)
    code = e[:, 0] * (int(e.max()) + 1) + e[:, 1]
    back = e[:, 1] * (int(e.max()) + 1) + e[:, 0]
    uniq, counts = np.unique(code, return_counts=True)
    return bool((counts == 1).all()) and bool(np.isin(back, uniq).all())


def euler_characteristic(num_vertices, triangles):
    e = np.sort(directed_edges(triangles), 1)
    return num_vertices - len(np.unique(e, axis=0)) + len(triangles)


def enclosed_volume(positions, triangles):
    p, t = np.asarray(positions, np.float64), np.asarray(triangles, np.int64)
    return float(np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0)
