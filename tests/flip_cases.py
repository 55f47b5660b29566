"""The meshes every test of the Delaunay repair by flips uses (tests/test_flip.py, tests/test_flip_gpu.py), stated once, with the
numpy statement's answers (geometry.flip_faces_statement) computed once per session and never modified.  Nothing here needs a
GPU or the library.

A case is (xyz float32 [V, 3], cells int32 [T, 4], faces int32 [F, 3], face_tets int32 [F, 2]); the face table is
edge_split_cases.face_table (every sorted id triple once, its first two rows, -1 = no second row).  The groups: hand-made rows (the
violated convex bipyramid: a 2-3 flip; the ring of three around a reflex edge: a 3-2 flip, whose three faces are three candidates
for the same rows, so two are lost; the ring with four rows and the ring with its third row missing: unflippable; a cospherical
face: verdict uncertain; d, e and an edge in one plane: orientation uncertain; d and e on one side: invalid, also where the orientation is uncertain too; an id >= V; a NaN
coordinate; two bipyramids that share a row: the smaller face id wins; a Delaunay mesh: nothing violated; no tetrahedra); soups of
bipyramids and lone tetrahedra at every wave, block and grid-cap edge of T, of F and of the candidate count (the constants are
read from the .hip source); and a random mesh of 400 points moved under the step limiter, as it is and after one edge-split and
one centroid-split round."""
import importlib
import re
from pathlib import Path

import numpy as np
import torch

from edge_split_cases import face_table, bits, vol6, hull_faces   # noqa: F401  (re-exported to the tests)

ROOT = Path(__file__).resolve().parents[1]
_CACHE = {}
EMPTY = 0xFFFFFFFF
ARRAYS = ("cells", "cell_sources", "flipped", "tet_flip", "tet_offsets", "face_flip", "counters")
COUNTERS = ("interior", "violated", "verdict_uncertain", "refused_id", "refused_invalid", "refused_uncertain",
            "refused_unflippable", "refused_lost", "accepted_23", "accepted_32")


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def kernel_constants():
    """(threads per block, grid cap in blocks) of tn_flip.hip, read from its source"""
    text = (ROOT / "tetra-nerf_amd" / "csrc" / "tn_flip.hip").read_text()
    bt = int(re.search(r"constexpr int BT = (\d+);", text).group(1))
    blocks = int(re.search(r"constexpr unsigned FLIP_BLOCKS = (\d+);", text).group(1))
    return bt, blocks


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def _case(xyz, cells, table_of=None):
    cells = np.asarray(cells, np.int64).reshape(-1, 4)
    return np.asarray(xyz, np.float32).reshape(-1, 3), _i32(cells), *face_table(cells if table_of is None else table_of)


# ------------------------------------------------------------------------------------------------------------------ hand-made
TRIANGLE = ((1, 0, 0), (-0.5, 0.875, 0), (-0.5, -0.875, 0))                   # around the z axis, in the plane z = 0


def bipyramid(h=0.3125, offset=0, shift=(0, 0, 0)):
    """the triangle with the apices (0, 0, h) and (0, 0, -h), as the two rows that share the triangle.  h = 0.3125: the lower apex is
    inside the upper row's circumsphere and the axis crosses the triangle: a 2-3 flip.  h = 2: locally Delaunay."""
    pts = np.array([*TRIANGLE, (0, 0, h), (0, 0, -h)], np.float64) + np.asarray(shift, np.float64)
    return pts.astype(np.float32), np.array([[0, 1, 2, 3], [0, 1, 2, 4]], np.int64) + offset


def ring3(rows=(0, 1, 2)):
    """the axis x = (0, 0, 2), y = (0, 0, -2) with the triangle around it, as the three rows (x, y, r_i, r_i+1): the bipyramid's
    other triangulation, with tall apices, where every face (x, y, r_i) is violated and xy is its reflex edge: a 3-2 flip"""
    pts = np.array([(0, 0, 2), (0, 0, -2), *TRIANGLE], np.float32)
    cells = np.array([[0, 1, 2 + i, 2 + (i + 1) % 3] for i in range(3)], np.int64)[list(rows)]
    return pts, cells


def ring4():
    """four rows around the axis; seen from d = (0, 1, 0) the segment from c to e passes beyond the axis: the face (x, y, d) is a
    3-2 candidate whose two neighbours across the axis are different rows"""
    pts = np.array([(0, 0, 2), (0, 0, -2), (1, 0, 0), (0, 1, 0), (-1, -0.25, 0), (0.25, -1, 0)], np.float32)
    return pts, np.array([[0, 1, 2, 3], [0, 1, 3, 4], [0, 1, 4, 5], [0, 1, 5, 2]], np.int64)


def _cospherical():
    pts = np.array([(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)], np.float32)      # all on the unit sphere
    return _case(pts, [[0, 1, 2, 3], [0, 1, 2, 4]])


def _coplanar_edge():
    pts = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 0.25), (0, 0, -0.25)], np.float32)   # a, b, d, e in the plane y = 0
    return _case(pts, [[0, 1, 2, 3], [0, 1, 2, 4]])


def _same_side():
    pts, cells = bipyramid()
    pts[4] = (0.125, 0, 0.125)                                                # e above the triangle, beside d, inside the sphere
    return _case(pts, cells)


def _same_side_coplanar():
    """d and e above the triangle AND in one plane with a and b: invalid comes before uncertain"""
    pts = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 0.25), (0, 0, 0.125)], np.float32)
    return _case(pts, [[0, 1, 2, 3], [0, 1, 2, 4]])


def _bad_id():
    pts, cells = bipyramid()
    cells[1, 3] = 5                                                           # V = 5
    return _case(pts, cells)


def _nan():
    pts, cells = bipyramid()
    pts[4, 1] = np.nan
    return _case(pts, cells)


def _shared_row():
    """rows (a,b,c,d), (a,b,c,e), (a,b,e,g): the middle row is wanted by the faces (a,b,c) and (a,b,e), both violated and convex"""
    pts = np.array([(1, 0, 0), (-0.5, 0.875, 0), (-0.5, -0.875, 0), (0, 0, 0.3125), (0, 0, -0.3125), (0.1875, 0.8125, -0.0625)], np.float32)
    return _case(pts, [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 4, 5]])


def _mesh_case(mesh):
    xyz, cells = mesh
    return _case(xyz, cells)


# ----------------------------------------------------------------------------------------------------------------------- soups
def soup(copies, lone=0, cut=False):
    """`copies` violated bipyramids (2 rows, 7 faces, one candidate each) and `lone` single tetrahedra (4 faces), copy n moved by
    (3 (n mod 7), 3 (n mod 5), 1.5 (n mod 3)) plus 32 (n // 105) along x so that the roundings differ and no two copies touch.
    cut: the last bipyramid loses its second row."""
    key = ("soup", copies, lone, cut)
    if key not in _CACHE:
        pts, cells = bipyramid()
        n = np.arange(copies + lone)
        shift = np.stack([3 * (n % 7) + 32 * (n // 105), 3 * (n % 5), 1.5 * (n % 3)], 1).astype(np.float32)
        xyz = (pts[None] + shift[:, None]).reshape(-1, 3).astype(np.float32)
        both = (cells[None] + (len(pts) * n[:copies])[:, None, None]).reshape(-1, 4)
        if cut:
            both = both[:-1]
        alone = cells[:1] + (len(pts) * n[copies:])[:, None]
        _CACHE[key] = _case(xyz, np.concatenate([both, alone]))
    return _CACHE[key]


def soup_edges():
    bt, blocks = kernel_constants()
    return tuple(e + k for e in (64, bt, bt * blocks) for k in (-1, 0, 1))


def soup_for(what, n):
    """the soup whose T, F or candidate count is n"""
    if what == "T":
        return soup((n + 1) // 2, cut=bool(n % 2))
    if what == "F":                                                           # 7 p + 4 q = n
        q = (2 * n) % 7
        assert (n - 4 * q) % 7 == 0 and n >= 4 * q
        return soup((n - 4 * q) // 7, q)
    return soup(n)


# ---------------------------------------------------------------------------------------------------------- the moved mesh
MOVED = {"points": 400, "seed": 3, "sigma": 0.02, "fraction": 0.45}


def moved_mesh(points=None, seed=None):
    """(xyz float32 [V, 3] moved, cells int32 [T, 4]): scenes.random_mesh, every vertex moved by N(0, sigma) and the step limited by
    geometry.limit_vertex_step_statement, so that no tetrahedron inverts"""
    points, seed = points or MOVED["points"], MOVED["seed"] if seed is None else seed
    key = ("moved", points, seed)
    if key not in _CACHE:
        scenes = importlib.import_module("tetra-nerf_amd.scenes")
        xyz, cells = scenes.random_mesh(points, seed)
        xyz, cells = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(cells, np.int32)
        new = (xyz + np.random.default_rng(100 + seed).normal(scale=MOVED["sigma"], size=xyz.shape)).astype(np.float32)
        out = geometry().limit_vertex_step_statement(torch.from_numpy(xyz), torch.from_numpy(new), torch.from_numpy(cells), MOVED["fraction"])
        assert int(out["counters"][2]) == 0 and int(out["counters"][3]) == 0
        _CACHE[key] = (np.ascontiguousarray(out["xyz"].numpy(), np.float32), cells)
    return _CACHE[key]


def _moved_split(method):
    g = geometry()
    xyz, cells = moved_mesh()
    select = (np.random.default_rng(11).random(len(cells)) < 0.2).astype(np.uint8)
    if method == "edge":
        out = g.split_edges_statement(xyz, cells, select, *face_table(cells))
    else:
        out = g.split_tetrahedra_statement(xyz, cells, select)
    return _case(out["vertices"], out["cells"])


FIXED = {
    "bipyramid_23": lambda s: _case(*bipyramid()),
    "ring3_32": lambda s: _case(*ring3()),
    "ring4_unflippable": lambda s: _case(*ring4()),
    "ring3_missing_t2": lambda s: _case(*ring3((0, 2))),
    "cospherical": lambda s: _cospherical(),
    "coplanar_edge": lambda s: _coplanar_edge(),
    "same_side": lambda s: _same_side(),
    "same_side_coplanar": lambda s: _same_side_coplanar(),
    "bad_id": lambda s: _bad_id(),
    "nan": lambda s: _nan(),
    "shared_row": lambda s: _shared_row(),
    "nothing_violated": lambda s: _mesh_case(s.random_mesh(200, 4)),
    "bipyramid_regular": lambda s: _case(*bipyramid(2.0)),
    "no_tets": lambda s: (np.zeros((3, 3), np.float32), np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int32)),
    "moved_400": lambda s: _mesh_case(moved_mesh()),
    "moved_400_edge_split": lambda s: _moved_split("edge"),
    "moved_400_centroid_split": lambda s: _moved_split("centroid"),
}
# the cases whose input is a conforming mesh in which something is flipped: the structure tests
MESHES = ("bipyramid_23", "ring3_32", "shared_row", "moved_400", "moved_400_edge_split", "moved_400_centroid_split")


def names(soups=False, grid_cap=True):
    out = list(FIXED)
    if soups:
        bt, blocks = kernel_constants()
        out += [f"soup_{what}_{n}" for what in ("T", "F", "C") for n in soup_edges() if grid_cap or n < bt * blocks - 1]
    return out


def case(scenes, name):
    if name not in _CACHE:
        if name.startswith("soup_"):
            _, what, n = name.split("_")
            c = soup_for(what, int(n))
        else:
            c = FIXED[name](scenes)
        c = (np.ascontiguousarray(c[0], np.float32), np.ascontiguousarray(c[1], np.int32), np.ascontiguousarray(c[2], np.int32),
             np.ascontiguousarray(c[3], np.int32))
        for a in c:
            a.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def statement(scenes, name):
    key = ("statement", name)
    if key not in _CACHE:
        _CACHE[key] = geometry().flip_faces_statement(*case(scenes, name))
        for a in _CACHE[key].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _CACHE[key]


def counters(scenes, name):
    return dict(zip(COUNTERS, statement(scenes, name)["counters"].tolist()))


def repaired(scenes=None):
    """geometry.flip_to_delaunay_statement on the moved mesh with face_table, once per session"""
    if "repaired" not in _CACHE:
        xyz, cells = moved_mesh()
        _CACHE["repaired"] = geometry().flip_to_delaunay_statement(xyz, cells, face_table)
    return _CACHE["repaired"]
