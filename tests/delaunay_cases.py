"""The meshes, moves and hand-made cases every test of the Delaunay monitor and of the per-tetrahedron state transfer uses
(tests/test_delaunay.py, tests/test_delaunay_gpu.py), stated once, with the numpy statement's answers
(geometry.delaunay_face_statement) computed once per session and never modified.

The face table is the tracer's where there is one (TetrahedraTracer.face_tables); `face_tets_of` builds one on the CPU in the same
spirit -- faces in first-seen order over the tetrahedra, (first tetrahedron, second tetrahedron or EMPTY) -- for the tests that
have no library call to make.  The verdict on a face is a function of its row alone, so the order of the rows is immaterial."""
import importlib
from fractions import Fraction

import numpy as np

EMPTY = 0xFFFFFFFF
SIGMA = 0.005                       # the Gaussian move after which random_mesh(400, 3) is valid but no longer Delaunay
_CACHE = {}


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def face_tets_of(cells):
    """uint32 [F, 2]: the two tetrahedra of every face, faces in first-seen order; the second is EMPTY on the hull"""
    cells = np.asarray(cells).astype(np.int64)
    T = len(cells)
    tri = np.sort(np.stack([cells[:, [1, 2, 3]], cells[:, [0, 2, 3]], cells[:, [0, 1, 3]], cells[:, [0, 1, 2]]], 1).reshape(-1, 3), 1)
    tet = np.repeat(np.arange(T), 4)
    _, first, inverse, counts = np.unique(tri, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    assert counts.max() <= 2, "a triangle shared by more than two tetrahedra"
    order = np.argsort(first, kind="stable")                  # unique rows by first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    face = rank[inverse]
    out = np.full((len(order), 2), EMPTY, np.uint32)
    seen = np.zeros(len(order), bool)
    for i in np.argsort(face, kind="stable"):                 # the rows of one face in the order of their tetrahedra
        out[face[i], 1 if seen[face[i]] else 0] = tet[i]
        seen[face[i]] = True
    return out


def mesh(scenes, name):
    """(points float32 [V, 3], cells int32 [T, 4]), made once"""
    if ("mesh", name) not in _CACHE:
        if name == "random_400_moved":
            pts, cells = mesh(scenes, "random_400")
            pts = (pts + np.random.default_rng(17).normal(scale=SIGMA, size=pts.shape)).astype(np.float32)
        else:
            make = {
                "random_400": lambda: scenes.random_mesh(400, 3),
                "grid_5": lambda: scenes.grid_mesh(5),
                "cube": lambda: scenes.cube_mesh(),
                "random_1500": lambda: scenes.random_mesh(1500, 1),
                "random_20000": lambda: scenes.random_mesh(20000, 23),       # more faces than lanes of the capped grid
            }[name]
            pts, cells = make()
        _CACHE["mesh", name] = (np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(cells).astype(np.int32))
    return _CACHE["mesh", name]


# ---- hand-made two-tetrahedron meshes: t0 = (0, 1, 2, 3), t1 = (1, 2, 3, 4) share the face (1, 2, 3); vertex 4 is `e`
_UNIT = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]          # circumsphere: centre (1/2, 1/2, 1/2), radius^2 3/4
HAND = {
    # name: (points, cells, state of the one interior face, counters)
    "inside": (_UNIT + [[0.9, 0.9, 0.9]], [[0, 1, 2, 3], [1, 2, 3, 4]], 2, [1, 1, 0, 0]),
    "outside": (_UNIT + [[1.1, 1.1, 1.1]], [[0, 1, 2, 3], [1, 2, 3, 4]], 1, [1, 0, 0, 0]),
    "on_sphere": (_UNIT + [[1, 1, 1]], [[0, 1, 2, 3], [1, 2, 3, 4]], 3, [1, 0, 1, 0]),        # integer cube corners: exactly 0
    # t0 with two corners exchanged: negative orientation as stored, the same verdicts, and the inverted counter on a violation
    "inside_negative": (_UNIT + [[0.9, 0.9, 0.9]], [[1, 0, 2, 3], [1, 2, 3, 4]], 2, [1, 1, 0, 1]),
    "outside_negative": (_UNIT + [[1.1, 1.1, 1.1]], [[1, 0, 2, 3], [1, 2, 3, 4]], 1, [1, 0, 0, 0]),
    "one_tet": (_UNIT, [[0, 1, 2, 3]], None, [0, 0, 0, 0]),
}


def hand(name):
    pts, cells, state, counters = HAND[name]
    return np.asarray(pts, np.float32), np.asarray(cells, np.int32), state, counters


def case(scenes, name):
    """(points, cells, face_tets uint32 [F, 2] by face_tets_of) of a mesh or a hand-made case, made once"""
    if ("case", name) not in _CACHE:
        pts, cells = hand(name)[:2] if name in HAND else mesh(scenes, name)
        _CACHE["case", name] = (pts, cells, face_tets_of(cells))
    return _CACHE["case", name]


def statement(scenes, name, face_tets=None):
    """the numpy statement's answer on `case(name)` (on `face_tets` if given: a tracer's table), made once -- do not write into it"""
    key = ("statement", name, None if face_tets is None else face_tets.tobytes())
    if key not in _CACHE:
        pts, cells, ft = case(scenes, name)
        _CACHE[key] = geometry().delaunay_face_statement(cells, ft if face_tets is None else face_tets, pts)
    return _CACHE[key]


# ---- exact arithmetic on the fp32 values
def _det(rows):
    """determinant of a small square matrix of Fractions by cofactor expansion along the first row"""
    if len(rows) == 1:
        return rows[0][0]
    total = Fraction(0)
    for j, a in enumerate(rows[0]):
        if a:
            minor = [r[:j] + r[j + 1:] for r in rows[1:]]
            total += (-1) ** j * a * _det(minor)
    return total


def exact_signs(p, e):
    """(sign of the in-sphere determinant translated by e, sign of the orientation determinant translated by p3) of one face in
    exact rational arithmetic: p float32 [4, 3], e float32 [3]"""
    P = [[Fraction(float(x)) for x in row] for row in p]
    E = [Fraction(float(x)) for x in e]
    ins = []
    for row in P:
        d = [row[a] - E[a] for a in range(3)]
        ins.append(d + [d[0] * d[0] + d[1] * d[1] + d[2] * d[2]])
    ori = [[P[k][a] - P[3][a] for a in range(3)] for k in range(3)]
    sign = lambda x: (x > 0) - (x < 0)   # noqa: E731
    return sign(_det(ins)), sign(_det(ori))


# ---- the transfer
def occupancy_like(T, seed):
    """float32 [T] >= 0 with two thirds exact zeros, as an occupancy field under a threshold looks"""
    rng = np.random.default_rng(seed)
    v = rng.random(T).astype(np.float32)
    v[rng.random(T) < 0.66] = 0.0
    return v


def remap_brute_force(old_cells, new_cells, values, num_vertices):
    """the transfer as two plain loops over floats (non-negative inputs only)"""
    star = [0.0] * num_vertices
    for c, v in zip(np.asarray(old_cells).tolist(), np.asarray(values).tolist()):
        for k in c:
            if k < num_vertices:
                star[k] = max(star[k], v)
    out = [max([star[k] for k in c if k < num_vertices] + [0.0]) for c in np.asarray(new_cells).tolist()]
    return np.asarray(out, np.float32), np.asarray(star, np.float32)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)
