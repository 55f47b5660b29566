"""The meshes, dead masks and soups every test of vertex pruning uses (tests/test_prune.py, tests/test_prune_gpu.py), stated once,
with the numpy statement's answers (geometry.prune_vertices_statement) computed once per session and never modified.  Nothing
here needs a GPU or the library; the face tables of the meshes come from the oracle (oracle.build_faces).

A case is (xyz float32 [V, 3], cells int32 [T, 4], dead uint8 [T], faces int32 [F, 3], face_tets int32 [F, 2], vertex_select
uint8 [V] or None).  The groups: MESHES -- Delaunay meshes with a ball of dead tetrahedra or all of them dead, and the removal
count the statement gives for each (REMOVED, asserted) --; and SOUPS -- random ids at every wave, block and grid-cap edge of V,
T and F (the constants are read from the .hip source), no tetrahedra, every vertex removed, a vertex selection, ids >= V."""
import importlib
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_CACHE = {}
EMPTY = 0xFFFFFFFF
ARRAYS = ("vertices", "new_id", "kept_ids", "offsets", "counters")


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def kernel_constants():
    """(threads per block, grid cap in blocks) of tn_prune.hip, read from its source"""
    text = (ROOT / "tetra-nerf_amd" / "csrc" / "tn_prune.hip").read_text()
    bt = int(re.search(r"constexpr int BT = (\d+);", text).group(1))
    blocks = int(re.search(r"constexpr unsigned PRUNE_BLOCKS = (\d+);", text).group(1))
    return bt, blocks


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def face_table(cells):
    """(faces int32 [F, 3], face_tets int32 [F, 2]) of the oracle: first-seen order, -1 = no second tetrahedron"""
    from oracle import tn_oracle

    tn_oracle.build()
    faces, face_tets = tn_oracle.build_faces(np.ascontiguousarray(cells, np.int32).reshape(-1, 4))
    return np.ascontiguousarray(faces.view(np.int32)), np.ascontiguousarray(face_tets.view(np.int32))


def ball(xyz, cells, radius, centre=0.5):
    """uint8 [T]: the tetrahedra whose centroid (float64 mean of the fp32 corners) lies within `radius` of the centre"""
    centroid = np.asarray(xyz, np.float64)[np.asarray(cells, np.int64)].mean(1)
    return (np.linalg.norm(centroid - centre, axis=1) < radius).astype(np.uint8)


def _mesh(scenes, which):
    return {"rand600_41": lambda: scenes.random_mesh(600, 41), "rand1500_31": lambda: scenes.random_mesh(1500, 31),
            "grid6": lambda: scenes.grid_mesh(6), "grid6j": lambda: scenes.grid_mesh(6, 0.1),
            "rand600_3": lambda: scenes.random_mesh(600, 3)}[which]()


# name -> (mesh, dead: a ball radius or "all")
MESHES = {
    "rand600_41_b025": ("rand600_41", 0.25), "rand600_41_b035": ("rand600_41", 0.35), "rand1500_31_b030": ("rand1500_31", 0.30),
    "grid6_all": ("grid6", "all"), "grid6j_all": ("grid6j", "all"), "rand600_all": ("rand600_3", "all"),
}
REMOVED = {"rand600_41_b025": 13, "rand600_41_b035": 46, "rand1500_31_b030": 76, "grid6_all": 64, "grid6j_all": 168, "rand600_all": 535}
GENERAL_POSITION = ("rand600_41_b025", "rand600_41_b035", "rand1500_31_b030", "grid6j_all", "rand600_all")


def soup_sizes():
    bt, blocks = kernel_constants()
    return (1, bt - 1, bt, bt + 1, bt * blocks + 1)


def _random_soup(V, T, F, seed, past_V=False):
    """random ids in [0, V), 80 % of the tetrahedra dead, 5 % of the faces on the hull; past_V: some ids >= V in both tables"""
    rng = np.random.default_rng(seed)
    xyz = rng.random((V, 3)).astype(np.float32)
    cells = rng.integers(0, V, (T, 4)).astype(np.int64)
    faces = rng.integers(0, V, (F, 3)).astype(np.int64)
    face_tets = np.stack([rng.integers(0, max(T, 1), F), np.where(rng.random(F) < 0.05, EMPTY, rng.integers(0, max(T, 1), F))], 1)
    if past_V:
        cells[rng.random((T, 4)) < 0.02] = V
        cells[rng.random((T, 4)) < 0.02] = EMPTY
        faces[rng.random((F, 3)) < 0.05] = V + 7
        faces[rng.random((F, 3)) < 0.05] = EMPTY
    dead = (rng.random(T) < 0.8).astype(np.uint8)
    i32 = lambda a: np.ascontiguousarray(a.astype(np.uint32).view(np.int32))   # noqa: E731
    return xyz, i32(cells), dead, i32(faces), i32(face_tets), None


def _all_removed():
    """every vertex named, every tetrahedron dead, no hull face: V' = 0"""
    V, T = 257, 300
    rng = np.random.default_rng(4)
    cells = np.concatenate([np.arange(V), rng.integers(0, V, 4 * T - V)]).reshape(T, 4).astype(np.int32)
    faces = rng.integers(0, V, (50, 3)).astype(np.int32)
    face_tets = rng.integers(0, T, (50, 2)).astype(np.int32)
    return rng.random((V, 3)).astype(np.float32), cells, np.ones(T, np.uint8), faces, face_tets, None


def _with_select():
    xyz, cells, dead, faces, face_tets, _ = _random_soup(1000, 700, 400, 12)
    return xyz, cells, dead, faces, face_tets, (np.random.default_rng(13).random(1000) < 0.5).astype(np.uint8)


def _no_tets():
    xyz, _, _, faces, face_tets, _ = _random_soup(300, 1, 20, 14)
    return xyz, np.zeros((0, 4), np.int32), np.zeros(0, np.uint8), faces, face_tets, None


SPECIAL = {"soup_no_tets": _no_tets, "soup_all_removed": _all_removed, "soup_select": _with_select,
           "soup_ids_past_V": lambda: _random_soup(600, 500, 300, 15, past_V=True)}


def names(soups=False):
    out = list(MESHES)
    if soups:
        out += [f"soup_{n}" for n in soup_sizes()] + list(SPECIAL)
    return out


def case(scenes, name):
    if name not in _CACHE:
        if name in MESHES:
            which, dead = MESHES[name]
            xyz, cells = _mesh(scenes, which)
            xyz, cells = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(cells, np.int32)
            mask = np.ones(len(cells), np.uint8) if dead == "all" else ball(xyz, cells, dead)
            c = (xyz, cells, mask, *face_table(cells), None)
        elif name in SPECIAL:
            c = SPECIAL[name]()
        else:
            n = int(name.split("_")[1])
            c = _random_soup(n, n, n, n)
        for a in c:
            if a is not None:
                a.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def statement(scenes, name):
    key = ("statement", name)
    if key not in _CACHE:
        _CACHE[key] = geometry().prune_vertices_statement(*case(scenes, name))
        for a in _CACHE[key].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _CACHE[key]


def values_for(V, rows, seed=0):
    """a per-vertex array f32 [rows, V]: N(0, 1)"""
    return np.random.default_rng(1000 * rows + seed).normal(size=(rows, V)).astype(np.float32)


def vol6(p):
    """signed ((p1-p0) x (p2-p0)) . (p3-p0) of p float64 [n, 4, 3]"""
    return np.einsum("ni,ni->n", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])


def hull_position_triples(xyz, cells):
    """the set of hull faces of a mesh, each as the sorted triple of its three corner positions (float32 bit patterns)"""
    f = np.concatenate([cells[:, [1, 2, 3]], cells[:, [0, 2, 3]], cells[:, [0, 1, 3]], cells[:, [0, 1, 2]]]).astype(np.int64)
    s = np.sort(f, 1)
    u, n = np.unique(s, axis=0, return_counts=True)
    hull = u[n == 1]
    pos = np.ascontiguousarray(xyz, np.float32).view(np.uint32)[hull]                    # [h, 3, 3]
    return {tuple(sorted(map(tuple, p.tolist()))) for p in pos}
