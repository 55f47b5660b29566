"""The cases of the face-table tests (tests/test_face_table.py on the CPU, tests/test_face_table_gpu.py on the GPU), and the numpy
statement's answers (geometry.face_table_statement / face_sightings_statement) computed once per session and never modified.
Nothing here needs a GPU.

A case is (cells int32 [T, 4], V).  A prefix of a Delaunay mesh's rows is a valid soup: no face is in more than two rows."""
import importlib

import numpy as np

import flip_cases as fc

EMPTY = 0xFFFFFFFF
ARRAYS = ("partner", "face_index", "counters", "faces", "face_tets", "tet_faces")
FLAG_CELL_OOB, FLAG_TRIPLE_FACE = 1, 2
_CACHE = {}

# T at which the 4T sightings cross a wave (64) and a block (256), 8T + 16 crosses a power of two (the hash doubles: 8 * 30 + 16 =
# 256), 4T crosses 1024 blocks of 256 (65,536) -- whether or not a launcher caps its grid
PREFIXES = (1, 2, 15, 16, 17, 30, 31, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537)
BIG_MESH = {"points": 10500, "seed": 5}     # scenes.random_mesh: more than 65,537 rows


def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def big_mesh():
    if "big" not in _CACHE:
        scenes = importlib.import_module("tetra-nerf_amd.scenes")
        xyz, cells = scenes.random_mesh(BIG_MESH["points"], BIG_MESH["seed"])
        cells = np.ascontiguousarray(cells, np.int32)
        assert len(cells) > PREFIXES[-1], len(cells)
        cells.setflags(write=False)
        _CACHE["big"] = (len(xyz), cells)
    return _CACHE["big"]


def _rows(*rows):
    return np.array(rows, np.int32).reshape(-1, 4)


FIXED = {
    "no_rows": lambda: (_rows(), 4),
    "one_row": lambda: (_rows((0, 1, 2, 3)), 4),
    "two_rows_one_face": lambda: (_rows((0, 1, 2, 3), (1, 2, 3, 4)), 5),
    "moved_400": lambda: (fc.moved_mesh()[1], len(fc.moved_mesh()[0])),
    "triple_face": lambda: (_rows((0, 1, 2, 3), (0, 1, 2, 4), (5, 2, 1, 0), (6, 7, 8, 9)), 10),
    "repeated_id": lambda: (_rows((0, 0, 1, 2), (4, 5, 6, 7)), 8),
    "id_past_V": lambda: (_rows((0, 1, 2, 3), (1, 2, 3, 9), (1, 2, 9, -1)), 9),
    "identical_rows": lambda: (_rows((0, 1, 2, 3), (0, 1, 2, 3), (4, 5, 6, 7)), 8),
}


def names(prefixes=False, big=True):
    return list(FIXED) + ([f"prefix_{n}" for n in PREFIXES if big or n < 1000] if prefixes else [])


def case(name):
    if name not in _CACHE:
        if name.startswith("prefix_"):
            V, cells = big_mesh()
            c = (cells[:int(name.split("_")[1])], V)
        else:
            c = FIXED[name]()
        cells = np.ascontiguousarray(c[0], np.int32).reshape(-1, 4)
        cells.setflags(write=False)
        _CACHE[name] = (cells, int(c[1]))
    return _CACHE[name]


def statement(name):
    """{"partner", "face_index", "counters", "faces", "face_tets", "tet_faces"} uint32, of geometry's two statements"""
    key = ("statement", name)
    if key not in _CACHE:
        cells, V = case(name)
        g = geometry()
        _, partner, face_index, _ = g.face_sightings_statement(cells)
        faces, face_tets, tet_faces, counters = g.face_table_statement(cells, V)
        out = {"partner": partner, "face_index": face_index, "counters": counters, "faces": faces, "face_tets": face_tets,
               "tet_faces": tet_faces}
        for a in out.values():
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def table_of(cells):
    """(faces int32 [F, 3], face_tets int32 [F, 2]) by the statement: what flip_to_delaunay_statement takes as face_table"""
    faces, face_tets, _, counters = geometry().face_table_statement(cells)
    assert int(counters[2]) == 0
    return faces.view(np.int32), face_tets.view(np.int32)


def repaired():
    """geometry.flip_to_delaunay_statement on flip_cases.moved_mesh() with the statement's tables, once per session"""
    if "repaired" not in _CACHE:
        xyz, cells = fc.moved_mesh()
        _CACHE["repaired"] = geometry().flip_to_delaunay_statement(xyz, cells, table_of)
    return _CACHE["repaired"]
