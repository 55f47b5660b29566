"""The face table of any cell rows on the CPU: the rule as the numpy statement
(geometry.face_table_statement), as the oracle's and the host build's first-seen tables, and as the host emulation of the two
entries (tests/host/face_table_emul.cpp: the element functions of csrc/tn_build_core.h in a loop, sightings visited in ascending
and in a shuffled order) -- all equal on every case of tests/face_table_cases.py --, the structure of the table, the face count
after a round of flips, the flip loop on the statement's tables, and the declarations of the new entries."""
import ctypes
import importlib
import os
import re
import shutil
import struct
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import face_table_cases as ftc
import flip_cases as fc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"
EMPTY = ftc.EMPTY


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None or not Path("/opt/rocm/include/hip/hip_runtime.h").exists():
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path_factory.mktemp("host") / "face_table_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "face_table_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, cells, V):
    T = len(cells)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQ", V, T))
        f.write(np.ascontiguousarray(cells, np.int32).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    out = {"counters": np.frombuffer(raw, np.uint32, 4)}
    F, at = int(out["counters"][0]), 16
    for key, shape in (("partner", (4 * T,)), ("face_index", (4 * T + 1,)), ("faces", (F, 3)), ("face_tets", (F, 2)), ("tet_faces", (T, 4))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, np.uint32, count, at).reshape(shape)
        at += 4 * count
    assert at == len(raw)
    return out


def assert_equal(got, want, what):
    keys = ("counters",) if int(want["counters"][2]) & ftc.FLAG_TRIPLE_FACE else ftc.ARRAYS      # a triple face: the flag and the counts
    for key in keys:
        assert got[key].shape == want[key].shape, f"{what}: {key} {got[key].shape} vs {want[key].shape}"
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), f"{what}: {key}"


@pytest.mark.parametrize("name", ftc.names(prefixes=True))
def test_emulated_entries_equal_the_statement_in_both_schedules(emul, tmp_path, name):
    assert_equal(_run_emul(emul, tmp_path, *ftc.case(name)), ftc.statement(name), name)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: no rows, a triple
    face, a repeated id, ids past V (0xFFFFFFFF among them), identical rows, the sizes around the doubling of the hash"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ftc.names() + ["prefix_1", "prefix_30", "prefix_31", "prefix_257"]:
        assert_equal(_run_emul(exe, tmp_path, *ftc.case(name)), ftc.statement(name), name)


# ------------------------------------------------------------------------------------------------ what the cases are named for
EXPECTED = {   # F, hull faces, flags
    "no_rows": [0, 0, 0],
    "one_row": [4, 4, 0],
    "two_rows_one_face": [7, 6, 0],
    "triple_face": [15, 14, ftc.FLAG_TRIPLE_FACE],
    "repeated_id": [7, 6, 0],                      # (0, 0, 1, 2): its local faces 0 and 1 are both {0, 1, 2} and pair up
    "id_past_V": [10, 8, ftc.FLAG_CELL_OOB],
    "identical_rows": [8, 4, 0],
}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_the_cases_are_what_they_are_named_for(name):
    assert ftc.statement(name)["counters"].tolist() == EXPECTED[name] + [0]


def test_the_hand_made_tables():
    s = ftc.statement("two_rows_one_face")
    # faces in order of first sighting 4 t + j, ids as face_of_tet orders them: local face j = ids (j + 1) & 3, (j + 2) & 3, (j + 3) & 3
    assert s["faces"].tolist() == [[1, 2, 3], [2, 3, 0], [3, 0, 1], [0, 1, 2], [2, 3, 4], [3, 4, 1], [4, 1, 2]]
    assert s["face_tets"].tolist() == [[0, 1], [0, EMPTY], [0, EMPTY], [0, EMPTY], [1, EMPTY], [1, EMPTY], [1, EMPTY]]
    assert s["tet_faces"].tolist() == [[0, 1, 2, 3], [4, 5, 6, 0]]
    assert s["partner"].tolist() == [7, EMPTY, EMPTY, EMPTY, EMPTY, EMPTY, EMPTY, 0]
    assert s["face_index"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7]
    s = ftc.statement("repeated_id")               # a row that repeats an id pairs its own sightings by the same rule
    assert s["partner"][:4].tolist() == [1, 0, EMPTY, EMPTY] and s["tet_faces"][0].tolist() == [0, 0, 1, 2]
    assert s["face_tets"][0].tolist() == [0, 0]
    s = ftc.statement("identical_rows")
    assert s["partner"][:8].tolist() == [4, 5, 6, 7, 0, 1, 2, 3] and s["face_tets"][:4].tolist() == [[0, 1]] * 4
    s = ftc.statement("no_rows")
    assert s["faces"].shape == (0, 3) and s["face_tets"].shape == (0, 2) and s["tet_faces"].shape == (0, 4) and s["face_index"].tolist() == [0]
    # without V no id is out of bounds
    assert ftc.geometry().face_table_statement(ftc.case("id_past_V")[0])[3].tolist() == [10, 8, 0, 0]


# ------------------------------------------------------------------------------------------------- the other first-seen tables
@pytest.mark.parametrize("mesh", ["cube", "bottle", "moved_400", "prefix_257"])
def test_statement_equals_the_oracle(oracle, scenes, bottle, mesh):
    cells = scenes.cube_mesh()[1] if mesh == "cube" else bottle["cells"] if mesh == "bottle" else ftc.case(mesh)[0]
    faces, face_tets, _, counters = ftc.geometry().face_table_statement(cells)
    want_faces, want_ft = oracle.build_faces(cells)
    assert faces.dtype == want_faces.dtype and np.array_equal(faces, want_faces) and np.array_equal(face_tets, want_ft)
    assert counters.tolist() == [len(want_faces), int((want_ft[:, 1] == EMPTY).sum()), 0, 0]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """the g++ route of tests/test_host_build.py: csrc/tn_mesh.cpp behind tests/host/host_build_check.cpp"""
    if shutil.which("g++") is None or not Path("/opt/rocm/include/hip/hip_runtime.h").exists():
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path_factory.mktemp("host") / "host_build_check"
    cmd = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "host_build_check.cpp"), str(CSRC / "tn_mesh.cpp")]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


def _host_table(exe, tmp_path, pts, cells):
    mesh, out = tmp_path / "mesh.bin", tmp_path / "faces.bin"
    with open(mesh, "wb") as f:
        f.write(struct.pack("<QQ", len(pts), len(cells)))
        f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        f.write(np.ascontiguousarray(cells).astype(np.uint32).tobytes())
    r = subprocess.run([str(exe), str(mesh), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = out.read_bytes()
    F = struct.unpack("<Q", raw[:8])[0]
    return np.frombuffer(raw, np.uint32, 3 * F, 8).reshape(F, 3), np.frombuffer(raw, np.uint32, 2 * F, 8 + 12 * F).reshape(F, 2)


@pytest.mark.parametrize("mesh", ["cube", "bottle", "moved_400"])
def test_statement_equals_the_host_build(host_check, tmp_path, scenes, bottle, mesh):
    if mesh == "cube":
        pts, cells = scenes.cube_mesh()
    elif mesh == "bottle":
        pts, cells = bottle["vertices"], bottle["cells"]
    else:
        pts, cells = fc.moved_mesh()
    faces, face_tets = _host_table(host_check, tmp_path, pts, cells)
    got = ftc.geometry().face_table_statement(cells)
    assert np.array_equal(got[0], faces) and np.array_equal(got[1], face_tets)


# ------------------------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("name", [n for n in ftc.names(prefixes=True) if n != "triple_face"])
def test_table_structure(name):
    cells, _ = ftc.case(name)
    s = ftc.statement(name)
    c = np.where(cells < 0, cells.astype(np.int64) + (1 << 32), cells.astype(np.int64))
    T, F = len(c), len(s["faces"])
    faces, ft, tf = s["faces"].astype(np.int64), s["face_tets"].astype(np.int64), s["tet_faces"].astype(np.int64)
    interior = ft[:, 1] != EMPTY
    # hull count + 2 * interior = 4T
    assert int(s["counters"][1]) == int((~interior).sum()) and int(s["counters"][1]) + 2 * int(interior.sum()) == 4 * T
    # every face names rows that hold its ids (as a multiset: rows that repeat an id)
    key = np.sort(faces, 1)
    for col in (0, 1):
        rows = np.flatnonzero(interior) if col else np.arange(F)
        held = c[ft[rows, col]]
        for f, row in zip(rows[:2000], held[:2000]):
            rest = list(row)
            for v in key[f]:
                assert v in rest, (name, f, col)
                rest.remove(v)
    # tet_faces inverts face_tets: face f is named by exactly the sightings of its rows, and the sighting's ids are the face's
    assert tf.shape == (T, 4) and (tf < F).all()
    j = np.arange(4)
    sight = np.sort(np.stack([c[:, (j + 1) & 3], c[:, (j + 2) & 3], c[:, (j + 3) & 3]], -1), -1)            # [T, 4, 3]
    assert np.array_equal(sight, key[tf])
    count = np.bincount(tf.reshape(-1), minlength=F)
    assert np.array_equal(count, np.where(interior, 2, 1))
    t_of = np.repeat(np.arange(T), 4)
    firsts = np.full(F, 4 * T, np.int64)
    np.minimum.at(firsts, tf.reshape(-1), np.arange(4 * T))
    assert np.array_equal(firsts >> 2, ft[:, 0]) and (np.diff(firsts) > 0).all()                             # ids rank the first sightings
    last = np.zeros(F, np.int64)
    np.maximum.at(last, tf.reshape(-1), np.arange(4 * T))
    assert np.array_equal((last >> 2)[interior], ft[interior, 1]) and t_of.size == 4 * T


def test_face_count_after_a_round_of_flips():
    """F' = F + 2 K23 - 2 K32: a 2-3 flip removes one face and adds three, a 3-2 flip removes three and adds one -- what lets the
    flip loop pass F' to tn_face_table_emit without a read-back"""
    g = ftc.geometry()
    xyz, cells = fc.moved_mesh()
    seen = 0
    for _ in range(4):
        faces, face_tets = ftc.table_of(cells)
        out = g.flip_faces_statement(xyz, cells, faces, face_tets)
        if out["num_23"] + out["num_32"] == 0:
            break
        after = g.face_table_statement(out["cells"])[3]
        assert int(after[2]) == 0 and int(after[0]) == len(faces) + 2 * out["num_23"] - 2 * out["num_32"]
        assert int(after[1]) == int((face_tets[:, 1] == -1).sum())                                           # flips keep the hull
        seen += out["num_23"] + out["num_32"]
        cells = out["cells"]
    assert seen > 100


def test_the_flip_loop_on_the_statements_tables_is_the_loop_on_the_host_builds(host_check, tmp_path):
    """flip_to_delaunay_statement driven by face_table_statement gives the same rounds as driven by the host build's tables"""
    xyz, cells = fc.moved_mesh()
    want = ftc.repaired()

    def host_tables(c):
        faces, face_tets = _host_table(host_check, tmp_path, xyz, c)
        return faces.view(np.int32), face_tets.view(np.int32)

    got = ftc.geometry().flip_to_delaunay_statement(xyz, cells, host_tables)
    assert got["num_rounds"] == want["num_rounds"] > 1 and [r.tolist() for r in got["rounds"]] == [r.tolist() for r in want["rounds"]]
    assert np.array_equal(got["cells"], want["cells"]) and np.array_equal(got["cell_sources"], want["cell_sources"])
    assert 100 * want["violated"] <= int(want["rounds"][0][1])


# ------------------------------------------------------------------------------------------------------------- the adapter
def test_adapter_passes_reload_only_when_configured():
    """config.delaunay_repair_reload = "once" reaches flip_to_delaunay as reload=; absent, the call has exactly the arguments it had
    (a stand-in that takes no other keyword)"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    cells = torch.zeros((3, 4), dtype=torch.int32)
    calls = []

    class _Tracer:
        supports_flip = True
        tetrahedra_vertices = torch.zeros((4, 3))
        tetrahedra_cells = cells

        def delaunay_check(self):
            return {"counters": torch.tensor([100, 9, 0, 0])}

        def flip_to_delaunay(self, xyz=None, tet_values=(), max_rounds=32):
            calls.append({})
            return {"num_rounds": 0, "violated": 0, "rounds": [[100, 0, 0, 0, 0, 0, 0, 0, 0, 0]], "cells": cells, "tet_values": []}

    class _Reloading(_Tracer):
        supports_face_table = True

        def flip_to_delaunay(self, xyz=None, tet_values=(), max_rounds=32, reload="round"):
            calls.append({"reload": reload})
            return {"num_rounds": 0, "violated": 0, "rounds": [[100, 0, 0, 0, 0, 0, 0, 0, 0, 0]], "cells": cells, "tet_values": []}

    def model(**config):
        return types.SimpleNamespace(config=types.SimpleNamespace(delaunay_repair="flip", **config), tetrahedra_cells=cells)

    assert plugin._monitor_delaunay(_Tracer(), model(), 0.05, False) is False and calls == [{}]
    del calls[:]
    assert plugin._monitor_delaunay(_Reloading(), model(delaunay_repair_reload="once"), 0.05, False) is False
    assert calls == [{"reload": "once"}]
    del calls[:]
    assert plugin._monitor_delaunay(_Reloading(), model(delaunay_repair_reload=None), 0.05, False) is False
    assert calls == [{"reload": "round"}]                                     # (the stand-in's own default: nothing was passed)
    with pytest.raises(ValueError, match="delaunay_repair_reload"):
        plugin._monitor_delaunay(_Reloading(), model(delaunay_repair_reload="never"), 0.05, False)
    with pytest.raises(RuntimeError, match="reload"):
        plugin._monitor_delaunay(_Tracer(), model(delaunay_repair_reload="once"), 0.05, False)


# -------------------------------------------------------------------------------------------------------------- the entries
def test_entries_are_declared_bound_and_exported():
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    binding = importlib.import_module("tetra-nerf_amd._lib")
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and binding.ABI_VERSION == 6
    for name in ("tn_face_table_count", "tn_face_table_emit"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in binding.SYMBOLS
    lib = binding.load()
    assert len(lib.tn_face_table_count.argtypes) == 8 and len(lib.tn_face_table_emit.argtypes) == 9
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert hasattr(ext, "face_table") and hasattr(ext, "flip_to_delaunay") and ext.TetrahedraTracer.supports_face_table is True
    g = ftc.geometry()
    assert (g.FACE_TABLE_FLAG_CELL_OOB, g.FACE_TABLE_FLAG_TRIPLE_FACE) == (ext.FACE_TABLE_FLAG_CELL_OOB, ext.FACE_TABLE_FLAG_TRIPLE_FACE) == (1, 2)
    core = (CSRC / "tn_build_core.h").read_text()
    assert re.search(r"FLAG_CELL_OOB = 1u", core) and re.search(r"FLAG_TRIPLE_FACE = 2u", core)


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, before a device is touched: these run without a GPU"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = ctypes.c_void_p(64)                        # never dereferenced: the calls below are refused first
    assert lib.tn_face_table_count(0, 4, 2 ** 30, x, x, x, x, None) != 0 and b"2^30" in lib.tn_last_error()
    for args in ((0, 4, 1, None, x, x, x), (0, 4, 1, x, None, x, x), (0, 4, 1, x, x, None, x), (0, 4, 1, x, x, x, None),
                 (0, 4, 0, None, None, None, x), (0, 4, 0, None, None, x, None)):
        assert lib.tn_face_table_count(*args, None) != 0 and b"null pointer" in lib.tn_last_error(), args
    assert lib.tn_face_table_emit(2 ** 30, x, x, x, 4, x, x, x, None) != 0 and b"2^30" in lib.tn_last_error()
    assert lib.tn_face_table_emit(1, x, x, x, 5, x, x, x, None) != 0 and b"num_faces" in lib.tn_last_error()
    for args in ((1, None, x, x, 4, x, x, x), (1, x, None, x, 4, x, x, x), (1, x, x, None, 4, x, x, x), (1, x, x, x, 4, None, x, x),
                 (1, x, x, x, 4, x, None, x)):
        assert lib.tn_face_table_emit(*args, None) != 0 and b"null pointer" in lib.tn_last_error(), args
    assert lib.tn_face_table_emit(0, None, None, None, 0, None, None, None, None) == 0         # no rows: nothing to do, nothing launched


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    cells = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.face_table(cells)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.flip_to_delaunay(torch.zeros((4, 3)), cells)
