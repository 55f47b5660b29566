"""Vertex pruning without a GPU (tn_prune_count / tn_prune_count_tables / tn_prune_emit / tn_prune_vertex_rows, csrc/tn_prune.hip;
the rule: DESIGN.md section 4.21).  Layers: tests/host/prune_emul.cpp -- which drives the element functions of
csrc/tn_prune_core.h, the bodies of the kernels -- byte for byte against the numpy statements on every case of
tests/prune_cases.py; the statement against a plain-loop restatement of the rule; what the rule promises (the counters add up, no
live and no hull vertex goes, each mesh case removes what the statement says and at least one vertex); the Delaunay cells of the
kept points (the convex hull and the volume unchanged); the occupancy carried through remap_tet_values; and the declarations and
refusals of the entries.  (The kernels themselves: tests/test_prune_gpu.py.)"""
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

import prune_cases as pc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"
ROWS = 3                                                                      # the per-vertex array the emulation carries


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "prune_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe), str(ROOT / "tests" / "host" / "prune_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def prune_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, cells, dead, faces, face_tets, select, values):
    V, T, F, rows = len(xyz), len(cells), len(faces), len(values)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQQQ", V, T, F, rows, select is not None))
        for a, dtype in ((xyz, np.float32), (cells, np.int32), (dead, np.uint8), (faces, np.int32), (face_tets, np.int32)):
            f.write(np.ascontiguousarray(a, dtype).tobytes())
        if select is not None:
            f.write(np.ascontiguousarray(select, np.uint8).tobytes())
        f.write(np.ascontiguousarray(values, np.float32).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    offsets = np.frombuffer(raw, np.uint32, V + 1)
    Vp, at, out = int(offsets[V]), 4 * (V + 1), {"offsets": offsets}
    for key, dtype, shape in (("counters", np.uint32, (5,)), ("new_id", np.int32, (V,)), ("kept_ids", np.int32, (Vp,)),
                              ("vertices", np.float32, (Vp, 3)), ("rows", np.float32, (rows, Vp)), ("rows_vm", np.float32, (Vp, rows))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += 4 * count
    assert at == len(raw)
    out["num_kept"] = Vp
    return out


def _check_emulation(exe, tmp_path, scenes, name):
    g = pc.geometry()
    c = pc.case(scenes, name)
    want = pc.statement(scenes, name)
    values = pc.values_for(len(c[0]), ROWS, seed=len(c[1]))
    got = _run_emul(exe, tmp_path, *c, values)
    assert got["num_kept"] == want["num_kept"], name
    for key in pc.ARRAYS:
        assert got[key].shape == want[key].shape and np.array_equal(pc.bits(got[key]), pc.bits(want[key])), (name, key)
    rows = g.prune_vertex_rows_statement(values, want["kept_ids"])
    assert np.array_equal(pc.bits(got["rows"]), pc.bits(rows)) and np.array_equal(pc.bits(got["rows_vm"]), pc.bits(np.ascontiguousarray(rows.T))), name
    return got


@pytest.mark.parametrize("name", pc.names(soups=True))
def test_emulated_kernels_equal_the_statement(prune_emul, tmp_path, scenes, name):
    got = _check_emulation(prune_emul, tmp_path, scenes, name)
    counters = got["counters"].tolist()
    assert counters[0] == sum(counters[1:]) and counters[1] == len(got["new_id"]) - got["num_kept"], (name, counters)
    if name == "soup_all_removed":
        assert got["num_kept"] == 0 and counters == [257, 257, 0, 0, 0]
    if name == "soup_no_tets":
        assert counters == [300, 0, 0, 0, 300]


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: ids past the table
    in cells and faces, no tetrahedra, every vertex removed, a selection"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ("soup_ids_past_V", "soup_no_tets", "soup_all_removed", "soup_select", "soup_1", "grid6_all"):
        _check_emulation(exe, tmp_path, scenes, name)


# --------------------------------------------------------------------------------------------------- the rule, restated
def _restate(xyz, cells, dead, faces, face_tets, select):
    """the rule as plain loops: the keep flag of every vertex and the five counters"""
    V = len(xyz)
    named, live, hull = [False] * V, [False] * V, [False] * V
    for row, d in zip(cells.view(np.uint32).tolist(), dead.tolist()):
        lives = not d or any(i >= V for i in row)
        for i in row:
            if i < V:
                named[i] = True
                live[i] = live[i] or lives
    for f, ft in zip(faces.view(np.uint32).tolist(), face_tets.view(np.uint32).tolist()):
        if ft[1] == pc.EMPTY:
            for i in f:
                if i < V:
                    hull[i] = True
    keep, n = [], [0] * 5
    for v in range(V):
        if select is not None and not select[v]:
            keep.append(True)
            continue
        n[0] += 1
        outcome = 2 if live[v] else 3 if hull[v] else 4 if not named[v] else 1
        n[outcome] += 1
        keep.append(outcome != 1)
    return np.array(keep, bool), n


@pytest.mark.parametrize("name", [n for n in pc.names(soups=True) if n != f"soup_{pc.soup_sizes()[-1]}"])
def test_statement_equals_a_restatement(scenes, name):
    c = pc.case(scenes, name)
    want = pc.statement(scenes, name)
    keep, counters = _restate(*c)
    assert np.array_equal(np.nonzero(keep)[0], want["kept_ids"]) and want["counters"].tolist() == counters, name
    assert np.array_equal(want["new_id"][keep], np.arange(keep.sum())) and (want["new_id"][~keep] == -1).all()
    assert np.array_equal(pc.bits(want["vertices"]), pc.bits(c[0][keep]))


def _hull_vertices(cells, V):
    """bool [V]: vertices of a face that only one tetrahedron has (computed from the cells, not from the face table)"""
    f = np.sort(np.concatenate([cells[:, [1, 2, 3]], cells[:, [0, 2, 3]], cells[:, [0, 1, 3]], cells[:, [0, 1, 2]]]), 1)
    u, n = np.unique(f, axis=0, return_counts=True)
    h = np.zeros(V, bool)
    h[u[n == 1].ravel()] = True
    return h


@pytest.mark.parametrize("name", list(pc.MESHES))
def test_counters_and_outcomes(scenes, name):
    xyz, cells, dead, faces, face_tets, _ = pc.case(scenes, name)
    s = pc.statement(scenes, name)
    V = len(xyz)
    counters = s["counters"].tolist()
    removed = np.setdiff1d(np.arange(V), s["kept_ids"])
    print(name, "counters", dict(zip(pc.geometry().PRUNE_COUNTER_NAMES, counters)))
    assert counters[0] == V == sum(counters[1:]) and counters[1] == s["num_removed"] == len(removed)
    assert s["num_removed"] == pc.REMOVED[name] >= 1                          # a rule that removes nothing cannot pass
    live = np.zeros(V, bool)
    live[cells[dead == 0].ravel()] = True
    assert not live[removed].any() and not _hull_vertices(cells, V)[removed].any()
    assert np.isin(removed, cells[dead != 0].ravel()).all()                   # every removed vertex was named, by dead tetrahedra only


# ------------------------------------------------------------------------------------------------------- cells and domain
_CELLS = {}


def _pruned_cells(scenes, name):
    if name not in _CELLS:
        _CELLS[name] = scenes.delaunay_cells(pc.statement(scenes, name)["vertices"])
    return _CELLS[name]


@pytest.mark.parametrize("name", list(pc.MESHES))
def test_pruned_mesh_keeps_the_domain(scenes, name):
    """The kept points' Delaunay cells cover what the loaded mesh covered.  Every hull-face vertex is kept and the loaded mesh
    triangulates the convex hull of its points, so the convex hull is unchanged.  Volume: sum |vol6| / 6 in float64 over both
    meshes agrees to 1e-12 relative -- each is the hull's volume up to the rounding of a few thousand float64 determinants at
    2^-53 each.  On the meshes in general position the hull faces, as position triples, are the same set before and after (the
    lattice's coplanar hull squares may be cut along either diagonal)."""
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    xyz, cells, *_ = pc.case(scenes, name)
    kept = pc.statement(scenes, name)["vertices"]
    new_cells = _pruned_cells(scenes, name)
    assert np.array_equal(ext.triangulate(torch.from_numpy(np.array(kept))).numpy(), new_cells)    # the wrapper the tracer calls
    vol = lambda x, c: float(np.abs(pc.vol6(x.astype(np.float64)[c.astype(np.int64)])).sum() / 6)   # noqa: E731
    before, after = vol(xyz, cells), vol(kept, new_cells)
    print(name, "V", len(xyz), "->", len(kept), "T", len(cells), "->", len(new_cells), "volume", before, after,
          "relative difference", abs(after - before) / before)
    assert abs(after - before) <= 1e-12 * before
    if name in pc.GENERAL_POSITION:
        assert pc.hull_position_triples(xyz, cells) == pc.hull_position_triples(kept, new_cells)


@pytest.mark.parametrize("name", ("rand600_41_b025", "rand600_41_b035", "rand1500_31_b030"))
def test_occupancy_is_carried_by_the_old_ids(scenes, name):
    """The occupancy of the pruned mesh is remap_tet_values_statement(old cells, kept_ids[new cells]): every new tetrahedron
    takes the largest value of any old tetrahedron around any of its four vertices -- conservative.  Checked against a plain loop
    over the old cells, and the statement's torch form against its numpy form."""
    g = pc.geometry()
    xyz, cells, dead, *_ = pc.case(scenes, name)
    s = pc.statement(scenes, name)
    V = len(xyz)
    occ = np.where(dead != 0, 0, np.random.default_rng(3).random(len(cells))).astype(np.float32)
    in_old = s["kept_ids"][_pruned_cells(scenes, name)]
    got = g.remap_tet_values_statement(cells, in_old, occ, V)["values"]
    star = np.zeros(V, np.float32)
    for row, value in zip(cells.tolist(), occ.tolist()):
        for v in row:
            star[v] = max(star[v], value)
    assert np.array_equal(got, star[in_old].max(1))
    t = g.remap_tet_values_statement(torch.from_numpy(np.array(cells)), torch.from_numpy(np.array(in_old)), torch.from_numpy(occ), V)["values"]
    assert np.array_equal(pc.bits(t.numpy()), pc.bits(got))
    assert got.max() == occ.max() > 0                                         # the most occupied tetrahedron is live: its vertices stay


def test_vertex_rows_statement():
    g = pc.geometry()
    values = pc.values_for(9, 3)
    ids = np.array([0, 2, 8, 9], np.int32)                                    # an id >= V: 0
    got = g.prune_vertex_rows_statement(values, ids)
    assert np.array_equal(got[:, :3], values[:, [0, 2, 8]]) and not got[:, 3].any()
    assert g.prune_vertex_rows_statement(values, np.zeros(0, np.int32)).shape == (3, 0)
    with pytest.raises(ValueError, match="rows"):
        g.prune_vertex_rows_statement(np.zeros((0, 4), np.float32), ids)
    with pytest.raises(ValueError, match="one entry per row"):
        g.prune_vertices_statement(np.zeros((4, 3), np.float32), np.zeros((2, 4), np.int32), np.zeros(3, np.uint8),
                                   np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int32))


def test_the_cases_are_what_they_are_named_for(scenes):
    bt, blocks = pc.kernel_constants()
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.PRUNE_GRID_LANES == bt * blocks and ext.TetrahedraTracer.supports_prune is True
    assert set(pc.soup_sizes()) == {1, bt - 1, bt, bt + 1, bt * blocks + 1}
    for n in pc.soup_sizes():
        xyz, cells, dead, faces, face_tets, _ = pc.case(scenes, f"soup_{n}")
        assert len(xyz) == len(cells) == len(faces) == n
    xyz, cells, *_ = pc.case(scenes, "soup_ids_past_V")
    assert (cells.view(np.uint32) == len(xyz)).any() and (cells == -1).any()
    assert pc.statement(scenes, "soup_select")["counters"][0] < len(pc.case(scenes, "soup_select")[0])
    assert len(pc.case(scenes, "soup_no_tets")[1]) == 0 and pc.statement(scenes, "soup_all_removed")["num_kept"] == 0


# ---------------------------------------------------------------------------------------------------------------- entries
def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_prune_count\(tn_tracer_t tracer, size_t num_vertices, const uint8_t \*dead, const uint8_t \*vertex_select,"
                     r"\s*uint32_t \*offsets,\s*uint32_t \*counters, void \*stream\);", header)
    assert re.search(r"int\s+tn_prune_count_tables\(int device, size_t num_vertices, size_t num_cells, const uint32_t \*cells,\s*"
                     r"size_t num_faces,\s*const uint32_t \*faces, const uint32_t \*face_tets, const uint8_t \*dead,\s*"
                     r"const uint8_t \*vertex_select,\s*uint32_t \*offsets, uint32_t \*counters, void \*stream\);", header)
    assert re.search(r"int\s+tn_prune_emit\(size_t num_vertices, const float \*xyz, const uint32_t \*offsets, size_t num_kept,\s*"
                     r"uint32_t \*new_id,\s*uint32_t \*kept_ids, float \*xyz_out, void \*stream\);", header)
    assert re.search(r"int\s+tn_prune_vertex_rows\(size_t rows, size_t num_vertices, size_t num_kept, const float \*values,\s*"
                     r"const float \*values_vm,\s*const uint32_t \*kept_ids, float \*out, float \*out_vm, void \*stream\);", header)
    assert "no reference counterpart" in header[header.index("Vertex pruning"):header.index("int tn_prune_count(")]
    lib = _lib.load()
    names = ("tn_prune_count", "tn_prune_count_tables", "tn_prune_emit", "tn_prune_vertex_rows")
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert [len(getattr(lib, n).argtypes) for n in names] == [7, 12, 8, 9]
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    for name in ("prune_vertices", "prune_vertex_rows"):
        assert hasattr(ext, name)
    assert hasattr(ext.TetrahedraTracer, "remove_vertices") and hasattr(ext.TetrahedraTracer, "prune_count")
    assert hasattr(importlib.import_module("tetra-nerf_amd.nerfstudio_plugin"), "prune")


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = 64                                                                    # a pointer that is never followed

    assert lib.tn_prune_count(None, 5, x, None, x, x, None) != 0

    def count(V=5, T=2, cells=x, F=3, faces=x, face_tets=x, dead=x, offsets=x, counters=x):
        return lib.tn_prune_count_tables(0, V, T, cells, F, faces, face_tets, dead, None, offsets, counters, None)

    for kw in (dict(cells=None), dict(dead=None), dict(faces=None), dict(face_tets=None), dict(offsets=None), dict(counters=None)):
        assert count(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert count(T=2 ** 30) != 0 and b"2^30" in lib.tn_last_error()
    assert count(V=2 ** 32 - 1) != 0 and b"vertices" in lib.tn_last_error()

    def emit(V=5, xyz=x, offsets=x, K=4, new_id=x, kept=x, out=x):
        return lib.tn_prune_emit(V, xyz, offsets, K, new_id, kept, out, None)

    for kw in (dict(xyz=None), dict(offsets=None), dict(new_id=None), dict(kept=None), dict(out=None)):
        assert emit(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert emit(K=6) != 0 and b"exceeds" in lib.tn_last_error()

    def rows(n=64, V=5, K=4, values=x, vm=None, kept=x, out=x, out_vm=None):
        return lib.tn_prune_vertex_rows(n, V, K, values, vm, kept, out, out_vm, None)

    assert rows(n=0) != 0 and b"rows" in lib.tn_last_error()
    assert rows(K=6) != 0 and b"exceeds" in lib.tn_last_error()
    for kw in (dict(values=None), dict(kept=None), dict(out=None)):
        assert rows(**kw) != 0 and b"null" in lib.tn_last_error(), kw


def test_wrappers_refuse_host_tensors(scenes):
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    xyz, cells, dead, faces, face_tets, _ = (None if a is None else torch.from_numpy(np.array(a)) for a in pc.case(scenes, "grid6_all"))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.prune_vertices(xyz, cells, dead, faces, face_tets)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.prune_vertex_rows(torch.zeros(3, 9), torch.zeros(2, dtype=torch.int32))


def test_plugin_prune_needs_a_condition():
    """dead=None and no condition: ValueError before anything runs (a stand-in model whose tracer holds host tensors)"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    tracer = types.SimpleNamespace(supports_prune=True, tetrahedra_cells=torch.zeros(6, 4, dtype=torch.int32), device=torch.device("cpu"))
    model = types.SimpleNamespace(get_tetrahedra_tracer=lambda: tracer, tetrahedra_field=torch.zeros(64, 9),
                                  tetrahedra_vertices=torch.zeros(9, 3))
    with pytest.raises(ValueError, match="give `dead`"):
        plugin.prune(model)
    with pytest.raises(ValueError, match="occupancy_below needs"):
        plugin.prune(model, occupancy_below=0.1)
    with pytest.raises(ValueError, match="stats must be"):
        plugin.prune(model, stats=torch.zeros(5, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="one entry per tetrahedron"):
        plugin.prune(model, torch.ones(5, dtype=torch.bool))
