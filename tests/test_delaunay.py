"""The Delaunay monitor and the per-tetrahedron state transfer without a GPU (tn_delaunay_check / tn_remap_tet_values,
csrc/tn_delaunay.hip; the predicate and its bound: DESIGN.md section 4.16).  Four layers: the numpy statement against exact
rational arithmetic on the fp32 values (every certain state is the exact sign, every exact zero is uncertain), the hand-made
two-tetrahedron meshes of tests/delaunay_cases.py, tests/host/delaunay_emul.cpp -- which drives the element functions of
csrc/tn_delaunay_core.h, the bodies of the kernels -- bit for bit against the statement, and the transfer against two plain
loops and its conservative property on a re-triangulated mesh.  Then the entries' declarations and the adapter's call order on
a tracer that only records calls.  (The kernels themselves: tests/test_delaunay_gpu.py.)"""
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

import delaunay_cases as dc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"


# ----------------------------------------------------------------------------------------------------------------- statement
def test_sign_convention_on_the_unit_tetrahedron():
    """e = (0.3, 0.3, 0.3) is inside the circumsphere of the unit tetrahedron: the two determinants have the same sign there,
    whichever way the tetrahedron is stored; the orientation determinant has the opposite sign of tet_orient"""
    g = dc.geometry()
    unit = np.asarray(dc._UNIT, np.float64)
    e = np.asarray([[0.3, 0.3, 0.3]], np.float32).astype(np.float64)
    for order in ([0, 1, 2, 3], [1, 0, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        p = unit[order][None]
        ins, ori = g.insphere_det(p, e)[0][0], g.orient_det(p)[0][0]
        assert ins * ori > 0, order
        assert np.sign(ori) == -int(g.tet_orient(torch.from_numpy(unit[order]), torch.tensor([[0, 1, 2, 3]]))[0])
        far = np.asarray([[2.0, 2.0, 2.0]])
        assert g.insphere_det(p, far)[0][0] * ori < 0, order
    assert g.INSPHERE_BOUND == (16 + 224 * 2.0 ** -53) * 2.0 ** -53 and g.ORIENT_BOUND == (7 + 56 * 2.0 ** -53) * 2.0 ** -53


@pytest.mark.parametrize("name", ["random_400", "random_400_moved", "grid_5", "cube"])
def test_statement_against_exact_arithmetic(scenes, name):
    """every certain state equals the exact sign relation; every exactly-zero determinant is uncertain"""
    g = dc.geometry()
    pts, cells, ft = dc.case(scenes, name)
    s = dc.statement(scenes, name)
    interior, t0, _, e = g.delaunay_faces(cells, ft)
    state = s["face_state"][interior]
    counters = s["counters"].tolist()
    print(name, "tets", len(cells), "faces", len(ft), "interior, violated, uncertain, inverted", counters,
          "hull", int((~interior).sum()))
    assert counters[0] == interior.sum() == len(state) and np.all(s["face_state"][~interior] == 0)
    assert counters[1] == (state == 2).sum() and counters[2] == (state == 3).sum() and np.all(state >= 1)
    assert len(ft) - counters[0] > 0                                          # every mesh has a hull
    wrong = zeros = 0
    for i in range(len(state)):
        si, so = dc.exact_signs(pts[cells[t0[i]]], pts[e[i]])
        if si == 0 or so == 0:
            zeros += 1
            assert state[i] == 3, (i, "an exactly-zero determinant must be uncertain")
        elif state[i] != 3:
            wrong += state[i] != (2 if si == so else 1)
    print(name, "exact zeros", zeros, "certain states that differ from the exact sign", wrong)
    assert wrong == 0
    per_tet = np.zeros(len(cells), np.int64)
    for i in np.nonzero(interior)[0][state == 2]:
        per_tet[ft[i].astype(np.int64)] += 1
    np.testing.assert_array_equal(s["tet_violations"], per_tet)
    assert s["tet_violations"].dtype == np.uint8 and s["face_state"].dtype == np.int8 and per_tet.max() <= 4


def test_what_the_meshes_are_there_for(scenes):
    """general-position Delaunay cells: nothing violated, nothing uncertain; the same cells on the moved vertices: violations;
    the lattice: cospherical corners, most faces uncertain"""
    built, moved, grid = (dc.statement(scenes, n)["counters"].tolist() for n in ("random_400", "random_400_moved", "grid_5"))
    assert built[1] == 0 and built[2] == 0 and built[0] > 4000
    assert moved[1] > 0 and moved[0] == built[0]
    assert grid[1] == 0 and grid[2] > grid[0] // 2


@pytest.mark.parametrize("name", sorted(dc.HAND))
def test_hand_made_cases(name):
    g = dc.geometry()
    pts, cells, state, counters = dc.hand(name)
    ft = dc.face_tets_of(cells)
    s = g.delaunay_face_statement(cells, ft, pts)
    assert s["counters"].tolist() == counters
    interior = ft[:, 1] != dc.EMPTY
    if state is None:
        assert not interior.any() and np.all(s["face_state"] == 0) and s["tet_violations"].tolist() == [0]
        return
    assert interior.sum() == 1 and s["face_state"][interior].tolist() == [state] and np.all(s["face_state"][~interior] == 0)
    assert s["tet_violations"].tolist() == ([1, 1] if state == 2 else [0, 0])
    if state != 3:                                                            # the verdict is symmetric in the two tetrahedra
        swapped = ft.copy()
        swapped[interior] = swapped[interior][:, ::-1]
        assert g.delaunay_face_statement(cells, swapped, pts)["face_state"][interior].tolist() == [state]


def test_statement_in_torch_equals_numpy(scenes):
    g = dc.geometry()
    for name in ("random_400_moved", "grid_5"):
        pts, cells, ft = dc.case(scenes, name)
        want = dc.statement(scenes, name)
        got = g.delaunay_face_statement(torch.from_numpy(cells), torch.from_numpy(ft.view(np.int32)), torch.from_numpy(pts))
        for k in ("face_state", "tet_violations", "counters"):
            np.testing.assert_array_equal(got[k].numpy(), want[k], err_msg=f"{name}: {k}")


def test_nan_is_uncertain():
    g = dc.geometry()
    pts, cells, _, _ = dc.hand("inside")
    pts = pts.copy()
    pts[4, 1] = np.nan
    s = g.delaunay_face_statement(cells, dc.face_tets_of(cells), pts)
    assert s["counters"].tolist() == [1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "delaunay_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "delaunay_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def delaunay_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, cells, face_tets, values, new_cells):
    V, T, F, T2 = len(xyz), len(cells), len(face_tets), len(new_cells)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQQ", V, T, F, T2))
        f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
        f.write(np.ascontiguousarray(cells).astype(np.uint32).tobytes())
        f.write(np.ascontiguousarray(face_tets).astype(np.uint32).tobytes())
        f.write(np.ascontiguousarray(values, np.float32).tobytes())
        f.write(np.ascontiguousarray(new_cells).astype(np.uint32).tobytes())
    # (the sanitizer build: bounds and undefined behaviour are the point; its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    assert len(raw) == F + T + 16 + 4 * V + 4 * T2
    state, raw = np.frombuffer(raw[:F], np.int8), raw[F:]
    per_tet, raw = np.frombuffer(raw[:T], np.uint8), raw[T:]
    counters, raw = np.frombuffer(raw[:16], np.uint32), raw[16:]
    star, raw = np.frombuffer(raw[:4 * V], np.uint32), raw[4 * V:]
    return state, per_tet, counters, star, np.frombuffer(raw, np.uint32)


@pytest.mark.parametrize("name", ["random_400", "random_400_moved", "grid_5", "cube"] + sorted(dc.HAND))
def test_emulated_kernels_equal_the_statement(delaunay_emul, tmp_path, scenes, name):
    g = dc.geometry()
    pts, cells, ft = dc.case(scenes, name)
    want = dc.statement(scenes, name)
    values = dc.occupancy_like(len(cells), 3)
    new_cells = cells[::-1][: max(1, len(cells) // 2)].copy()
    new_cells[0, 0] = len(pts) + 5                                            # an id past the table: passed over
    state, per_tet, counters, star, out = _run_emul(delaunay_emul, tmp_path, pts, cells, ft, values, new_cells)
    np.testing.assert_array_equal(state, want["face_state"])
    np.testing.assert_array_equal(per_tet, want["tet_violations"])
    assert counters.tolist() == want["counters"].tolist()
    r = g.remap_tet_values_statement(cells, new_cells, values, len(pts))
    np.testing.assert_array_equal(star, dc.bits(r["star_max"]))
    np.testing.assert_array_equal(out, dc.bits(r["values"]))


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds on the mesh whose
    T is no multiple of four (the byte counters live in whole words)"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    pts, cells, ft = dc.case(scenes, "random_400_moved")
    assert len(cells) % 4
    want = dc.statement(scenes, "random_400_moved")
    state, per_tet, counters, _, _ = _run_emul(exe, tmp_path, pts, cells, ft, dc.occupancy_like(len(cells), 3), cells[:7])
    np.testing.assert_array_equal(state, want["face_state"])
    np.testing.assert_array_equal(per_tet, want["tet_violations"])
    assert counters.tolist() == want["counters"].tolist()


# ------------------------------------------------------------------------------------------------------------------ transfer
def test_transfer_statement_equals_the_plain_loops(scenes):
    g = dc.geometry()
    pts, cells, _ = dc.case(scenes, "random_400")
    V = len(pts)
    new_cells = scenes.delaunay_cells(dc.case(scenes, "random_400_moved")[0].astype(np.float64))
    values = dc.occupancy_like(len(cells), 5)
    want, want_star = dc.remap_brute_force(cells, new_cells, values, V)
    for kind in ("numpy", "torch"):
        conv = (lambda x: x) if kind == "numpy" else torch.from_numpy
        r = g.remap_tet_values_statement(conv(cells), conv(new_cells), conv(values), V)
        np.testing.assert_array_equal(dc.bits(np.asarray(r["values"])), dc.bits(want), err_msg=kind)
        np.testing.assert_array_equal(dc.bits(np.asarray(r["star_max"])), dc.bits(want_star), err_msg=kind)


def test_transfer_is_conservative_on_a_retriangulated_mesh(scenes):
    """nothing that was live is culled: a new tetrahedron is at least as live as EVERY old tetrahedron around each of its
    vertices -- and the price: it is exactly as live as the liveliest of them (one ring of dilation, no more)"""
    g = dc.geometry()
    pts, cells, _ = dc.case(scenes, "random_400")
    moved = dc.case(scenes, "random_400_moved")[0]
    new_cells = scenes.delaunay_cells(moved.astype(np.float64))
    assert new_cells.shape != cells.shape or not np.array_equal(new_cells, cells)
    values = dc.occupancy_like(len(cells), 7)
    new = g.remap_tet_values_statement(cells, new_cells, values, len(pts))["values"]
    around = [set() for _ in range(len(pts))]
    for t, c in enumerate(cells.tolist()):
        for v in c:
            around[v].add(t)
    for t, c in enumerate(new_cells.tolist()):
        ring = sorted(set().union(*(around[v] for v in c)))
        assert np.all(new[t] >= values[ring]) and new[t] == values[ring].max()
    live_before, live_after = (values > 0.5).sum(), (new > 0.5).sum()
    print("tets", len(cells), "->", len(new_cells), "live above 0.5:", int(live_before), "->", int(live_after))
    assert live_before > 0 and live_after > 0


def test_transfer_edges():
    """a vertex no new cell names; a vertex no old cell names contributes 0; ids past the table are passed over; the rule on
    what the contract excludes: the maximum of the bit patterns"""
    g = dc.geometry()
    old = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int32)
    new = np.array([[1, 2, 3, 5], [5, 6, 7, 8], [0, 1, 2, 9]], np.int32)      # 4: in no new cell; 5..8: in no old cell; 9 >= V
    v = np.array([0.25, 0.75], np.float32)
    r = g.remap_tet_values_statement(old, new, v, 9)
    assert r["star_max"].tolist() == [0.25, 0.75, 0.75, 0.75, 0.75, 0, 0, 0, 0]
    assert r["values"].tolist() == [0.75, 0.0, 0.75]
    assert g.remap_tet_values_statement(old, new[:0], v, 9)["values"].shape == (0,)
    assert g.remap_tet_values_statement(old[:0], new, v[:0], 9)["values"].tolist() == [0, 0, 0]
    # bit patterns: a set sign bit beats everything, a positive NaN beats every number, +inf beats every finite value
    weird = np.array([np.inf, -1e-30], np.float32)
    r = g.remap_tet_values_statement(old, new, weird, 9)
    assert dc.bits(r["values"]).tolist() == [int(dc.bits(weird)[1]), 0, int(dc.bits(weird)[1])]
    r = g.remap_tet_values_statement(old, new, np.array([np.inf, 3.0], np.float32), 9)
    assert r["values"].tolist() == [np.inf, 0.0, np.inf]
    r = g.remap_tet_values_statement(old, new, np.array([np.nan, np.inf], np.float32), 9)
    assert dc.bits(r["values"]).tolist() == [0x7FC00000, 0, 0x7FC00000]


# ------------------------------------------------------------------------------------------------------------------- entries
def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_delaunay_check\(tn_tracer_t tracer, size_t num_vertices, const float \*xyz, uint32_t \*counters,\s*"
                     r"int8_t \*face_state,\s*uint8_t \*tet_violations, void \*stream\);", header)
    assert re.search(r"int\s+tn_remap_tet_values\(size_t num_vertices, size_t num_old_cells, const uint32_t \*old_cells,\s*"
                     r"const float \*old_values,\s*size_t num_new_cells, const uint32_t \*new_cells, float \*new_values,\s*"
                     r"float \*star_max, void \*stream\);", header)
    lib = _lib.load()
    for name in ("tn_delaunay_check", "tn_remap_tet_values"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert len(lib.tn_delaunay_check.argtypes) == 7 and len(lib.tn_remap_tet_values.argtypes) == 9
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.supports_delaunay_check is True
    for name in ("delaunay_check", "retriangulate"):
        assert hasattr(ext.TetrahedraTracer, name)
    assert hasattr(ext, "remap_tet_values")
    src = (CSRC / "tn_delaunay.hip").read_text()
    blocks = int(re.search(r"constexpr unsigned DELAUNAY_BLOCKS = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr int BT = (\d+);", src).group(1))
    assert ext.TetrahedraTracer.DELAUNAY_GRID_LANES == blocks * threads
    g = dc.geometry()
    core = (CSRC / "tn_delaunay_core.h").read_text()
    assert "INSPHERE_BOUND = (16.0 + 224.0 * EPS) * EPS" in core and "ORIENT_BOUND = (7.0 + 56.0 * EPS) * EPS" in core
    assert g.DELAUNAY_EPS == 2.0 ** -53 and "EPS = 1.0 / 9007199254740992.0" in core and 2.0 ** 53 == 9007199254740992.0
    assert (g.FACE_HULL, g.FACE_REGULAR, g.FACE_VIOLATED, g.FACE_UNCERTAIN) == (0, 1, 2, 3)


def test_host_side_checks_raise_before_anything_runs():
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    cells, values = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.remap_tet_values(cells, cells, values, 4)


# ------------------------------------------------------------------------------------------------------------------- adapter
class _RecordingTracer:
    """what _follow_vertices and _monitor_delaunay touch of a TetrahedraTracer, recording every call"""
    supports_refit = True
    supports_vertex_step_limit = True
    supports_delaunay_check = True

    def __init__(self, vertices, cells, counters):
        self.tetrahedra_vertices, self.tetrahedra_cells = vertices, cells
        self._refittable = False
        self.calls = []
        self.counters = counters                     # what delaunay_check reports, one list per call

    def load_tetrahedra(self, xyz, cells, refittable=False):
        self.calls.append(("load", refittable))
        self._refittable = refittable
        self.tetrahedra_vertices, self.tetrahedra_cells = xyz, cells

    def update_vertices(self, xyz):
        self.calls.append(("update",))
        self.tetrahedra_vertices = xyz

    def limit_vertex_step(self, xyz_old, xyz_new, fraction=0.25, verify=True):
        self.calls.append(("limit",))
        return torch.zeros(4, dtype=torch.int32), torch.ones(len(xyz_old))

    def delaunay_check(self, xyz=None, face_state=False, tet_violations=False):
        self.calls.append(("check", xyz, face_state, tet_violations))
        return {"counters": torch.tensor(self.counters.pop(0), dtype=torch.int32), "face_state": None, "tet_violations": None}

    def retriangulate(self, xyz, tet_values=()):
        self.calls.append(("retriangulate", xyz, tuple(tet_values)))
        cells = torch.ones(5, 4, dtype=torch.int32)
        self.load_tetrahedra(xyz, cells, refittable=self._refittable)
        return {"cells": cells, "tet_values": [torch.full((5,), 2.0) for _ in tet_values], "num_tetrahedra": 5}


def _names(tracer):
    return [c[0] for c in tracer.calls]


def test_adapter_checks_every_nth_call_and_retriangulates_above_the_threshold():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.nn.Parameter(torch.arange(12, dtype=torch.float32).reshape(4, 3))
    cells = torch.zeros(3, 4, dtype=torch.int32)
    tracer = _RecordingTracer(v, cells, [[100, 5, 1, 0], [100, 6, 0, 0], [100, 0, 0, 0]])
    occupancy = torch.tensor([0.0, 1.0, 0.0])
    model = types.SimpleNamespace(tetrahedra_cells=cells, tetrahedra_occupancy=occupancy,
                                  config=types.SimpleNamespace(num_tetrahedra_cells=3))
    follow = lambda: plugin._follow_vertices(tracer, model, 0.3, 2, 0.05)   # noqa: E731
    follow()                                                          # call 1: the load with the refit tables, no check
    assert _names(tracer) == ["load"]
    with torch.no_grad():
        v += 1.0
    follow()                                                          # call 2: limit, refit, THEN the check: 5 % is not above 5 %
    assert _names(tracer) == ["load", "limit", "update", "check"]
    assert tracer.calls[3][1:] == (None, False, False)                # on the vertices the tracer follows; no optional array
    assert model._tn_delaunay_counters.dtype == torch.int64 and model._tn_delaunay_counters.tolist() == [100, 5, 1, 0]
    assert model.tetrahedra_cells is cells and model.tetrahedra_occupancy is occupancy
    follow()                                                          # call 3: nothing moved, not a checking call
    assert _names(tracer) == ["load", "limit", "update", "check"]
    with torch.no_grad():
        v += 1.0
    follow()                                                          # call 4: 6 % is above: re-triangulation
    assert _names(tracer) == ["load", "limit", "update", "check", "limit", "update", "check", "retriangulate", "load"]
    _, xyz, carried = tracer.calls[7]
    assert xyz is v and len(carried) == 1 and torch.equal(carried[0], occupancy)
    assert tracer.calls[8] == ("load", True)                          # the tracer keeps following
    assert model.tetrahedra_cells is tracer.tetrahedra_cells and model.tetrahedra_cells.shape == (5, 4)
    assert model.tetrahedra_occupancy.tolist() == [2.0] * 5 and model.config.num_tetrahedra_cells == 5
    assert model._tn_delaunay_counters.tolist() == [200, 11, 1, 0] and model._tn_retriangulations == 1
    assert torch.equal(tracer._tn_vertex_snapshot, v.detach()) and tracer._tn_vertex_snapshot.data_ptr() != v.data_ptr()
    assert tracer._tn_vertex_key == (v._version, v.data_ptr())
    follow()                                                          # call 5: nothing moved: no refit against the new cells
    follow()                                                          # call 6: the check alone, nothing violated
    assert _names(tracer)[9:] == ["check"] and model._tn_retriangulations == 1
    assert model._tn_delaunay_counters.tolist() == [300, 11, 1, 0]


def test_adapter_replaces_registered_buffers_under_their_names():
    """on a torch module the two tensors stay registered buffers: the state dict keeps its keys and carries the new sizes"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.nn.Parameter(torch.zeros(4, 3))
    cells = torch.zeros(3, 4, dtype=torch.int32)
    model = torch.nn.Module()
    model.register_buffer("tetrahedra_cells", cells)
    model.register_buffer("tetrahedra_occupancy", torch.nn.Parameter(torch.zeros(3)))      # as the reference registers it
    model.config = types.SimpleNamespace(num_tetrahedra_cells=3)
    tracer = _RecordingTracer(v, cells, [[10, 9, 0, 0]])
    plugin._follow_vertices(tracer, model, None, 1, 0.5)
    assert _names(tracer) == ["load", "check", "retriangulate", "load"]
    state = model.state_dict()
    assert sorted(state) == ["tetrahedra_cells", "tetrahedra_occupancy"]
    assert state["tetrahedra_cells"].shape == (5, 4) and state["tetrahedra_occupancy"].tolist() == [2.0] * 5
    assert model.config.num_tetrahedra_cells == 5 and not hasattr(tracer, "_tn_vertex_snapshot")


def test_adapter_without_a_threshold_only_counts():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.nn.Parameter(torch.zeros(4, 3))
    tracer = _RecordingTracer(v, torch.zeros(3, 4, dtype=torch.int32), [[10, 9, 0, 0], [10, 9, 0, 0]])
    model = types.SimpleNamespace()
    for _ in range(2):
        plugin._follow_vertices(tracer, model, None, 1, None)
    assert _names(tracer) == ["load", "check", "check"] and model._tn_delaunay_counters.tolist() == [20, 18, 0, 0]
    assert not hasattr(tracer, "_tn_vertex_snapshot")


def test_adapter_without_the_fields_calls_what_it_called():
    """absent or None: nothing new runs, whatever else is configured"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.nn.Parameter(torch.zeros(4, 3))
    for args in ((0.3,), (0.3, None, 0.01), (None, None, None)):
        tracer = _RecordingTracer(v, torch.zeros(3, 4, dtype=torch.int32), [])
        plugin._follow_vertices(tracer, types.SimpleNamespace(), *args)
        with torch.no_grad():
            v += 1.0
        plugin._follow_vertices(tracer, types.SimpleNamespace(), *args)
        assert "check" not in _names(tracer) and "retriangulate" not in _names(tracer)
        assert not hasattr(tracer, "_tn_follow_calls")


def test_adapter_refuses_the_monitor_without_refit():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    tracer = _RecordingTracer(torch.zeros(4, 3), torch.zeros(1, 4, dtype=torch.int32), [])
    model = types.SimpleNamespace(config=types.SimpleNamespace(delaunay_check_every=4), mlp_base=object(),
                                  get_tetrahedra_tracer=lambda: tracer)
    with pytest.raises(ValueError, match="refit_vertices"):
        plugin.fused_get_outputs(model, None)
    assert tracer.calls == []
