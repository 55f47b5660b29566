"""The isosurface extraction without a GPU (tn_isosurface_count / tn_isosurface_emit, csrc/tn_isosurface.hip; the rule: DESIGN.md
section 4.17).  Layers: tests/host/isosurface_emul.cpp -- which drives the element functions of csrc/tn_isosurface_core.h, the
bodies of the kernels -- bit for bit against the numpy statement on every case of tests/isosurface_cases.py; the statement's own
properties (closed, oriented, Euler characteristic 2, on the plane, normals along the gradient); its table against the header's and
against geometry; a plain-loop restatement that rejects four mutations of the rule on named cases; the PLY round trip; and the
refusals of the entries, the wrappers and the adapter.  (The kernels themselves: tests/test_isosurface_gpu.py.)"""
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

import isosurface_cases as ic

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "isosurface_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "isosurface_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def isosurface_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, cells, values, level, mask):
    V, T = len(values), len(cells)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQfI", V, T, 0 if mask is None else 1, level, 0))
        f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
        f.write(np.ascontiguousarray(cells, np.int32).tobytes())
        f.write(np.ascontiguousarray(values, np.float32).tobytes())
        if mask is not None:
            f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    out = {"tri_offsets": np.frombuffer(raw, np.uint32, T + 1), "ref_offsets": np.frombuffer(raw, np.uint32, T + 1, 4 * (T + 1))}
    at = 8 * (T + 1)
    N, M = struct.unpack_from("<Q", raw, at)[0], int(out["tri_offsets"][T])
    at += 8
    for key, dtype, count, shape in (("triangles", np.int32, 3 * M, (M, 3)), ("triangle_tets", np.int32, M, (M,)),
                                     ("edge_vertices", np.int32, 2 * N, (N, 2)), ("edge_t", np.float32, N, (N,)),
                                     ("positions", np.float32, 3 * N, (N, 3))):
        out[key] = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += 4 * count
    assert at == len(raw)
    out["num_triangles"], out["num_refs"] = M, int(out["ref_offsets"][T])
    return out


def _assert_equal(got, want, what):
    assert got["num_triangles"] == want["num_triangles"] and got["num_refs"] == want["num_refs"], what
    for key in ic.ARRAYS + ("tri_offsets", "ref_offsets"):
        if key in got:
            assert got[key].shape == want[key].shape, f"{what}: {key} {got[key].shape} vs {want[key].shape}"
            assert np.array_equal(ic.bits(got[key]), ic.bits(want[key])), f"{what}: {key}"


@pytest.mark.parametrize("name", ic.names())
def test_emulated_kernels_equal_the_statement(isosurface_emul, tmp_path, scenes, name):
    want = ic.statement(scenes, name)
    got = _run_emul(isosurface_emul, tmp_path, *ic.case(scenes, name))
    _assert_equal(got, want, name)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: ids past the table,
    a mask, the largest id, and a surface of some size"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ("skip_id_past_V", "skip_id_empty", "ids_around_2_16", "sphere_120_masked", "soup_257", "no_tets"):
        _assert_equal(_run_emul(exe, tmp_path, *ic.case(scenes, name)), ic.statement(scenes, name), name)


# ------------------------------------------------------------------------------------------------- the statement's properties
def test_the_cases_are_what_they_are_named_for(scenes):
    bt, blocks = ic.kernel_constants()
    assert bt % 64 == 0 and set(ic.size_edges()) >= {63, 64, 65, bt - 1, bt, bt + 1, bt * blocks - 1, bt * blocks, bt * blocks + 1}
    for name in ic.names():
        xyz, cells, values, level, mask = ic.case(scenes, name)
        assert xyz.shape == (len(values), 3) and cells.shape[1:] == (4,) and (mask is None or mask.shape == (len(cells),))
        if name.startswith("soup_"):
            crossed = np.count_nonzero(np.diff(ic.statement(scenes, name)["tri_offsets"].astype(np.int64)))
            assert len(cells) == int(name[5:]) and crossed > 0
            if len(cells) > 2500:                                             # "about a tenth" holds for the mesh, not for a small cut
                assert 0.05 * len(cells) < crossed < 0.2 * len(cells)
    assert len(ic.case(scenes, "ids_around_2_16")[2]) == 2 ** 16 + 1 and len(ic.case(scenes, "ids_around_2_20")[2]) == 2 ** 20 + 1
    for power in (16, 20):
        ids = ic.statement(scenes, f"ids_around_2_{power}")["edge_vertices"]
        assert ids.max() == 2 ** power and (ids == 2 ** power - 1).any() and (ids < 4).any()


@pytest.mark.parametrize("orient", sorted(ic.ORDERS))
@pytest.mark.parametrize("code", range(16))
def test_every_table_row_faces_the_low_side(scenes, code, orient):
    """geometry, not the table, is the reference: on one tetrahedron the interpolant is linear, so every emitted triangle's normal
    has a negative product with its gradient, whichever way the tetrahedron is stored"""
    name = f"code_{code:02d}_{orient}"
    xyz, cells, values, level, _ = ic.case(scenes, name)
    s = ic.statement(scenes, name)
    pop = bin(code).count("1")
    assert s["num_triangles"] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[pop] and s["num_refs"] == {0: 0, 1: 3, 2: 4, 3: 3, 4: 0}[pop]
    assert len(s["positions"]) == s["num_refs"] and s["triangle_tets"].tolist() == [0] * s["num_triangles"]
    x = xyz.astype(np.float64)
    grad = np.linalg.solve(x[1:] - x[0], values[1:].astype(np.float64) - float(values[0]))
    p = s["positions"].astype(np.float64)
    for tri in s["triangles"]:
        normal = np.cross(p[tri[1]] - p[tri[0]], p[tri[2]] - p[tri[0]])
        assert normal @ grad < -1e-3 * np.linalg.norm(normal) * np.linalg.norm(grad) and np.linalg.norm(normal) > 1e-3, (name, tri)
    if pop == 2:                                                              # the two triangles share an edge, oppositely directed
        assert ic.euler_characteristic(4, s["triangles"]) == 1
        e = {tuple(r) for r in ic.directed_edges(s["triangles"]).tolist()}
        assert len(e) == 6 and sum((b, a) in e for a, b in e) == 2


def test_flat_tetrahedron_counts_as_positive(scenes):
    g = ic.geometry()
    for name, code in (("flat_1_edge_code", 1), ("flat_2_edge_code", 6)):
        xyz, cells, _, _, _ = ic.case(scenes, name)
        assert int(g.tet_orient(torch.from_numpy(xyz), torch.from_numpy(cells))[0]) == 0
        s = ic.statement(scenes, name)
        # cells = (0, 1, 2, 3): the tet edges in their own order are the keys in ascending order, so a vertex id is its edge's rank
        crossing = sorted({e for row in g.ISO_TRI_TABLE[code] for e in row if e >= 0})
        want = [[crossing.index(e) for e in row] for row in g.ISO_TRI_TABLE[code] if row[0] >= 0]
        assert cells.tolist() == [[0, 1, 2, 3]] and s["triangles"].tolist() == want      # the rows as written: no swap at orient 0


def test_degenerate_values(scenes):
    xyz, cells, values, level, _ = ic.case(scenes, "value_at_level")
    s = ic.statement(scenes, "value_at_level")
    assert s["num_triangles"] == 1 and s["edge_t"].tolist() == [0.0, 0.0, 0.0] and s["edge_vertices"].tolist() == [[0, 1], [0, 2], [0, 3]]
    assert np.array_equal(s["positions"], np.repeat(xyz[:1], 3, 0))           # a zero-area triangle at the vertex itself, kept
    s = ic.statement(scenes, "value_at_level_far_end")                        # the corner at the level is the LARGER id of its edges
    assert s["num_triangles"] == 1 and s["edge_t"].tolist() == [1.0, 1.0, 1.0] and s["edge_vertices"][:, 1].tolist() == [3, 3, 3]
    s = ic.statement(scenes, "all_at_level")
    assert s["num_triangles"] == 0 and s["num_refs"] == 0 and s["positions"].shape == (0, 3)


def test_each_skip_reason_alone_silences_its_tetrahedron(scenes):
    g = ic.geometry()
    both = ic.statement(scenes, "pair")
    assert both["triangle_tets"].tolist() == [0, 1] and both["num_refs"] == 6 and len(both["positions"]) == 4      # two edges welded
    assert both["edge_vertices"].tolist() == [[0, 1], [1, 2], [1, 3], [1, 4]]
    xyz, cells, values, level, _ = ic.case(scenes, "pair")
    alone = g.isosurface_statement(xyz, cells[1:], values, level)
    for name in ic.SKIPPED_FIRST:
        s = ic.statement(scenes, name)
        assert s["triangle_tets"].tolist() == [1] and s["tri_offsets"].tolist() == [0, 0, 1] and s["ref_offsets"].tolist() == [0, 0, 3], name
        for key in ("positions", "triangles", "edge_vertices", "edge_t"):
            assert np.array_equal(ic.bits(s[key]), ic.bits(alone[key])), (name, key)
    kept = ic.statement(scenes, "kept_below_2_126")                           # the largest float below the bound still emits
    assert kept["triangle_tets"].tolist() == [0, 1]
    empty, none = ic.statement(scenes, "no_tets"), ic.statement(scenes, "no_crossing")
    assert empty["tri_offsets"].tolist() == [0] and none["tri_offsets"].tolist() == [0, 0, 0]
    for s in (empty, none):
        assert s["positions"].shape == (0, 3) and s["triangles"].shape == (0, 3) and s["edge_vertices"].shape == (0, 2)


def test_vertices_ascend_by_the_smaller_id_first(scenes):
    s = ic.statement(scenes, "key_a_first")
    assert s["edge_vertices"].tolist() == [[1, 10], [1, 11], [1, 70000], [2, 5], [2, 12], [2, 13]]
    for name in ic.names(large=False):
        ev = ic.statement(scenes, name)["edge_vertices"].astype(np.int64)
        key = ev[:, 0] << 32 | ev[:, 1]
        assert np.all(ev[:, 0] < ev[:, 1]) and np.all(np.diff(key) > 0), name
        tets = ic.statement(scenes, name)["triangle_tets"]
        assert np.all(np.diff(tets) >= 0), name


@pytest.mark.parametrize("name", sorted(ic.SPHERES))
def test_closed_surfaces(scenes, name):
    s = ic.statement(scenes, name)
    T = len(ic.case(scenes, name)[1])
    volume = ic.enclosed_volume(s["positions"], s["triangles"])
    chi = ic.euler_characteristic(len(s["positions"]), s["triangles"])
    print(name, "T", T, "vertices", len(s["positions"]), "triangles", len(s["triangles"]), "chi", chi, "volume", volume,
          "of the sphere's", volume / (4 / 3 * np.pi * 0.6 ** 3))
    assert ic.closed_and_oriented(s["triangles"]) and chi == 2
    assert volume > 0                                                         # outward normals; the analytic volume is no reference
    assert np.all((s["edge_t"] >= 0) & (s["edge_t"] <= 1))


def test_masked_surface_is_the_unmasked_one_on_the_kept_tetrahedra(scenes):
    g = ic.geometry()
    xyz, cells, values, level, mask = ic.case(scenes, "sphere_120_masked")
    s, full = ic.statement(scenes, "sphere_120_masked"), ic.statement(scenes, "sphere_120")
    assert 0 < s["num_triangles"] < full["num_triangles"] and not ic.closed_and_oriented(s["triangles"])
    assert np.all(mask[s["triangle_tets"]] == 1)
    kept = np.nonzero(mask)[0]
    cut = g.isosurface_statement(xyz, cells[kept], values, level)
    assert np.array_equal(kept[cut["triangle_tets"]], s["triangle_tets"])
    for key in ("positions", "triangles", "edge_vertices", "edge_t"):
        assert np.array_equal(ic.bits(cut[key]), ic.bits(s[key])), key


def test_linear_field_lies_on_its_plane(scenes):
    xyz, cells, values, level, _ = ic.case(scenes, "linear")
    s = ic.statement(scenes, "linear")
    bound, _ = ic.plane_bound(xyz, values)
    d = ic.plane_distance(s["positions"])
    print("linear: vertices", len(d), "max distance", np.abs(d).max(), "bound", bound)
    assert len(d) > 100 and np.abs(d).max() <= bound and bound < 2e-6
    # normals: the vertices are within `bound` of the plane, so a triangle's cross product leaves the plane's normal by at most
    # delta = 2 bound (|u| + |v|) + 4 bound^2; where |cross| > 4 delta the triangle is non-degenerate and its side is decided
    p, t = s["positions"].astype(np.float64), s["triangles"]
    u, v = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    cross = np.cross(u, v)
    unit = ic.PLANE_N / np.linalg.norm(ic.PLANE_N)
    along = cross @ unit
    off = np.linalg.norm(cross - along[:, None] * unit, axis=1)
    delta = 2 * bound * (np.linalg.norm(u, axis=1) + np.linalg.norm(v, axis=1)) + 4 * bound ** 2
    decided = np.linalg.norm(cross, axis=1) > 4 * delta
    print("triangles", len(t), "non-degenerate", int(decided.sum()))
    assert decided.sum() > 0.9 * len(t) and np.all(off <= delta) and np.all(along[decided] < 0)


# --------------------------------------------------------------------------------------------------------------- the table
def test_table_equals_the_header():
    g = ic.geometry()
    core = (CSRC / "tn_isosurface_core.h").read_text()
    body = core[core.index("TRI_TABLE[16][2][3] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    numbers = [int(x) for x in re.findall(r"-?\d+", re.sub(r"//.*", "", body))]
    assert len(numbers) == 96 and np.array_equal(np.array(numbers).reshape(16, 2, 3), np.array(g.ISO_TRI_TABLE))
    edges = core[core.index("EDGE_CORNERS[6][2] = "):]
    assert [int(x) for x in re.findall(r"\d", edges[edges.index("{"):edges.index(";")])] == [c for e in g.ISO_EDGE_CORNERS for c in e]
    assert "VALUE_LIMIT = 8.507059173023462e37f" in core and float(np.float32(8.507059173023462e37)) == 2.0 ** 126 == g.ISO_VALUE_LIMIT
    assert "MAX_TETS = 1ull << 30" in core and g.ISO_MAX_TETS == 1 << 30
    for code, rows in enumerate(g.ISO_TRI_TABLE):                             # rows name crossing edges only, each triangle three
        crossing = {e for e, (a, b) in enumerate(g.ISO_EDGE_CORNERS) if (code >> a ^ code >> b) & 1}
        used = {e for row in rows for e in row if e >= 0}
        assert used == crossing and all(len(set(row)) == 3 or row == (-1, -1, -1) for row in rows), code


# -------------------------------------------------------------------------------------------- a restatement and its mutations
def _restate(case, table=None, swap=True, key_bits=64, sorted_pair=True):
    """the rule as a plain loop over tetrahedra with a dictionary for the welding; the keywords are the four mutations"""
    g = ic.geometry()
    xyz, cells, values, level, mask = case
    table, ec = table or g.ISO_TRI_TABLE, g.ISO_EDGE_CORNERS
    V, L = len(values), np.float32(level)
    tris, verts = [], {}
    for ti, c in enumerate(np.ascontiguousarray(cells).view(np.uint32).tolist()):
        if (mask is not None and not mask[ti]) or any(i >= V for i in c):
            continue
        v = values[c]
        if not all(abs(float(x)) < 2.0 ** 126 for x in v):
            continue
        code = sum(1 << k for k in range(4) if v[k] >= L)
        negative = float(g._vol6(xyz[c].astype(np.float64)[None])[0]) < 0
        for row in table[code]:
            if row[0] < 0:
                continue
            row = [row[0], row[2], row[1]] if swap and negative else list(row)
            keys = []
            for e in row:
                i, j = c[ec[e][0]], c[ec[e][1]]
                key = (min(i, j) << 32 | max(i, j)) & ((1 << key_bits) - 1)
                if key not in verts:
                    s, d = (min(i, j), max(i, j)) if sorted_pair else (i, j)
                    t = (L - values[s]) / (values[d] - values[s])
                    verts[key] = xyz[s] + t * (xyz[d] - xyz[s])
                keys.append(key)
            tris.append(keys)
    index = {k: n for n, k in enumerate(sorted(verts))}
    positions = np.array([verts[k] for k in sorted(verts)], np.float32).reshape(-1, 3)
    return positions, np.array([[index[k] for k in t] for t in tris], np.int32).reshape(-1, 3)


def _same(a, want):
    return a[0].shape == want["positions"].shape and np.array_equal(ic.bits(a[0]), ic.bits(want["positions"])) and \
        np.array_equal(a[1], want["triangles"])


def test_restatement_equals_the_statement(scenes):
    for name in ic.names(large=False):
        assert _same(_restate(ic.case(scenes, name)), ic.statement(scenes, name)), name


def test_mutations_of_the_rule_are_rejected_by_named_cases(scenes):
    g = ic.geometry()
    swapped = [list(map(tuple, rows)) for rows in g.ISO_TRI_TABLE]
    swapped[5][1] = (0, 2, 5)                                                 # a swapped corner pair in one table row
    mutations = {
        "a swapped corner pair in one table row": ("code_05_pos", dict(table=swapped)),
        "the orientation swap dropped": ("code_01_neg", dict(swap=False)),
        "keys cut to 32 bits": ("key_a_first", dict(key_bits=32)),
        "t taken from the unsorted pair": ("code_01_neg", dict(sorted_pair=False)),
    }
    for what, (name, kw) in mutations.items():
        case, want = ic.case(scenes, name), ic.statement(scenes, name)
        assert _same(_restate(case), want), name
        assert not _same(_restate(case, **kw), want), f"{what}: not rejected by {name}"
    # and on a closed surface the first two show as a surface that is no longer oriented
    case = ic.case(scenes, "sphere_56")
    assert ic.closed_and_oriented(_restate(case)[1])
    assert not ic.closed_and_oriented(_restate(case, table=swapped)[1]) and not ic.closed_and_oriented(_restate(case, swap=False)[1])


# --------------------------------------------------------------------------------------------------------------------- PLY
def test_ply_round_trip(tmp_path, scenes):
    io = importlib.import_module("tetra-nerf_amd.tetrahedra_io")
    s = ic.statement(scenes, "sphere_56")
    colors = np.random.default_rng(1).integers(0, 256, (len(s["positions"]), 3)).astype(np.uint8)
    for name, c in (("plain.ply", None), ("colored.ply", colors)):
        io.save_mesh_ply(tmp_path / name, torch.from_numpy(s["positions"]), s["triangles"], c)
        raw = (tmp_path / name).read_bytes()
        assert raw.startswith(b"ply\nformat binary_little_endian 1.0\n")
        got = io.load_mesh_ply(tmp_path / name)
        assert got["positions"].dtype == torch.float32 and got["triangles"].dtype == torch.int32
        assert np.array_equal(ic.bits(got["positions"].numpy()), ic.bits(s["positions"])) and np.array_equal(got["triangles"].numpy(), s["triangles"])
        assert (got["colors"] is None) if c is None else (got["colors"].dtype == torch.uint8 and np.array_equal(got["colors"].numpy(), c))
        body = len(s["positions"]) * (12 if c is None else 15) + len(s["triangles"]) * 13
        assert len(raw) == raw.index(b"end_header\n") + 11 + body
    io.save_mesh_ply(tmp_path / "empty.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert io.load_mesh_ply(tmp_path / "empty.ply")["triangles"].shape == (0, 3)
    with pytest.raises(ValueError, match="uint8"):
        io.save_mesh_ply(tmp_path / "bad.ply", s["positions"], s["triangles"], colors.astype(np.float32))
    with pytest.raises(ValueError, match="not in positions"):
        io.save_mesh_ply(tmp_path / "bad.ply", s["positions"][:3], s["triangles"])
    (tmp_path / "cut.ply").write_bytes((tmp_path / "plain.ply").read_bytes()[:-5])
    with pytest.raises(ValueError, match="promises"):
        io.load_mesh_ply(tmp_path / "cut.ply")
    (tmp_path / "ascii.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="binary_little_endian"):
        io.load_mesh_ply(tmp_path / "ascii.ply")


# ---------------------------------------------------------------------------------------------------------------- entries
def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_isosurface_count\(size_t num_vertices, size_t num_cells, const uint32_t \*cells, const float \*values,\s*"
                     r"float level,\s*const uint8_t \*tet_mask, uint32_t \*tri_offsets, uint32_t \*ref_offsets, void \*stream\);", header)
    assert re.search(r"int\s+tn_isosurface_emit\(size_t num_vertices, size_t num_cells, const float \*xyz, const uint32_t \*cells,\s*"
                     r"const float \*values,\s*float level, const uint8_t \*tet_mask, const uint32_t \*tri_offsets,\s*"
                     r"const uint32_t \*ref_offsets,\s*size_t num_triangles, size_t num_refs, uint32_t \*triangles,\s*"
                     r"uint32_t \*triangle_tets,\s*uint32_t \*edge_vertices, float \*edge_t, float \*positions,\s*"
                     r"uint32_t \*num_out_vertices, void \*stream\);", header)
    assert "no reference counterpart" in header[header.index("Isosurface extraction"):header.index("int tn_isosurface_count")]
    lib = _lib.load()
    for name in ("tn_isosurface_count", "tn_isosurface_emit"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert len(lib.tn_isosurface_count.argtypes) == 9 and len(lib.tn_isosurface_emit.argtypes) == 18
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.supports_isosurface is True and hasattr(ext.TetrahedraTracer, "isosurface") and hasattr(ext, "isosurface")
    bt, blocks = ic.kernel_constants()
    assert ext.TetrahedraTracer.ISOSURFACE_GRID_LANES == bt * blocks
    for name in ("extract_mesh", "vertex_normals"):
        assert hasattr(importlib.import_module("tetra-nerf_amd.render"), name)
    assert hasattr(importlib.import_module("tetra-nerf_amd.nerfstudio_plugin"), "extract_mesh")


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    lib = _lib.load()
    x = 64                                                                    # a pointer that is never followed
    count = lambda V, T, cells, values, level, tri=x, ref=x: lib.tn_isosurface_count(V, T, cells, values, level, None, tri, ref, None)   # noqa: E731
    for level in (float("nan"), float("inf"), -float("inf"), 2.0 ** 126, -2.0 ** 126, 1e300):
        assert count(5, 2, x, x, level) != 0 and b"level" in lib.tn_last_error(), level
    assert count(5, 2 ** 30, x, x, 0.0) != 0 and b"2^30" in lib.tn_last_error()
    assert count(2 ** 32 - 1, 2, x, x, 0.0) != 0 and b"vertices" in lib.tn_last_error()
    for args in ((5, 2, None, x, 0.0), (5, 2, x, None, 0.0), (5, 2, x, x, 0.0, None), (5, 2, x, x, 0.0, x, None), (5, 0, None, None, 0.0, None)):
        assert count(*args) != 0 and b"null" in lib.tn_last_error(), args

    def emit(V=5, T=2, xyz=x, cells=x, values=x, level=0.0, tri=x, ref=x, nt=1, nr=3, a=x, b=x, c=x, d=x, e=x, n=x):
        return lib.tn_isosurface_emit(V, T, xyz, cells, values, level, None, tri, ref, nt, nr, a, b, c, d, e, n, None)

    for kw in (dict(xyz=None), dict(cells=None), dict(values=None), dict(tri=None), dict(ref=None), dict(a=None), dict(b=None),
               dict(c=None), dict(d=None), dict(e=None), dict(n=None), dict(T=0, cells=None, values=None, xyz=None, nt=0, nr=0, n=None)):
        assert emit(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert emit(level=float("nan")) != 0 and emit(T=2 ** 30) != 0
    assert emit(nt=5) != 0 and b"exceed" in lib.tn_last_error() and emit(nr=9) != 0 and b"exceed" in lib.tn_last_error()


def test_statement_and_wrappers_refuse():
    g = ic.geometry()
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    render = importlib.import_module("tetra-nerf_amd.render")
    xyz, cells, values, _, _ = ic.FIXED["pair"]()
    for level in (np.nan, np.inf, 2.0 ** 126, 1e39):
        with pytest.raises(ValueError, match="level"):
            g.isosurface_statement(xyz, cells, values, level)
    t = lambda a: torch.from_numpy(a)   # noqa: E731
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.isosurface(t(xyz), t(cells), t(values), 0.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.mlp_forward(torch.zeros(64, 5), None, [], 1)
    for pair in (dict(occupancy=torch.zeros(2)), dict(occupancy_threshold=0.5)):
        with pytest.raises(ValueError, match="both or neither"):
            render.extract_mesh(t(xyz), t(cells), torch.zeros(64, 5), None, 0.0, **pair)


def test_adapter_passes_the_models_buffers_and_the_occupancy_pair(tmp_path, monkeypatch):
    """render.extract_mesh replaced by a stand-in that records its call: the adapter hands over the model's buffers, the
    occupancy pair only when both exist, and writes what comes back"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    render = importlib.import_module("tetra-nerf_amd.render")
    io = importlib.import_module("tetra-nerf_amd.tetrahedra_io")
    calls = []
    mesh = {"positions": torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), "triangles": torch.tensor([[0, 1, 2]], dtype=torch.int32),
            "colors": torch.tensor([[0.0, 0.5, 1.0], [1.5, -1.0, 0.25], [0.2, 0.4, 0.6]])}

    def recorder(xyz, cells, field, mlp, level, occupancy=None, occupancy_threshold=None, **kw):
        calls.append((xyz, cells, field, mlp, level, occupancy, occupancy_threshold, kw))
        return mesh

    monkeypatch.setattr(render, "extract_mesh", recorder)
    v, c, f, occ = torch.zeros(4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.nn.Parameter(torch.zeros(64, 4)), torch.ones(1)
    model = types.SimpleNamespace(tetrahedra_vertices=torch.nn.Parameter(v), tetrahedra_cells=c, tetrahedra_field=f,
                                  config=types.SimpleNamespace())
    assert plugin.extract_mesh(model, 3.5) is mesh and not list(tmp_path.iterdir())
    xyz, cells, field, mlp, level, o, thr, kw = calls[-1]
    assert torch.equal(xyz, v) and not xyz.requires_grad and cells.data_ptr() == c.data_ptr() and field is f and level == 3.5 and o is None and thr is None
    assert isinstance(mlp, plugin.ModelMLP) and mlp.model is model
    model.tetrahedra_occupancy = occ                                          # the buffer without the threshold: no mask
    plugin.extract_mesh(model, 3.5)
    assert calls[-1][5] is None and calls[-1][6] is None
    model.config.occupancy_threshold = 0.25
    plugin.extract_mesh(model, 3.5, path=tmp_path / "out" / "mesh.ply")
    assert torch.equal(calls[-1][5], occ) and calls[-1][6] == 0.25
    got = io.load_mesh_ply(tmp_path / "out" / "mesh.ply")
    assert got["colors"].tolist() == [[0, 128, 255], [255, 0, 64], [51, 102, 153]] and got["triangles"].tolist() == [[0, 1, 2]]
    model.config.hidden_size = 64
    with pytest.raises(RuntimeError, match="hidden_size"):
        plugin.extract_mesh(model, 3.5)
