"""The edge split without a GPU (tn_edge_split_count(_tables) / tn_edge_split_emit, csrc/tn_edge_split.hip; the rule: DESIGN.md
section 4.22).  Layers: tests/host/edge_split_emul.cpp -- which drives the element functions of csrc/tn_edge_split_core.h, the
bodies of the kernels -- bit for bit against the numpy statement on the cases of tests/edge_split_cases.py, also under the host
sanitizers as a stand-alone program; a plain-loop restatement of the rule that equals the vectorised statement and rejects four
mutations on named cases; the structure of the split mesh; the preservation of the piecewise-linear field against a bound that
is derived, not measured, over one and over three generations; and the declarations and refusals of the entries.  (The kernels
themselves: tests/test_edge_split_gpu.py.)"""
import ctypes
import importlib
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import edge_split_cases as ec
import split_cases as sc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"
EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _t(a):
    return torch.from_numpy(np.array(a))                                      # (the cases are read-only: a copy)


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "edge_split_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "edge_split_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def edge_split_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, cells, select, faces, face_tets):
    V, T, F = len(xyz), len(cells), len(faces)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQ", V, T, F))
        for a, dtype in ((xyz, np.float32), (cells, np.int32), (select, np.uint8), (faces, np.int32), (face_tets, np.int32)):
            f.write(np.ascontiguousarray(a, dtype).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    counters = np.frombuffer(raw, np.uint32, 10)
    Kv, Kt, at, out = int(counters[8]), int(counters[9]), 40, {"counters": counters}
    for key, dtype, shape in (("tet_offsets", np.uint32, (T + 1,)), ("tet_edge", np.int32, (T,)), ("bisected", np.uint8, (T,)),
                              ("edge_vertices", np.int32, (Kv, 2)), ("vertices", np.float32, (V + Kv, 3)), ("cells", np.int32, (T + Kt, 4)),
                              ("cell_parent", np.int32, (T + Kt,)), ("vertex_parents", np.int32, (Kv, 4))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += np.dtype(dtype).itemsize * count
    assert at == len(raw)
    out.update(num_new=Kv, num_rows=Kt, num_cells=T + Kt)
    return out


def assert_equal(got, want, what):
    for key in ("num_new", "num_rows", "num_cells"):
        assert got[key] == want[key], f"{what}: {key} {got[key]} vs {want[key]}"
    for key in ec.ARRAYS:
        assert got[key].shape == want[key].shape, f"{what}: {key} {got[key].shape} vs {want[key].shape}"
        assert got[key].dtype == want[key].dtype and np.array_equal(ec.bits(got[key]), ec.bits(want[key])), f"{what}: {key}"


CPU_SOUPS = [n for n in ec.names(soups=True) if n not in ec.FIXED and int(n.split("_")[1]) <= 1300] + \
    [f"soup_{ec.soup_sizes()[-1]}_third"]


@pytest.mark.parametrize("name", ec.names() + CPU_SOUPS)
def test_emulated_kernels_equal_the_statement(edge_split_emul, tmp_path, scenes, name):
    got = _run_emul(edge_split_emul, tmp_path, *ec.case(scenes, name))
    assert_equal(got, ec.statement(scenes, name), name)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: ids past the table,
    a NaN, a repeated id, every refusal, empty inputs"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ("ring_bad_ids", "ring_nan", "ring_repeated_id", "ring_lost", "ring_flat", "ring_sound", "grid_4_all", "cube_all",
                 "random_300_30pct", "none_asked", "no_tets", "soup_257_third"):
        assert_equal(_run_emul(exe, tmp_path, *ec.case(scenes, name)), ec.statement(scenes, name), name)


# ------------------------------------------------------------------------------------------------ what the cases are named for
EXPECTED = {   # asked, asked refused id, asked refused flat, candidates, refused id / hull / lost / flat, accepted, bisected
    "cube_all": [12, 0, 0, 6, 0, 6, 0, 0, 0, 0],
    "ring_sound": [5, 0, 0, 1, 0, 0, 0, 0, 1, 5],
    "ring_flat": [5, 0, 1, 1, 0, 0, 0, 1, 0, 0],
    "ring_lost": [6, 0, 0, 2, 0, 0, 1, 0, 1, 1],
    "ring_bad_ids": [7, 2, 0, 1, 1, 0, 0, 0, 0, 0],
    "ring_nan": [5, 0, 2, 1, 0, 0, 0, 1, 0, 0],
    "ring_repeated_id": [6, 0, 1, 1, 0, 0, 0, 1, 0, 0],
    "none_asked": [0] * 10,
    "no_tets": [0] * 10,
}


def test_the_cases_are_what_they_are_named_for(scenes):
    bt, blocks = ec.kernel_constants()
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.EDGE_SPLIT_GRID_LANES == bt * blocks and ext.TetrahedraTracer.supports_edge_split is True
    assert set(ec.soup_sizes()) >= {1, 63, 64, 65, 255, 256, 257, bt * blocks - 1, bt * blocks, bt * blocks + 1}
    for name, want in EXPECTED.items():
        assert ec.statement(scenes, name)["counters"].tolist() == want, name
    s = ec.statement(scenes, "ring_sound")                                    # the edge ab = (0, 1), its midpoint the origin
    assert s["edge_vertices"].tolist() == [[0, 1]] and s["vertices"][7].tolist() == [0, 0, 0] and s["vertex_parents"].tolist() == [[0, 1, 0, 1]]
    assert s["cells"].tolist()[:2] == [[0, 7, 2, 3], [0, 7, 3, 4]] and s["cells"].tolist()[5] == [7, 1, 2, 3]
    assert ec.statement(scenes, "ring_lost")["edge_vertices"].tolist() == [[0, 7]]   # the stray row's own edge, not ab
    for name in ("ring_sound", "ring_flat", "ring_lost"):                     # ab is every ring row's longest edge
        xyz, cells = ec.case(scenes, name)[:2]
        d = np.linalg.norm(xyz[cells[:5]][:, :, None] - xyz[cells[:5]][:, None], axis=-1)
        assert np.all(d.max((1, 2)) == d[:, 0, 1]) and np.all(np.sort(d.reshape(5, -1), 1)[:, -3] < 2)
    for C in ec.candidate_counts()[0]:
        c = ec.counters(scenes, f"rings_{C}_all")
        assert c["candidates"] == c["accepted"] == C and c["bisected"] == 5 * C
    c = ec.counters(scenes, "soup_257_third")                                 # 51 whole rings and an open one: its ab is on the hull
    assert c["candidates"] == 52 and c["refused_hull"] == 1 and c["accepted"] == 51 and c["bisected"] == 255
    assert ec.counters(scenes, "soup_257_none")["asked"] == 0 and ec.counters(scenes, "soup_257_one")["accepted"] == 1
    seen = np.zeros(10, bool)
    for name in ec.names():
        seen |= ec.statement(scenes, name)["counters"] > 0
    assert seen.all(), [n for n, s in zip(ec.COUNTERS, seen) if not s]


def test_every_counter_is_non_zero_in_a_named_case(scenes):
    where = {"asked": "ring_sound", "asked_refused_id": "ring_bad_ids", "asked_refused_flat": "ring_nan", "candidates": "cube_all",
             "refused_id": "ring_bad_ids", "refused_hull": "cube_all", "refused_lost": "ring_lost", "refused_flat": "ring_flat",
             "accepted": "ring_sound", "bisected": "ring_sound"}
    assert tuple(where) == ec.COUNTERS == sc.geometry().EDGE_SPLIT_COUNTER_NAMES
    for counter, name in where.items():
        assert ec.counters(scenes, name)[counter] > 0, (counter, name)
    prototype = ec.counters(scenes, "random_300_30pct")                       # the figures the rule was designed with
    assert [prototype[k] for k in ("asked", "candidates", "refused_hull", "refused_lost", "refused_flat", "accepted", "bisected")] == \
        [483, 422, 52, 266, 0, 104, 422]


# -------------------------------------------------------------------------------------------- a restatement and its mutations
def _orient(q):                                                               # 0 also for NaN
    with np.errstate(invalid="ignore", over="ignore"):
        v = float(ec.vol6(np.asarray(q, np.float64)[None])[0])
    return 1 if v > 0 else (-1 if v < 0 else 0)


def _restate(case, key_tie=True, among_candidates=True, hull_before_lost=True, hi_in_place=True):
    """the rule as plain loops over tetrahedra, faces and edges, with dicts and sets where the statement sorts and searches; the
    keywords are the four mutations.  Returns the statement's arrays and, for the tests, what every row nominated."""
    xyz, cells, select, faces, face_tets = case
    V, T = len(xyz), len(cells)
    rows = [list(map(int, r)) for r in cells.view(np.uint32)]

    def length(e):
        with np.errstate(invalid="ignore", over="ignore"):
            d = xyz[e[1]] - xyz[e[0]]
            return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

    def beats(e, f):
        le, lf = length(e), length(f)
        return bool(le > lf) or (bool(le == lf) and key_tie and e < f)

    def best(edges):
        b = edges[0]
        for e in edges[1:]:
            if beats(e, b):
                b = e
        return b

    def edges_of(c):
        return [(min(c[a], c[b]), max(c[a], c[b])) for a, b in EDGE_CORNERS]

    nominated, asked_id, asked_flat = {}, 0, 0
    for t in range(T):
        if not select[t]:
            continue
        if any(i >= V for i in rows[t]):
            asked_id += 1
        elif _orient(xyz[rows[t]]) == 0:
            asked_flat += 1
        else:
            nominated[t] = best(edges_of(rows[t]))
    candidates = set(nominated.values())
    said, winner = {e: set() for e in candidates}, {}
    for t in range(T):
        c = rows[t]
        held = [e for e in edges_of(c) if e in candidates]
        if not held:
            continue
        if any(i >= V for i in c):
            for e in held:
                said[e].add("id")
            continue
        w = best(held if among_candidates else edges_of(c))
        for e in held:
            if e != w:
                said[e].add("lost")
        if w not in candidates:
            continue
        winner[t] = w
        p = xyz[c]
        s = _orient(p)
        lo, hi = xyz[w[0]], xyz[w[1]]
        with np.errstate(invalid="ignore", over="ignore"):
            mid = ((lo + hi) + (lo + hi)) * np.float32(0.25)
        flat = s == 0
        for end in w:
            q = p.copy()
            q[c.index(end)] = mid
            flat = flat or _orient(q) != s
        if flat:
            said[w].add("flat")
    for f in range(len(faces)):
        if face_tets[f, 1] != -1:
            continue
        ids = [int(i) for i in faces[f].view(np.uint32)]
        for k in range(3):
            e = (min(ids[k], ids[(k + 1) % 3]), max(ids[k], ids[(k + 1) % 3]))
            if e in candidates:
                said[e].add("hull")
    order = ("id", "hull", "lost", "flat") if hull_before_lost else ("id", "lost", "hull", "flat")
    verdict = {e: next((r for r in order if r in said[e]), "accepted") for e in candidates}
    accepted = sorted(e for e in candidates if verdict[e] == "accepted")
    rank = {e: j for j, e in enumerate(accepted)}
    vertices = [list(v) for v in xyz]
    for lo, hi in accepted:
        with np.errstate(invalid="ignore", over="ignore"):
            vertices.append(list(((xyz[lo] + xyz[hi]) + (xyz[lo] + xyz[hi])) * np.float32(0.25)))
    out, appended, parent, bisected = [list(r) for r in rows], [], list(range(T)), np.zeros(T, np.uint8)
    for t in range(T):
        w = winner.get(t)
        if w is None or verdict[w] != "accepted":
            continue
        bisected[t] = 1
        first, second = (w[1], w[0]) if hi_in_place else (w[0], w[1])
        c = rows[t]
        out[t] = [V + rank[w] if i == c.index(first) else v for i, v in enumerate(c)]
        appended.append([V + rank[w] if i == c.index(second) else v for i, v in enumerate(c)])
        parent.append(t)
    count = lambda r: sum(1 for e in candidates if verdict[e] == r)           # noqa: E731
    counters = [int(np.count_nonzero(select)), asked_id, asked_flat, len(candidates), count("id"), count("hull"), count("lost"),
                count("flat"), len(accepted), int(bisected.sum())]
    return {"vertices": np.array(vertices, np.float32).reshape(-1, 3), "cells": np.array(out + appended, np.uint32).view(np.int32).reshape(-1, 4),
            "cell_parent": np.array(parent, np.int32), "edge_vertices": np.array(accepted, np.uint32).view(np.int32).reshape(-1, 2),
            "bisected": bisected, "counters": np.array(counters, np.uint32), "nominated": nominated, "verdict": verdict}


def _same(a, want):
    return all(a[k].shape == want[k].shape and np.array_equal(ec.bits(a[k]), ec.bits(want[k]))
               for k in ("vertices", "cells", "cell_parent", "edge_vertices", "bisected", "counters"))


@pytest.mark.parametrize("name", ec.names() + ["soup_65_third", "soup_257_all"])
def test_restatement_equals_the_statement(scenes, name):
    assert _same(_restate(ec.case(scenes, name)), ec.statement(scenes, name)), name


def test_mutations_of_the_rule_are_rejected_by_named_cases(scenes):
    mutations = {
        "priority without the key tie-break": ("grid_4_all", dict(key_tie=False)),
        "winner taken among all edges instead of candidates": ("random_300_30pct", dict(among_candidates=False)),
        "precedence swapped": ("random_300_30pct", dict(hull_before_lost=False)),
        "child slots swapped": ("ring_sound", dict(hi_in_place=False)),
    }
    for what, (name, kw) in mutations.items():
        case, want = ec.case(scenes, name), ec.statement(scenes, name)
        assert not _same(_restate(case, **kw), want), f"{what}: not rejected by {name}"


# --------------------------------------------------------------------------------------------------------------- structure
def check_structure(oracle, case, s, name):
    """the split mesh s of the conforming mesh `case` (also used on the generations below)"""
    xyz, cells, select = case[:3]
    V, T, Kv, Kt = len(xyz), len(cells), s["num_new"], s["num_rows"]
    assert Kv > 0 and Kt >= Kv and s["cells"].shape == (T + Kt, 4) and s["vertices"].shape == (V + Kv, 3)
    oracle.build_faces(np.ascontiguousarray(s["cells"]))                      # raises on a face in three tetrahedra: conforming
    assert ec.hull_faces(s["cells"]) == ec.hull_faces(cells)                  # the hull-face set is the input's exactly
    parent, bis = s["cell_parent"].astype(np.int64), np.nonzero(s["bisected"])[0]
    assert np.array_equal(parent, np.concatenate([np.arange(T), bis])) and np.array_equal(np.diff(s["tet_offsets"].astype(np.int64)), s["bisected"])
    untouched = np.setdiff1d(np.arange(T), bis)
    assert np.array_equal(s["cells"][untouched], cells[untouched]) and np.array_equal(bits32(s["vertices"][:V]), bits32(xyz))
    # children: the slot of hi / lo replaced by the new vertex, the other slots in their stored order
    j = s["tet_edge"][bis].astype(np.int64)
    lo, hi = s["edge_vertices"][j, 0], s["edge_vertices"][j, 1]
    child0, child1, old = s["cells"][bis], s["cells"][T:], cells[bis]
    assert np.array_equal(child0, np.where(old == hi[:, None], V + j[:, None], old))
    assert np.array_equal(child1, np.where(old == lo[:, None], V + j[:, None], old))
    assert ((old == lo[:, None]).sum(1) == 1).all() and ((old == hi[:, None]).sum(1) == 1).all()
    # accepted edges share no row: every row holds at most one, and the rows that hold one are the bisected rows
    accepted = {tuple(e) for e in s["edge_vertices"].tolist()}
    held = np.array([sum((min(r[a], r[b]), max(r[a], r[b])) in accepted for a, b in EDGE_CORNERS) for r in cells.tolist()])
    assert held.max() == 1 and np.array_equal(held, s["bisected"])
    # stored orientations are kept
    g = ec.geometry()
    before = g.tet_orient(_t(xyz), _t(cells)).numpy()
    after = g.tet_orient(_t(s["vertices"]), _t(s["cells"])).numpy()
    assert np.array_equal(after, before[parent]) and np.all(before[bis] != 0)
    # Each child's volume is half its parent's.  The signed volume is affine in one corner, with gradient n = the cross product of
    # two edges of the opposite face; child 0 is the parent with p_hi moved to the midpoint m~, so vol(child 0) - vol / 2 =
    # n . (m~ - m) exactly, m the exact midpoint.  m~ = ((a + b) + (a + b)) * 0.25f: the sum rounds once, the doubling and the quarter
    # are exact, so |m~ - m| <= u |a + b| / 2 <= u M per coordinate, M = max |coordinate|.  The bound asked for is 2 u M |n|_1: one
    # u M |n|_1 for that rounding and as much for the float64 evaluation of the two determinants (below 20 2^-53 M L^2 with L the
    # longest edge), which it covers wherever |n|_1 >= 20 2^-29 L^2 -- every face that is not a needle of aspect 10^-7, asserted.
    p64, c64 = xyz.astype(np.float64), s["vertices"].astype(np.float64)
    vol = ec.vol6(p64[old])
    M = np.abs(p64[old]).max((1, 2))
    L = np.linalg.norm(p64[old][:, :, None] - p64[old][:, None], axis=-1).max((1, 2))
    worst = 0.0
    for child, moved in ((child0, hi), (child1, lo)):
        rest = np.stack([row[row != m] for row, m in zip(old, moved)])         # the opposite face, [n, 3]
        q = p64[rest]
        n1 = np.abs(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])).sum(1)
        assert np.all(n1 >= 20 * 2.0 ** -29 * L * L)
        err, bound = np.abs(ec.vol6(c64[child]) - vol / 2), 2 * ec.U * M * n1
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
    print(name, "K_v", Kv, "K_t", Kt, "largest |child volume - parent / 2| / bound", worst)
    return worst


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_asked_rows_are_explained(case, s):
    """every asked row that is not bisected is explained by a counter: it has an id >= V, or is flat, or the edge it nominated was
    refused for one of the four reasons; a row whose nominated edge was accepted IS bisected"""
    r = _restate(case)
    select, c = case[2], dict(zip(ec.COUNTERS, s["counters"].tolist()))
    asked = np.nonzero(select)[0]
    assert len(asked) == c["asked"] == c["asked_refused_id"] + c["asked_refused_flat"] + len(r["nominated"])
    assert c["candidates"] == c["refused_id"] + c["refused_hull"] + c["refused_lost"] + c["refused_flat"] + c["accepted"]
    reasons = {"id": 0, "hull": 0, "lost": 0, "flat": 0, "accepted": 0}
    for e, v in r["verdict"].items():
        reasons[v] += 1
    assert [reasons[k] for k in ("id", "hull", "lost", "flat", "accepted")] == s["counters"].tolist()[4:9]
    for t, e in r["nominated"].items():
        assert bool(s["bisected"][t]) or r["verdict"][e] != "accepted", t
        if r["verdict"][e] == "accepted":
            assert s["edge_vertices"][s["tet_edge"][t]].tolist() == list(e)


@pytest.mark.parametrize("name", ec.MESHES)
def test_split_mesh_structure(scenes, oracle, name):
    case, s = ec.case(scenes, name), ec.statement(scenes, name)
    check_structure(oracle, case, s, name)
    check_asked_rows_are_explained(case, s)


# ------------------------------------------------------------------------------------------------------------ preservation
def field_bound_terms(xyz, cells, field, rows):
    """per bisected parent `rows` of the mesh: (F0, gradient, p0) of its float64 interpolant and B = 2 u max|F| + |grad P|_1 2 u
    max|coordinate| [n, field rows], the bound on |F~_m - P(m~)| at the new vertex (see test_split_field_is_the_parent_field)"""
    F0, grad, p0 = sc.parent_interpolant(xyz, cells[rows], field)
    maxF = np.abs(field.astype(np.float64).T[cells[rows]]).max(1)
    M = np.abs(xyz.astype(np.float64)[cells[rows]]).max((1, 2))
    return F0, grad, p0, 2 * ec.U * maxF + np.abs(grad).sum(2) * 2 * ec.U * M[:, None]


def field_fraction(case, s, field, new_field):
    """the largest |child interpolant - parent interpolant| / bound over the corners and the centroid of every child, none skipped"""
    xyz, cells = case[:2]
    T = len(cells)
    bis = np.nonzero(s["bisected"])[0]
    F0, grad, p0, B = field_bound_terms(xyz, cells, field, bis)
    j = s["tet_edge"][bis].astype(np.int64)
    new = len(xyz) + j
    m = s["vertices"].astype(np.float64)[new]
    P_m = F0 + np.einsum("nra,na->nr", grad, m - p0)                          # the parent's interpolant at the ROUNDED midpoint
    F_m = new_field.astype(np.float64).T[new]
    worst = 0.0
    for child in (s["cells"][bis], s["cells"][T:]):
        is_new = child == new[:, None]
        assert (is_new.sum(1) == 1).all()
        cf = new_field.astype(np.float64).T[child]                            # [n, 4, rows]: the child's corner values
        pf = np.where(is_new[:, :, None], P_m[:, None], cf)                   # the parent's interpolant there: P is the field at an old corner
        assert np.array_equal(np.where(is_new[:, :, None], 0, cf), np.where(is_new[:, :, None], 0, field.astype(np.float64).T[np.minimum(child, len(xyz) - 1)]))
        for lam_m, child_value, parent_value in ((is_new[:, :, None] * 1.0, cf, pf),
                                                 (np.full((len(bis), 1, 1), 0.25), cf.mean(1, keepdims=True), pf.mean(1, keepdims=True))):
            diff, bound = np.abs(child_value - parent_value), lam_m * B[:, None]
            assert np.all(diff <= bound)
            worst = max(worst, float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1), 0).max()))
    assert np.array_equal(F_m, new_field.astype(np.float64)[:, new].T) and len(bis) == s["num_rows"]
    return worst


@pytest.mark.parametrize("name", ec.MESHES)
def test_split_field_is_the_parent_field(scenes, name):
    """The piecewise-linear field of the split mesh is the parent's, up to the rounding of the midpoint and of the mean.

    Let P be the affine interpolant of one field row F on a bisected row, m the exact midpoint of its edge (lo, hi), m~ the fp32
    one, F~_m the new vertex's value.  A point of a child is x = sum_old l_j p_j + l_m m~ with barycentrics summing to 1; the
    child's interpolant there is sum l_j F_j + l_m F~_m, and P is affine, so P(x) = sum l_j F_j + l_m P(m~): the difference is
    EXACTLY l_m (F~_m - P(m~)).  F~_m = ((F_lo + F_hi) + (F_lo + F_hi)) * 0.25f: the sum rounds once, the doubling and the quarter
    are exact, so |F~_m - P(m)| <= u |F_lo + F_hi| / 2 <= u max|F|, and per coordinate |m~ - m| <= u max|coordinate|, hence
    |P(m~) - P(m)| <= |grad P|_1 u max|coordinate|.  The bound asserted is the one the rule was specified with,
        |difference| <= l_m (2 u max|F_parent| + |grad P|_1 2 u max|coordinate|),      u = 2^-24,
    twice that, with grad P from the parent in float64; l_m is 1 at the new vertex, 1/4 at the centroid and 0 at an old corner,
    where both sides are the same number.  Every bisected row, both children, four corners and the centroid; the largest
    fraction of the bound is printed (profiles/edge_split_errors.txt)."""
    g = ec.geometry()
    case, s = ec.case(scenes, name), ec.statement(scenes, name)
    field = ec.values_for(len(case[0]), 4, seed=7)
    worst = field_fraction(case, s, field, g.split_vertex_rows_statement(field, s["vertex_parents"]))
    print(name, "bisected rows", s["num_rows"], "largest difference / bound", worst)


def test_three_generations(edge_split_emul, tmp_path, scenes, oracle):
    """Three passes over the 30 % case with the selection carried as cat(select & ~bisected, zeros): at every generation the
    emulation equals the statement on the previous generation's output, the mesh keeps its structure, and the field's bound
    telescopes as in DESIGN.md section 4.18: at the centroid x of a generation-3 row, |I_3(x) - I_0(x)| <= sum_g B_g(the
    generation g - 1 ancestor of the row), B_g the one-generation bound at l_m = 1 where that ancestor was bisected and 0 where not."""
    g = ec.geometry()
    xyz, cells, select, faces, face_tets = ec.case(scenes, "random_300_30pct")
    field = ec.values_for(len(xyz), 4, seed=9)
    xyz0, cells0, field0 = xyz, cells, field
    hull0, open_rows, chain, bounds = ec.hull_faces(cells), [], [], []
    for generation in range(1, 4):
        case = (xyz, cells, select, faces, face_tets)
        s = g.split_edges_statement(*case)
        assert_equal(_run_emul(edge_split_emul, tmp_path, *case), s, f"generation {generation}")
        check_structure(oracle, case, s, f"generation {generation}")
        check_asked_rows_are_explained(case, s)
        new_field = g.split_vertex_rows_statement(field, s["vertex_parents"])
        print("generation", generation, "largest difference / bound", field_fraction(case, s, field, new_field))
        bis = np.nonzero(s["bisected"])[0]
        B = np.zeros((len(cells), field.shape[0]))
        B[bis] = field_bound_terms(xyz, cells, field, bis)[3]
        bounds.append(B)
        chain.append(s["cell_parent"].astype(np.int64))
        open_rows.append(int(np.count_nonzero(select)))
        select = np.concatenate([select & ~s["bisected"], np.zeros(s["num_rows"], np.uint8)])
        xyz, cells, field = s["vertices"], s["cells"], new_field
        faces, face_tets = ec.face_table(cells)
    assert ec.hull_faces(cells) == hull0 and open_rows[0] == 483 and open_rows[1] < open_rows[0] and open_rows[2] < open_rows[1]
    anc, total = np.arange(len(cells)), np.zeros((len(cells), field.shape[0]))
    for parent, B in zip(chain[::-1], bounds[::-1]):
        anc = parent[anc]
        total += B[anc]
    live = g.tet_orient(_t(xyz0), _t(cells0)).numpy()[anc] != 0                # (no flat row in this mesh)
    assert live.all()
    F0, grad, p0 = sc.parent_interpolant(xyz0, cells0[anc], field0)
    x = xyz.astype(np.float64)[cells].mean(1)
    diff = np.abs(field.astype(np.float64).T[cells].mean(1) - (F0 + np.einsum("nra,na->nr", grad, x - p0)))
    moved = total > 0
    print("three generations: rows", len(cells), "largest difference / telescoped bound", float((diff[moved] / total[moved]).max()))
    # a row none of whose ancestors was bisected has the generation-0 field: what is left is the float64 evaluation of P
    assert np.all(diff[moved] <= total[moved]) and np.all(diff[~moved] <= 64 * 2.0 ** -53 * np.abs(field0).max() * 64)
    vol0, vol3 = np.abs(ec.vol6(xyz0.astype(np.float64)[cells0])).sum(), np.abs(ec.vol6(xyz.astype(np.float64)[cells])).sum()
    assert abs(vol3 - vol0) <= 1e-12 * vol0


# ---------------------------------------------------------------------------------------------------------------- entries
def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_edge_split_count_tables\(int device, size_t num_vertices, size_t num_cells, const float \*xyz,\s*"
                     r"const uint32_t \*cells,\s*const uint8_t \*select, size_t num_faces, const uint32_t \*faces,\s*"
                     r"const uint32_t \*face_tets,\s*uint32_t \*tet_offsets, uint32_t \*tet_edge, uint8_t \*bisected,\s*"
                     r"uint32_t \*edge_vertices,\s*uint32_t \*counters, void \*stream\);", header)
    assert re.search(r"int\s+tn_edge_split_count\(tn_tracer_t tracer, size_t num_vertices, const float \*xyz, const uint8_t \*select,\s*"
                     r"uint32_t \*tet_offsets,\s*uint32_t \*tet_edge, uint8_t \*bisected, uint32_t \*edge_vertices,\s*"
                     r"uint32_t \*counters, void \*stream\);", header)
    assert re.search(r"int\s+tn_edge_split_emit\(size_t num_vertices, size_t num_cells, const float \*xyz, const uint32_t \*cells,\s*"
                     r"const uint32_t \*tet_offsets,\s*const uint32_t \*tet_edge, const uint32_t \*edge_vertices, size_t num_new,\s*"
                     r"size_t num_rows, float \*xyz_out,\s*uint32_t \*cells_out, uint32_t \*cell_parent, uint32_t \*vertex_parents,\s*"
                     r"void \*stream\);", header)
    assert "no reference counterpart" in header[header.index("Edge split"):header.index("int tn_edge_split_count_tables")]
    lib = _lib.load()
    for name in ("tn_edge_split_count", "tn_edge_split_count_tables", "tn_edge_split_emit"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert len(lib.tn_edge_split_count_tables.argtypes) == 15 and len(lib.tn_edge_split_count.argtypes) == 10
    assert len(lib.tn_edge_split_emit.argtypes) == 14
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert hasattr(ext, "split_edges") and hasattr(ext.TetrahedraTracer, "split_edges") and hasattr(ext.TetrahedraTracer, "edge_split_count")
    import inspect
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    assert inspect.signature(plugin.densify).parameters["method"].default == "centroid"
    core = (CSRC / "tn_edge_split_core.h").read_text()
    assert "split::mean4" in core and "guard::tet_orient" in core and "vol6" not in core   # reused, not restated
    assert "MAX_CELLS = split::MAX_CELLS" in core and ext.EDGE_SPLIT_MAX_CELLS == ec.geometry().SPLIT_MAX_CELLS == 1 << 30
    makefile = (CSRC / "Makefile").read_text()
    assert "tn_edge_split.hip" in makefile and "tn_edge_split_core.h" in makefile


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = 64                                                                    # a pointer that is never followed

    def count(V=5, T=2, F=3, xyz=x, cells=x, select=x, faces=x, face_tets=x, a=x, b=x, c=x, d=x, e=x):
        return lib.tn_edge_split_count_tables(0, V, T, xyz, cells, select, F, faces, face_tets, a, b, c, d, e, None)

    for kw in (dict(xyz=None), dict(cells=None), dict(select=None), dict(faces=None), dict(face_tets=None), dict(a=None), dict(b=None),
               dict(c=None), dict(d=None), dict(e=None), dict(T=0, F=0, a=None)):
        assert count(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert count(T=2 ** 30) != 0 and b"2^30" in lib.tn_last_error()
    assert count(V=2 ** 32 - 1) != 0 and b"vertices" in lib.tn_last_error()
    assert count(F=2 ** 32 - 1) != 0 and b"faces" in lib.tn_last_error()
    assert lib.tn_edge_split_count(None, 5, x, x, x, x, x, x, x, None) != 0   # no tracer

    def emit(V=5, T=4, xyz=x, cells=x, offsets=x, tet_edge=x, edges=x, Kv=1, Kt=3, a=x, b=x, c=x, d=x):
        return lib.tn_edge_split_emit(V, T, xyz, cells, offsets, tet_edge, edges, Kv, Kt, a, b, c, d, None)

    for kw in (dict(xyz=None), dict(cells=None), dict(offsets=None), dict(tet_edge=None), dict(edges=None), dict(a=None), dict(b=None),
               dict(c=None), dict(d=None)):
        assert emit(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert emit(Kv=5) != 0 and b"exceeds num_cells" in lib.tn_last_error()
    assert emit(Kt=5) != 0 and b"exceeds num_cells" in lib.tn_last_error()
    assert emit(V=2 ** 32 - 3, Kv=2) != 0 and b"vertices" in lib.tn_last_error()
    half = 2 ** 29
    assert emit(T=half, Kv=1, Kt=half) != 0 and b"2^30" in lib.tn_last_error()


def test_wrappers_refuse_host_tensors(scenes):
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    xyz, cells, select, faces, face_tets = (_t(a) for a in ec.case(scenes, "ring_sound"))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.split_edges(xyz, cells, select, faces, face_tets)
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    with pytest.raises(ValueError, match="method"):
        plugin.densify(None, select, method="face")


def test_statement_refuses_mismatched_inputs(scenes):
    g = ec.geometry()
    xyz, cells, select, faces, face_tets = ec.case(scenes, "ring_sound")
    with pytest.raises(ValueError, match="one entry per row"):
        g.split_edges_statement(xyz, cells, select[:3], faces, face_tets)
    with pytest.raises(ValueError, match="one row per face"):
        g.split_edges_statement(xyz, cells, select, faces, face_tets[:3])
