"""The Delaunay repair by bistellar flips on the CPU: the rule of csrc/tn_flip_core.h as the host emulation
of the kernels (tests/host/flip_emul.cpp), as the vectorised numpy statement (geometry.flip_faces_statement) and as a plain-loop
restatement below -- all three bit-equal on every case of tests/flip_cases.py --, the structure of the flipped mesh after every
round, exact arithmetic on what was flipped, convergence of the loop, the carry of per-tetrahedron values and the adapter.

The volume property is stated on the sum of |volume|: the rule fixes the slot order of the children, (x_k, y_k, d, e), so a child has
the orientation of (a, b, c, e), not that of the row it replaces, and a signed sum over rows of mixed stored orientation (what
scipy gives) is not an invariant of the rule."""
import ctypes
import importlib
import os
import re
import shutil
import struct
import subprocess
import types
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import flip_cases as fc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"
EMPTY = fc.EMPTY


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "flip_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe), str(ROOT / "tests" / "host" / "flip_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def flip_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, cells, faces, face_tets):
    V, T, F = len(xyz), len(cells), len(faces)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQ", V, T, F))
        for a, dtype in ((xyz, np.float32), (cells, np.int32), (faces, np.int32), (face_tets, np.int32)):
            f.write(np.ascontiguousarray(a, dtype).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    counters = np.frombuffer(raw, np.uint32, 10)
    K23, K32, at, out = int(counters[8]), int(counters[9]), 40, {"counters": counters}
    rows = T + K23 - K32
    for key, dtype, shape in (("tet_offsets", np.uint32, (T + 1,)), ("tet_flip", np.int32, (T,)), ("flipped", np.uint8, (T,)),
                              ("face_flip", np.int32, (F, 3)), ("cells", np.int32, (rows, 4)), ("cell_sources", np.int32, (rows, 3))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += np.dtype(dtype).itemsize * count
    assert at == len(raw)
    out.update(num_23=K23, num_32=K32, num_cells=rows)
    return out


def assert_equal(got, want, what):
    for key in ("num_23", "num_32", "num_cells"):
        assert got[key] == want[key], f"{what}: {key} {got[key]} vs {want[key]}"
    for key in fc.ARRAYS:
        assert got[key].shape == want[key].shape, f"{what}: {key} {got[key].shape} vs {want[key].shape}"
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), f"{what}: {key}"


CPU_SOUPS = fc.names(soups=True, grid_cap=False)[len(fc.FIXED):] + [f"soup_C_{fc.soup_edges()[-1]}"]


@pytest.mark.parametrize("name", fc.names() + CPU_SOUPS)
def test_emulated_kernels_equal_the_statement(flip_emul, tmp_path, scenes, name):
    assert_equal(_run_emul(flip_emul, tmp_path, *fc.case(scenes, name)), fc.statement(scenes, name), name)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: an id past the table,
    a NaN, every refusal, both flips, empty inputs, a face table that names rows past the cells"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ("bad_id", "nan", "bipyramid_23", "ring3_32", "ring4_unflippable", "ring3_missing_t2", "cospherical", "coplanar_edge",
                 "same_side", "same_side_coplanar", "shared_row", "nothing_violated", "no_tets", "moved_400", "soup_T_257"):
        assert_equal(_run_emul(exe, tmp_path, *fc.case(scenes, name)), fc.statement(scenes, name), name)
    xyz, cells, faces, face_tets = fc.case(scenes, "ring3_32")
    bad = np.array(face_tets)
    bad[bad[:, 1] >= 0, 1] = 7                                                 # rows past T: refused for the id, nothing is read
    want = fc.geometry().flip_faces_statement(xyz, cells, faces, bad)
    assert want["counters"].tolist() == [3, 0, 0, 3, 0, 0, 0, 0, 0, 0]
    assert_equal(_run_emul(exe, tmp_path, xyz, cells, faces, bad), want, "rows past T")


# ------------------------------------------------------------------------------------------------ what the cases are named for
EXPECTED = {   # interior, violated, verdict uncertain, refused id / invalid / uncertain / unflippable / lost, accepted 2-3, 3-2
    "bipyramid_23": [1, 1, 0, 0, 0, 0, 0, 0, 1, 0],
    "ring3_32": [3, 3, 0, 0, 0, 0, 0, 2, 0, 1],
    "ring3_missing_t2": [1, 1, 0, 0, 0, 0, 1, 0, 0, 0],
    "cospherical": [1, 0, 1, 0, 0, 0, 0, 0, 0, 0],
    "coplanar_edge": [1, 1, 0, 0, 0, 1, 0, 0, 0, 0],
    "same_side": [1, 1, 0, 0, 1, 0, 0, 0, 0, 0],
    "same_side_coplanar": [1, 1, 0, 0, 1, 0, 0, 0, 0, 0],
    "bad_id": [1, 0, 0, 1, 0, 0, 0, 0, 0, 0],
    "nan": [1, 0, 1, 0, 0, 0, 0, 0, 0, 0],
    "shared_row": [2, 2, 0, 0, 0, 0, 0, 1, 1, 0],
    "bipyramid_regular": [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    "no_tets": [0] * 10,
}


def test_the_cases_are_what_they_are_named_for(scenes):
    for name, want in EXPECTED.items():
        assert fc.statement(scenes, name)["counters"].tolist() == want, name
    c = fc.counters(scenes, "nothing_violated")
    assert c["interior"] > 2000 and c["violated"] == 0 and c["accepted_23"] + c["accepted_32"] == 0
    s = fc.statement(scenes, "nothing_violated")
    assert np.array_equal(s["cells"], fc.case(scenes, "nothing_violated")[1]) and not s["flipped"].any()
    # the ring of four: the face (x, y, d) -- ids (0, 1, 3) -- is a 3-2 candidate whose two neighbours across the axis differ
    xyz, cells, faces, face_tets = fc.case(scenes, "ring4_unflippable")
    f = faces.tolist().index([0, 1, 3])
    s = fc.statement(scenes, "ring4_unflippable")
    assert s["face_kind"][f] == fc.geometry().FLIP_K_UNFLIPPABLE and s["counters"][6] >= 1
    # the bipyramid: the convention of "good" is fixed here -- the axis crosses the inside of the triangle, all three o_k have the
    # sign of O(a, b, c, e), and the three children tile the two rows
    s, (xyz, cells, _, _) = fc.statement(scenes, "bipyramid_23"), fc.case(scenes, "bipyramid_23")
    assert s["cells"].tolist() == [[0, 1, 3, 4], [1, 2, 3, 4], [2, 0, 3, 4]] and s["cell_sources"].tolist() == [[0, 1, -1]] * 3
    p = xyz.astype(np.float64)
    assert np.isclose(np.abs(fc.vol6(p[s["cells"]])).sum(), np.abs(fc.vol6(p[cells])).sum(), rtol=1e-14)
    s = fc.statement(scenes, "ring3_32")
    assert s["num_cells"] == 2 and (s["cell_sources"] >= 0).all() and sorted(s["cell_sources"][0].tolist()) == [0, 1, 2]
    for name in fc.names(soups=True, grid_cap=False):
        if name.startswith("soup_"):
            _, what, n = name.split("_")
            c = fc.case(scenes, name)
            assert int(n) == {"T": len(c[1]), "F": len(c[2]), "C": fc.counters(scenes, name)["accepted_23"]}[what], name
    bt, blocks = fc.kernel_constants()
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.FLIP_GRID_LANES == bt * blocks and blocks <= 1024 and bt == 256


def test_every_counter_is_non_zero_in_a_named_case(scenes):
    seen = np.zeros(10, np.int64)
    for name in fc.FIXED:
        seen += fc.statement(scenes, name)["counters"] > 0
    assert (seen > 0).all(), seen


# ------------------------------------------------------------------------------------------------------- the rule in plain loops
def _sign(g, q):
    det, perm = g.orient_det(np.asarray(q, np.float64)[None])
    return 0 if not abs(det[0]) > g.ORIENT_BOUND * perm[0] else (1 if det[0] > 0 else -1)


def _restate(case, invalid_first=True, smallest_id=True, check_t2=True):
    """the rule face by face; the three switches are the mutations test_mutations... rejects"""
    g = fc.geometry()
    xyz, cells, faces, face_tets = case
    V, T, F = len(xyz), len(cells), len(faces)
    x = xyz.astype(np.float64)
    u32 = lambda a: [[int(v) & 0xFFFFFFFF for v in row] for row in np.asarray(a).tolist()]   # noqa: E731
    c, f, ft = u32(cells), u32(faces), u32(face_tets)
    slot = lambda row, ids: next((j for j in range(4) if row[j] not in ids), -1)   # noqa: E731
    tet_faces = [[EMPTY] * 4 for _ in range(T)]
    for i in range(F):
        for t in ft[i]:
            if t < T and slot(c[t], f[i]) >= 0:
                tet_faces[t][slot(c[t], f[i])] = i
    kind, third, apex = ["hull"] * F, [EMPTY] * F, [None] * F
    for i in range(F):
        t0, t1 = ft[i]
        if t1 == EMPTY:
            continue
        kind[i] = "id"
        if t0 >= T or t1 >= T or max(f[i] + c[t0] + c[t1]) >= V or slot(c[t0], f[i]) < 0 or slot(c[t1], f[i]) < 0:
            continue
        d, e = c[t0][slot(c[t0], f[i])], c[t1][slot(c[t1], f[i])]
        apex[i] = (d, e)
        ev = next((v for v in c[t1] if v not in c[t0]), c[t1][3])
        with np.errstate(invalid="ignore", over="ignore"):
            ins, ori = g.insphere_det(x[c[t0]][None], x[ev][None]), g.orient_det(x[c[t0]][None])
            if not (abs(ins[0][0]) > g.INSPHERE_BOUND * ins[1][0] and abs(ori[0][0]) > g.ORIENT_BOUND * ori[1][0]):
                kind[i] = "verdict_uncertain"
                continue
            if (ins[0][0] > 0) != (ori[0][0] > 0):
                kind[i] = "regular"
                continue
            a, b, cc = f[i]
            sd, se = _sign(g, x[[a, b, cc, d]]), _sign(g, x[[a, b, cc, e]])
            o = [_sign(g, x[[f[i][k], f[i][(k + 1) % 3], d, e]]) for k in range(3)]
        invalid, uncertain = sd == 0 or se == 0 or sd == se, 0 in o
        if invalid and (invalid_first or not uncertain):
            kind[i] = "invalid"
        elif uncertain:
            kind[i] = "uncertain"
        elif sum(v == se for v in o) == 3:
            kind[i] = 1
        elif sum(v == se for v in o) == 2:
            k = [v == se for v in o].index(False)
            z, want = f[i][(k + 2) % 3], {f[i][k], f[i][(k + 1) % 3], d, e}
            nb = []
            for row, t in ((c[t0], t0), (c[t1], t1)):
                gf = tet_faces[t][row.index(z)]
                nb.append(EMPTY if gf >= F else (ft[gf][1] if ft[gf][0] == t else ft[gf][0] if ft[gf][1] == t else EMPTY))
            if check_t2:
                ok = nb[0] == nb[1] and nb[0] < T and nb[0] not in (t0, t1) and set(c[nb[0]]) == want
            else:
                ok = nb[0] < T
            kind[i], third[i] = (2 + k, nb[0]) if ok else ("unflippable", EMPTY)
        else:
            kind[i] = "unflippable"
    claim = [None] * T
    for i in range(F):
        if isinstance(kind[i], int):
            for t in (*ft[i], third[i]):
                if t != EMPTY and (claim[t] is None or (i < claim[t] if smallest_id else i > claim[t])):
                    claim[t] = i
    accepted = [i for i in range(F) if isinstance(kind[i], int) and all(claim[t] == i for t in (*ft[i], third[i]) if t != EMPTY)]
    lost = sum(isinstance(k, int) for k in kind) - len(accepted)
    deleted = {third[i] for i in accepted if third[i] != EMPTY}
    position, n = {}, 0
    for t in range(T):
        position[t] = n
        n += t not in deleted
    K23 = sum(kind[i] == 1 for i in accepted)
    out, src = [None] * (n + K23), [None] * (n + K23)
    taken = {t for i in accepted for t in (*ft[i], third[i]) if t != EMPTY}
    for t in range(T):
        if t not in taken:
            out[position[t]], src[position[t]] = c[t], [t, EMPTY, EMPTY]
    rank = 0
    for i in accepted:
        d, e = apex[i]
        good = [k for k in range(3) if kind[i] == 1 or k != kind[i] - 2]
        places = [position[ft[i][0]], position[ft[i][1]]] + ([n + rank] if kind[i] == 1 else [])
        rank += kind[i] == 1
        for k, at in zip(good, places):
            out[at], src[at] = [f[i][k], f[i][(k + 1) % 3], d, e], [ft[i][0], ft[i][1], third[i]]
    names = ["interior", "violated", "verdict_uncertain", "id", "invalid", "uncertain", "unflippable"]
    count = {k: 0 for k in names}
    for k in kind:
        count["interior"] += k != "hull"
        count["violated"] += isinstance(k, int) or k in ("invalid", "uncertain", "unflippable")
        if k in count:
            count[k] += 1
    counters = [count[k] for k in names] + [lost, K23, len(accepted) - K23]
    as_i32 = lambda a, w: np.array(a, np.int64).astype(np.uint32).view(np.int32).reshape(-1, w)   # noqa: E731
    return {"counters": counters, "cells": as_i32(out, 4), "cell_sources": as_i32(src, 3), "accepted": accepted, "kind": kind,
            "third": third, "apex": apex}


def _same(r, s):
    return r["counters"] == s["counters"].tolist() and np.array_equal(r["cells"], s["cells"]) and np.array_equal(r["cell_sources"], s["cell_sources"])


@pytest.mark.parametrize("name", fc.names() + ["soup_T_65", "soup_F_257"])
def test_restatement_equals_the_statement(scenes, name):
    r, s = _restate(fc.case(scenes, name)), fc.statement(scenes, name)
    assert _same(r, s), name
    assert r["accepted"] == np.nonzero(s["face_flip"][:, 0])[0].tolist()


def test_mutations_of_the_rule_are_rejected_by_named_cases(scenes):
    """uncertain decided before invalid; the LARGEST face id wins a row; the third row taken without its checks"""
    for mutation, cases in ((dict(invalid_first=False), ("same_side_coplanar",)), (dict(smallest_id=False), ("ring3_32", "shared_row", "moved_400")),
                            (dict(check_t2=False), ("ring4_unflippable", "moved_400"))):
        for name in cases:
            assert not _same(_restate(fc.case(scenes, name), **mutation), fc.statement(scenes, name)), (mutation, name)


# --------------------------------------------------------------------------------------------------------------- structure
def check_round(oracle, case, s, name):
    """one round s = flip_faces_statement(case) on a conforming mesh"""
    g = fc.geometry()
    xyz, cells, faces, face_tets = case
    T, K23, K32 = len(cells), s["num_23"], s["num_32"]
    new = s["cells"]
    assert new.shape == (T + K23 - K32, 4) and s["num_cells"] == len(new)
    # conforming: no face in more than two rows (oracle.build_faces raises on one); the hull-face set is the input's exactly
    oracle.build_faces(np.ascontiguousarray(new))
    tri = np.sort(np.concatenate([new[:, [1, 2, 3]], new[:, [0, 2, 3]], new[:, [0, 1, 3]], new[:, [0, 1, 2]]]), 1)
    assert np.unique(tri, axis=0, return_counts=True)[1].max() <= 2
    assert fc.hull_faces(new) == fc.hull_faces(cells)
    # the volume
    p = xyz.astype(np.float64)
    before, after = np.abs(fc.vol6(p[cells])).sum(), np.abs(fc.vol6(p[new])).sum()
    assert abs(after - before) <= 64 * 2.0 ** -53 * before * max(1, np.log2(len(cells) + 1)), (name, before, after)
    # accepted flips share no row; flipped = their rows; an untouched row is copied to its offset
    ff, ft = s["face_flip"].astype(np.int64), face_tets.astype(np.int64)
    acc = np.nonzero(ff[:, 0])[0]
    rows = np.concatenate([ft[acc, 0], ft[acc, 1], ff[acc, 1][ff[acc, 0] >= 2]])
    assert len(np.unique(rows)) == len(rows) == 2 * K23 + 3 * K32
    flipped = np.zeros(T, bool)
    flipped[rows] = True
    assert np.array_equal(flipped, s["flipped"].astype(bool)) and np.array_equal(s["tet_flip"] >= 0, flipped)
    keep = np.nonzero(~flipped)[0]
    off = s["tet_offsets"].astype(np.int64)
    assert np.array_equal(new[off[keep]], cells[keep]) and np.array_equal(s["cell_sources"][off[keep]], np.stack([keep, -1 + 0 * keep, -1 + 0 * keep], 1))
    assert off[-1] == T - K32
    # every new row has a certain orientation, with the sign of its siblings
    src = s["cell_sources"].astype(np.int64)
    fresh = np.nonzero(src[:, 1] >= 0)[0]
    assert len(fresh) == 3 * K23 + 2 * K32
    q = p[new[fresh]]
    with np.errstate(invalid="ignore"):
        sign = g._orient_sign(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    assert (sign != 0).all()
    for t0 in np.unique(src[fresh, 0]):
        assert len(set(sign[src[fresh, 0] == t0].tolist())) == 1
    # the children lie inside the union of their sources: as much volume in as out, flip by flip
    vol_new, vol_old = np.abs(fc.vol6(p[new])), np.abs(fc.vol6(p[cells]))
    for i in acc:
        mine = fresh[src[fresh, 0] == ft[i, 0]]
        olds = [ft[i, 0], ft[i, 1]] + ([ff[i, 1]] if ff[i, 0] >= 2 else [])
        assert np.isclose(vol_new[mine].sum(), vol_old[olds].sum(), rtol=1e-9), (name, i)
    # every violated face is flipped or explained by a refusal
    c = dict(zip(fc.COUNTERS, s["counters"].tolist()))
    assert c["violated"] == c["refused_invalid"] + c["refused_uncertain"] + c["refused_unflippable"] + c["refused_lost"] + K23 + K32
    want = g.delaunay_face_statement(cells, face_tets, xyz)["counters"]
    assert [c["interior"], c["violated"], c["verdict_uncertain"]] == want[:3].tolist() and c["refused_id"] == 0
    return c


@pytest.mark.parametrize("name", fc.MESHES)
def test_flipped_mesh_structure(scenes, oracle, name):
    c = check_round(oracle, fc.case(scenes, name), fc.statement(scenes, name), name)
    assert c["accepted_23"] + c["accepted_32"] > 0


def _circumsphere_holds(p, e):
    """exact: is e strictly inside the sphere through the four points p (rows of Fractions)?"""
    a = [[2 * (p[i][k] - p[0][k]) for k in range(3)] for i in (1, 2, 3)]
    b = [sum(p[i][k] ** 2 - p[0][k] ** 2 for k in range(3)) for i in (1, 2, 3)]
    det3 = lambda m: (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])   # noqa: E731
                      + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    d = det3(a)
    assert d != 0
    centre = [det3([[b[r] if k == col else a[r][k] for k in range(3)] for r in range(3)]) / d for col in range(3)]
    r2 = sum((p[0][k] - centre[k]) ** 2 for k in range(3))
    return sum((e[k] - centre[k]) ** 2 for k in range(3)) < r2


@pytest.mark.parametrize("name", ("bipyramid_23", "ring3_32", "shared_row", "moved_400", "moved_400_edge_split"))
def test_every_accepted_face_is_violated_in_exact_arithmetic(scenes, name):
    xyz, cells, faces, face_tets = fc.case(scenes, name)
    s = fc.statement(scenes, name)
    exact = [[Fraction(float(v)) for v in row] for row in xyz]
    acc = np.nonzero(s["face_flip"][:, 0])[0]
    assert len(acc)
    for i in acc:
        t0, t1 = face_tets[i]
        e = next(v for v in cells[t1].tolist() if v not in cells[t0].tolist())
        assert _circumsphere_holds([exact[v] for v in cells[t0]], exact[e]), (name, i)


# --------------------------------------------------------------------------------------------------------------- the loop
def test_the_loop_converges_on_the_moved_mesh(scenes, oracle):
    """The cap is a condition: at most 1 % of the initially violated faces remain, and every one that does is counted as
    unflippable or uncertain.  (Measured on this input: 332 violated faces at the start, 0 after 5 rounds.)"""
    g = fc.geometry()
    xyz, cells = fc.moved_mesh()
    r = fc.repaired()
    first, last = r["rounds"][0].tolist(), r["rounds"][-1].tolist()
    print("violated at the start", first[1], "rounds", r["num_rounds"], "left", last[1], "unflippable", last[6], "uncertain", last[5])
    assert first[1] > 0.03 * first[0] and r["num_rounds"] < 32 and last[8] + last[9] == 0
    assert last[1] == last[5] + last[6] and last[4] == 0 and last[7] == 0
    assert 100 * last[1] <= first[1]
    assert r["violated"] == last[1] and r["unflippable"] == last[6]
    # the monitor's own statement reports the same remaining count
    faces, face_tets = fc.face_table(r["cells"])
    assert g.delaunay_face_statement(r["cells"], face_tets, xyz)["counters"][1] == last[1]
    # every round on the way keeps the structure; the composed sources partition the volume they came from
    now = np.array(cells)
    for n in range(r["num_rounds"]):
        case = (xyz, now, *fc.face_table(now))
        s = g.flip_faces_statement(*case)
        assert s["counters"].tolist() == r["rounds"][n].tolist()
        check_round(oracle, case, s, f"round {n}")
        now = s["cells"]
    assert np.array_equal(now, r["cells"]) and fc.hull_faces(now) == fc.hull_faces(cells)
    src = r["cell_sources"]
    assert len(src) == len(now) and (src[:, 0] != EMPTY).all() and set(src[src != EMPTY].tolist()) == set(range(len(cells)))
    assert np.all((np.diff(src, axis=1) > 0) | (src[:, 1:] == EMPTY))


@pytest.mark.parametrize("name,rounds", (("moved_400_centroid_split", 17), ("moved_400_edge_split", 10)))
def test_the_loop_converges_on_the_split_meshes(scenes, name, rounds):
    """what one centroid-split and one edge-split round leave of the moved mesh: the same condition, at most 1 % of the initially
    violated faces remain and each is counted as unflippable or uncertain (on these inputs: none remain)"""
    g = fc.geometry()
    xyz, cells, _, _ = fc.case(scenes, name)
    r = g.flip_to_delaunay_statement(xyz, cells, fc.face_table)
    first, last = r["rounds"][0].tolist(), r["rounds"][-1].tolist()
    print(name, "violated at the start", first[1], "rounds", r["num_rounds"], "left", last[1])
    assert first[1] > 0.1 * first[0] and r["num_rounds"] == rounds and last[8] + last[9] == 0
    assert last[1] == last[5] + last[6] and last[4] == 0 and last[7] == 0 and 100 * last[1] <= first[1]
    faces, face_tets = fc.face_table(r["cells"])
    assert g.delaunay_face_statement(r["cells"], face_tets, xyz)["counters"][1] == last[1]
    assert fc.hull_faces(r["cells"]) == fc.hull_faces(cells)
    p = xyz.astype(np.float64)
    before, after = np.abs(fc.vol6(p[cells])).sum(), np.abs(fc.vol6(p[r["cells"]])).sum()
    assert abs(after - before) <= 1e-12 * before


def test_max_rounds_stops_the_loop(scenes):
    g = fc.geometry()
    xyz, cells = fc.moved_mesh()
    r = g.flip_to_delaunay_statement(xyz, cells, fc.face_table, max_rounds=2)
    full = fc.repaired()
    assert r["num_rounds"] == 2 and len(r["rounds"]) == 3 and [a.tolist() for a in r["rounds"]] == [a.tolist() for a in full["rounds"][:3]]
    r = g.flip_to_delaunay_statement(xyz, cells, fc.face_table, max_rounds=0)
    assert r["num_rounds"] == 0 and np.array_equal(r["cells"], cells) and r["violated"] == full["rounds"][0][1]


def test_flip_tet_values_is_conservative(scenes):
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    g = fc.geometry()
    for name in ("moved_400", "ring3_32", "bipyramid_23", "no_tets"):
        s, T = fc.statement(scenes, name), len(fc.case(scenes, name)[1])
        values = np.abs(np.random.default_rng(4).normal(size=T)).astype(np.float32)
        values[::7] = 0.0
        got = ext.flip_tet_values(torch.from_numpy(values), torch.from_numpy(np.array(s["cell_sources"]))).numpy()
        assert np.array_equal(fc.bits(got), fc.bits(g.flip_tet_values_statement(values, s["cell_sources"])))
        src = s["cell_sources"].astype(np.int64)
        for k in range(3):
            has = src[:, k] >= 0
            assert np.all(got[has] >= values[src[has, k]])
        assert np.array_equal(got[src[:, 1] < 0], values[src[src[:, 1] < 0, 0]])          # an untouched row keeps its value
    # the composition of the sources: torch and numpy agree
    full = fc.repaired()
    xyz, cells = fc.moved_mesh()
    now, sources = np.array(cells), None
    for n in range(full["num_rounds"]):
        s = g.flip_faces_statement(xyz, now, *fc.face_table(now))
        sources = ext.compose_cell_sources(sources, torch.from_numpy(np.array(s["cell_sources"])))
        now = s["cells"]
    want = np.where(full["cell_sources"] == EMPTY, -1, full["cell_sources"])
    assert np.array_equal(sources.numpy(), want)


# ------------------------------------------------------------------------------------------------------------------- adapter
class _FlipTracer:
    """test_delaunay's recording tracer with flip_to_delaunay"""
    supports_flip = True

    def __new__(cls, vertices, cells, counters, flips):
        from test_delaunay import _RecordingTracer

        class Tracer(_RecordingTracer):
            supports_flip = True

            def flip_to_delaunay(self, xyz=None, tet_values=(), max_rounds=32):
                self.calls.append(("flip", xyz, tuple(tet_values)))
                rounds, left = flips.pop(0)
                out_cells = self.tetrahedra_cells
                if rounds:
                    out_cells = torch.full((4, 4), 2, dtype=torch.int32)
                    self.load_tetrahedra(self.tetrahedra_vertices, out_cells, refittable=self._refittable)
                return {"cells": out_cells, "tet_values": [torch.full((len(out_cells),), 3.0) for _ in tet_values], "num_rounds": rounds,
                        "rounds": [[100, 9, 0, 0, 0, 0, 0, 0, 1, 0]] * rounds + [[100, left, 0, 0, 0, 0, left, 0, 0, 0]], "violated": left,
                        "unflippable": left}
        return Tracer(vertices, cells, counters)


def _model(cells, **config):
    return types.SimpleNamespace(tetrahedra_cells=cells, tetrahedra_occupancy=torch.tensor([0.0, 1.0, 0.0]),
                                 config=types.SimpleNamespace(num_tetrahedra_cells=3, **config))


def test_adapter_call_order_with_and_without_delaunay_repair():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    names = lambda tracer: [c[0] for c in tracer.calls]   # noqa: E731
    v = torch.nn.Parameter(torch.zeros(4, 3))
    cells = torch.zeros(3, 4, dtype=torch.int32)
    # absent: today's calls exactly
    tracer, model = _FlipTracer(v, cells, [[100, 9, 0, 0]], []), _model(cells)
    assert plugin._monitor_delaunay(tracer, model, 0.05, False) and names(tracer) == ["check", "retriangulate", "load"]
    assert model._tn_retriangulations == 1 and not hasattr(model, "_tn_flip_repairs")
    # "flip", and the flips bring the share under the threshold: no Qhull; cells, occupancy and statistics follow
    tracer, model = _FlipTracer(v, cells, [[100, 9, 0, 0]], [(3, 1)]), _model(cells, delaunay_repair="flip")
    model._tn_tet_stats = torch.ones(3, 3, dtype=torch.int64)
    model.get_tetrahedra_tracer = lambda: tracer
    assert plugin._monitor_delaunay(tracer, model, 0.05, False) and names(tracer) == ["check", "flip", "load"]
    assert tracer.calls[1][1] is None and torch.equal(tracer.calls[1][2][0], torch.tensor([0.0, 1.0, 0.0]))
    assert model.tetrahedra_cells is tracer.tetrahedra_cells and model.tetrahedra_cells.shape == (4, 4)
    assert model.tetrahedra_occupancy.tolist() == [3.0] * 4 and model.config.num_tetrahedra_cells == 4
    assert model._tn_flip_repairs == 1 and not hasattr(model, "_tn_retriangulations")
    assert model._tn_tet_stats.shape[0] == 4 and not model._tn_tet_stats.any()          # reset, as after a split
    # "flip", but what is left is still above: the re-triangulation after the flips, on the carried occupancy
    tracer, model = _FlipTracer(v, cells, [[100, 9, 0, 0]], [(2, 7)]), _model(cells, delaunay_repair="flip")
    assert plugin._monitor_delaunay(tracer, model, 0.05, False) and names(tracer) == ["check", "flip", "load", "retriangulate", "load"]
    assert tracer.calls[3][2][0].tolist() == [3.0] * 4 and model._tn_flip_repairs == 1 and model._tn_retriangulations == 1
    # "flip", nothing flippable and above: Qhull alone; under the threshold: nothing at all
    tracer, model = _FlipTracer(v, cells, [[100, 9, 0, 0]], [(0, 9)]), _model(cells, delaunay_repair="flip")
    assert plugin._monitor_delaunay(tracer, model, 0.05, False) and names(tracer) == ["check", "flip", "retriangulate", "load"]
    tracer, model = _FlipTracer(v, cells, [[100, 5, 0, 0]], []), _model(cells, delaunay_repair="flip")
    assert not plugin._monitor_delaunay(tracer, model, 0.05, False) and names(tracer) == ["check"]
    with pytest.raises(ValueError, match="delaunay_repair"):
        plugin._monitor_delaunay(_FlipTracer(v, cells, [[100, 9, 0, 0]], []), _model(cells, delaunay_repair="qhull"), 0.05, False)


# ---------------------------------------------------------------------------------------------------------------- entries
def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    for name in ("tn_flip_count_tables", "tn_flip_count", "tn_flip_emit", "tn_flip_emit_loaded"):
        assert re.search(r"int\s+" + name + r"\(", header) and name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    lib = _lib.load()
    assert len(lib.tn_flip_count_tables.argtypes) == 14 and len(lib.tn_flip_count.argtypes) == 9
    assert len(lib.tn_flip_emit.argtypes) == 13 and len(lib.tn_flip_emit_loaded.argtypes) == 9
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert hasattr(ext, "flip_faces") and hasattr(ext, "flip_tet_values") and hasattr(ext.TetrahedraTracer, "flip_to_delaunay")
    core = (CSRC / "tn_flip_core.h").read_text()
    assert "delaunay::orient_det" in core and "delaunay::face_verdict" in core and "double " not in core.split("#pragma once")[1]   # no new arithmetic
    g = fc.geometry()
    assert ext.FLIP_MAX_CELLS == g.SPLIT_MAX_CELLS == 1 << 30 and tuple(fc.COUNTERS) == g.FLIP_COUNTER_NAMES
    makefile = (CSRC / "Makefile").read_text()
    assert "tn_flip.hip" in makefile and "tn_flip_core.h" in makefile


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = 64                                                                    # a pointer that is never followed

    def count(V=5, T=2, F=3, xyz=x, cells=x, faces=x, face_tets=x, a=x, b=x, c=x, d=x, e=x):
        return lib.tn_flip_count_tables(0, V, T, xyz, cells, F, faces, face_tets, a, b, c, d, e, None)

    for kw in (dict(xyz=None), dict(cells=None), dict(faces=None), dict(face_tets=None), dict(a=None), dict(b=None), dict(c=None),
               dict(d=None), dict(e=None), dict(T=0, F=0, a=None)):
        assert count(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert count(T=2 ** 30) != 0 and b"2^30" in lib.tn_last_error()
    assert count(V=2 ** 32 - 1) != 0 and b"vertices" in lib.tn_last_error()
    assert count(F=2 ** 32 - 1) != 0 and b"faces" in lib.tn_last_error()
    assert lib.tn_flip_count(None, 5, x, x, x, x, x, x, None) != 0              # no tracer
    assert lib.tn_flip_emit_loaded(None, x, x, x, 1, 0, x, x, None) != 0

    def emit(T=7, F=9, cells=x, faces=x, face_tets=x, offsets=x, tet_flip=x, face_flip=x, K23=1, K32=1, a=x, b=x):
        return lib.tn_flip_emit(T, cells, F, faces, face_tets, offsets, tet_flip, face_flip, K23, K32, a, b, None)

    for kw in (dict(cells=None), dict(faces=None), dict(face_tets=None), dict(offsets=None), dict(tet_flip=None), dict(face_flip=None),
               dict(a=None), dict(b=None)):
        assert emit(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert emit(K23=10) != 0 and b"exceeds num_faces" in lib.tn_last_error()
    assert emit(K23=2, K32=2) != 0 and b"more rows" in lib.tn_last_error()
    assert emit(T=2 ** 30 - 1, F=2 ** 30, K23=1, K32=0) != 0 and b"2^30" in lib.tn_last_error()


def test_wrappers_refuse_host_tensors(scenes):
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    xyz, cells, faces, face_tets = (torch.from_numpy(np.array(a)) for a in fc.case(scenes, "bipyramid_23"))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.flip_faces(xyz, cells, faces, face_tets)


def test_statement_refuses_mismatched_inputs(scenes):
    xyz, cells, faces, face_tets = fc.case(scenes, "bipyramid_23")
    with pytest.raises(ValueError, match="one row per face"):
        fc.geometry().flip_faces_statement(xyz, cells, faces, face_tets[:3])
