"""The isosurface refinement without a GPU (tn_isosurface_refine_*, csrc/tn_isosurface_refine.hip; the rule: DESIGN.md section
4.17).  Layers: tests/host/isosurface_refine_emul.cpp -- which drives the element functions of csrc/tn_isosurface_core.h, the bodies
of the kernels -- bit for bit against the numpy statement (geometry.isosurface_refine_statement) on every case of
tests/isosurface_refine_cases.py, plain and under the host sanitizers; no round = the extraction's own bits; the order of the
candidates; the selection rule on crafted densities; nesting; the a-priori residual bound on the analytic spheres; a plain-loop
restatement that rejects four mutations of the rule on named cases; the entries and the refusals.  (The kernels themselves:
tests/test_isosurface_refine_gpu.py.)"""
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
import isosurface_refine_cases as rc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"
C = rc.C


def _g():
    return ic.geometry()


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "isosurface_refine_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "isosurface_refine_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def refine_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, ev, values, level, rounds, dens=None, expect=0):
    """dens f32 [rounds, N, 7]: the densities given (kind 0); None: the emulation's own -(|p|^2) (kind 1)"""
    V, N = len(values), len(ev)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQQfI", V, N, rounds, 0 if dens is not None else 1, level, 0))
        f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
        f.write(np.ascontiguousarray(ev, np.int32).tobytes())
        f.write(np.ascontiguousarray(values, np.float32).tobytes())
        if dens is not None:
            f.write(np.ascontiguousarray(dens[:rounds], np.float32).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    if expect:
        assert r.returncode == expect, (r.returncode, r.stdout, r.stderr)
        return None
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    at, out = 0, {"vertex_indices": [], "barycentric": [], "brackets": [], "flags": []}
    for _ in range(rounds):
        out["vertex_indices"].append(np.frombuffer(raw, np.int32, 4 * C * N, at).reshape(N * C, 4))
        at += 16 * C * N
        out["barycentric"].append(np.frombuffer(raw, np.float32, 3 * C * N, at).reshape(N * C, 3))
        at += 12 * C * N
    for _ in range(rounds + 1):
        out["brackets"].append(np.frombuffer(raw, np.float32, 4 * N, at).reshape(N, 4))
        at += 16 * N
        out["flags"].append(np.frombuffer(raw, np.uint8, N, at))
        at += N
    out["edge_t"] = np.frombuffer(raw, np.float32, N, at)
    at += 4 * N
    out["positions"] = np.frombuffer(raw, np.float32, 3 * N, at).reshape(N, 3)
    at += 12 * N
    assert at == len(raw)
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(ic.bits(a), ic.bits(b))


def _assert_emul_is_statement(got, want, rounds, what, recorded=None):
    for r in range(rounds + 1):
        assert _same(got["brackets"][r], want["brackets"][r]), f"{what}: bracket after {r} rounds"
    assert _same(got["brackets"][-1], want["edge_bracket"]) and np.array_equal(got["flags"][-1], want["edge_frozen"]), what
    assert _same(got["edge_t"], want["edge_t"]) and _same(got["positions"], want["positions"]), what
    for r, (a, b, t) in enumerate(recorded or []):                            # what the statement asked its density for
        vi, bc = got["vertex_indices"][r], got["barycentric"][r]
        assert np.array_equal(vi, np.stack([a, b, a, a], 1)) and _same(bc[:, 0], t) and not bc[:, 1:].any(), (what, r)


def _recording(fn):
    calls = []

    def wrapped(a, b, t):
        calls.append((a.copy(), b.copy(), np.array(t, np.float32)))
        return fn(a, b, t)

    return wrapped, calls


CRAFTED_N = (0, 1, len(rc.NAMES), 3 * len(rc.NAMES) + 5)


@pytest.mark.parametrize("N", CRAFTED_N)
def test_emulation_equals_the_statement_on_crafted_densities(refine_emul, tmp_path, N):
    xyz, ev, values, level, dens = rc.crafted(N)
    for rounds in (0, 1, rc.ROUNDS):
        fn, calls = _recording(rc.replay(dens))
        want = _g().isosurface_refine_statement(xyz, ev, values, level, fn, rounds)
        got = _run_emul(refine_emul, tmp_path, xyz, ev, values, level, rounds, dens)
        _assert_emul_is_statement(got, want, rounds, f"crafted {N} x {rounds}", calls)
        assert len(calls) == rounds


@pytest.mark.parametrize("name", sorted(ic.SPHERES))
def test_emulation_equals_the_statement_on_the_spheres(refine_emul, tmp_path, scenes, name):
    xyz, _, values, level, s = rc.sphere_surface(scenes, name)
    for rounds in (0, 2, 8):
        fn, calls = _recording(rc.radial_density(xyz))
        want = _g().isosurface_refine_statement(xyz, s["edge_vertices"], values, level, fn, rounds)
        got = _run_emul(refine_emul, tmp_path, xyz, s["edge_vertices"], values, level, rounds)
        _assert_emul_is_statement(got, want, rounds, f"{name} x {rounds}", calls)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: ids past the table
    (every crafted set has them), one id past an EMPTY table, short and empty arrays, and a surface of some size"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for N in CRAFTED_N:
        xyz, ev, values, level, dens = rc.crafted(N)
        assert N < len(rc.NAMES) or (ev >= len(values)).any()
        want = _g().isosurface_refine_statement(xyz, ev, values, level, rc.replay(dens), rc.ROUNDS)
        _assert_emul_is_statement(_run_emul(exe, tmp_path, xyz, ev, values, level, rc.ROUNDS, dens), want, rc.ROUNDS, f"crafted {N}")
    # every id past the table, analytic densities (the candidates ask for vertex 0, which exists)
    xyz, ev, values, level, _ = rc.crafted(3, only="a_inside")
    far = np.array([[7, 9], [6, -2 ** 31], [-1, -1]], np.int32)                     # (as uint32: 2^31 and 2^32 - 1)
    want = _g().isosurface_refine_statement(xyz, far, values, level, rc.radial_density(xyz), 2)
    assert want["edge_frozen"].tolist() == [2, 2, 2] and not want["positions"].any()
    _assert_emul_is_statement(_run_emul(exe, tmp_path, xyz, far, values, level, 2), want, 2, "ids past the table")
    # no vertices at all: without rounds the ids are checked and nothing is read; with rounds the candidates would name vertex 0
    none = np.zeros((0, 3), np.float32)
    got = _run_emul(exe, tmp_path, none, far, none[:, 0], level, 0)
    assert got["flags"][0].tolist() == [2, 2, 2] and not got["positions"].any()
    _run_emul(exe, tmp_path, none, far, none[:, 0], level, 1, expect=3)
    xyz, _, values, level, s = rc.sphere_surface(scenes, "sphere_120")
    want = _g().isosurface_refine_statement(xyz, s["edge_vertices"], values, level, rc.radial_density(xyz), 3)
    _assert_emul_is_statement(_run_emul(exe, tmp_path, xyz, s["edge_vertices"], values, level, 3), want, 3, "sphere_120")
    _run_emul(exe, tmp_path, xyz, s["edge_vertices"], values, level, 9, expect=3)
    _run_emul(exe, tmp_path, xyz, s["edge_vertices"], values, float("nan"), 1, expect=3)


# ------------------------------------------------------------------------------------------------------------ no round
@pytest.mark.parametrize("name", ic.names(large=False))
def test_no_round_is_the_extraction(scenes, name):
    """rounds = 0 returns isosurface_statement's edge_t and positions bit for bit, the sign of a zero t included"""
    xyz, _, values, level, _ = ic.case(scenes, name)
    s = ic.statement(scenes, name)

    def never(*a):
        raise AssertionError("the density was asked for without a round")

    got = _g().isosurface_refine_statement(xyz, s["edge_vertices"], values, level, never, 0)
    assert _same(got["edge_t"], s["edge_t"]) and _same(got["positions"], s["positions"]), name
    assert not got["edge_frozen"].any() and len(got["brackets"]) == 1
    if name == "value_at_level":
        assert np.signbit(s["edge_t"]).all() and np.signbit(got["edge_t"]).all()      # (level - v_a) / negative = -0: kept


# ------------------------------------------------------------------------------------------------------------ the candidates
def test_candidates_are_ordered_inside_their_bracket():
    lo, hi = rc.order_brackets()
    assert len(lo) > 3e6 and (lo <= hi).all() and (lo >= 0).all() and (hi <= 1).all()
    assert (lo == hi).sum() >= 200000 and (np.nextafter(lo, np.float32(2)) == hi).sum() > 100000
    t = _g().isosurface_refine_candidates(lo, hi)
    full = np.concatenate([lo[:, None], t, hi[:, None]], 1)
    assert t.dtype == np.float32 and (np.diff(full, axis=1) >= 0).all()
    same = lo == hi
    assert (t[same] == lo[same, None]).all()
    # from (0, 1) every bracket is exact: t_j = j / 8, and after r rounds a multiple of 8^-r
    assert _g().isosurface_refine_candidates([0.0], [1.0])[0].tolist() == [j / 8 for j in range(1, 8)]
    core = (CSRC / "tn_isosurface_core.h").read_text()
    assert "REFINE_CANDIDATES = 7" in core and "REFINE_MAX_ROUNDS = 8" in core and "(float)j * 0.125f" in core
    assert _g().ISO_REFINE_CANDIDATES == 7 == C and _g().ISO_REFINE_MAX_ROUNDS == 8
    assert "REFINE_FROZEN = 1, REFINE_BAD_IDS = 2" in core and (_g().ISO_REFINE_FROZEN, _g().ISO_REFINE_BAD_IDS) == (1, 2)


# ------------------------------------------------------------------------------------------------------------ the selection
def _crafted_one(name, rounds):
    xyz, ev, values, level, dens = rc.crafted(1, only=name)
    out = _g().isosurface_refine_statement(xyz, ev, values, level, rc.replay(dens), rounds)
    return out, xyz, ev


def test_selection_on_crafted_densities():
    L = rc.LEVEL
    exp = {  # after one round: (t_lo, t_hi, s_lo, s_hi), flag
        "a_inside": ((0.5, 0.625, 0.3, 0.1), 0), "b_inside": ((0.25, 0.375, 0.0, 0.25), 0),
        "candidate_at_level": ((0.375, 0.5, L, -1.0), 0), "candidate_at_level_b_inside": ((0.25, 0.375, -1.0, L), 0),
        "two_changes": ((0.125, 0.25, 1.0, -1.0), 0), "three_changes": ((0.25, 0.375, -1.0, 1.0), 0),
        "first_interval": ((0.0, 0.125, 1.0, -1.0), 0), "last_interval": ((0.875, 1.0, 1.0, -1.0), 0),
        "inf_in_round_0": ((0.0, 1.0, -1.0, 1.0), 1), "nan_hides_a_change": ((0.0, 1.0, 1.0, -1.0), 1),
        "values_on_one_side": ((0.0, 1.0, 1.0, 0.5), 1), "bad_id": ((0.0, 1.0, 0.0, 0.0), 2),
        "below_big_is_kept": ((0.25, 0.375, 1.0, -1.0), 0),
    }
    for name, (bracket, flag) in exp.items():
        out, _, _ = _crafted_one(name, 1)
        assert out["edge_bracket"][0].tolist() == [float(np.float32(x)) for x in bracket] and out["edge_frozen"][0] == flag, name
    # a candidate at the level: the vertex sits on it (q = 0), from either side
    assert _crafted_one("candidate_at_level", 1)[0]["edge_t"][0] == 0.375
    assert _crafted_one("candidate_at_level_b_inside", 1)[0]["edge_t"][0] == 0.375
    # the second round of three_changes: the first change again
    assert _crafted_one("three_changes", 2)[0]["edge_bracket"][0].tolist() == [0.25 + 1 / 64, 0.25 + 2 / 64, -1.0, 1.0]
    # frozen for good: the bracket of the round before the bad candidate stays, although later rows would move it
    for name, at in (("nan_in_round_1", 1), ("big_in_round_2", 2), ("inf_in_round_0", 0)):
        outs = [_crafted_one(name, r)[0] for r in range(rc.ROUNDS + 1)]
        for r, out in enumerate(outs):
            assert out["edge_frozen"][0] == (1 if r > at else 0), (name, r)
            if r > at:
                assert _same(out["edge_bracket"], outs[at]["edge_bracket"]) and _same(out["positions"], outs[at]["positions"]), (name, r)
        assert not _same(outs[at]["edge_bracket"], outs[0]["edge_bracket"]) or at == 0
    # started frozen or with a bad id: the vertex is on the edge (an end of it), or at the origin
    out, xyz, ev = _crafted_one("values_on_one_side", 2)
    assert out["edge_t"][0] == 1.0 and _same(out["positions"][0], xyz[1])
    out, xyz, ev = _crafted_one("value_out_of_range", 2)
    assert out["edge_frozen"][0] == 1 and out["edge_t"][0] == 0.0 and _same(out["positions"][0], xyz[0])
    out, _, _ = _crafted_one("bad_id", 2)
    assert out["edge_t"][0] == 0.0 and not out["positions"].any()


def test_brackets_nest_and_keep_their_sides(scenes):
    sets = [rc.crafted(4 * len(rc.NAMES)) + (None,)]
    for name in sorted(ic.SPHERES):
        xyz, _, values, level, s = rc.sphere_surface(scenes, name)
        sets.append((xyz, s["edge_vertices"], values, level, None, rc.radial_density(xyz)))
    for xyz, ev, values, level, dens, fn in sets:
        out = _g().isosurface_refine_statement(xyz, ev, values, level, fn or rc.replay(dens), rc.ROUNDS)
        live = out["edge_frozen"] == 0
        for before, after in zip(out["brackets"], out["brackets"][1:]):
            assert (after[:, 0] >= before[:, 0]).all() and (after[:, 1] <= before[:, 1]).all() and (after[:, 0] <= after[:, 1]).all()
            assert ((after[live, 2] >= np.float32(level)) != (after[live, 3] >= np.float32(level))).all()
        width = out["edge_bracket"][live, 1] - out["edge_bracket"][live, 0]
        assert live.sum() > 0 and (width == np.float32(8.0 ** -rc.ROUNDS)).all()     # exact: every end is a multiple of 8^-rounds
        t = out["edge_t"][live]
        assert ((t >= out["edge_bracket"][live, 0]) & (t <= out["edge_bracket"][live, 1])).all()


# ------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("name", sorted(ic.SPHERES))
def test_refined_vertices_lie_on_the_sphere_within_the_bound(scenes, name):
    """the residual |D(p) - level| of every vertex, D = -(|x|^2) in float64, against the a-priori bound of
    isosurface_refine_cases.residual_bound; the enclosed volume is printed, not asserted: vertices on the surface give an inscribed
    polyhedron, whose volume can shrink"""
    xyz, _, values, level, s = rc.sphere_surface(scenes, name)
    ev = s["edge_vertices"]
    # D along an edge is a concave parabola in t; its ends lie on the two sides of the level, so it crosses once: no frozen edge,
    # no choice among crossings.  Checked: the float64 values of the ends straddle the float32 level.
    x = xyz.astype(np.float64)
    L = float(np.float32(level))
    da, db = rc.radial64(x[ev[:, 0]]), rc.radial64(x[ev[:, 1]])
    assert ((da >= L) != (db >= L)).all() and len(ev) > 30
    worst = {}
    for rounds in (0, 1, 2, 4, 8):
        out = _g().isosurface_refine_statement(xyz, ev, values, level, rc.radial_density(xyz), rounds)
        assert not out["edge_frozen"].any()
        bound, W = rc.residual_bound(xyz, ev, rounds)
        width = (out["edge_bracket"][:, 1].astype(np.float64) - out["edge_bracket"][:, 0])
        res = np.abs(rc.radial64(out["positions"]) - L)
        volume = ic.enclosed_volume(out["positions"], s["triangles"])
        worst[rounds] = res.max()
        print(f"{name} rounds {rounds}: vertices {len(ev)} max residual {res.max():.3e} max residual / bound {(res / bound).max():.3f} "
              f"max distance from the sphere {np.abs(np.linalg.norm(out['positions'].astype(np.float64), axis=1) - np.sqrt(-L)).max():.3e} "
              f"volume / sphere's {volume / (4 / 3 * np.pi * (-L) ** 1.5):.4f}")
        assert (width <= W).all() and (res <= bound).all(), (name, rounds)
        assert ic.closed_and_oriented(s["triangles"]) and volume > 0
    assert worst[2] < worst[0]


# -------------------------------------------------------------------------------------------- a restatement and its mutations
def _restate(xyz, ev, values, level, dens, rounds, first=True, at_level_inside=True, clamp=True, nan_freezes=True):
    """the rule as a plain loop over the vertices; the keywords are the four mutations"""
    f32 = np.float32
    L, V = f32(level), len(values)
    inside = (lambda s: s >= L) if at_level_inside else (lambda s: s > L)
    ts, ps = [], []
    with np.errstate(all="ignore"):
        for i, (a, b) in enumerate(np.ascontiguousarray(ev).view(np.uint32).tolist()):
            if a >= V or b >= V:
                ts.append(f32(0)), ps.append(np.zeros(3, f32))
                continue
            lo, hi, slo, shi = f32(0), f32(1), values[a], values[b]
            frozen = not (abs(float(slo)) < 2.0 ** 126 and abs(float(shi)) < 2.0 ** 126 and inside(slo) != inside(shi))
            for r in range(rounds):
                if frozen:
                    break
                s = dens[r, i]
                bad = [not abs(float(x)) < 2.0 ** 126 for x in s]
                if any(bad) and nan_freezes:
                    frozen = True
                    break
                w = hi - lo
                t = [lo] + [lo + f32(j) * f32(0.125) * w for j in range(1, 8)] + [hi]
                v = [slo] + list(s) + [shi]
                js = [j for j in range(8) if bool(inside(v[j])) != bool(inside(v[j + 1]))]
                if not js:
                    frozen = True
                    break
                j = js[0] if first else js[-1]
                lo, hi, slo, shi = t[j], t[j + 1], v[j], v[j + 1]
            q = (L - slo) / (shi - slo)
            m = q * (hi - lo)
            t = m if lo == 0 else lo + m
            if clamp:
                t = lo if not t >= lo else (hi if t > hi else t)
            ts.append(f32(t)), ps.append(xyz[a] + f32(t) * (xyz[b] - xyz[a]))
    return np.array(ts, f32), np.array(ps, f32).reshape(-1, 3)


def test_restatement_equals_the_statement_and_mutations_are_rejected():
    g = _g()
    xyz, ev, values, level, dens = rc.crafted(2 * len(rc.NAMES))
    want = g.isosurface_refine_statement(xyz, ev, values, level, rc.replay(dens), rc.ROUNDS)
    t, p = _restate(xyz, ev, values, level, dens, rc.ROUNDS)
    assert _same(t, want["edge_t"]) and _same(p, want["positions"])
    mutations = {
        "the last sign change instead of the first": ("two_changes", dict(first=False)),
        "> instead of >=": ("candidate_at_level", dict(at_level_inside=False)),
        "an unclamped final t": ("values_on_one_side", dict(clamp=False)),
        "a NaN treated as outside instead of freezing": ("nan_hides_a_change", dict(nan_freezes=False)),
    }
    for what, (name, kw) in mutations.items():
        xyz, ev, values, level, dens = rc.crafted(1, only=name)
        want = g.isosurface_refine_statement(xyz, ev, values, level, rc.replay(dens), 2)
        t, p = _restate(xyz, ev, values, level, dens, 2)
        assert _same(t, want["edge_t"]) and _same(p, want["positions"]), name
        t, p = _restate(xyz, ev, values, level, dens, 2, **kw)
        assert not (_same(t, want["edge_t"]) and _same(p, want["positions"])), f"{what}: not rejected by {name}"


# ---------------------------------------------------------------------------------------------------------------- entries
ENTRIES = ("tn_isosurface_refine_begin", "tn_isosurface_refine_points", "tn_isosurface_refine_select", "tn_isosurface_refine_vertices")


def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    block = header[header.index("Isosurface refinement"):header.index("int tn_isosurface_refine_begin")]
    assert "no reference counterpart" in block and "section 4.17" in block
    lib = _lib.load()
    for name, nargs in zip(ENTRIES, (8, 9, 7, 9)):
        assert re.search(rf"int\s+{name}\(", header) and name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
        assert len(getattr(lib, name).argtypes) == nargs
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib.SYMBOLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert {x.split()[-1] for x in exported.splitlines() if " T tn_" in x} == declared
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert hasattr(ext, "isosurface_refine") and hasattr(ext, "isosurface_refine_with") and ext.ISOSURFACE_REFINE_MAX_ROUNDS == 8
    text = (CSRC / "tn_isosurface_refine.hip").read_text()
    assert (int(re.search(r"constexpr int BT = (\d+);", text).group(1)), int(re.search(r"ISO_BLOCKS = (\d+);", text).group(1))) == ic.kernel_constants()


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = 64                                                                    # an aligned pointer that is never followed

    def begin(V=5, N=3, ev=x, values=x, level=0.0, br=x, fl=x):
        return lib.tn_isosurface_refine_begin(V, N, ev, values, level, br, fl, None)

    def points(V=5, N=3, rnd=0, ev=x, br=x, fl=x, vi=x, bc=x):
        return lib.tn_isosurface_refine_points(V, N, rnd, ev, br, fl, vi, bc, None)

    def select(N=3, rnd=0, level=0.0, dens=x, br=x, fl=x):
        return lib.tn_isosurface_refine_select(N, rnd, level, dens, br, fl, None)

    def vertices(V=5, N=3, xyz=x, ev=x, br=x, level=0.0, et=x, pos=x):
        return lib.tn_isosurface_refine_vertices(V, N, xyz, ev, br, level, et, pos, None)

    err = lib.tn_last_error
    for level in (float("nan"), float("inf"), -float("inf"), 2.0 ** 126, -2.0 ** 126, 1e300):
        for call in (begin, select, vertices):
            assert call(level=level) != 0 and b"level" in err(), (call.__name__, level)
    for call in (points, select):
        assert call(rnd=8) != 0 and b"round" in err() and call(rnd=2 ** 32 - 1) != 0 and b"round" in err()
    for call, names in ((begin, ("ev", "values", "br", "fl")), (points, ("ev", "br", "fl", "vi", "bc")), (select, ("dens", "br", "fl")),
                        (vertices, ("xyz", "ev", "br", "et", "pos"))):
        for name in names:
            assert call(**{name: None}) != 0 and b"null" in err(), (call.__name__, name)
        if call is not select:
            assert call(V=2 ** 32 - 1) != 0 and b"vertices" in err()
        assert call(N=2 ** 32) != 0 and b"surface vertices" in err()
        assert call(N=0, **{name: None for name in names}) == 0               # nothing to do, nothing to look at
    for call, name, bad in ((begin, "ev", 68), (begin, "br", 72), (points, "vi", 72), (points, "br", 68), (select, "br", 72), (vertices, "ev", 68),
                            (vertices, "et", 66), (select, "dens", 66)):
        assert call(**{name: bad}) != 0 and b"aligned" in err(), (call.__name__, name)
    assert points(V=0) != 0 and b"vertex 0" in err()


def test_statement_and_wrappers_refuse():
    g = _g()
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    xyz, ev, values, level, dens = rc.crafted(4)
    for bad in (np.nan, np.inf, 2.0 ** 126, 1e39):
        with pytest.raises(ValueError, match="level"):
            g.isosurface_refine_statement(xyz, ev, values, bad, rc.replay(dens), 1)
    for rounds in (9, -1):
        with pytest.raises(ValueError, match="rounds"):
            g.isosurface_refine_statement(xyz, ev, values, level, rc.replay(dens), rounds)
    with pytest.raises(ValueError, match="one row per vertex"):
        g.isosurface_refine_statement(xyz[:-1], ev, values, level, rc.replay(dens), 1)
    t = torch.from_numpy
    surface = {"edge_vertices": t(ev)}
    with pytest.raises(RuntimeError, match="rounds"):
        ext.isosurface_refine_with(surface, t(xyz), t(values), level, None, 9)
    with pytest.raises(RuntimeError, match="rounds"):
        ext.isosurface_refine(surface, t(xyz), t(values), level, torch.zeros(64, 8), [], -1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.isosurface_refine_with(surface, t(xyz), t(values), level, None, 1)


def test_adapter_and_extract_mesh_hand_the_rounds_down(tmp_path, monkeypatch):
    """nerfstudio_plugin.extract_mesh passes refine_rounds on only when it is asked for (the default call is what it was)"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    render = importlib.import_module("tetra-nerf_amd.render")
    calls = []
    mesh = {"positions": torch.zeros(3, 3), "triangles": torch.tensor([[0, 1, 2]], dtype=torch.int32), "colors": torch.zeros(3, 3)}
    monkeypatch.setattr(render, "extract_mesh", lambda *a, **kw: calls.append(kw) or mesh)
    model = types.SimpleNamespace(tetrahedra_vertices=torch.nn.Parameter(torch.zeros(4, 3)), tetrahedra_cells=torch.zeros(1, 4, dtype=torch.int32),
                                  tetrahedra_field=torch.nn.Parameter(torch.zeros(64, 4)), config=types.SimpleNamespace())
    plugin.extract_mesh(model, 1.0)
    plugin.extract_mesh(model, 1.0, refine_rounds=0)
    plugin.extract_mesh(model, 1.0, refine_rounds=3)
    assert ["refine_rounds" in kw for kw in calls] == [False, False, True] and calls[2]["refine_rounds"] == 3
