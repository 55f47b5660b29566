"""The tetrahedron split without a GPU (tn_split_count / tn_split_emit / tn_split_vertex_rows, csrc/tn_split.hip; the rule:
DESIGN.md section 4.18).  Layers: tests/host/split_emul.cpp -- which drives the element functions of csrc/tn_split_core.h, the
bodies of the kernels -- bit for bit against the numpy statements on every case of tests/split_cases.py; the statement's own
structure (conforming, orientations kept, volumes add up, parents consistent); the preservation of the piecewise-linear field
against a bound that is derived, not measured; a plain-loop restatement that rejects four mutations of the rule on named cases;
optim.grow_parameter on both optimiser classes; and the declarations and refusals of the entries.  (The kernels themselves:
tests/test_split_gpu.py.)"""
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

import split_cases as sc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"
ROWS = 3                                                                      # the per-vertex array the emulation carries


def _t(a):
    return torch.from_numpy(np.array(a))                                      # (the cases are read-only: a copy)


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "split_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "split_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def split_emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, xyz, cells, select, values, mode):
    V, T, rows = len(xyz), len(cells), len(values)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQQ", V, T, rows, mode))
        for a, dtype in ((xyz, np.float32), (cells, np.int32), (select, np.uint8), (values, np.float32)):
            f.write(np.ascontiguousarray(a, dtype).tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    offsets = np.frombuffer(raw, np.uint32, T + 1)
    K, at, out = int(offsets[T]), 4 * (T + 1), {"offsets": offsets}
    for key, dtype, shape in (("counters", np.uint32, (4,)), ("vertices", np.float32, (V + K, 3)), ("cells", np.int32, (T + 3 * K, 4)),
                              ("cell_parent", np.int32, (T + 3 * K,)), ("vertex_parents", np.int32, (K, 4)),
                              ("rows", np.float32, (rows, V + K)), ("rows_vm", np.float32, (V + K, rows))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += 4 * count
    assert at == len(raw)
    out["num_new"] = K
    return out


def _assert_equal(got, want, what):
    assert got["num_new"] == want["num_new"], what
    for key in sc.ARRAYS:
        assert got[key].shape == want[key].shape, f"{what}: {key} {got[key].shape} vs {want[key].shape}"
        assert np.array_equal(sc.bits(got[key]), sc.bits(want[key])), f"{what}: {key}"


def _check_emulation(exe, tmp_path, scenes, name, mode="mean"):
    g = sc.geometry()
    xyz, cells, select = sc.case(scenes, name)
    want = sc.statement(scenes, name)
    values = sc.values_for(len(xyz), ROWS, seed=len(cells))
    got = _run_emul(exe, tmp_path, xyz, cells, select, values, {"mean": 0, "zero": 1}[mode])
    _assert_equal(got, want, name)
    rows = g.split_vertex_rows_statement(values, want["vertex_parents"], new=mode)
    assert np.array_equal(sc.bits(got["rows"]), sc.bits(rows)) and np.array_equal(sc.bits(got["rows_vm"]), sc.bits(np.ascontiguousarray(rows.T))), name
    return got


@pytest.mark.parametrize("name", sc.names())
def test_emulated_kernels_equal_the_statement(split_emul, tmp_path, scenes, name):
    got = _check_emulation(split_emul, tmp_path, scenes, name)
    counters = got["counters"].tolist()
    xyz, cells, select = sc.case(scenes, name)
    assert counters[0] == int(np.count_nonzero(select)) == sum(counters[1:]) and counters[1] == got["num_new"]
    if name in sc.REFUSED_FLAT:
        assert counters[2] == sc.REFUSED_FLAT[name] and counters[3] == 0, (name, counters)
    if name == "id_past_V":
        assert counters == [5, 3, 0, 2] and got["offsets"].tolist() == [0, 1, 1, 2, 2, 3]
    if name == "nan_coordinate":
        assert counters == [3, 2, 1, 0] and got["offsets"].tolist() == [0, 1, 1, 2]
    if name in ("none_asked", "no_tets"):
        assert counters == [0, 0, 0, 0] and got["num_new"] == 0 and np.array_equal(got["cells"], cells)
        assert np.array_equal(sc.bits(got["vertices"]), sc.bits(xyz))
    if name == "near_duplicates_400_all":                                     # refused for the ROUNDED centroid: none of them is flat
        g = sc.geometry()
        refused = np.nonzero(np.diff(got["offsets"].astype(np.int64)) == 0)[0]
        assert len(refused) == 86 and np.all(g.tet_orient(_t(xyz), _t(cells[refused])).numpy() != 0)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path, scenes):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: ids past the table,
    a NaN, refusals, empty inputs, and both modes of the new columns"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ("id_past_V", "nan_coordinate", "grid_4_all", "cube_all", "none_asked", "no_tets"):
        _check_emulation(exe, tmp_path, scenes, name)
    got = _check_emulation(exe, tmp_path, scenes, "cube_all", mode="zero")
    assert not got["rows"][:, 9:].any() and got["rows"].shape == (ROWS, 21)


# --------------------------------------------------------------------------------------------------------------- structure
STRUCTURED = ("cube_all", "random_300_30pct", "grid_4_all", "grid_6_all", "near_duplicates_400_all")


@pytest.mark.parametrize("name", STRUCTURED)
def test_split_mesh_is_conforming_and_keeps_orientations(scenes, oracle, name):
    xyz, cells, select = sc.case(scenes, name)
    check_structure(oracle, xyz, cells, sc.statement(scenes, name), name)


def check_structure(oracle, xyz, cells, s, name):
    """the checks of the test above on one split: (xyz, cells) is the input, s the statement's answer (also used on the generation
    meshes of tests/lifecycle_lib.py, whose input is itself the output of a split)"""
    V, T, K = len(xyz), len(cells), s["num_new"]
    assert K > 0 and s["cells"].shape == (T + 3 * K, 4) and s["vertices"].shape == (V + K, 3)
    faces, face_tets = oracle.build_faces(s["cells"])                         # raises on a face in three tetrahedra
    faces0, _ = oracle.build_faces(cells)
    assert len(faces) == len(faces0) + 6 * K                                  # every split adds its six inner faces, and no other
    # parents: consistent with the cells
    parent, vp = s["cell_parent"].astype(np.int64), s["vertex_parents"]
    accepted = np.nonzero(np.diff(s["offsets"].astype(np.int64)))[0]
    assert np.array_equal(parent[:T], np.arange(T)) and np.array_equal(parent[T:], np.repeat(accepted, 3))
    assert np.array_equal(vp, cells[accepted])
    untouched = np.setdiff1d(np.arange(T), accepted)
    assert np.array_equal(s["cells"][untouched], cells[untouched])
    for i in range(4):
        rows = accepted if i == 0 else T + 3 * np.arange(K) + i - 1
        child = s["cells"][rows]
        assert np.array_equal(child[:, i], V + np.arange(K)) and np.array_equal(np.delete(child, i, 1), np.delete(cells[accepted], i, 1))
    # every tetrahedron of the split mesh has the orientation of its parent as stored
    g = sc.geometry()
    before = g.tet_orient(_t(xyz), _t(cells)).numpy()
    after = g.tet_orient(_t(s["vertices"]), _t(s["cells"])).numpy()
    assert np.array_equal(after, before[parent]) and np.all(before[accepted] != 0)
    # The children's signed volumes add up to the parent's.  Exactly: child i is the parent with p_i replaced by c, its volume is
    # lambda_i(c) times the parent's, and the four barycentrics of ANY point c sum to 1.  What is left is the float64 evaluation
    # of the five determinants on the fp32 coordinates.  With M = max |coordinate| and L <= 2 M the longest edge, an edge vector
    # is exact up to 2^-53 M, and the two products and two sums of a determinant add at most 7 2^-53 L^3: together below
    # 10 2^-53 M L^2 per determinant, 50 2^-53 M L^2 for the five.  The width is w = |V| / D with D = the largest of the seven
    # cross products of tet_width_orient (faces and opposite edges), so the bound asked for, 8 2^-24 |V| M / w = 8 2^-24 M D,
    # covers that wherever D >= 50 2^-32 L^2 -- every tetrahedron that is not a needle of aspect 10^-8, which is asserted.
    p64, c64 = xyz.astype(np.float64)[cells[accepted]], s["vertices"].astype(np.float64)
    total = np.zeros(K)
    for i in range(4):
        rows = accepted if i == 0 else T + 3 * np.arange(K) + i - 1
        total += sc.vol6(c64[s["cells"][rows]])
    vol = sc.vol6(p64)
    width = g.tet_width64(torch.from_numpy(p64)).numpy()
    M = np.abs(p64).max((1, 2))
    L = np.linalg.norm(p64[:, :, None] - p64[:, None], axis=-1).max((1, 2))
    D = np.abs(vol) / width
    assert np.all(D >= 50 * 2.0 ** -32 * L * L)
    bound = 8 * sc.U * np.abs(vol) * (M / width)
    print(name, "K", K, "largest |sum - parent| / bound", float((np.abs(total - vol) / bound).max()))
    assert np.all(np.abs(total - vol) <= bound)


# ------------------------------------------------------------------------------------------------------------ preservation
@pytest.mark.parametrize("name", STRUCTURED)
def test_split_field_is_the_parent_field(scenes, name):
    """The piecewise-linear field of the split mesh is the parent's, up to the rounding of the centroid and of the mean.

    Let P be the parent's affine interpolant of one field row F, c the exact centroid, c~ the fp32 one, F~_c the fp32 mean.  A point
    of child i is x = sum_{j != i} l_j p_j + l_c c~ with barycentrics summing to 1.  The child's interpolant there is
    sum l_j F_j + l_c F~_c; P is affine, so P(x) = sum l_j F_j + l_c P(c~).  The difference is EXACTLY l_c (F~_c - P(c~)).
    F~_c = ((F_a + F_b) + (F_c + F_d)) * 0.25f: the two levels of sums round once each, the product by a power of two does not, so
    |F~_c - mean F| <= ((1 + u)^2 - 1) max|F| < 3 u max|F|, and P(c) = mean F exactly.  The same holds per coordinate of c~:
    |c~ - c|_inf < 3 u max|coordinate|, hence |P(c~) - P(c)| <= |grad P|_1 3 u max|coordinate|.  Together
        |difference| <= l_c (3 u max|F_parent| + |grad P|_1 3 u max|coordinate|),      u = 2^-24,
    with grad P from the parent in float64.  Both sides are evaluated in float64 from the statement's fp32 outputs; every child and
    every sample is checked.  (In the near-duplicates mesh the float64 solve for grad P is itself ill-conditioned; the bound
    scales with the same gradient, and the figures are printed.)"""
    g = sc.geometry()
    xyz, cells, _ = sc.case(scenes, name)
    s = sc.statement(scenes, name)
    V, T, K = len(xyz), len(cells), s["num_new"]
    field = sc.values_for(V, 4, seed=7)
    new_field = g.split_vertex_rows_statement(field, s["vertex_parents"])
    rng = np.random.default_rng(11)
    accepted = np.nonzero(np.diff(s["offsets"].astype(np.int64)))[0]
    rows = np.concatenate([accepted, T + np.arange(3 * K)])                   # every child
    slot = np.concatenate([np.zeros(K, np.int64), np.tile([1, 2, 3], K)])     # where the new vertex sits in it
    parent = s["cell_parent"].astype(np.int64)[rows]
    F0, grad, p0 = sc.parent_interpolant(xyz, cells[accepted], field)         # per accepted PARENT (a refused one may be flat)
    of = np.searchsorted(accepted, parent)                                    # child -> its row in those three
    lam = rng.dirichlet(np.ones(4), (len(rows), 8))                           # [n, 8 samples, 4] inside each child
    cv = s["vertices"].astype(np.float64)[s["cells"][rows]]                   # [n, 4, 3]
    cf = new_field.astype(np.float64).T[s["cells"][rows]]                     # [n, 4, rows]
    x = np.einsum("nsk,nka->nsa", lam, cv)
    child_value = np.einsum("nsk,nkr->nsr", lam, cf)
    parent_value = F0[of][:, None] + np.einsum("nra,nsa->nsr", grad[of], x - p0[of][:, None])
    lam_c = lam[np.arange(len(rows)), :, slot]                                # [n, 8]
    maxF = np.abs(field.astype(np.float64).T[cells[parent]]).max(1)           # [n, rows]
    M = np.abs(xyz.astype(np.float64)[cells[parent]]).max((1, 2))             # [n]
    bound = lam_c[:, :, None] * (3 * sc.U * maxF + np.abs(grad[of]).sum(2) * 3 * sc.U * M[:, None])[:, None]
    diff = np.abs(child_value - parent_value)
    print(name, "children", len(rows), "samples", diff.size, "largest difference", float(diff.max()), "largest difference / bound",
          float((diff / bound).max()))
    assert len(rows) == 4 * K and np.all(diff <= bound)


# -------------------------------------------------------------------------------------------- a restatement and its mutations
def _restate(case, accepted_rank=True, pairwise=True, parent_sign=True, overwrite=True):
    """the rule as a plain loop over tetrahedra; the keywords are the four mutations"""
    xyz, cells, select = case
    V, T = len(xyz), len(cells)
    f32 = np.float32
    rows, vertices, appended, asked_rank = [list(map(int, r)) for r in cells.view(np.uint32)], [list(v) for v in xyz], [], 0
    for t in range(T):
        if not select[t]:
            continue
        rank, asked_rank = asked_rank, asked_rank + 1
        c = rows[t]
        if any(i >= V for i in c):
            continue
        p = xyz[c]
        if pairwise:
            cen = ((p[0] + p[1]) + (p[2] + p[3])) * f32(0.25)
        else:
            cen = (((p[0] + p[1]) + p[2]) + p[3]) * f32(0.25)
        def orient(q):                                                        # 0 also for NaN
            v = float(sc.vol6(q.astype(np.float64)[None])[0])
            return 1 if v > 0 else (-1 if v < 0 else 0)

        s = orient(p)
        want = s if parent_sign else 1
        if s == 0 or any(orient(np.concatenate([p[:i], cen[None], p[i + 1:]])) != want for i in range(4)):
            continue
        k = len(vertices) - V if accepted_rank else rank
        new = V + k
        vertices.append(list(cen))
        children = [c[:i] + [new] + c[i + 1:] for i in range(4)]
        if overwrite:
            rows[t] = children[0]
            appended += children[1:]
        else:
            appended += children[1:] + children[:1]
    return np.array(vertices, np.float32).reshape(-1, 3), np.array(rows + appended, np.uint32).view(np.int32).reshape(-1, 4)


def _same(a, want):
    return a[0].shape == want["vertices"].shape and np.array_equal(sc.bits(a[0]), sc.bits(want["vertices"])) and \
        a[1].shape == want["cells"].shape and np.array_equal(a[1], want["cells"])


def test_restatement_equals_the_statement(scenes):
    for name in sc.names():
        assert _same(_restate(sc.case(scenes, name)), sc.statement(scenes, name)), name


def test_mutations_of_the_rule_are_rejected_by_named_cases(scenes):
    mutations = {
        "children numbered by the asked rank": ("grid_4_all", dict(accepted_rank=False)),
        "the centroid summed left to right": ("random_300_30pct", dict(pairwise=False)),
        'the parent\'s sign replaced by "positive"': ("cube_all", dict(parent_sign=False)),
        "child 0 appended instead of overwriting": ("cube_all", dict(overwrite=False)),
    }
    for what, (name, kw) in mutations.items():
        case, want = sc.case(scenes, name), sc.statement(scenes, name)
        assert _same(_restate(case), want), name
        assert not _same(_restate(case, **kw), want), f"{what}: not rejected by {name}"
    g = sc.geometry()                                                         # why the cube rejects "positive": half of it is negative
    xyz, cells, _ = sc.case(scenes, "cube_all")
    assert (g.tet_orient(_t(xyz), _t(cells)).numpy() < 0).any()


def test_vertex_rows_statement(scenes):
    g = sc.geometry()
    s = sc.statement(scenes, "random_300_30pct")
    V = 300
    ints = sc.values_for(V, 3, integers=True)
    got = g.split_vertex_rows_statement(ints, s["vertex_parents"])
    exact = ints.astype(np.float64)[:, s["vertex_parents"]].sum(2) / 4         # sums of four small integers and their quarters are exact
    assert np.array_equal(got[:, :V], ints) and np.array_equal(got[:, V:].astype(np.float64), exact)
    assert not g.split_vertex_rows_statement(ints, s["vertex_parents"], new="zero")[:, V:].any()
    bad = np.array([[0, 1, 2, V], [0, 1, 2, 3]], np.int32)                     # a parent id >= V: 0
    assert g.split_vertex_rows_statement(ints, bad)[:, V].tolist() == [0, 0, 0] and g.split_vertex_rows_statement(ints, bad)[:, V + 1].any()
    with pytest.raises(ValueError, match="mean"):
        g.split_vertex_rows_statement(ints, bad, new="median")
    with pytest.raises(ValueError, match="one entry per row"):
        g.split_tetrahedra_statement(np.zeros((4, 3), np.float32), np.zeros((2, 4), np.int32), np.zeros(3, np.uint8))


def test_the_cases_are_what_they_are_named_for(scenes):
    bt, blocks = sc.kernel_constants()
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.SPLIT_GRID_LANES == bt * blocks and ext.TetrahedraTracer.supports_split is True
    assert set(sc.soup_sizes()) >= {1, 63, 64, 65, 255, 256, 257, bt * blocks - 1, bt * blocks, bt * blocks + 1}
    xyz, cells, select = sc.case(scenes, "random_300_30pct")
    assert 0.25 * len(cells) < select.sum() < 0.35 * len(cells)
    for T in (65, 257):
        xyz, cells = sc.soup(scenes, T)
        assert len(cells) == T and cells.max() < len(xyz)
        s = sc.statement(scenes, f"soup_{T}_third")
        assert s["num_new"] == (T + 2) // 3 and sc.statement(scenes, f"soup_{T}_none")["num_new"] == 0
        assert sc.statement(scenes, f"soup_{T}_one")["num_new"] == 1 and sc.statement(scenes, f"soup_{T}_all")["num_new"] == T


# ----------------------------------------------------------------------------------------------------------- grow_parameter
def _stepped(cls, params, steps=3):
    opt = cls(params, lr=1e-2)
    for _ in range(steps):
        for p in params:
            p.grad = torch.ones_like(p)
        opt.step()
    return opt


def test_grow_parameter_moves_the_state(monkeypatch):
    optim = importlib.import_module("tetra-nerf_amd.optim")
    torch.manual_seed(0)
    field, other = torch.nn.Parameter(torch.randn(4, 5)), torch.nn.Parameter(torch.randn(7))
    opt = _stepped(torch.optim.RAdam, [field, other])
    m, v = opt.state[field]["exp_avg"], opt.state[field]["exp_avg_sq"]
    new = torch.nn.Parameter(torch.cat([field.detach(), torch.zeros(4, 2)], 1))
    grown_m = torch.cat([m, torch.full((4, 2), 0.5)], 1)
    assert optim.grow_parameter(opt, field, new, exp_avg=grown_m) is new
    assert [p is new for p in opt.param_groups[0]["params"]] == [True, False] and field not in opt.state
    assert all(p is not field for g in opt.param_groups for p in g["params"])
    st = opt.state[new]
    assert float(st["step"]) == 3 and st["exp_avg"].data_ptr() == grown_m.data_ptr() and torch.equal(st["exp_avg"], grown_m)
    assert st["exp_avg_sq"].shape == (4, 7) and not st["exp_avg_sq"].any()
    assert float(opt.state[other]["step"]) == 3
    new.grad, other.grad = torch.ones_like(new), torch.ones_like(other)
    opt.step()                                                                # the optimiser goes on
    assert float(opt.state[new]["step"]) == 4
    with pytest.raises(ValueError, match="not a parameter"):
        optim.grow_parameter(opt, field, torch.nn.Parameter(torch.zeros(4, 9)))
    with pytest.raises(ValueError, match="shape"):
        optim.grow_parameter(opt, new, torch.nn.Parameter(torch.zeros(4, 9)), exp_avg=torch.zeros(4, 8))
    # a parameter that was never stepped has no state and gets none
    fresh = torch.optim.RAdam([field])
    optim.grow_parameter(fresh, field, new)
    assert fresh.param_groups[0]["params"] == [new] and len(fresh.state) == 0

    # FusedRAdam's host side: construction, state, state_dict (its step needs the device; here the parameter check is lifted)
    monkeypatch.setattr(optim, "_check_param", lambda p: None)
    a, b = torch.nn.Parameter(torch.randn(4, 5)), torch.nn.Parameter(torch.randn(7))
    theirs = _stepped(torch.optim.RAdam, [a, b])
    ours = optim.FusedRAdam([a, b], lr=1e-2)
    ours.load_state_dict(theirs.state_dict())
    grown = torch.nn.Parameter(torch.zeros(4, 8))
    optim.grow_parameter(ours, a, grown, exp_avg=torch.ones(4, 8), exp_avg_sq=torch.ones(4, 8))
    assert float(ours.state[grown]["step"]) == 3 and a not in ours.state and ours.param_groups[0]["params"][0] is grown
    # the state dicts still interchange, in both directions
    back = torch.optim.RAdam([grown, b], lr=1e-2)
    back.load_state_dict(ours.state_dict())
    assert float(back.state[grown]["step"]) == 3 and torch.equal(back.state[grown]["exp_avg"], torch.ones(4, 8))
    again = optim.FusedRAdam([grown, b], lr=1e-2)
    again.load_state_dict(back.state_dict())
    assert float(again.state[b]["step"]) == 3 and again.state[grown]["exp_avg_sq"].shape == (4, 8)


# ---------------------------------------------------------------------------------------------------------------- entries
def test_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_split_count\(size_t num_vertices, size_t num_cells, const float \*xyz, const uint32_t \*cells,\s*"
                     r"const uint8_t \*select,\s*uint32_t \*offsets, uint32_t \*counters, void \*stream\);", header)
    assert re.search(r"int\s+tn_split_emit\(size_t num_vertices, size_t num_cells, const float \*xyz, const uint32_t \*cells,\s*"
                     r"const uint32_t \*offsets,\s*size_t num_new, float \*xyz_out, uint32_t \*cells_out, uint32_t \*cell_parent,\s*"
                     r"uint32_t \*vertex_parents,\s*void \*stream\);", header)
    assert re.search(r"int\s+tn_split_vertex_rows\(size_t rows, size_t num_vertices, size_t num_new, const float \*values,\s*"
                     r"const float \*values_vm,\s*const uint32_t \*vertex_parents, uint32_t new_mode, float \*out, float \*out_vm,\s*"
                     r"void \*stream\);", header)
    assert "no reference counterpart" in header[header.index("Tetrahedron split"):header.index("int tn_split_count")]
    lib = _lib.load()
    for name in ("tn_split_count", "tn_split_emit", "tn_split_vertex_rows"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert len(lib.tn_split_count.argtypes) == 8 and len(lib.tn_split_emit.argtypes) == 11 and len(lib.tn_split_vertex_rows.argtypes) == 10
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    for name in ("split_tetrahedra", "split_vertex_rows"):
        assert hasattr(ext, name)
    assert hasattr(ext.TetrahedraTracer, "split_tetrahedra")
    assert hasattr(importlib.import_module("tetra-nerf_amd.nerfstudio_plugin"), "densify")
    assert hasattr(importlib.import_module("tetra-nerf_amd.optim"), "grow_parameter")
    core = (CSRC / "tn_split_core.h").read_text()
    assert "MAX_CELLS = 1ull << 30" in core and sc.geometry().SPLIT_MAX_CELLS == 1 << 30
    assert "guard::tet_orient" in core and "vol6" not in core                # the orientation is reused, not restated


def test_the_entries_refuse_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = 64                                                                    # a pointer that is never followed

    def count(V=5, T=2, xyz=x, cells=x, select=x, offsets=x, counters=x):
        return lib.tn_split_count(V, T, xyz, cells, select, offsets, counters, None)

    for kw in (dict(xyz=None), dict(cells=None), dict(select=None), dict(offsets=None), dict(counters=None),
               dict(T=0, xyz=None, cells=None, select=None, offsets=None)):
        assert count(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert count(T=2 ** 30) != 0 and b"2^30" in lib.tn_last_error()
    assert count(V=2 ** 32 - 1) != 0 and b"vertices" in lib.tn_last_error()

    def emit(V=5, T=2, xyz=x, cells=x, offsets=x, K=1, a=x, b=x, c=x, d=x):
        return lib.tn_split_emit(V, T, xyz, cells, offsets, K, a, b, c, d, None)

    for kw in (dict(xyz=None), dict(cells=None), dict(offsets=None), dict(a=None), dict(b=None), dict(c=None), dict(d=None)):
        assert emit(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert emit(K=3) != 0 and b"exceeds num_cells" in lib.tn_last_error()
    assert emit(V=2 ** 32 - 3, K=2) != 0 and b"vertices" in lib.tn_last_error()
    third = (2 ** 30) // 4
    assert emit(T=third + 4, K=third) != 0 and b"2^30" in lib.tn_last_error()

    def rows(n=64, V=5, K=1, values=x, vm=None, parents=x, mode=0, out=x, out_vm=None):
        return lib.tn_split_vertex_rows(n, V, K, values, vm, parents, mode, out, out_vm, None)

    assert rows(n=0) != 0 and b"rows" in lib.tn_last_error()
    assert rows(mode=2) != 0 and b"new_mode" in lib.tn_last_error()
    for kw in (dict(values=None), dict(parents=None), dict(out=None)):
        assert rows(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert rows(V=2 ** 32 - 2, K=1) != 0 and b"vertices" in lib.tn_last_error()


def test_wrappers_refuse_host_tensors(scenes):
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    xyz, cells, select = (_t(a) for a in sc.case(scenes, "cube_all"))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.split_tetrahedra(xyz, cells, select)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.split_vertex_rows(torch.zeros(3, 9), cells[:1])
    with pytest.raises(RuntimeError, match="mean"):
        ext.split_vertex_rows(torch.zeros(3, 9), cells[:1], new="median")
