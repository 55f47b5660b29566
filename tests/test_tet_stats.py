"""The per-tetrahedron training statistics without a GPU (tn_tet_stats_accumulate, csrc/tn_tet_stats.hip; the rule:
csrc/tn_tet_stats_core.h; the statement: render.tet_stats_statement).

Bar: every comparison is of integers, byte for byte -- no tolerance.  The host emulation (tests/host/tet_stats_emul.cpp: the
core header's three rules and a lane-by-lane model of the kernel's 64-lane run fold with its carry) equals the statement on every
named case of tests/tet_stats_cases.py, also under the host sanitizers; a sample-by-sample restatement in Python scalars equals
it too, and each named mutation of the rule is rejected by the case built for it.

The FMA-style mutation (ONE rounding of w^ * v^ * 2^32 instead of a rounded fp32 product scaled afterwards) needs no case: it
is the same function.  Scaling by 2^32 commutes with the rounding to fp32 wherever the product is a normal number and nothing
overflows (at most 2^40 here); where fl32(w^ v^) is subnormal both forms are below 2^-126 * 2^32 = 2^-94 and rint gives 0.
test_single_rounding_of_the_scaled_product_is_the_same_function shows it on the values where it could differ."""
import ctypes
import importlib
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tet_stats_cases as tc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"


# ------------------------------------------------------------------------------------------------------------ host emulation
def _build_emul(tmp_path_factory, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("host") / "tet_stats_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "tet_stats_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and extra and "sanitize" in r.stderr + " ".join(extra) and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime to link")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return _build_emul(tmp_path_factory)


def _run_emul(exe, tmp_path, c):
    rows, S = c["cells"].shape
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    rays = 0 if c["ray_value"] is None else len(c["ray_value"])
    with open(src, "wb") as f:
        f.write(struct.pack("<QQQQQQ", c["T"], rows, S, rows if c["count"] is None else c["count"], c["ray_index"] is not None, rays))
        f.write(c["cells"].tobytes())
        f.write(c["weights"].tobytes())
        if c["ray_index"] is not None:
            f.write(c["ray_index"].tobytes())
        if rays:
            f.write(c["ray_value"].tobytes())
        f.write(c["stats0"].tobytes())
    # (the sanitizer build: its leak check at exit needs ptrace, which a sandbox may refuse)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    return np.frombuffer(dst.read_bytes(), np.int64).reshape(c["T"], 3), int(r.stdout.split()[1])


@pytest.mark.parametrize("name", tc.names())
def test_emulated_kernel_equals_the_statement(emul, tmp_path, name):
    c = tc.case(name)
    got, adds = _run_emul(emul, tmp_path, c)
    want = tc.statement(c)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:3])
    assert (name == "count_zero") == np.array_equal(want, c["stats0"])       # every other case adds something
    # only run heads reach memory: three adds per run of equal accepted cells at most (the carry joins runs across chunks)
    rows = c["cells"].shape[0] if c["count"] is None else c["count"]
    cells = c["cells"][:rows]
    ok = (cells >= 0) & (cells < c["T"])
    runs = int((ok & np.concatenate([np.ones((rows, 1), bool), cells[:, 1:] != cells[:, :-1]], 1)).sum())
    assert adds == 3 * runs, (name, adds, runs)


def test_emulation_under_the_host_sanitizers(tmp_path_factory, tmp_path):
    """the stand-alone program built with -fsanitize=address,undefined reads and writes nothing out of bounds: ids at and past T,
    rows past count, a last chunk of one lane, NaN and inf through the float-to-integer conversions"""
    exe = _build_emul(tmp_path_factory, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for name in ("invalid_ids", "count_rows", "value_edges", "all_distinct", "single_sample", "aba"):
        c = tc.case(name)
        assert np.array_equal(_run_emul(exe, tmp_path, c)[0], tc.statement(c)), name


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", tc.names())
def test_restatement_equals_the_statement(name):
    c = tc.case(name)
    assert np.array_equal(tc.restatement(c), tc.statement(c)), name


@pytest.mark.parametrize("mutation, name", [("truncate", "half_ties"), ("accept_ids_above_T", "invalid_ids"),
                                            ("read_padded_rows", "count_rows"), ("no_value_clamp", "value_edges")])
def test_mutations_of_the_rule_are_rejected_by_named_cases(mutation, name):
    c = tc.case(name)
    want = tc.statement(c)
    assert not np.array_equal(tc.restatement(c, mutation), want), (mutation, name)
    assert {m for m, _ in [(mutation, name)]} <= set(tc.MUTATIONS)


def test_single_rounding_of_the_scaled_product_is_the_same_function():
    """rint(fl32(w^ v^) 2^32) == rint(fl32(w^ v^ 2^32)): the product of two fp32 values is exact in a double, so the right side
    is computed exactly here; tried where the two could part -- products that are subnormal or round at the fp32 boundary"""
    rng = np.random.default_rng(0)
    w = np.concatenate([rng.random(4000, dtype=np.float32), np.float32(2.0) ** -rng.integers(0, 149, 4000) * rng.random(4000, dtype=np.float32),
                        np.float32([0, 1, 2.0 ** -126, 2.0 ** -149, 1 - 2.0 ** -24])])
    v = np.concatenate([256 * rng.random(4000, dtype=np.float32), np.float32(2.0) ** -rng.integers(0, 149, 4000) * rng.random(4000, dtype=np.float32),
                        np.float32([256, 2.0 ** -149, 2.0 ** -100, 1e-30, 256])])
    two_step = np.rint((w * v).astype(np.float32).astype(np.float64) * 2.0 ** 32)
    one_step = np.rint((w.astype(np.float64) * v.astype(np.float64) * 2.0 ** 32).astype(np.float32).astype(np.float64))
    assert np.array_equal(two_step, one_step)
    assert ((w * v) < np.float32(2.0 ** -126)).sum() > 500                   # the subnormal range was visited


def test_the_statement_on_a_hand_computed_table():
    r = tc.render()
    stats = np.zeros((3, 3), np.int64)
    cells = np.int32([[0, 1, -1, 3, 2]])
    got = r.tet_stats_statement(stats, cells, np.float32([[0.5, 1.5, 1, 1, np.nan]]), np.float32([2.0]))
    assert got.tolist() == [[1, 2 ** 31, 2 ** 32], [1, 2 ** 32, 2 ** 33], [1, 0, 0]] and not stats.any()
    # uint32 cells with 0xFFFFFFFF and torch tensors are the same samples; a second batch adds
    again = r.tet_stats_statement(torch.from_numpy(got), torch.from_numpy(cells), torch.tensor([[0.5, 1.5, 1, 1, float("nan")]]), torch.tensor([2.0]))
    assert np.array_equal(again, 2 * got)
    assert np.array_equal(r.tet_stats_statement(stats, cells.view(np.uint32), np.float32([[0.5, 1.5, 1, 1, np.nan]]), np.float32([2.0])), got)
    # the capacity the header states: the largest terms
    top = r.tet_stats_statement(stats, np.int32([[0]]), np.float32([[7.0]]), np.float32([1e9]))
    assert top[0].tolist() == [1, 2 ** 32, 2 ** 40]
    core = (CSRC / "tn_tet_stats_core.h").read_text()
    assert "MAX_SAMPLES_PER_CELL = (int64_t)1 << 23" in core and (2 ** 23 - 1) * 2 ** 40 < 2 ** 63 <= 2 ** 23 * 2 ** 40


# ------------------------------------------------------------------------------------------------------------------ scores
def test_scores_on_hand_computed_tables():
    r = tc.render()
    one = 2 ** 32
    stats = torch.tensor([[4, 2 * one, 3 * one], [7, 0, 0], [1, one // 2, one // 4], [0, 0, 0], [2, one, 0]], dtype=torch.int64)
    want = {"error": [3.0, 0.0, 0.25, 0.0, 0.0], "mean_error": [1.5, 0.0, 0.5, 0.0, 0.0], "weight": [2.0, 0.0, 0.5, 0.0, 1.0],
            "hits": [4.0, 7.0, 1.0, 0.0, 2.0]}
    for kind, values in want.items():
        got = r.tet_stats_scores(stats, kind)
        assert got.dtype == torch.float32 and got.tolist() == values, kind
    # float64 inside: sums beyond fp32's integers keep their low bits up to the last conversion
    big = torch.tensor([[1, (2 ** 30 + 1) * one, (2 ** 30 + 1) * one]], dtype=torch.int64)
    assert r.tet_stats_scores(big, "mean_error").tolist() == [1.0] and r.tet_stats_scores(big, "weight").tolist() == [float(np.float32(2 ** 30 + 1))]
    with pytest.raises(ValueError, match="kind"):
        r.tet_stats_scores(stats, "median")


# --------------------------------------------------------------------------------------------------------------- selection
def test_selection_ties_and_min_hits():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    one = 2 ** 32
    #                     hits weight error
    stats = torch.tensor([[5, one, 2 * one],      # 0: score 2
                          [5, one, 3 * one],      # 1: score 3
                          [1, one, 9 * one],      # 2: score 9, one hit
                          [5, one, 3 * one],      # 3: score 3 (ties with 1)
                          [0, 0, 0],              # 4: never sampled
                          [5, one, 3 * one],      # 5: score 3 (ties with 1 and 3)
                          [9, 4 * one, 4 * one]], dtype=torch.int64)    # 6: score 4, mean 1
    sel = lambda **kw: torch.nonzero(plugin.densify_selection(stats, **kw))[:, 0].tolist()   # noqa: E731
    assert sel() == [0, 1, 2, 3, 5, 6]                                        # min_hits None: at least one sample
    assert sel(min_hits=0) == [0, 1, 2, 3, 4, 5, 6]
    assert sel(min_hits=2) == [0, 1, 3, 5, 6]
    assert sel(min_hits=2, max_new=1) == [6]
    assert sel(min_hits=2, max_new=2) == [1, 6]                               # the tie at 3 goes to the lowest id
    assert sel(min_hits=2, max_new=3) == [1, 3, 6]
    assert sel(max_new=1) == [2] and sel(max_new=0) == []
    assert sel(min_hits=2, max_new=2, score="mean_error") == [1, 3]           # 6 has mean 1
    assert sel(min_hits=2, max_new=1, score="hits") == [6]
    assert sel(min_hits=2, max_new=2, score="weight") == [0, 6]               # four tie at weight 1: the lowest id
    mask = torch.tensor([1, 0, 1, 1, 1, 1, 0], dtype=torch.bool)
    assert sel(mask=mask, min_hits=2, max_new=2) == [3, 5]
    assert sel(mask=mask, min_hits=2, max_new=99) == [0, 3, 5]


class _StandInTracer:
    supports_split = True

    def __init__(self, T):
        self.device = torch.device("cpu")
        self.tetrahedra_cells = torch.zeros(T, 4, dtype=torch.int32)
        self.asked = []

    def tet_quality(self):
        return {"width": torch.arange(self.tetrahedra_cells.size(0), dtype=torch.float32)}

    def split_tetrahedra(self, mask, tet_values=()):
        self.asked.append(torch.nonzero(mask)[:, 0].tolist())
        return {"num_new": 0, "counters": torch.zeros(4, dtype=torch.int32)}


def test_densify_selects_by_the_statistics_on_a_stand_in(monkeypatch):
    """densify up to the split: a stand-in tracer records the mask and accepts nothing"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    monkeypatch.setattr(ext, "field_is_registered", lambda f: False)
    one = 2 ** 32
    stats = torch.tensor([[5, one, 2 * one], [5, one, 3 * one], [1, one, 9 * one], [5, one, 3 * one], [0, 0, 0], [5, one, 3 * one]], dtype=torch.int64)
    tracer = _StandInTracer(6)
    model = SimpleNamespace(get_tetrahedra_tracer=lambda: tracer, tetrahedra_field=torch.zeros(64, 4), tetrahedra_vertices=torch.zeros(4, 3),
                            tetrahedra_occupancy=torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0, 1.0]))
    res = plugin.densify(model, stats=stats, min_hits=2, max_new=2)
    assert tracer.asked[-1] == [1, 3] and res["num_new"] == 0 and res["stats_reset"] is False
    plugin.densify(model, stats=stats, min_hits=2, max_new=2, occupancy_threshold=0.5)        # the existing conditions still cut
    assert tracer.asked[-1] == [3, 5]
    plugin.densify(model, stats=stats, min_width=3.0)
    assert tracer.asked[-1] == [3, 5]
    plugin.densify(model, torch.tensor([1, 1, 1, 0, 1, 0]), stats=stats, max_new=2)            # the caller's mask, cut by score
    assert tracer.asked[-1] == [1, 2]
    model._tn_tet_stats = stats
    plugin.densify(model, stats=True, max_new=1, score="mean_error")
    assert tracer.asked[-1] == [2]
    # what was there before: no statistics, the widest
    del model._tn_tet_stats
    res = plugin.densify(model, min_width=0.0, max_new=2)
    assert tracer.asked[-1] == [4, 5] and "stats_reset" not in res
    for kw, match in ((dict(stats=True), "stats=True"), (dict(stats=stats[:3]), r"i64 \[T, 3\]"), (dict(min_hits=2, min_width=0.0), "min_hits"),
                      (dict(), "give")):
        with pytest.raises(ValueError, match=match):
            plugin.densify(model, **kw)


class _MeshChangingTracer(_StandInTracer):
    """a stand-in that loads what it returns, as the tracer does: split_tetrahedra accepts every asked tetrahedron (shapes only),
    retriangulate gives two more cells, delaunay_check reports 9 of 10 interior faces violated"""
    supports_delaunay_check = True

    def __init__(self, vertices, cells):
        super().__init__(len(cells))
        self.tetrahedra_vertices, self.tetrahedra_cells = vertices, cells

    def split_tetrahedra(self, mask, tet_values=()):
        xyz, cells = self.tetrahedra_vertices.detach(), self.tetrahedra_cells
        asked = torch.nonzero(mask)[:, 0]
        K, T = len(asked), len(cells)
        parent = torch.cat([torch.arange(T), asked.repeat_interleave(3)])
        out = {"num_new": K, "counters": torch.tensor([K, K, 0, 0], dtype=torch.int32), "vertices": torch.cat([xyz, xyz[:K] + 0.5]),
               "cells": cells[parent], "vertex_parents": cells[asked], "tet_values": [t[parent] for t in tet_values]}
        self.tetrahedra_vertices, self.tetrahedra_cells = out["vertices"], out["cells"]
        return out

    def retriangulate(self, xyz, tet_values=()):
        cells = torch.zeros(len(self.tetrahedra_cells) + 2, 4, dtype=torch.int32)
        self.tetrahedra_vertices, self.tetrahedra_cells = xyz, cells
        return {"cells": cells, "tet_values": [torch.full((len(cells),), 2.0) for _ in tet_values], "num_tetrahedra": len(cells)}

    def delaunay_check(self):
        return {"counters": torch.tensor([10, 9, 0, 0], dtype=torch.int32)}


def test_every_mesh_change_leaves_model_and_tracer_agreeing(monkeypatch):
    """the three places that change the mesh under a model -- densify's split, its re-triangulation, the monitor's -- leave the
    config sizes, the vertex key, the snapshot and the zeroed statistics in agreement with the tensors now on the model"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    monkeypatch.setattr(ext, "field_is_registered", lambda f: False)
    monkeypatch.setattr(ext, "unregister_field", lambda f: None)
    monkeypatch.setattr(ext, "split_vertex_rows", lambda field, parents, new, values_vm=None, want_vertex_major=False:
                        (torch.cat([field, field[:, :len(parents)]], 1), None))
    v = torch.nn.Parameter(torch.arange(18, dtype=torch.float32).reshape(6, 3))
    tracer = _MeshChangingTracer(v, torch.zeros(4, 4, dtype=torch.int32))
    tracer._tn_vertex_snapshot = v.detach().clone()
    model = SimpleNamespace(get_tetrahedra_tracer=lambda: tracer, tetrahedra_field=torch.zeros(64, 6), tetrahedra_vertices=v,
                            tetrahedra_cells=tracer.tetrahedra_cells, tetrahedra_occupancy=torch.ones(4),
                            config=SimpleNamespace(num_tetrahedra_vertices=6, num_tetrahedra_cells=4))

    def agree(V, T):
        w = model.tetrahedra_vertices
        assert isinstance(w, torch.nn.Parameter) and tracer.tetrahedra_vertices is w and w.shape == (V, 3)
        assert model.tetrahedra_cells is tracer.tetrahedra_cells and model.tetrahedra_cells.shape == (T, 4)
        assert model.tetrahedra_occupancy.shape == (T,) and model.tetrahedra_field.shape == (64, V)
        assert (model.config.num_tetrahedra_vertices, model.config.num_tetrahedra_cells) == (V, T)
        assert tracer._tn_vertex_key == (w._version, w.data_ptr())
        assert torch.equal(tracer._tn_vertex_snapshot, w.detach()) and tracer._tn_vertex_snapshot.data_ptr() != w.data_ptr()
        assert model._tn_tet_stats.shape == (T, 3) and not model._tn_tet_stats.any()

    model._tn_tet_stats = torch.ones(4, 3, dtype=torch.int64)
    res = plugin.densify(model, torch.tensor([1, 0, 1, 0]))
    assert (res["num_new"], res["num_cells"], res["retriangulated"], res["stats_reset"]) == (2, 10, False, True)
    agree(8, 10)
    model._tn_tet_stats = torch.ones(10, 3, dtype=torch.int64)
    res = plugin.densify(model, torch.tensor([1] + [0] * 9), retriangulate=True)
    assert (res["num_new"], res["num_cells"], res["retriangulated"], res["stats_reset"]) == (1, 15, True, True)
    assert model.tetrahedra_occupancy.tolist() == [2.0] * 15
    agree(9, 15)
    model._tn_tet_stats = torch.ones(15, 3, dtype=torch.int64)
    assert plugin._monitor_delaunay(tracer, model, 0.5, True)
    assert model._tn_retriangulations == 1 and model._tn_delaunay_counters.tolist() == [10, 9, 0, 0]
    agree(9, 17)


# ---------------------------------------------------------------------------------------------------------------- entries
def test_entry_is_declared_bound_and_exported():
    """an additive entry: the ABI number stays, the header declares it, the binding binds it, the library exports it"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_tet_stats_accumulate\(uint32_t num_cells, size_t num_rows, uint32_t samples_per_ray, const uint32_t \*cells,\s*"
                     r"const float \*sigma,\s*const float \*edges, const float \*ray_value, const uint32_t \*ray_index,\s*"
                     r"const uint32_t \*count,\s*int64_t \*stats, void \*stream\);", header)
    comment = header[header.index("per-tetrahedron training statistics"):header.index("int tn_tet_stats_accumulate")]
    for word in ("no reference counterpart", "2^23", "half to even", "NOT read", "8192"):
        assert word in comment, word
    lib = _lib.load()
    assert "tn_tet_stats_accumulate" in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "tn_tet_stats_accumulate")
    assert len(lib.tn_tet_stats_accumulate.argtypes) == 11
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    r = tc.render()
    assert hasattr(ext, "tet_stats_accumulate") and hasattr(ext, "tet_stats_new") and ext.TET_STATS_MAX_SAMPLES == 8192
    assert hasattr(r, "tet_stats_statement") and hasattr(r, "tet_stats_scores") and hasattr(r.TetraRenderer, "accumulate_tet_stats")
    z = ext.tet_stats_new(5, "cpu")
    assert z.dtype == torch.int64 and tuple(z.shape) == (5, 3) and not z.any()
    kernel = (CSRC / "tn_tet_stats.hip").read_text()
    assert "ray_composite(S, " in kernel and "nullptr, nullptr, nullptr, wl, lane)" in kernel        # the composite's own weights, in LDS
    assert "tetstats::accept" in kernel and "tetstats::weight_term" in kernel and "tetstats::error_term" in kernel


def test_the_entry_refuses_before_anything_runs():
    """every refusal is decided on the host, in front of the first call into the runtime: it can be asked for without a device"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    x = 64                                                                    # a pointer that is never followed

    def call(T=5, rows=2, S=8, cells=x, sigma=x, edges=x, ray_value=None, ray_index=None, count=None, stats=x):
        return lib.tn_tet_stats_accumulate(T, rows, S, cells, sigma, edges, ray_value, ray_index, count, stats, None)

    for kw in (dict(cells=None), dict(sigma=None), dict(edges=None), dict(stats=None)):
        assert call(**kw) != 0 and b"null" in lib.tn_last_error(), kw
    assert call(S=0) != 0 and b"samples_per_ray" in lib.tn_last_error()
    assert call(S=8193) != 0 and b"8192" in lib.tn_last_error()              # refused, not truncated
    assert call(rows=2 ** 32) != 0 and b"rows" in lib.tn_last_error()
    assert call(T=0, cells=None, stats=None) == 0 and call(rows=0, cells=None) == 0     # nothing to do: nothing is touched


def test_wrapper_and_renderer_refusals():
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    r = tc.render()
    stats, cells = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.tet_stats_accumulate(stats, cells, torch.zeros(2, 8), torch.zeros(2, 9))
    unbound = object.__new__(r.TetraRenderer)                                 # refused in front of everything else
    with pytest.raises(RuntimeError, match="fused=True"):
        r.TetraRenderer.render_train(unbound, None, None, fused=False, tet_stats=True)
    with pytest.raises(RuntimeError, match="occupancy_sampler"):
        r.TetraRenderer.render_train(unbound, None, None, occupancy_sampler=True, tet_stats=True)
    assert r.TetraRenderer.accumulate_tet_stats(unbound, stats, None, None) is stats           # no ray hit: nothing to add
