"""Named cases of the per-tetrahedron training statistics (tn_tet_stats_accumulate; the rule: csrc/tn_tet_stats_core.h, the
statement: render.tet_stats_statement), shared by tests/test_tet_stats.py (CPU: statement, restatement, host emulation) and
tests/test_tet_stats_gpu.py.

A case is a dict of numpy arrays: T, cells i32 [rows, S] (-1 = unmatched), weights f32 [rows, S] (given weights: the CPU tests do
not form them; the GPU tests replace them by the composite's own), ray_value f32 [rays] or None, ray_index i32 [rows] or None,
count int or None, stats0 i64 [T, 3] (non-zero: the entry accumulates)."""
import importlib

import numpy as np

EMPTY = -1
TWO32 = float(2 ** 32)


def render():
    return importlib.import_module("tetra-nerf_amd.render")


def run_cells(rng, rows, S, T, longest=100):
    """cells of `rows` rays: runs of random length 1 .. longest of random ids < T -- runs start, end and cross every 64-lane
    boundary, neighbouring runs may name the same tetrahedron, and a tetrahedron may come back later on the ray (A B A)"""
    cells = np.empty((rows, S), np.int32)
    for q in range(rows):
        at = 0
        while at < S:
            n = int(rng.integers(1, longest + 1))
            cells[q, at:at + n] = int(rng.integers(0, T))
            at += n
    return cells


def stats0(rng, T):
    return rng.integers(1, 1 << 40, size=(T, 3), dtype=np.int64)


def _case(T, cells, weights, ray_value=None, ray_index=None, count=None, seed=0):
    cells = np.ascontiguousarray(cells, np.int32)
    return {"T": int(T), "cells": cells, "weights": np.ascontiguousarray(weights, np.float32).reshape(cells.shape),
            "ray_value": None if ray_value is None else np.ascontiguousarray(ray_value, np.float32),
            "ray_index": None if ray_index is None else np.ascontiguousarray(ray_index, np.int32),
            "count": count, "stats0": stats0(np.random.default_rng(1000 + seed), T)}


def _runs(seed=1, rows=5, S=200, T=37):
    rng = np.random.default_rng(seed)
    return _case(T, run_cells(rng, rows, S, T), rng.random((rows, S), dtype=np.float32), 4 * rng.random(rows, dtype=np.float32), seed=seed)


def _aba():
    rng = np.random.default_rng(2)
    cells = np.tile(np.int32([3, 5, 3, 3, 5, 0, 3]), 30)[None, :200].repeat(2, 0)
    return _case(7, cells, rng.random(cells.shape, dtype=np.float32), np.float32([0.25, 3.0]), seed=2)


def _one_tet():
    rng = np.random.default_rng(3)
    return _case(1, np.zeros((3, 130), np.int32), rng.random((3, 130), dtype=np.float32), np.float32([1, 2, 0.5]), seed=3)


def _all_distinct():
    rng = np.random.default_rng(4)
    rows, S = 3, 129
    return _case(rows * S, np.arange(rows * S).reshape(rows, S), rng.random((rows, S), dtype=np.float32), rng.random(rows, dtype=np.float32), seed=4)


def _invalid_ids():
    rng = np.random.default_rng(5)
    T, rows, S = 11, 4, 150
    cells = run_cells(rng, rows, S, T, longest=9)
    pick = rng.integers(0, 4, size=cells.shape)
    cells = np.where(pick == 0, EMPTY, np.where(pick == 1, T + (cells & 1), cells)).astype(np.int32)    # -1, T, T + 1
    cells[0, :3] = (T, T + 1, EMPTY)
    return _case(T, cells, rng.random((rows, S), dtype=np.float32) + 0.25, 1 + rng.random(rows, dtype=np.float32), seed=5)


def _count_rows():
    """the sync-free form: 6 rows of which 3 are real, the padded ones repeat ray 4 with weights that would show"""
    rng = np.random.default_rng(6)
    T, rows, S = 9, 6, 70
    cells = run_cells(rng, rows, S, T, longest=20)
    weights = rng.random((rows, S), dtype=np.float32)
    weights[3:] = 1.0
    return _case(T, cells, weights, 1 + rng.random(8, dtype=np.float32), np.int32([4, 6, 7, 4, 4, 4]), count=3, seed=6)


def _half_ties():
    """weights whose 2^32-fold is k + 1/2 exactly (half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4) or k + 3/4 (truncation
    loses one), and a ray value of 1/2 and 3/2 that makes more of them in the error channel"""
    k = np.arange(64, dtype=np.float64)
    w = np.concatenate([(k + 0.5) / TWO32, (k + 0.75) / TWO32, (2 * k + 1) / TWO32]).astype(np.float32)
    cells = (np.arange(w.size) // 5 % 4).astype(np.int32)
    return _case(4, np.stack([cells, cells]), np.stack([w, w]), np.float32([0.5, 1.5]), seed=7)


def _value_edges():
    """every branch of the two clamps: ray values NaN, -1, -0, 0, 256, 257, inf, a small one; weights NaN, negative, -0, above 1, inf"""
    v = np.float32([np.nan, -1, -0.0, 0, 256, 257, np.inf, 1e-3])
    w = np.float32([0.5, np.nan, -0.5, -0.0, 1.0, 1.5, np.inf, 0.999, 2.0 ** -40, 1e-45])
    weights = np.tile(w, (len(v), 2))
    cells = np.tile(np.arange(weights.shape[1], dtype=np.int32) % 3, (len(v), 1))
    return _case(3, cells, weights, v, seed=8)


def _no_ray_value():
    c = _runs(seed=9, rows=2, S=65, T=5)
    c["ray_value"] = None
    return c


def _ray_index_only():
    rng = np.random.default_rng(10)
    T, rows, S = 6, 4, 64
    return _case(T, run_cells(rng, rows, S, T, 30), rng.random((rows, S), dtype=np.float32), np.float32([9, 0.5, 2, 7, 100]), np.int32([4, 0, 0, 2]), seed=10)


_BUILDERS = {"runs": _runs, "aba": _aba, "one_tet": _one_tet, "all_distinct": _all_distinct, "invalid_ids": _invalid_ids,
             "count_rows": _count_rows, "count_zero": lambda: dict(_count_rows(), count=0), "half_ties": _half_ties,
             "value_edges": _value_edges, "no_ray_value": _no_ray_value, "ray_index_only": _ray_index_only,
             "single_sample": lambda: _case(2, [[1], [1], [0]], [[0.5], [0.25], [1.0]], [2.0, 4.0, 300.0], seed=11)}
_CACHE = {}


def names():
    return tuple(_BUILDERS)


def case(name):
    if name not in _CACHE:
        c = _BUILDERS[name]()
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def statement(c, stats=None, weights=None):
    return render().tet_stats_statement(c["stats0"] if stats is None else stats, c["cells"], c["weights"] if weights is None else weights,
                                        c["ray_value"], c["ray_index"], c["count"])


# ---- the plain-loop restatement, with named mutations of the rule ----------------------------------------------------------------
MUTATIONS = ("truncate", "accept_ids_above_T", "read_padded_rows", "no_value_clamp")


def _rint_half_even(x):
    """x >= 0, an exact binary fraction held in a Python float"""
    lo = int(x)
    frac = x - lo
    return lo + 1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else lo


def restatement(c, mutation=None):
    """the rule sample by sample in Python scalars; fp32 products through numpy scalars, the scaling by 2^32 in exact doubles"""
    assert mutation is None or mutation in MUTATIONS
    T, cells, weights = c["T"], c["cells"], c["weights"]
    out = [[int(x) for x in row] for row in c["stats0"]]
    rows = cells.shape[0] if c["count"] is None or mutation == "read_padded_rows" else min(cells.shape[0], c["count"])
    quantise = (lambda x: int(x)) if mutation == "truncate" else _rint_half_even
    for q in range(rows):
        ray = q if c["ray_index"] is None else int(c["ray_index"][q])
        v = np.float32(1) if c["ray_value"] is None else c["ray_value"][ray]
        vh = (v if mutation == "no_value_clamp" and v < np.inf else np.float32(256) if v > 256 else v) if v >= 0 else np.float32(0)
        for i in range(cells.shape[1]):
            t = int(cells[q, i]) & 0xFFFFFFFF
            if mutation == "accept_ids_above_T" and t != 0xFFFFFFFF:
                t %= T
            if not t < T:
                continue
            w = weights[q, i]
            wh = (np.float32(1) if w > 1 else w) if w >= 0 else np.float32(0)
            out[t][0] += 1
            out[t][1] += quantise(float(wh) * TWO32)
            out[t][2] += quantise(float(np.float32(wh * vh)) * TWO32)
    return np.array(out, dtype=np.int64)


# ---- GPU inputs: sigma and edges whose composite weights take the place of a case's given weights ---------------------------------
def sigma_edges(rng, rows, S, scale=3.0):
    """ascending edges on [0.5, 6.5] and densities with a long tail, an optical depth of about 2 * scale along the ray whatever S:
    weights from tiny to nearly 1"""
    steps = rng.random((rows, S + 1), dtype=np.float32) + np.float32(0.01)
    edges = np.float32(0.5) + np.cumsum(steps, axis=1, dtype=np.float32) * np.float32(6.0 / (S + 1))
    sigma = rng.standard_exponential((rows, S)).astype(np.float32) ** 2 * np.float32(scale / 3.0)
    return np.ascontiguousarray(sigma, np.float32), np.ascontiguousarray(edges, np.float32)
