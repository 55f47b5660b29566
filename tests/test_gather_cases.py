"""The inputs and references of tests/gather_cases.py, checked without a GPU: the CPU oracle (oracle/tn_oracle.c, the fp32
sequential statement the forward kernels must equal bit for bit) stays within the a-priori bounds of the float64 references, equals
them exactly on the exact fill, and every case holds the conditions the bounds and the GPU tests rely on.  A failure of
tests/test_gather_edges_gpu.py is then the kernel's, not the test's.

Conditions on the CONTENT of a stream (a permuted-slot carry, both single-EMPTY slots, a duplicate, every forced edge) are asserted
on every case with n >= 63: the overlays are placed from n = 24 on and a stream of a few samples (n = 1 is one tuple) cannot
hold all of them; the edges that fit (7 -> 8 from n = 9 on) are asserted on every case."""
import numpy as np
import pytest

import gather_cases as gc

ALL_CASES = sorted(set(gc.FORWARD64_CASES + gc.FORWARD_CASES + gc.ADJOINT_CASES + gc.BARY_CASES))
EXTRA = [("run_lengths", gc.run_length_case), ("last_vertices", gc.last_vertices_case)]


def _worst(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("fill", ["random", "exact"])
@pytest.mark.parametrize("D", gc.DIMS)
def test_oracle_within_bounds_of_float64(oracle, D, fill):
    worst_f, worst_b = 0.0, 0.0
    cases = [(f"{c}", gc.case(*c, fill)) for c in ALL_CASES if c[0] == D]
    if D == 4:
        cases += [(name, make(fill)) for name, make in EXTRA]
    for name, c in cases:
        fwd = oracle.interpolate_values(c["vi"], c["bc"], c["field"]).astype(np.float64)
        err = np.abs(fwd - c["fwd"])
        bound = (D + 1) * gc.U * c["fwd_A"]
        worst_f = max(worst_f, _worst(err, bound))
        assert (err <= bound).all(), (name, "forward", _worst(err, bound))
        adj = oracle.interpolate_values_backward(c["vi"], c["bc"], c["field"], c["g"]).astype(np.float64).T
        err = np.abs(adj - c["adj"])
        bound = (c["count"][:, None] + 1) * gc.U * c["adj_A"]
        worst_b = max(worst_b, _worst(err, bound))
        assert (err <= bound).all(), (name, "adjoint", _worst(err, bound))
        if fill == "exact":
            assert np.array_equal(fwd, c["fwd"]), (name, "forward, exact fill")
            assert np.array_equal(adj, c["adj"]), (name, "adjoint, exact fill")
            assert not np.signbit(adj[c["count"] == 0]).any()
    print(f"D={D} {fill}: oracle error / bound, forward {worst_f:.3f}, adjoint {worst_b:.3f}")


@pytest.mark.parametrize("fill", ["random", "exact"])
def test_conditions_on_the_inputs(fill):
    cases = [(f"{c}", c[2], gc.case(*c, fill)) for c in ALL_CASES] + [(name, 0, make(fill)) for name, make in EXTRA]
    for name, n, c in cases:
        vi, bc, cnt = c["vi"], c["bc"], c["count"]
        D = vi.shape[1]
        assert vi.dtype == np.int32 and bc.dtype == np.float32 and vi.min() >= -1 and vi.max() < c["V"]
        assert int(cnt.max()) <= gc.MAX_COUNT, (name, int(cnt.max()))
        assert int(cnt.sum()) == int((vi >= 0).sum())
        if fill == "exact":
            assert 8 * 64 * int(cnt.max()) < 2 ** 24
            assert np.array_equal(bc * 8, np.round(bc * 8)) and float(bc.sum(1).max()) <= (D - 1) / 8
            w = gc.weights32(bc)
            assert float(w.min()) >= 0 and float(w[:, 0].min()) >= 1 / 8 and float(w.max()) <= 1
            for k in ("g", "field"):
                assert np.array_equal(c[k], np.round(c[k])) and float(np.abs(c[k]).max()) <= 8
        if n == 0:
            continue
        st = gc.stream_stats(vi)
        assert st["edges"] == st["expected_edges"], (name, st)
        if n >= 63:
            assert st["permuted_carry"] >= 1 and st["duplicate"] >= 1 and st["all_empty"] >= 1, (name, st)
            assert st["single_empty_slot0"] >= 1 and st["single_empty_last"] >= 1, (name, st)


def test_run_length_stream_has_the_lengths():
    for fill in ("random", "exact"):
        c = gc.run_length_case(fill)
        assert tuple(c["count"][:len(gc.DET_LENGTHS)]) == gc.DET_LENGTHS
        c = gc.last_vertices_case(fill)
        assert c["V"] == gc.DET_GRID + 37 and int(c["count"][:gc.DET_GRID].sum()) == 0 and (c["count"][gc.DET_GRID:] > 0).all()


def test_bounds_see_one_dropped_term():
    """The adjoint bound is meant to catch ONE lost contribution: at the largest count of the cases, dropping the largest
    term of an element moves it by more than the bound in most elements sampled (the reason for MAX_COUNT)."""
    c = gc.case(4, 64, 1000, "random")
    v = int(c["count"].argmax())
    s, k = np.argwhere(c["vi"] == v)[0]
    term = np.abs(gc.weights32(c["bc"])[s, k].astype(np.float64) * c["g"][s].astype(np.float64))
    bound = (c["count"][v] + 1) * gc.U * c["adj_A"][v]
    assert np.median(term / bound) > 10


def test_walk_stream_is_a_walk():
    """consecutive distinct full tuples of one ray share exactly D - 1 vertices"""
    rng = np.random.default_rng(5)
    for D in gc.DIMS:
        vi, _ = gc.walk_stream(rng, 4000, 500, D)
        full = (vi >= 0).all(1) & (np.array([len(set(r)) for r in vi.tolist()]) == D)
        a, b = vi[:-1][full[:-1] & full[1:]], vi[1:][full[:-1] & full[1:]]
        shared = np.array([len(set(x) & set(y)) for x, y in zip(a.tolist(), b.tolist())])
        assert (shared == D - 1).sum() > 300 and (shared == D).sum() > 1000
        runs = np.diff(np.flatnonzero(np.concatenate([[True], (vi[1:] != vi[:-1]).any(1), [True]])))
        assert runs.max() <= 12
