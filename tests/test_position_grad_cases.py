"""The cases of tests/position_grad_cases.py held to their own claims on the CPU, and the torch statement of part (B),
geometry.sample_positions_backward, in float32 held to the float64 references on every case the GPU test uploads: what
tests/test_position_grad_edges_gpu.py asserts of k_sample_positions_bwd is asserted here of the statement first, so a failure on the
GPU is the kernel's.  The loops of the kernel are modelled in numpy (position_grad_cases.loop_model): the true bounds visit every
sample of every table entry once, and each of three wrong bounds is rejected by some table entry -- the mutation argument for the
size tables, made on the model, never on the kernel."""
import importlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import position_grad_cases as pgc

EXACT_CASES = [("mixed", R, S) for R, S in pgc.EDGE_SHAPES] + [("rays", 8, S) for S in pgc.CLASS_RAY_S] + [("one_tet",) + pgc.ONE_TET_SHAPE]
RANDOM_CASES = [("mixed", R, S) for R, S in pgc.RANDOM_SHAPES] + [("rays", 8, S) for S in pgc.CLASS_RAY_S]


def _case(fill, kind, R, S):
    if kind == "one_tet":
        return pgc.one_tet_case()
    return pgc.class_ray_case(fill, S) if kind == "rays" else pgc.mixed_case(fill, R, S)


@pytest.fixture(scope="module")
def geometry():
    return importlib.import_module("tetra-nerf_amd.geometry")


def test_sizes_sit_on_the_edges():
    C, B, F = pgc.CHUNK, pgc.RAYS_PER_BLOCK, pgc.IN_FLIGHT
    assert F == pgc.RAYS_PER_BLOCK * pgc.MAX_BLOCKS == 32768
    chunks = lambda S: -(-S // C)             # noqa: E731
    # S: one sample; the last S of one partial chunk, the first full chunk, the first partial chunk after a full one; the same
    # around two chunks; a partial chunk of one lane after four full ones (a lane's fifth sample)
    assert pgc.S_EDGES == (1, 2, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 4 * C + 1)
    assert [chunks(S) for S in pgc.S_EDGES] == [1, 1, 1, 1, 2, 2, 2, 3, 5]
    assert [S % C for S in pgc.S_EDGES] == [1, 2, C - 1, 0, 1, C - 1, 0, 1, 1]
    # R: one block with idle waves, a full block, the first second block; the cap on either side; a third ray for wave 0
    assert pgc.R_EDGES == (1, B - 1, B, B + 1, F - 1, F, F + 1, 2 * F + 1)
    assert [pgc.launch(R)[0] for R in pgc.R_EDGES] == [1, 1, 1, 2, pgc.MAX_BLOCKS, pgc.MAX_BLOCKS, pgc.MAX_BLOCKS, pgc.MAX_BLOCKS]
    assert pgc.launch(F - 1 - B)[0] == pgc.MAX_BLOCKS - 1
    assert [pgc.trips(R) for R in pgc.R_EDGES] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert pgc.trips(2 * F) == 2
    # at R = 65,537 wave 0 of block 0 owns rays 0, 32,768 and 65,536
    _, _, writers = pgc.loop_model(2 * F + 1, 1)
    assert list(range(0, 2 * F + 1, pgc.launch(2 * F + 1)[1])) == [0, F, 2 * F] and bool((writers == 1).all())
    # every S edge runs at a handful of rays, the large R at S = 1 and 3 only: the largest case stays under 200 k samples
    assert {(R, S) for S in pgc.S_EDGES for R in pgc.R_SMALL} <= set(pgc.EDGE_SHAPES)
    assert {(R, S) for R in pgc.R_EDGES for S in (1, 3)} <= set(pgc.EDGE_SHAPES)
    assert max(R * S for R, S in pgc.EDGE_SHAPES) < 200_000
    assert 19_000 < pgc.ONE_TET_SHAPE[0] * pgc.ONE_TET_SHAPE[1] < 21_000
    assert set(pgc.CLASS_RAY_S) <= set(pgc.S_EDGES) and set(pgc.CHAIN_S) <= set(pgc.S_EDGES)


def test_the_restated_constants_are_the_launchers():
    """the three constants of position_grad_cases.py, read back from the kernel and its launcher: a change of the block, the chunk or
    the cap fails here first -- the tables then have to move with the edge"""
    text = (Path(__file__).resolve().parents[1] / "tetra-nerf_amd" / "csrc" / "tn_position_grad.hip").read_text()
    kernel = text[text.index("void k_sample_positions_bwd("):text.index("}  // namespace\n\nvoid launch_interpolate")]
    launcher = text[text.index("void launch_sample_positions_backward("):]

    def numbers(where, pattern):
        m = re.search(pattern, where)
        assert m, pattern
        return [int(g) for g in m.groups()]

    assert numbers(text, r"__launch_bounds__\((\d+)\) void k_sample_positions_bwd") == [64 * pgc.RAYS_PER_BLOCK]
    assert numbers(launcher, r"hipLaunchKernelGGL\(k_sample_positions_bwd, dim3\(grid\), dim3\((\d+)\)") == [64 * pgc.RAYS_PER_BLOCK]
    assert numbers(launcher, r"nblocks = \(R \+ (\d+)\) / (\d+);") == [pgc.RAYS_PER_BLOCK - 1, pgc.RAYS_PER_BLOCK]
    a, b, c, d = numbers(launcher, r"nblocks < (\d+)u \* (\d+)u \? nblocks : (\d+)u \* (\d+)u")
    assert a * b == c * d == pgc.MAX_BLOCKS
    assert numbers(kernel, r"for \(uint32_t s0 = 0; s0 < S; s0 \+= (\d+)\)") == [pgc.CHUNK]
    assert numbers(kernel, r"const int lane = threadIdx\.x & (\d+);") == [pgc.CHUNK - 1]
    assert "wave0 = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)" in kernel
    assert "nwaves = (size_t)gridDim.x * (blockDim.x >> 6)" in kernel
    assert "for (size_t r = wave0; r < R; r += nwaves)" in kernel


ALL_SHAPES = sorted(set(pgc.EDGE_SHAPES) | set(pgc.RANDOM_SHAPES) | {pgc.ONE_TET_SHAPE} | {(8, S) for S in pgc.CLASS_RAY_S})


def _model_is_right(R, S, **wrong):
    visits, lane, writers = pgc.loop_model(R, S, **wrong)
    s = np.arange(S)
    return bool((visits == 1).all()) and bool((writers == 1).all()) and bool((lane == (s % pgc.CHUNK)[None, :]).all())


def test_the_loops_visit_every_sample_once():
    for R, S in ALL_SHAPES:
        assert _model_is_right(R, S), (R, S)


@pytest.mark.parametrize("wrong", [dict(whole_chunks_only=True), dict(stride_off=-1), dict(ray_end_off=-1)], ids=lambda w: next(iter(w)))
def test_a_wrong_loop_bound_is_rejected_by_the_tables(wrong):
    """`s0 + 64 <= S`, a stride of nwaves - 1, `r < R - 1`: each fails at some (R, S) of the tables"""
    caught = [(R, S) for R, S in pgc.EDGE_SHAPES if not _model_is_right(R, S, **wrong)]
    print(f"{wrong}: rejected by {len(caught)} of {len(pgc.EDGE_SHAPES)} table entries, first {caught[:3]}")
    assert caught
    if "stride_off" in wrong:         # shows where the last wave's ray is taken again by wave 0: a full last block, or a second trip
        assert all(R >= pgc.launch(R)[1] for R, S in caught) and any(R > pgc.IN_FLIGHT for R, S in caught)
    if "whole_chunks_only" in wrong:
        assert all(S % pgc.CHUNK for R, S in caught)


def _statement32(geometry, c):
    S = c["S"]
    t = lambda k, shape: torch.from_numpy(np.array(c[k])).reshape(shape)      # noqa: E731
    return geometry.sample_positions_backward(t("vi", (-1, 4)), t("bc", (-1, 3)), t("gb", (-1, 3)), t("verts", (-1, 3)), t("t", (-1,)), S)


def _check_zeros(c, out):
    """exact zeros at every dead sample, in the rows of all-dead rays, at every vertex that no live sample names"""
    ref = c["ref"]
    live = ref["live"]
    assert torch.equal(out["live"].reshape(live.shape), live)
    pts = out["points"].reshape(c["R"], c["S"], 3)
    assert bool((pts[~live] == 0).all())
    dead_rays = ~live.any(1)
    assert bool((out["origins"][dead_rays] == 0).all()) and bool((out["directions"][dead_rays] == 0).all())
    assert bool((out["vertices"][~ref["named"]] == 0).all())
    for k in ("points", "origins", "directions", "vertices"):
        assert bool(torch.isfinite(out[k]).all()), k


def _check_shares(c, mixed=True):
    """`mixed`: a case whose classes are the seeded draw (a class-ray case holds whole rays of every class instead)"""
    sh = pgc.shares(c)
    n = c["R"] * c["S"]
    assert 2 * sh["live"] >= n or not mixed, sh
    assert sh["live"] == sh[pgc.LIVE] + sh[pgc.CONTROL]                    # the classes are what the reference finds dead
    if n >= 64:
        assert all(sh[k] >= 1 for k in pgc.DEAD_CLASSES), sh
        assert sh["poisoned"] >= 3, sh
        for k in pgc.DEAD_CLASSES if mixed else ():
            assert abs(sh[k] - n / 16) <= 1 + 4 * np.sqrt(n / 16), (k, sh)
    assert pgc.check_gap(c["ref"]["size"].numpy())
    ids = c["vi"].reshape(-1, 4).astype(np.int64)
    poisoned = np.isnan(c["bc"].reshape(-1, 3)).any(1)
    assert np.isin(c["cls"].reshape(-1)[poisoned], pgc.ID_DEAD).all()      # poison sits on id-dead samples only
    assert bool((((ids < 0) | (ids >= c["V"])).any(1) == np.isin(c["cls"].reshape(-1), pgc.ID_DEAD)).all())
    return sh


@pytest.mark.parametrize("kind,R,S", EXACT_CASES)
def test_exact_fill(geometry, kind, R, S):
    c = _case("exact", kind, R, S)
    ref = c["ref"]
    sh = _check_shares(c, kind != "rays")
    margin = pgc.exactness_margin(c, ref)
    assert margin < 1, margin
    # the fill is what the module says it is
    live = ref["live"].numpy()
    assert np.array_equal(c["verts"][:-20], np.round(c["verts"][:-20])) and float(np.abs(c["verts"][:-20]).max()) <= 8
    fin = np.isfinite(c["bc"]).all(-1) & np.isfinite(c["gb"]).all(-1)
    for k, unit, lo, hi in (("bc", 8, -1 / 8, 1), ("t", 4, 0, 16)):
        v = c[k][fin]
        assert np.array_equal(v * unit, np.round(v * unit)) and v.min() >= lo and v.max() <= hi, k
    assert np.abs(c["gb"][live]).max() <= 4 and np.array_equal(c["gb"][live], np.round(c["gb"][live]))
    for r in range(min(c["R"], 64)):              # no two live samples of a ray share a g
        g = c["gb"][r][live[r] & (c["cls"][r] == pgc.LIVE)]
        assert len(np.unique(g, axis=0)) == len(g)
    m = ref["points"].numpy()
    assert np.array_equal(m * 4, np.round(m * 4))
    if kind == "one_tet":
        named = ref["named"].numpy()
        assert int(named.sum()) == 4 and sh["live"] > 10_000
    # the statement in float32: the float64 reference bit for bit, in any order of the samples
    out = _statement32(geometry, c)
    _check_zeros(c, out)
    for k in ("points", "origins", "directions", "vertices"):
        want = ref[k].to(torch.float32)
        assert torch.equal(want.double(), ref[k]), k                      # the reference is a float32 number
        assert torch.equal(out[k].reshape(want.shape), want), k
    if c["R"] * c["S"] <= 20_000:
        # the float64 statement says the same once the samples it cannot call dead (|m64| >= 2^128) have no gradient
        out64 = geometry.sample_positions_backward(
            torch.from_numpy(np.array(c["vi"])).reshape(-1, 4), torch.from_numpy(np.array(c["bc"])).reshape(-1, 3).double(),
            torch.where((ref["size"] >= pgc.F32_RANGE)[:, None], torch.zeros(1, dtype=torch.float64),
                        torch.from_numpy(np.array(c["gb"])).reshape(-1, 3).double()),
            torch.from_numpy(np.array(c["verts"])).double(), torch.from_numpy(np.array(c["t"])).reshape(-1).double(), c["S"],
            weights=torch.from_numpy(pgc.weights32(c["bc"].reshape(-1, 3))).double())
        for k in ("points", "origins", "directions", "vertices"):
            assert torch.equal(out64[k].reshape(ref[k].shape), ref[k]), k
        # a permutation of the rays (and with it of the order of every vertex sum): the same vertex bits
        perm = torch.randperm(c["R"], generator=torch.Generator().manual_seed(1))
        t = lambda k: torch.from_numpy(np.array(c[k]))[perm]              # noqa: E731
        out_p = geometry.sample_positions_backward(t("vi").reshape(-1, 4), t("bc").reshape(-1, 3), t("gb").reshape(-1, 3),
                                                   torch.from_numpy(np.array(c["verts"])), t("t").reshape(-1), c["S"])
        assert torch.equal(out_p["vertices"], out["vertices"]) and torch.equal(out_p["origins"], out["origins"][perm])


@pytest.mark.parametrize("kind,R,S", RANDOM_CASES)
def test_random_fill(geometry, kind, R, S):
    c = _case("random", kind, R, S)
    ref = c["ref"]
    _check_shares(c, kind != "rays")
    live = ref["live"]
    bc, t = c["bc"][live.numpy()], c["t"]
    assert bc.min() >= 0 and bc.sum(-1).max() <= 1 + 1e-6                  # inside the cell
    for r in range(c["R"]):                                                # t increases along the ray (NaN: poison)
        tr = t[r][np.isfinite(t[r])]
        assert bool((np.diff(tr) > 0).all())
    out = _statement32(geometry, c)
    _check_zeros(c, out)
    err = (out["points"].reshape(c["R"], c["S"], 3).double() - ref["points"]).norm(dim=-1)
    assert bool((err <= ref["bound_points"]).all())
    worst = {"points": float((err / ref["bound_points"].clamp_min(1e-300)).max())}
    for k, b in (("origins", "bound_o"), ("directions", "bound_d"), ("vertices", "bound_v")):
        e = (out[k].double() - ref[k]).abs()
        worst[k] = float((e / ref[b].clamp_min(1e-300)).max())
        assert bool((e <= ref[b]).all()), (k, worst[k])
    print(f"statement fp32 {kind} R={c['R']} S={S}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_the_control_is_live_and_large():
    for fill in ("exact", "random"):
        c = pgc.class_ray_case(fill, 65)
        ctl = c["cls"] == pgc.CONTROL
        assert bool(c["ref"]["live"].numpy()[ctl].all())
        size = c["ref"]["size"].numpy().reshape(c["cls"].shape)
        big = size[ctl & (np.abs(c["gb"][..., 0]) >= 0.25)]
        assert len(big) and 2.0 ** 98 <= big.min() and big.max() <= 2.0 ** 103
        over = np.isin(c["vi"][..., 1], c["special"]["tiny"][1:2]) | np.isin(c["vi"][..., 1], c["special"]["needle"][1:2])
        assert over.any() and bool((size[over] > 2.0 ** 148).all()) and not c["ref"]["live"].numpy()[over].any()


def test_poisoned_dead_samples_give_exact_zeros_in_the_statement(geometry):
    """class 6, the disagreement this file was written around: an id-dead sample with NaN barycentrics, NaN t and NaN g.  Selected
    away (torch.where), not multiplied by zero: vertices and directions stay finite and equal the unpoisoned call bit for bit."""
    c = pgc.class_ray_case("exact", 65)
    assert pgc.shares(c)["poisoned"] > 65
    out = _statement32(geometry, c)
    clean = {k: np.array(c[k]) for k in ("bc", "gb", "t")}
    bad = np.isnan(clean["bc"]).any(-1)
    assert bad.any() and np.isnan(clean["t"][bad]).all() and np.isnan(clean["gb"][bad]).all()
    for k in clean:
        clean[k][bad] = 0.25
    ref = geometry.sample_positions_backward(torch.from_numpy(np.array(c["vi"])).reshape(-1, 4), torch.from_numpy(clean["bc"]).reshape(-1, 3),
                                             torch.from_numpy(clean["gb"]).reshape(-1, 3), torch.from_numpy(np.array(c["verts"])),
                                             torch.from_numpy(clean["t"]).reshape(-1), c["S"])
    for k in ("points", "origins", "directions", "vertices"):
        assert bool(torch.isfinite(out[k]).all()), k
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("S", pgc.CHAIN_S)
def test_chain_statement_in_fp32_meets_the_derived_tolerance(geometry, S):
    """(A) then (B) as torch statements in float32 against float64 autograd of the forward statement (position_grad_cases.
    chain_reference derives the tolerance): the convention of the case -- bc, t, o, d, the vertex order -- is the forward's."""
    c = pgc.chain_case(S)
    ref = c["ref"]
    n = c["R"] * S
    assert 2 * int(ref["live"].sum()) >= n and (S == 1 or int((~ref["live"]).sum()) > 0)
    t = lambda k: torch.from_numpy(np.array(c[k]))                      # noqa: E731
    gb = geometry.gather_backward_barycentrics(t("vi").reshape(n, 4), t("field").t().contiguous(), t("G").reshape(n, -1))
    out = geometry.sample_positions_backward(t("vi").reshape(n, 4), t("bc").reshape(n, 3), gb, t("verts"), t("t").reshape(n), S)
    assert torch.equal(out["live"], ref["live"])
    for k, b in (("origins", "bound_o"), ("directions", "bound_d"), ("vertices", "bound_v")):
        err = (out[k].double() - ref[k]).abs()
        print(f"chain statement fp32 S={S} {k}: worst error / tolerance {float((err / ref[b].clamp_min(1e-300)).max()):.3f}, "
              f"max |gradient| {float(ref[k].abs().max()):.3g}")
        assert bool((err <= ref[b]).all()), k
        assert bool((out[k][ref[b] == 0] == 0).all()), k
        # the tolerance pins the convention: on most elements it is a small part of the gradient, where a wrong sign, vertex order
        # or ray parameter is an error of the order of the gradient itself
        rel = float((ref[b] / ref[k].abs().clamp_min(1e-300))[ref[k] != 0].median())
        print(f"    median tolerance / |gradient| = {rel:.2e}")
        assert float(ref[k].abs().max()) > 0 and rel < 0.05
