"""tests/mlp_edge_cases.py without a GPU: what makes a failure of tests/test_mlp_edges_gpu.py the kernel's and not the test's.

1. the sizes sit on the edges they name, given the launchers' constants restated in mlp_edge_cases.py (the table of the sizes is
   restated here in numbers, not recomputed);
2. the integer fills are exact (every partial sum an integer below 2^24), the single rows sit where they claim to, no reference
   output is identically zero;
3. on `random` and on the real problem, at the three smallest sizes and one mid size, the fp32 PyTorch evaluation of every
   statement -- one admissible order of the same fp32 arithmetic -- meets the bound the GPU test applies to the kernel;
4. every real problem has live and dead ReLU units in every layer at the first and last sample of every edge named."""
import math
import re
from pathlib import Path

import pytest
import torch

import dw_x3_cases as dw
import mlp_edge_cases as cases
from gather_cases import U

SHAPES = [(R, S) for R, S, _ in cases.SIZES]
STATEMENT_SHAPES = [(1, 1), (127, 1), (8, 16), (113, 145)]      # the three smallest and one mid size


def test_sizes_sit_on_the_edges():
    ns = [R * S for R, S in SHAPES]
    assert ns == [1, 127, 128, 129, 255, 256, 257, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536, 65537, 65537, 65793, 66049]
    assert len(set(SHAPES)) == len(SHAPES)
    for R, S in SHAPES:
        assert math.gcd(S, 32) == 1 or (R, S) in ((8, 16), (16, 16), (2048, 8), (4096, 8), (4096, 16)), (R, S)
    groups = lambda n, g: -(-n // g)
    # k_mlp_forward*: 256-sample groups, 256 blocks
    assert (cases.FWD_GROUP, cases.GROUP_GRID) == (256, 256)
    assert [groups(n, 256) for n in (255, 256, 257)] == [1, 1, 2]
    assert [groups(n, 256) for n in (65535, 65536, 65537, 65793, 66049)] == [256, 256, 257, 258, 259]
    assert 65537 - 256 * 256 == 1                      # block 0's second group holds one sample
    assert 65793 - 257 * 256 == 1 and 257 % 256 == 1   # group 256 (full) on block 0, group 257 (one sample) on block 1
    assert 66049 - 258 * 256 == 1 and 258 % 256 == 2   # groups 256, 257 (full) on blocks 0, 1, group 258 (one sample) on block 2
    # k_mlp_backward*: 128-sample groups, 256 blocks
    assert cases.DX_GROUP == 128
    assert [n % 128 for n in (127, 128, 129)] == [127, 0, 1]
    assert [groups(n, 128) for n in (32767, 32768, 32769)] == [256, 256, 257] and 32769 - 256 * 128 == 1
    # the GEMMs: slices of a multiple of 32 samples, 512 at most
    assert [cases.slicing(n, 32) for n in (16383, 16384, 16385)] == [(512, 32), (512, 32), (257, 64)]
    assert 16385 - 256 * 64 == 1 and 16383 - 511 * 32 == 31
    # the rgb head: multiples of 128
    assert [cases.slicing(n, 128) for n in (65535, 65536, 65537)] == [(512, 128), (512, 128), (257, 256)]
    # the per-ray sums and the compaction
    assert cases.RAY_GRID == 2048 and cases.RAY_SUB == 8 and (2048, 8) in SHAPES and (4096, 8) in SHAPES
    assert {R for R, _ in cases.RAY_SUM_SIZES} == {1, 2047, 2048, 2049, 4097} and {S for _, S in cases.RAY_SUM_SIZES} == {1, 7, 8, 9, 17}
    assert cases.COMPACT_ROWS == [2048 * 256 - 1, 2048 * 256, 2048 * 256 + 1]
    assert (cases.COMPACT_GRID, cases.COMPACT_BLOCK) == (2048, 256)
    assert {R * S for R, S in cases.FORWARD_EDGES} == {1, 255, 256, 257, 65535, 65536, 65537, 65793, 66049} and len(cases.FORWARD_EDGES) == 10
    assert {R * S for R, S in cases.DX_EDGES} == {127, 128, 129, 32767, 32768, 32769, 65537} and len(cases.DX_EDGES) == 8
    assert cases.second_owner_rows(65793) == dict(fwd=65536, dx=32768, dw=160, rgb=256)
    assert cases.second_owner_rows(32769) == dict(dx=32768, dw=96, rgb=128) and cases.second_owner_rows(128) == dict(dw=32)


def test_the_restated_constants_are_the_launchers():
    """the constants of mlp_edge_cases.py, read back from the launchers' source: a change of a block cap, a group or a slice unit
    fails here first -- SIZES (and the table above) then have to move with the edge"""
    csrc = Path(__file__).resolve().parents[1] / "tetra-nerf_amd" / "csrc"
    text = {name: (csrc / name).read_text() for name in ("tn_mlp_common.h", "tn_mlp_bwd.hip", "tn_mlp_grad.hip", "tn_occupancy_train.hip")}

    def number(name, pattern):
        m = re.search(pattern, text[name])
        assert m, (name, pattern)
        return [int(g) for g in m.groups()]

    assert number("tn_mlp_common.h", r"constexpr int MLP_BLOCK = (\d+);") == [2 * cases.FWD_GROUP]          # 32 samples per 64-lane wave
    assert number("tn_mlp_bwd.hip", r"constexpr int BWD_BLOCK = (\d+);") == [2 * cases.DX_GROUP]
    assert number("tn_mlp_common.h", r"const size_t group = \(size_t\)\(block / (\d+)\) \* (\d+);") == [64, 32]
    assert number("tn_mlp_common.h", r"return \(unsigned\)\(ngroups < (\d+) \? ngroups : (\d+)\);") == [cases.GROUP_GRID] * 2
    assert number("tn_mlp_grad.hip", r"constexpr int DW_GRID = (\d+);") == [cases.DW_GRID]
    assert re.findall(r"slicing\(n, (\d+)\)", text["tn_mlp_grad.hip"]) == [str(cases.DW_UNIT), str(cases.RGB_UNIT)]
    for name in ("tn_mlp_bwd.hip", "tn_occupancy_train.hip"):
        a, b, c, d = number(name, r"rays < (\d+) \* (\d+) \? rays : (\d+) \* (\d+)")
        assert a * b == c * d == cases.RAY_GRID
        assert "threadIdx.x >> 3, sub = threadIdx.x & 7" in text[name] and cases.RAY_SUB == 8
    assert number("tn_occupancy_train.hip", r"blocks = \(n_live \+ (\d+)\) / (\d+);") == [cases.COMPACT_BLOCK - 1, cases.COMPACT_BLOCK]
    assert number("tn_occupancy_train.hip", r"blocks < (\d+) \? blocks : (\d+)") == [cases.COMPACT_GRID] * 2


# where the single row of one_first_of_second_trip sits: n -> (second GEMM slice, second rgb-head slice)
SECOND_SLICE = {1: (None, None), 127: (32, None), 128: (32, None), 129: (32, 128), 257: (32, 128), 16383: (32, 128), 16384: (32, 128),
                16385: (64, 128), 32768: (64, 128), 32769: (96, 128), 65536: (128, 128), 65537: (160, 256), 65793: (160, 256), 66049: (160, 256)}


@pytest.mark.parametrize("R,S", SHAPES, ids=cases.IDS)
def test_fills(R, S):
    n = R * S
    assert cases.exactness_condition(n)
    slack = (1 + 2.0 ** -7) ** 2
    fills = [("small", None), ("one_last", None), ("random", None)]
    fills += [("one_first_of_second_trip", unit) for unit in (cases.DW_UNIT, cases.RGB_UNIT) if cases.slicing(n, unit)[0] > 1]
    for kind, unit in fills:
        f = cases.fill(kind, R, S) if unit is None else cases.fill(kind, R, S, unit)
        assert f["dhead"].shape == (4, n) and f["dirs"].shape == (R, 3) and all(f[k].shape == (n, w) for k, w in dw.WIDTH.items())
        if kind != "random":
            assert dw.exact_in_fp32(f), kind
            assert float((f["dhead"][1:4].double().abs() @ f["h4"].double().abs()).max()) * slack < dw.EXACT_LIMIT
            assert float(f["dhead"].double().abs().sum(1).max()) < dw.EXACT_LIMIT
            assert all(bool((f[k] == f[k].round()).all()) for k in list(dw.WIDTH) + ["dhead"])
        if kind == "one_last":
            assert cases.nonzero_rows(f) == [n - 1]
        if kind == "one_first_of_second_trip":
            row = cases.slicing(n, unit)[1]
            assert cases.nonzero_rows(f) == [row] and 0 < row < n
            if n in SECOND_SLICE:
                assert row == SECOND_SLICE[n][0 if unit == cases.DW_UNIT else 1]
            assert bool((f["d4"][row] == torch.arange(1, 129)).all()) and f["dhead"][:, row].tolist() == [3.0, -2.0, 5.0, 7.0]
        # no reference output is identically zero (fp32 is enough to see that)
        ref = cases.param_sums_in(f, torch.float32)
        assert set(ref) == {"w1", "b1", "w2", "b2", "w3", "b3", "wd", "bd", "wh", "bh", "wr", "br"}
        for k, v in ref.items():
            assert float(v.abs().max()) > 0, (kind, k)
        assert float(ref["wh"][:, :27].abs().max()) > 0 and float(ref["wh"][:, 27:].abs().max()) > 0
    for unit, col in ((cases.DW_UNIT, 0), (cases.RGB_UNIT, 1)):
        if n in SECOND_SLICE and SECOND_SLICE[n][col] is None:
            assert cases.slicing(n, unit)[0] == 1


def test_one_ray_fill_and_the_lists():
    f = cases.one_ray(65537, 1, 160)
    assert cases.nonzero_rows(f) == [160] and dw.exact_in_fp32(f)
    f = cases.one_ray(43, 3, 11)
    assert cases.nonzero_rows(f) == [33, 34, 35]
    for rays, S in cases.RAY_SUM_SIZES:
        for kind in ("small", "random"):
            assert float(cases.ray_d4(kind, rays, S).abs().view(rays, S, 128).sum((1, 2)).min()) > 0      # every ray has a term
        listed, last = cases.dropping_list(rays, S)
        ray = torch.div(listed.long(), S, rounding_mode="floor")
        assert bool((listed[1:] > listed[:-1]).all()) and not bool((ray % 7 == 3).any()) and int(ray[-1]) == last
        counts = torch.bincount(ray, minlength=rays)
        want = torch.full((rays,), S)
        want[torch.arange(rays) % 7 == 3] = 0
        want[last] = 1
        assert torch.equal(counts, want) and int(listed[-1]) == last * S
    val, mag, cnt = cases.ray_sums(cases.ray_d4("small", 9, 7), 7)
    assert val.shape == (9, 128) and bool((cnt == 7).all()) and bool((val == val.round()).all()) and float(mag.max()) <= 56


def test_the_two_statements_of_the_parameter_sums_agree():
    """param_sums (tests/test_dw_x3_gpu.py::_references on quad-major buffers + the rgb head) = param_sums_in(float64) on the plain
    fill: the layout helpers and the two formulas say the same"""
    for R, S in ((43, 3), (1, 257)):
        f = cases.fill("random", R, S)
        ref = cases.param_sums(cases.quad_buffers(f), f["dirs"], S)
        plain = cases.param_sums_in(f, torch.float64)
        for k in plain:
            assert torch.allclose(ref[k][0], plain[k], rtol=1e-13, atol=0), k
            assert bool((ref[k][1] >= ref[k][0].abs() * (1 - 1e-12)).all()), k


@pytest.mark.parametrize("R,S", STATEMENT_SHAPES, ids=lambda v: str(v))
def test_fp32_pytorch_meets_the_bounds_the_gpu_test_applies(R, S):
    n = R * S
    # parameter sums on `random`: (c + 1) u sum |terms|, c = n
    f = cases.fill("random", R, S)
    ref = cases.param_sums(cases.quad_buffers(f), f["dirs"], S)
    got = cases.param_sums_in(f, torch.float32)
    for k, (d64, mag) in ref.items():
        err = (got[k].double() - d64).abs()
        assert bool((err <= cases.sum_bound(mag, n)).all()), (k, float((err / cases.sum_bound(mag, n).clamp_min(1e-300)).max()))
    # per-ray sums: (S + 1) u sum |terms|
    d4 = cases.ray_d4("random", R, S)
    val, mag, cnt = cases.ray_sums(d4, S)
    got = d4.view(R, S, 128).sum(1)
    assert bool(((got.double() - val).abs() <= (S + 1) * U * mag).all()) and float(val.abs().max()) > 0
    # the network layer by layer from the STORED (fp32) layer before, and the dX chain, on the real problem
    p = cases.problem(R, S)
    w = p["w"]
    for biased in (False, True):
        net = {k: v.float() for k, v in cases.network(p, cases.gather64(p), biased=biased).items()}      # what a run stores
        steps = [(net["x0"], w[0], w[1], None, "h1"), (net["h1"], w[2], w[3], None, "h2"), (net["h2"], w[4], w[5], None, "h3")]
        hin, bias = cases.head_input(p, net["h3"])
        steps.append((hin, w[8], w[9], bias if biased else None, "h4"))
        for x, W, b, extra, name in steps:
            h32, bound = cases.layer(x, W, b, extra, dtype=torch.float32)
            h64, _ = cases.layer(x, W, b, extra)
            assert bool(((h32.double() - h64).abs() <= bound).all()), name
            assert float((net[name].double() - h64).abs().max()) <= float(bound.max())      # (and the chain of statements holds together)
        dsr = net["dhead"][0][:, None]
        chain = [(net["d4"], w[8][:, 27:], net["h3"] > 0, dsr * w[6], "d3"), (net["d3"], w[4], net["h2"] > 0, None, "d2"),
                 (net["d2"], w[2], net["h1"] > 0, None, "d1"), (net["d1"], w[0], None, None, "dx0")]
        for d_in, W, mask, extra, name in chain:
            d32, bound = cases.dx_layer(d_in, W, mask, extra, dtype=torch.float32)
            d64, _ = cases.dx_layer(d_in, W, mask, extra)
            assert bool(((d32.double() - d64).abs() <= bound).all()), name
        # dhead: softplus' and sigmoid' from the stored outputs, a few fp32 roundings of factors in [0, 1]
        s32, c32 = net["sigma"], net["rgb"]
        dsr32 = p["d_sigma"] * (1 - torch.exp(-s32))
        dsr64 = p["d_sigma"].double() * (1 - torch.exp(-s32.double()))
        assert bool(((dsr32.double() - dsr64).abs() <= 4e-7 * p["d_sigma"].double().abs()).all())
        drr32 = p["d_rgb"] * c32 * (1 - c32)
        drr64 = p["d_rgb"].double() * c32.double() * (1 - c32.double())
        assert bool(((drr32.double() - drr64).abs() <= 4e-7 * p["d_rgb"].double().abs()).all())
    # the inference bars on the default-initialised model: 5e-6 on sigma, 2e-6 on rgb (tests/test_render_gpu.py)
    q = cases.problem(R, S, default_init=True)
    x0 = cases.gather64(q)
    n64, n32 = cases.network(q, x0, biased=False), cases.network(q, x0.float(), biased=False, dtype=torch.float32)
    assert float((n32["sigma"].double() - n64["sigma"]).abs().max()) < 5e-6
    assert float((n32["rgb"].double() - n64["rgb"]).abs().max()) < 2e-6


@pytest.mark.parametrize("R,S", [(R, S) for R, S in SHAPES if R * S >= 127], ids=[i for i, (R, S) in zip(cases.IDS, SHAPES) if R * S >= 127])
def test_both_relu_branches_are_live_at_every_edge(R, S):
    p = cases.problem(R, S)
    rows = torch.tensor(cases.edge_samples(p["n"]))
    assert {0, p["n"] - 1} <= set(rows.tolist())
    x0 = cases.gather64(p, rows)
    for biased in (False, True):
        net = cases.network(p, x0, rows, biased=biased)
        for name in ("h1", "h2", "h3", "h4"):
            live = net[name] > 0
            assert bool(live.any(1).all()) and bool((~live).any(1).all()), (name, biased)
        for name in ("d1", "d2", "d3", "d4", "dx0"):
            assert bool(net[name].ne(0).any(1).all()), name
        assert float(net["sigma"].min()) > 0 and 0 < float(net["rgb"].min()) and float(net["rgb"].max()) < 1
