"""The conditions tests/test_ray_stages_gpu.py rests on, checked for the REFERENCES alone (no kernel, no GPU): the inputs of
tests/ray_stage_lib.py are well scaled, and the fp32 evaluation of every statement of render.py stays within its bar of the
float64 evaluation on them -- so a failure of the GPU test is the kernel's, not the statement's or the inputs'."""
import pytest
import torch

import ray_stage_lib as lib


@pytest.mark.parametrize("S", lib.COMPOSITE_S)
def test_composite_inputs_are_scaled_and_fp32_autograd_is_close(S):
    inp = lib.composite_inputs(S)
    assert inp["sigma"].shape == (48, S) and inp["edges"].shape == (48, S + 1)
    dd = (inp["edges"][:, 1:] - inp["edges"][:, :-1]).double() * inp["sigma"].double()
    for i, (name, k) in enumerate(lib.composite_classes(S)):
        rows = slice(i * lib.RAYS_PER_CLASS, (i + 1) * lib.RAYS_PER_CLASS)
        if name == "empty":
            assert float(inp["sigma"][rows].abs().max()) == 0
        elif name == "thin":
            assert float(inp["sigma"][rows].max()) < 4
        else:
            assert float(inp["sigma"][rows, k:].min()) >= 100 and (k == 0 or float(inp["sigma"][rows, :k].max()) < 1)
            if S >= 63:      # what the class is for: a total of delta sigma whose ulp is the size of a thin ray's whole sum
                assert float(dd[rows].sum(-1).min()) > 30
    cases = [c for c in lib.composite_cases() if c[0] == S]
    assert len(cases) == (5 if S == 129 else 3)
    for _, bg, use_rgb, use_acc in cases:
        scales = lib.composite_scales(inp, bg, use_rgb, use_acc)
        assert float(scales[0].min()) > lib.MIN_SCALE, (S, bg, use_rgb, use_acc, float(scales[0].min()))
        assert not use_rgb or float(scales[1].min()) > lib.MIN_SCALE
        want = lib.composite_gradients(inp, bg, torch.float64, use_rgb, use_acc)
        got = lib.composite_gradients(inp, bg, torch.float32, use_rgb, use_acc)
        es, ec = lib.composite_errors(got, want, scales)
        assert float(es.max()) <= lib.FLOOR and float(ec.max()) <= lib.FLOOR, (S, bg, lib.per_class(es, S), lib.per_class(ec, S))
        if not use_rgb:
            assert float(got[1].abs().max()) == 0 and float(want[1].abs().max()) == 0


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("S,num_fine", lib.PDF_SHAPES)
def test_pdf_statement_fp32_is_close_to_float64(S, num_fine, train):
    inp = lib.pdf_inputs(S, num_fine, train)
    nf = inp["near_far"]
    assert inp["edges"].shape == (lib.PDF_RAYS, S + 1) and bool((nf[:, 1] - nf[:, 0] >= 0.5).all())
    assert bool((inp["edges"][:, 1:] >= inp["edges"][:, :-1]).all())
    assert float(inp["weights"][::5].abs().max()) == 0 and float(inp["weights"].sum(-1).max()) <= 1 + 1e-6
    want = lib.pdf_statement(inp, num_fine, torch.float64)
    got = lib.pdf_statement(inp, num_fine, torch.float32)
    assert want.shape == (lib.PDF_RAYS, S + num_fine + 2)
    err = lib.pdf_error(got, want, inp)
    assert float(err.max()) <= 2e-5, float(err.max())


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("S", lib.COARSE_S)
def test_coarse_statement_fp32_is_close_to_float64(S, biased, train):
    rows = lib.coarse_rows()
    nv, hd = rows["num_visited"], rows["hit_distances"]
    assert sorted(set(nv.tolist())) == list(lib.COARSE_NV) and hd.shape == (54, lib.COARSE_M, 2)
    for r in range(len(nv)):
        n, z, m = int(nv[r]), int(rows["zero_slot"][r]), int(rows["neg_slot"][r])
        assert bool((hd[r, n:] == lib.FILL).all())
        if n >= 3:
            assert 0 < z < n - 1 and 0 < m < n - 1 and z != m
            assert float(hd[r, z, 1]) == float(hd[r, z, 0]) and float(hd[r, m, 1]) < float(hd[r, m, 0])
    t_rand = lib.coarse_draws(S) if train else None
    idx, want = lib.coarse_statement(rows, S, biased, t_rand, torch.float64)
    _, got = lib.coarse_statement(rows, S, biased, t_rand, torch.float32)
    assert len(idx) == 48 and want.shape == (48, S + 1)
    err = lib.coarse_error(got, want, rows, idx)
    assert float(err.max()) <= 4e-7, float(err.max())
