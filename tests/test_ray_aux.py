"""Expected depth and distortion loss, the statements alone (no GPU): render.composite_aux_statement against an independent
transcription of mip-NeRF 360 eq. 15, the linear-time form and the closed-form dL/dw the kernels of csrc/tn_ray_aux.hip evaluate
against the pairwise statement, and the usability of the inputs tests/test_ray_aux_gpu.py holds the kernels to (ray_aux_lib)."""
import importlib
import re
from pathlib import Path

import pytest
import torch

import ray_aux_lib as aux
import ray_stage_lib as lib

render = lib.render
ROOT = Path(__file__).resolve().parents[1]
SMALL = (1, 2, 5, 64, 65)


def _eq15_absolute_midpoints(w, e):
    """mip-NeRF 360 eq. 15, written out with loops over i and j on the ABSOLUTE midpoints: sum_ij w_i w_j |(s_i + s_{i+1}) / 2 -
    (s_j + s_{j+1}) / 2| + 1/3 sum_i w_i^2 (s_{i+1} - s_i)."""
    R, S = w.shape
    out = torch.zeros(R, dtype=w.dtype)
    mid = (e[:, :-1] + e[:, 1:]) / 2
    for i in range(S):
        for j in range(S):
            out += w[:, i] * w[:, j] * (mid[:, i] - mid[:, j]).abs()
        out += w[:, i] ** 2 * (e[:, i + 1] - e[:, i]) / 3
    return out


@pytest.mark.parametrize("S", SMALL)
def test_statement_equals_eq15_and_the_linear_time_form_in_float64(S):
    inp = lib.composite_inputs(S)
    sigma, e = inp["sigma"].double(), inp["edges"].double()
    moment, dist = render.composite_aux_statement(sigma, e)
    w = render.ray_weights(sigma, e)
    span = e[:, -1] - e[:, 0]
    assert float(((dist - _eq15_absolute_midpoints(w, e)).abs() / span).max()) <= 1e-14
    # 2 sum_i w_i (u'_i W_i - WU_i) + 1/3 sum w^2 delta, with exclusive prefix sums
    u = ((e[:, :-1] - e[:, :1]) + (e[:, 1:] - e[:, :1])) / 2
    W, WU = torch.cumsum(w, -1) - w, torch.cumsum(w * u, -1) - w * u
    linear = 2 * (w * (u * W - WU)).sum(-1) + (w * w * (e[:, 1:] - e[:, :-1])).sum(-1) / 3
    assert float(((dist - linear).abs() / span).max()) <= 1e-14
    # depth_moment = sum w (e_i + e_{i+1}) / 2
    assert float(((moment - (w * (e[:, :-1] + e[:, 1:]) / 2).sum(-1)).abs() / e[:, -1]).max()) <= 1e-14
    assert float(dist[:8].min()) > 0 and float(dist[-8:].abs().max()) == 0 and float(moment[-8:].abs().max()) == 0    # thin / empty rays


@pytest.mark.parametrize("S", SMALL)
def test_closed_form_dw_equals_float64_autograd_of_the_statement(S):
    inp = lib.composite_inputs(S)
    e = inp["edges"].double()
    w = render.ray_weights(inp["sigma"].double(), e).requires_grad_(True)
    # the statement as a function of the weights (its own expressions, ray_weights left out)
    e0 = e[:, :1]
    u = ((e[:, :-1] - e0) + (e[:, 1:] - e0)) / 2
    moment = e0[:, 0] * w.sum(-1) + (w * u).sum(-1)
    dist = (w[:, :, None] * w[:, None, :] * (u[:, :, None] - u[:, None, :]).abs()).sum((-2, -1)) + (w * w * (e[:, 1:] - e[:, :-1])).sum(-1) / 3
    g = torch.Generator().manual_seed(7)
    gm, gd = torch.randn(48, generator=g).double(), torch.randn(48, generator=g).double()
    (auto,) = torch.autograd.grad((moment * gm).sum() + (dist * gd).sum(), w)
    dm, dd = aux.dw_closed_form(w.detach(), e)
    want = gm[:, None] * dm + gd[:, None] * dd
    assert float((auto - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert torch.allclose(render.composite_aux_statement(inp["sigma"].double(), e)[1], dist.detach(), rtol=0, atol=1e-15)


def test_sizes_cover_both_sides_of_every_change_of_form():
    assert set(lib.COMPOSITE_S) <= set(aux.AUX_S)
    for edge in (64, 128, 320, 576):         # a second chunk; the groups of 2, 5, 9 chunks; the second trip of the largest
        assert edge in aux.AUX_S and edge + 1 in aux.AUX_S


@pytest.mark.parametrize("S", aux.AUX_S)
def test_inputs_are_usable_fp32_statement_within_floor_of_float64(S):
    """Neither condition involves a kernel: the fp32 statement (fp32 autograd) is within FLOOR = 2^-20 of float64 in all three
    measures, and every ray's scale exceeds MIN_SCALE.  Measured on the CPU for the sizes of the list: at most 2.5e-7 (depth
    moment), 1.7e-7 (distortion) and 4.2e-7 (d sigma, all four cotangents, black background) on the nine sizes of
    ray_stage_lib.COMPOSITE_S."""
    inp, cot = lib.composite_inputs(S), aux.cotangents(S)
    if S in lib.COMPOSITE_S:
        assert aux.cotangent_attempt(S) == 0        # the cotangents are randn, randn from manual_seed(S)
        g = torch.Generator().manual_seed(S)
        assert torch.equal(cot[0], torch.randn(48, generator=g)) and torch.equal(cot[1], torch.randn(48, generator=g))
    ev = aux.value_errors(aux.statement(inp, torch.float32), aux.reference_values(S), inp)
    sc = aux.scales(inp, cot, aux.BACKGROUND, "all")
    es, ec = aux.gradient_errors(aux.gradients(inp, cot, aux.BACKGROUND, torch.float32, "all"), aux.reference_gradients(S, aux.BACKGROUND, "all"), sc)
    print(f"ray-aux inputs S={S}: depth moment {float(ev[0].max()):.3e} distortion {float(ev[1].max()):.3e} d sigma {float(es.max()):.3e} "
          f"d rgb {float(ec.max()):.3e}; least scale {float(sc[0].min()):.3e}")
    assert float(sc[0].min()) > aux.MIN_SCALE
    assert float(ev[0].max()) <= aux.FLOOR and float(ev[1].max()) <= aux.FLOOR and float(es.max()) <= aux.FLOOR


def test_absolute_midpoints_lose_digits_the_relative_ones_keep():
    """Why the definition uses u': at S = 2 the fp32 pairwise term on absolute midpoints (edges near 1, span 0.02) is above the
    floor, on the midpoints relative to the first edge it is not."""
    inp = lib.composite_inputs(2)
    e32, w32 = inp["edges"], render.ray_weights(inp["sigma"], inp["edges"])
    want = aux.reference_values(2)
    got_abs = _eq15_absolute_midpoints(w32, e32)
    got_rel = render.composite_aux_statement(inp["sigma"], e32)[1]
    span = (inp["edges"][:, -1] - inp["edges"][:, 0]).double()
    assert float(((got_rel.double() - want[1]).abs() / span).max()) <= aux.FLOOR < float(((got_abs.double() - want[1]).abs() / span).max())


def test_header_declares_both_entries_and_the_abi_stays_6():
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define TN_ABI_VERSION 6\b", header)
    assert re.search(r"\bint tn_composite_aux\(size_t num_rays, uint32_t num_samples, const float \*sigma, const float \*edges,", header)
    assert re.search(r"\bint tn_composite_backward_aux\(size_t num_rays, uint32_t num_samples,", header)
    assert 'DepthRenderer(method="expected")' in header and "lossfun_distortion" in header
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    assert _lib.ABI_VERSION == 6 and {"tn_composite_aux", "tn_composite_backward_aux"} <= set(_lib.SYMBOLS)


@pytest.mark.parametrize("method", ["render_train", "render"])
def test_aux_outputs_refuse_the_occupancy_sampler_before_any_launch(method):
    """The composite's edges are live-length coordinates under the occupancy-guided sampler: refused, in front of the first launch
    (a renderer without a tracer, tensors on the CPU)."""
    rd = object.__new__(render.TetraRenderer)
    o = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="live-length"):
        getattr(rd, method)(o, o, occupancy=torch.zeros(3), occupancy_threshold=0.1, occupancy_sampler=True, aux_outputs=True)


def test_aux_outputs_of_divides_and_masks_a_zero_span():
    moment, dist = torch.tensor([2.0, 0.0, 3.0]), torch.tensor([0.5, 0.0, 7.0])
    acc = torch.tensor([[0.5], [0.0], [1.0]])
    edges = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, 4.0, 4.0]])
    exp, d = render.aux_outputs_of(moment, dist, acc, edges)
    assert exp.shape == d.shape == (3, 1)
    assert torch.allclose(exp[:, 0], torch.tensor([4.0, 0.0, 3.0])) and torch.equal(d[:, 0], torch.tensor([0.25, 0.0, 0.0]))
