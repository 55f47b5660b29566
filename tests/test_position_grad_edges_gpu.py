"""k_sample_positions_bwd (csrc/tn_position_grad.hip), part (B) of the position gradients, at every edge of its launch and on every
branch of its liveness rule, against float64.  Inputs, references and bounds come from tests/position_grad_cases.py (checked on the
CPU, together with the torch statement, by tests/test_position_grad_cases.py).  What is asserted:
  exact fill   (integer vertices, power-of-two tetrahedra: every partial sum is exact in fp32 in ANY order, so the correct result has
               one bit pattern) points, origins, directions and vertices -- summed with atomics and by the deterministic path --
               EQUAL the float64 reference, no tolerance; torch.equal compares values, so +0 = -0 and a NaN equals nothing;
  random fill  the a-priori bounds of position_grad_cases.py, no exclusions;
  zeros        a dead sample has points == 0, an all-dead ray origins == directions == 0, a vertex no live sample names == 0 --
               with NaN barycentrics, NaN t and NaN g on id-dead samples;
  sizes        S on either side of one, two and four 64-sample chunks, R on either side of the 4-ray block and of the 32,768 rays in
               flight, 65,537 rays (a third ray for wave 0), 19,939 samples in one tetrahedron.
Every call runs with cpp._POISON on: an element of points, origins or directions the kernel fails to write is a NaN.
`RATIO` lines (pytest -s) are what profiles/position_grad_edges_gpu.txt records."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import position_grad_cases as pgc

pytestmark = pytest.mark.gpu

EXACT_CASES = [("mixed", R, S) for R, S in pgc.EDGE_SHAPES] + [("rays", 8, S) for S in pgc.CLASS_RAY_S] + [("one_tet",) + pgc.ONE_TET_SHAPE]
RANDOM_CASES = [("mixed", R, S) for R, S in pgc.RANDOM_SHAPES] + [("rays", 8, S) for S in pgc.CLASS_RAY_S]
OUTPUTS = ("points", "origins", "directions", "vertices")


@pytest.fixture(autouse=True)
def poison(tn, monkeypatch):
    monkeypatch.setattr(tn.cpp, "_POISON", True)


def _case(fill, kind, R, S):
    if kind == "one_tet":
        return pgc.one_tet_case()
    return pgc.class_ray_case(fill, S) if kind == "rays" else pgc.mixed_case(fill, R, S)


def _dev(c, device, *keys):
    return [torch.from_numpy(np.array(c[k])).to(device) for k in keys]          # (a copy: the shared cases are read-only arrays)


def _run(tn, c, device, deterministic=False, distances=True, **want):
    vi, bc, gb, verts, t = _dev(c, device, "vi", "bc", "gb", "verts", "t")
    before = tn.cpp.DETERMINISTIC_FIELD_GRADIENT
    tn.cpp.DETERMINISTIC_FIELD_GRADIENT = deterministic
    try:
        out = tn.cpp.sample_positions_backward(vi, bc, gb, verts, t if distances else None, **want)
    finally:
        tn.cpp.DETERMINISTIC_FIELD_GRADIENT = before
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, out))


ALL = dict(want_points=True, want_origins=True, want_directions=True, want_vertices=True)


def _check_zeros(c, out, what):
    ref = c["ref"]
    live = ref["live"]
    for k in OUTPUTS:
        assert bool(torch.isfinite(out[k]).all()), (what, k)
    assert bool((out["points"].cpu()[~live] == 0).all()), what
    dead_rays = ~live.any(1)
    assert bool((out["origins"].cpu()[dead_rays] == 0).all()) and bool((out["directions"].cpu()[dead_rays] == 0).all()), what
    assert bool((out["vertices"].cpu()[~ref["named"]] == 0).all()), what


@pytest.mark.parametrize("kind,R,S", EXACT_CASES)
def test_exact_fill_equals_float64(tn, device, kind, R, S):
    c = _case("exact", kind, R, S)
    ref = c["ref"]
    out = _run(tn, c, device, **ALL)
    for k in OUTPUTS:
        got, want = out[k].cpu(), ref[k].to(torch.float32)
        assert got.shape == want.shape and got.dtype == torch.float32
        bad = (got != want) | torch.isnan(got)
        assert not bool(bad.any()), (k, int(bad.sum()), "first at", torch.nonzero(bad)[0].tolist())
        assert torch.equal(got, want), k
    _check_zeros(c, out, "atomic")
    det = [_run(tn, c, device, deterministic=True, want_vertices=True)["vertices"] for _ in range(2)]
    assert torch.equal(det[0].cpu(), ref["vertices"].to(torch.float32)), "deterministic vertices"
    assert torch.equal(det[0].view(torch.int32), det[1].view(torch.int32))
    assert bool((det[0].cpu()[~ref["named"]] == 0).all())


@pytest.mark.parametrize("kind,R,S", RANDOM_CASES)
def test_random_fill_within_the_a_priori_bounds(tn, device, kind, R, S):
    c = _case("random", kind, R, S)
    ref = c["ref"]
    out = _run(tn, c, device, **ALL)
    _check_zeros(c, out, "atomic")
    det = [_run(tn, c, device, deterministic=True, want_vertices=True)["vertices"] for _ in range(2)]
    assert torch.equal(det[0].view(torch.int32), det[1].view(torch.int32))
    assert bool(torch.isfinite(det[0]).all()) and bool((det[0].cpu()[~ref["named"]] == 0).all())
    err = (out["points"].cpu().double() - ref["points"]).norm(dim=-1)
    worst = {"points": float((err / ref["bound_points"].clamp_min(1e-300)).max())}
    fails = [] if bool((err <= ref["bound_points"]).all()) else ["points"]
    for name, got, k, b in (("origins", out["origins"], "origins", "bound_o"), ("directions", out["directions"], "directions", "bound_d"),
                            ("vertices", out["vertices"], "vertices", "bound_v"), ("vertices_det", det[0], "vertices", "bound_v")):
        e = (got.cpu().double() - ref[k]).abs()
        worst[name] = float((e / ref[b].clamp_min(1e-300)).max())
        if not bool((e <= ref[b]).all()):
            fails.append(name)
        assert bool((got.cpu()[ref[b] == 0] == 0).all()), name            # nothing lands where no live sample points
    print(f"RATIO random {kind} R={c['R']} S={S}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, (fails, worst)


@pytest.mark.parametrize("kind,R,S", [("mixed", 9, 129), ("rays", 8, 65)])
def test_output_selection_gives_the_same_bits(tn, device, kind, R, S):
    c = _case("exact", kind, R, S)
    full = _run(tn, c, device, **ALL)
    for k in OUTPUTS:
        one = _run(tn, c, device, **{"want_" + k: True})
        assert all(one[j] is None for j in OUTPUTS if j != k), k
        assert torch.equal(one[k].view(torch.int32), full[k].view(torch.int32)), k
    one = _run(tn, c, device, distances=False, want_origins=True)
    assert torch.equal(one["origins"].view(torch.int32), full["origins"].view(torch.int32)) and one["directions"] is None
    with pytest.raises(RuntimeError, match="want_directions needs the sample distances"):
        _run(tn, c, device, distances=False, want_directions=True)


SUBSETS = [s for k in range(4) for s in itertools.combinations(("vertices", "origins", "directions"), k)]


@pytest.mark.parametrize("S", (1, 65, 129))
def test_through_the_autograd_node(tn, device, S):
    """sample_positions_grad with each subset of {vertices, origins, directions} requiring grad: the op's gradients, None where none
    is required, the barycentric gradient passed through unchanged (NaN and inf payloads included: compared as bit patterns)"""
    c = pgc.mixed_case("exact", 9, S)
    full = _run(tn, c, device, **ALL)
    vi, bc, gb, verts, t = _dev(c, device, "vi", "bc", "gb", "verts", "t")
    for subset in SUBSETS:
        b = bc.clone().requires_grad_(True)
        leaf = dict(vertices=verts.clone().requires_grad_("vertices" in subset),
                    origins=torch.zeros(c["R"], 3, device=device, requires_grad="origins" in subset),
                    directions=torch.ones(c["R"], 3, device=device, requires_grad="directions" in subset))
        out = tn.sample_positions_grad(b, vi, leaf["vertices"], leaf["origins"], leaf["directions"], t)
        assert torch.equal(out.detach().view(torch.int32), bc.view(torch.int32))
        out.backward(gb)
        assert torch.equal(b.grad.view(torch.int32), gb.view(torch.int32)), subset
        for k in ("vertices", "origins", "directions"):
            if k in subset:
                assert torch.equal(leaf[k].grad.view(torch.int32), full[k].view(torch.int32)), (subset, k)
            else:
                assert leaf[k].grad is None, (subset, k)


@pytest.mark.parametrize("S", pgc.CHAIN_S)
def test_chain_against_autograd_of_the_forward_statement(tn, device, S):
    """(A) then (B) through the public ops: the gradient of sum G . interpolate_values(vi, sample_positions_grad(bc, ...), field)
    w.r.t. origins, directions and vertices, against float64 autograd of b = barycentrics_of(o + t d, verts[vi]) followed by the
    gather statement on the live samples.  This pins the convention, not only the closed form.  The tolerance is derived in
    position_grad_cases.chain_reference: the (A) bound propagated through the solve, plus the (B) bounds, plus the rounding of the
    weights; the fp32 torch statement measures <= 0.03 of it on the CPU (tests/test_position_grad_cases.py), and the tolerance is a
    median 5e-5 .. 5e-4 of the gradient it bounds."""
    c = pgc.chain_case(S)
    ref = c["ref"]
    vi, bc, verts, t, o, d, field, G = _dev(c, device, "vi", "bc", "verts", "t", "o", "d", "field", "G")
    for x in (verts, o, d):
        x.requires_grad_(True)
    b = bc.clone().requires_grad_(True)
    feats = tn.interpolate_values(vi, tn.sample_positions_grad(b, vi, verts, o, d, t), field)
    assert feats.shape == G.shape
    (feats * G).sum().backward()
    assert b.grad is not None and bool(torch.isfinite(b.grad).all())
    for k, got, bound in (("origins", o.grad, "bound_o"), ("directions", d.grad, "bound_d"), ("vertices", verts.grad, "bound_v")):
        err = (got.cpu().double() - ref[k]).abs()
        print(f"RATIO chain S={S} {k}: worst error / tolerance {float((err / ref[bound].clamp_min(1e-300)).max()):.3f}, "
              f"max |gradient| {float(ref[k].abs().max()):.3g}")
        assert bool(torch.isfinite(got).all()), k
        assert bool((err <= ref[bound]).all()), (k, int((err > ref[bound]).sum()))
        assert bool((got.cpu()[ref[bound] == 0] == 0).all()), k


def test_refusals_touch_nothing(tn, device):
    """the C entry refuses R S >= 2^32 before any launch; the wrapper refuses wrong shapes and types before it allocates"""
    clib = importlib.import_module("tetra-nerf_amd._lib")
    lib = clib.load()
    vi = torch.arange(4, dtype=torch.int32, device=device).repeat(4, 1)
    bc = torch.full((4, 3), 0.25, device=device)
    gb = torch.ones(4, 3, device=device)
    t = torch.ones(4, device=device)
    verts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]], device=device)
    outs = [torch.full(shape, float("nan"), device=device) for shape in ((4, 3), (4, 3), (4, 3), (4, 3))]
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = lib.tn_sample_positions_backward(2 ** 32, 1, 4, vi.data_ptr(), bc.data_ptr(), gb.data_ptr(), t.data_ptr(), verts.data_ptr(),
                                          *[x.data_ptr() for x in outs], stream)
    msg = lib.tn_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "too many samples" in msg, (rc, msg)
    assert all(bool(torch.isnan(x).all()) for x in outs)
    rc = lib.tn_sample_positions_backward(4, 1, 4, vi.data_ptr(), bc.data_ptr(), gb.data_ptr(), None, verts.data_ptr(),
                                          None, None, outs[2].data_ptr(), None, stream)
    torch.cuda.synchronize()
    assert rc != 0 and "needs the sample distances" in lib.tn_last_error().decode() and bool(torch.isnan(outs[2]).all())
    # the same four samples are accepted as 4 rays of 1 sample: m = g = (1, 1, 1) in the unit tetrahedron
    assert lib.tn_sample_positions_backward(4, 1, 4, vi.data_ptr(), bc.data_ptr(), gb.data_ptr(), t.data_ptr(), verts.data_ptr(),
                                            *[x.data_ptr() for x in outs[:3]], None, stream) == 0
    torch.cuda.synchronize()
    assert all(bool((x == 1).all()) for x in outs[:3])
    # the wrapper
    cpp = tn.cpp
    v3, b3, g3, t2 = vi.view(2, 2, 4), bc.view(2, 2, 3), gb.view(2, 2, 3), t.view(2, 2)
    for args, text in (((vi, b3, g3, verts, t2), r"vertex_indices must be i32 \[R,S,4\]"),
                       ((v3.long(), b3, g3, verts, t2), r"vertex_indices must be i32 \[R,S,4\]"),
                       ((v3, bc, g3, verts, t2), r"barycentric_coordinates must be f32 \[R,S,3\]"),
                       ((v3, b3, g3.double(), verts, t2), r"grad_bary must be f32 \[R,S,3\]"),
                       ((v3, b3, g3, verts[:, :2].contiguous(), t2), r"vertices must be f32 \[V,3\]"),
                       ((v3, b3, g3, verts, t), r"distances must be f32 \[R,S\]"),
                       ((v3, b3, g3, verts.cpu(), t2), "vertices must be a CUDA tensor"),
                       ((v3, b3, g3.transpose(0, 1), verts, t2), "grad_bary must be contiguous")):
        with pytest.raises(RuntimeError, match=text):
            cpp.sample_positions_backward(*args, want_origins=True, want_vertices=True)
