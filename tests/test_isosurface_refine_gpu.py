"""The isosurface refinement on the GPU (tn_isosurface_refine_begin / _points / _select / _vertices,
csrc/tn_isosurface_refine.hip; cpp.isosurface_refine, cpp.isosurface_refine_with, TetrahedraTracer.isosurface(refine=...),
render.extract_mesh(refine_rounds=...), nerfstudio_plugin.extract_mesh(refine_rounds=...)).

Bar: on the crafted densities of tests/isosurface_refine_cases.py, at every wave, block and grid-cap edge of N, the gather inputs of
every round, the brackets and flags after every round, edge_t and positions equal the numpy statement
(geometry.isosurface_refine_statement) byte for byte, inside patterned buffers whose other words stay, twice the same.  With the
real network: the topology arrays are the extraction's own, no round is the extraction, the brackets nest, and the float64
network evaluated at both ends of every final bracket lies on the side the kernel says within 5e-6 -- the bar the suite holds the
density of the fused forward to against float64 in fp32 and bf16x3 (tests/test_render_gpu.py::test_mlp_forward_vs_float64,
tests/test_mlp_edges_gpu.py::test_inference_forwards)."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import isosurface_cases as ic
import isosurface_refine_cases as rc
from test_gather_edges_gpu import PAD, Guarded

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
C = rc.C
SIGMA_BAR = 5e-6        # tests/test_render_gpu.py::test_mlp_forward_vs_float64: |sigma - float64| in fp32 and in bf16x3


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _same(t, want):
    got = t.detach().cpu().contiguous().numpy()
    return got.shape == want.shape and np.array_equal(ic.bits(got), ic.bits(np.ascontiguousarray(want)))


def sizes():
    """N below, at and above a wave and a block, and the first N whose 7 N candidates are more than the capped grid has lanes (the
    grid-stride loop of the points kernel comes round)"""
    bt, blocks = ic.kernel_constants()
    over = -(-(bt * blocks + 1) // C)
    assert (bt, blocks) == (256, 1024) and over == 37450 and C * (over - 1) <= bt * blocks < C * over
    return [0, 1, 63, 64, 65, bt - 1, bt, bt + 1, over]


_WANT = {}


def _want(N):
    """the crafted case of N edges and the numpy statement's answer on it after every number of rounds, made once"""
    if N not in _WANT:
        xyz, ev, values, level, dens = rc.crafted(N)
        g = ic.geometry()
        outs = [g.isosurface_refine_statement(xyz, ev, values, level, rc.replay(dens), r) for r in range(rc.ROUNDS + 1)]
        _WANT[N] = (xyz, ev, values, level, dens, outs)
    return _WANT[N]


class Bytes:
    """n bytes inside a Guarded buffer; the bytes behind them in its last word count as margin"""

    def __init__(self, n, device):
        self.n, self.g = n, Guarded((n + 3) // 4, device)
        self.view = self.g.inner.view(torch.uint8)[:n]

    def intact(self):
        tail = self.g.inner.view(torch.uint8)[self.n:]
        return self.g.margins_intact() and torch.equal(tail, self.g.pattern[PAD:PAD + self.g.words].view(torch.uint8)[self.n:])


def _drive(tn, device, N, rounds):
    """the four entries through ctypes on guarded buffers, the densities of round r = the crafted ones; returns what each step
    left (clones) and the guards"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    xyz, ev, values, level, dens, _ = _want(N)
    V = len(values)
    x, e, v, d = _dev(xyz, device), _dev(ev, device), _dev(values, device), _dev(dens, device)
    br, vi, bc, et, pos = (Guarded(k * N, device) for k in (4, 4 * C, 3 * C, 1, 3))
    fl = Bytes(N, device)
    p = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    s = tn.cpp._stream(device)
    seen = {"vi": [], "bc": [], "brackets": [], "flags": []}
    keep = lambda: (seen["brackets"].append(br.inner.clone().view(torch.float32).view(N, 4)), seen["flags"].append(fl.view.clone()))   # noqa: E731
    assert lib.tn_isosurface_refine_begin(V, N, p(e), p(v), level, p(br.inner), p(fl.view), s) == 0
    keep()
    for r in range(rounds):
        assert lib.tn_isosurface_refine_points(V, N, r, p(e), p(br.inner), p(fl.view), p(vi.inner), p(bc.inner), s) == 0
        seen["vi"].append(vi.inner.clone().view(N * C, 4))
        seen["bc"].append(bc.inner.clone().view(torch.float32).view(N * C, 3))
        assert lib.tn_isosurface_refine_select(N, r, level, p(d[r]), p(br.inner), p(fl.view), s) == 0
        keep()
    assert lib.tn_isosurface_refine_vertices(V, N, p(x), p(e), p(br.inner), level, p(et.inner), p(pos.inner), s) == 0
    torch.cuda.synchronize()
    seen["edge_t"], seen["positions"] = et.inner.clone().view(torch.float32), pos.inner.clone().view(torch.float32).view(N, 3)
    assert all(g.margins_intact() for g in (br, vi, bc, et, pos)) and fl.intact(), N
    return seen


@pytest.mark.parametrize("N", sizes())
def test_kernels_equal_the_statement_on_crafted_densities(tn, device, N):
    xyz, ev, values, level, dens, outs = _want(N)
    R = rc.ROUNDS
    seen = _drive(tn, device, N, R)
    want = outs[R]
    for r in range(R + 1):
        assert _same(seen["brackets"][r], want["brackets"][r]), f"N {N}: brackets after {r} rounds"
        assert np.array_equal(seen["flags"][r].cpu().numpy(), outs[r]["edge_frozen"]), f"N {N}: flags after {r} rounds"
    a, b = (np.where(want["edge_frozen"] == 2, 0, ev[:, k]).repeat(C) for k in (0, 1))
    g = ic.geometry()
    for r in range(R):
        t = g.isosurface_refine_candidates(want["brackets"][r][:, 0], want["brackets"][r][:, 1]).reshape(-1)
        assert np.array_equal(seen["vi"][r].cpu().numpy(), np.stack([a, b, a, a], 1).astype(np.int32).reshape(-1, 4)), f"N {N}: vertex_indices {r}"
        assert _same(seen["bc"][r], np.stack([t, np.zeros_like(t), np.zeros_like(t)], 1).reshape(-1, 3)), f"N {N}: barycentric {r}"
    assert _same(seen["edge_t"], want["edge_t"]) and _same(seen["positions"], want["positions"]), N
    again = _drive(tn, device, N, R)
    for key in ("edge_t", "positions"):
        assert torch.equal(seen[key].view(torch.int32), again[key].view(torch.int32)), (N, key)
    assert all(torch.equal(u.view(torch.int32), w.view(torch.int32)) for u, w in zip(seen["brackets"] + seen["bc"], again["brackets"] + again["bc"]))
    print("N", N, "frozen", int((want["edge_frozen"] == 1).sum()), "bad ids", int((want["edge_frozen"] == 2).sum()))


@pytest.mark.parametrize("N", [0, 1, 257, 37450])
def test_callback_form_equals_the_statement(tn, device, N):
    """cpp.isosurface_refine_with: the callback sees the gather's inputs of every round and answers with the crafted densities"""
    xyz, ev, values, level, dens, outs = _want(N)
    d = _dev(dens, device)
    surface = {"edge_vertices": _dev(ev, device), "triangles": torch.zeros(1, 3, dtype=torch.int32, device=device), "num_refs": 5}
    for rounds in (0, 1, rc.ROUNDS):
        asked = []

        def fn(vi, bc):
            assert vi.dtype == torch.int32 and tuple(vi.shape) == (N * C, 4) and bc.dtype == torch.float32 and tuple(bc.shape) == (N * C, 3)
            asked.append(bc[:, 0].clone())
            return d[len(asked) - 1].reshape(-1)

        got = tn.cpp.isosurface_refine_with(surface, _dev(xyz, device), _dev(values, device), level, fn, rounds)
        want = outs[rounds]
        assert len(asked) == (rounds if N else 0)
        assert got["edge_vertices"] is surface["edge_vertices"] and got["triangles"] is surface["triangles"] and got["num_refs"] == 5
        assert got["edge_frozen"].dtype == torch.uint8 and np.array_equal(got["edge_frozen"].cpu().numpy(), want["edge_frozen"])
        for key, name in (("edge_bracket", "edge_bracket"), ("edge_t", "edge_t"), ("positions", "positions")):
            assert got[key].dtype == torch.float32 and _same(got[key], want[name]), (N, rounds, key)
    with pytest.raises(RuntimeError, match="rounds"):
        tn.cpp.isosurface_refine_with(surface, _dev(xyz, device), _dev(values, device), level, None, 9)
    if N:
        with pytest.raises(RuntimeError, match="density_fn"):
            tn.cpp.isosurface_refine_with(surface, _dev(xyz, device), _dev(values, device), level, lambda vi, bc: bc[:, 0], 1)
        with pytest.raises(RuntimeError, match="level"):
            tn.cpp.isosurface_refine_with(surface, _dev(xyz, device), _dev(values, device), float("nan"), lambda vi, bc: d[0].reshape(-1), 1)


def test_refused_calls_touch_nothing(tn, device):
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    N = 300
    xyz, ev, values, level, dens, _ = _want(N)
    V = len(values)
    x, e, v, d = _dev(xyz, device), _dev(ev, device), _dev(values, device), _dev(dens, device)
    br, vi, bc, et, pos = (Guarded(k * N, device) for k in (4, 4 * C, 3 * C, 1, 3))
    fl = Guarded((N + 3) // 4, device)
    p = lambda t: t.data_ptr()   # noqa: E731
    B, F = p(br.inner), p(fl.inner)
    refused = [
        lib.tn_isosurface_refine_begin(V, N, p(e), p(v), float("nan"), B, F, None),
        lib.tn_isosurface_refine_begin(V, N, p(e), None, level, B, F, None),
        lib.tn_isosurface_refine_begin(V, N, p(e) + 4, p(v), level, B, F, None),
        lib.tn_isosurface_refine_begin(V, N, p(e), p(v), level, B + 4, F, None),
        lib.tn_isosurface_refine_begin(V, N, p(e), p(v), level, B, None, None),
        lib.tn_isosurface_refine_points(V, N, 8, p(e), B, F, p(vi.inner), p(bc.inner), None),
        lib.tn_isosurface_refine_points(0, N, 0, p(e), B, F, p(vi.inner), p(bc.inner), None),
        lib.tn_isosurface_refine_points(V, N, 0, p(e), B, F, p(vi.inner) + 8, p(bc.inner), None),
        lib.tn_isosurface_refine_points(V, N, 0, p(e), B, F, p(vi.inner), None, None),
        lib.tn_isosurface_refine_select(N, 8, level, p(d[0]), B, F, None),
        lib.tn_isosurface_refine_select(N, 0, float("inf"), p(d[0]), B, F, None),
        lib.tn_isosurface_refine_select(N, 0, level, None, B, F, None),
        lib.tn_isosurface_refine_vertices(V, N, p(x), p(e), B, 2.0 ** 126, p(et.inner), p(pos.inner), None),
        lib.tn_isosurface_refine_vertices(V, N, None, p(e), B, level, p(et.inner), p(pos.inner), None),
        lib.tn_isosurface_refine_vertices(V, N, p(x), p(e), B, level, p(et.inner), None, None),
        lib.tn_isosurface_refine_vertices(2 ** 32 - 1, N, p(x), p(e), B, level, p(et.inner), p(pos.inner), None),
    ]
    torch.cuda.synchronize()
    assert all(rc_ != 0 for rc_ in refused), refused
    for g in (br, vi, bc, et, pos, fl):
        assert g.margins_intact() and bool(g.untouched().all())
    # N = 0 is a valid call of every entry and launches nothing
    assert lib.tn_isosurface_refine_begin(V, 0, None, p(v), level, None, None, None) == 0
    assert lib.tn_isosurface_refine_points(V, 0, 0, None, None, None, None, None, None) == 0
    assert lib.tn_isosurface_refine_select(0, 0, level, None, None, None, None) == 0
    assert lib.tn_isosurface_refine_vertices(V, 0, p(x), None, None, level, None, None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- the network
_NET = {}


def _network(tn, scenes, device, mode):
    """sphere_300's mesh, a random [64, V] field and random weights (as tests/test_isosurface_gpu.py draws them), the kernel's own
    vertex densities in `mode`, the level = their median, the extraction, and its refinement after 0 .. 4 rounds"""
    if mode not in _NET:
        render = importlib.import_module("tetra-nerf_amd.render")
        xyz, cells = ic.sphere_mesh(scenes, *ic.SPHERES["sphere_300"])
        torch.manual_seed(3)
        mlp = render.TetraMLP().to(device)
        field = (torch.randn(64, len(xyz), device=device) * 0.5).contiguous()
        w = [t.detach() for t in render.mlp_weights(mlp)]
        x, c = _dev(xyz, device), _dev(cells, device)
        values = tn.cpp.mlp_forward(field, None, w, 1, mode=mode)
        level = float(values.median())
        surface = tn.cpp.isosurface(x, c, values, level)
        refined = [tn.cpp.isosurface_refine(surface, x, values, level, field, w, r, mode=mode) for r in range(5)]
        _NET[mode] = dict(xyz=x, cells=c, mlp=mlp, field=field, w=w, values=values, level=level, surface=surface, refined=refined)
    return _NET[mode]


def _sigma64(net, ev, t):
    """the float64 network's density at xyz-parameter t of the edges ev: features (1 - t) f_a + t f_b of the float32 field"""
    render = importlib.import_module("tetra-nerf_amd.render")
    m64 = render.TetraMLP().double().to(net["field"].device)
    m64.load_state_dict({k: v.double() for k, v in net["mlp"].state_dict().items()})
    rows = net["field"].t().double()
    t = t.double()[:, None]
    with torch.no_grad():
        return render.coarse_sigma(m64, (1.0 - t) * rows[ev[:, 0].long()] + t * rows[ev[:, 1].long()])


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_refinement_on_the_network(tn, scenes, device, mode):
    net = _network(tn, scenes, device, mode)
    surface, refined, level = net["surface"], net["refined"], net["level"]
    N = len(surface["positions"])
    assert N > 200
    again = tn.cpp.isosurface(net["xyz"], net["cells"], net["values"], level)
    for r, out in enumerate(refined):
        for key in ("triangles", "triangle_tets", "edge_vertices", "tri_offsets", "ref_offsets"):
            assert out[key] is surface[key] and torch.equal(out[key], again[key]), (r, key)
        assert out["num_triangles"] == surface["num_triangles"] and out["num_refs"] == surface["num_refs"]
        assert tuple(out["edge_bracket"].shape) == (N, 4) and tuple(out["edge_frozen"].shape) == (N,) and out["edge_frozen"].dtype == torch.uint8
        assert tuple(out["positions"].shape) == (N, 3) and tuple(out["edge_t"].shape) == (N,)
    # no round: the extraction's bytes, in new arrays
    for key in ("positions", "edge_t"):
        assert refined[0][key] is not surface[key] and torch.equal(refined[0][key].view(torch.int32), surface[key].view(torch.int32)), key
    ev = surface["edge_vertices"]
    begin = torch.stack([torch.zeros(N, device=device), torch.ones(N, device=device), net["values"][ev[:, 0].long()], net["values"][ev[:, 1].long()]], 1)
    assert torch.equal(refined[0]["edge_bracket"].view(torch.int32), begin.view(torch.int32)) and not bool(refined[0]["edge_frozen"].any())
    # the brackets nest, an eighth at a time
    for r in range(1, 5):
        lo0, hi0 = refined[r - 1]["edge_bracket"][:, 0], refined[r - 1]["edge_bracket"][:, 1]
        lo1, hi1 = refined[r]["edge_bracket"][:, 0], refined[r]["edge_bracket"][:, 1]
        assert not bool(refined[r]["edge_frozen"].any())
        assert bool((lo1 >= lo0).all()) and bool((hi1 <= hi0).all()) and bool(((hi1 - lo1) == 8.0 ** -r).all()), r
        t = refined[r]["edge_t"]
        assert bool(((t >= lo1) & (t <= hi1)).all())
    # the float64 network at both ends of every final bracket lies on the side the kernel says, within the forward's own bar
    for r in (1, 2, 4):
        br = refined[r]["edge_bracket"]
        worst = 0.0
        for t, s in ((br[:, 0], br[:, 2]), (br[:, 1], br[:, 3])):
            s64 = _sigma64(net, ev, t)
            inside = s >= level
            ok = torch.where(inside, s64 >= level - SIGMA_BAR, s64 < level + SIGMA_BAR)
            worst = max(worst, float((s64 - s.double()).abs().max()))
            assert bool(ok.all()), (mode, r, int((~ok).sum()))
        assert bool(((br[:, 2] >= level) != (br[:, 3] >= level)).all())
        res = (_sigma64(net, ev, refined[r]["edge_t"]) - level).abs()
        print(f"{mode} rounds {r}: vertices {N} max |kernel - float64| at the bracket ends {worst:.3e} (bar {SIGMA_BAR}); "
              f"residual |sigma64(vertex) - level| max {float(res.max()):.3e} mean {float(res.mean()):.3e}")
    res0 = (_sigma64(net, ev, surface["edge_t"]) - level).abs()
    print(f"{mode} rounds 0: residual max {float(res0.max()):.3e} mean {float(res0.mean()):.3e}")
    assert float(res.max()) < float(res0.max())


def test_extract_mesh_refines_before_the_colour_pass(tn, scenes, device):
    render = importlib.import_module("tetra-nerf_amd.render")
    net = _network(tn, scenes, device, "fp32")
    x, c, field, mlp, level = net["xyz"], net["cells"], net["field"], net["mlp"], net["level"]
    plain = render.extract_mesh(x, c, field, mlp, level)
    zero = render.extract_mesh(x, c, field, mlp, level, refine_rounds=0)
    assert set(zero) == set(plain) and "edge_bracket" not in plain
    for key in plain:
        if key in ("directions", "colors"):
            # the vertex normals are an index_add_, whose sums have no fixed order: two calls of the unchanged code differ in the
            # last bits of the unit normals (at most ten-odd terms of size <= 1: 1e-6) and, through the head, within the project's
            # 1e-5 fp32 bar in the colours
            assert float((zero[key] - plain[key]).abs().max()) <= (1e-6 if key == "directions" else 1e-5), key
        elif isinstance(plain[key], torch.Tensor):
            assert torch.equal(zero[key].view(torch.int32), plain[key].view(torch.int32)), key
        else:
            assert zero[key] == plain[key], key
    for key in ("positions", "edge_t", "triangles"):
        assert torch.equal(plain[key].view(torch.int32), net["surface"][key].view(torch.int32)), key
    out = render.extract_mesh(x, c, field, mlp, level, refine_rounds=2)
    want = net["refined"][2]
    for key in ("positions", "edge_t", "edge_bracket", "edge_frozen", "triangles", "edge_vertices"):
        assert torch.equal(out[key].view(torch.uint8), want[key].view(torch.uint8)), key
    assert not torch.equal(out["positions"], plain["positions"])
    # directions from the refined normals, colours gathered at the refined edge_t: a separate call on the returned arrays
    dirs = out["directions"]
    again = -render.vertex_normals(out["positions"], out["triangles"])      # (an index_add_: the order of its sums is not fixed)
    assert float((dirs - again).abs().max()) <= 1e-5 and float((dirs - plain["directions"]).abs().max()) > 1e-4
    ev, t = out["edge_vertices"], out["edge_t"]
    vi = torch.stack([ev[:, 0], ev[:, 1], ev[:, 0], ev[:, 0]], 1).contiguous()
    bc = torch.stack([t, torch.zeros_like(t), torch.zeros_like(t)], 1).contiguous()
    rgb = tn.cpp.mlp_forward_gather(vi, bc, field, dirs.contiguous(), net["w"], 1)[1]
    assert torch.equal(out["colors"].view(torch.int32), rgb.view(torch.int32)) and not torch.equal(out["colors"], plain["colors"])
    with pytest.raises(RuntimeError, match="rounds"):
        render.extract_mesh(x, c, field, mlp, level, refine_rounds=9)


def test_tracer_method_refines_on_the_loaded_tables(tn, scenes, device):
    net = _network(tn, scenes, device, "fp32")
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(net["xyz"], net["cells"])
    plain = tr.isosurface(net["values"], net["level"])
    assert "edge_bracket" not in plain and torch.equal(plain["positions"].view(torch.int32), net["surface"]["positions"].view(torch.int32))
    got = tr.isosurface(net["values"], net["level"], refine={"rounds": 3, "field": net["field"], "weights": net["w"]})
    want = net["refined"][3]
    for key in ("positions", "edge_t", "edge_bracket", "edge_frozen", "triangles", "triangle_tets", "edge_vertices"):
        assert torch.equal(got[key].view(torch.uint8), want[key].view(torch.uint8)), key
    fn = lambda vi, bc: tn.cpp.mlp_forward_gather(vi, bc, net["field"], None, net["w"], 1)   # noqa: E731
    via = tr.isosurface(net["values"], net["level"], refine={"rounds": 3, "density_fn": fn})
    assert torch.equal(via["positions"].view(torch.int32), want["positions"].view(torch.int32))
    for bad in ({"rounds": 1}, {"field": net["field"], "weights": net["w"]}, {"rounds": 1, "density_fn": fn, "field": net["field"], "weights": net["w"]}):
        with pytest.raises(RuntimeError, match="refine"):
            tr.isosurface(net["values"], net["level"], refine=bad)
    tr.close()


def test_adapter_writes_the_refined_vertices(tn, scenes, device, tmp_path):
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    standins = importlib.import_module("nerfstudio_standins")
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    io = importlib.import_module("tetra-nerf_amd.tetrahedra_io")
    xyz, cells = ic.sphere_mesh(scenes, *ic.SPHERES["sphere_300"])
    torch.manual_seed(0)
    model = standins.StandInTetrahedraNerf(standins.Config(), torch.from_numpy(xyz), torch.from_numpy(cells)).to(device)
    with torch.no_grad():
        model.tetrahedra_field[:] = torch.randn(64, len(xyz), device=device) * 0.5
        sigma = plugin.ModelMLP(model).coarse_sigma(model.tetrahedra_field.t())
    level = float(sigma.median())
    plain = plugin.extract_mesh(model, level)
    mesh = plugin.extract_mesh(model, level, path=tmp_path / "mesh.ply", refine_rounds=2)
    w = [t.detach() for t in plugin.ModelMLP(model).fused_weights()]
    surface = tn.cpp.isosurface(_dev(xyz, device), _dev(cells, device), mesh["densities"], level)
    want = tn.cpp.isosurface_refine(surface, _dev(xyz, device), mesh["densities"], level, model.tetrahedra_field.detach(), w, 2)
    assert torch.equal(mesh["positions"].view(torch.int32), want["positions"].view(torch.int32)) and torch.equal(mesh["triangles"], plain["triangles"])
    ply = io.load_mesh_ply(tmp_path / "mesh.ply")
    assert torch.equal(ply["positions"], mesh["positions"].cpu()) and not torch.equal(ply["positions"], plain["positions"].cpu())
    assert torch.equal(ply["triangles"], mesh["triangles"].cpu()) and len(ply["positions"]) > 100
    assert torch.equal(ply["colors"], (mesh["colors"].clamp(0, 1) * 255.0).round().to(torch.uint8).cpu())
