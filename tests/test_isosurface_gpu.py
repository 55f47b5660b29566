"""The isosurface extraction on the GPU (tn_isosurface_count / tn_isosurface_emit, csrc/tn_isosurface.hip; cpp.isosurface,
TetrahedraTracer.isosurface, render.extract_mesh, nerfstudio_plugin.extract_mesh).

Bar: on every case of tests/isosurface_cases.py the five arrays, the two offset arrays and both totals equal the numpy statement
(geometry.isosurface_statement) byte for byte; two runs give the same bytes; a refused call touches nothing and a call with
smaller totals writes nothing behind them; the tracer's method is the free function; extract_mesh's surface is the statement's on
the kernel's own densities and its colours are within the project's 1e-5 fp32 bar of the PyTorch MLP on the same features and
directions."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import isosurface_cases as ic

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _extract(tn, device, case):
    xyz, cells, values, level, mask = case
    return tn.cpp.isosurface(_dev(xyz, device), _dev(cells, device), _dev(values, device), level, _dev(mask, device))


def _compare(got, want, what):
    assert got["num_triangles"] == want["num_triangles"] and got["num_refs"] == want["num_refs"], what
    for key, dtype in (("positions", torch.float32), ("triangles", torch.int32), ("triangle_tets", torch.int32),
                       ("edge_vertices", torch.int32), ("edge_t", torch.float32), ("tri_offsets", torch.int32), ("ref_offsets", torch.int32)):
        assert got[key].dtype == dtype and got[key].is_cuda and tuple(got[key].shape) == want[key].shape, (what, key, got[key].shape)
        bad = np.nonzero(ic.bits(got[key].cpu().numpy()).reshape(-1) != ic.bits(want[key]).reshape(-1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {want[key].size} words of {key} differ (first: {bad[:1]})"


@pytest.mark.parametrize("name", ic.names())
def test_kernels_equal_the_statement(tn, device, scenes, name):
    want = ic.statement(scenes, name)
    got = _extract(tn, device, ic.case(scenes, name))
    print(name, "T", len(ic.case(scenes, name)[1]), "triangles", got["num_triangles"], "refs", got["num_refs"], "vertices", len(got["positions"]))
    _compare(got, want, name)


def test_two_runs_give_the_same_bytes(tn, device, scenes):
    bt, blocks = ic.kernel_constants()
    for name in ("sphere_1000", f"soup_{bt * blocks + 1}"):
        a, b = _extract(tn, device, ic.case(scenes, name)), _extract(tn, device, ic.case(scenes, name))
        for key in ic.ARRAYS:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (name, key)


def test_tracer_method_is_the_free_function(tn, device, scenes):
    g = ic.geometry()
    xyz, cells, values, level, _ = ic.case(scenes, "sphere_300")
    _, _, _, _, mask = ic.case(scenes, "sphere_120_masked")
    tr = tn.TetrahedraTracer(device)
    assert tr.supports_isosurface
    with pytest.raises(RuntimeError, match="load"):
        tr.isosurface(_dev(values, device), level)
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
    _compare(tr.isosurface(_dev(values, device), level), ic.statement(scenes, "sphere_300"), "loaded vertices")
    moved = (xyz + np.random.default_rng(4).normal(scale=0.01, size=xyz.shape)).astype(np.float32)
    mask = (np.random.default_rng(6).random(len(cells)) < 0.6).astype(np.uint8)
    got = tr.isosurface(_dev(values, device), level, tet_mask=_dev(mask, device).bool(), xyz=_dev(moved, device))
    _compare(got, g.isosurface_statement(moved, cells, values, level, mask), "explicit vertices, bool mask")
    with pytest.raises(RuntimeError):
        tr.isosurface(_dev(values, device), level, xyz=_dev(moved[:-1], device))
    tr.close()


def test_refused_and_short_calls_touch_nothing_they_do_not_own(tn, device, scenes):
    """a refused call leaves every output as it was; a call told smaller totals than the surface has -- what a caller who changed
    `values` between the two entries amounts to -- writes nothing behind those totals"""
    lib = importlib.import_module("tetra-nerf_amd._lib").load()
    xyz, cells, values, level, _ = ic.case(scenes, "sphere_300")
    want = ic.statement(scenes, "sphere_300")
    V, T, M, R = len(values), len(cells), want["num_triangles"], want["num_refs"]
    x, c, v = _dev(xyz, device), _dev(cells, device), _dev(values, device)
    p = lambda t: t.data_ptr()   # noqa: E731
    seven = lambda *shape, dtype=torch.int32: torch.full(shape, 7, dtype=dtype, device=device)   # noqa: E731
    tri_off, ref_off = seven(T + 1), seven(T + 1)
    for args in ((V, T, p(c), p(v), float("nan"), None, p(tri_off), p(ref_off)), (V, T, None, p(v), level, None, p(tri_off), p(ref_off)),
                 (V, T, p(c), p(v), level, None, None, p(ref_off)), (V, 2 ** 30, p(c), p(v), level, None, p(tri_off), p(ref_off)),
                 (V, T, p(c), p(v), 2.0 ** 126, None, p(tri_off), p(ref_off))):
        assert lib.tn_isosurface_count(*args, None) != 0
    torch.cuda.synchronize()
    assert bool((tri_off == 7).all()) and bool((ref_off == 7).all())
    assert lib.tn_isosurface_count(V, T, p(c), p(v), level, None, p(tri_off), p(ref_off), None) == 0
    assert tri_off.tolist() == want["tri_offsets"].tolist() and ref_off.tolist() == want["ref_offsets"].tolist()
    tris, tets, ev = seven(M, 3), seven(M), seven(R, 2)
    et, pos, n = seven(R, dtype=torch.float32), seven(R, 3, dtype=torch.float32), seven(1)
    outs = (p(tris), p(tets), p(ev), p(et), p(pos), p(n))
    good = (V, T, p(x), p(c), p(v), level, None, p(tri_off), p(ref_off), M, R)
    for bad in ((V, T, None) + good[3:], good[:5] + (float("inf"),) + good[6:], good[:9] + (2 * T + 1, R), good[:9] + (M, 4 * T + 1)):
        assert lib.tn_isosurface_emit(*bad, *outs, None) != 0
    for k in range(6):
        assert lib.tn_isosurface_emit(*good, *(None if j == k else o for j, o in enumerate(outs)), None) != 0
    torch.cuda.synchronize()
    for t in (tris, tets, ev, et, pos, n):
        assert bool((t == 7).all())
    # smaller totals: the stores stop there
    assert lib.tn_isosurface_emit(*good[:9], M - 9, R - 11, *outs, None) == 0
    torch.cuda.synchronize()
    assert bool((tris[M - 9:] == 7).all()) and bool((tets[M - 9:] == 7).all()) and bool((tets[:M - 9] != 7).any())
    assert bool((ev[R - 11:] == 7).all()) and bool((et[R - 11:] == 7).all()) and bool((pos[R - 11:] == 7).all())
    assert 0 < int(n) <= R - 11 and int(tris[:M - 9].max()) < R - 11 and int(tris[:M - 9].min()) >= 0
    # and the full call on the same buffers is the statement
    assert lib.tn_isosurface_emit(*good, *outs, None) == 0
    N = int(n)
    assert N == len(want["positions"]) and np.array_equal(tris.cpu().numpy(), want["triangles"])
    assert np.array_equal(ic.bits(pos[:N].cpu().numpy()), ic.bits(want["positions"])) and bool((pos[N:] == 7).all())
    # the wrappers' own refusals
    with pytest.raises(RuntimeError, match="level"):
        tn.cpp.isosurface(x, c, v, float("nan"))
    with pytest.raises(RuntimeError, match="int32"):
        tn.cpp.isosurface(x, c.long(), v, level)
    with pytest.raises(RuntimeError, match="xyz"):
        tn.cpp.isosurface(x[:-1], c, v, level)
    with pytest.raises(RuntimeError, match="tet_mask"):
        tn.cpp.isosurface(x, c, v, level, torch.ones(T + 1, dtype=torch.uint8, device=device))


# ------------------------------------------------------------------------------------------------------------- extract_mesh
def _field_and_mlp(render, V, device, seed):
    torch.manual_seed(seed)
    mlp = render.TetraMLP().to(device)
    field = (torch.randn(64, V, device=device) * 0.5).contiguous()
    return field, mlp


def test_extract_mesh_on_a_synthetic_field(tn, device, scenes):
    g = ic.geometry()
    render = importlib.import_module("tetra-nerf_amd.render")
    xyz, cells = ic.sphere_mesh(scenes, *ic.SPHERES["sphere_300"])
    V, T = len(xyz), len(cells)
    field, mlp = _field_and_mlp(render, V, device, 3)
    with torch.no_grad():
        sigma = render.coarse_sigma(mlp, field.t())                           # the PyTorch density at the vertices
    level = float(sigma.median())
    out = render.extract_mesh(_dev(xyz, device), _dev(cells, device), field, mlp, level)
    np.testing.assert_allclose(out["densities"].cpu().numpy(), sigma.cpu().numpy(), rtol=1e-5, atol=1e-5)
    want = g.isosurface_statement(xyz, cells, out["densities"], level)        # the kernel's own densities
    _compare(out, want, "extract_mesh")
    N = len(out["positions"])
    print("extract_mesh: V", V, "T", T, "level", level, "vertices", N, "triangles", out["num_triangles"])
    assert N > 200 and out["colors"].shape == (N, 3) and out["directions"].shape == (N, 3)
    # colours: the PyTorch MLP on the same features (the gather of the same two field rows) and the same directions
    ev, t = out["edge_vertices"].long(), out["edge_t"][:, None]
    rows = field.t()
    feats = (1.0 - t) * rows[ev[:, 0]] + t * rows[ev[:, 1]]
    with torch.no_grad():
        _, rgb = mlp(feats, out["directions"])
    err = float((out["colors"] - rgb).abs().max())
    print("colours: max |fused - torch|", err)
    assert err <= 1e-5
    np.testing.assert_allclose(out["directions"].norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)
    # the occupancy pair masks what an evaluation render would cull; colours off: nothing but the surface
    occ = torch.rand(T, generator=torch.Generator().manual_seed(1)).to(device)
    masked = render.extract_mesh(_dev(xyz, device), _dev(cells, device), field, mlp, level, occupancy=occ, occupancy_threshold=0.4,
                                 colors=False)
    assert masked["colors"] is None and masked["directions"] is None
    _compare(masked, g.isosurface_statement(xyz, cells, out["densities"], level, (occ.cpu().numpy() >= 0.4).astype(np.uint8)), "masked")
    assert 0 < masked["num_triangles"] < out["num_triangles"]
    none = render.extract_mesh(_dev(xyz, device), _dev(cells, device), field, mlp, float(sigma.max()) + 1.0)
    assert none["positions"].shape == (0, 3) and none["colors"].shape == (0, 3) and none["num_triangles"] == 0


def test_adapter_on_the_stand_in_model(tn, device, scenes, tmp_path):
    g = ic.geometry()
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
    mesh = plugin.extract_mesh(model, level, path=tmp_path / "mesh.ply")
    _compare(mesh, g.isosurface_statement(xyz, cells, mesh["densities"], level), "adapter")
    np.testing.assert_allclose(mesh["densities"].cpu().numpy(), sigma.cpu().numpy(), rtol=1e-5, atol=1e-5)
    ply = io.load_mesh_ply(tmp_path / "mesh.ply")
    assert torch.equal(ply["positions"], mesh["positions"].cpu()) and torch.equal(ply["triangles"], mesh["triangles"].cpu())
    assert torch.equal(ply["colors"], (mesh["colors"].clamp(0, 1) * 255.0).round().to(torch.uint8).cpu()) and len(ply["positions"]) > 100
    # with the reference's occupancy buffer and a threshold the culled tetrahedra are masked out
    occ = torch.rand(len(cells), generator=torch.Generator().manual_seed(2)).to(device)
    model.register_buffer("tetrahedra_occupancy", occ)
    model.config.occupancy_threshold = 0.5
    masked = plugin.extract_mesh(model, level)
    _compare(masked, g.isosurface_statement(xyz, cells, mesh["densities"], level, (occ.cpu().numpy() >= 0.5).astype(np.uint8)), "adapter, masked")
