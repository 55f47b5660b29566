"""The Delaunay monitor, the per-tetrahedron state transfer and the re-triangulation on the GPU (tn_delaunay_check /
tn_remap_tet_values, csrc/tn_delaunay.hip; TetrahedraTracer.delaunay_check / retriangulate, remap_tet_values).

Bar: face states, violated faces per tetrahedron and the four counters equal the numpy statement
(geometry.delaunay_face_statement on the tracer's own face table) as integers, on both builds, on the loaded and on explicit
vertices, and past the grid cap; the transferred values equal geometry.remap_tet_values_statement bit for bit; a mesh drifted
under the step limiter until it stops being Delaunay is Delaunay again after retriangulate, traces like a tracer freshly loaded
on the new cells and like the oracle, and keeps every live tetrahedron's neighbourhood live."""
import numpy as np
import pytest
import torch

import delaunay_cases as dc

pytestmark = pytest.mark.gpu
MESHES = ["cube", "random_400", "grid_5"] + sorted(dc.HAND)
KEYS = ("num_visited_cells", "visited_cells", "vertex_indices", "hit_distances", "barycentric_coordinates")


def _dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _tracer(tn, device, pts, cells, gpu_build=1, **kw):
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    tr.load_tetrahedra(_dev(pts, device), _dev(cells, device), **kw)
    return tr


def _face_tets(tr):
    return np.ascontiguousarray(tr.face_tables()[1].numpy()).view(np.uint32)


def _compare(got, want, what, T, F):
    assert got["counters"].dtype == torch.int32 and got["counters"].shape == (4,) and got["counters"].is_cuda
    assert got["face_state"].dtype == torch.int8 and got["face_state"].shape == (F,)
    assert got["tet_violations"].dtype == torch.uint8 and got["tet_violations"].shape == (T,)
    state, per_tet = got["face_state"].cpu().numpy(), got["tet_violations"].cpu().numpy()
    bad = np.nonzero(state != want["face_state"])[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {F} face states differ (first: face {bad[:1]})"
    bad = np.nonzero(per_tet != want["tet_violations"])[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {T} per-tetrahedron counts differ (first: {bad[:1]})"
    assert got["counters"].tolist() == want["counters"].tolist(), what


@pytest.mark.parametrize("gpu_build", [1, 0])
@pytest.mark.parametrize("mesh", MESHES)
def test_kernel_equals_the_statement(tn, device, scenes, mesh, gpu_build):
    g = dc.geometry()
    pts, cells, _ = dc.case(scenes, mesh)
    tr = _tracer(tn, device, pts, cells, gpu_build)
    ft = _face_tets(tr)
    T, F = len(cells), len(ft)
    want = dc.statement(scenes, mesh, ft)
    got = tr.delaunay_check(face_state=True, tet_violations=True)              # xyz=None: the loaded vertices
    print(mesh, "gpu_build", gpu_build, "T", T, "F", F, "counters", got["counters"].tolist())
    _compare(got, want, f"{mesh}: loaded vertices", T, F)
    if mesh in dc.HAND:
        assert got["counters"].tolist() == dc.hand(mesh)[3]
    # explicit vertices: the same cells on moved positions (random_400: the move of the CPU tests, which violates faces)
    moved = dc.case(scenes, "random_400_moved")[0] if mesh == "random_400" else \
        (pts + np.random.default_rng(2).normal(scale=0.02, size=pts.shape)).astype(np.float32)
    want = g.delaunay_face_statement(cells, ft, moved)
    got = tr.delaunay_check(_dev(moved, device), face_state=True, tet_violations=True)
    _compare(got, want, f"{mesh}: explicit vertices", T, F)
    if mesh == "random_400":
        assert want["counters"][1] > 0
    # the optional arrays are optional, and the counters do not depend on them
    only = tr.delaunay_check(_dev(moved, device))
    assert only["face_state"] is None and only["tet_violations"] is None and only["counters"].tolist() == want["counters"].tolist()
    tr.close()


def test_faces_past_the_grid_cap(tn, device, scenes):
    """more faces than lanes of the capped grid: the loop takes a second trip; T is no multiple of 4 or a second mesh is taken"""
    g = dc.geometry()
    pts, cells = dc.mesh(scenes, "random_20000")
    tr = _tracer(tn, device, pts, cells)
    ft = _face_tets(tr)
    T, F = len(cells), len(ft)
    print("random_20000: T", T, "F", F, "lanes", tn.TetrahedraTracer.DELAUNAY_GRID_LANES)
    assert F > tn.TetrahedraTracer.DELAUNAY_GRID_LANES
    want = g.delaunay_face_statement(cells, ft, pts)
    _compare(tr.delaunay_check(face_state=True, tet_violations=True), want, "as built", T, F)
    assert want["counters"][1] == 0
    moved = (pts + np.random.default_rng(3).normal(scale=0.002, size=pts.shape)).astype(np.float32)
    want = g.delaunay_face_statement(cells, ft, moved)
    print("moved: counters", want["counters"].tolist())
    assert want["counters"][1] > 1000 and want["face_state"][tn.TetrahedraTracer.DELAUNAY_GRID_LANES:].max() >= 2
    _compare(tr.delaunay_check(_dev(moved, device), face_state=True, tet_violations=True), want, "moved", T, F)
    tr.close()


# ------------------------------------------------------------------------------------------------------------------ transfer
def _remap_and_compare(tn, device, old_cells, new_cells, values, V, what):
    g = dc.geometry()
    want = g.remap_tet_values_statement(old_cells, new_cells, values, V)
    out, star = tn.cpp.remap_tet_values(_dev(old_cells, device), _dev(new_cells, device), _dev(values, device), V, return_star_max=True)
    assert out.dtype == torch.float32 and out.shape == (len(new_cells),) and star.shape == (V,)
    assert np.array_equal(dc.bits(star.cpu().numpy()), dc.bits(want["star_max"])), f"{what}: star_max"
    assert np.array_equal(dc.bits(out.cpu().numpy()), dc.bits(want["values"])), f"{what}: values"
    return out


@pytest.mark.parametrize("mesh", ["cube", "random_400", "grid_5", "inside", "one_tet"])
def test_transfer_equals_the_statement(tn, device, scenes, mesh):
    pts, cells, _ = dc.case(scenes, mesh)
    new_cells = scenes.delaunay_cells(dc.case(scenes, "random_400_moved")[0].astype(np.float64)) if mesh == "random_400" \
        else cells[::-1][: max(1, len(cells) // 2)].copy()
    _remap_and_compare(tn, device, cells, new_cells, dc.occupancy_like(len(cells), 5), len(pts), mesh)


def test_transfer_edges(tn, device):
    """ids past the table on both sides; empty sides; and the rule on what the contract excludes (NaN, negative, -0)"""
    old = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [4, 20, 21, 22]], np.int32)
    new = np.array([[1, 2, 3, 5], [5, 6, 7, 8], [0, 1, 2, 9], [4, 30, 31, 32]], np.int32)
    for values in ([0.25, 0.75, 0.5], [np.inf, 3.0, 0.0], [np.nan, np.inf, 1.0], [1.0, -1e-30, 2.0], [1.0, -0.0, 0.0]):
        out = _remap_and_compare(tn, device, old, new, np.array(values, np.float32), 9, str(values))
    assert out.tolist()[1] == 0.0                                             # vertices no old cell names contribute 0
    assert tn.cpp.remap_tet_values(_dev(old, device), _dev(new[:0], device), _dev(np.ones(3, np.float32), device), 9).shape == (0,)
    none = tn.cpp.remap_tet_values(_dev(old[:0], device), _dev(new, device), _dev(np.ones(0, np.float32), device), 9)
    assert none.tolist() == [0.0] * 4


def test_transfer_past_the_grid_cap(tn, device):
    """T one block past the lanes of the capped grids on both sides: both loops take a second trip"""
    lanes = tn.TetrahedraTracer.DELAUNAY_GRID_LANES
    rng = np.random.default_rng(9)
    V, T_old, T_new = 5000, lanes + 37, lanes + 291
    old = rng.integers(0, V, size=(T_old, 4)).astype(np.int32)
    new = rng.integers(0, V, size=(T_new, 4)).astype(np.int32)
    values = np.zeros(T_old, np.float32)
    live = rng.choice(T_old, 300, replace=False)
    values[live] = rng.random(300).astype(np.float32) + 0.5
    values[T_old - 1] = 7.0                                                   # the last lane of the second trip has work
    out = _remap_and_compare(tn, device, old, new, values, V, "past the grid cap")
    assert 0 < int((out > 0).sum()) < T_new and float(out.max()) == 7.0


# ---------------------------------------------------------------------------------------------------------------- whole loop
def test_drift_retriangulate_and_trace(tn, device, scenes, oracle):
    g = dc.geometry()
    pts, cells = dc.mesh(scenes, "random_1500")
    V, M = len(pts), 256
    v, old_cells = _dev(pts, device), _dev(cells, device)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(v, old_cells, refittable=True)
    assert tr.delaunay_check()["counters"].tolist()[1:] == [0, 0, 0]
    rng = np.random.default_rng(31)
    violated = steps = 0
    while violated == 0 and steps < 40:                                       # an optimiser's drift, limited and followed
        snapshot = v.clone()
        v += _dev(rng.normal(scale=0.01, size=pts.shape).astype(np.float32), device)
        counters, _ = tr.limit_vertex_step(snapshot, v, 0.25)
        assert counters.tolist()[2:] == [0, 0], "flipped / collapsed"
        tr.update_vertices(v)
        violated = tr.delaunay_check()["counters"].tolist()[1]
        steps += 1
    print("steps", steps, "counters", tr.delaunay_check()["counters"].tolist())
    assert violated > 0
    moved = v.cpu().numpy()
    occupancy = dc.occupancy_like(len(cells), 13)
    out = tr.retriangulate(v, [_dev(occupancy, device)])
    new_cells = out["cells"]
    assert out["num_tetrahedra"] == len(new_cells) and new_cells.dtype == torch.int32 and new_cells.is_cuda
    assert tr.tetrahedra_cells is new_cells and tr.tetrahedra_vertices is v and tr._refittable
    after = tr.delaunay_check()["counters"].tolist()
    print("after retriangulate: T", len(cells), "->", len(new_cells), "counters", after)
    assert after[1] == 0 and after[0] > 0
    # the tracer answers as one freshly loaded on the returned cells, and as the oracle
    fresh = tn.TetrahedraTracer(device)
    fresh.load_tetrahedra(v.clone(), new_cells.clone())
    o, d = scenes.outside_in_rays(2048, 41)
    a, b = tr.trace_rays(_dev(o, device), _dev(d, device), M), fresh.trace_rays(_dev(o, device), _dev(d, device), M)
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(moved, new_cells.cpu().numpy())
    want = ot.trace_rays(o, d, M)
    assert int(a["num_visited_cells"].max()) > 0
    for k in KEYS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: retriangulated vs freshly loaded"
        assert np.array_equal(a[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), f"{k}: vs the oracle"
    # it still follows its vertices
    v += 1e-4
    tr.update_vertices(v)
    # the transferred occupancy: the statement's, and conservative against the old mesh
    carried = out["tet_values"][0].cpu().numpy()
    new_np = new_cells.cpu().numpy()
    assert np.array_equal(dc.bits(carried), dc.bits(g.remap_tet_values_statement(cells, new_np, occupancy, V)["values"]))
    star = np.zeros(V, np.float32)
    np.maximum.at(star, cells.reshape(-1), np.repeat(occupancy, 4))
    assert np.all(carried[:, None] >= star[new_np]) and np.array_equal(carried, star[new_np].max(1))
    for t in np.nonzero(occupancy > 0)[0][:50]:                               # spelled out: around every vertex of a live old cell
        touching = np.isin(new_np, cells[t]).any(1)
        assert np.all(carried[touching] >= occupancy[t])
    tr.close(); fresh.close()


def test_a_failed_triangulation_leaves_the_tracer_as_it_was(tn, device, scenes):
    pts, cells = dc.mesh(scenes, "random_400")
    tr = _tracer(tn, device, pts, cells)
    loaded_v, loaded_c = tr.tetrahedra_vertices, tr.tetrahedra_cells
    flat = _dev(np.ascontiguousarray(pts * np.float32([1, 1, 0])), device)    # coplanar points: Qhull refuses
    with pytest.raises(Exception):
        tr.retriangulate(flat)
    assert tr.tetrahedra_vertices is loaded_v and tr.tetrahedra_cells is loaded_c
    assert tr.delaunay_check()["counters"].tolist()[1] == 0
    o, d = scenes.outside_in_rays(256, 4)
    assert int(tr.trace_rays(_dev(o, device), _dev(d, device), 256)["num_visited_cells"].max()) > 0
    tr.close()


# -------------------------------------------------------------------------------------------------------------------- errors
def test_errors_touch_nothing(tn, device, scenes):
    pts, cells = dc.mesh(scenes, "cube")
    tr = _tracer(tn, device, pts, cells)
    x = _dev(pts, device)
    empty = tn.TetrahedraTracer(device)
    with pytest.raises(RuntimeError, match="load"):
        empty.delaunay_check()
    with pytest.raises(RuntimeError, match="load"):
        empty.delaunay_check(x)
    with pytest.raises(RuntimeError, match="load"):
        empty.retriangulate(x)
    with pytest.raises(RuntimeError):
        tr.delaunay_check(x[:8])                                              # another V
    with pytest.raises(RuntimeError, match="float32"):
        tr.delaunay_check(x.double())
    with pytest.raises(RuntimeError, match="CUDA"):
        tr.delaunay_check(x.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        tr.delaunay_check(torch.zeros(len(pts), 4, device=device)[:, :3])
    with pytest.raises(RuntimeError, match="tet_values"):
        tr.retriangulate(x, [torch.zeros(len(cells) + 1, device=device)])
    c = _dev(cells, device)
    with pytest.raises(RuntimeError, match="int32"):
        tn.cpp.remap_tet_values(c.long(), c, torch.zeros(len(cells), device=device), len(pts))
    with pytest.raises(RuntimeError, match="one value per row"):
        tn.cpp.remap_tet_values(c, c, torch.zeros(len(cells) + 1, device=device), len(pts))
    # the C entries themselves
    lib, V, T, F = tr._lib, len(pts), len(cells), int(tr._lib.tn_num_faces(tr._h))
    counters = torch.full((4,), 7, dtype=torch.int32, device=device)
    state = torch.full((F,), 7, dtype=torch.int8, device=device)
    per_tet = torch.full((4 * ((T + 3) // 4) + 4,), 7, dtype=torch.uint8, device=device)
    p = lambda t: t.data_ptr()   # noqa: E731
    assert lib.tn_delaunay_check(empty._h, V, p(x), p(counters), p(state), p(per_tet), None) != 0
    assert lib.tn_delaunay_check(tr._h, V - 1, p(x), p(counters), p(state), p(per_tet), None) != 0
    assert lib.tn_delaunay_check(tr._h, V, None, p(counters), p(state), p(per_tet), None) != 0
    assert lib.tn_delaunay_check(tr._h, V, p(x), None, p(state), p(per_tet), None) != 0
    assert lib.tn_delaunay_check(tr._h, V, p(x), p(counters), p(state), p(per_tet) + 1, None) != 0       # misaligned byte counters
    assert b"aligned" in lib.tn_last_error()
    out, star = torch.full((T,), 7.0, device=device), torch.full((V,), 7.0, device=device)
    vals = torch.ones(T, device=device)
    for args in ((None, p(vals), p(c), p(out), p(star)), (p(c), None, p(c), p(out), p(star)), (p(c), p(vals), None, p(out), p(star)),
                 (p(c), p(vals), p(c), None, p(star)), (p(c), p(vals), p(c), p(out), None)):
        assert lib.tn_remap_tet_values(V, T, args[0], args[1], T, args[2], args[3], args[4], None) != 0
    torch.cuda.synchronize()
    assert counters.tolist() == [7] * 4 and bool((state == 7).all()) and bool((per_tet == 7).all())
    assert bool((out == 7).all()) and bool((star == 7).all())
    # a good call writes the T bytes it owns, whole words of them, and nothing behind
    assert lib.tn_delaunay_check(tr._h, V, p(x), p(counters), None, p(per_tet), None) == 0
    torch.cuda.synchronize()
    assert per_tet[4 * ((T + 3) // 4):].tolist() == [7] * 4 and int(per_tet[:T].max()) <= 4
    empty.close(); tr.close()
