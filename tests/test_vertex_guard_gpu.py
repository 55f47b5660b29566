"""The vertex step limiter on the GPU (tn_tet_quality / tn_limit_vertex_step, csrc/tn_vertex_guard.hip;
TetrahedraTracer.tet_quality / limit_vertex_step).

Bar: star widths, widths, orientations, the limited positions and the four counters equal the torch statement
(geometry.limit_vertex_step_statement, computed on the CPU once per mesh: tests/vertex_guard_cases.py) bit for bit; inside the
bound the call's own cross-check counts no flipped and no collapsed tetrahedron while the unlimited step flips some; a tracer
refitted to the limited vertices answers as one freshly loaded on them."""
import numpy as np
import pytest
import torch

import vertex_guard_cases as vc

pytestmark = pytest.mark.gpu
_TRACERS = {}


def _dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _loaded(tn, device, name, old, cells, **kw):
    """a tracer loaded on (old, cells), made once per name"""
    if name not in _TRACERS:
        tr = tn.TetrahedraTracer(device)
        tr.load_tetrahedra(_dev(old, device), _dev(cells, device), **kw)
        _TRACERS[name] = tr
    return _TRACERS[name]


def _assert_bits(got, want, what):
    got, want = vc.bits(got.cpu()), vc.bits(want.cpu())
    if not torch.equal(got, want):
        bad = (got != want).reshape(len(got), -1).any(1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(got)} rows differ (first: {int(bad.nonzero()[0, 0])})")


def _limit_and_compare(tr, device, old, new, want, fraction, what, verify=True):
    x = _dev(new, device)
    counters, star = tr.limit_vertex_step(_dev(old, device), x, fraction, verify=verify)
    assert counters.dtype == torch.int32 and counters.shape == (4,) and counters.device == x.device
    _assert_bits(star, want["star_width"], f"{what}: star_width")
    _assert_bits(x, want["xyz"], f"{what}: limited positions")
    expect = want["counters"].tolist()
    assert counters.tolist() == (expect if verify else expect[:2] + [0, 0]), what
    return counters


@pytest.mark.parametrize("mesh", vc.KERNEL_MESHES)
def test_kernels_equal_the_statement(tn, device, scenes, mesh):
    old, new, cells = vc.case(scenes, mesh)
    tr = _loaded(tn, device, mesh, old, cells)
    w, o, star = vc.quality(scenes, mesh)
    q = tr.tet_quality()
    assert q["orient"].dtype == torch.int8
    _assert_bits(q["width"], w, f"{mesh}: width")
    assert torch.equal(q["orient"].cpu(), o), f"{mesh}: orient"
    _assert_bits(q["star_width"], star, f"{mesh}: star_width of tet_quality")
    _limit_and_compare(tr, device, old, new, vc.statement(scenes, mesh, 0.45), 0.45, mesh)
    _limit_and_compare(tr, device, old, new, vc.statement(scenes, mesh, 0.25), 0.25, f"{mesh} at 0.25, no verify", verify=False)


@pytest.mark.parametrize("mesh", vc.KERNEL_MESHES)
def test_the_guard_holds_where_it_claims_to(tn, device, scenes, mesh):
    old, new, cells = vc.case(scenes, mesh)
    tr = _loaded(tn, device, mesh, old, cells)
    x = _dev(new, device)
    counters, _ = tr.limit_vertex_step(_dev(old, device), x, 0.45)
    c = counters.tolist()
    print(mesh, "counters", c)
    assert c[0] > 0 and c[2] == 0 and c[3] == 0
    before = tr.tet_quality()["orient"].to(torch.int32)
    assert int((before * tr.tet_quality(x)["orient"].to(torch.int32) < 0).sum()) == 0
    unlimited = tr.tet_quality(_dev(new, device))["orient"].to(torch.int32)
    flips = int((before * unlimited < 0).sum())
    print(mesh, "tetrahedra the unlimited step flips:", flips)
    assert flips > 0


def test_edges_of_the_clamp(tn, device, scenes):
    """V = 1501 and T = 9682 are off every wave and block multiple; vertex 1500 is named by no cell"""
    g = vc.geometry()
    old, new, cells = vc.case(scenes, "random_1500")
    assert len(cells) % 64 and (len(old) + 1) % 64
    old = np.concatenate([old, [[5.0, 6.0, 7.0]]]).astype(np.float32)
    new = np.concatenate([new, [[50.0, -60.0, 70.0]]]).astype(np.float32)
    new[3, 1], new[7, 0] = np.nan, np.inf
    tr = _loaded(tn, device, "random_1501", old, cells)
    want = g.limit_vertex_step_statement(torch.from_numpy(old), torch.from_numpy(new), torch.from_numpy(cells), 0.45)
    assert not want["frozen"][[3, 7]].any() and want["clamped"][[3, 7]].all() and not want["clamped"][1500]
    x = _dev(new, device)
    counters, star = tr.limit_vertex_step(_dev(old, device), x, 0.45)
    _assert_bits(x, want["xyz"], "limited positions")
    assert counters.tolist() == want["counters"].tolist()
    assert int(vc.bits(star.cpu())[1500]) == 0x7F800000                       # +inf: never limited
    _assert_bits(x[1500:], torch.from_numpy(new[1500:]), "the vertex no cell names")
    _assert_bits(x[[3, 7]], torch.from_numpy(old[[3, 7]]), "the NaN and the inf vertex went back")
    # nothing moved: nothing written, nothing counted
    same = _dev(old, device)
    counters, _ = tr.limit_vertex_step(_dev(old, device), same, 0.45)
    _assert_bits(same, torch.from_numpy(old), "unmoved vertices")
    assert counters.tolist() == [0, 0, 0, 0]
    # verify=False: counters 0 and 1 as with the pass, 2 and 3 stay at the 0 the call wrote
    off, _ = tr.limit_vertex_step(_dev(old, device), _dev(new, device), 0.45, verify=False)
    assert off.tolist() == want["counters"].tolist()[:2] + [0, 0] and off.tolist()[0] > 0


def test_one_block_past_the_grid_cap(tn, device):
    """T and V one block past the lanes of the capped grids: the kernels' loops take a second trip.  Cells are drawn at random
    over 1000 of the vertices, so orientation means nothing here; only equality with the statement counts.  load_tetrahedra
    refuses such cells (triangles shared by many tetrahedra), and the limiter reads nothing of a tracer but the cells tensor
    it borrows: the tracer is loaded on a chain of T tetrahedra (i, i+1, i+2, i+3) along a helix and the random cells are then
    written into that tensor."""
    g = vc.geometry()
    lanes = tn.TetrahedraTracer.VERTEX_GUARD_GRID_LANES
    T = lanes + 37
    V = T + 3
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(V, 1000, replace=False))
    ids[-1] = V - 1                                                             # the last lane of the second trip has work
    pick = rng.integers(0, 1000, size=(T, 4))
    for _ in range(8):                                                          # four different vertices per cell
        srt = np.sort(pick, 1)
        bad = (srt[:, 1:] == srt[:, :-1]).any(1)
        pick[bad] = rng.integers(0, 1000, size=(int(bad.sum()), 4))
    assert not bad.any()
    cells = ids[pick].astype(np.int32)
    old = rng.uniform(-1, 1, size=(V, 3)).astype(np.float32)
    new = (old + rng.normal(scale=1e-4, size=(V, 3))).astype(np.float32)
    new[V - 1] = old[V - 1] + np.float32(0.5)
    w, o = g.tet_width_orient(torch.from_numpy(old), torch.from_numpy(cells))
    want = g.limit_vertex_step_statement(torch.from_numpy(old), torch.from_numpy(new), torch.from_numpy(cells), 0.45)
    kept = ~want["clamped"] & ~want["frozen"]
    assert want["clamped"][ids].sum() > 100 and kept[ids].sum() > 100 and want["clamped"][V - 1]
    i = np.arange(V, dtype=np.float64)
    helix = np.stack([np.cos(0.1 * i), np.sin(0.1 * i), 1e-3 * i], 1).astype(np.float32)
    borrowed = _dev((np.arange(T)[:, None] + np.arange(4)[None, :]).astype(np.int32), device)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(_dev(helix, device), borrowed)
    borrowed.copy_(_dev(cells, device))
    q = tr.tet_quality(_dev(old, device))
    _assert_bits(q["width"], w, "width")
    assert torch.equal(q["orient"].cpu(), o)
    _assert_bits(q["star_width"], want["star_width"], "star_width")
    _limit_and_compare(tr, device, old, new, want, 0.45, "past the grid cap")
    tr.close()


def test_limited_step_then_refit_equals_a_fresh_load(tn, device, scenes):
    old, new, cells = vc.case(scenes, "random_1500")
    tr = tn.TetrahedraTracer(device)
    v = _dev(old, device)
    tr.load_tetrahedra(v, _dev(cells, device), refittable=True)
    x = _dev(new, device)
    counters, _ = tr.limit_vertex_step(v, x, 0.45)
    tr.update_vertices(x)
    fresh = tn.TetrahedraTracer(device)
    fresh.load_tetrahedra(x.clone(), _dev(cells, device))
    o, d = scenes.outside_in_rays(4096, 40)
    to, td = _dev(o, device), _dev(d, device)
    a, b = tr.trace_rays(to, td, 256), fresh.trace_rays(to, td, 256)
    assert int(a["num_visited_cells"].max()) > 0
    for k in a:
        _assert_bits(a[k], b[k], f"{k}: refitted to the limited vertices vs freshly loaded on them")
    assert counters.tolist()[2:] == [0, 0]
    tr.close(); fresh.close()


def test_errors_touch_nothing(tn, device, scenes):
    old, new, cells = vc.case(scenes, "cube")
    tr = _loaded(tn, device, "cube", old, cells)
    a, b = _dev(old, device), _dev(new, device)
    for fraction in (0.0, -0.25, 0.4500001, 1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="fraction"):
            tr.limit_vertex_step(a, b, fraction)
    empty = tn.TetrahedraTracer(device)
    with pytest.raises(RuntimeError, match="load"):
        empty.limit_vertex_step(a, b, 0.25)
    with pytest.raises(RuntimeError, match="load"):
        empty.tet_quality(a)
    with pytest.raises(RuntimeError):
        tr.limit_vertex_step(a[:8], b[:8], 0.25)                                # another V
    with pytest.raises(RuntimeError):
        tr.tet_quality(a[:8])
    with pytest.raises(RuntimeError, match="float32"):
        tr.limit_vertex_step(a.double(), b, 0.25)
    with pytest.raises(RuntimeError, match="float32"):
        tr.limit_vertex_step(a, b.double(), 0.25)
    with pytest.raises(RuntimeError, match="CUDA"):
        tr.limit_vertex_step(a.cpu(), b, 0.25)
    with pytest.raises(RuntimeError, match="CUDA"):
        tr.tet_quality(a.cpu())
    wide = torch.zeros(len(old), 4, device=device)
    with pytest.raises(RuntimeError, match="contiguous"):
        tr.limit_vertex_step(a, wide[:, :3], 0.25)
    with pytest.raises(RuntimeError, match="contiguous"):
        tr.tet_quality(wide[:, :3])
    # the C entries themselves: the loaded V, null pointers, unknown flags
    lib, V = tr._lib, len(old)
    star, counters = torch.full((V,), 7.0, device=device), torch.full((4,), 7, dtype=torch.int32, device=device)
    p = lambda t: t.data_ptr()
    assert lib.tn_limit_vertex_step(tr._h, V - 1, p(a), p(b), 0.25, p(star), p(counters), 0, None) != 0
    assert lib.tn_limit_vertex_step(empty._h, V, p(a), p(b), 0.25, p(star), p(counters), 0, None) != 0
    assert lib.tn_limit_vertex_step(tr._h, V, p(a), p(b), 0.5, p(star), p(counters), 0, None) != 0
    assert lib.tn_limit_vertex_step(tr._h, V, p(a), p(b), 0.25, p(star), p(counters), 2, None) != 0
    for args in ((None, p(b), p(star), p(counters)), (p(a), None, p(star), p(counters)), (p(a), p(b), None, p(counters)),
                 (p(a), p(b), p(star), None)):
        assert lib.tn_limit_vertex_step(tr._h, V, args[0], args[1], 0.25, args[2], args[3], 0, None) != 0
    assert lib.tn_tet_quality(tr._h, V, None, None, None, p(star), None) != 0
    assert lib.tn_tet_quality(tr._h, V + 1, p(a), None, None, p(star), None) != 0
    torch.cuda.synchronize()
    _assert_bits(b, torch.from_numpy(new), "xyz_new after refused calls")
    assert star.tolist() == [7.0] * V and counters.tolist() == [7] * 4
    # and every output of tn_tet_quality is optional
    assert lib.tn_tet_quality(tr._h, V, p(a), None, None, None, None) == 0
    empty.close()
