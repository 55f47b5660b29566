"""The refit on the GPU (tn_update_vertices, csrc/tn_refit.hip; TetrahedraTracer.update_vertices).

`tr` is loaded with refittable=True on vertices A and refitted to B (tests/refit_cases.py: interior vertices moved by a tenth of
their star's smallest height, then an affine map that moves the mesh out of its old box); `fresh` is loaded on B.  Bar: every
query answers on `tr` as it does on `fresh`, bit for bit; the tables hold a fresh build's geometry at the refitted tracer's own
(kept) order; nothing topological is touched; a refit back to A restores every table byte for byte."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

import refit_cases

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))

KEYS = ("num_visited_cells", "visited_cells", "vertex_indices", "hit_distances", "barycentric_coordinates")
MESHES = ("random_1500", "grid_12_jitter", "grid_16", "cube")
M = 256
_CASES = {}


def _case(scenes, name):
    """(A, B, cells) of one mesh, made once per session"""
    if name not in _CASES:
        pts, cells = refit_cases.meshes(scenes)[name]
        _CASES[name] = (np.ascontiguousarray(pts, np.float32), refit_cases.moved(pts, cells), np.ascontiguousarray(cells))
    return _CASES[name]


def _dev(x, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _tracer(tn, device, pts, cells, refittable=False, **options):
    tr = tn.TetrahedraTracer(device)
    for k, v in options.items():
        tr.set_option(k, v)
    tr.load_tetrahedra(_dev(pts, device), _dev(cells, device), refittable=refittable)
    return tr


def _refitted(tn, device, a, b, cells, **options):
    tr = _tracer(tn, device, a, cells, True, **options)
    tr.update_vertices(_dev(b, device))
    return tr


def _rays(scenes, device, n, seed):
    """outside-in and inside-out rays of the unit cube, moved with the mesh"""
    o1, d1 = scenes.outside_in_rays(n - n // 2, seed)
    o2, d2 = scenes.inside_out_rays(n // 2, seed + 1)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    o, d = refit_cases.affine(o), refit_cases.affine_dirs(d)
    return o, d, _dev(o, device), _dev(d, device)


def _assert_same_rows(a, b, ctx):
    import torch

    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        if not torch.equal(x, y):
            diff = (x != y).reshape(len(x), -1).any(1)
            raise AssertionError(f"{ctx}: {k} differs on {int(diff.sum())} rows (first: {int(diff.nonzero()[0, 0])})")


def _trace(tr, to, td, walk=None, **kw):
    if walk is not None:
        tr.set_option("walk", walk)
    out = tr.trace_rays(to, td, M, **kw)
    if walk is not None:
        tr.set_option("walk", 1)
    return out


def _compare_tracers(tr, fresh, scenes, device, ctx, seed=40):
    _, _, to, td = _rays(scenes, device, 3000, seed)
    bvh = _trace(tr, to, td, 0)
    _assert_same_rows(bvh, _trace(fresh, to, td, 0), f"{ctx}: BVH path, refitted vs fresh")
    walk = _trace(tr, to, td, 2)
    assert tr.trace_stats()["walk"] > 0 or ctx.startswith("cube")
    _assert_same_rows(walk, _trace(fresh, to, td, 2), f"{ctx}: walk, refitted vs fresh")
    _assert_same_rows(walk, bvh, f"{ctx}: walk vs BVH path on the refitted tracer")


@pytest.mark.parametrize("mesh", MESHES)
def test_refit_rows_equal_fresh_load(tn, device, scenes, oracle, mesh):
    a, b, cells = _case(scenes, mesh)
    tr, fresh = _refitted(tn, device, a, b, cells), _tracer(tn, device, b, cells)
    _compare_tracers(tr, fresh, scenes, device, mesh)
    _, _, to, td = _rays(scenes, device, 16384, 42)          # the default dispatch: the walk schedule
    big = _trace(tr, to, td)
    assert tr.trace_stats()["walk"] > 0
    _assert_same_rows(big, _trace(fresh, to, td), f"{mesh}: default dispatch, refitted vs fresh")
    if mesh != "random_1500":
        return
    for opts in (dict(writer_table=2), dict(leaf_width=32), dict(leaf_width=64)):
        _compare_tracers(_refitted(tn, device, a, b, cells, **opts), _tracer(tn, device, b, cells, **opts), scenes, device, f"{mesh} {opts}", 44)
    for ends in (0, 1, 3):
        tr.set_option("cert_ends", ends); fresh.set_option("cert_ends", ends)
        _compare_tracers(tr, fresh, scenes, device, f"{mesh} cert_ends={ends}", 46)
    tr.set_option("cert_ends", 2)
    # the oracle is the definition of a hit
    o, d, to, td = _rays(scenes, device, 2000, 48)
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(b, cells)
    want = ot.trace_rays(o, d, M)
    for walk in (0, 2):
        got = _trace(tr, to, td, walk)
        for k in KEYS:
            g, w = got[k].cpu().numpy(), np.ascontiguousarray(want[k])
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"walk={walk}: {k} differs from the oracle on B"


# ---------------------------------------------------------------------------------------------------------------- tables
def _records(tr):
    """the 64-byte walk records as uint32 [4T, 16] (tn_common.h: WalkVar), sorted by (caller tet id, entry face)"""
    r = tr.build_table(2).numpy().view(np.uint32).reshape(-1, 16)
    key = r[:, 8].astype(np.int64) * 4 + (np.arange(len(r)) & 3)
    assert len(np.unique(key)) == len(r)
    return r[np.argsort(key)]


_PN, _CODE_HI, _THIN = [0, 1, 2], 10, np.uint32(0xFF00)


def _topology(r):
    r = r.copy()
    r[:, _PN] = 0
    r[:, _CODE_HI] &= ~_THIN
    return r


def _hull_set(tr):
    """hull triangles as a set of (nine position words, face id, local face, caller tet id of the record)"""
    h = tr.build_table(4).numpy().view(np.uint32).reshape(-1, 12)
    orig = tr.build_table(2).numpy().view(np.uint32).reshape(-1, 16)[:, 8]
    rows = np.concatenate([h[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 11]], orig[4 * h[:, 7].astype(np.int64)][:, None]], 1)
    return {tuple(int(v) for v in row) for row in rows}


def _check_bvh(tr, F, leaf_width=16):
    """tests/test_build_gpu.py::_check_bvh: every face in exactly one leaf, every slot's box tight, references valid"""
    child = tr.build_table(5).numpy().view(np.uint32).reshape(-1, 64)
    boxes = tr.build_table(6).numpy().view(np.float32).reshape(-1, 6, 64)
    leaf_id = tr.build_table(7).numpy().view(np.uint32).reshape(-1, leaf_width)
    leaf_tri = tr.build_table(8).numpy().view(np.float32).reshape(-1, 9, leaf_width)
    n_nodes, n_leaves = child.shape[0], leaf_id.shape[0]
    ids = leaf_id[leaf_id != 0xFFFFFFFF]
    assert len(ids) == F and len(np.unique(ids)) == F, "every face must sit in exactly one leaf"
    seen_nodes, seen_leaves = np.zeros(n_nodes, bool), np.zeros(n_leaves, bool)
    seen_nodes[0] = True
    for w in range(n_nodes):
        for i in range(64):
            ch = int(child[w, i])
            if ch == 0xFFFFFFFF:
                assert boxes[w, 0, i] == np.inf and boxes[w, 3, i] == -np.inf
                continue
            lo, hi = boxes[w, :3, i], boxes[w, 3:, i]
            if ch >> 31:
                l = ch & 0x7FFFFFFF
                assert l < n_leaves and not seen_leaves[l]
                seen_leaves[l] = True
                m = leaf_id[l] != 0xFFFFFFFF
                tri = leaf_tri[l][:, m].reshape(3, 3, -1)      # [vertex, axis, face]
                assert np.all(tri.min(axis=0).min(axis=1) == lo) and np.all(tri.max(axis=0).max(axis=1) == hi)
            else:
                assert w < ch < n_nodes and not seen_nodes[ch], "children must have larger indices than their parent"
                seen_nodes[ch] = True
                m = child[ch] != 0xFFFFFFFF
                assert np.all(boxes[ch, :3][:, m].min(axis=1) == lo) and np.all(boxes[ch, 3:][:, m].max(axis=1) == hi)
    assert seen_nodes.all() and seen_leaves.all()


def _tables(tr, which=(0, 1, 2, 3, 4, 5, 6, 7, 8)):
    return {w: tr.build_table(w).numpy().copy() for w in which}


@pytest.mark.parametrize("mesh", MESHES)
def test_refit_tables(tn, device, scenes, mesh):
    a, b, cells = _case(scenes, mesh)
    ta, tb = _dev(a, device), _dev(b, device)
    tr = _tracer(tn, device, a, cells, True)
    first = _tables(tr)
    first_records = _records(tr)
    tr.update_vertices(ta.clone())                         # the vertices of the load: no byte changes
    for w, t in _tables(tr).items():
        assert np.array_equal(t, first[w]), f"{mesh}: table {w} changed in a refit to the loaded vertices"
    tr.update_vertices(tb)
    fresh = _tracer(tn, device, b, cells)
    got, want = _records(tr), _records(fresh)
    # geometry: a fresh build's bytes at the same (caller tet id, entry face); topology: untouched
    assert np.array_equal(got[:, _PN], want[:, _PN]), f"{mesh}: pn"
    assert np.array_equal(got[:, _CODE_HI] & _THIN, want[:, _CODE_HI] & _THIN), f"{mesh}: thin exponent"
    assert np.array_equal(_topology(got), _topology(first_records)), f"{mesh}: a topological field of a walk record changed"
    assert not np.array_equal(got[:, _PN], first_records[:, _PN])
    assert _hull_set(tr) == _hull_set(fresh), f"{mesh}: hull triangles"
    now = _tables(tr, (0, 1, 5, 7))
    for w in (0, 1, 5, 7):                                 # faces, face_tets, BVH child rows, leaf ids
        assert np.array_equal(now[w], first[w]), f"{mesh}: table {w} is topological and changed"
    _check_bvh(tr, len(first[1]) // 8)
    tr.update_vertices(ta)                                 # round trip
    for w, t in _tables(tr).items():
        assert np.array_equal(t, first[w]), f"{mesh}: table {w} differs from the first load after the round trip"


# ---------------------------------------------------------------------------------------------------------------- cached scalars
def test_refit_refreshes_cached_scalars(tn, device, scenes):
    ray_order = importlib.import_module("tetra-nerf_amd.ray_order")
    a, b, cells = _case(scenes, "random_1500")
    tr, fresh = _refitted(tn, device, a, b, cells), _tracer(tn, device, b, cells)
    # the key box of a binned call: B's, not A's (the affine map moved the mesh out of A's box)
    o, d, to, td = _rays(scenes, device, 16384, 50)
    plain = _trace(tr, to, td)
    binned = _trace(tr, to, td, bin_rays=True)
    order = tr.ray_order()
    _assert_same_rows(binned, plain, "binned vs unbinned after the refit")
    used = b[np.unique(cells)]
    want = np.argsort(ray_order.ray_keys(o, d, used.min(0), used.max(0)), kind="stable")
    assert np.array_equal(order, want), "ray_order() after the refit is not the order of B's box"
    assert not np.array_equal(want, np.argsort(ray_order.ray_keys(o, d, a.min(0), a.max(0)), kind="stable"))
    # point location and the all-triangles trace
    pos = _dev(refit_cases.affine(0.1 + 0.8 * np.random.default_rng(51).random((4000, 3))), device)
    _assert_same_rows(tr.find_tetrahedra(pos), fresh.find_tetrahedra(pos), "find_tetrahedra")
    assert float(tr.find_tetrahedra(pos)["valid_mask"].float().mean()) > 0.9
    _assert_same_rows(tr.trace_rays_triangles(to[:2000], td[:2000], M), fresh.trace_rays_triangles(to[:2000], td[:2000], M),
                      "trace_rays_triangles")
    # max |coordinate| (the pad of the BVH boxes): loaded near the origin, refitted far away
    far = (1000.0 * a.astype(np.float64) + 5000.0).astype(np.float32)
    tr2, fresh2 = _refitted(tn, device, a, far, cells), _tracer(tn, device, far, cells)
    o1, d1 = scenes.outside_in_rays(3000, 52)
    to2, td2 = _dev((1000.0 * o1.astype(np.float64) + 5000.0).astype(np.float32), device), _dev(d1, device)
    for walk in (0, 2):
        got = _trace(tr2, to2, td2, walk)
        _assert_same_rows(got, _trace(fresh2, to2, td2, walk), f"mesh moved to 1000 x + 5000, walk={walk}")
        assert int(got["num_visited_cells"].sum()) > 10 * 3000


def test_refit_keeps_the_field_cache_and_borrows_the_new_buffer(tn, device, scenes, monkeypatch):
    import torch

    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    a, b, cells = _case(scenes, "random_1500")
    _, _, to, td = _rays(scenes, device, 3000, 54)
    fresh = _tracer(tn, device, b, cells)
    want = {w: _trace(fresh, to, td, w) for w in (0, 2)}
    calls = []
    old, xyz = _dev(a, device), _dev(a, device)
    tr, tr2 = tn.TetrahedraTracer(device), tn.TetrahedraTracer(device)
    tr.load_tetrahedra(old, _dev(cells, device), refittable=True)
    tr2.load_tetrahedra(xyz, _dev(cells, device), refittable=True)
    monkeypatch.setattr(ext, "invalidate_field_cache", lambda *args, **kw: calls.append(args))
    new = _dev(b, device)
    tr.update_vertices(new)
    assert tr.tetrahedra_vertices is new and calls == []
    del old                                               # the first buffer is no longer borrowed
    torch.cuda.empty_cache()
    junk = torch.full((len(a), 3), float("nan"), device=device)     # (likely the freed block)
    for w in (0, 2):
        _assert_same_rows(_trace(tr, to, td, w), want[w], f"after freeing the loaded buffer, walk={w}")
    del junk
    # in place: the loaded tensor itself moves
    xyz.add_(_dev(b, device) - xyz)
    xyz.copy_(_dev(b, device))                            # (exactly B, whatever the rounding of the sum above)
    tr2.update_vertices(xyz)
    for w in (0, 2):
        _assert_same_rows(_trace(tr2, to, td, w), want[w], f"in-place move + update_vertices, walk={w}")
    assert calls == []


def test_refit_errors(tn, device, scenes):
    a, b, cells = _case(scenes, "random_1500")
    _, _, to, td = _rays(scenes, device, 3000, 56)
    ta, tb, tc = _dev(a, device), _dev(b, device), _dev(cells, device)
    o1, d1 = scenes.outside_in_rays(2000, 57)
    to1, td1 = _dev(o1, device), _dev(d1, device)
    tr = tn.TetrahedraTracer(device)
    with pytest.raises(RuntimeError, match="no mesh is loaded"):
        tr.update_vertices(tb)
    tr.load_tetrahedra(ta, tc, refittable=True)
    want = {w: _trace(tr, to1, td1, w) for w in (0, 2)}

    def still_traces_a(t, ctx):
        for w in (0, 2):
            _assert_same_rows(_trace(t, to1, td1, w), want[w], f"after the refused refit ({ctx}), walk={w}")
        assert t.tetrahedra_vertices is ta

    with pytest.raises(RuntimeError, match="the loaded mesh has"):
        tr.update_vertices(tb[:-1].contiguous())
    still_traces_a(tr, "V mismatch")
    with pytest.raises(RuntimeError, match="float32"):
        tr.update_vertices(tb.double())
    still_traces_a(tr, "dtype")
    assert tr._lib.tn_update_vertices(tr._h, len(a), None, None) != 0 and b"null" in tr._lib.tn_last_error()
    still_traces_a(tr, "null xyz")
    plain = tn.TetrahedraTracer(device)
    plain.load_tetrahedra(ta, tc)
    with pytest.raises(RuntimeError, match="refit_tables"):
        plain.update_vertices(tb)
    still_traces_a(plain, "loaded without the option")
    host = tn.TetrahedraTracer(device)
    host.set_option("gpu_build", 0)
    host.load_tetrahedra(ta, tc, refittable=True)
    with pytest.raises(RuntimeError, match="gpu_build"):
        host.update_vertices(tb)
    still_traces_a(host, "host build")
    # a refittable load followed by a plain one keeps nothing
    tr.load_tetrahedra(ta, tc)
    with pytest.raises(RuntimeError, match="refit_tables"):
        tr.update_vertices(tb)


def test_default_load_keeps_nothing(tn, device, scenes):
    a, b, cells = _case(scenes, "random_1500")
    tr = _tracer(tn, device, a, cells)
    assert tr.refit_table_bytes() == 0
    with pytest.raises(RuntimeError, match="refit_tables"):
        tr.update_vertices(_dev(b, device))
    kept = _tracer(tn, device, a, cells, True).refit_table_bytes()
    T = len(cells)
    print(f"refit tables at {T} tets: {kept} bytes = {kept / T:.1f} B per tet")
    assert 0 < kept < 40 * T          # DESIGN.md section 4.10 counts about 29 B per tet


# ---------------------------------------------------------------------------------------------------------------- adapter
def test_adapter_refits_when_the_vertex_version_moves(tn, device, scenes):
    import torch

    standins = importlib.import_module("nerfstudio_standins")
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    a, _, cells = _case(scenes, "random_1500")
    Fused = plugin.make_fused_model_class(standins.StandInTetrahedraNerf)

    def model_of(vertices, **extra):
        torch.manual_seed(0)
        m = Fused(standins.Config(num_samples=64, num_fine_samples=64, max_intersected_triangles=M), torch.from_numpy(vertices),
                  torch.from_numpy(cells)).to(device)
        for k, v in extra.items():
            setattr(m.config, k, v)
        with torch.no_grad():
            m.tetrahedra_field[0] = torch.rand(len(vertices), generator=torch.Generator().manual_seed(1)).to(device) * 6 - 3
        return m.eval()

    calls = []
    real = ext.TetrahedraTracer.update_vertices

    def spy(self, xyz):
        calls.append(self)
        return real(self, xyz)

    o, d = scenes.outside_in_rays(2048, 60)
    rb = standins.RayBundle(_dev(o, device), _dev(d, device))
    model = model_of(a, refit_vertices=True)
    ext.TetrahedraTracer.update_vertices = spy
    try:
        with torch.no_grad():
            before = model.get_outputs(rb)["rgb"].clone()
            assert calls == [] and model._tetrahedra_tracer.refit_table_bytes() > 0
            model.get_outputs(rb)
            assert calls == []                                 # nothing moved: no refit
            # an optimiser step on the vertex table (in place: the version counter moves)
            v = model.tetrahedra_vertices
            hull = torch.from_numpy(refit_cases.hull_vertices(cells)).to(device)
            step = torch.from_numpy((0.1 * refit_cases.star_min_height(a, cells)).astype(np.float32)).to(device)
            step[hull] = 0.0
            g = torch.randn(v.shape, generator=torch.Generator().manual_seed(2)).to(device)
            # (interior vertices by a tenth of their star's height, and the whole mesh shrunk to 0.8 about its centre)
            v.grad = -(g / g.norm(dim=1, keepdim=True)) * step[:, None] + 0.2 * (v - 0.5)
            torch.optim.SGD([v], lr=1.0).step()
            after = model.get_outputs(rb)["rgb"].clone()
            assert len(calls) == 1
            model.get_outputs(rb)
            assert len(calls) == 1
            reloaded = model_of(v.detach().cpu().numpy())       # a model whose tracer is loaded on the moved vertices
            want = reloaded.get_outputs(rb)["rgb"]
            assert torch.equal(after, want), float((after - want).abs().max())
            assert float((after - before).abs().max()) > 1e-3      # (a tracer left on the old vertices shows)
            # without the flag: today's route, the tracer is never refitted
            plain = model_of(a)
            plain.get_outputs(rb)
            plain.tetrahedra_vertices.add_(0.0)
            plain.get_outputs(rb)
            assert len(calls) == 1 and plain._tetrahedra_tracer.refit_table_bytes() == 0
    finally:
        ext.TetrahedraTracer.update_vertices = real


# ---------------------------------------------------------------------------------------------------------------- cost
def test_refit_is_not_slower_than_load(tn, device, scenes):
    """A floor, not the claim (profiles/refit_bench.txt is): the refit launches a strict subset of the load's work."""
    import time
    import torch

    pts, cells = scenes.random_mesh(15000, 0)
    x, c = _dev(pts, device), _dev(cells, device)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(x, c, refittable=True)              # warm-up of both
    tr.update_vertices(x)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    loads = [timed(lambda: tr.load_tetrahedra(x, c, refittable=True)) for _ in range(3)]
    refits = [timed(lambda: tr.update_vertices(x)) for _ in range(5)]
    print(f"{len(cells)} tets: load_tetrahedra {np.median(loads) * 1e3:.2f} ms, update_vertices {np.median(refits) * 1e3:.2f} ms")
    assert np.median(refits) < np.median(loads), (refits, loads)
