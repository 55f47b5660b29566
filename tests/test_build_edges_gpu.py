"""The device build (csrc/tn_build.hip) and the refit (csrc/tn_refit.hip) at their size edges, on the GPU.

The cases are those of tests/build_edge_cases.py: tet counts on the block, wave and grid-cap edges of the kernels (1 ... 2,387
tets, and 65,535 / 65,536 / 65,537 tets around the 1024 x 256 lanes of k_refit_records), face counts below and just above every
leaf width, meshes with unreferenced and NaN vertices.  tests/test_build_edge_cases.py asserts on the CPU that the oracle reports
hits on the rays used here and which size classes the cases meet.

Bars: the tables of the device build are the host build's bytes; the face BVH of either build is the median-split tree
(`check_median_splits`), not just a valid one; every query equals the oracle bit for bit; a refitted tracer holds a fresh
load's geometry in EVERY record, also those only the second grid-stride trip of k_refit_records writes, and the scalars that
trip reduces (max |coordinate|, the mesh box) are a fresh load's."""
import importlib

import numpy as np
import pytest

import build_edge_cases as bec
from test_build_gpu import KEYS, _check_bvh
from test_refit_gpu import _CODE_HI, _PN, _THIN, _assert_same_rows, _dev, _hull_set, _records, _tables, _topology

pytestmark = pytest.mark.gpu

N_RAYS, M = 512, 64
_ORACLES = {}


def _tracer(tn, device, pts, cells, refittable=False, **options):
    tr = tn.TetrahedraTracer(device)
    for k, v in options.items():
        tr.set_option(k, v)
    tr.load_tetrahedra(_dev(pts, device), _dev(cells, device), refittable=refittable)
    return tr


def _oracle(oracle, name, pts, cells):
    if name not in _ORACLES:
        ot = oracle.OracleTracer(use_bvh=True)
        ot.load_tetrahedra(pts, cells)
        _ORACLES[name] = ot
    return _ORACLES[name]


def _trace(tr, to, td, walk=None, **kw):
    if walk is not None:
        tr.set_option("walk", walk)
    out = tr.trace_rays(to, td, M, **kw)
    if walk is not None:
        tr.set_option("walk", 1)
    return out


def _assert_oracle_rows(got, want, ctx, rows=None):
    for k in KEYS:
        g, w = got[k].cpu().numpy(), np.ascontiguousarray(want[k])
        if rows is not None:
            g = g[rows]
        g, w = np.ascontiguousarray(g).view(np.uint32), w.view(np.uint32)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
            raise AssertionError(f"{ctx}: {k} differs from the oracle on {len(bad)} rows (first: {bad[:4]})")


def _rays(scenes, pts, cells, n=N_RAYS, seed=70):
    """the aimed rays of the case plus 256 rays of the unit cube's surroundings"""
    o, d = bec.aimed_rays(pts, cells, n, seed)
    o2, d2 = scenes.outside_in_rays(256, seed + 1)
    return np.concatenate([o, o2]), np.concatenate([d, d2])


# ---------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("leaf_width", bec.LEAF_WIDTHS)
@pytest.mark.parametrize("name", bec.NAMES)
def test_tables_device_vs_host(tn, device, scenes, name, leaf_width):
    pts, cells = bec.cases(scenes)[name]
    host = _tracer(tn, device, pts, cells, gpu_build=0, leaf_width=leaf_width)
    dev = _tracer(tn, device, pts, cells, gpu_build=1, leaf_width=leaf_width)
    for which, what in ((0, "faces"), (1, "face_tets"), (2, "walk records"), (3, "hull nodes"), (4, "hull triangles")):
        a, b = host.build_table(which).numpy(), dev.build_table(which).numpy()
        assert a.shape == b.shape, f"{name}: {what} size {a.shape} vs {b.shape}"
        diff = np.nonzero(a != b)[0]
        assert len(diff) == 0, f"{name}: {what} differ at byte {diff[:4]} ({len(diff)} bytes)"
    F, hull = bec.face_counts(cells)
    assert dev.build_table(1).numel() // 8 == F
    faces = dev.build_table(0).numpy().view(np.uint32).reshape(-1, 3)
    for tr, who in ((dev, "device"), (host, "host")):
        _check_bvh(tr, F, leaf_width)
        leaf_id = tr.build_table(7).numpy().view(np.uint32).reshape(-1, leaf_width)
        # (the host build's leaf rows are in position order too: final_face_order)
        assert bec.check_median_splits(faces, leaf_id, pts, leaf_width) == len(leaf_id) - 1, who
        assert len(leaf_id) == len(bec.leaf_counts(F, leaf_width))
    print(f"{name} leaf width {leaf_width}: T {len(cells)} F {F} hull {hull} leaves {len(leaf_id)} wide nodes "
          f"{dev.build_table(5).numel() // 256} in {bec.wide_levels(dev.build_table(5).numpy().view(np.uint32))} level(s)")


# ---------------------------------------------------------------------------------------------------------------- traces
@pytest.mark.parametrize("name", bec.SMALL)
def test_traces_equal_the_oracle(tn, device, oracle, scenes, name):
    pts, cells = bec.cases(scenes)[name]
    ot = _oracle(oracle, name, pts, cells)
    tr = _tracer(tn, device, pts, cells)
    o, d = _rays(scenes, pts, cells)
    to, td = _dev(o, device), _dev(d, device)
    want = ot.trace_rays(o, d, M)
    for walk in (0, 2):
        _assert_oracle_rows(_trace(tr, to, td, walk), want, f"{name}: walk={walk}")
    # the default dispatch at a size that takes the walk schedule
    o, d = bec.aimed_rays(pts, cells, 16384, 72)
    to, td = _dev(o, device), _dev(d, device)
    big = _trace(tr, to, td)
    _assert_oracle_rows(big, ot.trace_rays(o[::16], d[::16], M), f"{name}: default dispatch", slice(None, None, 16))
    _assert_same_rows(big, _trace(tr, to, td, 0), f"{name}: default dispatch vs the BVH path")


@pytest.mark.parametrize("name", bec.SMALL)
def test_locate_and_triangles_equal_the_oracle(tn, device, oracle, scenes, name):
    pts, cells = bec.cases(scenes)[name]
    ot = _oracle(oracle, name, pts, cells)
    tr = _tracer(tn, device, pts, cells)
    q = bec.locate_points(pts, cells, 2000, 74)
    want = ot.find_tetrahedra(q)
    got = {k: v.cpu().numpy() for k, v in tr.find_tetrahedra(_dev(q, device)).items()}
    np.testing.assert_array_equal(got["tetrahedra"], want["tetrahedra"])
    np.testing.assert_array_equal(got["vertex_indices"], want["vertex_indices"])
    np.testing.assert_array_equal(got["barycentric_coordinates"].view(np.uint32), want["barycentric_coordinates"].view(np.uint32))
    np.testing.assert_array_equal(got["valid_mask"], want["valid_mask"])
    if name != "flat":
        assert got["valid_mask"].any()
    o, d = bec.aimed_rays(pts, cells, N_RAYS, 70)
    want = ot.trace_rays_triangles(o, d, M)
    got = {k: v.cpu().numpy() for k, v in tr.trace_rays_triangles(_dev(o, device), _dev(d, device), M).items()}
    for k in ("num_visited_triangles", "visited_triangles", "vertex_indices"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("barycentric_coordinates", "hit_distances"):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- refit
def _moved_rays(a, cells, device, n=N_RAYS, seed=76):
    """the aimed rays of the loaded mesh, moved with it by the affine map of the move"""
    o, d = bec.aimed_rays(a, cells, n, seed)
    o, d = bec.affine(o), bec.affine_dirs(d)
    return o, d, _dev(o, device), _dev(d, device)


def _compare_tracers(tr, fresh, to, td, ctx, walked):
    """tests/test_refit_gpu.py::_compare_tracers on given rays"""
    bvh = _trace(tr, to, td, 0)
    _assert_same_rows(bvh, _trace(fresh, to, td, 0), f"{ctx}: BVH path, refitted vs fresh")
    walk = _trace(tr, to, td, 2)
    assert tr.trace_stats()["walk"] > 0 or not walked
    _assert_same_rows(walk, _trace(fresh, to, td, 2), f"{ctx}: walk, refitted vs fresh")
    _assert_same_rows(walk, bvh, f"{ctx}: walk vs BVH path on the refitted tracer")
    return bvh


@pytest.mark.parametrize("name", bec.NAMES)
def test_refit_equals_fresh_load(tn, device, scenes, name):
    """the assertions of tests/test_refit_gpu.py::test_refit_tables and ::_compare_tracers; `_records` compares every record,
    so on the stride cases also those at indices >= 262,144"""
    a, b, cells = bec.case_ab(scenes, name)
    ta, tb = _dev(a, device), _dev(b, device)
    tr = _tracer(tn, device, a, cells, True)
    first = _tables(tr)
    first_records = _records(tr)
    assert len(first_records) == 4 * len(cells)
    tr.update_vertices(tb)
    fresh = _tracer(tn, device, b, cells)
    got, want = _records(tr), _records(fresh)
    assert np.array_equal(got[:, _PN], want[:, _PN]), f"{name}: pn"
    assert np.array_equal(got[:, _CODE_HI] & _THIN, want[:, _CODE_HI] & _THIN), f"{name}: thin exponent"
    assert np.array_equal(_topology(got), _topology(first_records)), f"{name}: a topological field of a walk record changed"
    assert not np.array_equal(got[:, _PN], first_records[:, _PN])
    assert _hull_set(tr) == _hull_set(fresh), f"{name}: hull triangles"
    now = _tables(tr, (0, 1, 5, 7))
    for w in (0, 1, 5, 7):
        assert np.array_equal(now[w], first[w]), f"{name}: table {w} is topological and changed"
    _check_bvh(tr, len(first[1]) // 8)
    _, _, to, td = _moved_rays(a, cells, device)
    rows = _compare_tracers(tr, fresh, to, td, name, walked=len(cells) > 2000)
    if name != "flat":
        assert float((rows["num_visited_cells"] > 0).float().mean()) >= 0.8     # (the oracle's share on the loaded mesh: >= 0.9)
    tr.update_vertices(ta)
    for w, t in _tables(tr).items():
        assert np.array_equal(t, first[w]), f"{name}: table {w} differs from the first load after the round trip"


def _check_scalars(tn, device, a, b, cells, ctx):
    """what tests/test_refit_gpu.py::test_refit_refreshes_cached_scalars checks, on the aimed rays: the key box of a binned call
    is the box of the referenced, moved vertices; max |coordinate| after a refit far away is a fresh load's"""
    ray_order = importlib.import_module("tetra-nerf_amd.ray_order")
    tr = _tracer(tn, device, a, cells, True)
    tr.update_vertices(_dev(b, device))
    o, d, to, td = _moved_rays(a, cells, device, 16384, 78)
    plain = _trace(tr, to, td)
    assert tr.trace_stats()["walk"] > 0
    binned = _trace(tr, to, td, bin_rays=True)
    order = tr.ray_order()
    _assert_same_rows(binned, plain, f"{ctx}: binned vs unbinned after the refit")
    lo, hi = bec.ref_box(b, cells)
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
    want = np.argsort(ray_order.ray_keys(o, d, lo, hi), kind="stable")
    assert len(order) == len(want) and np.array_equal(order, want), f"{ctx}: ray_order() after the refit is not the order of B's box"
    lo_a, hi_a = bec.ref_box(a, cells)
    assert not np.array_equal(want, np.argsort(ray_order.ray_keys(o, d, lo_a, hi_a), kind="stable"))
    # max |coordinate| (the pad of the BVH boxes): loaded near the origin, refitted far away
    far = (1000.0 * a.astype(np.float64) + 5000.0).astype(np.float32)
    tr.update_vertices(_dev(far, device))
    fresh = _tracer(tn, device, far, cells)
    o1, d1 = bec.aimed_rays(a, cells, N_RAYS, 80)
    to2, td2 = _dev((1000.0 * o1.astype(np.float64) + 5000.0).astype(np.float32), device), _dev(d1, device)
    for walk in (0, 2):
        got = _trace(tr, to2, td2, walk)
        _assert_same_rows(got, _trace(fresh, to2, td2, walk), f"{ctx}: mesh moved to 1000 x + 5000, walk={walk}")
        assert float((got["num_visited_cells"] > 0).float().mean()) >= 0.8
    return tr


@pytest.mark.parametrize("name", bec.STRIDE)
def test_refit_scalars_at_the_grid_cap(tn, device, scenes, name):
    a, b, cells = bec.case_ab(scenes, name)
    _check_scalars(tn, device, a, b, cells, name)


def test_refit_reductions_from_the_second_trip_alone(tn, device, scenes):
    """stride_tail: the four records the second grid-stride trip of k_refit_records writes belong to the one tetrahedron that
    holds max |coordinate| and spans the mesh box after the move, so a reduction value lost on that trip (or a wrong stride, or a
    wrong order[i >> 2] there) changes scene_max and the box.  Which records those are is read from the tet-id word of table 2."""
    a, b, cells = bec.case_ab(scenes, "stride_tail")
    tr = _tracer(tn, device, a, cells, True)
    raw = tr.build_table(2).numpy().view(np.uint32).reshape(-1, 16)
    assert len(raw) == bec.REFIT_GRID_LANES + 4
    assert raw[bec.REFIT_GRID_LANES:, 8].tolist() == [len(cells) - 1] * 4, "the added tetrahedron is not the last of the kept order"
    tail = cells[-1]
    q = b[bec.referenced(cells)]
    for k in range(3):
        assert q[:, k].min() in b[tail, k] and q[:, k].max() in b[tail, k]
    assert np.abs(q).max() == np.abs(b[tail]).max()
    tr.update_vertices(_dev(b, device))
    fresh = _tracer(tn, device, b, cells)
    got, want = _records(tr), _records(fresh)
    # (sorted by tet id: the last four rows are the added tetrahedron's; pn of entry face e is the vertex opposite e)
    assert {tuple(r) for r in got[-4:, _PN].view(np.float32).tolist()} == {tuple(r) for r in b[tail].tolist()}
    assert np.array_equal(got[:, _PN], want[:, _PN]) and np.array_equal(got[:, _CODE_HI] & _THIN, want[:, _CODE_HI] & _THIN)
    # scene_max: the pad of the BVH boxes (the BVH path and the walk's fallbacks), the box: the keys of a binned call
    ray_order = importlib.import_module("tetra-nerf_amd.ray_order")
    o, d = bec.aimed_rays(b, cells, 16384, 82)
    to, td = _dev(o, device), _dev(d, device)
    plain = _trace(tr, to, td)
    _assert_same_rows(plain, _trace(fresh, to, td), "stride_tail: default dispatch, refitted vs fresh")
    binned = _trace(tr, to, td, bin_rays=True)
    order = tr.ray_order()
    _assert_same_rows(binned, plain, "stride_tail: binned vs unbinned")
    lo, hi = bec.ref_box(b, cells)
    want_order = np.argsort(ray_order.ray_keys(o, d, lo, hi), kind="stable")
    assert len(order) == len(want_order) and np.array_equal(order, want_order), "ray_order() is not the order of B's box"
    rest = np.setdiff1d(bec.referenced(cells), tail)
    assert not np.array_equal(want_order, np.argsort(ray_order.ray_keys(o, d, b[rest].min(0), b[rest].max(0)), kind="stable"))
    _compare_tracers(tr, fresh, to[:N_RAYS], td[:N_RAYS], "stride_tail", walked=True)


# ---------------------------------------------------------------------------------------------------------------- NaN
def test_nan_in_unreferenced_vertices_changes_nothing(tn, device, scenes):
    """load, trace, binned call, refit and far refit of `nan_unused` against the same mesh with the unreferenced vertices at 0:
    bit-equal rows and the same binned order, which is numpy's over the box of the referenced vertices (so max |coordinate| and
    the box are finite: _check_scalars)"""
    a, b, cells = bec.case_ab(scenes, "nan_unused")
    un = bec.unreferenced(a, cells)
    assert len(un) and np.isnan(a[un]).all() and np.isnan(b[un]).all()
    a0, b0 = bec.zeroed_unused(a, cells), bec.zeroed_unused(b, cells)
    o, d = _rays(scenes, a, cells)
    to, td = _dev(o, device), _dev(d, device)
    tr, tr0 = _tracer(tn, device, a, cells, True), _tracer(tn, device, a0, cells, True)
    for w in range(9):
        assert np.array_equal(tr.build_table(w).numpy(), tr0.build_table(w).numpy()), f"table {w} depends on an unreferenced vertex"
    for walk in (0, 2):
        _assert_same_rows(_trace(tr, to, td, walk), _trace(tr0, to, td, walk), f"nan_unused: loaded, walk={walk}")
    ob, db = bec.aimed_rays(a, cells, 16384, 84)
    tob, tdb = _dev(ob, device), _dev(db, device)
    x, x0 = _trace(tr, tob, tdb, bin_rays=True), _trace(tr0, tob, tdb, bin_rays=True)
    order, order0 = tr.ray_order(), tr0.ray_order()
    _assert_same_rows(x, x0, "nan_unused: binned call")
    ray_order = importlib.import_module("tetra-nerf_amd.ray_order")
    lo, hi = bec.ref_box(a, cells)
    want = np.argsort(ray_order.ray_keys(ob, db, lo, hi), kind="stable")
    assert len(order) == len(want) and np.array_equal(order, want) and np.array_equal(order0, want)
    tr.update_vertices(_dev(b, device)); tr0.update_vertices(_dev(b0, device))
    for w in range(9):
        assert np.array_equal(tr.build_table(w).numpy(), tr0.build_table(w).numpy()), f"refitted table {w} depends on an unreferenced vertex"
    _, _, tom, tdm = _moved_rays(a, cells, device)
    for walk in (0, 2):
        _assert_same_rows(_trace(tr, tom, tdm, walk), _trace(tr0, tom, tdm, walk), f"nan_unused: refitted, walk={walk}")
    _check_scalars(tn, device, a, b, cells, "nan_unused")


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("gpu_build", (0, 1))
def test_zero_cells_are_refused(tn, device, oracle, scenes, gpu_build):
    """tn_load_tetrahedra refuses a mesh without cells ahead of its first allocation and launch, whichever build is selected; the
    tracer loads and traces a mesh afterwards"""
    import torch

    pts, cells = bec.cases(scenes)["single"]
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    with pytest.raises(RuntimeError, match="at least one tetrahedron"):
        tr.load_tetrahedra(_dev(pts, device), torch.zeros((0, 4), dtype=torch.int32, device=device))
    tr.load_tetrahedra(_dev(pts, device), _dev(cells, device))
    o, d = bec.aimed_rays(pts, cells, N_RAYS, 70)
    got = tr.trace_rays(_dev(o, device), _dev(d, device), M)
    _assert_oracle_rows(got, _oracle(oracle, "single", pts, cells).trace_rays(o, d, M), f"single after the refusal, gpu_build={gpu_build}")
    assert float((got["num_visited_cells"] > 0).float().mean()) >= 0.9
