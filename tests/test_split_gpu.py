"""The tetrahedron split on the GPU (tn_split_count / tn_split_emit / tn_split_vertex_rows, csrc/tn_split.hip; cpp.split_tetrahedra,
cpp.split_vertex_rows, TetrahedraTracer.split_tetrahedra, nerfstudio_plugin.densify).

Bar: on every case of tests/split_cases.py -- the stock scenes and the cube soups at every wave, block and grid-cap edge -- the
four arrays, the offsets and the counters equal the numpy statement (geometry.split_tetrahedra_statement) byte for byte; the grown
per-vertex arrays equal geometry.split_vertex_rows_statement byte for byte at every alignment of the two strides, with and without
the shadow on either side; a tracer loaded with the split mesh traces as the oracle loaded with it does, and hits the rays the
unsplit mesh hit; the field gathered through the real path on the split mesh stays within 8 x the unsplit mesh's own error
against the float64 parent interpolant; and the adapter's model trains on."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import split_cases as sc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import reference_model as rm   # noqa: E402

KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")
M_TRACE = 512


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.array(x)).to(device)   # (the cases are read-only: a copy)


def _lib():
    return importlib.import_module("tetra-nerf_amd._lib").load()


def _entries(device, xyz, cells, select):
    """the two entries called directly (the wrapper does not call the second one when nothing is accepted), outputs pre-filled"""
    lib = _lib()
    V, T = len(xyz), len(cells)
    x, c, s = _dev(xyz, device), _dev(cells, device), _dev(select, device)
    fill = lambda *shape, dtype=torch.int32: torch.full(shape, 0x7F7F7F7F if dtype == torch.int32 else float("nan"), dtype=dtype, device=device)   # noqa: E731
    offsets, counters = fill(T + 1), fill(4)
    assert lib.tn_split_count(V, T, x.data_ptr(), c.data_ptr(), s.data_ptr(), offsets.data_ptr(), counters.data_ptr(), None) == 0, lib.tn_last_error()
    K = int(offsets[T].item())
    vertices, new_cells = fill(V + K, 3, dtype=torch.float32), fill(T + 3 * K, 4)
    cell_parent, vertex_parents = fill(T + 3 * K), fill(K, 4)
    assert lib.tn_split_emit(V, T, x.data_ptr(), c.data_ptr(), offsets.data_ptr(), K, vertices.data_ptr(), new_cells.data_ptr(),
                             cell_parent.data_ptr(), vertex_parents.data_ptr(), None) == 0, lib.tn_last_error()
    return {"vertices": vertices, "cells": new_cells, "cell_parent": cell_parent, "vertex_parents": vertex_parents, "offsets": offsets,
            "counters": counters, "num_new": K}


def _compare(got, want, what, keys=sc.ARRAYS):
    assert got["num_new"] == want["num_new"], (what, got["num_new"], want["num_new"])
    for key in keys:
        g = got[key].cpu().numpy()
        assert got[key].is_cuda and g.shape == want[key].shape, (what, key, g.shape, want[key].shape)
        bad = np.nonzero(sc.bits(g).view(np.uint32).reshape(-1) != sc.bits(want[key]).view(np.uint32).reshape(-1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {want[key].size} words of {key} differ (first: {bad[:1]})"


@pytest.mark.parametrize("name", sc.names(soups=True))
def test_kernels_equal_the_statement(tn, device, scenes, name):
    xyz, cells, select = sc.case(scenes, name)
    want = sc.statement(scenes, name)
    got = _entries(device, xyz, cells, select)
    print(name, "T", len(cells), "asked", int(select.sum()), "counters", got["counters"].tolist())
    _compare(got, want, name)


def test_wrapper_is_the_entries_and_two_runs_give_the_same_bytes(tn, device, scenes):
    bt, blocks = sc.kernel_constants()
    for name in ("random_300_30pct", "grid_6_all", f"soup_{bt * blocks + 1}_third", "none_asked"):
        xyz, cells, select = sc.case(scenes, name)
        args = _dev(xyz, device), _dev(cells, device), _dev(select, device)
        a, b = tn.cpp.split_tetrahedra(*args), tn.cpp.split_tetrahedra(args[0], args[1], args[2].bool())
        keys = tuple(k for k in sc.ARRAYS if k != "offsets")
        _compare(a, sc.statement(scenes, name), name, keys)
        for key in keys:
            assert a[key].dtype == (torch.float32 if key == "vertices" else torch.int32)
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (name, key)
    assert a["num_new"] == 0 and a["vertices"] is args[0] and a["cells"] is args[1]      # nothing accepted: the inputs themselves


def test_refused_and_short_calls_touch_nothing_they_do_not_own(tn, device, scenes):
    """a refused call leaves every output as it was; a call told a smaller num_new than was counted -- what a caller who changed
    the inputs between the two entries amounts to -- writes nothing behind it"""
    lib = _lib()
    xyz, cells, select = sc.case(scenes, "random_300_30pct")
    want = sc.statement(scenes, "random_300_30pct")
    V, T, K = len(xyz), len(cells), want["num_new"]
    x, c, s = _dev(xyz, device), _dev(cells, device), _dev(select, device)
    p = lambda t: t.data_ptr()   # noqa: E731
    seven = lambda *shape, dtype=torch.int32: torch.full(shape, 7, dtype=dtype, device=device)   # noqa: E731
    offsets, counters = seven(T + 1), seven(4)
    for args in ((V, T, None, p(c), p(s), p(offsets), p(counters)), (V, 2 ** 30, p(x), p(c), p(s), p(offsets), p(counters)),
                 (V, T, p(x), p(c), p(s), None, p(counters)), (2 ** 32 - 1, T, p(x), p(c), p(s), p(offsets), p(counters))):
        assert lib.tn_split_count(*args, None) != 0
    torch.cuda.synchronize()
    assert bool((offsets == 7).all()) and bool((counters == 7).all())
    assert lib.tn_split_count(V, T, p(x), p(c), p(s), p(offsets), p(counters), None) == 0
    assert offsets.tolist() == want["offsets"].tolist() and counters.tolist() == want["counters"].tolist()
    short = K - 5
    vertices, new_cells = seven(V + K, 3, dtype=torch.float32), seven(T + 3 * K, 4)
    parent, vp = seven(T + 3 * K), seven(K, 4)
    outs = (p(vertices), p(new_cells), p(parent), p(vp))
    assert lib.tn_split_emit(V, T, p(x), p(c), p(offsets), T + 1, *outs, None) != 0
    assert lib.tn_split_emit(V, T, p(x), None, p(offsets), K, *outs, None) != 0
    torch.cuda.synchronize()
    for t in (vertices, new_cells, parent, vp):
        assert bool((t == 7).all())
    assert lib.tn_split_emit(V, T, p(x), p(c), p(offsets), short, *outs, None) == 0
    torch.cuda.synchronize()
    assert bool((vertices[V + short:] == 7).all()) and bool((new_cells[T + 3 * short:] == 7).all())
    assert bool((parent[T + 3 * short:] == 7).all()) and bool((vp[short:] == 7).all())
    assert np.array_equal(vertices[:V + short].cpu().numpy().view(np.uint32), want["vertices"][:V + short].view(np.uint32))
    assert np.array_equal(vp[:short].cpu().numpy(), want["vertex_parents"][:short])


# ------------------------------------------------------------------------------------------------------- the per-vertex arrays
# every (V mod 4, (V + K) mod 4) at V ~ 260; K = 0, 1, 65; V = 64 +- 1 (one tile of the new-column kernel, one 16-byte chunk more
# or less per row) and 65,536 + 1
SHAPES = [(V, K) for V in (260, 261, 262, 263) for K in (64, 65, 66, 67)] + \
         [(260, 0), (261, 1), (262, 65), (63, 1), (63, 65), (64, 65), (65, 1), (65, 65), (65537, 65), (65537, 0)]


def _parents(V, K, seed):
    rng = np.random.default_rng(seed)
    vp = rng.integers(0, V, (K, 4)).astype(np.int32)
    if K >= 2:
        vp[K // 2, 2] = V                                                     # an id past the table: that column is 0
    if K >= 3:
        vp[0] = [V - 1, 0, V - 1, 0]                                          # the two ends of a row
    return vp


@pytest.mark.parametrize("rows", (1, 3, 64))
@pytest.mark.parametrize("V,K", SHAPES)
def test_vertex_rows_equal_the_statement(tn, device, V, K, rows):
    g = sc.geometry()
    assert {(v % 4, (v + k) % 4) for v, k in SHAPES} == {(a, b) for a in range(4) for b in range(4)}
    vp = _parents(V, K, 100 * V + K)
    for integers in (False, True):
        values = sc.values_for(V, rows, seed=V + K, integers=integers)
        v, par = _dev(values, device), _dev(vp, device)
        vm = v.t().contiguous()
        for mode in ("mean", "zero"):
            want = g.split_vertex_rows_statement(values, vp, new=mode)
            for values_vm in (None, vm):
                for want_vm in (False, True):
                    got = tn.cpp.split_vertex_rows(v, par, new=mode, values_vm=values_vm, want_vertex_major=want_vm)
                    out, out_vm = got if want_vm else (got, None)
                    what = (V, K, rows, mode, values_vm is not None, want_vm, integers)
                    assert tuple(out.shape) == (rows, V + K) and np.array_equal(sc.bits(out.cpu().numpy()), sc.bits(want)), what
                    if want_vm:
                        assert tuple(out_vm.shape) == (V + K, rows)
                        assert torch.equal(out_vm.view(torch.int32), tn.cpp._transpose_field(out).view(torch.int32)), what
            if mode == "zero":
                assert not want[:, V:].any()
        if integers and K:                                                    # sums of four small integers and their quarters are exact
            ok = (vp < V).all(1)
            exact = np.where(ok, values.astype(np.float64)[:, np.where(vp < V, vp, 0)].sum(2) / 4, 0)
            assert np.array_equal(g.split_vertex_rows_statement(values, vp)[:, V:].astype(np.float64), exact)


def test_vertex_rows_on_a_misaligned_output(tn, device):
    """an output that is not 16-byte aligned takes the element-wise stores; the entry is called directly on a shifted view"""
    lib, g = _lib(), sc.geometry()
    V, K, rows = 261, 66, 3
    values, vp = sc.values_for(V, rows, seed=5), _parents(V, K, 5)
    v, par = _dev(values, device), _dev(vp, device)
    storage = torch.full((rows * (V + K) + 2,), 7.0, device=device)
    out = storage[1:-1]
    assert out.data_ptr() % 16 == 4
    assert lib.tn_split_vertex_rows(rows, V, K, v.data_ptr(), None, par.data_ptr(), 0, out.data_ptr(), None, None) == 0
    assert np.array_equal(sc.bits(out.cpu().numpy().reshape(rows, V + K)), sc.bits(g.split_vertex_rows_statement(values, vp)))
    assert storage[0].item() == 7.0 and storage[-1].item() == 7.0


# ------------------------------------------------------------------------------------------------------------------ the tracer
def _trace(tr, o, d):
    return tr.trace_rays(o, d, M_TRACE)


@pytest.mark.parametrize("name", ("random_300_30pct", "cube_all"))
def test_tracer_split_traces_as_the_oracle_on_the_split_mesh(tn, device, scenes, oracle, name):
    xyz, cells, select = sc.case(scenes, name)
    want = sc.statement(scenes, name)
    V, T, K = len(xyz), len(cells), want["num_new"]
    o, d = scenes.outside_in_rays(2000, 12)
    od = _dev(o, device), _dev(d, device)
    tr = tn.TetrahedraTracer(device)
    assert tr.supports_split
    with pytest.raises(RuntimeError, match="load"):
        tr.split_tetrahedra(_dev(select, device))
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device), refittable=True)
    hit_before = _trace(tr, *od)["num_visited_cells"] > 0
    occ = torch.rand(T, device=device)
    field = _dev(sc.values_for(V, 64, seed=3), device)
    # nothing asked: the tracer is not touched, the inputs come back as they are
    same = tr.split_tetrahedra(torch.zeros(T, dtype=torch.uint8, device=device), vertex_rows=(field,), tet_values=(occ,))
    assert same["num_new"] == 0 and same["vertices"] is tr.tetrahedra_vertices and same["vertex_rows"][0] is field and same["tet_values"][0] is occ
    out = tr.split_tetrahedra(_dev(select, device), vertex_rows=(field,), tet_values=(occ,))
    _compare(out, want, name, tuple(k for k in sc.ARRAYS if k != "offsets"))
    assert tr.tetrahedra_vertices is out["vertices"] and tr.tetrahedra_cells is out["cells"] and tr._refittable
    assert torch.equal(out["tet_values"][0], occ[out["cell_parent"].long()])
    assert np.array_equal(sc.bits(out["vertex_rows"][0].cpu().numpy()),
                          sc.bits(sc.geometry().split_vertex_rows_statement(field.cpu().numpy(), want["vertex_parents"])))
    # the project's standard parity: every row of the five arrays is the oracle's on the same mesh, bit for bit
    got = _trace(tr, *od)
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(want["vertices"], want["cells"])
    ref = ot.trace_rays(o, d, M_TRACE)
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k].cpu().numpy()).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert len(bad) == 0, f"{name}: {k} differs from the oracle on {len(bad)} rows (first: {bad[:4]})"
    assert torch.equal(got["num_visited_cells"] > 0, hit_before) and int(hit_before.sum()) > 1000
    # the monitor runs on the split mesh, and a re-triangulation of its vertices leaves no violated face
    counters = tr.delaunay_check()["counters"].tolist()
    assert counters[0] > 0
    again = tr.retriangulate(tr.tetrahedra_vertices, tet_values=(out["tet_values"][0],))
    after = tr.delaunay_check()["counters"].tolist()
    print(name, "K", K, "delaunay counters of the split mesh", counters, "after retriangulate", after, "T'", again["num_tetrahedra"])
    assert after[1] == 0
    tr.close()


def _midpoint_error(tn, device, tr, o, d, field, parent_of, F0, grad, p0):
    """the largest |gathered feature - float64 parent interpolant| over the midpoints of every traversed segment"""
    od = _dev(o, device), _dev(d, device)
    out = _trace(tr, *od)
    num = out["num_visited_cells"].long()
    S = int(num.max())
    hd = out["hit_distances"][:, :S]
    mid = (0.5 * (hd[..., 0] + hd[..., 1])).contiguous()
    live = torch.arange(S, device=device)[None] < num[:, None]
    mid = torch.where(live, mid, torch.full_like(mid, 1e30)).contiguous()     # behind the last segment: matched by nothing
    inter = tr.find_visited_cells(out["num_visited_cells"], out["visited_cells"], out["barycentric_coordinates"], out["hit_distances"],
                                  out["vertex_indices"], mid)
    feats = tn.interpolate_values(inter["vertex_indices"], inter["barycentric_coordinates"], field)
    mask = (inter["mask"] & live).cpu().numpy()
    cell = inter["cell_indices"].cpu().numpy()[mask]
    parent = parent_of[cell]
    r, _ = np.nonzero(mask)
    x = o.astype(np.float64)[r] + mid.cpu().numpy().astype(np.float64)[mask][:, None] * d.astype(np.float64)[r]
    want = F0[parent] + np.einsum("nra,na->nr", grad[parent], x - p0[parent])
    got = feats.cpu().numpy().astype(np.float64)[mask]
    return float(np.abs(got - want).max()), int(mask.sum())


def test_field_through_the_real_path_is_the_parent_field(tn, device, scenes):
    """trace -> find_visited_cells -> interpolate_values at the midpoints of the split mesh's segments, against the float64 PARENT
    interpolant at o + t d.  The tolerance is the parent commit's own behaviour: the identical procedure on the UNSPLIT mesh gives
    e0, and the split mesh must stay within 8 e0 -- a child's smallest height is at least a quarter of its parent's, so its
    barycentrics are up to 4 x worse conditioned, times 2 for the rounding of the centroid and of the mean."""
    xyz, cells, select = sc.case(scenes, "random_300_30pct")
    want = sc.statement(scenes, "random_300_30pct")
    V, T = len(xyz), len(cells)
    field_np = sc.values_for(V, 64, seed=9)
    F0, grad, p0 = sc.parent_interpolant(xyz, cells, field_np)                # every tetrahedron of random_mesh has volume
    o, d = scenes.outside_in_rays(2000, 12)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
    field = _dev(field_np, device)
    e0, n0 = _midpoint_error(tn, device, tr, o, d, field, np.arange(T), F0, grad, p0)
    out = tr.split_tetrahedra(_dev(select, device), vertex_rows=(field,))
    e1, n1 = _midpoint_error(tn, device, tr, o, d, out["vertex_rows"][0], out["cell_parent"].cpu().numpy().astype(np.int64), F0, grad, p0)
    print(f"field through the real path: unsplit e0 = {e0:.3e} over {n0} midpoints, split = {e1:.3e} over {n1} midpoints, "
          f"ratio {e1 / e0:.2f} (bound 8)")
    assert n1 > n0 > 10000 and e0 > 0 and e1 <= 8 * e0
    tr.close()


# ----------------------------------------------------------------------------------------------------------------- the adapter
def test_densify_grows_the_model_and_training_goes_on(tn, device, scenes, monkeypatch):
    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    optim = importlib.import_module("tetra-nerf_amd.optim")
    g = sc.geometry()
    plugin.install(ref.TetrahedraNerf)
    try:
        pts, cells = scenes.random_mesh(1500, 31)
        model = rm.build_model(ref, pts, cells, num_samples=48, num_fine_samples=48).to(device)
        V, T = len(pts), len(cells)
        if getattr(model, "tetrahedra_occupancy", None) is None:             # (the reference registers it under use_occupancy_field)
            model.register_buffer("tetrahedra_occupancy", torch.zeros(T, device=device))
        model.tetrahedra_occupancy = torch.rand(T, device=device)
        o, d = scenes.outside_in_rays(1024, 33)
        rb = rm.ray_bundle(ref, o, d, device, camera_indices=np.arange(len(o)) % 3)
        target = torch.rand(len(o), 3, device=device)
        weights = plugin.weights_from_model(model)
        opt = optim.FusedRAdam([model.tetrahedra_field] + weights, lr=1e-3)

        def train_step():
            opt.zero_grad(set_to_none=True)
            out = model(rb)
            model.get_loss_dict(out, {"image": target})["rgb_loss"].backward()
            opt.step()

        model.train()
        train_step()
        old_field, old_occ = model.tetrahedra_field, model.tetrahedra_occupancy.clone()
        old_m = opt.state[old_field]["exp_avg"].clone()
        assert tn.cpp.field_is_registered(old_field)
        model.eval()
        with torch.no_grad():
            before = model(rb)["rgb"].clone()
        select = torch.from_numpy(np.random.default_rng(2).random(T) < 0.1).to(device)
        want = g.split_tetrahedra_statement(pts, cells, select.cpu().numpy())
        K = want["num_new"]
        res = plugin.densify(model, select, optimizer=opt)
        assert res["num_new"] == K > 0.08 * T and res["num_vertices"] == V + K and res["num_cells"] == T + 3 * K
        assert res["counters"].tolist() == want["counters"].tolist() and not res["retriangulated"]
        # names, kinds, shapes, config
        names = dict(model.named_parameters())
        buffers = dict(model.named_buffers())
        assert names["tetrahedra_field"] is model.tetrahedra_field and tuple(model.tetrahedra_field.shape) == (64, V + K)
        assert isinstance(model.tetrahedra_field, torch.nn.Parameter) and model.tetrahedra_field.requires_grad
        assert tuple(buffers["tetrahedra_cells"].shape) == (T + 3 * K, 4) and tuple(buffers["tetrahedra_occupancy"].shape) == (T + 3 * K,)
        assert tuple(model.tetrahedra_vertices.shape) == (V + K, 3)
        assert model.config.num_tetrahedra_vertices == V + K and model.config.num_tetrahedra_cells == T + 3 * K
        assert np.array_equal(sc.bits(model.tetrahedra_vertices.detach().cpu().numpy()), sc.bits(want["vertices"]))
        assert np.array_equal(model.tetrahedra_cells.cpu().numpy(), want["cells"])
        assert torch.equal(model.tetrahedra_occupancy, old_occ[torch.from_numpy(want["cell_parent"]).long().to(device)])
        assert np.array_equal(sc.bits(model.tetrahedra_field.detach().cpu().numpy()),
                              sc.bits(g.split_vertex_rows_statement(old_field.detach().cpu().numpy(), want["vertex_parents"])))
        tracer = model.get_tetrahedra_tracer()
        assert tracer.tetrahedra_vertices is model.tetrahedra_vertices and tracer.tetrahedra_cells is model.tetrahedra_cells
        # the optimiser: the old parameter is gone, the step count stays, the moments are the carried ones
        new_field = model.tetrahedra_field
        assert all(p is not old_field for grp in opt.param_groups for p in grp["params"]) and old_field not in opt.state
        assert float(opt.state[new_field]["step"]) == 1
        assert np.array_equal(sc.bits(opt.state[new_field]["exp_avg"].cpu().numpy()),
                              sc.bits(g.split_vertex_rows_statement(old_m.cpu().numpy(), want["vertex_parents"])))
        assert not tn.cpp.field_is_registered(old_field) and tn.cpp.field_is_registered(new_field)
        # the frame: the same function up to rounding; recorded, not asserted (a ReLU decision may flip)
        calls = []
        transpose = tn.cpp._transpose_field
        monkeypatch.setattr(tn.cpp, "_transpose_field", lambda f: (calls.append(tuple(f.shape)), transpose(f))[1])
        with torch.no_grad():
            after = model(rb)["rgb"]
        print(f"densify: K = {K} of T = {T}; fused get_outputs frame before vs after: max |difference| = "
              f"{float((after - before).abs().max()):.3e}, mean = {float((after - before).abs().mean()):.3e}")
        assert bool(torch.isfinite(after).all())
        model.train()
        for _ in range(3):
            train_step()
        assert float(opt.state[new_field]["step"]) == 4 and bool(torch.isfinite(new_field).all())
        assert (64, V + K) not in calls, calls                               # the shadow was served: installed by densify, then by the steps
        theirs = torch.optim.RAdam([new_field] + weights, lr=1e-3)
        theirs.load_state_dict(opt.state_dict())
        assert float(theirs.state[new_field]["step"]) == 4 and tuple(theirs.state[new_field]["exp_avg"].shape) == (64, V + K)
        # the policy route: occupancy and width, cut to the widest, then a Delaunay mesh
        res = plugin.densify(model, occupancy_threshold=0.5, min_width=1e-3, max_new=50, optimizer=opt, new_moments="zero", retriangulate=True)
        assert 0 < res["num_new"] <= 50 and res["retriangulated"] and model.config.num_tetrahedra_cells == res["num_cells"]
        assert tuple(model.tetrahedra_field.shape) == (64, res["num_vertices"]) and len(model.tetrahedra_occupancy) == res["num_cells"]
        assert not opt.state[model.tetrahedra_field]["exp_avg"][:, V + K:].any()
        train_step()
        assert model.get_tetrahedra_tracer().delaunay_check()["counters"].tolist()[1] == 0
    finally:
        plugin.uninstall(ref.TetrahedraNerf)
