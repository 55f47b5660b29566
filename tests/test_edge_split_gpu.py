"""The edge split on the GPU (tn_edge_split_count / tn_edge_split_count_tables / tn_edge_split_emit, csrc/tn_edge_split.hip;
cpp.split_edges, TetrahedraTracer.split_edges, nerfstudio_plugin.densify(method="edge")).

Bar: on every case of tests/edge_split_cases.py -- the stock scenes, the hand-made rings and the ring soups at every wave, block
and grid-cap edge of T and of the candidate count -- every output array equals the numpy statement
(geometry.split_edges_statement) byte for byte, with guard words around every output left as they were; two runs give the same
bytes; refused and short calls touch nothing they do not own; the tracer's own tables give what the explicit tables give; a
tracer that split its mesh traces as the oracle loaded with the split mesh does, on both builds and both kernel families; the
field gathered through the real path on the split mesh stays within 8 x the unsplit mesh's own error against the float64 parent
interpolant; and the adapter's model grows, trains on, and equals a fresh rebuild from its state dict."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import edge_split_cases as ec
import lifecycle_lib as ll
import split_cases as sc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import reference_model as rm   # noqa: E402

KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")
M_TRACE = 512
GUARD = 64                            # guard elements in front of and behind every output
FILL = 0x7F7F7F7F


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.array(x)).to(device)   # (the cases are read-only: a copy)


def _lib():
    return importlib.import_module("tetra-nerf_amd._lib").load()


class _Guarded:
    """an output array with GUARD elements of a fill pattern on either side"""

    def __init__(self, device, *shape, dtype=torch.int32):
        n = int(np.prod(shape))
        fill = 0x7F if dtype == torch.uint8 else FILL
        self.storage = torch.full((n + 2 * GUARD,), fill, dtype=torch.uint8 if dtype == torch.uint8 else torch.int32, device=device)
        self.fill, self.n, self.shape, self.dtype = fill, n, shape, dtype

    def ptr(self):
        return self.storage.data_ptr() + GUARD * self.storage.element_size()

    def array(self):
        body = self.storage[GUARD:GUARD + self.n]
        return (body.view(torch.float32) if self.dtype == torch.float32 else body).reshape(self.shape)

    def guards_intact(self):
        return bool((self.storage[:GUARD] == self.fill).all()) and bool((self.storage[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.storage == self.fill).all())


def _count_outputs(device, T):
    return {"tet_offsets": _Guarded(device, T + 1), "tet_edge": _Guarded(device, T), "bisected": _Guarded(device, T, dtype=torch.uint8),
            "edge_vertices": _Guarded(device, T, 2), "counters": _Guarded(device, 10)}


def _emit_outputs(device, V, T, Kv, Kt):
    return {"vertices": _Guarded(device, V + Kv, 3, dtype=torch.float32), "cells": _Guarded(device, T + Kt, 4),
            "cell_parent": _Guarded(device, T + Kt), "vertex_parents": _Guarded(device, Kv, 4)}


def _call_count(lib, V, T, F, x, c, s, f, ft, outs):
    return lib.tn_edge_split_count_tables(0, V, T, x.data_ptr(), c.data_ptr(), s.data_ptr(), F, f.data_ptr(), ft.data_ptr(),
                                          outs["tet_offsets"].ptr(), outs["tet_edge"].ptr(), outs["bisected"].ptr(),
                                          outs["edge_vertices"].ptr(), outs["counters"].ptr(), None)


def _call_emit(lib, V, T, x, c, count, Kv, Kt, outs):
    return lib.tn_edge_split_emit(V, T, x.data_ptr(), c.data_ptr(), count["tet_offsets"].ptr(), count["tet_edge"].ptr(),
                                  count["edge_vertices"].ptr(), Kv, Kt, outs["vertices"].ptr(), outs["cells"].ptr(),
                                  outs["cell_parent"].ptr(), outs["vertex_parents"].ptr(), None)


def _entries(device, xyz, cells, select, faces, face_tets):
    """the two entries called directly (the wrapper does not call the second one when nothing is accepted), every output between
    guard words"""
    lib = _lib()
    V, T, F = len(xyz), len(cells), len(faces)
    x, c, s, f, ft = (_dev(a, device) for a in (xyz, cells, select, faces, face_tets))
    count = _count_outputs(device, T)
    assert _call_count(lib, V, T, F, x, c, s, f, ft, count) == 0, lib.tn_last_error()
    counters = count["counters"].array().tolist()
    Kv, Kt = counters[8], counters[9]
    emit = _emit_outputs(device, V, T, Kv, Kt)
    assert _call_emit(lib, V, T, x, c, count, Kv, Kt, emit) == 0, lib.tn_last_error()
    torch.cuda.synchronize()
    for key, o in {**count, **emit}.items():
        assert o.guards_intact(), f"{key}: a guard word was written"
    assert bool((count["edge_vertices"].array()[Kv:] == FILL).all()), "edge_vertices: a row behind K_v was written"
    out = {k: o.array() for k, o in {**count, **emit}.items()}
    out["edge_vertices"] = out["edge_vertices"][:Kv]
    out.update(num_new=Kv, num_rows=Kt, num_cells=T + Kt)
    return out


def _compare(got, want, what, keys=ec.ARRAYS):
    for key in ("num_new", "num_rows", "num_cells"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in keys:
        g = got[key].cpu().numpy()
        assert got[key].is_cuda and g.shape == want[key].shape, (what, key, g.shape, want[key].shape)
        a, b = np.ascontiguousarray(g).reshape(-1), np.ascontiguousarray(want[key]).reshape(-1)
        bad = np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0] if len(a) else []
        assert len(bad) == 0, f"{what}: {len(bad)} of {want[key].size} elements of {key} differ (first: {bad[:1]})"


@pytest.mark.parametrize("name", ec.names(soups=True))
def test_kernels_equal_the_statement(tn, device, scenes, name):
    case = ec.case(scenes, name)
    want = ec.statement(scenes, name)
    got = _entries(device, *case)
    print(name, "T", len(case[1]), "counters", got["counters"].tolist())
    _compare(got, want, name)


def test_wrapper_is_the_entries_and_two_runs_give_the_same_bytes(tn, device, scenes):
    bt, blocks = ec.kernel_constants()
    for name in ("random_300_30pct", "grid_6_all", "near_duplicates_400_all", f"soup_{bt * blocks + 1}_third", "none_asked"):
        args = [_dev(a, device) for a in ec.case(scenes, name)]
        a = tn.cpp.split_edges(*args)
        b = tn.cpp.split_edges(args[0], args[1], args[2].bool(), args[3], args[4])
        _compare(a, ec.statement(scenes, name), name)
        for key in ec.ARRAYS:
            assert a[key].dtype == (torch.float32 if key == "vertices" else torch.uint8 if key == "bisected" else torch.int32)
            assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), (name, key)
    assert a["num_new"] == 0 and a["vertices"] is args[0] and a["cells"] is args[1]      # nothing accepted: the inputs themselves


def test_refused_and_short_calls_touch_nothing_they_do_not_own(tn, device, scenes):
    """a refused call leaves every output as it was; a call told smaller counts than were counted -- what a caller who changed the
    inputs between the two entries amounts to -- writes nothing behind them"""
    lib = _lib()
    case = ec.case(scenes, "random_300_30pct")
    want = ec.statement(scenes, "random_300_30pct")
    xyz, cells = case[:2]
    V, T, F, Kv, Kt = len(xyz), len(cells), len(case[3]), want["num_new"], want["num_rows"]
    x, c, s, f, ft = (_dev(a, device) for a in case)
    count = _count_outputs(device, T)
    p = lambda t: t.data_ptr()   # noqa: E731
    o = [count[k].ptr() for k in ("tet_offsets", "tet_edge", "bisected", "edge_vertices", "counters")]
    for args in ((0, V, T, None, p(c), p(s), F, p(f), p(ft), *o), (0, V, 2 ** 30, p(x), p(c), p(s), F, p(f), p(ft), *o),
                 (0, V, T, p(x), p(c), p(s), F, None, p(ft), *o), (0, 2 ** 32 - 1, T, p(x), p(c), p(s), F, p(f), p(ft), *o),
                 (0, V, T, p(x), p(c), p(s), F, p(f), p(ft), o[0], None, *o[2:])):
        assert lib.tn_edge_split_count_tables(*args, None) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in count.values())
    assert _call_count(lib, V, T, F, x, c, s, f, ft, count) == 0
    assert count["counters"].array().tolist() == want["counters"].tolist()
    emit = _emit_outputs(device, V, T, Kv, Kt)
    assert _call_emit(lib, V, T, x, c, count, T + 1, Kt, emit) != 0
    assert _call_emit(lib, V, T, x, c, count, Kv, T + 1, emit) != 0
    assert lib.tn_edge_split_emit(V, T, p(x), None, count["tet_offsets"].ptr(), count["tet_edge"].ptr(), count["edge_vertices"].ptr(), Kv, Kt,
                                  emit["vertices"].ptr(), emit["cells"].ptr(), emit["cell_parent"].ptr(), emit["vertex_parents"].ptr(), None) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in emit.values())
    short_v, short_t = Kv - 5, Kt - 7
    assert _call_emit(lib, V, T, x, c, count, short_v, short_t, emit) == 0
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in emit.values())
    assert bool((emit["vertices"].array().view(torch.int32)[V + short_v:] == FILL).all()) and bool((emit["vertex_parents"].array()[short_v:] == FILL).all())
    assert bool((emit["cells"].array()[T + short_t:] == FILL).all()) and bool((emit["cell_parent"].array()[T + short_t:] == FILL).all())
    assert np.array_equal(emit["vertices"].array()[:V + short_v].cpu().numpy().view(np.uint32), want["vertices"][:V + short_v].view(np.uint32))
    # an appended row whose edge is behind the short num_new has no vertex to name: it is its parent's row, copied
    parent = want["cell_parent"][T:T + short_t]
    known = (want["tet_edge"][parent] < short_v)[:, None]
    assert np.array_equal(emit["cells"].array()[T:T + short_t].cpu().numpy(), np.where(known, want["cells"][T:T + short_t], cells[parent]))
    assert np.array_equal(emit["cell_parent"].array()[T:T + short_t].cpu().numpy(), parent) and known.sum() > 300 and (~known).sum() > 0


# ------------------------------------------------------------------------------------------------------------------ the tracer
def _tracer_case(scenes, name):
    """(case, rays): the 30 % case under the stock rays; a soup of 13 whole rings under rays moved to its copies"""
    case = ec.case(scenes, name)
    o, d = scenes.outside_in_rays(2000, 12)
    if name.startswith("soup"):
        n = np.arange(len(o)) % 13
        o = (o - 0.5 + np.stack([(2 * n) % 7, n % 5, 0.5 * (n % 3)], 1)).astype(np.float32)
    return case, np.ascontiguousarray(o), np.ascontiguousarray(d)


@pytest.mark.parametrize("gpu_build", [1, 0])
@pytest.mark.parametrize("name", ("random_300_30pct", "soup_65_third"))
def test_tracer_split_traces_as_the_oracle_on_the_split_mesh(tn, device, scenes, oracle, name, gpu_build):
    (xyz, cells, select, faces, face_tets), o, d = _tracer_case(scenes, name)
    want = ec.statement(scenes, name)
    V, T = len(xyz), len(cells)
    od = _dev(o, device), _dev(d, device)
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    assert tr.supports_edge_split
    with pytest.raises(RuntimeError, match="load"):
        tr.split_edges(_dev(select, device))
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device), refittable=True)
    hit_before = tr.trace_rays(*od, M_TRACE)["num_visited_cells"] > 0
    occ = torch.rand(T, device=device)
    field = _dev(ec.values_for(V, 64, seed=3), device)
    # the count entry on the tracer's own tables is the entry on explicit tables
    own = tr.edge_split_count(_dev(select, device))
    for key in ("tet_offsets", "tet_edge", "bisected", "counters"):
        assert np.array_equal(own[key].cpu().numpy().view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), (name, key)
    assert np.array_equal(own["edge_vertices"][:want["num_new"]].cpu().numpy(), want["edge_vertices"])
    # nothing asked: the tracer is not touched, the inputs come back as they are
    same = tr.split_edges(torch.zeros(T, dtype=torch.uint8, device=device), vertex_rows=(field,), tet_values=(occ,))
    assert same["num_new"] == 0 and same["vertices"] is tr.tetrahedra_vertices and same["vertex_rows"][0] is field and same["tet_values"][0] is occ
    out = tr.split_edges(_dev(select, device), vertex_rows=(field,), tet_values=(occ,))
    _compare(out, want, name)
    assert tr.tetrahedra_vertices is out["vertices"] and tr.tetrahedra_cells is out["cells"] and tr._refittable
    assert torch.equal(out["tet_values"][0], occ[out["cell_parent"].long()])
    assert np.array_equal(ec.bits(out["vertex_rows"][0].cpu().numpy()),
                          ec.bits(ec.geometry().split_vertex_rows_statement(field.cpu().numpy(), want["vertex_parents"])))
    # the project's standard parity: every row of the five arrays is the oracle's on the same mesh, bit for bit
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(want["vertices"], want["cells"])
    ref = ot.trace_rays(o, d, M_TRACE)
    for walk in (0, 2):
        tr.set_option("walk", walk)
        got = tr.trace_rays(*od, M_TRACE)
        for k in KEYS:
            g, w = np.ascontiguousarray(got[k].cpu().numpy()).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
            bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
            assert len(bad) == 0, f"{name} gpu_build={gpu_build} walk={walk}: {k} differs from the oracle on {len(bad)} rows (first: {bad[:4]})"
        assert torch.equal(got["num_visited_cells"] > 0, hit_before) and int(hit_before.sum()) > 300
    print(name, "gpu_build", gpu_build, "K_v", want["num_new"], "K_t", want["num_rows"], "rays that hit", int(hit_before.sum()))
    tr.close()


def test_field_through_the_real_path_is_the_parent_field(tn, device, scenes):
    """trace -> find_visited_cells -> interpolate_values at the midpoints of the split mesh's segments, against the float64 PARENT
    interpolant at o + t d.  The tolerance is the one tests/test_split_gpu.py allows the centroid split: the identical procedure
    on the UNSPLIT mesh gives e0, and the split mesh must stay within 8 e0 (a child of a bisection keeps the heights above three
    of its faces and halves the fourth: it is conditioned no worse than a centroid child)."""
    tsg = importlib.import_module("test_split_gpu")
    xyz, cells, select, faces, face_tets = ec.case(scenes, "random_300_30pct")
    V, T = len(xyz), len(cells)
    field_np = ec.values_for(V, 64, seed=9)
    F0, grad, p0 = sc.parent_interpolant(xyz, cells, field_np)                # every tetrahedron of random_mesh has volume
    o, d = scenes.outside_in_rays(2000, 12)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
    field = _dev(field_np, device)
    e0, n0 = tsg._midpoint_error(tn, device, tr, o, d, field, np.arange(T), F0, grad, p0)
    out = tr.split_edges(_dev(select, device), vertex_rows=(field,))
    e1, n1 = tsg._midpoint_error(tn, device, tr, o, d, out["vertex_rows"][0], out["cell_parent"].cpu().numpy().astype(np.int64), F0, grad, p0)
    print(f"field through the real path: unsplit e0 = {e0:.3e} over {n0} midpoints, edge split = {e1:.3e} over {n1} midpoints, "
          f"ratio {e1 / e0:.2f} (bound 8)")
    assert n1 > n0 > 10000 and e0 > 0 and e1 <= 8 * e0
    tr.close()


# ----------------------------------------------------------------------------------------------------------------- the adapter
def test_densify_by_edges_grows_the_model_and_training_goes_on(tn, device, scenes, monkeypatch):
    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    optim = importlib.import_module("tetra-nerf_amd.optim")
    g = ec.geometry()
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
        old_m, old_v = opt.state[old_field]["exp_avg"].clone(), opt.state[old_field]["exp_avg_sq"].clone()
        assert tn.cpp.field_is_registered(old_field)
        model.eval()
        with torch.no_grad():
            before = model(rb)["rgb"].clone()
        select = torch.from_numpy(np.random.default_rng(2).random(T) < 0.1).to(device)
        with pytest.raises(ValueError, match="method"):
            plugin.densify(model, select, optimizer=opt, method="face")
        want = g.split_edges_statement(pts, cells, select.cpu().numpy(), *ec.face_table(cells))
        Kv, Kt = want["num_new"], want["num_rows"]
        res = plugin.densify(model, select, optimizer=opt, method="edge")
        assert res["num_new"] == Kv > 0 and res["num_vertices"] == V + Kv and res["num_cells"] == T + Kt and Kt > Kv
        assert res["counters"].tolist() == want["counters"].tolist() and not res["retriangulated"]
        assert np.array_equal(res["bisected"].cpu().numpy(), want["bisected"])
        # names, kinds, shapes, config
        names, buffers = dict(model.named_parameters()), dict(model.named_buffers())
        assert names["tetrahedra_field"] is model.tetrahedra_field and tuple(model.tetrahedra_field.shape) == (64, V + Kv)
        assert isinstance(model.tetrahedra_field, torch.nn.Parameter) and model.tetrahedra_field.requires_grad
        assert tuple(buffers["tetrahedra_cells"].shape) == (T + Kt, 4) and tuple(buffers["tetrahedra_occupancy"].shape) == (T + Kt,)
        assert model.config.num_tetrahedra_vertices == V + Kv and model.config.num_tetrahedra_cells == T + Kt
        assert np.array_equal(ec.bits(model.tetrahedra_vertices.detach().cpu().numpy()), ec.bits(want["vertices"]))
        assert np.array_equal(model.tetrahedra_cells.cpu().numpy(), want["cells"])
        assert torch.equal(model.tetrahedra_occupancy, old_occ[torch.from_numpy(want["cell_parent"]).long().to(device)])
        assert np.array_equal(ec.bits(model.tetrahedra_field.detach().cpu().numpy()),
                              ec.bits(g.split_vertex_rows_statement(old_field.detach().cpu().numpy(), want["vertex_parents"])))
        tracer = model.get_tetrahedra_tracer()
        assert tracer.tetrahedra_vertices is model.tetrahedra_vertices and tracer.tetrahedra_cells is model.tetrahedra_cells
        # the optimiser: the old parameter is gone, the step count stays, the moments are the carried ones
        new_field = model.tetrahedra_field
        assert all(p is not old_field for grp in opt.param_groups for p in grp["params"]) and old_field not in opt.state
        assert float(opt.state[new_field]["step"]) == 1
        for key, old in (("exp_avg", old_m), ("exp_avg_sq", old_v)):
            assert np.array_equal(ec.bits(opt.state[new_field][key].cpu().numpy()),
                                  ec.bits(g.split_vertex_rows_statement(old.cpu().numpy(), want["vertex_parents"]))), key
        assert not tn.cpp.field_is_registered(old_field) and tn.cpp.field_is_registered(new_field)
        calls = []
        transpose = tn.cpp._transpose_field
        monkeypatch.setattr(tn.cpp, "_transpose_field", lambda f: (calls.append(tuple(f.shape)), transpose(f))[1])
        with torch.no_grad():
            after = model(rb)["rgb"]
        print(f"densify(method='edge'): K_v = {Kv}, K_t = {Kt} of T = {T}; fused get_outputs frame before vs after: max |difference| = "
              f"{float((after - before).abs().max()):.3e}, mean = {float((after - before).abs().mean()):.3e}")
        assert bool(torch.isfinite(after).all())
        model.train()
        for _ in range(3):
            train_step()
        assert float(opt.state[new_field]["step"]) == 4 and bool(torch.isfinite(new_field).all())
        assert (64, V + Kv) not in calls, calls                              # the shadow was served: installed by densify, then by the steps
        # what was left unsplit is split by calling again with the selection carried
        carried = torch.cat([select & ~res["bisected"].bool(), torch.zeros(Kt, dtype=torch.bool, device=device)])
        again = plugin.densify(model, carried, optimizer=opt, method="edge")
        assert again["num_new"] > 0 and tuple(model.tetrahedra_field.shape) == (64, V + Kv + again["num_new"])
        train_step()
        assert bool(torch.isfinite(model.tetrahedra_field).all())
        # the default is the centroid split, as before
        last = plugin.densify(model, torch.ones(model.tetrahedra_cells.shape[0], dtype=torch.bool, device=device), max_new=20, optimizer=opt)
        assert last["counters"].numel() == 4 and 0 < last["num_new"] <= 20 and last["num_cells"] == again["num_cells"] + 3 * last["num_new"]
    finally:
        plugin.uninstall(ref.TetrahedraNerf)


# ------------------------------------------------------------------------------------------------------------- lived vs rebuilt
POINTS = ("after the edge split", "at the end")


def test_an_edge_split_model_equals_a_fresh_rebuild(tn, device, scenes):
    """scenario A's model (tests/lifecycle_lib.py): 2 steps, densify(method="edge") of the lifecycle ball, check point, 2 steps,
    check point, under the deterministic field gradient: a model rebuilt from the state dict renders and trains to the same bits"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
        life = ll._Life(tn, device, scenes, "A")
        life.plugin.install(life.ref.TetrahedraNerf)
        try:
            life.train(2)
            V, T = life.model.tetrahedra_vertices.shape[0], life.model.tetrahedra_cells.shape[0]
            res = life.plugin.densify(life.model, ll._ball(life.model), optimizer=life.opt, method="edge")
            life.check_point(POINTS[0])
            life.train(2)
            life.check_point(POINTS[1])
        finally:
            life.plugin.uninstall(life.ref.TetrahedraNerf)
    print("\n".join(life.log))
    assert res["num_new"] > 0 and res["num_cells"] > T + res["num_new"] and res["stats_reset"] is True
    for point in POINTS:
        lived, fresh, fresh2 = (life.results[point][k] for k in ("lived", "fresh", "fresh2"))
        bad = ll.compare(fresh, fresh2)
        assert not bad, f"{point}: two fresh rebuilds differ in\n  " + "\n  ".join(bad)
        bad = ll.compare(lived, fresh)
        assert not bad, f"{point}: the edge-split model differs from a fresh rebuild in\n  " + "\n  ".join(bad)
        assert len(lived) > 60 and lived["8 state/tetrahedra_vertices"].shape[0] == V + res["num_new"]
