"""Vertex pruning on the GPU (tn_prune_count / tn_prune_count_tables / tn_prune_emit / tn_prune_vertex_rows, csrc/tn_prune.hip;
cpp.prune_vertices, cpp.prune_vertex_rows, TetrahedraTracer.prune_count / remove_vertices, nerfstudio_plugin.prune).

Bar: on every case of tests/prune_cases.py -- the meshes with their dead balls and the random soups at every wave, block and
grid-cap edge -- the offsets, counters, new ids, kept ids and compacted vertices equal the numpy statement
(geometry.prune_vertices_statement) byte for byte, and no word outside the outputs changes; the compacted per-vertex arrays equal
geometry.prune_vertex_rows_statement byte for byte at every alignment of the two strides, with and without the shadow on either
side; a tracer loaded with the pruned mesh traces as the oracle loaded with it does and hits the rays the unpruned mesh hit; the
adapter's model trains on, densifies on, and equals a model rebuilt from its state, bit for bit."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import lifecycle_lib as ll
import prune_cases as pc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import reference_model as rm   # noqa: E402

KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")
M_TRACE = 512
GUARD = 64                                                                    # pattern words in front of and behind every output
PATTERN = 0x7F7F7F7F


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.array(x)).to(device)   # (the cases are read-only: a copy)


def _lib():
    return importlib.import_module("tetra-nerf_amd._lib").load()


class _Out:
    """an int32 output of n words inside a storage of pattern words; .t is the output"""

    def __init__(self, n, device):
        self.n, self.storage = n, torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=device)
        self.t = self.storage[GUARD:GUARD + n]

    def ptr(self):
        return self.t.data_ptr()

    def untouched_outside(self):
        s = self.storage.cpu().numpy()
        return bool((s[:GUARD] == PATTERN).all() and (s[GUARD + self.n:] == PATTERN).all())


def _entries(device, xyz, cells, dead, faces, face_tets, select, values=None):
    """the entries called directly (the wrapper does not call emit when nothing is removed), outputs inside pattern words"""
    lib = _lib()
    V, T, F = len(xyz), len(cells), len(faces)
    x, c, d, f, ft, s = (_dev(a, device) for a in (xyz, cells, dead, faces, face_tets, select))
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    offsets, counters = _Out(V + 1, device), _Out(5, device)
    assert lib.tn_prune_count_tables(device.index or 0, V, T, p(c), F, p(f), p(ft), p(d), p(s), offsets.ptr(), counters.ptr(), None) == 0, \
        lib.tn_last_error()
    Vp = int(offsets.t[V].item())
    new_id, kept, vertices = _Out(V, device), _Out(Vp, device), _Out(3 * Vp, device)
    assert lib.tn_prune_emit(V, p(x), offsets.ptr(), Vp, new_id.ptr(), kept.ptr(), vertices.ptr(), None) == 0, lib.tn_last_error()
    outs = {"offsets": offsets, "counters": counters, "new_id": new_id, "kept_ids": kept, "vertices": vertices}
    if values is not None:
        rows = len(values)
        v = _dev(values, device)
        vm = v.t().contiguous()
        for name, values_vm in (("rows", None), ("rows_from_vm", vm)):
            out, out_vm = _Out(rows * Vp, device), _Out(Vp * rows, device)
            assert lib.tn_prune_vertex_rows(rows, V, Vp, v.data_ptr(), p(values_vm), kept.ptr(), out.ptr(), out_vm.ptr(), None) == 0
            outs[name], outs[name + "_vm"] = out, out_vm
    torch.cuda.synchronize()
    return outs, Vp


def _compare(got, want, what):
    for key in pc.ARRAYS:
        g = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else got[key]
        w = pc.bits(want[key]).view(np.uint32).reshape(-1)
        g = np.ascontiguousarray(g).view(np.uint32).reshape(-1)
        bad = np.nonzero(g != w)[0] if g.shape == w.shape else [-1]
        assert len(bad) == 0, f"{what}: {len(bad)} of {w.size} words of {key} differ (first: {bad[:1]})"


@pytest.mark.parametrize("name", pc.names(soups=True))
def test_entries_equal_the_statement(tn, device, scenes, name):
    g = pc.geometry()
    c = pc.case(scenes, name)
    want = pc.statement(scenes, name)
    values = pc.values_for(len(c[0]), 3, seed=len(c[1]))
    outs, Vp = _entries(device, *c, values)
    print(name, "V", len(c[0]), "T", len(c[1]), "F", len(c[3]), "counters", outs["counters"].t.tolist())
    assert Vp == want["num_kept"]
    _compare({k: outs[k].t for k in pc.ARRAYS}, want, name)
    rows = g.prune_vertex_rows_statement(values, want["kept_ids"])
    for key in ("rows", "rows_from_vm"):
        assert np.array_equal(outs[key].t.cpu().numpy(), pc.bits(rows).reshape(-1).view(np.int32)), (name, key)
        assert np.array_equal(outs[key + "_vm"].t.cpu().numpy(), pc.bits(np.ascontiguousarray(rows.T)).reshape(-1).view(np.int32)), (name, key)
    for key, o in outs.items():
        assert o.untouched_outside(), (name, key)
    if name in pc.MESHES:                                                     # the tracer's entry, on its own face tables
        xyz, cells, dead = c[:3]
        tr = tn.TetrahedraTracer(device)
        tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
        offsets, counters = tr.prune_count(_dev(dead, device))
        assert np.array_equal(offsets.cpu().numpy().view(np.uint32), want["offsets"]) and counters.tolist() == want["counters"].tolist()
        tr.close()


def test_wrapper_is_the_entries_and_two_runs_give_the_same_bytes(tn, device, scenes):
    bt, blocks = pc.kernel_constants()
    for name in ("rand600_41_b035", "grid6_all", f"soup_{bt * blocks + 1}", "soup_select", "soup_no_tets"):
        xyz, cells, dead, faces, face_tets, select = (_dev(a, device) for a in pc.case(scenes, name))
        a = tn.cpp.prune_vertices(xyz, cells, dead, faces, face_tets, select)
        b = tn.cpp.prune_vertices(xyz, cells, dead.bool(), faces, face_tets, None if select is None else select.bool())
        want = pc.statement(scenes, name)
        _compare(a, want, name)
        assert a["num_kept"] == want["num_kept"] and a["num_removed"] == want["num_removed"]
        for key in pc.ARRAYS:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (name, key)
    assert a["num_removed"] == 0 and a["vertices"] is xyz                     # nothing removed: the input itself


# ------------------------------------------------------------------------------------------------------- the per-vertex arrays
# (V, V') on either side of 64 and 256, V' = 0, 1, 2, 3 mod 4, V' = V and V' = 0
SHAPES = [(63, 61), (65, 62), (64, 64), (66, 63), (70, 0), (255, 253), (257, 255), (300, 256), (300, 257), (261, 260), (259, 259)]


def _kept(V, Vp, seed):
    ids = np.sort(np.random.default_rng(seed).choice(V, Vp, replace=False)).astype(np.int32)
    if Vp >= 2 and V - Vp >= 2:
        ids[-1] = V + 1                                                       # an id past the table: that column is 0
    return ids


@pytest.mark.parametrize("rows", (1, 3, 64))
@pytest.mark.parametrize("V,Vp", SHAPES)
def test_vertex_rows_equal_the_statement(tn, device, V, Vp, rows):
    g = pc.geometry()
    assert {vp % 4 for _, vp in SHAPES} == {0, 1, 2, 3}
    ids = _kept(V, Vp, 100 * V + Vp)
    values = pc.values_for(V, rows, seed=V + Vp)
    v, kept = _dev(values, device), _dev(ids, device)
    want = g.prune_vertex_rows_statement(values, ids)
    for values_vm in (None, v.t().contiguous()):
        for want_vm in (False, True):
            got = tn.cpp.prune_vertex_rows(v, kept, values_vm=values_vm, want_vertex_major=want_vm)
            out, out_vm = got if want_vm else (got, None)
            what = (V, Vp, rows, values_vm is not None, want_vm)
            assert tuple(out.shape) == (rows, Vp) and np.array_equal(pc.bits(out.cpu().numpy()), pc.bits(want)), what
            if want_vm:
                assert tuple(out_vm.shape) == (Vp, rows)
                assert torch.equal(out_vm.view(torch.int32), out.t().contiguous().view(torch.int32)), what


# ------------------------------------------------------------------------------------------------------------------ the tracer
def _trace(tr, o, d):
    return tr.trace_rays(o, d, M_TRACE)


def test_tracer_remove_vertices_traces_as_the_oracle_on_the_pruned_mesh(tn, device, scenes, oracle, monkeypatch):
    name = "rand1500_31_b030"
    g = pc.geometry()
    xyz, cells, dead, *_ = pc.case(scenes, name)
    want = pc.statement(scenes, name)
    V, T = len(xyz), len(cells)
    o, d = scenes.outside_in_rays(1024, 33)
    od = _dev(o, device), _dev(d, device)
    tr = tn.TetrahedraTracer(device)
    assert tr.supports_prune
    with pytest.raises(RuntimeError, match="load"):
        tr.remove_vertices(_dev(dead, device))
    x, c = _dev(xyz, device), _dev(cells, device)
    tr.load_tetrahedra(x, c, refittable=True)
    hit_before = _trace(tr, *od)["num_visited_cells"] > 0
    occ = torch.from_numpy(np.where(dead != 0, 0, np.random.default_rng(3).random(T)).astype(np.float32)).to(device)
    field = _dev(pc.values_for(V, 64, seed=3), device)
    # nothing removed: the tracer is not touched, the inputs come back as they are
    same = tr.remove_vertices(torch.zeros(T, dtype=torch.uint8, device=device), vertex_rows=(field,), tet_values=(occ,))
    assert same["num_removed"] == 0 and same["vertices"] is x and same["cells"] is c and same["vertex_rows"][0] is field
    assert same["tet_values"][0] is occ and tr.tetrahedra_vertices is x and tr.tetrahedra_cells is c
    # a triangulation that raises: the tracer is exactly as before
    ext = tn.cpp

    def fail(points):
        raise RuntimeError("QH6154 qhull precision error (simulated)")

    with monkeypatch.context() as mp:
        mp.setattr(ext, "triangulate", fail)
        with pytest.raises(RuntimeError, match="QH6154"):
            tr.remove_vertices(_dev(dead, device), vertex_rows=(field,), tet_values=(occ,))
    assert tr.tetrahedra_vertices is x and tr.tetrahedra_cells is c
    assert torch.equal(_trace(tr, *od)["num_visited_cells"] > 0, hit_before)
    out = tr.remove_vertices(_dev(dead, device), vertex_rows=(field,), tet_values=(occ,))
    _compare(out, want, name)
    assert out["num_removed"] == want["num_removed"] == pc.REMOVED[name] and out["counters"].tolist() == want["counters"].tolist()
    new_cells = scenes.delaunay_cells(want["vertices"])
    assert np.array_equal(out["cells"].cpu().numpy(), new_cells) and out["num_tetrahedra"] == len(new_cells)
    assert tr.tetrahedra_vertices is out["vertices"] and tr.tetrahedra_cells is out["cells"] and tr._refittable
    assert np.array_equal(pc.bits(out["vertex_rows"][0].cpu().numpy()), pc.bits(g.prune_vertex_rows_statement(field.cpu().numpy(), want["kept_ids"])))
    carried = g.remap_tet_values_statement(cells, want["kept_ids"][new_cells], occ.cpu().numpy(), V)["values"]
    assert np.array_equal(pc.bits(out["tet_values"][0].cpu().numpy()), pc.bits(carried))
    # the project's standard parity: every row of the five arrays is the oracle's on the same mesh, bit for bit
    got = _trace(tr, *od)
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(want["vertices"], new_cells)
    ref = ot.trace_rays(o, d, M_TRACE)
    for k in KEYS:
        gk, w = np.ascontiguousarray(got[k].cpu().numpy()).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        bad = np.nonzero((gk != w).reshape(len(gk), -1).any(1))[0]
        assert len(bad) == 0, f"{name}: {k} differs from the oracle on {len(bad)} rows (first: {bad[:4]})"
    assert torch.equal(got["num_visited_cells"] > 0, hit_before) and int(hit_before.sum()) > 500
    tr.close()


# ----------------------------------------------------------------------------------------------------------------- the adapter
def test_prune_shrinks_the_model_and_training_goes_on(tn, device, scenes, monkeypatch):
    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    optim = importlib.import_module("tetra-nerf_amd.optim")
    g = pc.geometry()
    plugin.install(ref.TetrahedraNerf)
    try:
        xyz, cells, dead, *_ = pc.case(scenes, "rand1500_31_b030")
        want = pc.statement(scenes, "rand1500_31_b030")
        model = rm.build_model(ref, np.array(xyz), np.array(cells), num_samples=48, num_fine_samples=48).to(device)
        V, T = len(xyz), len(cells)
        if getattr(model, "tetrahedra_occupancy", None) is None:             # (the reference registers it under use_occupancy_field)
            model.register_buffer("tetrahedra_occupancy", torch.zeros(T, device=device))
        model.tetrahedra_occupancy = torch.rand(T, device=device)
        model.config.densify_stats = True
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
        old_field, old_occ, old_cells = model.tetrahedra_field, model.tetrahedra_occupancy.clone(), model.tetrahedra_cells
        old_m, old_v = opt.state[old_field]["exp_avg"].clone(), opt.state[old_field]["exp_avg_sq"].clone()
        tracer = model.get_tetrahedra_tracer()
        assert tn.cpp.field_is_registered(old_field) and model._tn_tet_stats.any()
        mask = torch.from_numpy(np.array(dead)).to(device)
        # a triangulation that raises: tracer and model untouched
        with monkeypatch.context() as mp:
            mp.setattr(tn.cpp, "triangulate", lambda points: (_ for _ in ()).throw(RuntimeError("QH6154 simulated")))
            with pytest.raises(RuntimeError, match="QH6154"):
                plugin.prune(model, mask, optimizer=opt)
        assert model.tetrahedra_field is old_field and model.tetrahedra_cells is old_cells and opt.state[old_field]["exp_avg"].shape == (64, V)
        assert tracer.tetrahedra_cells is old_cells and model.get_tetrahedra_tracer() is tracer
        res = plugin.prune(model, mask, optimizer=opt)
        R, Vp = want["num_removed"], want["num_kept"]
        assert res["num_removed"] == R == pc.REMOVED["rand1500_31_b030"] and res["num_vertices"] == Vp
        assert res["counters"].tolist() == want["counters"].tolist() and res["stats_reset"] is True
        new_cells = scenes.delaunay_cells(want["vertices"])
        Tp = len(new_cells)
        assert res["num_cells"] == Tp
        # names, kinds, shapes, config
        names = dict(model.named_parameters())
        buffers = dict(model.named_buffers())
        assert names["tetrahedra_field"] is model.tetrahedra_field and tuple(model.tetrahedra_field.shape) == (64, Vp)
        assert isinstance(model.tetrahedra_field, torch.nn.Parameter) and model.tetrahedra_field.requires_grad
        assert tuple(buffers["tetrahedra_cells"].shape) == (Tp, 4) and tuple(buffers["tetrahedra_occupancy"].shape) == (Tp,)
        assert tuple(model.tetrahedra_vertices.shape) == (Vp, 3)
        assert model.config.num_tetrahedra_vertices == Vp and model.config.num_tetrahedra_cells == Tp
        assert np.array_equal(pc.bits(model.tetrahedra_vertices.detach().cpu().numpy()), pc.bits(want["vertices"]))
        assert np.array_equal(model.tetrahedra_cells.cpu().numpy(), new_cells)
        carried = g.remap_tet_values_statement(cells, want["kept_ids"][new_cells], old_occ.cpu().numpy(), V)["values"]
        assert np.array_equal(pc.bits(model.tetrahedra_occupancy.cpu().numpy()), pc.bits(carried))
        kept = torch.from_numpy(np.array(want["kept_ids"])).long().to(device)
        new_field = model.tetrahedra_field
        assert torch.equal(new_field.detach().view(torch.int32), old_field.detach()[:, kept].view(torch.int32))
        tracer = model.get_tetrahedra_tracer()
        assert tracer.tetrahedra_vertices is model.tetrahedra_vertices and tracer.tetrahedra_cells is model.tetrahedra_cells
        # the statistics: zeros of the new size
        assert tuple(model._tn_tet_stats.shape) == (Tp, 3) and not model._tn_tet_stats.any()
        # the optimiser: the old parameter is gone, the step count stays, the moments are the kept columns
        assert all(p is not old_field for grp in opt.param_groups for p in grp["params"]) and old_field not in opt.state
        assert float(opt.state[new_field]["step"]) == 1
        assert torch.equal(opt.state[new_field]["exp_avg"].view(torch.int32), old_m[:, kept].view(torch.int32))
        assert torch.equal(opt.state[new_field]["exp_avg_sq"].view(torch.int32), old_v[:, kept].view(torch.int32))
        assert not tn.cpp.field_is_registered(old_field) and tn.cpp.field_is_registered(new_field)
        calls = []
        transpose = tn.cpp._transpose_field
        monkeypatch.setattr(tn.cpp, "_transpose_field", lambda f: (calls.append(tuple(f.shape)), transpose(f))[1])
        model.eval()
        with torch.no_grad():
            assert bool(torch.isfinite(model(rb)["rgb"]).all())
        model.train()
        for _ in range(3):
            train_step()
        assert float(opt.state[new_field]["step"]) == 4 and bool(torch.isfinite(new_field).all())
        assert (64, Vp) not in calls, calls                                   # the shadow was served: installed by prune, then by the steps
        theirs = torch.optim.RAdam([new_field] + weights, lr=1e-3)
        theirs.load_state_dict(opt.state_dict())
        assert float(theirs.state[new_field]["step"]) == 4 and tuple(theirs.state[new_field]["exp_avg"].shape) == (64, Vp)
        # nothing removable left under the same rule: nothing touched
        again = plugin.prune(model, occupancy_below=0.0, optimizer=opt)
        assert again["num_removed"] == 0 and model.tetrahedra_field is new_field
        # a densify after the prune
        grown = plugin.densify(model, torch.ones(Tp, dtype=torch.bool, device=device), max_new=30, stats=True, optimizer=opt)
        assert grown["num_new"] > 0 and tuple(model.tetrahedra_field.shape) == (64, Vp + grown["num_new"])
        train_step()
        assert bool(torch.isfinite(model.tetrahedra_field).all())
    finally:
        plugin.uninstall(ref.TetrahedraNerf)


# ------------------------------------------------------------------------------------------------------------- lived vs rebuilt
_SCENARIO = {}
POINTS = ("after the prune", "at the end")


def _scenario(tn, device, scenes):
    """scenario A's model (tests/lifecycle_lib.py): 2 steps, prune of the lifecycle ball, check point, 2 steps, check point; run
    once per session under the deterministic field gradient"""
    if "res" not in _SCENARIO:
        try:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
                life = ll._Life(tn, device, scenes, "A")
                life.plugin.install(life.ref.TetrahedraNerf)
                try:
                    life.train(2)
                    life.results["prune"] = life.plugin.prune(life.model, dead=ll._ball(life.model), optimizer=life.opt)
                    life.check_point(POINTS[0])
                    life.train(2)
                    life.check_point(POINTS[1])
                finally:
                    life.plugin.uninstall(life.ref.TetrahedraNerf)
            life.results["log"] = life.log
            _SCENARIO["res"] = life.results
        except Exception as e:   # noqa: BLE001
            _SCENARIO["res"] = e
    if isinstance(_SCENARIO["res"], Exception):
        raise _SCENARIO["res"]
    return _SCENARIO["res"]


def test_a_pruned_model_equals_a_fresh_rebuild(tn, device, scenes):
    res = _scenario(tn, device, scenes)
    print("\n".join(res["log"]))
    assert res["prune"]["num_removed"] == pc.REMOVED["rand600_41_b025"] and res["prune"]["stats_reset"] is True
    for point in POINTS:
        lived, fresh, fresh2 = res[point]["lived"], res[point]["fresh"], res[point]["fresh2"]
        for side in (lived, fresh):
            assert np.array_equal(pc.bits(side["7 shadow"]), pc.bits(side["7 shadow/field_t"]))
        bad = ll.compare(fresh, fresh2)
        assert not bad, f"{point}: two fresh rebuilds differ in\n  " + "\n  ".join(bad)
        bad = ll.compare(lived, fresh)
        assert not bad, f"{point}: the pruned model differs from a fresh rebuild in\n  " + "\n  ".join(bad)
        assert len(lived) > 60 and lived["8 state/tetrahedra_vertices"].shape[0] == 600 - pc.REMOVED["rand600_41_b025"]
