"""The face table on the GPU without a tracer (tn_face_table_count / tn_face_table_emit, csrc/tn_build.hip; cpp.face_table,
cpp.flip_to_delaunay, TetrahedraTracer.flip_to_delaunay(reload="once"), config.delaunay_repair_reload).

Bar: on every case of tests/face_table_cases.py -- the hand-made rows and the prefixes of one mesh at every wave, block, hash-doubling
and 1024-block edge of T -- every output array of the two entries equals the numpy statement (geometry.face_table_statement) byte
for byte, with guard words around every output left as they were; two runs give the same bytes; refused and short calls touch
nothing they do not own; a face in three rows sets its flag and nothing else goes wrong; the wrapper's table is the tracer's after a
load, on both builds; the flip loop that loads once gives what the loop that reloads every round gives and what the statement's loop
gives, leaves a tracer that traces as a fresh load, and does not touch the tracer while it runs; the free function needs no tracer;
and the adapter's model repaired that way trains on and equals a fresh rebuild."""
import importlib

import numpy as np
import pytest
import torch

import face_table_cases as ftc
import flip_cases as fc
import lifecycle_lib as ll

pytestmark = pytest.mark.gpu

KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")
M_TRACE = 512
GUARD = 64                            # guard elements in front of and behind every output
FILL = 0x7F7F7F7F


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.array(x)).to(device)   # (the cases are read-only: a copy)


def _lib():
    return importlib.import_module("tetra-nerf_amd._lib").load()


class _Guarded:
    """an int32 output array with GUARD elements of a fill pattern on either side"""

    def __init__(self, device, *shape):
        n = int(np.prod(shape))
        self.storage = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device=device)
        self.n, self.shape = n, shape

    def ptr(self):
        return self.storage.data_ptr() + GUARD * 4

    def array(self):
        return self.storage[GUARD:GUARD + self.n].reshape(self.shape)

    def guards_intact(self):
        return bool((self.storage[:GUARD] == FILL).all()) and bool((self.storage[GUARD + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.storage == FILL).all())


def _count_outputs(device, T):
    return {"partner": _Guarded(device, 4 * T), "face_index": _Guarded(device, 4 * T + 1), "counters": _Guarded(device, 4)}


def _emit_outputs(device, T, F):
    return {"faces": _Guarded(device, F, 3), "face_tets": _Guarded(device, F, 2), "tet_faces": _Guarded(device, T, 4)}


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _call_count(lib, V, c, outs):
    return lib.tn_face_table_count(0, V, c.size(0), _ptr(c), outs["partner"].ptr(), outs["face_index"].ptr(), outs["counters"].ptr(), None)


def _call_emit(lib, c, count, F, outs):
    return lib.tn_face_table_emit(c.size(0), _ptr(c), count["partner"].ptr(), count["face_index"].ptr(), F, outs["faces"].ptr(),
                                  outs["face_tets"].ptr(), outs["tet_faces"].ptr(), None)


def _entries(device, cells, V):
    """the two entries called directly, every output between guard words; F comes from the counters, as a caller reads it"""
    lib = _lib()
    c = _dev(cells, device)
    count = _count_outputs(device, len(cells))
    assert _call_count(lib, V, c, count) == 0, lib.tn_last_error()
    F = count["counters"].array().tolist()[0]
    assert 0 <= F <= 4 * len(cells)
    emit = _emit_outputs(device, len(cells), F)
    assert _call_emit(lib, c, count, F, emit) == 0, lib.tn_last_error()
    torch.cuda.synchronize()
    for key, o in {**count, **emit}.items():
        assert o.guards_intact(), f"{key}: a guard word was written"
    return {k: o.array() for k, o in {**count, **emit}.items()}


def _compare(got, want, what, keys=ftc.ARRAYS):
    for key in keys:
        g = np.ascontiguousarray(got[key].cpu().numpy()).view(np.uint32)
        assert got[key].is_cuda and g.shape == want[key].shape, (what, key, g.shape, want[key].shape)
        bad = np.nonzero(g.reshape(-1) != want[key].reshape(-1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {want[key].size} elements of {key} differ (first: {bad[:1]})"


@pytest.mark.parametrize("name", ftc.names(prefixes=True))
def test_entries_equal_the_statement_and_two_runs_give_the_same_bytes(tn, device, name):
    cells, V = ftc.case(name)
    want = ftc.statement(name)
    got, again = _entries(device, cells, V), _entries(device, cells, V)
    print(name, "T", len(cells), "counters", got["counters"].tolist())
    if int(want["counters"][2]) & ftc.FLAG_TRIPLE_FACE:
        # a statement about the flag: which two of the three sightings pair is left open, the counts are not, and (above) no guard word
        # was written
        _compare(got, want, name, keys=("counters",))
        _compare(again, want, name, keys=("counters",))
        return
    _compare(got, want, name)
    for key in ftc.ARRAYS:
        assert torch.equal(got[key], again[key]), (name, key)


def test_refused_and_short_calls_touch_nothing_they_do_not_own(tn, device):
    lib = _lib()
    cells, V = ftc.case("moved_400")
    want = ftc.statement("moved_400")
    T, F = len(cells), len(want["faces"])
    c = _dev(cells, device)
    count = _count_outputs(device, T)
    p, o = c.data_ptr(), [count[k].ptr() for k in ("partner", "face_index", "counters")]
    for args in ((0, V, T, None, *o), (0, V, T, p, None, o[1], o[2]), (0, V, T, p, o[0], None, o[2]), (0, V, T, p, o[0], o[1], None),
                 (0, V, 2 ** 30, p, *o), (0, V, 0, None, None, None, o[2])):
        assert lib.tn_face_table_count(*args, None) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in count.values())
    assert _call_count(lib, V, c, count) == 0
    assert [h & 0xFFFFFFFF for h in count["counters"].array().tolist()] == want["counters"].tolist()
    emit = _emit_outputs(device, T, F)
    e = [emit[k].ptr() for k in ("faces", "face_tets", "tet_faces")]
    for args in ((T, p, o[0], o[1], 4 * T + 1, *e), (2 ** 30, p, o[0], o[1], F, *e), (T, None, o[0], o[1], F, *e), (T, p, None, o[1], F, *e),
                 (T, p, o[0], None, F, *e), (T, p, o[0], o[1], F, None, e[1], e[2]), (T, p, o[0], o[1], F, e[0], None, e[2])):
        assert lib.tn_face_table_emit(*args, None) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in emit.values())
    # a num_faces smaller than F: no row >= num_faces is written, the rows below it are the table's, and a sighting names a face
    # below num_faces or was not written
    short = F - 37
    emit = _emit_outputs(device, T, short)
    assert _call_emit(lib, c, count, short, emit) == 0
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in emit.values())
    assert np.array_equal(emit["faces"].array().cpu().numpy().view(np.uint32), want["faces"][:short])
    assert np.array_equal(emit["face_tets"].array().cpu().numpy().view(np.uint32), want["face_tets"][:short])
    tf = emit["tet_faces"].array().cpu().numpy().view(np.uint32)
    assert np.array_equal(tf, np.where(want["tet_faces"] < short, want["tet_faces"], FILL)) and int((tf == FILL).sum()) >= 37
    # num_faces == 0 with null tables, and tet_faces == NULL: the tables alone
    assert lib.tn_face_table_emit(T, p, o[0], o[1], 0, None, None, None, None) == 0
    emit = _emit_outputs(device, T, F)
    assert lib.tn_face_table_emit(T, p, o[0], o[1], F, emit["faces"].ptr(), emit["face_tets"].ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert emit["tet_faces"].untouched() and emit["faces"].guards_intact() and emit["face_tets"].guards_intact()
    assert np.array_equal(emit["faces"].array().cpu().numpy().view(np.uint32), want["faces"])
    assert np.array_equal(emit["face_tets"].array().cpu().numpy().view(np.uint32), want["face_tets"])
    # no rows: empties and zero counters
    none = _count_outputs(device, 0)
    assert lib.tn_face_table_count(0, V, 0, None, None, none["face_index"].ptr(), none["counters"].ptr(), None) == 0
    torch.cuda.synchronize()
    assert none["counters"].array().tolist() == [0, 0, 0, 0] and none["face_index"].array().tolist() == [0]
    assert all(g.guards_intact() for g in none.values())


# ------------------------------------------------------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("gpu_build", [1, 0])
def test_wrapper_gives_the_tracers_own_table(tn, device, gpu_build):
    xyz, cells = fc.moved_mesh()
    c = _dev(cells, device)
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    tr.load_tetrahedra(_dev(xyz, device), c)
    faces, face_tets = tr.face_tables()
    out = tn.cpp.face_table(c)
    assert set(out) >= {"faces", "face_tets", "tet_faces", "counters", "num_faces"}
    assert out["num_faces"] == len(faces) and out["counters"].is_cuda and out["faces"].dtype == torch.int32
    assert torch.equal(out["faces"].cpu(), faces) and torch.equal(out["face_tets"].cpu(), face_tets)
    want = ftc.statement("moved_400")
    assert np.array_equal(out["tet_faces"].cpu().numpy().view(np.uint32), want["tet_faces"])
    assert [h & 0xFFFFFFFF for h in out["counters"].tolist()] == want["counters"].tolist()
    assert tn.cpp.face_table(c, len(xyz))["num_faces"] == len(faces)
    tr.close()


def test_wrapper_raises_the_builds_own_errors(tn, device):
    cells, V = ftc.case("triple_face")
    with pytest.raises(RuntimeError, match="shared by more than two tetrahedra"):
        tn.cpp.face_table(_dev(cells, device))
    cells, V = ftc.case("id_past_V")
    with pytest.raises(RuntimeError, match="out of bounds"):
        tn.cpp.face_table(_dev(cells, device), V)
    out = tn.cpp.face_table(_dev(cells, device))                              # without V only ids are compared: the table is defined
    _compare(out, ftc.statement("id_past_V"), "id_past_V", keys=("faces", "face_tets", "tet_faces"))
    empty = tn.cpp.face_table(torch.zeros((0, 4), dtype=torch.int32, device=device))
    assert empty["num_faces"] == 0 and empty["faces"].shape == (0, 3) and empty["tet_faces"].shape == (0, 4)
    tr = tn.TetrahedraTracer(device)
    assert tr.supports_face_table
    xyz, mesh = fc.moved_mesh()
    tr.load_tetrahedra(_dev(xyz, device), _dev(mesh, device))
    with pytest.raises(RuntimeError, match="reload"):
        tr.flip_to_delaunay(reload="never")
    tr.close()


# ------------------------------------------------------------------------------------------------------------------ the flip loop
def _same_repair(got, want, what):
    """two dicts of flip_to_delaunay, or one against the statement's loop"""
    numpy = isinstance(want["cells"], np.ndarray)
    rounds = [r.tolist() for r in want["rounds"]] if numpy else [list(r) for r in want["rounds"]]
    assert [list(r) for r in got["rounds"]] == rounds, what
    for key in ("num_rounds", "violated", "unflippable"):
        assert got[key] == want[key], (what, key)
    cells = want["cells"] if numpy else want["cells"].cpu().numpy()
    src = np.where(want["cell_sources"] == fc.EMPTY, -1, want["cell_sources"]) if numpy else want["cell_sources"].cpu().numpy()
    assert np.array_equal(got["cells"].cpu().numpy(), cells) and got["num_tetrahedra"] == len(cells), what
    assert np.array_equal(got["cell_sources"].cpu().numpy(), src), what
    if not numpy:
        for a, b in zip(got["tet_values"], want["tet_values"]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@pytest.mark.parametrize("gpu_build", [1, 0])
def test_loading_once_equals_loading_every_round(tn, device, scenes, gpu_build):
    xyz, cells = fc.moved_mesh()
    T = len(cells)
    x, c = _dev(xyz, device), _dev(cells, device)
    o, d = scenes.outside_in_rays(2000, 12)
    od = _dev(o, device), _dev(d, device)
    occ = torch.rand(T, device=device)
    occ[::5] = 0.0
    every = tn.TetrahedraTracer(device)
    every.set_option("gpu_build", gpu_build)
    every.load_tetrahedra(x, c, refittable=bool(gpu_build))
    want = every.flip_to_delaunay(tet_values=(occ,), reload="round")
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    tr.load_tetrahedra(x, c, refittable=bool(gpu_build))
    # max_rounds = 0 counts, emits nothing and loads nothing: the tracer stays as loaded while rounds run on tables of their own
    loads = []
    load = tr.load_tetrahedra
    tr.load_tetrahedra = lambda *a, **k: (loads.append(1), load(*a, **k))[1]
    none = tr.flip_to_delaunay(tet_values=(occ,), max_rounds=0, reload="once")
    assert none["num_rounds"] == 0 and none["rounds"] == want["rounds"][:1] and none["cells"] is c and tr.tetrahedra_cells is c and not loads
    assert none["tet_values"][0] is occ
    out = tr.flip_to_delaunay(tet_values=(occ,), reload="once")
    assert loads == [1]                                                       # exactly one load, at the end
    _same_repair(out, want, f"gpu_build={gpu_build}: once vs round")
    _same_repair(out, ftc.repaired(), f"gpu_build={gpu_build}: once vs the statement's loop")
    assert out["num_rounds"] > 1 and 100 * out["violated"] <= out["rounds"][0][1] and out["rounds"][0][1] > 100
    assert tr.tetrahedra_cells is out["cells"] and tr.tetrahedra_vertices is x and tr._refittable == bool(gpu_build)
    assert out["tet_values"][0].shape == (out["num_tetrahedra"],)
    # the monitor on the repaired tracer reports the last round's counters
    check = tr.delaunay_check()["counters"].tolist()
    assert check[:3] == list(out["rounds"][-1][:3]) and check[1] == out["violated"]
    # it traces as a fresh load of the returned cells, on both kernel families
    fresh = tn.TetrahedraTracer(device)
    fresh.set_option("gpu_build", gpu_build)
    fresh.load_tetrahedra(x, out["cells"])
    for walk in (0, 2):
        tr.set_option("walk", walk)
        fresh.set_option("walk", walk)
        got, other = tr.trace_rays(*od, M_TRACE), fresh.trace_rays(*od, M_TRACE)
        for k in KEYS:
            assert torch.equal(got[k].view(torch.int32), other[k].view(torch.int32)), (walk, k)
        assert int((got["num_visited_cells"] > 0).sum()) > 300
    # a second call finds nothing to do, returns its inputs and loads nothing
    new_occ = out["tet_values"][0]
    again = tr.flip_to_delaunay(tet_values=(new_occ,), reload="once")
    assert again["num_rounds"] == 0 and again["cells"] is out["cells"] and again["tet_values"][0] is new_occ
    assert tr.tetrahedra_cells is out["cells"] and loads == [1]
    # max_rounds
    tr.load_tetrahedra(x, c)
    part = tr.flip_to_delaunay(max_rounds=2, reload="once")
    assert part["num_rounds"] == 2 and len(part["rounds"]) == 3 and part["rounds"] == out["rounds"][:3]
    assert tr.tetrahedra_cells is part["cells"]
    print("gpu_build", gpu_build, "rounds", out["num_rounds"], "violated", out["rounds"][0][1], "->", out["violated"], "T", T, "->", out["num_tetrahedra"])
    for t in (tr, fresh, every):
        t.close()


def test_a_round_that_raises_leaves_the_tracer_as_it_was(tn, device, monkeypatch):
    xyz, cells = fc.moved_mesh()
    x, c = _dev(xyz, device), _dev(cells, device)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(x, c)
    before = tr.delaunay_check()["counters"].tolist()
    calls = []
    count = tn.cpp._face_table_count

    def second_table_fails(cells, V):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("the second table fails")
        return count(cells, V)

    monkeypatch.setattr(tn.cpp, "_face_table_count", second_table_fails)
    with pytest.raises(RuntimeError, match="second table"):
        tr.flip_to_delaunay(reload="once")
    assert tr.tetrahedra_cells is c and tr.delaunay_check()["counters"].tolist() == before
    tr.close()


def test_free_function_needs_no_tracer(tn, device):
    xyz, cells = fc.moved_mesh()
    x, c = _dev(xyz, device), _dev(cells, device)
    occ = torch.rand(len(cells), device=device)
    out = tn.cpp.flip_to_delaunay(x, c, tet_values=(occ,))
    want = ftc.repaired()
    _same_repair(out, want, "free function vs the statement's loop")
    # the carried values: the largest over the composed sources (the largest per round, round after round; values >= 0)
    src, carried = out["cell_sources"].cpu().numpy(), occ.cpu().numpy()
    best = np.where(src >= 0, carried[np.maximum(src, 0)], 0.0).max(1)
    assert np.array_equal(out["tet_values"][0].cpu().numpy(), best.astype(np.float32))
    part = tn.cpp.flip_to_delaunay(x, c, max_rounds=2)
    assert part["num_rounds"] == 2 and part["rounds"] == out["rounds"][:3]
    none = tn.cpp.flip_to_delaunay(x, out["cells"])
    assert none["num_rounds"] == 0 and none["cells"] is out["cells"]


# ----------------------------------------------------------------------------------------------------------------- the adapter
POINTS = ("after the repair", "at the end")


def test_a_model_repaired_with_one_load_trains_on_and_equals_a_fresh_rebuild(tn, device, scenes):
    """tests/test_flip_gpu.py's scenario with config.delaunay_repair_reload = "once": scenario B's model (tests/lifecycle_lib.py),
    2 steps, a centroid split of the lifecycle ball, 4 steps -- the monitor repairs by flips on tables of their own and loads once --,
    a frame, check point, 2 steps, a frame, check point, under the deterministic field gradient"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
        life = ll._Life(tn, device, scenes, "B")
        life.model.config.delaunay_repair, life.model.config.retriangulate_above = "flip", 0.02
        life.model.config.delaunay_repair_reload = "once"
        modes = []
        flip = tn.cpp.TetrahedraTracer.flip_to_delaunay
        mp.setattr(tn.cpp.TetrahedraTracer, "flip_to_delaunay", lambda self, *a, **k: (modes.append(k.get("reload")), flip(self, *a, **k))[1])
        life.plugin.install(life.ref.TetrahedraNerf)
        try:
            life.train(2)
            res = life.plugin.densify(life.model, ll._ball(life.model), optimizer=life.opt)
            T = life.model.tetrahedra_cells.shape[0]
            field_before = life.model.tetrahedra_field.shape
            life.train(4)
            life.frame()
            repairs, qhull = getattr(life.model, "_tn_flip_repairs", 0), getattr(life.model, "_tn_retriangulations", 0)
            counters = life.model.get_tetrahedra_tracer().delaunay_check()["counters"].tolist()
            life.check_point(POINTS[0])
            life.train(2)
            life.frame()
            life.check_point(POINTS[1])
        finally:
            life.plugin.uninstall(life.ref.TetrahedraNerf)
    print("\n".join(life.log), "\nflip repairs", repairs, "re-triangulations", qhull, "monitor after the repair", counters, "modes", modes)
    assert res["num_new"] > 0 and repairs >= 1 and qhull == 0 and modes and set(modes) == {"once"}
    assert counters[1] <= 0.02 * counters[0] and life.model.tetrahedra_cells.shape[0] > T and life.model.tetrahedra_field.shape == field_before
    assert bool(torch.isfinite(life.model.tetrahedra_field).all())
    for point in POINTS:
        lived, fresh, fresh2 = (life.results[point][k] for k in ("lived", "fresh", "fresh2"))
        bad = ll.compare(fresh, fresh2)
        assert not bad, f"{point}: two fresh rebuilds differ in\n  " + "\n  ".join(bad)
        bad = ll.compare(lived, fresh)
        assert not bad, f"{point}: the repaired model differs from a fresh rebuild in\n  " + "\n  ".join(bad)
        assert len(lived) > 60
