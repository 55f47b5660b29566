"""The Delaunay repair by flips on the GPU (tn_flip_count / tn_flip_count_tables / tn_flip_emit / tn_flip_emit_loaded,
csrc/tn_flip.hip; cpp.flip_faces, cpp.flip_tet_values, TetrahedraTracer.flip_to_delaunay, config.delaunay_repair = "flip").

Bar: on every case of tests/flip_cases.py -- the hand-made rows, the moved mesh and its splits, and the soups at every wave, block
and grid-cap edge of T, of F and of the candidate count -- every output array equals the numpy statement
(geometry.flip_faces_statement) byte for byte, with guard words around every output left as they were; two runs give the same
bytes; refused and short calls touch nothing they do not own; the tracer's own tables give what explicit tables give, on both
builds; a tracer repaired by flip_to_delaunay reports what the statement's loop reports, traces as a fresh load of the same cells
and as the oracle, on both kernel families; per-vertex state is not touched; the carried occupancy dominates every source; and
the adapter's model is repaired, trains on, and equals a fresh rebuild from its state dict."""
import importlib

import numpy as np
import pytest
import torch

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
    """an output array with GUARD elements of a fill pattern on either side"""

    def __init__(self, device, *shape, dtype=torch.int32):
        n = int(np.prod(shape))
        fill = 0x7F if dtype == torch.uint8 else FILL
        self.storage = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
        self.fill, self.n, self.shape = fill, n, shape

    def ptr(self):
        return self.storage.data_ptr() + GUARD * self.storage.element_size()

    def array(self):
        return self.storage[GUARD:GUARD + self.n].reshape(self.shape)

    def guards_intact(self):
        return bool((self.storage[:GUARD] == self.fill).all()) and bool((self.storage[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.storage == self.fill).all())


def _count_outputs(device, T, F):
    return {"tet_offsets": _Guarded(device, T + 1), "tet_flip": _Guarded(device, T), "flipped": _Guarded(device, T, dtype=torch.uint8),
            "face_flip": _Guarded(device, F, 3), "counters": _Guarded(device, 10)}


def _emit_outputs(device, rows):
    return {"cells": _Guarded(device, rows, 4), "cell_sources": _Guarded(device, rows, 3)}


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _call_count(lib, V, T, F, x, c, f, ft, outs):
    return lib.tn_flip_count_tables(0, V, T, _ptr(x), _ptr(c), F, _ptr(f), _ptr(ft), outs["tet_offsets"].ptr(), outs["tet_flip"].ptr(),
                                    outs["flipped"].ptr(), outs["face_flip"].ptr(), outs["counters"].ptr(), None)


def _call_emit(lib, T, F, c, f, ft, count, K23, K32, outs):
    return lib.tn_flip_emit(T, _ptr(c), F, _ptr(f), _ptr(ft), count["tet_offsets"].ptr(), count["tet_flip"].ptr(), count["face_flip"].ptr(),
                            K23, K32, outs["cells"].ptr(), outs["cell_sources"].ptr(), None)


def _entries(device, xyz, cells, faces, face_tets):
    """the two entries called directly (the wrapper does not call the second one when nothing is accepted), every output between
    guard words"""
    lib = _lib()
    V, T, F = len(xyz), len(cells), len(faces)
    x, c, f, ft = (_dev(a, device) for a in (xyz, cells, faces, face_tets))
    count = _count_outputs(device, T, F)
    assert _call_count(lib, V, T, F, x, c, f, ft, count) == 0, lib.tn_last_error()
    counters = count["counters"].array().tolist()
    K23, K32 = counters[8], counters[9]
    emit = _emit_outputs(device, T + K23 - K32)
    assert _call_emit(lib, T, F, c, f, ft, count, K23, K32, emit) == 0, lib.tn_last_error()
    torch.cuda.synchronize()
    for key, o in {**count, **emit}.items():
        assert o.guards_intact(), f"{key}: a guard word was written"
    out = {k: o.array() for k, o in {**count, **emit}.items()}
    out.update(num_23=K23, num_32=K32, num_cells=T + K23 - K32)
    return out


def _compare(got, want, what, keys=fc.ARRAYS):
    for key in ("num_23", "num_32", "num_cells"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in keys:
        g = got[key].cpu().numpy()
        assert got[key].is_cuda and g.shape == want[key].shape, (what, key, g.shape, want[key].shape)
        a, b = np.ascontiguousarray(g).reshape(-1), np.ascontiguousarray(want[key]).reshape(-1)
        bad = np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0] if len(a) else []
        assert len(bad) == 0, f"{what}: {len(bad)} of {want[key].size} elements of {key} differ (first: {bad[:1]})"


@pytest.mark.parametrize("name", fc.names(soups=True))
def test_kernels_equal_the_statement(tn, device, scenes, name):
    case = fc.case(scenes, name)
    want = fc.statement(scenes, name)
    got = _entries(device, *case)
    print(name, "T", len(case[1]), "F", len(case[2]), "counters", got["counters"].tolist())
    _compare(got, want, name)


def test_wrapper_is_the_entries_and_two_runs_give_the_same_bytes(tn, device, scenes):
    bt, blocks = fc.kernel_constants()
    for name in ("moved_400", "moved_400_edge_split", "ring3_32", f"soup_T_{bt * blocks + 1}", "nothing_violated"):
        args = [_dev(a, device) for a in fc.case(scenes, name)]
        a, b = tn.cpp.flip_faces(*args), tn.cpp.flip_faces(*args)
        _compare(a, fc.statement(scenes, name), name)
        for key in fc.ARRAYS:
            assert a[key].dtype == (torch.uint8 if key == "flipped" else torch.int32)
            assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), (name, key)
    assert a["num_23"] + a["num_32"] == 0 and a["cells"] is args[1]          # nothing accepted: the input itself
    # the carry of a per-tetrahedron array, on the device
    name = "moved_400"
    s, T = fc.statement(scenes, name), len(fc.case(scenes, name)[1])
    values = np.abs(np.random.default_rng(4).normal(size=T)).astype(np.float32)
    got = tn.cpp.flip_tet_values(_dev(values, device), _dev(s["cell_sources"], device))
    assert np.array_equal(fc.bits(got.cpu().numpy()), fc.bits(fc.geometry().flip_tet_values_statement(values, s["cell_sources"])))


def test_refused_and_short_calls_touch_nothing_they_do_not_own(tn, device, scenes):
    """a refused call leaves every output as it was; a call told smaller counts than were counted -- what a caller who changed the
    inputs between the two entries amounts to -- writes nothing behind them"""
    lib = _lib()
    case, want = fc.case(scenes, "moved_400"), fc.statement(scenes, "moved_400")
    V, T, F, K23, K32 = len(case[0]), len(case[1]), len(case[2]), want["num_23"], want["num_32"]
    x, c, f, ft = (_dev(a, device) for a in case)
    count = _count_outputs(device, T, F)
    p = lambda t: t.data_ptr()   # noqa: E731
    o = [count[k].ptr() for k in ("tet_offsets", "tet_flip", "flipped", "face_flip", "counters")]
    for args in ((0, V, T, None, p(c), F, p(f), p(ft), *o), (0, V, 2 ** 30, p(x), p(c), F, p(f), p(ft), *o),
                 (0, V, T, p(x), p(c), F, None, p(ft), *o), (0, 2 ** 32 - 1, T, p(x), p(c), F, p(f), p(ft), *o),
                 (0, V, T, p(x), p(c), F, p(f), p(ft), o[0], None, *o[2:])):
        assert lib.tn_flip_count_tables(*args, None) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in count.values())
    assert _call_count(lib, V, T, F, x, c, f, ft, count) == 0
    assert count["counters"].array().tolist() == want["counters"].tolist()
    rows = T + K23 - K32
    emit = _emit_outputs(device, rows)
    assert _call_emit(lib, T, F, c, f, ft, count, F + 1, K32, emit) != 0
    assert _call_emit(lib, T, F, c, f, ft, count, T, T, emit) != 0
    assert lib.tn_flip_emit(T, None, F, p(f), p(ft), o[0], o[1], o[3], K23, K32, emit["cells"].ptr(), emit["cell_sources"].ptr(), None) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in emit.values())
    # fewer 2-3 flips than were counted: the appended rows behind the short count are not written, nothing behind the buffer is
    short = K23 - 5
    emit = _emit_outputs(device, T + short - K32)
    assert _call_emit(lib, T, F, c, f, ft, count, short, K32, emit) == 0
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in emit.values())
    assert np.array_equal(emit["cells"].array().cpu().numpy(), want["cells"][:T + short - K32])
    # more 3-2 flips than were counted (rows = T + K23 - K32 - 3): every store stays inside the smaller buffer
    emit = _emit_outputs(device, rows - 3)
    assert _call_emit(lib, T, F, c, f, ft, count, K23, K32 + 3, emit) == 0
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in emit.values())


# ------------------------------------------------------------------------------------------------------------------ the tracer
def _tracer_tables(tr, device):
    faces, face_tets = tr.face_tables()
    return faces.numpy(), face_tets.numpy()


@pytest.mark.parametrize("gpu_build", [1, 0])
def test_tracer_entries_on_its_own_tables(tn, device, scenes, gpu_build):
    """tn_flip_count / tn_flip_emit_loaded on the tracer's tables give the statement on those tables; xyz = NULL is the loaded xyz"""
    g = fc.geometry()
    xyz, cells = fc.moved_mesh()
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    assert tr.supports_flip
    with pytest.raises(RuntimeError, match="load"):
        tr.flip_count()
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
    want = g.flip_faces_statement(xyz, cells, *_tracer_tables(tr, device))
    assert want["num_23"] > 20 and want["num_32"] > 5
    own = tr.flip_count()
    for key in ("tet_offsets", "tet_flip", "flipped", "face_flip", "counters"):
        assert np.array_equal(own[key].cpu().numpy().view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), key
    T, F = len(cells), own["face_flip"].size(0)
    out = _count_outputs(device, T, F)
    assert _lib().tn_flip_count(tr._h, len(xyz), None, out["tet_offsets"].ptr(), out["tet_flip"].ptr(), out["flipped"].ptr(),
                                out["face_flip"].ptr(), out["counters"].ptr(), None) == 0
    assert out["counters"].array().tolist() == want["counters"].tolist() and all(o.guards_intact() for o in out.values())
    _compare(tr.flip_faces(), want, f"gpu_build={gpu_build}")
    assert tr.tetrahedra_cells.shape[0] == T                                 # one round alone does not touch the tracer
    tr.close()


@pytest.mark.parametrize("gpu_build", [1, 0])
def test_flip_to_delaunay_repairs_the_tracer(tn, device, scenes, oracle, gpu_build):
    g = fc.geometry()
    xyz, cells = fc.moved_mesh()
    V, T = len(xyz), len(cells)
    o, d = scenes.outside_in_rays(2000, 12)
    od = _dev(o, device), _dev(d, device)
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    x = _dev(xyz, device)
    tr.load_tetrahedra(x, _dev(cells, device), refittable=bool(gpu_build))
    hit_before = tr.trace_rays(*od, M_TRACE)["num_visited_cells"] > 0
    # the statement's loop on the face tables this build gives
    helper = tn.TetrahedraTracer(device)
    helper.set_option("gpu_build", gpu_build)

    def tables(c):
        helper.load_tetrahedra(x, _dev(c, device))
        return _tracer_tables(helper, device)

    want = g.flip_to_delaunay_statement(xyz, cells, tables)
    # per-vertex state: the field and a stand-in optimiser's moments are not the call's business -- bit-identical before and after
    field = torch.nn.Parameter(torch.randn(64, V, device=device))
    moments = {"exp_avg": torch.randn(64, V, device=device), "exp_avg_sq": torch.rand(64, V, device=device)}
    kept = [t.detach().clone() for t in (field, *moments.values(), x)]
    occ = torch.rand(T, device=device)
    occ[::5] = 0.0
    out = tr.flip_to_delaunay(tet_values=(occ,))
    for t, k in zip((field, *moments.values(), x), kept):
        assert torch.equal(t.detach().view(torch.int32), k.view(torch.int32))
    assert [list(r) for r in out["rounds"]] == [r.tolist() for r in want["rounds"]]
    assert out["num_rounds"] == want["num_rounds"] > 1 and out["violated"] == want["violated"] and out["unflippable"] == want["unflippable"]
    assert np.array_equal(out["cells"].cpu().numpy(), want["cells"]) and out["num_tetrahedra"] == len(want["cells"])
    assert np.array_equal(out["cell_sources"].cpu().numpy(), np.where(want["cell_sources"] == fc.EMPTY, -1, want["cell_sources"]))
    assert tr.tetrahedra_cells is out["cells"] and tr.tetrahedra_vertices is x and tr._refittable == bool(gpu_build)
    # the cap of the CPU test, on the device: at most 1 % of the initially violated faces remain
    assert 100 * out["violated"] <= out["rounds"][0][1] and out["rounds"][0][1] > 100
    # the monitor on the repaired tracer reports the last round's counters
    check = tr.delaunay_check()["counters"].tolist()
    assert check[:3] == list(out["rounds"][-1][:3]) and check[1] == out["violated"]
    # the occupancy dominates every source
    src, new_occ = out["cell_sources"], out["tet_values"][0]
    assert new_occ.shape == (out["num_tetrahedra"],)
    for k in range(src.size(1)):
        has = src[:, k] >= 0
        assert bool((new_occ[has] >= occ[src[has, k]]).all())
    single = src[:, 1:].lt(0).all(1) if src.size(1) > 1 else torch.ones_like(src[:, 0], dtype=torch.bool)
    assert torch.equal(new_occ[single], occ[src[single, 0]]) and int(single.sum()) > T // 2
    # a second call finds nothing to do and touches nothing
    again = tr.flip_to_delaunay(tet_values=(new_occ,))
    assert again["num_rounds"] == 0 and again["cells"] is out["cells"] and again["tet_values"][0] is new_occ and tr.tetrahedra_cells is out["cells"]
    # the repaired tracer traces as a fresh load of the same cells and as the oracle
    fresh = tn.TetrahedraTracer(device)
    fresh.set_option("gpu_build", gpu_build)
    fresh.load_tetrahedra(x, out["cells"])
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(xyz, want["cells"])
    ref = ot.trace_rays(o, d, M_TRACE)
    for walk in (0, 2):
        tr.set_option("walk", walk)
        fresh.set_option("walk", walk)
        got, other = tr.trace_rays(*od, M_TRACE), fresh.trace_rays(*od, M_TRACE)
        for k in KEYS:
            assert torch.equal(got[k].view(torch.int32), other[k].view(torch.int32)), (walk, k)
            a, w = np.ascontiguousarray(got[k].cpu().numpy()).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
            bad = np.nonzero((a != w).reshape(len(a), -1).any(1))[0]
            assert len(bad) == 0, f"gpu_build={gpu_build} walk={walk}: {k} differs from the oracle on {len(bad)} rows (first: {bad[:4]})"
        assert torch.equal(got["num_visited_cells"] > 0, hit_before) and int(hit_before.sum()) > 300      # the traced domain stays
    print("gpu_build", gpu_build, "rounds", out["num_rounds"], "violated", out["rounds"][0][1], "->", out["violated"], "T", T, "->", out["num_tetrahedra"])
    # max_rounds
    tr.load_tetrahedra(x, _dev(cells, device))
    part = tr.flip_to_delaunay(max_rounds=2)
    assert part["num_rounds"] == 2 and len(part["rounds"]) == 3 and part["rounds"] == out["rounds"][:3]
    for t in (tr, fresh, helper):
        t.close()


# ----------------------------------------------------------------------------------------------------------------- the adapter
POINTS = ("after the repair", "at the end")


def test_a_model_repaired_by_flips_trains_on_and_equals_a_fresh_rebuild(tn, device, scenes):
    """scenario B's model (tests/lifecycle_lib.py: moving vertices, limiter, monitor every 2nd call) with delaunay_repair = "flip"
    and a threshold the split mesh exceeds: 2 steps, a centroid split of the lifecycle ball, 4 steps -- the monitor repairs by
    flips --, a frame, check point, 2 steps, a frame, check point, under the deterministic field gradient"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
        life = ll._Life(tn, device, scenes, "B")
        life.model.config.delaunay_repair, life.model.config.retriangulate_above = "flip", 0.02
        life.plugin.install(life.ref.TetrahedraNerf)
        try:
            life.train(2)
            res = life.plugin.densify(life.model, ll._ball(life.model), optimizer=life.opt)
            T = life.model.tetrahedra_cells.shape[0]
            field_before = life.model.tetrahedra_field.shape
            life.train(4)
            life.frame()                                                      # (the pending move is limited and followed: scenario B's pattern)
            repairs, qhull = getattr(life.model, "_tn_flip_repairs", 0), getattr(life.model, "_tn_retriangulations", 0)
            counters = life.model.get_tetrahedra_tracer().delaunay_check()["counters"].tolist()
            life.check_point(POINTS[0])
            life.train(2)
            life.frame()
            life.check_point(POINTS[1])
        finally:
            life.plugin.uninstall(life.ref.TetrahedraNerf)
    print("\n".join(life.log), "\nflip repairs", repairs, "re-triangulations", qhull, "monitor after the repair", counters)
    assert res["num_new"] > 0 and repairs >= 1 and qhull == 0
    assert counters[1] <= 0.02 * counters[0] and life.model.tetrahedra_cells.shape[0] > T and life.model.tetrahedra_field.shape == field_before
    assert bool(torch.isfinite(life.model.tetrahedra_field).all())
    for point in POINTS:
        lived, fresh, fresh2 = (life.results[point][k] for k in ("lived", "fresh", "fresh2"))
        bad = ll.compare(fresh, fresh2)
        assert not bad, f"{point}: two fresh rebuilds differ in\n  " + "\n  ".join(bad)
        bad = ll.compare(lived, fresh)
        assert not bad, f"{point}: the repaired model differs from a fresh rebuild in\n  " + "\n  ".join(bad)
        assert len(lived) > 60
