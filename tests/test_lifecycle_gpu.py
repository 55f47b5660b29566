"""The product of the steps, on the GPU (tests/lifecycle_lib.py has the helpers and the docstrings of both parts).

Part A: a model that LIVED THROUGH mesh adaptation -- training steps, densify by statistics and by a region, a re-triangulation by
densify and one by the Delaunay monitor inside get_outputs, vertices moved by the optimiser, shortened by the limiter and followed
by the refit -- against a FRESH REBUILD from its state dict and its optimiser's state dict.  One fixed probe (two evaluation
frames, a trace, the tracer's quality / Delaunay / isosurface queries, one training batch with every gradient, the optimiser step,
the field shadow) runs on both; every entry must be equal bit for bit.  Precondition, tested on its own: two fresh rebuilds agree.
What the adapter keeps outside the state dict is listed and classified in lifecycle_lib.ADAPTER_ATTRIBUTES; a new `_tn_*`
attribute fails test_every_adapter_attribute_is_classified until it is classified there.

Part B: the kernels on meshes that are themselves the output of a split (generation g - 1 input of the deepest generation of each
family): split kernels = statement byte for byte; trace = oracle bit for bit on both builds; limiter = statement, refit = fresh
load, no tetrahedron flips; Delaunay counters and isosurface = their statements; the field through the real path against the
float64 generation-0 interpolant within 2 * 4^g of the unsplit mesh's own error."""
import numpy as np
import pytest
import torch

import lifecycle_lib as ll
import split_cases as sc
import test_delaunay_gpu as tdg
import test_isosurface_gpu as tig
import test_refit_gpu as trg
import test_split_gpu as tsg
import test_vertex_guard_gpu as tvg

pytestmark = pytest.mark.gpu
M = 512
_dev = tsg._dev


# =========================================================================================================== part B: generations
@pytest.mark.parametrize("name", ll.DEEPEST)
def test_split_kernels_equal_the_statement_on_generation_input(tn, device, scenes, name):
    xyz, cells, select, want = ll.step(scenes, name)
    got = tsg._entries(device, xyz, cells, select)
    print(name, "input T", len(cells), "asked", int(select.sum()), "counters", got["counters"].tolist())
    tsg._compare(got, want, name)
    # the field's 64 rows, the shadow given and asked for
    g = sc.geometry()
    V, K = len(xyz), want["num_new"]
    values = sc.values_for(V, 64, seed=V)
    v, par = _dev(values, device), _dev(want["vertex_parents"], device)
    rows = g.split_vertex_rows_statement(values, want["vertex_parents"])
    for mode in ("mean", "zero"):
        expect = rows if mode == "mean" else g.split_vertex_rows_statement(values, want["vertex_parents"], new="zero")
        out, out_vm = tn.cpp.split_vertex_rows(v, par, new=mode, values_vm=v.t().contiguous(), want_vertex_major=True)
        assert tuple(out.shape) == (64, V + K) and np.array_equal(sc.bits(out.cpu().numpy()), sc.bits(expect)), (name, mode)
        assert np.array_equal(sc.bits(out_vm.cpu().numpy()), sc.bits(np.ascontiguousarray(expect.T))), (name, mode, "shadow")


@pytest.mark.parametrize("gpu_build", [1, 0])
@pytest.mark.parametrize("name", ("cube_gen5", "region_gen3"))
def test_trace_equals_the_oracle_on_generation_meshes(tn, device, scenes, oracle, name, gpu_build):
    xyz, cells = ll.mesh(scenes, name)
    o, d = scenes.outside_in_rays(2000, 12)
    ot = oracle.OracleTracer(use_bvh=True)
    ot.load_tetrahedra(xyz, cells)
    want = ot.trace_rays(o, d, M)
    assert int(want["num_visited_cells"].max()) < M and int((want["num_visited_cells"] > 0).sum()) == 2000   # no ray is cut
    tr = tn.TetrahedraTracer(device)
    tr.set_option("gpu_build", gpu_build)
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
    od = _dev(o, device), _dev(d, device)
    for walk in (0, 2):
        tr.set_option("walk", walk)
        got = tr.trace_rays(*od, M)
        assert int(got["num_visited_cells"].max()) < M
        for k in tsg.KEYS:
            a, b = np.ascontiguousarray(got[k].cpu().numpy()).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
            bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
            assert len(bad) == 0, f"{name} gpu_build={gpu_build} walk={walk}: {k} differs from the oracle on {len(bad)} rows (first: {bad[:4]})"
    print(name, "gpu_build", gpu_build, "T", len(cells), "most tetrahedra on a ray", int(want["num_visited_cells"].max()))
    tr.close()


def test_limiter_and_refit_on_a_third_generation_mesh(tn, device, scenes):
    g = sc.geometry()
    xyz, cells = ll.mesh(scenes, "region_gen3")
    new = (xyz + np.random.default_rng(5).normal(scale=0.01, size=xyz.shape)).astype(np.float32)
    want = g.limit_vertex_step_statement(torch.from_numpy(np.array(xyz)), torch.from_numpy(new), torch.from_numpy(np.array(cells)), 0.25)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device), refittable=True)
    x = _dev(new, device)
    counters = tvg._limit_and_compare(tr, device, np.array(xyz), new, want, 0.25, "region_gen3")
    c = counters.tolist()
    print("region_gen3: limiter counters", c, "of", len(xyz), "vertices")
    assert c[0] > 0.5 * len(xyz) and c[2] == 0 and c[3] == 0
    tr.limit_vertex_step(_dev(xyz, device), x, 0.25)
    limited = x.cpu().numpy()
    assert np.array_equal(sc.bits(limited), sc.bits(want["xyz"].numpy()))
    # no tetrahedron flips: float64 orientation on the limited vertices
    before, after = sc.vol6(xyz.astype(np.float64)[cells]), sc.vol6(limited.astype(np.float64)[cells])
    assert np.all(before != 0) and np.array_equal(np.sign(before), np.sign(after))
    unlimited = sc.vol6(new.astype(np.float64)[cells])
    assert int((np.sign(unlimited) != np.sign(before)).sum()) > 0              # (the proposal itself flips some)
    # the refit: every query answers as on a tracer freshly loaded on the limited vertices
    tr.update_vertices(x)
    fresh = tn.TetrahedraTracer(device)
    fresh.load_tetrahedra(_dev(limited, device), _dev(cells, device))
    o1, d1 = scenes.outside_in_rays(1500, 40)
    o2, d2 = scenes.inside_out_rays(1500, 41)
    to, td = _dev(np.concatenate([o1, o2]), device), _dev(np.concatenate([d1, d2]), device)
    for walk in (0, 2):
        tr.set_option("walk", walk), fresh.set_option("walk", walk)
        a, b = tr.trace_rays(to, td, M), fresh.trace_rays(to, td, M)
        trg._assert_same_rows(a, b, f"region_gen3, walk={walk}: refitted vs fresh")
        assert int(a["num_visited_cells"].max()) < M and int((a["num_visited_cells"] > 0).sum()) > 2900
    tr.close(), fresh.close()


def test_delaunay_and_isosurface_on_a_third_generation_mesh(tn, device, scenes):
    g = sc.geometry()
    xyz, cells = ll.mesh(scenes, "region_gen3")
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
    ft = tdg._face_tets(tr)
    want = g.delaunay_face_statement(cells, ft, xyz)
    got = tr.delaunay_check(face_state=True, tet_violations=True)
    print("region_gen3: delaunay counters", got["counters"].tolist())
    tdg._compare(got, want, "region_gen3", len(cells), len(ft))
    assert want["counters"][1] > 1000                                          # a split mesh is not Delaunay
    values = ll.smooth_scalar(xyz)
    level = float(np.median(values))
    surface = tr.isosurface(_dev(values, device), level)
    expect = g.isosurface_statement(xyz, cells, values, level)
    assert expect["num_triangles"] > 1000
    tig._compare(surface, expect, "region_gen3")
    tr.close()


def test_field_through_the_real_path_across_generations(tn, device, scenes):
    """tests/test_split_gpu.py::_midpoint_error (trace -> find_visited_cells -> interpolate_values at the midpoint of every traversed
    segment) on random30_gen{1,2,3}, against the float64 GENERATION-0 interpolant of the ancestor at o + t d.  Bar: e_g <= 2 * 4^g * e0
    with e0 the same procedure on the unsplit mesh, measured here -- the argument the existing test gives for g = 1, extended: a
    child's smallest height is at least a quarter of its parent's, so the barycentrics are up to 4 x worse conditioned per
    generation, times 2 for the rounding of the centroid and of the mean."""
    xyz0, cells0 = ll.mesh(scenes, "random30_gen0")
    fields = ll.fields(scenes, "random30", 64, seed=9)
    F0, grad, p0 = sc.parent_interpolant(xyz0, cells0, fields[0])
    o, d = scenes.outside_in_rays(2000, 12)
    errors = []
    for g in range(4):
        name = f"random30_gen{g}"
        xyz, cells = ll.mesh(scenes, name)
        tr = tn.TetrahedraTracer(device)
        tr.load_tetrahedra(_dev(xyz, device), _dev(cells, device))
        e, n = tsg._midpoint_error(tn, device, tr, o, d, _dev(fields[g], device), ll.ancestors(scenes, name), F0, grad, p0)
        tr.close()
        errors.append((e, n))
        if g:
            print(f"field through the real path, {name}: T = {len(cells)}, e{g} = {e:.3e} over {n} midpoints = {e / errors[0][0]:.2f} e0 "
                  f"(bar {2 * 4 ** g}; e0 = {errors[0][0]:.3e} over {errors[0][1]} midpoints)")
    e0, n0 = errors[0]
    assert e0 > 0 and n0 > 10000
    for g in range(1, 4):
        assert errors[g][1] > errors[g - 1][1] and errors[g][0] <= 2 * 4 ** g * e0, (g, errors)


# ============================================================================================ part A: lived against a fresh rebuild
POINTS = ("after the first densify", "at the end")


@pytest.mark.parametrize("kind", ("A", "B"))
def test_two_fresh_rebuilds_agree(tn, device, scenes, kind):
    """the precondition of everything below: the probe is deterministic on two models rebuilt from the same state"""
    res = ll.scenario(tn, device, scenes, kind)
    print("\n".join(res["log"]))
    for point in POINTS:
        bad = ll.compare(res[point]["fresh"], res[point]["fresh2"])
        assert not bad, f"scenario {kind}, {point}: two fresh rebuilds differ in\n  " + "\n  ".join(bad)
        mask = res[point]["fresh"]["1 frame/ray_mask"]
        assert 0 < int(mask.sum()) < mask.size                                # the evaluation rays hit and miss
        assert len(res[point]["fresh"]) > 60


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("kind", ("A", "B"))
def test_lived_model_equals_a_fresh_rebuild(tn, device, scenes, kind, point):
    res = ll.scenario(tn, device, scenes, kind)
    lived, fresh = res[point]["lived"], res[point]["fresh"]
    # probe step 7: the field's vertex-major shadow is the field, on both sides
    for side in (lived, fresh):
        assert np.array_equal(sc.bits(side["7 shadow"]), sc.bits(side["7 shadow/field_t"]))
    bad = ll.compare(lived, fresh)
    assert not bad, f"scenario {kind}, {point}: the lived model differs from a fresh rebuild in\n  " + "\n  ".join(bad)


def test_scenario_a_is_what_it_is_named_for(tn, device, scenes):
    res = ll.scenario(tn, device, scenes, "A")
    assert 0 < res["split"]["num_new"] <= 40 and res["split"]["stats_reset"] is True and not res["split"]["retriangulated"]
    assert 0 < res["split2"]["num_new"] <= 40 and res["split2"]["retriangulated"]
    # the optimiser's state after each densify is the statement's carry of the state before (lifecycle_lib.densify_and_check)
    assert res["carried"] == [("tetrahedra_field", "exp_avg", "mean"), ("tetrahedra_field", "exp_avg_sq", "mean"),
                              ("tetrahedra_field", "exp_avg", "zero"), ("tetrahedra_field", "exp_avg_sq", "zero")]
    end = res["at the end"]["lived"]
    assert end["5 train/tet_stats_added"].any() and "5 train/occupancy" in end
    assert "5 train/grad/tetrahedra_vertices" not in end
    # the second anchor of the frame: the split model against the unsplit one (lived against fresh cannot see what both share)
    before, after = res["frame_before"], res["frame_after"]
    assert torch.equal(before["ray_mask"], after["ray_mask"])
    diff = (after["rgb"] - before["rgb"]).abs()
    print(f"scenario A, first densify: K = {res['split']['num_new']}; evaluation frame before vs after: max |rgb difference| = "
          f"{float(diff.max()):.3e}, mean = {float(diff.mean()):.3e}; accumulation {float((after['accumulation'] - before['accumulation']).abs().max()):.3e}"
          " (recorded, not asserted: a ReLU decision may flip)")
    assert bool(torch.isfinite(after["rgb"]).all())


def test_scenario_b_is_what_it_is_named_for(tn, device, scenes):
    res = ll.scenario(tn, device, scenes, "B")
    assert res["split"]["num_new"] > 100 and res["split2"]["num_new"] > res["split"]["num_new"]
    # the second split asked children of the first (no re-triangulation in between), and the monitor then re-triangulated
    assert res["retriangulations_before_second_split"] == 0 and res["retriangulations"] >= 1
    # inside the call that re-triangulated, before the batch was added: statistics of the new size, all zero
    seen = res["stats_after_retriangulation"]
    assert len(seen) >= 1 and all(s is not None and s[0] == (s[2], 3) and not s[1] for s in seen), seen
    assert res["carried"] == 2 * [(n, m, "mean") for n in ll.CARRIED_PARAMETERS for m in ("exp_avg", "exp_avg_sq")]
    # what _follow_vertices remembers was reset by densify: the snapshot is the split vertex table, the key is its key
    assert res["derived_after_split"] == (True, True, True), res["derived_after_split"]
    print("scenario B: vertex step counters (clamped, frozen, flipped, collapsed)", res["vertex_step_counters"],
          "delaunay counters (interior, violated, uncertain, violated inverted)", res["delaunay_counters"])
    assert res["vertex_step_counters"][0] > 0 and res["vertex_step_counters"][2:] == [0, 0]      # the limiter shortened moves; none flipped
    end = res["at the end"]["lived"]
    assert "5 train/grad/tetrahedra_vertices" in end and end["5 train/grad/tetrahedra_vertices"].any()
    assert "5 train/loss/distortion_loss" in end and "1 frame/distortion" in end and "8 state/vertex_snapshot" in end
    assert end["6 step/exp_avg/tetrahedra_vertices"].shape == end["8 state/tetrahedra_vertices"].shape


def test_every_adapter_attribute_is_classified(tn, device, scenes):
    """every `_tn_*` attribute found on the model, its tracer and its renderer after scenario B is in
    lifecycle_lib.ADAPTER_ATTRIBUTES: the next cache someone adds has to be classified there"""
    res = ll.scenario(tn, device, scenes, "B")
    found = res["at the end attributes"]
    for side in ("lived", "fresh"):
        for where, names in found[side].items():
            unknown = [n for n in names if n not in ll.ADAPTER_ATTRIBUTES[where]]
            assert not unknown, f"{side} {where}: {unknown} not classified in lifecycle_lib.ADAPTER_ATTRIBUTES"
    # scenario B exercises every one of them on the lived side
    for where, table in ll.ADAPTER_ATTRIBUTES.items():
        assert sorted(table) == found["lived"][where], (where, found["lived"][where])
    assert set(v for t in ll.ADAPTER_ATTRIBUTES.values() for v in t.values()) == {ll.CARRIED, ll.DERIVED, ll.DIAGNOSTIC}
