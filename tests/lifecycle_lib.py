"""What the lifecycle tests share (tests/test_lifecycle.py, tests/test_lifecycle_gpu.py): a plain module, no fixtures.

Part 1, the GENERATION meshes: a mesh that is itself the output of a split (geometry.split_tetrahedra_statement applied again and
again), computed once per session and never modified.  Three families --
    cube_gen{1..5}       scenes.cube_mesh(), every tetrahedron asked each time
    region_gen{1..4}     scenes.random_mesh(300, 3), every tetrahedron whose centroid lies within 0.25 of (0.5, 0.5, 0.5) asked
    random30_gen{1..4}   the same mesh, a fresh 30 % asked each time (generation 1 is split_cases' random_300_30pct)
`<family>_gen0` is the unsplit mesh.  Nothing here needs a GPU or the library.

Part 2, the LIVED-THROUGH model against a FRESH REBUILD (GPU): rebuild / carry_over / probe / compare and the two scenarios, run
once per session; every test of tests/test_lifecycle_gpu.py that looks at them reads the recorded results."""
import copy
import dataclasses
import importlib
import sys
from pathlib import Path

import numpy as np

import split_cases as sc

ROOT = Path(__file__).resolve().parents[1]
_CACHE = {}
CENTRE, RADIUS = 0.5, 0.25

# name -> number of tetrahedra; asserted by test_the_generations_are_what_they_are_named_for
GENERATION_CELLS = {
    "cube_gen0": 12, "cube_gen1": 48, "cube_gen2": 192, "cube_gen3": 768, "cube_gen4": 3072, "cube_gen5": 12288,
    "region_gen0": 1754, "region_gen1": 2162, "region_gen2": 3635, "region_gen3": 9275, "region_gen4": 31112,
    "random30_gen0": 1754, "random30_gen1": 3203, "random30_gen2": 5951, "random30_gen3": 11219, "random30_gen4": 21407,
}
DEPTH = {"cube": 5, "region": 4, "random30": 4}
DEEPEST = tuple(f"{family}_gen{g}" for family, g in DEPTH.items())


def names(family=None, first=1):
    return [f"{f}_gen{g}" for f, depth in DEPTH.items() if family in (None, f) for g in range(first, depth + 1)]


def _parse(name):
    family, g = name.rsplit("_gen", 1)
    return family, int(g)


def in_region(xyz, cells):
    """uint8 [T]: the tetrahedra whose centroid (float64 mean of the fp32 corners) lies within RADIUS of the centre"""
    centroid = np.asarray(xyz, np.float64)[np.asarray(cells, np.int64)].mean(1)
    return (np.linalg.norm(centroid - CENTRE, axis=1) < RADIUS).astype(np.uint8)


def _selection(family, g, xyz, cells):
    """what generation g (>= 1) of the family asks of generation g - 1"""
    if family == "cube":
        return np.ones(len(cells), np.uint8)
    if family == "region":
        return in_region(xyz, cells)
    return (np.random.default_rng(30 + g - 1).random(len(cells)) < 0.3).astype(np.uint8)


def step(scenes, name):
    """(xyz, cells, select) of generation g - 1 and the statement's answer, whose "vertices" and "cells" ARE generation g"""
    if name not in _CACHE:
        family, g = _parse(name)
        assert g >= 1, name
        xyz, cells = mesh(scenes, f"{family}_gen{g - 1}")
        select = _selection(family, g, xyz, cells)
        select.setflags(write=False)
        out = sc.geometry().split_tetrahedra_statement(xyz, cells, select)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = (xyz, cells, select, out)
    return _CACHE[name]


def mesh(scenes, name):
    """(xyz f32 [V, 3], cells i32 [T, 4]) of a generation, read-only"""
    family, g = _parse(name)
    if g == 0:
        key = ("gen0", family)
        if key not in _CACHE:
            xyz, cells = scenes.cube_mesh() if family == "cube" else scenes.random_mesh(300, 3)
            xyz, cells = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(cells, np.int32)
            xyz.setflags(write=False), cells.setflags(write=False)
            _CACHE[key] = (xyz, cells)
        return _CACHE[key]
    out = step(scenes, name)[3]
    return out["vertices"], out["cells"]


def ancestors(scenes, name):
    """int64 [T_g]: the generation-0 tetrahedron every tetrahedron of the generation descends from"""
    family, g = _parse(name)
    anc = np.arange(len(mesh(scenes, name)[1]))
    for k in range(g, 0, -1):
        anc = step(scenes, f"{family}_gen{k}")[3]["cell_parent"].astype(np.int64)[anc]
    return anc


def fields(scenes, family, rows=4, seed=7):
    """[field f32 [rows, V_g] for g = 0 .. depth]: N(0, 1) on generation 0, carried by split_vertex_rows_statement"""
    key = ("fields", family, rows, seed)
    if key not in _CACHE:
        g0 = sc.geometry()
        out = [sc.values_for(len(mesh(scenes, f"{family}_gen0")[0]), rows, seed=seed)]
        for g in range(1, DEPTH[family] + 1):
            out.append(g0.split_vertex_rows_statement(out[-1], step(scenes, f"{family}_gen{g}")[3]["vertex_parents"]))
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def barycentrics64(p, x):
    """float64 [n, s, 4]: the barycentric coordinates of the points x [n, s, 3] in the tetrahedra p [n, 4, 3]"""
    A = np.swapaxes(p[:, 1:] - p[:, :1], 1, 2)                                 # columns: the three edge vectors
    lam = np.swapaxes(np.linalg.solve(A, np.swapaxes(x - p[:, :1], 1, 2)), 1, 2)
    return np.concatenate([1.0 - lam.sum(2, keepdims=True), lam], 2)


def smooth_scalar(xyz):
    """a smooth per-vertex scalar (f32 [V]) whose median level set cuts the mesh: the squared distance from an off-centre point"""
    x = np.asarray(xyz, np.float32)
    d = x - np.array([0.45, 0.55, 0.5], np.float32)
    return np.ascontiguousarray((d * d).sum(1, dtype=np.float32))


# ======================================================================================================================
# Part 2: the adapter's state outside the state dict
# ======================================================================================================================
CARRIED, DERIVED, DIAGNOSTIC = "carried", "derived (must be rebuilt equal)", "diagnostic counter"
# every `_tn_*` attribute the adapter keeps on the model, on its tracer and on its renderer.  carried: legitimately outside the
# state dict and shaping the next batch -- carry_over copies it; derived: a cache of what the state dict holds -- a fresh model
# rebuilds it on its first call, and the probe shows that it rebuilt it equal; diagnostic: a counter nothing reads back.
ADAPTER_ATTRIBUTES = {
    "model": {
        "_tn_renderer": DERIVED,                 # keyed by (tracer, field) identity: nerfstudio_plugin._renderer_for
        "_tn_tet_stats": CARRIED,                # sums that continue; zeroed by densify and by a re-triangulation
        "_tn_tet_stats_pending": DERIVED,        # one batch's sample placement between get_outputs and get_loss_dict; None after
        "_tn_delaunay_counters": DIAGNOSTIC,
        "_tn_vertex_step_counters": DIAGNOSTIC,
        "_tn_retriangulations": DIAGNOSTIC,
    },
    "tracer": {
        "_tn_vertex_key": DERIVED,               # (version, storage) of the vertex table at the last load / refit
        "_tn_vertex_snapshot": DERIVED,          # the vertices of the last load / refit: what the limiter shortens against
        "_tn_follow_calls": CARRIED,             # which call is the delaunay_check_every-th
    },
    "renderer": {
        "_tn_train_batches": CARRIED,            # which training batch is the occupancy_refresh_every-th
    },
}
TRACE_KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")
ISO_KEYS = ("positions", "triangles", "triangle_tets", "edge_vertices", "edge_t", "tri_offsets", "ref_offsets")


def adapter_attribute_names(model):
    """{"model" | "tracer" | "renderer": the sorted `_tn_*` instance attributes found there}"""
    tracer = model.get_tetrahedra_tracer()
    objects = {"model": model, "tracer": tracer, "renderer": getattr(model, "_tn_renderer", None)}
    return {where: sorted(k for k in vars(obj) if k.startswith("_tn_")) if obj is not None else [] for where, obj in objects.items()}


def _modules():
    if str(ROOT / "tests" / "golden") not in sys.path:
        sys.path.insert(0, str(ROOT / "tests" / "golden"))
    rm =importlib.import_module("reference_model")
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    optim = importlib.import_module("tetra-nerf_amd.optim")
    return rm, plugin, optim


def optimise_vertices(model):
    """the model's vertex table becomes an optimised parameter under its name (the reference registers it as a buffer)"""
    import torch

    v = model.tetrahedra_vertices
    if not isinstance(v, torch.nn.Parameter):
        model.tetrahedra_vertices = torch.nn.Parameter(v.detach().clone(), requires_grad=True)
    return model.tetrahedra_vertices


def rebuild(ref, model, opt):
    """The FRESH side: a model built from the lived model's config and its current V and T, given the lived state dict; a new
    FusedRAdam over the new parameters in the lived optimiser's group order, given its state dict (a deep copy: torch's
    load_state_dict keeps tensors that already have the right device and dtype).  Tracer, renderer, field registration and shadow
    are created by the first call, as for any new model.  Returns (fresh model, fresh optimiser)."""
    import torch

    rm, plugin, optim = _modules()
    cfg = model.config
    declared = {f.name for f in dataclasses.fields(cfg)}
    given = {k: copy.deepcopy(getattr(cfg, k)) for k in declared
             - {"_target", "num_tetrahedra_vertices", "num_tetrahedra_cells", "collider_params", "tetrahedra_path"}}
    device = model.tetrahedra_field.device
    V, T = model.tetrahedra_vertices.shape[0], model.tetrahedra_cells.shape[0]
    fresh = rm.build_model(ref, np.zeros((V, 3), np.float32), np.zeros((T, 4), np.int32), num_train_data=model.num_train_data,
                           far_plane=float(model.collider.far_plane), **given)
    for k, v in vars(cfg).items():                                            # the opt-ins: no fields of the reference's config
        if k not in declared:
            setattr(fresh.config, k, copy.deepcopy(v))
    fresh = fresh.to(device)
    if isinstance(model.tetrahedra_vertices, torch.nn.Parameter):
        optimise_vertices(fresh)
    state = model.state_dict()
    assert set(state) == set(fresh.state_dict()), set(state) ^ set(fresh.state_dict())
    fresh.load_state_dict(state)
    occupancy = getattr(model, "tetrahedra_occupancy", None)
    if occupancy is not None and not isinstance(occupancy, torch.nn.Parameter):
        fresh.tetrahedra_occupancy = fresh.tetrahedra_occupancy.detach().clone()   # a plain buffer, as the lived model's
    fresh.train(model.training)
    name_of = {id(p): n for n, p in model.named_parameters()}
    new = dict(fresh.named_parameters())
    groups = [{"params": [new[name_of[id(p)]] for p in g["params"]]} for g in opt.param_groups]
    fresh_opt = optim.FusedRAdam(groups, lr=opt.param_groups[0]["lr"])
    fresh_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    return fresh, fresh_opt


def carried_state(lived):
    """What ADAPTER_ATTRIBUTES classifies as carried -- and the sync-free decision's last known fraction of hitting rays, which is
    the renderer's own -- read from the lived model by name (the statistics as a clone)."""
    tracer, rd = lived.get_tetrahedra_tracer(), getattr(lived, "_tn_renderer", None)
    stats = getattr(lived, "_tn_tet_stats", None)
    return {"_tn_train_batches": getattr(rd, "_tn_train_batches", None), "fraction": None if rd is None else rd._sync_free.fraction,
            "_tn_follow_calls": getattr(tracer, "_tn_follow_calls", None), "_tn_tet_stats": None if stats is None else stats.clone()}


def apply_carried(fresh, state):
    """Give a fresh model the carried state.  Its tracer and renderer are made here, as its first call would make them -- which
    is why this runs AFTER the lived model was probed: every load_tetrahedra forgets the shadows of ALL registered fields
    (cpp.invalidate_field_cache), so a tracer made earlier would repair a stale shadow of the lived model before the probe saw it."""
    _, plugin, _ = _modules()
    tracer = fresh.get_tetrahedra_tracer()
    if state["fraction"] is not None:
        rd = plugin._renderer_for(fresh, tracer)
        if state["_tn_train_batches"] is not None:
            rd._tn_train_batches = state["_tn_train_batches"]
        rd._sync_free.fraction = state["fraction"]
    if state["_tn_follow_calls"] is not None:
        tracer._tn_follow_calls = state["_tn_follow_calls"]
    if state["_tn_tet_stats"] is not None:
        object.__setattr__(fresh, "_tn_tet_stats", state["_tn_tet_stats"].clone())
    return fresh


def carry_over(lived, fresh):
    """apply_carried(fresh, carried_state(lived)): for a lived model that is not probed in between"""
    return apply_carried(fresh, carried_state(lived))


def _np(t):
    return np.array(t.detach().cpu().numpy(), order="C", copy=True)           # (a host tensor such as the optimiser's `step` shares its memory)


def _frame(model, rb, out, tag):
    import torch

    model.eval()
    with torch.no_grad():
        res = model(rb)
    for k in ("rgb", "accumulation", "depth", "ray_mask", "expected_depth", "distortion"):
        if k in res:
            out[f"{tag}/{k}"] = _np(res[k])


def probe(tn, model, opt, rays, seed):
    """One fixed sequence of everything the adapter serves, on `model`: {entry: numpy array}.  rays: {"eval": ray bundle (hits and
    misses), "train": ray bundle (every ray hits), "target": f32 [R, 3], "trace": (origins, directions) on the device}."""
    import torch

    cpp = tn.cpp
    out = {}
    _frame(model, rays["eval"], out, "1 frame")
    tracer = model.get_tetrahedra_tracer()
    traced = tracer.trace_rays(*rays["trace"], int(model.config.max_intersected_triangles))
    for k in TRACE_KEYS:
        out[f"2 trace/{k}"] = _np(traced[k])
    for k, v in tracer.tet_quality().items():
        out[f"3 tet_quality/{k}"] = _np(v)
    out["3 delaunay/counters"] = _np(tracer.delaunay_check()["counters"])
    xyz = tracer.tetrahedra_vertices.detach()
    d = xyz - xyz.new_tensor([0.45, 0.55, 0.5])
    values = (d * d).sum(1).contiguous()
    surface = tracer.isosurface(values, float(values.median()))
    for k in ISO_KEYS:
        out[f"4 isosurface/{k}"] = _np(surface[k])
    out["4 isosurface/totals"] = np.array([surface["num_triangles"], surface["num_refs"]], np.int64)
    # one training batch
    torch.manual_seed(seed)
    model.train()
    opt.zero_grad(set_to_none=True)
    before = getattr(model, "_tn_tet_stats", None)
    before = None if before is None else before.clone()
    res = model(rays["train"])
    losses = model.get_loss_dict(res, {"image": rays["target"]})
    loss = sum(losses.values())
    loss.backward()
    out["5 train/loss"] = _np(loss)
    for k, v in sorted(losses.items()):
        out[f"5 train/loss/{k}"] = _np(v)
    out["5 train/rgb"] = _np(res["rgb"])
    for n, p in model.named_parameters():
        if p.grad is not None:
            out[f"5 train/grad/{n}"] = _np(p.grad)
    assert "5 train/grad/tetrahedra_field" in out
    occupancy = getattr(model, "tetrahedra_occupancy", None)
    if occupancy is not None:
        out["5 train/occupancy"] = _np(occupancy)
    after = getattr(model, "_tn_tet_stats", None)
    if after is not None:
        out["5 train/tet_stats_added"] = _np(after - before if before is not None and before.shape == after.shape else after)
    assert getattr(model, "_tn_tet_stats_pending", None) is None
    opt.step()
    for n, p in model.named_parameters():
        out[f"6 step/param/{n}"] = _np(p)
        for k, v in sorted(opt.state.get(p, {}).items()):
            out[f"6 step/{k}/{n}"] = _np(v) if isinstance(v, torch.Tensor) else np.array(v)
    field = model.tetrahedra_field
    out["7 shadow"] = _np(cpp.field_vertex_major(field))
    out["7 shadow/field_t"] = np.ascontiguousarray(_np(field).T)
    _frame(model, rays["eval"], out, "8 frame")
    snapshot = getattr(model.get_tetrahedra_tracer(), "_tn_vertex_snapshot", None)
    if snapshot is not None:
        out["8 state/vertex_snapshot"] = _np(snapshot)
    for k in ("tetrahedra_vertices", "tetrahedra_cells"):
        out[f"8 state/{k}"] = _np(getattr(model, k))
    return out


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.view(np.uint8).reshape(-1)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).reshape(-1)


def compare(a, b):
    """the entries of two probes that are not equal bit for bit: [message per entry]"""
    bad = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            bad.append(f"{k}: only on one side")
        elif a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
            bad.append(f"{k}: {a[k].dtype} {a[k].shape} against {b[k].dtype} {b[k].shape}")
        else:
            diff = np.nonzero(_words(a[k]) != _words(b[k]))[0]
            if len(diff):
                bad.append(f"{k}: {len(diff)} of {a[k].size} words differ (first: {int(diff[0])})")
    return bad


def _rays(scenes, ref, device):
    import torch

    rm, _, _ = _modules()
    o, d = scenes.outside_in_rays(1024, 33)
    po, pd = scenes.pinhole_rays(24, 24, eye=(0.5, 2.6, 0.6), lookat=(0.5, 0.5, 0.5))    # the corners of the image miss the cube
    eo, ed = scenes.outside_in_rays(448, 35)
    eo, ed = np.concatenate([eo, np.asarray(po, np.float32).reshape(-1, 3)]), np.concatenate([ed, np.asarray(pd, np.float32).reshape(-1, 3)])
    to, td = scenes.outside_in_rays(1024, 37)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)   # noqa: E731
    return {"train": rm.ray_bundle(ref, o, d, device, camera_indices=np.arange(len(o)) % 3),
            "eval": rm.ray_bundle(ref, eo, ed, device, camera_indices=np.zeros(len(eo), np.int64)),
            "target": torch.rand(len(o), 3, generator=torch.Generator().manual_seed(5)).to(device),
            "trace": (dev(to), dev(td))}


class _Life:
    """a model, its optimiser and what was recorded of its life"""

    def __init__(self, tn, device, scenes, kind):
        import torch

        rm, plugin, optim = _modules()
        self.tn, self.device, self.scenes, self.kind = tn, device, scenes, kind
        self.ref, self.plugin = rm.load(), plugin
        self.rays = _rays(scenes, self.ref, device)
        pts, cells = scenes.random_mesh(600, 41 if kind == "A" else 43)
        self.pts, self.cells0 = pts, cells
        extra = dict(use_biased_sampler=True) if kind == "B" else {}
        model = rm.build_model(self.ref, pts, cells, num_samples=24, num_fine_samples=24, max_intersected_triangles=256,
                               use_occupancy_field=True, **extra).to(device)
        gen = torch.Generator().manual_seed(9)
        model.tetrahedra_occupancy = torch.rand(len(cells), generator=gen).to(device)     # a plain buffer under the reference's name
        cfg = model.config
        if kind == "A":
            cfg.occupancy_decay, cfg.densify_stats = 0.95, True
            params = [model.tetrahedra_field] + plugin.weights_from_model(model)
        else:
            cfg.position_gradients, cfg.refit_vertices, cfg.vertex_step_fraction = True, True, 0.25
            cfg.delaunay_check_every, cfg.retriangulate_above = 2, RETRIANGULATE_ABOVE
            cfg.distortion_loss_mult, cfg.densify_stats = 1e-2, True
            cfg.occupancy_decay, cfg.occupancy_train_threshold, cfg.occupancy_refresh_every = 0.95, 0.3, 3
            # the vertices in a group of their own, at a rate at which the limiter has something to shorten
            params = [{"params": [model.tetrahedra_field] + plugin.weights_from_model(model)},
                      {"params": [optimise_vertices(model)], "lr": 1e-2}]
        self.model, self.opt = model, optim.FusedRAdam(params, lr=1e-3)
        self.keys = set(model.state_dict())
        self.results, self.log, self.steps = {}, [], 0

    def train(self, n):
        import torch

        model = self.model
        model.train()
        for _ in range(n):
            self.steps += 1
            torch.manual_seed(100 + self.steps)
            self.opt.zero_grad(set_to_none=True)
            before = getattr(model, "_tn_retriangulations", 0)
            out = model(self.rays["train"])
            if getattr(model, "_tn_retriangulations", 0) != before:
                # the monitor gave the vertices new cells inside this call: the statistics of the old cells are gone BEFORE the batch is added
                stats = getattr(model, "_tn_tet_stats", None)
                self.results.setdefault("stats_after_retriangulation", []).append(
                    None if stats is None else (tuple(stats.shape), bool(stats.any()), int(model.tetrahedra_cells.shape[0])))
            sum(model.get_loss_dict(out, {"image": self.rays["target"]}).values()).backward()
            self.opt.step()

    def frame(self):
        import torch

        self.model.eval()
        with torch.no_grad():
            return {k: v.clone() for k, v in self.model(self.rays["eval"]).items()}

    def check_point(self, name):
        """lived against fresh, and fresh against fresh, at this point of the life"""
        model, opt = self.model, self.opt
        assert set(model.state_dict()) == self.keys
        sides = [rebuild(self.ref, model, opt) for _ in range(2)]             # (no tracer yet: see apply_carried)
        state = carried_state(model)
        seed = 1000 + self.steps
        lived = probe(self.tn, model, opt, self.rays, seed)
        self.steps += 1                                                       # (the probe's batch is one more step of the life)
        fresh = [probe(self.tn, apply_carried(m, state), o, self.rays, seed) for m, o in sides]
        self.results[name] = {"lived": lived, "fresh": fresh[0], "fresh2": fresh[1]}
        self.results[name + " attributes"] = {"lived": adapter_attribute_names(model), "fresh": adapter_attribute_names(sides[0][0])}
        self.log.append(f"{self.kind} {name}: V = {model.tetrahedra_vertices.shape[0]}, T = {model.tetrahedra_cells.shape[0]}, "
                        f"{len(lived)} probe entries, step {self.steps}")


# scenario B: the fraction of violated interior faces is 0.065 after the ball of random_mesh(600, 43) was split once and 0.131 after
# it was split twice (geometry.delaunay_face_statement on the unmoved vertices), so the monitor re-triangulates after the SECOND split
RETRIANGULATE_ABOVE = 0.1
CARRIED_PARAMETERS = ("tetrahedra_field", "tetrahedra_vertices")


def _optimiser_rows(model, opt):
    """{parameter name: (step, exp_avg, exp_avg_sq)} of the per-vertex parameters the optimiser holds state for, as numpy copies"""
    import torch

    out = {}
    for name in CARRIED_PARAMETERS:
        p = getattr(model, name)
        state = opt.state.get(p) if isinstance(p, torch.nn.Parameter) else None
        if state:
            out[name] = (float(state["step"]), _np(state["exp_avg"]), _np(state["exp_avg_sq"]))
    return out


def densify_and_check(life, *args, new_moments="mean", retriangulate=False, **kw):
    """plugin.densify on the life's model, then -- before anything else runs on the grown state -- the optimiser's state against
    the numpy statement: `step` kept, both moments of every old vertex kept bit for bit, the moments of a new vertex
    split_vertex_rows_statement's mean of its four parents' (or 0), each moment under its own name.  The parents are read from
    the split's own rule: child 0 overwrites its parent's row with the new vertex in slot 0.  Raises AssertionError."""
    g = sc.geometry()
    model, opt = life.model, life.opt
    before = _optimiser_rows(model, opt)
    old_cells, V = _np(model.tetrahedra_cells), model.tetrahedra_vertices.shape[0]
    res = life.plugin.densify(model, *args, optimizer=opt, new_moments=new_moments, retriangulate=retriangulate, **kw)
    K = res["num_new"]
    after = _optimiser_rows(model, opt)
    assert K > 0 and set(after) == set(before) and before, (K, sorted(before), sorted(after))
    parents = None
    if not retriangulate:
        cells = _np(model.tetrahedra_cells)[:len(old_cells)]
        rows = np.nonzero(cells[:, 0] >= V)[0]                                 # the accepted parents, in the order of their new vertices
        assert len(rows) == K and np.array_equal(cells[rows, 0], V + np.arange(K)), "the split did not number its vertices by accepted rank"
        parents = old_cells[rows]
    for name, (step, m, v) in before.items():
        step2, m2, v2 = after[name]
        assert step2 == step, f"{name}: step {step} became {step2}"
        for what, old, got in (("exp_avg", m, m2), ("exp_avg_sq", v, v2)):
            vertex_major = name == "tetrahedra_vertices"                       # [V, 3]; the field's are [64, V]
            old_rows, got_rows = (old.T, got.T) if vertex_major else (old, got)
            assert got_rows.shape == (old_rows.shape[0], V + K), (name, what, got.shape)
            if new_moments == "zero" or parents is None:
                want = np.concatenate([old_rows, np.zeros((old_rows.shape[0], K), np.float32)], 1)
                assert new_moments == "zero", "a re-triangulating densify is checked with new_moments='zero' only"
            else:
                want = g.split_vertex_rows_statement(np.ascontiguousarray(old_rows), parents, new="mean")
            bad = np.nonzero(sc.bits(np.ascontiguousarray(got_rows)).reshape(-1) != sc.bits(want).reshape(-1))[0]
            assert len(bad) == 0, f"densify: {what} of {name} is not the carried {what}: {len(bad)} of {want.size} words differ (first: {bad[:1]})"
            life.results.setdefault("carried", []).append((name, what, new_moments))
    return res


def _ball(model):
    """bool [T] on the device: the tetrahedra whose centroid lies within RADIUS of the centre"""
    v = model.tetrahedra_vertices.detach()
    centroid = v[model.tetrahedra_cells.long()].double().mean(1)
    return (centroid - CENTRE).norm(dim=1) < RADIUS


def _scenario_a(life):
    model = life.model
    life.train(2)
    before = life.frame()
    res = densify_and_check(life, stats=True, min_hits=1, max_new=40)
    after = life.frame()
    life.results["split"] = res
    life.results["frame_before"], life.results["frame_after"] = before, after
    life.check_point("after the first densify")
    life.train(2)
    res = densify_and_check(life, stats=True, max_new=40, new_moments="zero", retriangulate=True)
    life.results["split2"] = res
    life.train(2)
    life.frame()
    life.check_point("at the end")


def _derived_after_split(model):
    """what `_follow_vertices` remembers, right after a densify: (the snapshot is the new vertex table bit for bit, the key is the
    new table's) -- what a fresh model's first call would remember"""
    import torch

    tracer, v = model.get_tetrahedra_tracer(), model.tetrahedra_vertices
    snapshot = getattr(tracer, "_tn_vertex_snapshot", None)
    return (snapshot is not None and snapshot.shape == v.shape and torch.equal(snapshot.view(torch.int32), v.detach().view(torch.int32)),
            getattr(tracer, "_tn_vertex_key", None) == (v._version, v.data_ptr()), tracer.tetrahedra_vertices is v)


def _scenario_b(life):
    model = life.model
    life.train(3)
    res = densify_and_check(life, _ball(model))
    life.results["split"] = res
    life.results["derived_after_split"] = _derived_after_split(model)
    life.check_point("after the first densify")
    life.train(3)
    life.results["retriangulations_before_second_split"] = getattr(model, "_tn_retriangulations", 0)
    res = densify_and_check(life, _ball(model))
    life.results["split2"] = res
    life.train(3)
    life.frame()
    life.results["retriangulations"] = getattr(model, "_tn_retriangulations", 0)
    life.results["vertex_step_counters"] = model._tn_vertex_step_counters.tolist()
    life.results["delaunay_counters"] = model._tn_delaunay_counters.tolist()
    life.check_point("at the end")


def scenario(tn, device, scenes, kind):
    """The recorded results of scenario "A" (field only) or "B" (moving vertices), run ONCE per session under the deterministic
    field gradient; an exception of the run is recorded and raised again for every test that asks (nothing is run twice)."""
    import pytest

    key = ("scenario", kind)
    if key not in _CACHE:
        _, plugin, _ = _modules()
        life = None
        try:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
                life = _Life(tn, device, scenes, kind)
                plugin.install(life.ref.TetrahedraNerf)
                try:
                    (_scenario_a if kind == "A" else _scenario_b)(life)
                finally:
                    plugin.uninstall(life.ref.TetrahedraNerf)
            life.results["log"] = life.log
            _CACHE[key] = life.results
        except Exception as e:   # noqa: BLE001
            _CACHE[key] = e
    if isinstance(_CACHE[key], Exception):
        raise _CACHE[key]
    return _CACHE[key]
