"""Occupancy-culled training on the CPU: the ABI additions, the PyTorch statement of culled training
(render_train(fused=False, occupancy_threshold=): the oracle of the fused path) against a by-hand masked run, the argument rules,
and the nerfstudio adapter's wiring.  The kernels: tests/test_train_culled_gpu.py."""
import ctypes
import importlib
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from test_occupancy import _stub_model, scene   # noqa: F401  (the CPU scene and the recording renderer of the occupancy tests)

ROOT = Path(__file__).resolve().parents[1]
render = importlib.import_module("tetra-nerf_amd.render")
NEW = ("tn_mlp_forward_gather_train_indexed", "tn_mlp_param_grads_indexed", "tn_mlp_ray_head_grad_indexed", "tn_compact_rows")


def test_abi_additions_keep_version_6():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/tetranerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the shared library"
        assert name in _lib.SYMBOLS
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "model.py:98-99,256-265" in comment, name
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header)
    assert _lib.ABI_VERSION == 6 and lib.tn_abi_version() == 6


def _renderer(sc, S, S_fine, tracer=None, mlp=None, **kw):
    return render.TetraRenderer(tracer or sc.tracer, sc.field, mlp or sc.mlp, S, 256, num_fine_samples=S_fine, cache_field=False,
                                device_samplers=False, interpolate_values=sc.interp, **kw)


def _params(sc):
    return [sc.field] + list(sc.mlp.parameters())


def _step(sc, rd, rand, target, **kw):
    """outputs and autograd gradients (field + the twelve MLP tensors; None -> zeros) of one unfused training call.  (Deterministic
    algorithms: the gather's backward is an accumulating index_put, whose order of additions otherwise changes from run to run --
    two runs of the SAME call then differ in the field gradient's last bits.)"""
    sc.field.requires_grad_(True)
    for p in _params(sc):
        p.grad = None
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        out = rd.render_train(sc.o, sc.d, rand=rand, fused=False, **kw)
        loss = ((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()
        loss.backward()
    finally:
        torch.use_deterministic_algorithms(before)
    grads = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in _params(sc)]
    return {k: v.detach() for k, v in out.items()}, grads


@pytest.mark.parametrize("S,S_fine", [(13, 0), (9, 7)])
def test_unfused_culled_training_equals_a_masked_run(scene, S, S_fine):
    sc = scene
    hit = int((sc.tracer.trace_rays(sc.o, sc.d, 256)["num_visited_cells"] > 0).sum())
    g = torch.Generator().manual_seed(3)
    rand = {"coarse": torch.rand(hit, S + 1, generator=g), "fine": torch.rand(hit, S_fine + 1, generator=g)}
    target = torch.rand(len(sc.o), 3, generator=g)
    occ = torch.rand(sc.T, generator=torch.Generator().manual_seed(1))
    thr = 0.5

    plain, g_plain = _step(sc, _renderer(sc, S, S_fine), rand, target)
    # threshold 0 culls nothing: the plain call
    zero, g_zero = _step(sc, _renderer(sc, S, S_fine), rand, target, occupancy=occ, occupancy_threshold=0.0)
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(zero[k], plain[k]), k
    assert all(torch.equal(a, b) for a, b in zip(g_zero, g_plain))
    # the renderer's own threshold is the default of the argument
    dflt, _ = _step(sc, _renderer(sc, S, S_fine, train_occupancy_threshold=thr), rand, target, occupancy=occ)
    # a threshold above every occupancy: the background frame, and no gradient at all
    empty, g_empty = _step(sc, _renderer(sc, S, S_fine), rand, target, occupancy=occ, occupancy_threshold=2.0)
    assert torch.all(empty["accumulation"] == 0.0) and torch.all(empty["rgb"] == 1.0)
    assert all(not x.any() for x in g_empty)

    # mixed: the same function on a tracer that records the culled samples of each pass and an MLP that masks with them
    seen = []

    class Recording:
        def trace_rays(self, *a):
            return sc.tracer.trace_rays(*a)

        def find_visited_cells(self, *a, **kw):
            out = sc.tracer.find_visited_cells(*a, **kw)
            seen.append(render.cull_mask_statement(out["cell_indices"], occ, thr))
            return out

    class Masked:
        def fused_weights(self):
            return render.mlp_weights(sc.mlp)

        def coarse_sigma(self, feats):
            return torch.where(seen[-1], torch.zeros(()), render.coarse_sigma(sc.mlp, feats))

        def __call__(self, feats, dirs):
            sigma, col = sc.mlp(feats, dirs)
            m = seen[-1][..., None]
            return torch.where(m, torch.zeros(()), sigma), torch.where(m, torch.zeros(()), col)

    by_hand, g_hand = _step(sc, _renderer(sc, S, S_fine, tracer=Recording(), mlp=Masked()), rand, target)
    assert len(seen) == (2 if S_fine else 1) and all(0 < int(m.sum()) < m.numel() for m in seen)
    cap = {}
    mixed, g_mixed = _step(sc, _renderer(sc, S, S_fine), rand, target, occupancy=occ, occupancy_threshold=thr, capture=cap)
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(mixed[k], by_hand[k]), k
        assert torch.equal(dflt[k], mixed[k]), k
    assert all(torch.equal(a, b) for a, b in zip(g_mixed, g_hand))
    assert not torch.equal(mixed["rgb"], plain["rgb"]) and any(x.any() for x in g_mixed)
    assert torch.equal(cap["culled"], seen[-1]) and cap["cell_indices"].shape == seen[-1].shape
    # the occupancy itself is an input, not a parameter: untouched without a decay
    assert torch.equal(occ, torch.rand(sc.T, generator=torch.Generator().manual_seed(1)))


def test_argument_rules(scene):
    sc = scene
    rd = _renderer(sc, 8, 0)
    occ = torch.zeros(sc.T)
    with pytest.raises(RuntimeError, match="occupancy_threshold needs the occupancy"):
        rd.render_train(sc.o, sc.d, occupancy_threshold=0.5)
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render_train(sc.o, sc.d, occupancy=occ)
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render_train(sc.o, sc.d, occupancy_decay=0.9)
    # the update is a kernel of the fused path, with or without a threshold
    with pytest.raises(RuntimeError, match="fused path"):
        rd.render_train(sc.o, sc.d, fused=False, occupancy=occ, occupancy_decay=0.9)
    with pytest.raises(RuntimeError, match="fused path"):
        rd.render_train(sc.o, sc.d, fused=False, occupancy=occ, occupancy_decay=0.9, occupancy_threshold=0.5)
    # the renderer's default threshold does not turn a call without an occupancy into an error
    with torch.no_grad():
        _renderer(sc, 8, 0, train_occupancy_threshold=0.5).render_train(sc.o, sc.d, fused=False)
    assert rd.train_occupancy_threshold is None


def test_plugin_passes_the_training_threshold_only_with_its_own_key_and_not_on_refresh_batches():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    rays = SimpleNamespace(origins=torch.zeros(3, 3), directions=torch.ones(3, 3))
    occ = torch.zeros(7)
    occ_keys = {"occupancy", "occupancy_threshold", "occupancy_decay"}

    def train_calls(config, occupancy, batches):
        model = _stub_model(config, occupancy)
        model.training = True
        for _ in range(batches):
            plugin.fused_get_outputs(model, rays)
        assert all(k == "render_train" for k, _ in model._tn_renderer.calls)
        return [kw for _, kw in model._tn_renderer.calls]

    # the evaluation threshold stays evaluation only; without the buffer nothing is passed
    for config, occupancy in (({"occupancy_threshold": 0.1}, occ), ({"occupancy_train_threshold": 0.2}, None),
                              ({"occupancy_train_threshold": None}, occ)):
        assert all(not occ_keys & set(kw) for kw in train_calls(config, occupancy, 3)), config
    # the new key: threshold without a decay; every 16th batch of the renderer runs unculled
    kws = train_calls({"occupancy_train_threshold": 0.2}, occ, 33)
    for i, kw in enumerate(kws, 1):
        if i % 16 == 0:
            assert not occ_keys & set(kw), i
        else:
            assert kw["occupancy"] is occ and kw["occupancy_threshold"] == 0.2 and "occupancy_decay" not in kw, i
    # with a decay: the refresh batches still update
    kws = train_calls({"occupancy_train_threshold": 0.2, "occupancy_decay": 0.9, "occupancy_refresh_every": 3}, occ, 7)
    for i, kw in enumerate(kws, 1):
        assert kw["occupancy"] is occ and kw["occupancy_decay"] == 0.9
        assert ("occupancy_threshold" in kw) == (i % 3 != 0), i
    # below 1: never refreshed
    assert all("occupancy_threshold" in kw for kw in train_calls({"occupancy_train_threshold": 0.2, "occupancy_refresh_every": 0}, occ, 5))
    # an evaluation call of such a model is not culled by the training key
    model = _stub_model({"occupancy_train_threshold": 0.2}, occ)
    plugin.fused_get_outputs(model, rays)
    assert model._tn_renderer.calls[0][0] == "render" and not occ_keys & set(model._tn_renderer.calls[0][1])
