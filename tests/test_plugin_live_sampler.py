"""config.occupancy_sampler of the nerfstudio plug-in (tetra-nerf_amd/nerfstudio_plugin.py): read with getattr, off when absent; it
reaches render() when the evaluation threshold is set and render_train() on culled batches only -- the unculled refresh batches keep
the ordinary sampler.  CPU part: the keyword arguments a recording renderer receives.  GPU part: a stand-in model around a real
TetraRenderer, the ops counted through monkeypatched wrappers."""
import importlib
from types import SimpleNamespace

import pytest
import torch

from test_occupancy import _stub_model

plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
render = importlib.import_module("tetra-nerf_amd.render")


def _kwargs(config, occupancy, training, batches=1):
    model = _stub_model(config, occupancy)
    model.training = training
    rays = SimpleNamespace(origins=torch.zeros(3, 3), directions=torch.ones(3, 3))
    for _ in range(batches):
        plugin.fused_get_outputs(model, rays)
    assert all(k == ("render_train" if training else "render") for k, _ in model._tn_renderer.calls)
    return [kw for _, kw in model._tn_renderer.calls]


def test_plugin_passes_the_sampler_only_with_its_key_and_only_on_culled_calls():
    occ = torch.zeros(7)
    both = {"occupancy_threshold": 0.1, "occupancy_train_threshold": 0.2, "occupancy_refresh_every": 3}
    # an absent field, False, or no threshold / no buffer: exactly as before
    for config, occupancy in ((both, occ), ({**both, "occupancy_sampler": False}, occ), ({"occupancy_sampler": True}, occ),
                              ({**both, "occupancy_sampler": True}, None)):
        for training in (False, True):
            assert all("occupancy_sampler" not in kw for kw in _kwargs(config, occupancy, training, 4)), (config, training)
    config = {**both, "occupancy_sampler": True}
    (ev,) = _kwargs(config, occ, False)
    assert ev["occupancy_sampler"] is True and ev["occupancy"] is occ and ev["occupancy_threshold"] == 0.1
    for i, kw in enumerate(_kwargs(config, occ, True, 7), 1):
        culled = i % 3 != 0
        assert ("occupancy_threshold" in kw) == culled and (kw.get("occupancy_sampler") is True) == culled, i
    # the evaluation threshold alone does not reach training, nor the training threshold evaluation
    assert "occupancy_sampler" not in _kwargs({"occupancy_threshold": 0.1, "occupancy_sampler": True}, occ, True)[0]
    assert "occupancy_sampler" not in _kwargs({"occupancy_train_threshold": 0.2, "occupancy_sampler": True}, occ, False)[0]


@pytest.mark.gpu
def test_plugin_routes_through_the_live_sampler_ops(tn, device, scenes, monkeypatch):
    pts, cells = scenes.random_mesh(600, 3)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(96, 4)
    rays = SimpleNamespace(origins=torch.from_numpy(o).to(device), directions=torch.from_numpy(d).to(device))
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(device)
    mlp.ray_head_bias = lambda ray_bundle: None
    field = (torch.randn(64, len(pts), device=device) * 0.5).requires_grad_(True)
    occ = torch.rand(len(cells), generator=torch.Generator().manual_seed(2)).to(device)
    counts = {"sample_live": 0, "live_to_distance": 0, "sample_coarse": 0}
    for name in counts:
        real = getattr(tn.cpp, name)
        monkeypatch.setattr(tn.cpp, name, (lambda real, name: lambda *a, **k: (counts.__setitem__(name, counts[name] + 1), real(*a, **k))[1])(real, name))

    def model_for(**config):
        model = SimpleNamespace(config=SimpleNamespace(background_color="white", **config), mlp_base=object(), training=False,
                                tetrahedra_field=field, tetrahedra_occupancy=occ, get_tetrahedra_tracer=lambda: tr)
        model._tn_renderer = render.TetraRenderer(tr, field, mlp, 9, 256, num_fine_samples=5)
        return model

    def run(model, training):
        before = dict(counts)
        model.training = training
        out = plugin.fused_get_outputs(model, rays)
        assert bool(torch.isfinite(out["rgb"]).all())
        if training:
            out["rgb"].sum().backward()
        return {k: counts[k] - before[k] for k in counts}

    config = dict(occupancy_threshold=0.5, occupancy_train_threshold=0.5, occupancy_refresh_every=3)
    off = model_for(**config)
    assert run(off, False)["sample_live"] == 0 and run(off, True) == {"sample_live": 0, "live_to_distance": 0, "sample_coarse": 1}
    on = model_for(occupancy_sampler=True, **config)
    # evaluation: one sampler call, the bin centres of both passes and the depth through the map
    assert run(on, False) == {"sample_live": 1, "live_to_distance": 3, "sample_coarse": 0}
    for batch in (1, 2, 3, 4):
        got = run(on, True)
        if batch % 3 == 0:       # the unculled refresh batch keeps the ordinary sampler
            assert got == {"sample_live": 0, "live_to_distance": 0, "sample_coarse": 1}, batch
        else:
            assert got == {"sample_live": 1, "live_to_distance": 3, "sample_coarse": 0}, batch
