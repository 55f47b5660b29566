"""config.aux_outputs / config.distortion_loss_mult of the nerfstudio plug-in (tetra-nerf_amd/nerfstudio_plugin.py): read with
getattr, off when absent.  CPU part: the keyword arguments a recording renderer receives, the wrapped get_loss_dict and the
(un)installation, on stand-in models.  GPU part: a stand-in model around a real TetraRenderer."""
import importlib
from types import SimpleNamespace

import pytest
import torch

from test_occupancy import _stub_model

plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
render = importlib.import_module("tetra-nerf_amd.render")
RAYS = SimpleNamespace(origins=torch.zeros(3, 3), directions=torch.ones(3, 3))


def _kwargs(config, training):
    model = _stub_model(config, None)
    model.training = training
    plugin.fused_get_outputs(model, RAYS)
    ((name, kw),) = model._tn_renderer.calls
    assert name == ("render_train" if training else "render")
    return kw


class _Reference:
    """A model class with the reference's two methods, as install() finds them."""

    def __init__(self, **config):
        self.config = SimpleNamespace(**config)

    def get_outputs(self, ray_bundle):
        return {"rgb": torch.zeros(2, 3)}

    def get_loss_dict(self, outputs, batch, metrics_dict=None):
        return {"rgb_loss": torch.tensor(1.5), "seen": (outputs, batch, metrics_dict)}


def test_plugin_passes_aux_outputs_only_when_asked():
    for training in (False, True):
        for config in ({}, {"aux_outputs": False}, {"aux_outputs": None, "distortion_loss_mult": None}):
            assert "aux_outputs" not in _kwargs(config, training), (config, training)
        for config in ({"aux_outputs": True}, {"distortion_loss_mult": 0.01}, {"aux_outputs": False, "distortion_loss_mult": 0.0}):
            assert _kwargs(config, training)["aux_outputs"] is True, (config, training)


def test_install_wraps_get_loss_dict_and_uninstall_restores_both():
    class Model(_Reference):
        pass

    ref_outputs, ref_loss = Model.get_outputs, Model.get_loss_dict
    assert plugin.install(Model) is Model and plugin.install(Model) is Model        # idempotent
    assert Model.get_outputs is plugin.fused_get_outputs and Model.get_loss_dict is plugin.fused_get_loss_dict
    assert Model._tn_reference_get_loss_dict is ref_loss
    outputs, batch = {"rgb": torch.zeros(4, 3), "distortion": torch.tensor([[1.0], [3.0]])}, {"image": 1}
    # fields absent: the reference's dictionary, the very object, unchanged
    got = Model().get_loss_dict(outputs, batch, {"m": 2})
    assert set(got) == {"rgb_loss", "seen"} and got["seen"][0] is outputs and got["seen"][1] is batch and got["seen"][2] == {"m": 2}
    # the multiplier without the output (a configuration that fell back to the reference body): unchanged as well
    assert set(Model(distortion_loss_mult=0.01).get_loss_dict({"rgb": outputs["rgb"]}, batch)) == {"rgb_loss", "seen"}
    assert set(Model(aux_outputs=True).get_loss_dict(outputs, batch)) == {"rgb_loss", "seen"}
    got = Model(distortion_loss_mult=0.01).get_loss_dict(outputs, batch)
    assert set(got) == {"rgb_loss", "seen", "distortion_loss"} and float(got["distortion_loss"]) == pytest.approx(0.02) and float(got["rgb_loss"]) == 1.5
    plugin.uninstall(Model)
    assert Model.get_outputs is ref_outputs and Model.get_loss_dict is ref_loss
    assert set(Model(distortion_loss_mult=0.01).get_loss_dict(outputs, batch)) == {"rgb_loss", "seen"}
    # and the subclass form
    Fused = plugin.make_fused_model_class(_Reference)
    assert _Reference.get_loss_dict is ref_loss or _Reference.get_loss_dict.__qualname__ == ref_loss.__qualname__
    got = Fused(distortion_loss_mult=2.0).get_loss_dict(outputs, batch)
    assert float(got["distortion_loss"]) == pytest.approx(4.0) and set(Fused().get_loss_dict(outputs, batch)) == {"rgb_loss", "seen"}


@pytest.mark.gpu
def test_plugin_outputs_and_distortion_loss_on_a_real_renderer(tn, device, scenes):
    pts, cells = scenes.random_mesh(600, 3)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(96, 4)
    rays = SimpleNamespace(origins=torch.from_numpy(o).to(device), directions=torch.from_numpy(d).to(device))
    torch.manual_seed(1)
    mlp = render.TetraMLP().to(device)
    mlp.ray_head_bias = lambda ray_bundle: None
    field = (torch.randn(64, len(pts), device=device) * 0.5).requires_grad_(True)

    class Model(_Reference):
        def __init__(self, **config):
            super().__init__(background_color="white", **config)
            self.mlp_base, self.training, self.tetrahedra_field = object(), False, field
            self._tn_renderer = render.TetraRenderer(tr, field, mlp, 9, 256, num_fine_samples=5)

        def get_tetrahedra_tracer(self):
            return tr

    plugin.install(Model)
    try:
        keys = {"rgb", "accumulation", "depth", "ray_mask"}
        for training in (False, True):
            off, on = Model(), Model(aux_outputs=True)
            off.training = on.training = training
            assert set(off.get_outputs(rays)) == keys                                   # fields absent: exactly the keys of before
            out = on.get_outputs(rays)
            assert set(out) == keys | {"expected_depth", "distortion"}
            assert out["expected_depth"].shape == out["distortion"].shape == (96, 1)
            assert set(on.get_loss_dict(out, {})) == {"rgb_loss", "seen"}
        model = Model(distortion_loss_mult=0.01)
        model.training = True
        out = model.get_outputs(rays)
        loss = model.get_loss_dict(out, {})
        assert set(loss) == {"rgb_loss", "seen", "distortion_loss"}
        assert float(out["distortion"].mean()) > 0
        assert float(loss["distortion_loss"]) == pytest.approx(0.01 * float(out["distortion"].mean()), rel=1e-6)
        field.grad = None
        loss["distortion_loss"].backward()
        assert field.grad is not None and bool(torch.isfinite(field.grad).all()) and float(field.grad.abs().max()) > 0
    finally:
        plugin.uninstall(Model)
        field.grad = None
