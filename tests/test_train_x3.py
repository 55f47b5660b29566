"""The bf16x3 training forward, CPU side: the new C-ABI entry (tn_mlp_forward_gather_train_ex) is declared, bound and
exported by the cross-compiled library, and the nerfstudio adapter hands `config.train_mlp_mode` to render_train -- and
nothing when the configuration (the reference's) has no such field.  The kernel is held to its checks in
tests/test_train_x3_gpu.py."""
import importlib
import inspect
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NAME = "tn_mlp_forward_gather_train_ex"


def test_new_symbol_declared_bound_and_exported():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    text = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", code)
    assert re.search(r"\btn_mlp_forward_gather_train\s*\(", code)           # the fp32 entry stays
    assert NAME in _lib.SYMBOLS
    assert "#define TN_ABI_VERSION 6" in text and _lib.ABI_VERSION == 6      # no existing signature changed
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T " + NAME + r"$", exported, flags=re.M)
    lib = _lib.load()
    # tn_mlp_forward_gather_train's arguments + the mode
    assert len(lib.tn_mlp_forward_gather_train_ex.argtypes) == len(lib.tn_mlp_forward_gather_train.argtypes) + 1


def test_public_surface(tn):
    render = importlib.import_module("tetra-nerf_amd.render")
    assert inspect.signature(tn.cpp.mlp_forward_gather_train).parameters["mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.__init__).parameters["train_mlp_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.render_train).parameters["mlp_mode"].default is None
    assert inspect.signature(render.TetraNerfModule.__init__).parameters["train_mlp_mode"].default == "fp32"
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        render.TetraRenderer(None, torch.zeros(64, 4), None, train_mlp_mode="fp16", cache_field=False)


class _Recorder:
    """stands in for the TetraRenderer of a model: records what the adapter hands to render_train"""

    def __init__(self):
        self.calls = []
        self.mlp = SimpleNamespace(ray_head_bias=lambda ray_bundle: None)

    def render_train(self, origins, directions, **kw):
        self.calls.append(kw)
        return {"rgb": torch.zeros(len(origins), 3)}


@pytest.mark.parametrize("field", [None, "bf16x3", "fp32"])
def test_adapter_passes_the_training_mode(monkeypatch, field):
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    rec = _Recorder()
    monkeypatch.setattr(plugin, "_renderer_for", lambda model, tracer: rec)
    cfg = SimpleNamespace(num_samples=8, num_fine_samples=8, background_color="white", use_gradient_scaling=True)
    if field is not None:
        cfg.train_mlp_mode = field
    model = SimpleNamespace(config=cfg, mlp_base=object(), training=True, get_tetrahedra_tracer=lambda: None)
    rb = SimpleNamespace(origins=torch.zeros(5, 3), directions=torch.ones(5, 3))
    out = plugin.fused_get_outputs(model, rb)
    assert tuple(out["rgb"].shape) == (5, 3) and len(rec.calls) == 1
    kw = rec.calls[0]
    if field is None:
        assert "mlp_mode" not in kw          # the reference's config has no such field: render_train's own default (fp32)
    else:
        assert kw["mlp_mode"] == field
    assert kw["gradient_scaling"] is True and "position_gradients" not in kw
