"""The bf16x3 dX chain, CPU side: the new C-ABI entry (tn_mlp_backward_ex) is declared, bound and exported by the cross-compiled
library, the public surface carries the adjoint mode with fp32 defaults, and the nerfstudio adapter hands
`config.train_adjoint_mode` to render_train -- and nothing when the configuration (the reference's) has no such field.  The
kernel is held to its checks in tests/test_adjoint_x3_gpu.py."""
import importlib
import inspect
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NAME = "tn_mlp_backward_ex"


def test_new_symbol_declared_bound_and_exported():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    text = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", code)
    assert re.search(r"\btn_mlp_backward\s*\(", code)                       # the fp32 entry stays
    assert NAME in _lib.SYMBOLS
    assert "#define TN_ABI_VERSION 6" in text and _lib.ABI_VERSION == 6      # no existing signature changed
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T " + NAME + r"$", exported, flags=re.M)
    assert re.search(r" T tn_mlp_backward$", exported, flags=re.M)
    lib = _lib.load()
    # tn_mlp_backward's arguments + the mode, in front of the stream
    old, new = lib.tn_mlp_backward.argtypes, lib.tn_mlp_backward_ex.argtypes
    assert len(new) == len(old) + 1
    assert list(new[:len(old) - 1]) == list(old[:-1]) and new[-1] is old[-1]
    import ctypes

    assert new[-2] is ctypes.c_int


def test_the_header_no_longer_says_the_chain_has_no_mode():
    text = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert "have no such mode" not in text


def test_public_surface(tn):
    render = importlib.import_module("tetra-nerf_amd.render")
    sig = inspect.signature(tn.cpp.mlp_backward).parameters
    assert sig["adjoint_mode"].default == "fp32" and sig["return_chain"].default is False
    assert inspect.signature(render.TetraRenderer.__init__).parameters["train_adjoint_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.render_train).parameters["adjoint_mode"].default is None
    assert inspect.signature(render.TetraNerfModule.__init__).parameters["train_adjoint_mode"].default == "fp32"
    # the forward's switches keep their defaults
    assert inspect.signature(render.TetraRenderer.__init__).parameters["train_mlp_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.render_train).parameters["mlp_mode"].default is None


@pytest.mark.parametrize("bad", ["bf16", "fp16"])
def test_constructor_rejects_what_is_no_adjoint_arithmetic(bad):
    render = importlib.import_module("tetra-nerf_amd.render")
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        render.TetraRenderer(None, torch.zeros(64, 4), None, train_adjoint_mode=bad, cache_field=False)


@pytest.mark.parametrize("forward", ["fp32", "bf16x3"])
@pytest.mark.parametrize("adjoint", ["fp32", "bf16x3"])
def test_constructor_takes_all_four_combinations(forward, adjoint):
    render = importlib.import_module("tetra-nerf_amd.render")
    rd = render.TetraRenderer(None, torch.zeros(64, 4), None, train_mlp_mode=forward, train_adjoint_mode=adjoint, cache_field=False)
    assert rd.train_mlp_mode == forward and rd.train_adjoint_mode == adjoint


def test_module_hands_the_adjoint_mode_to_its_renderer():
    render = importlib.import_module("tetra-nerf_amd.render")
    m = render.TetraNerfModule(None, 16, num_samples=8, num_fine_samples=8, train_adjoint_mode="bf16x3", cache_field=False)
    rd = m.renderer()
    assert rd.train_adjoint_mode == "bf16x3" and rd.train_mlp_mode == "fp32"
    rd = render.TetraNerfModule(None, 16, num_samples=8, num_fine_samples=8, cache_field=False).renderer()
    assert rd.train_adjoint_mode == "fp32"


class _Recorder:
    """stands in for the TetraRenderer of a model: records what the adapter hands to render_train"""

    def __init__(self):
        self.calls = []
        self.mlp = SimpleNamespace(ray_head_bias=lambda ray_bundle: None)

    def render_train(self, origins, directions, **kw):
        self.calls.append(kw)
        return {"rgb": torch.zeros(len(origins), 3)}


@pytest.mark.parametrize("forward", [None, "bf16x3"])
@pytest.mark.parametrize("field", [None, "bf16x3", "fp32"])
def test_adapter_passes_the_adjoint_mode(monkeypatch, field, forward):
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    rec = _Recorder()
    monkeypatch.setattr(plugin, "_renderer_for", lambda model, tracer: rec)
    cfg = SimpleNamespace(num_samples=8, num_fine_samples=8, background_color="white", use_gradient_scaling=True)
    if field is not None:
        cfg.train_adjoint_mode = field
    if forward is not None:
        cfg.train_mlp_mode = forward
    model = SimpleNamespace(config=cfg, mlp_base=object(), training=True, get_tetrahedra_tracer=lambda: None)
    rb = SimpleNamespace(origins=torch.zeros(5, 3), directions=torch.ones(5, 3))
    out = plugin.fused_get_outputs(model, rb)
    assert tuple(out["rgb"].shape) == (5, 3) and len(rec.calls) == 1
    kw = rec.calls[0]
    if field is None:
        assert "adjoint_mode" not in kw      # the reference's config has no such field: render_train's own default (fp32)
    else:
        assert kw["adjoint_mode"] == field
    # independent of the forward's field
    assert ("mlp_mode" in kw) == (forward is not None)
    assert kw["gradient_scaling"] is True and "position_gradients" not in kw
