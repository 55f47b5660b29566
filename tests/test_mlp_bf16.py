"""The plain-bf16 evaluation arithmetic of the fused MLP (mlp_mode="bf16", C-ABI mode 2), CPU side: the mode's name and number,
the entry points that must refuse it, the header's mode table, what the nerfstudio adapter hands to render(), and the
statement of the arithmetic itself (render.mlp_forward_bf16_statement) in float32 against float64.  The kernel is held to the
statement in tests/test_mlp_bf16_gpu.py."""
import importlib
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def render():
    return importlib.import_module("tetra-nerf_amd.render")


def test_mode_name_and_number(tn):
    assert tn.cpp._mode("bf16") == 2 and tn.cpp._mode(2) == 2
    assert tn.cpp._mode("fp32") == 0 and tn.cpp._mode("bf16x3") == 1      # (the other two stay where they were)


def test_training_and_one_launch_entry_points_refuse_it(tn, render):
    # the mode is looked at before any tensor is: nothing below needs a device
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        tn.cpp.mlp_forward_gather_train(None, None, None, None, [], 1, mode="bf16")
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        tn.cpp.render_rays(None, None, None, None, None, [], 8, mode="bf16")
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        render.TetraRenderer(None, torch.zeros(64, 4), None, train_mlp_mode="bf16", cache_field=False)
    rd = render.TetraRenderer(None, torch.zeros(64, 4), None, mlp_mode="bf16", cache_field=False)      # render()'s: accepted
    assert rd.mlp_mode == "bf16" and rd.train_mlp_mode == "fp32"
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        rd.render_train(torch.zeros(1, 3), torch.ones(1, 3), mlp_mode="bf16")
    with pytest.raises(RuntimeError, match='"bf16"'):          # ... and the message names the mode
        rd.render_train(torch.zeros(1, 3), torch.ones(1, 3), mlp_mode="bf16")
    assert not rd._one_launch_ok("bf16")                       # render() takes the kernel chain for it
    assert inspect.signature(render.TetraRenderer.render).parameters["mlp_mode"].default is None


def test_header_documents_mode_2_and_keeps_the_abi_version():
    text = (ROOT / "include" / "tetranerf_hip.h").read_text()
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    assert "#define TN_ABI_VERSION 6" in text and _lib.ABI_VERSION == 6
    table = text[text.index("Arithmetic `mode` of the two forward entry points"):text.index("int tn_mlp_forward(")]
    rows = re.findall(r"^ \*   (\d)  ", table, flags=re.M)
    assert rows == ["0", "1", "2"], rows
    third = table[table.index(" *   2  "):]
    for word in ("bf16", "round to nearest even", "accumulated in fp32", "reject mode 2"):
        assert word in third, word


class _Recorder:
    """stands in for the TetraRenderer of a model: records what the adapter hands to render / render_train"""

    def __init__(self):
        self.calls = []
        self.mlp = SimpleNamespace(ray_head_bias=lambda ray_bundle: None)

    def render(self, origins, directions, **kw):
        self.calls.append(("render", kw))
        return {"rgb": torch.zeros(len(origins), 3)}

    def render_train(self, origins, directions, **kw):
        self.calls.append(("render_train", kw))
        return {"rgb": torch.zeros(len(origins), 3)}


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("field", [None, "bf16", "fp32"])
def test_adapter_passes_the_evaluation_mode(monkeypatch, field, training):
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    rec = _Recorder()
    monkeypatch.setattr(plugin, "_renderer_for", lambda model, tracer: rec)
    cfg = SimpleNamespace(num_samples=8, num_fine_samples=8, background_color="white", use_gradient_scaling=True)
    if field is not None:
        cfg.eval_mlp_mode = field
    model = SimpleNamespace(config=cfg, mlp_base=object(), training=training, get_tetrahedra_tracer=lambda: None)
    rb = SimpleNamespace(origins=torch.zeros(5, 3), directions=torch.ones(5, 3))
    out = plugin.fused_get_outputs(model, rb)
    assert tuple(out["rgb"].shape) == (5, 3) and len(rec.calls) == 1
    name, kw = rec.calls[0]
    if training:
        assert name == "render_train" and "mlp_mode" not in kw      # the evaluation mode never reaches a training step
    elif field is None:
        assert name == "render" and "mlp_mode" not in kw            # the reference's config has no such field: render()'s default
    else:
        assert name == "render" and kw["mlp_mode"] == field


def test_statement_in_float32_agrees_with_float64(render):
    """The statement pins both roundings and leaves the order of the fp32 sums open: float64 sums are what every order
    approximates, float32 sums (torch's order on the CPU) are one of them.  The two agree as the kernel has to agree with the
    float64 form (tests/test_mlp_bf16_gpu.py, whole network): at most 0.2 % of the samples beyond 1e-5 (1 + |sigma|) on sigma or
    1e-5 on rgb -- an activation whose fp32 value sits on a bf16 rounding boundary may land on the neighbouring bf16 value --
    and none beyond 1e-3.  And the statement is not the fp32 network: its rgb differs from TetraMLP's by far more than that."""
    torch.manual_seed(21)
    mlp = render.TetraMLP()
    R, S = 64, 128
    torch.manual_seed(22)
    feats = torch.randn(R * S, 64) * 0.5
    dirs = torch.nn.functional.normalize(torch.randn(R, 3), dim=-1)[:, None, :].expand(R, S, 3).reshape(-1, 3)
    bias = (torch.randn(R, 128) * 0.7)[:, None, :].expand(R, S, 128).reshape(-1, 128)
    with torch.no_grad():
        for hb in (None, bias):
            s64, c64 = render.mlp_forward_bf16_statement(mlp, feats, dirs, hb)
            s32, c32 = render.mlp_forward_bf16_statement(mlp, feats, dirs, hb, dtype=torch.float32)
            assert s64.dtype == torch.float64 and s32.dtype == torch.float32 and tuple(c64.shape) == (R * S, 3)
            ds = (s32.double() - s64).abs()[:, 0]
            dc = (c32.double() - c64).abs().max(-1).values
            out = (ds > 1e-5 * (1 + s64[:, 0].abs())) | (dc > 1e-5)
            print(f"statement fp32 vs float64: outside 1e-5: {float(out.double().mean()):.2e} of the samples, "
                  f"max sigma {float(ds.max()):.2e}, max rgb {float(dc.max()):.2e}")
            assert float(out.double().mean()) <= 2e-3
            assert float(ds.max()) <= 1e-3 and float(dc.max()) <= 1e-3
        _, plain = mlp(feats, dirs)
        _, c64 = render.mlp_forward_bf16_statement(mlp, feats, dirs)
        assert float((plain.double() - c64).abs().mean()) > 1e-5        # (the rounding acts)
        assert float((plain.double() - c64).abs().max()) < 1e-2         # ... at the size bf16 operands explain
        # a zero ray_head_bias is no bias
        z64 = render.mlp_forward_bf16_statement(mlp, feats, dirs, torch.zeros_like(bias))[1]
        assert torch.equal(z64, c64)


def test_unit_roundoff_of_the_a_priori_bound(render):
    """The a-priori bound of tests/test_mlp_bf16_gpu.py::test_one_layer_a_priori_accuracy, on the STATEMENT (no kernel): one layer
    y = W x + b with both operands rounded to bf16, re-rounded once behind it, against the unrounded float64 layer.  With the unit
    roundoff of bf16 under round to nearest even, u = 2^-8 (8 significant bits), the bound (2u + u^2) sum|W x| + 65 * 2^-24 (...) +
    u |y| holds; with 2^-9 -- the figure of a 9-bit format, which the request for this mode named -- the statement itself exceeds
    it wherever the re-rounding term dominates.  This pins which constant the GPU test may use."""
    torch.manual_seed(12)
    n = 4096
    x = torch.randn(n, 64, dtype=torch.float64).float().double()
    x[::7] *= 1e-30            # rows whose products vanish: y = b, and the bound is the re-rounding term alone
    w = torch.randn(64, dtype=torch.float64).float().double()
    shift = float((x @ w).abs().max()) * 1.25 + 1.0
    b = torch.tensor(shift, dtype=torch.float64).float().double()
    y = render.bf16_round(render.bf16_round(x) @ render.bf16_round(w) + b)        # the layer, then the next layer's input rounding
    exact = x @ w + b
    mag = (x * w).abs().sum(1)
    ratio = {}
    for p in (8, 9):
        u = 2.0 ** -p
        bound = (2 * u + u * u) * mag + 65 * 2.0 ** -24 * ((1 + u) ** 2 * mag + float(b)) + u * exact.abs()
        ratio[p] = float(((y - exact).abs() / bound).max())
    assert ratio[8] <= 1.0 < ratio[9], ratio
