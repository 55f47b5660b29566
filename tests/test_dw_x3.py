"""The bf16x3 weight-gradient GEMMs, CPU side: the new C-ABI entry (tn_mlp_param_grads_ex) is declared, documented, bound and
exported by the cross-compiled library; the public surface carries the third switch with fp32 defaults; the adapter hands
`config.train_dw_mode` to render_train and nothing when the configuration has no such field; and the a-priori bound of the
arithmetic -- |six-product sum - a b| <= 2^-21 |a| |b| -- holds, emulated in torch, on the operand tensors
tests/test_dw_x3_gpu.py uploads (tests/dw_x3_cases.py builds them from seeds for both files).  That last check passes with or
without the kernel: it checks the yardstick the GPU test uses, not the code.

(The GPU test also runs on the buffers a real training forward and dX chain left, which do not exist without a GPU; the
"random" fill of the helper has their magnitudes and sparsity and is run by both files.)"""
import ctypes
import importlib
import inspect
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import dw_x3_cases as cases

ROOT = Path(__file__).resolve().parents[1]
NAME = "tn_mlp_param_grads_ex"


def test_header_declares_and_documents_the_entry_and_mode_1():
    text = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", code)
    assert re.search(r"\btn_mlp_param_grads\s*\(", code)                    # the fp32 entry stays
    # the comment in front of the declaration: what it replaces, and the arithmetic of mode 1
    doc = re.findall(r"/\*(.*?)\*/\s*int\s+" + NAME + r"\s*\(", text, flags=re.S)
    assert len(doc) == 1
    doc = " ".join(doc[0].split())
    assert "mode 0 (fp32 MFMA) IS tn_mlp_param_grads" in doc
    assert "mode 1 (bf16x3 MFMA)" in doc and "three bf16 pieces" in doc and "six products" in doc
    assert "mode 2" in doc
    assert "#define TN_ABI_VERSION 6" in text                                # no existing signature changed


def test_symbol_bound_and_exported():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    assert NAME in _lib.SYMBOLS and _lib.ABI_VERSION == 6
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T " + NAME + r"$", exported, flags=re.M)
    assert re.search(r" T tn_mlp_param_grads$", exported, flags=re.M)
    lib = _lib.load()
    # tn_mlp_param_grads' arguments + the mode, in front of the stream
    old, new = lib.tn_mlp_param_grads.argtypes, lib.tn_mlp_param_grads_ex.argtypes
    assert len(new) == len(old) + 1
    assert list(new[:len(old) - 1]) == list(old[:-1]) and new[-1] is old[-1]
    assert new[-2] is ctypes.c_int


def test_public_surface(tn):
    render = importlib.import_module("tetra-nerf_amd.render")
    assert inspect.signature(tn.cpp.mlp_backward).parameters["dw_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.__init__).parameters["train_dw_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.render_train).parameters["dw_mode"].default is None
    assert inspect.signature(render.TetraNerfModule.__init__).parameters["train_dw_mode"].default == "fp32"
    # the other two switches keep their defaults
    assert inspect.signature(tn.cpp.mlp_backward).parameters["adjoint_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.__init__).parameters["train_adjoint_mode"].default == "fp32"
    assert inspect.signature(render.TetraRenderer.__init__).parameters["train_mlp_mode"].default == "fp32"


@pytest.mark.parametrize("bad", ["bf16", "fp16"])
def test_constructor_rejects_what_is_no_training_arithmetic(bad):
    render = importlib.import_module("tetra-nerf_amd.render")
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        render.TetraRenderer(None, torch.zeros(64, 4), None, train_dw_mode=bad, cache_field=False)


@pytest.mark.parametrize("forward", ["fp32", "bf16x3"])
@pytest.mark.parametrize("adjoint", ["fp32", "bf16x3"])
@pytest.mark.parametrize("dw", ["fp32", "bf16x3"])
def test_constructor_takes_all_eight_combinations(forward, adjoint, dw):
    render = importlib.import_module("tetra-nerf_amd.render")
    rd = render.TetraRenderer(None, torch.zeros(64, 4), None, train_mlp_mode=forward, train_adjoint_mode=adjoint, train_dw_mode=dw,
                              cache_field=False)
    assert (rd.train_mlp_mode, rd.train_adjoint_mode, rd.train_dw_mode) == (forward, adjoint, dw)


def test_module_hands_the_dw_mode_to_its_renderer():
    render = importlib.import_module("tetra-nerf_amd.render")
    rd = render.TetraNerfModule(None, 16, num_samples=8, num_fine_samples=8, train_dw_mode="bf16x3", cache_field=False).renderer()
    assert rd.train_dw_mode == "bf16x3" and rd.train_adjoint_mode == "fp32" and rd.train_mlp_mode == "fp32"
    rd = render.TetraNerfModule(None, 16, num_samples=8, num_fine_samples=8, cache_field=False).renderer()
    assert rd.train_dw_mode == "fp32"


def test_the_autograd_node_is_absent_safe(tn, monkeypatch):
    """the nodes read their trailing modes by position: none, one or two of them leave the weight-gradient mode at fp32, a third
    one is the weight-gradient mode (run on recorders of the ops: tests/test_mlp_node_modes.py)"""
    import test_mlp_node_modes as nodes

    calls = nodes.install_recorders(tn.cpp, monkeypatch)
    for node in ("dense", "indexed"):
        for trailing in ((), ("bf16x3",), ("bf16x3", "bf16x3")):
            assert nodes.run_node(tn, calls, node, trailing, bias=False)[2] == "fp32"
        assert nodes.run_node(tn, calls, node, ("fp32", "fp32", "bf16x3"), bias=False) == ("fp32", "fp32", "bf16x3")


class _Recorder:
    """stands in for the TetraRenderer of a model: records what the adapter hands to render_train"""

    def __init__(self):
        self.calls = []
        self.mlp = SimpleNamespace(ray_head_bias=lambda ray_bundle: None)

    def render_train(self, origins, directions, **kw):
        self.calls.append(kw)
        return {"rgb": torch.zeros(len(origins), 3)}


@pytest.mark.parametrize("adjoint", [None, "bf16x3"])
@pytest.mark.parametrize("field", [None, "bf16x3", "fp32"])
def test_adapter_passes_the_dw_mode(monkeypatch, field, adjoint):
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    assert "`train_dw_mode`" in plugin.__doc__
    rec = _Recorder()
    monkeypatch.setattr(plugin, "_renderer_for", lambda model, tracer: rec)
    cfg = SimpleNamespace(num_samples=8, num_fine_samples=8, background_color="white", use_gradient_scaling=True)
    if field is not None:
        cfg.train_dw_mode = field
    if adjoint is not None:
        cfg.train_adjoint_mode = adjoint
    model = SimpleNamespace(config=cfg, mlp_base=object(), training=True, get_tetrahedra_tracer=lambda: None)
    rb = SimpleNamespace(origins=torch.zeros(5, 3), directions=torch.ones(5, 3))
    plugin.fused_get_outputs(model, rb)
    kw = rec.calls[0]
    if field is None:
        assert "dw_mode" not in kw          # the reference's config has no such field: render_train's own default (fp32)
    else:
        assert kw["dw_mode"] == field
    assert ("adjoint_mode" in kw) == (adjoint is not None) and "mlp_mode" not in kw


# ---- the yardstick: the emulated arithmetic on the operands of the GPU test
BOUND_CASES = [("small", 3, 7), ("a_mid", 3, 7), ("b_mid", 3, 7), ("mid_mid", 3, 7), ("one_last", 3, 7), ("random", 3, 7),
               ("a_mid", 37, 97), ("b_mid", 37, 97), ("random", 37, 97), ("random", 300, 257)]


@pytest.mark.parametrize("kind,R,S", BOUND_CASES, ids=[f"{k}-{R}x{S}" for k, R, S in BOUND_CASES])
def test_six_products_stay_inside_the_a_priori_bound(kind, R, S):
    """every product a b the four GEMMs form on this fill (all feature pairs of up to 64 samples spread over the chunk, the last
    one included): |sum of the six partial products - a b| <= 2^-21 |a| |b|, in float64; on the integer fills the six products
    are the product exactly"""
    f = cases.fill(kind, R, S)
    n = R * S
    rows = torch.unique(torch.cat([torch.linspace(0, n - 1, min(n, 64)).round().long(), torch.tensor([n - 1])]))
    worst = 0.0
    for a_name, b_name in cases.PAIRS:
        a, b = f[a_name][rows][:, :, None], f[b_name][rows][:, None, :]
        exact = a.double() * b.double()
        err = (cases.six_products(a, b) - exact).abs()
        bound = 2.0 ** -21 * exact.abs()
        assert bool((err <= bound).all()), (a_name, b_name)
        if kind != "random":
            assert float(err.max()) == 0.0, (a_name, b_name)
        nz = exact != 0
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / exact.abs()[nz]).max()))
    print(f"{kind} {R}x{S}: max |six products - a b| / |a b| = {worst:.3e} (bound 2^-21 = {2.0 ** -21:.3e})")
    if kind == "random":
        assert worst > 0        # (the split did drop something: the check is not vacuous)


@pytest.mark.parametrize("kind", ["a_mid", "b_mid", "mid_mid"])
def test_the_integer_fills_force_the_pieces_they_are_meant_to(kind):
    f = cases.fill(kind, 3, 7)
    a_mid = any(bool((cases.split3(f[a])[1] != 0).any()) for a, _ in cases.PAIRS)
    b_mid = any(bool((cases.split3(f[b])[1] != 0).any()) for _, b in cases.PAIRS)
    assert (a_mid, b_mid) == {"a_mid": (True, False), "b_mid": (False, True), "mid_mid": (True, True)}[kind]
    assert all(bool((cases.split3(f[k])[2] == 0).all()) for pair in cases.PAIRS for k in pair)     # 12 bits: no lo piece


def test_the_integer_fills_are_exact_in_fp32():
    """what makes 'bit for bit' a fair demand: every partial sum is an integer below 2^24, in any order and any split"""
    for R, S in cases.SHAPES:
        for kind in ("small", "one_last", "one_inner"):
            assert cases.exact_in_fp32(cases.fill(kind, R, S)), (kind, R, S)
    for R, S in cases.SHAPES[:2]:
        for kind in ("a_mid", "b_mid"):
            assert cases.exact_in_fp32(cases.fill(kind, R, S)), (kind, R, S)
    assert cases.exact_in_fp32(cases.fill("mid_mid", 3, 7))
