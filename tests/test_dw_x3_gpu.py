"""The bf16x3 weight-gradient GEMMs (tn_mlp_param_grads_ex mode 1, csrc/tn_mlp_x3_dw.hip) on the GPU, and their way up to
render_train(dw_mode="bf16x3") and the nerfstudio adapter (config.train_dw_mode).

The C entry is called directly through ctypes (as tests/test_adjoint_x3_gpu.py::_raw_chain calls the dX chain): the operand
buffers are the caller's, so the tests fill them.

Shapes (tests/dw_x3_cases.py::SHAPES), the smallest at which the kernel changes path given slices of 32 samples and at most 512
blocks: 3 x 7 = 21 (less than one step; a ray change inside a step for the encoding tile), 37 x 97 = 3,589 (fewer blocks than
the grid, partial last step), 257 x 64 = 16,448 (just above 512 x 32: every block has work, slices of 64), 300 x 257 = 77,100
(five steps per block, partial last block, a ray boundary every 257 samples).

1. mode 0 IS tn_mlp_param_grads, bit for bit; other modes are refused.
2. integer operands whose every partial sum is exact in fp32 (tests/test_dw_x3.py shows that): mode 1 = the exact result = mode 0
   bit for bit -- layout, indexing, the sample-to-K mapping, lanes beyond n.
3. the buffers of a real training forward + dX chain (and the helper's random fill): against the float64 product of the STORED
   operands, |dW - D64| <= 2^-21 |A|^T |B| + 4 y elementwise, y = the fp32 kernel's own largest error on the same tensor (measured
   here from mode 0).  First term: the bound this arithmetic is held to everywhere else; second: fp32 accumulation over the
   sample axis, which both kernels do with the same number of terms in a different order -- the factor 4 is the one the per-ray
   stage tests of this suite give the fp32 statement's measured error.  Bias gradients and d wd: 4 y + 2^-24 sum |terms|.
4. two mode-1 runs give the same bits.
5. render_train / TetraRenderer / the adapter."""
import ctypes as C
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

import dw_x3_cases as cases
from test_adjoint_x3_gpu import NAMES, _case, _quad_major, _same_bits, _tensor_rel, _train_setup, scene  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))

GRADS = NAMES[1:]                      # the twelve parameter tensors in the order of the C struct
ACTS = ("x0", "h1", "h2", "h3", "h4")
DS = ("d1", "d2", "d3", "d4")


def _to_quad_major(t):
    """[n, F] in feature order -> an [F, n] tensor whose memory is quad-major [F / 4][n][4] (include/tetranerf_hip.h)"""
    n, F = t.shape
    return t.reshape(n, F // 4, 4).permute(1, 0, 2).contiguous().reshape(F, n)


def _upload(f, device):
    """a fill of tests/dw_x3_cases.py as the buffers the entry takes"""
    b = {k: _to_quad_major(f[k].to(device)) for k in ACTS + DS}
    b["dhead"] = f["dhead"].to(device).contiguous()
    return b


_MLP = {}


def _handle(tn, device):
    """the entry needs a handle with weights set (it owns the scratch); the gradients do not depend on the weights"""
    import torch

    if "h" not in _MLP:
        render = importlib.import_module("tetra-nerf_amd.render")
        torch.manual_seed(5)
        _MLP["w"] = [x.detach() for x in render.mlp_weights(render.TetraMLP().to(device))]
    return tn.cpp.fused_mlp(_MLP["w"])


def _raw_grads(tn, device, b, dirs, S, mode):
    """mode None = tn_mlp_param_grads, otherwise tn_mlp_param_grads_ex(mode), into zero-filled gradients (the entry accumulates)"""
    import torch

    cpp = tn.cpp
    lib = cpp._lib.load()
    n = b["dhead"].shape[1]
    grads = [torch.zeros(shp, dtype=torch.float32, device=device) for shp in cpp._WEIGHT_SHAPES]
    gs = cpp._MlpWeightsStruct(*[g.data_ptr() for g in grads])
    bs = cpp._MlpBackwardBuffers(*[b[k].data_ptr() for k in ACTS], None, *[b[k].data_ptr() for k in DS], b["dhead"].data_ptr(), None)
    dirs = dirs.to(device).contiguous()
    head = (_handle(tn, device).handle, n, S, dirs.data_ptr(), C.byref(bs), C.byref(gs))
    stream = cpp._stream(device)
    if mode is None:
        cpp._lib.check(lib.tn_mlp_param_grads(*head, stream))
    else:
        cpp._lib.check(lib.tn_mlp_param_grads_ex(*head, mode, stream))
    torch.cuda.synchronize()
    return dict(zip(GRADS, grads))


def _case_buffers(c):
    """what the fp32 dX chain of a tests/test_adjoint_x3_gpu.py case left, as the entry's buffers"""
    a, ch = c["fwd"][2].acts, c["old"]
    return dict(x0=a[0:64], h1=a[64:192], h2=a[192:320], h3=a[320:448], h4=a[448:576], d1=ch["d1"], d2=ch["d2"], d3=ch["d3"],
                d4=ch["d4"], dhead=ch["dhead"])


def _plain(b):
    """the buffers back in [n, F] feature order, float64"""
    n = b["dhead"].shape[1]
    out = {k: _quad_major(b[k], n).double() for k in ACTS + DS}
    out["dhead"] = b["dhead"].double()
    return out


def _references(tn, b, dirs, S):
    """float64 statements of the nine tensors the GEMM kernels produce, from the stored operands: {name: (value, sum of the
    magnitudes of its terms)}"""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    p = _plain(b)
    n = p["dhead"].shape[1]
    # (the library encodes the directions in fp32; its table is internal, so this is PyTorch's fp32 statement of the same)
    enc = render.direction_encoding(dirs.to(b["dhead"].device).float()).double().repeat_interleave(S, dim=0)
    assert enc.shape == (n, 27)
    hb = torch.cat([enc, p["h3"]], 1)
    ref = {}
    for name, bias, a, x in (("wh", "bh", p["d4"], hb), ("w3", "b3", p["d3"], p["h2"]), ("w2", "b2", p["d2"], p["h1"]),
                             ("w1", "b1", p["d1"], p["x0"])):
        ref[name] = (a.t() @ x, a.abs().t() @ x.abs())
        ref[bias] = (a.sum(0), a.abs().sum(0))
    dsr = p["dhead"][0][:, None]
    ref["wd"] = ((dsr * p["h3"]).sum(0)[None], (dsr.abs() * p["h3"].abs()).sum(0)[None])
    return ref


# ---------------------------------------------------------------------------------------------------------------- 1
REAL = [(3, 7, 200, False, "fp32"), (37, 97, 5000, False, "fp32"), (37, 97, 5000, False, "bf16x3"), (257, 64, 5000, False, "fp32"),
        (300, 257, 5000, True, "fp32")]
REAL_IDS = [f"{R}x{S}{'-bias' if b else ''}-{f}" for R, S, V, b, f in REAL]
_RUNS = {}


def _real(tn, device, key):
    """the raw runs of one real case that the tests below share: computed once, left unchanged"""
    if key not in _RUNS:
        c = _case(tn, device, *key)
        b = _case_buffers(c)
        S = c["S"]
        _RUNS[key] = dict(c=c, b=b, old=_raw_grads(tn, device, b, c["dirs"], S, None), ex0=_raw_grads(tn, device, b, c["dirs"], S, 0),
                          x3=_raw_grads(tn, device, b, c["dirs"], S, 1), again=_raw_grads(tn, device, b, c["dirs"], S, 1))
    return _RUNS[key]


def _public(tn, c, **kw):
    sigma, rgb, saved = c["fwd"]
    res = tn.cpp.mlp_backward(saved, c["vi"], c["bc"], c["field"], c["dirs"], c["w"], sigma, rgb, c["d_sigma"], c["d_rgb"], **kw)
    return dict(zip(GRADS, res[1]))


@pytest.mark.parametrize("key", REAL, ids=REAL_IDS)
def test_mode_0_is_the_old_entry(tn, device, key):
    import torch

    r = _real(tn, device, key)
    default, named, x3 = _public(tn, r["c"]), _public(tn, r["c"], dw_mode="fp32"), _public(tn, r["c"], dw_mode="bf16x3")
    for k in GRADS:
        assert bool(torch.isfinite(r["old"][k]).all()) and float(r["old"][k].abs().max()) > 0, k
        assert _same_bits(r["ex0"][k], r["old"][k]), k
        assert _same_bits(default[k], r["old"][k]), k        # mlp_backward's default goes there
        assert _same_bits(named[k], r["old"][k]), k
        assert _same_bits(x3[k], r["x3"][k]), k              # and dw_mode="bf16x3" is mode 1


def test_other_modes_are_refused(tn, device):
    r = _real(tn, device, REAL[0])
    for mode in (2, 3, -1):
        with pytest.raises(RuntimeError, match="mlp mode must be"):
            _raw_grads(tn, device, r["b"], r["c"]["dirs"], r["c"]["S"], mode)
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        _public(tn, r["c"], dw_mode="bf16")


# ---------------------------------------------------------------------------------------------------------------- 2
EXACT = ([("small", R, S) for R, S in cases.SHAPES] + [(k, R, S) for k in ("a_mid", "b_mid") for R, S in cases.SHAPES[:2]]
         + [("mid_mid", 3, 7)] + [(k, R, S) for k in ("one_last", "one_inner") for R, S in cases.SHAPES])


@pytest.mark.parametrize("kind,R,S", EXACT, ids=[f"{k}-{R}x{S}" for k, R, S in EXACT])
def test_exact_integer_operands_bit_for_bit(tn, device, kind, R, S):
    """W1, W2, W3, Wh[:, 27:], b1, b2, b3, bh (and wd): mode 1 = the exact integer result = mode 0, bit for bit.  The encoding
    columns of Wh hold non-integers (sines) and are test 3's; wr, bd, br come from kernels the mode does not touch."""
    import torch

    f = cases.fill(kind, R, S)
    assert cases.exact_in_fp32(f)
    b = _upload(f, device)
    got, old = _raw_grads(tn, device, b, f["dirs"], S, 1), _raw_grads(tn, device, b, f["dirs"], S, 0)
    ref = _references(tn, b, f["dirs"], S)
    for k in ("w1", "w2", "w3", "wh", "b1", "b2", "b3", "bh", "wd"):
        want = ref[k][0].float()
        g, o = got[k], old[k]
        if k == "wh":
            want, g, o = want[:, 27:], g[:, 27:], o[:, 27:]
        assert float(want.abs().max()) > 0, k
        assert want.double().equal(ref[k][0] if k != "wh" else ref[k][0][:, 27:]), k        # (the reference is an fp32 number)
        bad = (g != want).nonzero()
        assert bad.numel() == 0, (k, bad[:4].tolist(), g[tuple(bad[0])].item(), want[tuple(bad[0])].item())
        assert _same_bits(g, want) and _same_bits(g, o), k
    assert bool(torch.isfinite(got["wh"]).all())
    for k in ("wr", "bd", "br"):
        assert _same_bits(got[k], old[k]), k


# ---------------------------------------------------------------------------------------------------------------- 3
def _check_against_float64(tn, device, label, b, dirs, S, x3, fp32):
    ref = _references(tn, b, dirs, S)
    for k in ("w1", "w2", "w3", "wh"):
        d64, mag = ref[k]
        y = float((fp32[k].double() - d64).abs().max())
        err = (x3[k].double() - d64).abs()
        bound = 2.0 ** -21 * mag + 4.0 * y
        print(f"{label} {k}: max err / bound = {float((err / bound).max()):.3f}  (max |dW - D64| = {float(err.max()):.3e}, fp32 kernel "
              f"y = {y:.3e}, max |D64| = {float(d64.abs().max()):.3e})")
        assert float(d64.abs().max()) > 0 and y > 0
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
    for k in ("b1", "b2", "b3", "bh", "wd"):
        d64, mag = ref[k]
        y = float((fp32[k].double() - d64).abs().max())
        err = (x3[k].double() - d64).abs()
        bound = 4.0 * y + 2.0 ** -24 * mag
        print(f"{label} {k}: max err / bound = {float((err / bound).max()):.3f}  (max err = {float(err.max()):.3e}, fp32 kernel y = {y:.3e})")
        assert bool((err <= bound).all()), (k, float((err / bound).max()))


@pytest.mark.parametrize("key", REAL, ids=REAL_IDS)
def test_real_buffers_against_float64_of_the_stored_operands(tn, device, key):
    r = _real(tn, device, key)
    c = r["c"]
    _check_against_float64(tn, device, REAL_IDS[REAL.index(key)], r["b"], c["dirs"], c["S"], r["x3"], r["old"])
    assert not _same_bits(r["x3"]["w2"], r["old"]["w2"])           # the other arithmetic did run
    for k in ("wr", "bd", "br"):
        assert _same_bits(r["x3"][k], r["old"][k]), k


@pytest.mark.parametrize("R,S", [cases.SHAPES[0], cases.SHAPES[1], cases.SHAPES[3]], ids=lambda v: str(v))
def test_random_fill_against_float64(tn, device, R, S):
    """the helper's random fill: the tensors on which tests/test_dw_x3.py emulates the arithmetic"""
    f = cases.fill("random", R, S)
    b = _upload(f, device)
    x3, fp32 = _raw_grads(tn, device, b, f["dirs"], S, 1), _raw_grads(tn, device, b, f["dirs"], S, 0)
    _check_against_float64(tn, device, f"random-{R}x{S}", b, f["dirs"], S, x3, fp32)
    assert not _same_bits(x3["w2"], fp32["w2"])


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("key", REAL, ids=REAL_IDS)
def test_deterministic(tn, device, key):
    r = _real(tn, device, key)
    for k in GRADS:
        assert _same_bits(r["again"][k], r["x3"][k]), k


# ---------------------------------------------------------------------------------------------------------------- 5
def test_render_train_end_to_end_and_off_is_off(tn, device, scene):
    """render_train(dw_mode="bf16x3") against the default call on the same draws (deterministic field gradient): the outputs and
    the field gradient are the default's BITS (dW touches neither); the weight gradients are finite, nonzero and within 1e-5 of
    the default's relative to each tensor's max.  The renderer's train_dw_mode takes the same path, "fp32" per call overrides
    it, a default call afterwards gives the default's bits again.  All three switches together: within 2e-5 of the default,
    outputs equal to the all-but-dW run."""
    import torch

    render = importlib.import_module("tetra-nerf_amd.render")
    before = tn.cpp.DETERMINISTIC_FIELD_GRADIENT
    tn.cpp.DETERMINISTIC_FIELD_GRADIENT = True
    try:
        rd, run = _train_setup(render, device, scene)
        assert rd.train_dw_mode == "fp32"
        want, want_g = run()
        got, got_g = run(dw_mode="bf16x3")
        rd.train_dw_mode = "bf16x3"
        again, again_g = run()
        back, back_g = run(dw_mode="fp32")
        rd.train_dw_mode = "fp32"
        after, after_g = run()
        rd2, run2 = _train_setup(render, device, scene, train_dw_mode="bf16x3")
        assert (rd2.train_dw_mode, rd2.train_adjoint_mode, rd2.train_mlp_mode) == ("bf16x3", "fp32", "fp32")
        built, built_g = run2()
        # independent of the other two switches: all eight combinations run; all three on, and all but dW
        combos = {}
        for fwd in ("fp32", "bf16x3"):
            for adj in ("fp32", "bf16x3"):
                for dw in ("fp32", "bf16x3"):
                    combos[(fwd, adj, dw)] = run(mlp_mode=fwd, adjoint_mode=adj, dw_mode=dw)
        with pytest.raises(RuntimeError, match="mlp mode must be"):
            run(dw_mode="bf16")
    finally:
        tn.cpp.DETERMINISTIC_FIELD_GRADIENT = before
    assert int(want["ray_mask"].sum()) > 300 and float(want["accumulation"].max()) > 0.5
    for k in ("rgb", "accumulation", "depth", "ray_mask"):
        for other in (got, again, back, after, built):
            assert torch.equal(other[k], want[k]), k
    for other in (got_g, again_g, back_g, after_g, built_g):
        assert _same_bits(other[0], want_g[0])                              # the field gradient: dW does not touch it
    differ = 0
    for name, g, wg, ag, bg_, fg, ug in list(zip(NAMES, got_g, want_g, again_g, back_g, after_g, built_g))[1:]:
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        rel = _tensor_rel(g, wg)
        print(f"{name}: max |bf16x3 dW - fp32 dW| / max |fp32| = {rel:.2e}")
        assert rel <= 1e-5, (name, rel)
        differ += int(not _same_bits(g, wg))
        assert _same_bits(ag, g) and _same_bits(ug, g), name            # the renderer's switch = the per-call override
        assert _same_bits(bg_, wg) and _same_bits(fg, wg), name        # off is off
    assert not _same_bits(got_g[NAMES.index("w2")], want_g[NAMES.index("w2")]) and differ >= 4, differ
    for k in ("wr", "bd", "br"):                                            # kernels the mode does not touch
        assert _same_bits(got_g[NAMES.index(k)], want_g[NAMES.index(k)]), k
    for key, (out, grads) in combos.items():
        base_out, base_g = combos[key[:2] + ("fp32",)]
        for k in ("rgb", "accumulation", "depth", "ray_mask"):
            assert torch.equal(out[k], base_out[k]), (key, k)               # dW never moves an output
        assert _same_bits(grads[0], base_g[0]), key
        for name, g in zip(NAMES, grads):
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, (key, name)
    for k in ("rgb", "accumulation", "depth", "ray_mask"):
        assert torch.equal(combos[("fp32", "fp32", "fp32")][0][k], want[k]), k
    all3, all3_g = combos[("bf16x3", "bf16x3", "bf16x3")]
    for name, g, wg in zip(NAMES, all3_g, want_g):
        rel = _tensor_rel(g, wg)
        print(f"all three bf16x3, {name}: max |g - default| / max |default| = {rel:.2e}")
        assert rel <= 2e-5, (name, rel)
    assert not _same_bits(all3_g[NAMES.index("w2")], combos[("bf16x3", "bf16x3", "fp32")][1][NAMES.index("w2")])


def test_adapter_trains_with_the_bf16x3_dw_when_the_config_says_so(tn, device, scenes):
    """nerfstudio adapter: a reference TetrahedraNerf (tests/golden/reference_model.py) whose config carries train_dw_mode =
    "bf16x3", in training mode, against the same model without the field under the same seed: the same outputs, gradients within
    1e-5 of the default's relative to each tensor's max, and W2's not bit-equal to the default's (a wrongly routed mode, or
    none, does not pass)."""
    import torch
    import reference_model as rm

    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    plugin.install(ref.TetrahedraNerf)
    before = tn.cpp.DETERMINISTIC_FIELD_GRADIENT
    tn.cpp.DETERMINISTIC_FIELD_GRADIENT = True
    try:
        pts, cells = scenes.random_mesh(6000, 31)
        model = rm.build_model(ref, pts, cells, num_samples=48, num_fine_samples=48).to(device).train()
        assert not hasattr(model.config, "train_dw_mode")
        o, d = scenes.outside_in_rays(1024, 33)
        rb = rm.ray_bundle(ref, o, d, device, camera_indices=np.arange(len(o)) % 3)
        target = torch.rand(len(o), 3, device=device)
        params = [model.tetrahedra_field] + plugin.weights_from_model(model)

        def step():
            for p in params:
                p.grad = None
            torch.manual_seed(7)
            out = model(rb)
            (((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()).backward()
            return {k: out[k].detach().clone() for k in ("rgb", "accumulation")}, [p.grad.clone() for p in params]

        want, want_g = step()
        model.config.train_dw_mode = "bf16x3"
        got, grads = step()
        for k in ("rgb", "accumulation"):
            assert torch.equal(got[k], want[k]), k
        assert float(want["accumulation"].max()) > 0.5
        for name, g, wg in zip(NAMES, grads, want_g):
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
            rel = _tensor_rel(g, wg)
            print(f"adapter {name}: max |bf16x3 dW - fp32 dW| / max |fp32| = {rel:.2e}")
            assert rel <= 1e-5, (name, rel)
        assert not _same_bits(grads[NAMES.index("w2")], want_g[NAMES.index("w2")])
    finally:
        tn.cpp.DETERMINISTIC_FIELD_GRADIENT = before
        plugin.uninstall(ref.TetrahedraNerf)
