"""The fused MLP training chain on the GPU at the sizes where its launchers change form (tests/mlp_edge_cases.py: SIZES,
RAY_SUM_SIZES, COMPACT_ROWS; checked on the CPU by tests/test_mlp_edge_cases.py): the saving forward, the inference forwards, the
dX chain, the twelve parameter gradients, the per-ray head-bias sums with their indexed twins, and tn_compact_rows.

Every comparison is with float64 of the inputs or of the run's own STORED operands -- never with another run of the kernel under
test, except where bit-identity of two entries is the statement.  The bounds are the ones the suite already holds each
arithmetic to (mlp_edge_cases.py quotes them) or the a-priori (c + 1) 2^-24 sum |terms| of an fp32 sum of c terms; none is tuned
to a kernel.  Integer fills have one correct bit pattern: every partial sum is an exact fp32 integer in any order.

The C entries are called through ctypes: outputs the caller allocates sit PAD words inside a pattern-filled buffer
(tests/test_gather_edges_gpu.py::Guarded) whose margins must stay untouched; every output is NaN-filled first.  Each test prints
`max err / bound` per tensor before it asserts (pytest -s; profiles/mlp_edges_gpu.txt records one run)."""
import copy
import ctypes as C
import importlib

import pytest
import torch

import mlp_edge_cases as cases
from gather_cases import U
from test_adjoint_x3_gpu import _decode_relu_masks, _quad_major, _raw_chain
from test_dw_x3_gpu import GRADS, _raw_grads, _to_quad_major, _upload
from test_gather_edges_gpu import Guarded
from test_mlp_bf16_gpu import _against_statement

pytestmark = pytest.mark.gpu
render = importlib.import_module("tetra-nerf_amd.render")

F32 = torch.float32
MODE = {"fp32": 0, "bf16x3": 1, "bf16": 2}
SHAPES = [(R, S) for R, S, _ in cases.SIZES]
SHAPE_IDS = cases.IDS
_ids = lambda shapes: [f"{R}x{S}" for R, S in shapes]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _held(label, name, err, bound):
    """prints max err / bound of one tensor; True when the bound holds on every element"""
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{label} {name}: max err / bound = {worst:.3f}  (max err {float(err.max()):.3e})")
    return bool((err <= bound).all())


def _carve(words, device, fill=float("nan")):
    """`words` floats of NaN between two pattern-filled margins"""
    g = Guarded(words, device)
    t = g.inner.view(F32)
    t.fill_(fill)
    return g, t


_P = {}


def _problem(R, S, device, default_init=False):
    key = (R, S, default_init)
    if key not in _P:
        _P[key] = cases.on(cases.problem(R, S, default_init), device)
    return _P[key]


# ---------------------------------------------------------------------------------------------------------------- 1
_FWD = {}


def _saving_forward(tn, device, R, S, mode, biased):
    """tn_mlp_forward_gather_train_ex into guarded, NaN-filled outputs and saves -- run once per case, left unchanged"""
    key = (R, S, mode, biased)
    if key in _FWD:
        return _FWD[key]
    cpp = tn.cpp
    p = _problem(R, S, device)
    n = p["n"]
    (gs, sigma), (gc, rgb), (ga, acts) = _carve(n, device), _carve(3 * n, device), _carve(576 * n, device)
    gm = Guarded(16 * n, device)                    # u64 [4, n, 2]
    gm.inner.fill_(-1)
    rgb, acts, masks = rgb.view(n, 3), acts.view(576, n), gm.inner.view(torch.int64).view(4, n, 2)
    bs = cpp._backward_buffers(acts, masks)
    mh = cpp.fused_mlp(p["w"])
    bias = p["bias"].contiguous() if biased else None
    cpp._lib.check(cpp._lib.load().tn_mlp_forward_gather_train_ex(
        mh.handle, n, S, p["vi"].data_ptr(), p["bc"].data_ptr(), cpp.field_vertex_major(p["field"]).data_ptr(), p["dirs"].data_ptr(),
        MODE[mode], sigma.data_ptr(), rgb.data_ptr(), C.byref(bs), None if bias is None else bias.data_ptr(), cpp._stream(device)))
    torch.cuda.synchronize()
    saved = cpp.MlpSaved()
    saved.acts, saved.masks, saved.sigma, saved.rgb, saved.n, saved.S = acts, masks, sigma, rgb, n, S
    _FWD[key] = dict(p=p, sigma=sigma, rgb=rgb, saved=saved, guards=(gs, gc, ga, gm), bias=bias)
    return _FWD[key]


def _layers(saved, n):
    a = saved.acts
    return [_quad_major(a[0:64], n)] + [_quad_major(a[64 + 128 * l:192 + 128 * l], n) for l in range(4)]


@pytest.mark.parametrize("biased", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("R,S", SHAPES, ids=SHAPE_IDS)
def test_saving_forward(tn, device, R, S, mode, biased):
    r = _saving_forward(tn, device, R, S, mode, biased)
    p, sigma, rgb, saved = r["p"], r["sigma"], r["rgb"], r["saved"]
    n, w = p["n"], p["w"]
    label = f"forward {R}x{S} {mode}{' bias' if biased else ''}"
    assert all(g.margins_intact() for g in r["guards"]), label
    assert bool(torch.isfinite(sigma).all()) and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(saved.acts).all())
    # the outputs are the inference kernel's bits in the same mode
    s_inf, c_inf = tn.cpp.mlp_forward_gather(p["vi"], p["bc"], p["field"], p["dirs"], w, S, mode=mode, ray_head_bias=r["bias"])
    assert _bits(sigma, s_inf) and _bits(rgb, c_inf), label
    assert float(sigma.max()) > 0
    if biased:         # the bias acts, on the colours only
        nb = _saving_forward(tn, device, R, S, mode, False)
        assert _bits(sigma, nb["sigma"]) and not _bits(rgb, nb["rgb"])
    # masks = the signs of the saved activations
    acts = _layers(saved, n)
    masks = _decode_relu_masks(saved.masks, n)
    for l in range(4):
        h = acts[l + 1]
        assert bool((h >= 0).all()), (label, l)
        assert torch.equal(masks[l], h.view(torch.int32) != 0), (label, l)
    # x0: the fp32 gather's bits in either mode, and the gather in float64 (the bar of tests/test_train_x3_gpu.py)
    assert _bits(acts[0], _layers(_saving_forward(tn, device, R, S, "fp32", False)["saved"], n)[0]), label
    err = (acts[0].double() - cases.gather64(p)).abs()
    print(f"{label} x0: max |x0 - gather64| = {float(err.max()):.3e} (bar 1e-5)")
    assert float(err.max()) < 1e-5
    # every saved layer follows from the stored one before it
    a64 = [a.double() for a in acts]
    hin, bias = cases.head_input(p, a64[3])
    steps = [(a64[0], w[0], w[1], None), (a64[1], w[2], w[3], None), (a64[2], w[4], w[5], None), (hin, w[8], w[9], bias if biased else None)]
    ok = []
    for l, (x, W, b, extra) in enumerate(steps):
        h64, bound = cases.layer(x, W, b, extra)
        assert float(h64.max()) > 0
        ok.append(_held(label, f"h{l + 1}", (a64[l + 1] - h64).abs(), bound))
    assert all(ok), (label, ok)
    # the carry of the fp32 kernel hands h4 and its mask word over to the block's next group (or to the flush): at the sizes where
    # a block runs two groups, those of its FIRST group and of the one-sample LAST group are the values, not the zeros a carry holds
    groups = -(-n // cases.FWD_GROUP)
    if groups > cases.GROUP_GRID:
        rows = torch.cat([torch.arange((groups - cases.GROUP_GRID) * cases.FWD_GROUP), torch.arange((groups - 2) * cases.FWD_GROUP, n)]).to(device)
        assert n % cases.FWD_GROUP == 1 and int(rows[-1]) == n - 1
        assert bool((acts[4][rows] != 0).any(1).all()), label
        assert bool((saved.masks[3, rows] != 0).any(1).all()), label
        h64, bound = cases.layer(hin[rows], w[8], w[9], bias[rows] if biased else None)
        assert bool((h64.max(1).values > 1e3 * bound.max(1).values).all())       # (a zero there is far outside the bound)


# ---------------------------------------------------------------------------------------------------------------- 2
def _c_forward(tn, device, p, mode, feats=None, density_only=False):
    """tn_mlp_forward (feats f32 [64, n] given) or tn_mlp_forward_gather through the C entry into guarded, NaN-filled outputs"""
    cpp = tn.cpp
    lib = cpp._lib.load()
    n, S = p["n"], p["S"]
    (gs, sigma), (gc, rgb) = _carve(n, device), _carve(3 * n, device)
    mh = cpp.fused_mlp(p["w"])
    dirs = None if density_only and feats is None else p["dirs"].data_ptr()
    rgb_ptr = None if density_only else rgb.data_ptr()
    if feats is None:
        cpp._lib.check(lib.tn_mlp_forward_gather(mh.handle, n, S, p["vi"].data_ptr(), p["bc"].data_ptr(), cpp.field_vertex_major(p["field"]).data_ptr(),
                                                 dirs, MODE[mode], sigma.data_ptr(), rgb_ptr, None, None, cpp._stream(device)))
    else:
        cpp._lib.check(lib.tn_mlp_forward(mh.handle, n, S, feats.data_ptr(), dirs, MODE[mode], sigma.data_ptr(), rgb_ptr, cpp._stream(device)))
    torch.cuda.synchronize()
    assert gs.margins_intact() and gc.margins_intact()
    assert bool(torch.isfinite(sigma).all())
    if density_only:
        assert bool(torch.isnan(rgb).all())
        return sigma, None
    assert bool(torch.isfinite(rgb).all())
    return sigma, rgb.view(n, 3)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("R,S", cases.FORWARD_EDGES, ids=_ids(cases.FORWARD_EDGES))
def test_inference_forwards(tn, device, R, S, mode):
    """the gather form, the feature-major form and the density-only form of both, on the default-initialised model.  fp32 and
    bf16x3: against the float64 network, 5e-6 on sigma and 2e-6 on rgb (tests/test_render_gpu.py::test_mlp_forward_vs_float64);
    bf16: against its own statement with the bar of tests/test_mlp_bf16_gpu.py::test_network_against_the_statement."""
    p = _problem(R, S, device, default_init=True)
    n = p["n"]
    label = f"inference {R}x{S} {mode}"
    if mode == "bf16":
        feats = tn.cpp.interpolate_values(p["vi"], p["bc"], p["field"]).reshape(n, 64)       # the gather's own bits
        mlp = copy.deepcopy(cases.problem(R, S, default_init=True)["mlp"]).to(device)
        with torch.no_grad():
            want = tuple(t.cpu() for t in render.mlp_forward_bf16_statement(mlp, feats, p["dirs"].repeat_interleave(S, dim=0)))
        feats_fm = feats.t().contiguous()
        for form, fm in (("gather", None), ("feature-major", feats_fm)):
            sigma, rgb = _c_forward(tn, device, p, mode, fm)
            _against_statement(sigma, rgb, want, f"{label} {form}")
            s_only, _ = _c_forward(tn, device, p, mode, fm, density_only=True)
            _against_statement(s_only, None, want, f"{label} {form} density only")
        return
    x64 = cases.gather64(p)
    feats_fm = x64.float().t().contiguous()
    ok = []
    for form, fm, x0 in (("gather", None, x64), ("feature-major", feats_fm, x64.float().double())):
        ref = cases.network(p, x0, biased=False)
        sigma, rgb = _c_forward(tn, device, p, mode, fm)
        s_only, _ = _c_forward(tn, device, p, mode, fm, density_only=True)
        for name, got, want, bar in (("sigma", sigma, ref["sigma"], 5e-6), ("rgb", rgb, ref["rgb"], 2e-6), ("sigma (density only)", s_only, ref["sigma"], 5e-6)):
            err = float((got.double() - want).abs().max())
            print(f"{label} {form} {name}: max err / bar = {err / bar:.3f}  (max err {err:.3e})")
            ok.append(err < bar)
    assert all(ok), (label, ok)


# ---------------------------------------------------------------------------------------------------------------- 3
DX_FORWARDS = [("fp32", True), ("bf16x3", False)]
_DX = {}


def _dx_runs(tn, device, R, S, fwd_mode, biased):
    key = (R, S, fwd_mode, biased)
    if key not in _DX:
        r = _saving_forward(tn, device, R, S, fwd_mode, biased)
        p = r["p"]
        c = dict(n=p["n"], w=p["w"], d_sigma=p["d_sigma"].contiguous(), d_rgb=p["d_rgb"].contiguous())
        fwd = (r["sigma"], r["rgb"], r["saved"])
        _DX[key] = {name: _raw_chain(tn, c, fwd, m) for name, m in (("old", None), ("old again", None), ("ex0", 0), ("x3", 1), ("x3 again", 1))}
    return _DX[key]


@pytest.mark.parametrize("fwd_mode,biased", DX_FORWARDS, ids=["fp32-bias", "bf16x3-plain"])
@pytest.mark.parametrize("R,S", cases.DX_EDGES, ids=_ids(cases.DX_EDGES))
def test_dx_chain(tn, device, R, S, fwd_mode, biased):
    """tn_mlp_backward and tn_mlp_backward_ex mode 1 on the saved buffers of test_saving_forward: d4, d3, d2, d1 and dx0 each follow
    from the stored layer before (the bound of tests/test_adjoint_x3_gpu.py), dhead from the stored outputs -- softplus' = 1 -
    exp(-sigma) and sigmoid' = rgb (1 - rgb) are factors in [0, 1] formed in a few fp32 roundings, so |dhead - dhead64| <= 4e-7 |d
    sigma| resp. |d rgb|, the suite's allowance for such a VALU statement."""
    r = _saving_forward(tn, device, R, S, fwd_mode, biased)
    runs = _dx_runs(tn, device, R, S, fwd_mode, biased)
    p, saved = r["p"], r["saved"]
    n, w = p["n"], [x.double() for x in p["w"]]
    masks = _decode_relu_masks(saved.masks, n)
    s64, c64 = r["sigma"].double(), r["rgb"].double()
    dhead64 = torch.cat([(p["d_sigma"].double() * (1 - torch.exp(-s64)))[None], (p["d_rgb"].double() * c64 * (1 - c64)).t()], 0)
    dhead_bound = 4e-7 * torch.cat([p["d_sigma"].double().abs()[None], p["d_rgb"].double().abs().t()], 0)
    for entry in ("old", "x3"):
        ch = runs[entry]
        label = f"dX {R}x{S} after {fwd_mode}{' bias' if biased else ''}, {'tn_mlp_backward' if entry == 'old' else 'mode 1'}"
        for k, v in ch.items():
            assert bool(torch.isfinite(v).all()), (label, k)           # (every value was written)
        d4, d3, d2, d1 = (_quad_major(ch[k], n).double() for k in ("d4", "d3", "d2", "d1"))
        dsr, drr = ch["dhead"][0].double()[:, None], ch["dhead"][1:4].double().t()
        ok = [_held(label, "dhead", (ch["dhead"].double() - dhead64).abs(), dhead_bound)]
        d4_64 = (drr @ w[10]) * masks[3]
        assert bool((d4[~masks[3]] == 0).all()), label
        ok.append(_held(label, "d4", (d4 - d4_64).abs(), (4e-7 * (drr.abs() @ w[10].abs()).max()).expand_as(d4)))
        for name, d_in, W, mask, extra, got in (("d3", d4, w[8][:, 27:], masks[2], dsr * w[6], d3), ("d2", d3, w[4], masks[1], None, d2),
                                                ("d1", d2, w[2], masks[0], None, d1), ("dx0", d1, w[0], None, None, ch["dx0"].double())):
            d64, bound = cases.dx_layer(d_in, W, mask, extra)
            assert float(d64.abs().max()) > 0, (label, name)
            if mask is not None:
                assert bool((got[~mask] == 0).all()), (label, name)
            ok.append(_held(label, name, (got - d64).abs(), bound))
        assert all(ok), (label, ok)
    # what the VALU computes is mode 0's bits; mode 0 is the old entry; two runs give the same bits
    assert _bits(runs["x3"]["dhead"], runs["old"]["dhead"]) and _bits(runs["x3"]["d4"], runs["old"]["d4"])
    for k in runs["old"]:
        assert _bits(runs["ex0"][k], runs["old"][k]) and _bits(runs["old again"][k], runs["old"][k]) and _bits(runs["x3 again"][k], runs["x3"][k]), k
    if n >= 127:
        assert not _bits(runs["x3"]["d3"], runs["old"]["d3"])          # (the other arithmetic did run)


# ---------------------------------------------------------------------------------------------------------------- 4
GEMMS, VALU_SUMS, RGB_HEAD = ("w1", "w2", "w3", "wh"), ("b1", "b2", "b3", "bh", "wd"), ("wr", "bd", "br")


def _check_sums(label, ref, n, fp32, x3):
    """fp32: |g - g64| <= (n + 1) u sum |terms| on all twelve; bf16x3 GEMMs: 2^-21 |A|^T |B| + 4 y; its bias sums and wd: 4 y + 2^-24 sum
    |terms|, y = the fp32 run's largest error on the tensor; the rgb head's kernels are not touched by the mode"""
    ok = []
    for k in GRADS:
        d64, mag = (t.reshape(fp32[k].shape) for t in ref[k])
        assert float(d64.abs().max()) > 0, (label, k)
        err32 = (fp32[k].double() - d64).abs()
        ok.append(_held(label, k + " (fp32)", err32, cases.sum_bound(mag, n)))
        y = float(err32.max())
        if k in GEMMS:
            ok.append(_held(label, k + " (bf16x3)", (x3[k].double() - d64).abs(), 2.0 ** -21 * mag + 4.0 * y))
        elif k in VALU_SUMS:
            ok.append(_held(label, k + " (bf16x3)", (x3[k].double() - d64).abs(), 4.0 * y + 2.0 ** -24 * mag))
        else:
            assert _bits(x3[k], fp32[k]), (label, k)
    assert all(ok), (label, ok)


INTEGER = [(R, S, kind, unit) for R, S in SHAPES
           for kind, unit in (("small", None), ("one_last", None), ("one_first_of_second_trip", cases.DW_UNIT), ("one_first_of_second_trip", cases.RGB_UNIT))
           if unit is None or cases.slicing(R * S, unit)[0] > 1]          # (a size without a second slice has no first row of one)
INTEGER_IDS = [f"{R}x{S}-{kind}" + ("" if unit is None else f"-slices_of_{unit}") for R, S, kind, unit in INTEGER]


@pytest.mark.parametrize("R,S,kind,unit", INTEGER, ids=INTEGER_IDS)
def test_param_grads_integer_fills_bit_for_bit(tn, device, R, S, kind, unit):
    """all twelve tensors of tn_mlp_param_grads and of mode 1 are the float64 result, bit for bit (Wh[:, 27:]: the encoding columns
    hold sines; they are held to the fp32 bound)."""
    n = R * S
    f = cases.fill(kind, R, S) if unit is None else cases.fill(kind, R, S, unit)
    assert cases.exactness_condition(n)
    b = _upload(f, device)
    ref = cases.param_sums(b, f["dirs"], S)
    runs = {"tn_mlp_param_grads": _raw_grads(tn, device, b, f["dirs"], S, None), "mode 1": _raw_grads(tn, device, b, f["dirs"], S, 1)}
    for entry, got in runs.items():
        label = f"dW {R}x{S} {kind}{'' if unit is None else f' (slices of {unit})'} {entry}"
        bad = []
        for k in GRADS:
            d64 = ref[k][0].reshape(got[k].shape)
            g = got[k]
            if k == "wh":
                enc_err = (g[:, :27].double() - d64[:, :27]).abs()
                assert _held(label, "wh[:, :27]", enc_err, (cases.sum_bound(ref[k][1], n) if entry != "mode 1" else 2.0 ** -21 * ref[k][1] + 4 * cases.sum_bound(ref[k][1], n))[:, :27]), label
                d64, g = d64[:, 27:], g[:, 27:]
            want = d64.float()
            assert want.double().equal(d64) and float(want.abs().max()) > 0, (label, k)      # (the reference is an fp32 number)
            wrong = int((g != want).sum())
            print(f"{label} {k}: {wrong} of {g.numel()} entries differ from the exact result")
            if wrong or not _bits(g, want):
                bad.append(k)
        assert not bad, (label, bad)


@pytest.mark.parametrize("R,S", SHAPES, ids=SHAPE_IDS)
def test_param_grads_random_fill(tn, device, R, S):
    f = cases.fill("random", R, S)
    b = _upload(f, device)
    ref = cases.param_sums(b, f["dirs"], S)
    _check_sums(f"dW {R}x{S} random", ref, R * S, _raw_grads(tn, device, b, f["dirs"], S, None), _raw_grads(tn, device, b, f["dirs"], S, 1))


@pytest.mark.parametrize("R,S", cases.DX_EDGES, ids=_ids(cases.DX_EDGES))
def test_param_grads_real_buffers(tn, device, R, S):
    """on what the fp32 saving forward (with a per-ray bias) and tn_mlp_backward left: float64 of the STORED operands"""
    r = _saving_forward(tn, device, R, S, "fp32", True)
    ch = _dx_runs(tn, device, R, S, "fp32", True)["old"]
    a, p = r["saved"].acts, r["p"]
    b = dict(x0=a[0:64], h1=a[64:192], h2=a[192:320], h3=a[320:448], h4=a[448:576], d1=ch["d1"], d2=ch["d2"], d3=ch["d3"], d4=ch["d4"],
             dhead=ch["dhead"])
    ref = cases.param_sums(b, p["dirs"], S)
    _check_sums(f"dW {R}x{S} real", ref, R * S, _raw_grads(tn, device, b, p["dirs"], S, None), _raw_grads(tn, device, b, p["dirs"], S, 1))


ONE_RAY = [(65537, 1, 159), (65537, 1, 160), (65537, 1, 65536), (1, 65537, 0), (43, 3, 11)]


@pytest.mark.parametrize("R,S,ray", ONE_RAY, ids=[f"{R}x{S}-ray{r}" for R, S, r in ONE_RAY])
def test_head_encoding_columns_are_the_listed_rays(tn, device, R, S, ray):
    """only one ray's samples are nonzero (small integers): dWh[:, :27] = (sum of that ray's d4) x enc(that ray), S terms per entry; the
    ray bookkeeping of the head-layer GEMM gone wrong shows as another ray's encoding -- O(1), against (S + 1) u sum |terms|.  Rays 159
    | 160 sit on either side of the first slice edge at S = 1, ray 65536 is the last slice's only sample; at 1 x 65537 the one ray spans
    every slice."""
    f = cases.one_ray(R, S, ray)
    b = _upload(f, device)
    ref = cases.param_sums(b, f["dirs"], S)
    d64, mag = ref["wh"]
    enc = render.direction_encoding(f["dirs"].to(device).float()).double()
    assert torch.allclose(d64[:, :27], f["d4"][ray * S:(ray + 1) * S].double().sum(0).to(device)[:, None] * enc[ray][None], rtol=1e-12, atol=1e-12)
    assert float(d64[:, :27].abs().max()) > 0
    for entry, mode in (("tn_mlp_param_grads", None), ("mode 1", 1)):
        got = _raw_grads(tn, device, b, f["dirs"], S, mode)["wh"]
        label = f"dWh {R}x{S} ray {ray} {entry}"
        bound = cases.sum_bound(mag, S) if mode is None else 2.0 ** -21 * mag + 4 * cases.sum_bound(mag, S)
        assert _held(label, "wh[:, :27]", (got.double() - d64).abs()[:, :27], bound[:, :27]), label
        assert _bits(got[:, 27:], d64[:, 27:].float()), label


# ---------------------------------------------------------------------------------------------------------------- 5
def _ray_sums(tn, device, d4_rows, n_samples, S, live=None):
    """tn_mlp_ray_head_grad (or its indexed twin over `live`) on d4 rows [m, 128] into a guarded, NaN-filled [rays, 128]"""
    cpp = tn.cpp
    lib = cpp._lib.load()
    m, rays = d4_rows.shape[0], n_samples // S
    d4 = _to_quad_major(d4_rows.to(device))
    bs = cpp._MlpBackwardBuffers(*([None] * 9), d4.data_ptr(), None, None)
    g, out = _carve(rays * 128, device)
    if live is None:
        assert m == n_samples
        cpp._lib.check(lib.tn_mlp_ray_head_grad(m, S, C.byref(bs), out.data_ptr(), cpp._stream(device)))
    else:
        assert live.dtype == torch.int32 and live.numel() >= m
        cpp._lib.check(lib.tn_mlp_ray_head_grad_indexed(m, n_samples, S, live.data_ptr(), C.byref(bs), out.data_ptr(), cpp._stream(device)))
    torch.cuda.synchronize()
    assert g.margins_intact()
    assert bool(torch.isfinite(out).all())
    return out.view(rays, 128)


@pytest.mark.parametrize("rays,S", cases.RAY_SUM_SIZES, ids=_ids(cases.RAY_SUM_SIZES))
def test_ray_head_sums(tn, device, rays, S):
    n = rays * S
    ok = []
    for kind in ("small", "random"):
        d4 = cases.ray_d4(kind, rays, S).to(device)
        label = f"ray sums {rays}x{S} {kind}"
        val, mag, cnt = cases.ray_sums(d4, S)
        assert float(val.abs().max()) > 0 and bool((cnt == S).all())
        dense = _ray_sums(tn, device, d4, n, S)
        identity = torch.arange(n, dtype=torch.int32, device=device)
        same = _ray_sums(tn, device, d4, n, S, live=identity)
        assert _bits(same, dense), label                      # the identity list: the dense entry's bits
        if kind == "small":
            assert _bits(dense, val.float()) and val.float().double().equal(val), label
        ok.append(_held(label, "dense", (dense.double() - val).abs(), (S + 1) * U * mag))
        # a list that drops every sample of the rays r % 7 == 3 and keeps one sample of the last remaining ray
        listed, last = cases.dropping_list(rays, S)
        k = listed.numel()
        live = torch.full((n,), cases.NOT_A_SAMPLE, dtype=torch.int32)
        live[:k] = listed
        live = live.to(device)
        got = _ray_sums(tn, device, d4[listed.long().to(device)], n, S, live=live)
        val, mag, cnt = cases.ray_sums(d4[listed.long().to(device)], S, listed=listed, rays=rays)
        assert int(cnt[last]) == 1 and (rays < 4 or bool((cnt == 0).any()))
        assert not bool(got[cnt == 0].any()), label             # a ray without a listed sample: exact zeros
        assert torch.equal(got[last], d4[last * S]), label      # one term: the sample itself (0 + -0 = +0: equal as values)
        if kind == "small":
            assert _bits(got, val.float()), label
        ok.append(_held(label, "dropping list", (got.double() - val).abs(), (cnt[:, None] + 1) * U * mag))
    assert all(ok), ok


def test_ray_head_sums_through_mlp_backward(tn, device):
    """the shipped ray count with S = 8: mlp_backward(want_ray_head_grad=True) against float64 of the chain it returns"""
    R, S = 4096, 8
    r = _saving_forward(tn, device, R, S, "fp32", True)
    p = r["p"]
    res = tn.cpp.mlp_backward(r["saved"], p["vi"], p["bc"], p["field"], p["dirs"], p["w"], r["sigma"], r["rgb"], p["d_sigma"], p["d_rgb"],
                              want_ray_head_grad=True, return_chain=True)
    d_ray, chain = res[2], res[3]
    assert d_ray.shape == (R, 128)
    val, mag, cnt = cases.ray_sums(_quad_major(chain.d4, p["n"]), S)
    assert float(val.abs().max()) > 0 and float(val.abs().amax(1).min()) > 0        # every ray has a gradient
    assert _held(f"ray sums {R}x{S} mlp_backward", "d_ray", (d_ray.double() - val).abs(), (S + 1) * U * mag)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("words", [1, 3, 4])
@pytest.mark.parametrize("n_live", cases.COMPACT_ROWS)
def test_compact_rows(tn, device, n_live, words):
    """a strided ascending list over a source of 2 n_live rows: every row equal, the destination's margins untouched"""
    cpp = tn.cpp
    src = torch.randint(0, 2 ** 31 - 1, (2 * n_live, words), dtype=torch.int32, generator=torch.Generator().manual_seed(n_live + words)).to(device)
    live = (2 * torch.arange(n_live, dtype=torch.int32) + 1).to(device)
    g = Guarded(n_live * words, device)
    before = g.inner.clone()
    cpp._lib.check(cpp._lib.load().tn_compact_rows(words, n_live, live.data_ptr(), src.data_ptr(), g.inner.data_ptr(), cpp._stream(device)))
    torch.cuda.synchronize()
    want = src[live.long()]
    got = g.inner.view(n_live, words)
    wrong = int((got != want).any(1).sum())
    print(f"compact rows {n_live} x {words} words: {wrong} rows differ; {int((got == before.view(n_live, words)).all(1).sum())} rows still hold the pattern")
    assert g.margins_intact()
    assert wrong == 0 and torch.equal(got, want)
