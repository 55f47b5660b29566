"""Occupancy-culled training on the GPU (csrc/tn_occupancy_train.hip, csrc/tn_occupancy_dw.hip): the indexed saving forward, the
adjoints on compact columns and render_train(occupancy=, occupancy_threshold=).

What is bit for bit (torch.equal on int32 views): everything a SAMPLE owns -- its outputs, its saved column, its column of the dX
chain, its row of the barycentric gradient -- because a sample is one lane column of both arithmetics; and, with the identity
list, every sum as well (the same terms in the same order).  What is a sum over a SHORTER list of terms (the field gradient, the
twelve weight gradients, the per-ray head-bias sums) is checked against float64 of the run's own compact buffers with the bounds
the suite already has:
  weight-gradient GEMMs, dw_mode "bf16x3"   2^-21 |A|^T |B| + 4 y, y = the fp32 kernel's largest error on the same tensor
                                            (tests/test_dw_x3_gpu.py); bias sums and d wd: 4 y + 2^-24 sum |terms|
  every fp32 sum of c terms in any order    (c + 1) u sum |terms|, u = 2^-24 (tests/gather_cases.py: adjoint_bound) -- the fp32
                                            GEMMs, bias sums, the rgb head, the per-ray sums and the gather adjoint (+ c 2^-126)

Sizes (from the kernels): 32 slots per wave, 256 per group, 256 blocks -- above 65,536 slots a block runs two groups, which is the
fp32 kernel's carry path; the dW slices are 32 slots up to 16,384 slots, so k = 33 has two; at S = 5 a wave's tile spans seven rays.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import gather_cases as gc
from test_adjoint_x3_gpu import _quad_major
from test_dw_x3_gpu import ACTS, DS, GRADS, _handle, _to_quad_major

pytestmark = pytest.mark.gpu

render = importlib.import_module("tetra-nerf_amd.render")
U = gc.U
MODES = ["fp32", "bf16x3"]
SHAPES = {(64, 5): (200, (0, 1, 31, 32, 33, 255, 256, 257, 320)), (300, 257): (5000, (257, 70000))}
NOT_A_SAMPLE = 0x7F7F7F7F


def _i32(x):
    return x.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_i32(a), _i32(b))


_PROBLEMS, _FULL = {}, {}


def _problem(R, S, dev):
    """inputs of one sample set with a per-ray bias, and seeded upstream gradients at a realistic loss scale -- built once"""
    if (R, S) not in _PROBLEMS:
        V = SHAPES[(R, S)][0]
        n = R * S
        torch.manual_seed(R + S)
        mlp = render.TetraMLP().to(dev)
        for p in mlp.parameters():      # larger weights than the default init: every ReLU / softplus / sigmoid branch is live
            p.data.mul_(1.5)
        g = torch.Generator().manual_seed(7 * R + S)
        vi = torch.randint(0, V, (n, 4), generator=g, dtype=torch.int32)
        vi[::17, 2] = -1                # EMPTY vertices are skipped by the gather
        _PROBLEMS[(R, S)] = dict(
            R=R, S=S, n=n, V=V, w=[x.detach() for x in render.mlp_weights(mlp)], field=(torch.randn(64, V, generator=g) * 0.7).to(dev),
            vi=vi.to(dev), bc=(torch.rand(n, 3, generator=g) / 3).to(dev).contiguous(),
            dirs=torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev),
            bias=(torch.randn(R, 128, generator=g) * 0.7).to(dev), d_sigma=(torch.randn(n, generator=g) * 1e-3).to(dev),
            d_rgb=(torch.randn(n, 3, generator=g) * 1e-3).to(dev))
    return _PROBLEMS[(R, S)]


def _backward(tn, p, saved, sigma, rgb, amode, wmode):
    res = tn.cpp.mlp_backward(saved, p["vi"], p["bc"], p["field"], p["dirs"], p["w"], sigma, rgb, p["d_sigma"], p["d_rgb"],
                              want_ray_head_grad=True, want_bary_grad=True, return_dx0=True, return_chain=True, adjoint_mode=amode,
                              dw_mode=wmode)
    grad_field, grads, d_ray, grad_bary, dx0, chain = res
    return dict(field=grad_field, grads=dict(zip(GRADS, grads)), d_ray=d_ray, bary=grad_bary, dx0=dx0, chain=chain)


def _full(tn, p, mode, amode=None, wmode=None):
    """the unculled saving forward (and, with the two adjoint modes, its backward) of a problem -- computed once, left unchanged"""
    key = (p["R"], p["S"], mode)
    if key not in _FULL:
        _FULL[key] = tn.cpp.mlp_forward_gather_train(p["vi"], p["bc"], p["field"], p["dirs"], p["w"], p["S"], ray_head_bias=p["bias"],
                                                     mode=mode)
    if amode is None:
        return _FULL[key]
    bkey = key + (amode, wmode)
    if bkey not in _FULL:
        sigma, rgb, saved = _FULL[key]
        _FULL[bkey] = _backward(tn, p, saved, sigma, rgb, amode, wmode)
    return _FULL[bkey]


def _indexed_forward(tn, p, live, k, mode):
    """the indexed saving forward into NaN-filled outputs"""
    dev = p["field"].device
    sigma = torch.full((p["n"],), float("nan"), device=dev)
    rgb = torch.full((p["n"], 3), float("nan"), device=dev)
    out = tn.cpp.mlp_forward_gather_train_indexed(live, k, p["vi"], p["bc"], p["field"], p["dirs"], p["w"], p["S"], ray_head_bias=p["bias"],
                                                  mode=mode, sigma=sigma, rgb=rgb)
    assert out[0] is sigma and out[1] is rgb
    saved = out[2]
    assert (saved.n, saved.n_samples, saved.S) == (k, p["n"], p["S"]) and saved.live is live
    assert saved.acts.shape == (576, k) and saved.masks.shape == (4, k, 2)
    return sigma, rgb, saved


def _columns(acts, n):
    """[576, n] quad-major saves -> [n, 576] with one row per sample"""
    return torch.cat([_quad_major(acts[a:b], n) for a, b in ((0, 64), (64, 192), (192, 320), (320, 448), (448, 576))], 1)


# ------------------------------------------------------------------------------------------------------------ identity list
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R,S", list(SHAPES))
def test_identity_list_is_the_unindexed_entry_bit_for_bit(tn, device, mode, R, S):
    p = _problem(R, S, device)
    n = p["n"]
    live = torch.arange(n, dtype=torch.int32, device=device)
    f_sigma, f_rgb, f_saved = _full(tn, p, mode)
    sigma, rgb, saved = _indexed_forward(tn, p, live, n, mode)
    assert _same(sigma, f_sigma) and _same(rgb, f_rgb)
    assert _same(saved.acts, f_saved.acts) and torch.equal(saved.masks, f_saved.masks)
    for amode, wmode in (("fp32", "fp32"), ("bf16x3", "bf16x3")):
        want = _full(tn, p, mode, amode, wmode)
        got = _backward(tn, p, saved, sigma, rgb, amode, wmode)
        for name in GRADS:
            assert float(want["grads"][name].abs().max()) > 0, name
            assert _same(got["grads"][name], want["grads"][name]), (amode, wmode, name)
        assert float(want["d_ray"].abs().max()) > 0 and _same(got["d_ray"], want["d_ray"]), (amode, wmode)
        assert _same(got["bary"], want["bary"]) and _same(got["dx0"], want["dx0"])


# ------------------------------------------------------------------------------------------------------------ sub-lists
def _sub_list(n, k, seed, dev, S=None):
    """k of n samples, ascending; with S: none of them on a ray r with r % 7 == 3 (rays without a live sample) while k allows it"""
    pool = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    if S is not None:
        kept = pool[torch.div(pool, S, rounding_mode="floor") % 7 != 3]
        pool = kept if kept.numel() >= k else pool
    listed = torch.sort(pool[:k]).values
    live = torch.full((n,), NOT_A_SAMPLE, dtype=torch.int32)       # (entries beyond the list: not a sample)
    live[:k] = listed.to(torch.int32)
    return live.to(dev), listed.to(dev)


def _float64_sums(p, live_idx, saved, chain, dx0):
    """float64 statements of every sum from the run's own compact buffers: {name: (value, sum of the magnitudes of the terms,
    largest number of terms of an element)}"""
    k, S = live_idx.numel(), p["S"]
    act = {name: _quad_major(saved.acts[a:b], k).double() for name, (a, b) in zip(ACTS, ((0, 64), (64, 192), (192, 320), (320, 448), (448, 576)))}
    d = {name: _quad_major(getattr(chain, name), k).double() for name in DS}
    dhead = chain.dhead.double()
    ray = torch.div(live_idx, S, rounding_mode="floor")
    enc = render.direction_encoding(p["dirs"].float()).double()[ray]      # (PyTorch's fp32 statement of the library's fp32 table)
    ref = {}
    for name, bias, a, x in (("wh", "bh", d["d4"], torch.cat([enc, act["h3"]], 1)), ("w3", "b3", d["d3"], act["h2"]),
                             ("w2", "b2", d["d2"], act["h1"]), ("w1", "b1", d["d1"], act["x0"])):
        ref[name] = (a.t() @ x, a.abs().t() @ x.abs(), k)
        ref[bias] = (a.sum(0), a.abs().sum(0), k)
    ref["wd"] = ((dhead[0][:, None] * act["h3"]).sum(0)[None], (dhead[0].abs()[:, None] * act["h3"].abs()).sum(0)[None], k)
    ref["wr"] = (dhead[1:4] @ act["h4"], dhead[1:4].abs() @ act["h4"].abs(), k)
    ref["bd"] = (dhead[0].sum()[None], dhead[0].abs().sum()[None], k)
    ref["br"] = (dhead[1:4].sum(1), dhead[1:4].abs().sum(1), k)
    # per-ray sums of d4
    R = p["R"]
    per_ray = torch.zeros(R, 128, dtype=torch.float64, device=ray.device).index_add_(0, ray, d["d4"])
    per_ray_abs = torch.zeros_like(per_ray).index_add_(0, ray, d["d4"].abs())
    counts = torch.bincount(ray, minlength=R)
    ref["d_ray"] = (per_ray, per_ray_abs, counts)
    # the gather's adjoint on the compacted rows (tests/gather_cases.py: adjoint_ref)
    vi = p["vi"][live_idx].cpu().numpy()
    bc = p["bc"][live_idx].cpu().numpy()
    adj, adj_A, cnt = gc.adjoint_ref(vi, bc, dx0.cpu().numpy(), p["V"])
    assert cnt.max() <= gc.MAX_COUNT
    ref["field"] = (torch.from_numpy(adj).t(), torch.from_numpy(gc.adjoint_bound(dict(count=cnt, adj_A=adj_A))).t(), None)
    return ref


def _check_sums(label, ref, got_w, got_fp32, x3):
    """got_w: the weight gradients of the mode under test; got_fp32: those of the fp32 GEMMs on the same buffers (y of the bf16x3
    bound); everything else is fp32 in every mode"""
    def report(name, err, bound):
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{label} {name}: max err / bound = {worst:.3f} (max err {float(err.max()):.3e})")
        assert bool((err <= bound).all()), (label, name, worst)

    for name in GRADS:
        d64, mag, c = ref[name]
        assert float(d64.abs().max()) > 0, name
        apriori = (c + 1) * U * mag
        err32 = (got_fp32[name].double() - d64).abs()
        report(name + " (fp32)", err32, apriori)
        if x3 and name in ("w1", "w2", "w3", "wh"):
            report(name + " (bf16x3)", (got_w[name].double() - d64).abs(), 2.0 ** -21 * mag + 4.0 * float(err32.max()))
        elif x3 and name in ("b1", "b2", "b3", "bh", "wd"):
            report(name + " (bf16x3)", (got_w[name].double() - d64).abs(), 4.0 * float(err32.max()) + 2.0 ** -24 * mag)
        elif x3:
            assert _same(got_w[name], got_fp32[name]), name          # the rgb head's kernels: the mode does not touch them


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R,S", list(SHAPES))
def test_sub_lists(tn, device, mode, R, S):
    p = _problem(R, S, device)
    n = p["n"]
    f_sigma, f_rgb, f_saved = _full(tn, p, mode)
    f_cols = _columns(f_saved.acts, n)
    for k in SHAPES[(R, S)][1]:
        live, listed = _sub_list(n, k, 31 * S + k, device, S)
        is_listed = torch.zeros(n, dtype=torch.bool, device=device)
        is_listed[listed] = True
        sigma, rgb, saved = _indexed_forward(tn, p, live, k, mode)
        # outputs: the unculled saving forward's bits at the listed samples, the NaN pre-fill everywhere else
        assert _same(sigma[listed], f_sigma[listed]) and _same(rgb[listed], f_rgb[listed]), k
        assert bool(torch.isnan(sigma[~is_listed]).all()) and bool(torch.isnan(rgb[~is_listed]).all()), k
        assert not bool(torch.isnan(sigma[listed]).any())
        # saves: slot i = column live[i]
        assert _same(_columns(saved.acts, k), f_cols[listed]), k
        assert torch.equal(saved.masks, f_saved.masks[:, listed]), k
        for amode, wmode in (("fp32", "fp32"), ("bf16x3", "bf16x3")):
            want = _full(tn, p, mode, amode, wmode)
            got = _backward(tn, p, saved, sigma, rgb, amode, wmode)
            ch, fch = got["chain"], want["chain"]
            for name in DS:
                assert _same(_quad_major(getattr(ch, name), k), _quad_major(getattr(fch, name), n)[listed]), (k, amode, name)
            assert _same(ch.dhead, fch.dhead[:, listed]) and _same(got["dx0"], want["dx0"][listed]), (k, amode)
            assert got["bary"].shape == (n, 3)
            assert torch.equal(got["bary"][listed], want["bary"][listed]) and not bool(got["bary"][~is_listed].any()), (k, amode)
            assert got["d_ray"].shape == (R, 128) and got["field"].shape == (64, p["V"])
            if k == 0:       # the empty list: no launch, every sum is empty
                assert not bool(got["field"].any()) and not bool(got["d_ray"].any())
                assert all(not bool(g.any()) for g in got["grads"].values())
                continue
            if k not in (257, 70000):
                continue
            # sums over the list against float64 of the run's own compact buffers
            ref = _float64_sums(p, listed, saved, ch, got["dx0"])
            fp32 = got if wmode == "fp32" else _backward(tn, p, saved, sigma, rgb, amode, "fp32")
            label = f"{R}x{S} k={k} {mode}/{amode}/{wmode}"
            _check_sums(label, ref, got["grads"], fp32["grads"], wmode == "bf16x3")
            d64, bound, _ = ref["field"]
            err = (got["field"].double().cpu() - d64).abs()
            print(f"{label} field: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert float(d64.abs().max()) > 0 and bool((err <= bound).all())
            d64, mag, counts = ref["d_ray"]
            assert bool((counts == 0).any()) or k == 70000
            assert not bool(got["d_ray"][counts == 0].any())              # a ray without a live sample: exactly zero
            err = (got["d_ray"].double() - d64).abs()
            assert bool((err <= (counts[:, None] + 1) * U * mag).all()) and float(d64.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ head-layer dW
def _raw_param_grads(tn, device, b, dirs, S, mode, live=None, n_samples=None):
    """tn_mlp_param_grads_ex (live None) or tn_mlp_param_grads_indexed through the C entry, into zero-filled gradients"""
    cpp = tn.cpp
    lib = cpp._lib.load()
    n = b["dhead"].shape[1]
    grads = [torch.zeros(shp, dtype=torch.float32, device=device) for shp in cpp._WEIGHT_SHAPES]
    gs = cpp._MlpWeightsStruct(*[g.data_ptr() for g in grads])
    bs = cpp._MlpBackwardBuffers(*[b[k].data_ptr() for k in ACTS], None, *[b[k].data_ptr() for k in DS], b["dhead"].data_ptr(), None)
    h = _handle(tn, device).handle
    if live is None:
        cpp._lib.check(lib.tn_mlp_param_grads_ex(h, n, S, dirs.data_ptr(), C.byref(bs), C.byref(gs), mode, cpp._stream(device)))
    else:
        cpp._lib.check(lib.tn_mlp_param_grads_indexed(h, n, n_samples, S, live.data_ptr(), dirs.data_ptr(), C.byref(bs), C.byref(gs), mode,
                                                      cpp._stream(device)))
    torch.cuda.synchronize()
    return dict(zip(GRADS, grads))


def _one_hot_buffers(n, col, device, unit=False):
    """buffers of n columns whose d4 is zero but for column `col`: d4[f] = 2^(f % 5 - 2), a power of two, so that d4[f] enc[k] is
    ONE exact product in either arithmetic (unit: d4[f] = 1); h3 holds small integers, everything else zeros"""
    g = torch.Generator().manual_seed(col)
    b = {k: torch.zeros(n, 64 if k == "x0" else 128) for k in ACTS + DS}
    b["h3"] = torch.randint(-8, 9, (n, 128), generator=g).float()
    b["d4"][col] = torch.ones(128) if unit else 2.0 ** (torch.arange(128) % 5 - 2).float()
    out = {k: _to_quad_major(v.to(device)) for k, v in b.items()}
    out["dhead"] = torch.zeros(4, n, device=device)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_head_layer_weight_gradient_takes_the_ray_of_the_listed_sample(tn, device, mode):
    R, S, k = 64, 5, 257
    n = R * S
    live, listed = _sub_list(n, k, 99, device)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=torch.Generator().manual_seed(4)), dim=-1).to(device)
    enc = render.direction_encoding(dirs)
    ray = torch.div(listed, S, rounding_mode="floor")
    change = int(torch.nonzero(ray[1:] != ray[:-1])[5]) + 1       # a ray change in the list: slots change - 1 | change
    assert ray[change] != ray[change - 1]
    d4 = 2.0 ** (torch.arange(128, device=device) % 5 - 2).float()
    for slot in (0, 31, 32, change - 1, change, k - 1):           # 31 | 32: the edge of the first dW slice
        got = _raw_param_grads(tn, device, _one_hot_buffers(k, slot, device), dirs, S, mode, live=live, n_samples=n)["wh"][:, :27]
        r = int(ray[slot])
        # the library's fp32 encoding table is internal; the row of ray r is read back through the UNINDEXED entry with a unit
        # column at the ray's first sample (1 * enc + zeros: exact), and the statement is then one exact product per entry:
        # dWh[f, k] = fl(d4[f] * enc(ray of live[slot])[k])
        table = _raw_param_grads(tn, device, _one_hot_buffers(n, r * S, device, unit=True), dirs, S, mode)["wh"][:, :27]
        assert _same(table, table[:1].expand(128, 27)) and float(table.abs().max()) > 0
        assert _same(got, d4[:, None] * table[:1]), (slot, r)
        # (and the unindexed entry with the same column at the sample itself gives the same bits)
        own = _raw_param_grads(tn, device, _one_hot_buffers(n, int(listed[slot]), device), dirs, S, mode)["wh"][:, :27]
        assert _same(got, own), (slot, r)
        # and that IS ray r: of all rays' encodings (PyTorch's statement of the table) the nearest
        others = (d4[:, None, None] * enc[None]).permute(1, 0, 2)                              # [R, 128, 27]
        assert int((others - got[None]).abs().amax((1, 2)).argmin()) == r, (slot, r)


def test_entry_arguments(tn, device):
    p = _problem(64, 5, device)
    live = torch.arange(p["n"], dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="mlp mode must be"):
        tn.cpp.mlp_forward_gather_train_indexed(live, 10, p["vi"], p["bc"], p["field"], p["dirs"], p["w"], p["S"], mode="bf16")
    lib = tn.cpp._lib.load()
    h = tn.cpp.fused_mlp(p["w"]).handle
    a = torch.empty(576, 10, device=device)
    m = torch.empty(4, 10, 2, dtype=torch.int64, device=device)
    bs = tn.cpp._backward_buffers(a, m)
    rc = lib.tn_mlp_forward_gather_train_indexed(h, 10, p["n"], p["S"], live.data_ptr(), p["vi"].data_ptr(), p["bc"].data_ptr(),
                                                 tn.cpp.field_vertex_major(p["field"]).data_ptr(), p["dirs"].data_ptr(), 2,
                                                 torch.empty(p["n"], device=device).data_ptr(),
                                                 torch.empty(p["n"], 3, device=device).data_ptr(), C.byref(bs), None, None)
    assert rc != 0 and b"mode 2" in lib.tn_last_error()
    # a list entry that is no sample stores no output
    bad = live.clone()
    bad[3] = NOT_A_SAMPLE
    sigma, rgb, _ = _indexed_forward(tn, p, bad, 10, "fp32")
    keep = torch.arange(p["n"], device=device) < 10
    keep[3] = False
    assert torch.equal(torch.isnan(sigma), ~keep) and torch.equal(torch.isnan(rgb).all(1), ~keep)
    # rows of 1, 3 and 4 words by the list; other widths are refused
    sub, listed = _sub_list(p["n"], 77, 5, device)
    for src in (p["d_sigma"], p["bc"], p["vi"]):
        assert torch.equal(tn.cpp.compact_rows(src, sub, 77), src[listed])
    assert tn.cpp.compact_rows(p["vi"], sub, 0).shape == (0, 4)
    with pytest.raises(RuntimeError, match="1, 3 or 4"):
        tn.cpp.compact_rows(torch.zeros(8, 2, device=device), sub, 3)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def small_scene(tn, device, scenes):
    """tests/test_occupancy_gpu.py's: 330 rays into a 900-point mesh + 37 that miss, shuffled"""
    pts, cells = scenes.random_mesh(900, 12)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(330, 13)
    o, d = np.concatenate([o, o[:37] + 40.0]), np.concatenate([d, d[:37]])
    perm = np.random.default_rng(1).permutation(len(o))
    torch.manual_seed(5)
    mlp = render.TetraMLP().to(device)
    field = torch.randn(64, len(pts), device=device) * 0.5
    to = torch.from_numpy(np.ascontiguousarray(o[perm], dtype=np.float32)).to(device)
    td = torch.from_numpy(np.ascontiguousarray(d[perm], dtype=np.float32)).to(device)
    return dict(tr=tr, mlp=mlp, field=field, o=to, d=td, T=len(cells), verts=torch.from_numpy(pts).to(device))


def _record_backward(tn, monkeypatch, records):
    """cpp.mlp_backward also leaves the run's own compact buffers in `records`, for the magnitudes of the sums"""
    backward = tn.cpp.mlp_backward

    def recording(saved, *a, **k):
        want = dict(k, want_ray_head_grad=True, return_dx0=True, return_chain=True)
        res = backward(saved, *a, **want)
        records.append(dict(saved=saved, d_ray=res[2], dx0=res[-2], chain=res[-1], dirs=a[3], vi=a[0].detach(), bc=a[1].detach(),
                            V=a[2].shape[1]))
        out = res[:2] + ((res[2],) if k.get("want_ray_head_grad") else ())
        return out + ((res[3],) if k.get("want_bary_grad") else ())

    monkeypatch.setattr(tn.cpp, "mlp_backward", recording)


def _term_magnitudes(rec, S):
    """sum of the magnitudes of the terms of every summed gradient of one recorded node, from its compact buffers: the twelve
    parameter tensors; "ray": per feature, the largest per-ray sum of |d4|.  "field_bound" [64, V] is a bound already: tests/
    gather_cases.py's adjoint_bound per vertex -- (c + 1) u sum |w| |d x0| + c 2^-126 over the c terms the vertex collects -- from
    the compacted vertex ids, barycentrics and d x0 rows of the listed samples"""
    saved = rec["saved"]
    k = saved.n
    live_idx = saved.live[:k].long()
    act = {name: _quad_major(saved.acts[a:b], k).double().abs() for name, (a, b) in zip(ACTS, ((0, 64), (64, 192), (192, 320), (320, 448), (448, 576)))}
    dd = {name: _quad_major(getattr(rec["chain"], name), k).double().abs() for name in DS}
    dhead = rec["chain"].dhead.double().abs()
    ray = torch.div(live_idx, S, rounding_mode="floor")
    enc = render.direction_encoding(rec["dirs"].detach().float()).double()[ray].abs()
    per_ray = torch.zeros(rec["dirs"].shape[0], 128, dtype=torch.float64, device=ray.device).index_add_(0, ray, dd["d4"])
    vi, bc = rec["vi"].reshape(-1, 4)[live_idx].cpu().numpy(), rec["bc"].reshape(-1, 3)[live_idx].float().cpu().numpy()
    _, adj_A, cnt = gc.adjoint_ref(vi, bc, rec["dx0"].detach().cpu().numpy(), rec["V"])
    field_bound = torch.from_numpy(gc.adjoint_bound(dict(count=cnt, adj_A=adj_A))).t().to(ray.device)
    return {"w1": dd["d1"].t() @ act["x0"], "b1": dd["d1"].sum(0), "w2": dd["d2"].t() @ act["h1"], "b2": dd["d2"].sum(0),
            "w3": dd["d3"].t() @ act["h2"], "b3": dd["d3"].sum(0), "wd": (dhead[0][:, None] * act["h3"]).sum(0)[None],
            "bd": dhead[0].sum()[None], "wh": dd["d4"].t() @ torch.cat([enc, act["h3"]], 1), "bh": dd["d4"].sum(0),
            "wr": dhead[1:4] @ act["h4"], "br": dhead[1:4].sum(1), "field_bound": field_bound, "ray": per_ray.amax(0)[None]}


class _Run:
    """one training batch of a renderer: outputs, the gradients of the field, the twelve MLP tensors and the per-ray bias (and of
    origins / directions / vertices with position gradients), and what the recorded MLP nodes' adjoints left"""

    def __init__(self, tn, sc, S_fine, sync_free, modes, position_gradients, masked, **call_kw):
        with pytest.MonkeyPatch.context() as mp:
            self._run(mp, tn, sc, S_fine, sync_free, modes, position_gradients, masked, **call_kw)

    def _run(self, monkeypatch, tn, sc, S_fine, sync_free, modes, position_gradients, masked, **call_kw):
        device = sc["field"].device
        mlp = render.TetraMLP().to(device)
        mlp.load_state_dict(sc["mlp"].state_dict())
        field = sc["field"].clone().requires_grad_(True)
        hb = (torch.randn(len(sc["o"]), 128, generator=torch.Generator().manual_seed(8)) * 0.5).to(device).requires_grad_(True)
        rd = render.TetraRenderer(sc["tr"], field, mlp, 11, 256, num_fine_samples=S_fine, sync_free_train=sync_free, sync_free_min_hits=0.0,
                                  train_mlp_mode=modes, train_adjoint_mode=modes, train_dw_mode=modes)
        self.leaves = [field] + list(mlp.parameters()) + [hb]
        kw = dict(ray_head_bias=hb)
        o, d = sc["o"], sc["d"]
        if position_gradients:
            o, d = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
            verts = sc["verts"].clone().requires_grad_(True)
            kw.update(position_gradients=True, vertices=verts)
            self.leaves += [o, d, verts]
        if not sync_free:
            hit = int((rd._trace(o.detach(), d.detach())["num_visited_cells"] > 0).sum())
            g = torch.Generator().manual_seed(21)
            kw["rand"] = {"coarse": torch.rand(hit, 12, generator=g).to(device), "fine": torch.rand(hit, S_fine + 1, generator=g).to(device)}
        self.records = []
        if masked is not None:
            # the unculled path of render_train with the EXISTING ops behind a torch.where mask: the coarse densities of
            # mlp_forward_gather and the outputs of the unculled _FusedMlpFunction are masked with cull_mask_statement on the cells
            # the last _locate matched
            occ, thr = masked
            cells = []
            locate = rd._locate
            monkeypatch.setattr(rd, "_locate", lambda *a, **k: (lambda t: (cells.append(t["cell_indices"]), t)[1])(locate(*a, **k)))
            gather = tn.cpp.mlp_forward_gather

            def coarse(*a, **k):
                sigma = gather(*a, **k)
                assert a[3] is None          # (render_train calls it for the coarse densities only)
                culled = render.cull_mask_statement(cells[-1], occ, thr).view(-1)
                return torch.where(culled, torch.zeros_like(sigma), sigma)

            monkeypatch.setattr(tn.cpp, "mlp_forward_gather", coarse)
            node = render._FusedMlpFunction

            class Masked:
                @staticmethod
                def apply(*a):
                    sigma, col = node.apply(*a)
                    culled = render.cull_mask_statement(cells[-1], occ, thr).view(-1)
                    self.culled = culled
                    return torch.where(culled, torch.zeros_like(sigma), sigma), torch.where(culled[:, None], torch.zeros_like(col), col)

            monkeypatch.setattr(render, "_FusedMlpFunction", Masked)
        else:
            _record_backward(tn, monkeypatch, self.records)
        torch.manual_seed(9)
        self.out = rd.render_train(o, d, gradient_scaling=True, **kw, **call_kw)
        target = torch.rand(len(sc["o"]), 3, generator=torch.Generator().manual_seed(2)).to(device)
        (((self.out["rgb"] - target) ** 2).mean() + 0.1 * self.out["accumulation"].mean()).backward()
        self.grads = [torch.zeros_like(x) if x.grad is None else x.grad.clone() for x in self.leaves]


E2E = [(7, True, "fp32", False), (7, False, "fp32", False), (0, True, "fp32", False), (0, False, "bf16x3", False), (7, False, "fp32", True),
       (7, True, "bf16x3", False)]


@pytest.mark.parametrize("S_fine,sync_free,modes,position_gradients", E2E)
def test_render_train_culled_end_to_end(tn, device, small_scene, monkeypatch, S_fine, sync_free, modes, position_gradients):
    sc = small_scene
    monkeypatch.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device)
    keys = ("rgb", "accumulation", "depth", "ray_mask")
    args = (tn, sc, S_fine, sync_free, modes, position_gradients)

    plain = _Run(*args, masked=(occ, 0.0))
    # threshold 0 culls nothing: the outputs of the plain call
    zero = _Run(*args, masked=None, occupancy=occ, occupancy_threshold=0.0)
    for k in keys:
        assert torch.equal(zero.out[k], plain.out[k]), k
    # a threshold above every occupancy: n_live = 0 -- the background frame and zero gradients
    empty = _Run(*args, masked=None, occupancy=occ, occupancy_threshold=2.0)
    assert torch.all(empty.out["accumulation"] == 0) and torch.all(empty.out["rgb"] == 1.0)
    assert all(not bool(g.any()) for g in empty.grads)
    assert sum(r["saved"].n for r in empty.records) == 0

    # the random occupancy at 0.5: the frame assembled from the existing ops with torch.where masking, bit for bit
    want = _Run(*args, masked=(occ, 0.5))
    got = _Run(*args, masked=None, occupancy=occ, occupancy_threshold=0.5)
    n = want.culled.numel()
    assert 0.2 * n < int(want.culled.sum()) < 0.8 * n
    for k in keys:
        assert torch.equal(got.out[k], want.out[k]), k
    assert not torch.equal(got.out["rgb"], plain.out["rgb"])
    assert occ.equal(torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device))      # no decay: no update
    (rec,) = got.records
    saved = rec["saved"]
    assert saved.n == n - int(want.culled.sum()) and saved.n_samples == n
    live_idx = saved.live[:saved.n].long()
    assert torch.equal(live_idx, torch.nonzero(~want.culled)[:, 0])

    # gradients: autograd through the assembly (the unculled node behind the mask) sums the SAME per-sample terms, plus exact
    # zeros, in another order.  Each side is within the bound of its arithmetic of the exact sum -- (c + 1) u sum |terms| for an
    # fp32 sum of c <= n terms (tests/gather_cases.py), + 2^-21 sum |terms| for the bf16x3 GEMMs (tests/test_dw_x3_gpu.py) --
    # hence within twice that of the other; the magnitudes come from the culled run's own compact buffers
    S = 11 + S_fine + (1 if S_fine else 0)
    mags = _term_magnitudes(rec, S)
    rel = 2 * ((n + 1) * U + (2.0 ** -21 if modes == "bf16x3" else 0.0))
    names = ["field"] + GRADS + ["ray"]
    for name, g, w in zip(names, got.grads, want.grads):
        assert bool(torch.isfinite(g).all()) and float(w.abs().max()) > 0, name
        err = (g.detach().double() - w.detach().double()).abs()
        if name == "field":      # the zero terms of the assembly add no rounding: both sides meet the bound of the listed terms
            bound = 2 * mags["field_bound"]
        else:
            bound = rel * (mags[name].expand_as(err) if name == "ray" else mags[name].reshape(err.shape))
        print(f"S_fine={S_fine} sync_free={sync_free} {modes} {name}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), name
    # a ray without a live sample (the rays that miss among them): a per-ray bias gradient of exactly zero
    hb_got, hb_want = got.grads[13], want.grads[13]
    dead = ~hb_want.bool().any(1)
    assert bool(dead.any()) and not bool(hb_got[dead].any())
    if position_gradients:
        g_o, g_d, g_v = got.grads[14:]
        w_o, w_d, w_v = want.grads[14:]
        # the barycentric gradient is per sample (and zero at culled samples in both runs), and the origin's gradient is a fixed
        # function of it per ray: equal.  Directions (+ the view term's per-ray sums) and vertices (atomics): 1e-3 of the largest
        # entry, the tolerance of tests/test_position_gradients.py's wiring test
        assert torch.equal(g_o, w_o) and float(w_o.abs().max()) > 0
        for a, b in ((g_d, w_d), (g_v, w_v)):
            assert float(b.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())


@pytest.mark.parametrize("sync_free", [True, False])
def test_culled_training_with_update_and_several_nodes(tn, device, small_scene, monkeypatch, sync_free):
    """threshold + decay: the update runs after the culled forward, on the masked densities; a list longer than train_node_samples
    goes through one node per slot range and gives the one-node batch's outputs (bit for bit) and gradients"""
    sc = small_scene
    monkeypatch.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
    mlp = render.TetraMLP().to(device)
    mlp.load_state_dict(sc["mlp"].state_dict())
    field = sc["field"].clone().requires_grad_(True)
    rd = render.TetraRenderer(sc["tr"], field, mlp, 11, 256, num_fine_samples=7, sync_free_train=sync_free, sync_free_min_hits=0.0)
    params = [field] + list(mlp.parameters())
    target = torch.rand(len(sc["o"]), 3, generator=torch.Generator().manual_seed(2)).to(device)
    occ0 = torch.rand(sc["T"], generator=torch.Generator().manual_seed(4)).to(device)

    def batch(**kw):
        torch.manual_seed(9)
        for x in params:
            x.grad = None
        out = rd.render_train(sc["o"], sc["d"], **kw)
        ((out["rgb"] - target) ** 2).mean().backward()
        return out, [x.grad.clone() for x in params]

    recorded = []
    real = tn.cpp.occupancy_update
    monkeypatch.setattr(tn.cpp, "occupancy_update", lambda o, c, s, d, **kw: (recorded.append((o.clone(), c.clone(), s.clone(), d)), real(o, c, s, d, **kw))[1])
    occ = occ0.clone()
    records = []
    with pytest.MonkeyPatch.context() as mp:
        _record_backward(tn, mp, records)
        one, g_one = batch(occupancy=occ0.clone(), occupancy_threshold=0.5)
    assert not recorded and len(records) == 1
    upd, g_upd = batch(occupancy=occ, occupancy_threshold=0.5, occupancy_decay=0.75)
    for k in ("rgb", "accumulation", "depth", "ray_mask"):
        assert torch.equal(upd[k], one[k]), k
    assert all(torch.equal(a, b) for a, b in zip(g_upd, g_one))
    (before, cells, sigma, decay), = recorded
    culled = render.cull_mask_statement(cells, occ0, 0.5)
    assert torch.equal(before, occ0) and decay == 0.75 and bool(culled.any()) and not bool(sigma[culled].any())
    want = render.occupancy_update_statement(occ0, cells, sigma, 0.75)
    assert torch.equal(_i32(occ), _i32(want))
    # several nodes: 1000 slots each
    rd.train_node_samples = 1000
    nodes = []
    apply = render._FusedMlpCulledFunction.apply
    monkeypatch.setattr(render._FusedMlpCulledFunction, "apply", staticmethod(lambda *a: (nodes.append(a[1]), apply(*a))[1]))
    many, g_many = batch(occupancy=occ0.clone(), occupancy_threshold=0.5)
    assert len(nodes) > 2 and all(k == 1000 for k in nodes[:-1]) and 0 < nodes[-1] <= 1000
    for k in ("rgb", "accumulation", "depth", "ray_mask"):
        assert torch.equal(many[k], one[k]), k
    # the same terms summed per slot range and then over the nodes: another order of an fp32 sum of c <= n terms, each side within
    # (c + 1) u sum |terms| of the exact sum (tests/gather_cases.py); magnitudes from the one-node run's compact buffers
    mags = _term_magnitudes(records[0], cells.shape[1])
    n = cells.numel()
    for name, a, b in zip(["field"] + GRADS, g_many, g_one):
        err = (a.double() - b.double()).abs()
        bound = 2 * mags["field_bound"] if name == "field" else 2 * (n + 1) * U * mags[name].reshape(err.shape)
        assert float(b.abs().max()) > 0 and bool((err <= bound).all()), name
