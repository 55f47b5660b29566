"""The gather kernels (tn_interp.hip, k_interp_bwd_bary of tn_position_grad.hip, the fused gather_features, the transposition and
the two uint32 helpers) at every edge of their dispatch, on ray-like index streams, against float64.

Inputs and references come from tests/gather_cases.py (checked on the CPU by tests/test_gather_cases.py).  What is asserted:
  forward   every word equals the CPU oracle's (the kernels keep its summation order), and no word outside the [Fd, n] result
            changes (the result sits 64 floats inside a buffer filled with a pattern: the partial-tile float4 stores);
  adjoint   exact fill (small integers and eighths: every partial sum is exact in fp32 in ANY order, so the correct result has
            one bit pattern): every word equals the float64 sum, on all entries, a vertex nobody samples stays +0, a pre-filled
            gradient becomes initial + sum;  random fill: |got - float64| <= (c + 1) 2^-24 A + c 2^-126 per element (c terms,
            A = sum |w| |g|: gather_cases.py derives it);
  sizes     the smallest that reach each branch: tile and batch edges of every kernel, the widths on either side of each vector
            path, run lengths around the quarter split of the deterministic adjoint, V past its grid, and for every grid-stride
            loop one case one block past its grid cap (SECOND_TRIP below quotes the launchers' constants).
The entry points are called through ctypes where a result pointer inside a guarded buffer or an entry without a Python wrapper
is needed.  `RATIO` lines (pytest -s) are what profiles/gather_edge_errors.txt records."""
import importlib

import numpy as np
import pytest
import torch

import gather_cases as gc

pytestmark = pytest.mark.gpu

PAD = 64          # words of pattern on either side of a guarded result (256 bytes: the result stays 16-byte aligned)


def _clib():
    return importlib.import_module("tetra-nerf_amd._lib")


def _call(fn, *args):
    _clib().check(fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]))


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)          # (a copy: the shared cases are read-only arrays)


class Guarded:
    """`words` 32-bit words of result between two PAD-word margins, all pre-filled with a pattern"""

    def __init__(self, words, device):
        total = words + 2 * PAD
        self.words = words
        self.pattern = ((torch.arange(total, dtype=torch.int64, device=device) * 2654435761 + 12345) % (1 << 31)).to(torch.int32)
        self.buf = self.pattern.clone()
        self.inner = self.buf[PAD:PAD + words]
        assert self.inner.data_ptr() % 16 == 0

    def margins_intact(self):
        e = PAD + self.words
        return torch.equal(self.buf[:PAD], self.pattern[:PAD]) and torch.equal(self.buf[e:], self.pattern[e:])

    def untouched(self):
        """mask over the inner words that still hold the pattern"""
        return self.inner == self.pattern[PAD:PAD + self.words]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ratio(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- forward -----------------------------------------------------------------------------------------------------------
def _forward_both_entries(lib, device, vi, bc, field):
    """tn_interpolate_values_vm (on torch's transposition of the field) and tn_interpolate_values (which transposes itself), each
    into a guarded buffer -> two [Fd, n] arrays"""
    n, D = vi.shape
    Fd, V = field.shape
    tvi, tbc, tf = _dev(vi, device), _dev(bc, device), _dev(field, device)
    tft = tf.t().contiguous()
    outs = []
    for entry in ("vm", "fm"):
        res = Guarded(Fd * n, device)
        if entry == "vm":
            _call(lib.tn_interpolate_values_vm, D, n, Fd, tvi, tbc, tft, res.inner, _stream(device))
        else:
            _call(lib.tn_interpolate_values, D, V, n, Fd, tvi, tbc, tf, res.inner, _stream(device))
        torch.cuda.synchronize()
        assert res.margins_intact(), f"{entry}: a word outside the [Fd, n] result was written"
        outs.append(res.inner.view(torch.float32).view(Fd, n).cpu().numpy())
    return outs


def _check_forward(lib, device, oracle, D, Fd, n):
    c = gc.case(D, Fd, n, "random")
    want = np.ascontiguousarray(np.moveaxis(oracle.interpolate_values(c["vi"], c["bc"], c["field"]), -1, 0))
    for name, got in zip(("vm", "fm"), _forward_both_entries(lib, device, c["vi"], c["bc"], c["field"])):
        bad = np.argwhere(_bits(got) != _bits(want))
        assert len(bad) == 0, (name, len(bad), "first (feature, sample):", bad[0].tolist(), c["vi"][bad[0][1]].tolist())
    bound = (D + 1) * gc.U * c["fwd_A"]
    print(f"RATIO forward D={D} Fd={Fd} n={n}: kernel = oracle {_ratio(np.abs(want.T.astype(np.float64) - c['fwd']), bound):.3f}")


@pytest.mark.parametrize("D,Fd,n", gc.FORWARD64_CASES)
def test_forward_fd64_bit_equal_to_oracle(tn, device, oracle, D, Fd, n):
    """k_interp_fwd64: n = 1 .. 1028 covers a lone sample, the 8-sample lane group and the 64-sample tile on either side, tiles
    whose lane groups store wide and whose last one stores scalar (252, 260: n % 4 == 0 and a partial group), odd n (scalar
    stores throughout) and more than one block (256 samples per block)."""
    _check_forward(_clib().load(), device, oracle, D, Fd, n)


@pytest.mark.parametrize("D,Fd,n", gc.FORWARD_CASES)
def test_forward_generic_bit_equal_to_oracle(tn, device, oracle, D, Fd, n):
    """k_interp_fwd: widths on either side of a 32-feature half (31, 32, 33), of the 64-feature block (60, 63, 65), with and
    without 16-byte rows (Fd % 4), one wave taking both the vector and the scalar branch (36: features 0..31 vector, 32..35
    scalar), several blocks of features (96 .. 192); n on either side of the 32-sample tile and the 128-sample block."""
    _check_forward(_clib().load(), device, oracle, D, Fd, n)


def test_fused_gather_equals_two_step(tn, device):
    """gather_features (tn_mlp_common.h) inside mlp_forward_gather against interpolate_values followed by mlp_forward, on a walk
    stream with single-EMPTY slots and duplicates; the tolerances of test_render_gpu.py::test_mlp_forward_gather_equals_two_step."""
    render = importlib.import_module("tetra-nerf_amd.render")
    torch.manual_seed(5)
    mlp = render.TetraMLP().to(device)
    w = render.mlp_weights(mlp)
    for R, S in ((1, 1), (5, 37), (40, 96)):
        rng = np.random.default_rng([R, S])
        V = 3000
        vi, bc = gc.walk_stream(rng, R * S, V, 4)
        if R * S >= 24:
            st = gc.stream_stats(vi)
            assert st["single_empty"] >= 2 and st["duplicate"] >= 1 and st["permuted_carry"] >= 1
        field = torch.randn(64, V, device=device)
        dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=device), dim=-1)
        tvi, tbc = _dev(vi, device).view(R, S, 4), _dev(bc, device).view(R, S, 3)
        for mode in ("fp32", "bf16x3"):
            feats = tn.cpp.interpolate_values(tvi, tbc, field)
            s2, c2 = tn.cpp.mlp_forward(feats.moveaxis(-1, 0).reshape(64, -1), dirs, w, S, mode=mode)
            s1, c1 = tn.cpp.mlp_forward_gather(tvi, tbc, field, dirs, w, S, mode=mode)
            np.testing.assert_allclose(s1.cpu().numpy(), s2.cpu().numpy(), rtol=1e-5, atol=2e-6)
            np.testing.assert_allclose(c1.cpu().numpy(), c2.cpu().numpy(), rtol=0, atol=2e-6)


# ---- adjoints ----------------------------------------------------------------------------------------------------------
def _initial(c, Fd, fill, device):
    """what the accumulating entries start from: integers on the exact fill (initial + sum stays exact), zeros otherwise (the
    bound has no term for a rounding at the size of an initial value)"""
    if fill != "exact":
        return torch.zeros(c["V"], Fd, device=device)
    g = torch.Generator().manual_seed(c["V"] + Fd)
    return torch.randint(-8, 9, (c["V"], Fd), generator=g).float().to(device)


def _check_adjoint(got, c, fill, what, init=None):
    """got [V, Fd] fp32 against the float64 sum (+ the initial contents)"""
    want = c["adj"] if init is None else c["adj"] + init.cpu().numpy().astype(np.float64)
    if fill == "exact":
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), want)
        bad = np.argwhere(_bits(got) != _bits(want32))
        assert len(bad) == 0, (what, len(bad), "first (vertex, feature):", bad[0].tolist(),
                               float(got[tuple(bad[0])]), float(want32[tuple(bad[0])]), int(c["count"][bad[0][0]]))
        return 0.0
    err, bound = np.abs(got.astype(np.float64) - want), gc.adjoint_bound(c)
    r = _ratio(err, bound)
    assert (err <= bound).all(), (what, r, np.argwhere(err > bound)[0].tolist())
    return r


def _atomic_entries(lib, device, c, fill):
    """-> {entry: [V, Fd] numpy}, and the initial contents tn_interpolate_values_backward_vm accumulated into"""
    n, D = c["vi"].shape
    Fd, V = c["g"].shape[1], c["V"]
    vi, bc, g = _dev(c["vi"], device), _dev(c["bc"], device), _dev(c["g"], device)
    st = _stream(device)
    init = _initial(c, Fd, fill, device)
    vm = init.clone()
    _call(lib.tn_interpolate_values_backward_vm, D, n, Fd, vi, bc, g, vm, st)
    rows = torch.full((Fd, V), float("nan"), device=device)
    _call(lib.tn_interpolate_values_backward_rows, D, V, n, Fd, vi, bc, g, rows, st)
    g_fm = g.t().contiguous()
    fm = torch.full((Fd, V), float("nan"), device=device)
    _call(lib.tn_interpolate_values_backward, D, V, n, Fd, vi, bc, g_fm, fm, st)
    torch.cuda.synchronize()
    return dict(vm=vm.cpu().numpy(), rows=rows.t().cpu().numpy(), fm=fm.t().cpu().numpy()), init


def _oracle_ratio(oracle, c):
    adj = oracle.interpolate_values_backward(c["vi"], c["bc"], c["field"], c["g"]).astype(np.float64).T
    return _ratio(np.abs(adj - c["adj"]), gc.adjoint_bound(c))


@pytest.mark.parametrize("fill", ["exact", "random"])
@pytest.mark.parametrize("D,Fd,n", gc.ADJOINT_CASES)
def test_adjoint_atomic(tn, device, oracle, D, Fd, n, fill):
    """k_interp_bwd through its three entries.  n on either side of the 8-sample batch, the 64-sample tile and the 256-sample
    block, with a tuple change forced on the last sample of each (gather_cases.EDGES); Fd on either side of the 64-lane feature
    block; D = 6 and D = 2 included."""
    c = gc.case(D, Fd, n, fill)
    got, init = _atomic_entries(_clib().load(), device, c, fill)
    r = {k: _check_adjoint(v, c, fill, k, init if k == "vm" else None) for k, v in got.items()}
    if fill == "exact":
        unsampled = c["count"] == 0
        for k in ("rows", "fm"):
            assert not _bits(got[k][unsampled]).any(), f"{k}: a vertex nobody samples is not +0"
    else:
        print(f"RATIO adjoint atomic D={D} Fd={Fd} n={n}: kernel vm {r['vm']:.3f} rows {r['rows']:.3f} fm {r['fm']:.3f}, "
              f"oracle {_oracle_ratio(oracle, c):.3f}, max c {int(c['count'].max())}")


def _det_cases():
    out = [("walk", a) for a in gc.ADJOINT_CASES]
    return out + [("run_lengths", None), ("last_vertices", None)]


def _det_case(kind, args, fill):
    if kind == "walk":
        return gc.case(*args, fill)
    return gc.run_length_case(fill) if kind == "run_lengths" else gc.last_vertices_case(fill)


@pytest.mark.parametrize("fill", ["exact", "random"])
@pytest.mark.parametrize("kind,args", _det_cases(), ids=lambda x: x if isinstance(x, str) else "-".join(map(str, x or ("crafted",))))
def test_adjoint_deterministic(tn, device, oracle, kind, args, fill):
    """k_interp_bwd_det on the atomic adjoint's cases, on vertices whose runs have exactly the lengths gather_cases.DET_LENGTHS
    (quarters of len * wave / 4: empty waves below 4, remainders at 5, 7, 9, 33, several 8-pair batches at 700) and on
    V = 16,384 + 37 with only the last 37 vertices sampled (the second trip of the one-block-per-vertex loop)."""
    lib = _clib().load()
    c = _det_case(kind, args, fill)
    n, D = c["vi"].shape
    Fd, V = c["g"].shape[1], c["V"]
    vi, bc, g = _dev(c["vi"], device), _dev(c["bc"], device), _dev(c["g"], device)
    init = _initial(c, Fd, fill, device)
    runs = []
    for _ in range(3):
        out = init.clone()
        _call(lib.tn_interpolate_values_backward_vm_det, D, V, n, Fd, vi, bc, g, out, _stream(device))
        runs.append(out)
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int32), runs[0].view(torch.int32)), "two runs differ"
    got = runs[0].cpu().numpy()
    r = _check_adjoint(got, c, fill, "det", init)
    if fill == "exact":
        atomic = init.clone()
        _call(lib.tn_interpolate_values_backward_vm, D, n, Fd, vi, bc, g, atomic, _stream(device))
        assert np.array_equal(_bits(got), _bits(atomic.cpu().numpy())), "deterministic and atomic adjoint differ"
        assert np.array_equal(_bits(got[c["count"] == 0]), _bits(init.cpu().numpy()[c["count"] == 0]))
    else:
        print(f"RATIO adjoint det {kind} D={D} Fd={Fd} n={n} V={V}: kernel {r:.3f}, oracle {_oracle_ratio(oracle, c):.3f}, "
              f"max c {int(c['count'].max())}")


@pytest.mark.parametrize("fill", ["exact", "random"])
@pytest.mark.parametrize("D,Fd,n", gc.BARY_CASES)
def test_bary_adjoint_on_walk_stream(tn, device, D, Fd, n, fill):
    """k_interp_bwd_bary: Fd = 36 takes the vector and the scalar branch in one wave, 64 the vector branch alone.  Random fill:
    the dot-product bound of test_position_gradients_gpu.py, (2 Fd + 2) u sum |G| (|F[v_k+1]| + |F[v_0]|).  Exact fill
    (differences of integers in [-8, 8], Fd <= 192: every partial sum an integer below 2^24): bit-equal."""
    c = gc.case(D, Fd, n, fill)
    want, A = gc.bary_adjoint_ref(c["vi"], c["g"], c["field"])
    got = tn.cpp.interpolate_values_backward_barycentrics(_dev(c["vi"], device), _dev(c["field"], device), _dev(c["g"], device))
    got = got.cpu().numpy()
    assert got.shape == (n, D - 1) and got.dtype == np.float32
    if fill == "exact":
        assert Fd <= 192 and np.array_equal(_bits(got), _bits(want.astype(np.float32)))
    else:
        err, bound = np.abs(got.astype(np.float64) - want), (2 * Fd + 2) * gc.U * A
        assert (err <= bound).all(), _ratio(err, bound)
        print(f"RATIO bary adjoint D={D} Fd={Fd} n={n}: kernel {_ratio(err, bound):.3f}")


# ---- the second trip of every grid-stride loop -------------------------------------------------------------------------
# n = grid cap x samples per block + 200.  The constants are the launchers':
#   k_interp_fwd64     run_fwd_vm (tn_interp.hip): 4096 blocks of 4 waves x 64 samples
#   k_interp_fwd       run_fwd_vm (tn_interp.hip): 4096 blocks of 4 waves x 32 samples
#   k_interp_bwd_bary  run_bwd_bary (tn_position_grad.hip): 4096 blocks of 4 waves x 32 samples
#   k_interp_bwd       run_bwd_vm (tn_interp.hip): 8192 blocks of 4 waves x 64 samples
SECOND_TRIP = dict(fwd64=4096 * 256 + 200, fwd=4096 * 128 + 200, bary=4096 * 128 + 200, bwd=8192 * 256 + 200)


def _big_stream(seed, n, V, D, exact):
    rng = np.random.default_rng(seed)
    vi, bc = gc.walk_stream(rng, n, V, D, exact=exact)
    return rng, vi, bc


@pytest.mark.parametrize("which,Fd", [("fwd64", 64), ("fwd", 4)])
def test_second_trip_forward(tn, device, oracle, which, Fd):
    n, V, D = SECOND_TRIP[which], 200_000, 4
    assert n == {"fwd64": 1_048_776, "fwd": 524_488}[which]
    rng, vi, bc = _big_stream(11, n, V, D, False)
    field = rng.standard_normal((Fd, V)).astype(np.float32)
    want = np.ascontiguousarray(np.moveaxis(oracle.interpolate_values(vi, bc, field), -1, 0))
    for name, got in zip(("vm", "fm"), _forward_both_entries(_clib().load(), device, vi, bc, field)):
        assert np.array_equal(_bits(got), _bits(want)), name


def test_second_trip_bary_adjoint(tn, device):
    n, V, D, Fd = SECOND_TRIP["bary"], 200_000, 4, 4
    assert n == 524_488
    rng, vi, bc = _big_stream(12, n, V, D, True)
    g, field = gc.fills(rng, n, V, Fd, exact=True)
    want, _ = gc.bary_adjoint_ref(vi, g, field)
    got = tn.cpp.interpolate_values_backward_barycentrics(_dev(vi, device), _dev(field, device), _dev(g, device))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.astype(np.float32)))


def test_second_trip_adjoint(tn, device):
    n, V, D, Fd = SECOND_TRIP["bwd"], 200_000, 4, 8
    assert n == 2_097_352
    rng, vi, bc = _big_stream(13, n, V, D, True)
    g, _ = gc.fills(rng, n, 1, Fd, exact=True)
    want, _, cnt = gc.adjoint_ref(vi, bc, g, V)
    assert 8 * 64 * int(cnt.max()) < 2 ** 24
    out = torch.zeros(V, Fd, device=device)
    _call(_clib().load().tn_interpolate_values_backward_vm, D, n, Fd, _dev(vi, device), _dev(bc, device), _dev(g, device), out,
          _stream(device))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want.astype(np.float32)))


# ---- off the model path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 65), (63, 129), (64, 64), (65, 1), (130, 777), (3, 100_000)])
def test_transpose_bytes_and_margins(tn, device, rows, cols):
    """k_transpose on shapes that are no multiple of its 64 x 64 tile, in either dimension"""
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, cols, generator=g).to(device)
    res = Guarded(rows * cols, device)
    _call(_clib().load().tn_transpose_f32, rows, cols, x, res.inner, _stream(device))
    torch.cuda.synchronize()
    assert res.margins_intact()
    assert torch.equal(res.inner.view(cols, rows), x.t().contiguous().view(torch.int32))


def _ulp(x, dtype):
    return np.spacing(np.abs(np.asarray(x)).astype(dtype)).astype(np.float64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("num", [255, 256, 257, 100_003])
def test_gather_uint32_blocks_and_bad_indices(tn, device, num, dtype):
    """one block short of, equal to and past 256 threads, and many blocks; -1 and out-of-range indices leave their slot"""
    g = torch.Generator().manual_seed(num)
    nv = 1000
    vals = torch.rand(nv, generator=g, dtype=dtype).to(device)
    idx = torch.randint(0, nv, (num,), generator=g, dtype=torch.int32)
    idx[::7] = -1
    idx[3::11] = nv
    idx[5::13] = nv + 12345
    idx = idx.to(device)
    words = vals.element_size() // 4
    res = Guarded(num * words, device)
    _call(_clib().load().tn_gather_uint32, vals.element_size(), nv, num, idx, vals, res.inner, _stream(device))
    torch.cuda.synchronize()
    assert res.margins_intact()
    ok = (idx >= 0) & (idx < nv)
    got = res.inner.view(num, words)
    want = vals[idx.long().clamp(0, nv - 1)].view(torch.int32).view(num, words)
    assert torch.equal(got[ok], want[ok])
    assert bool(res.untouched().view(num, words)[~ok].all())
    # and through the wrapper
    assert torch.equal(tn.gather_uint32(vals, 0, idx)[ok], vals[idx.long()[ok]])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("num", [255, 256, 257, 100_003])
def test_scatter_ema_uint32_unique_indices(tn, device, num, dtype):
    """x[k] = x[k] decay + (1 - decay) v in the tensor's type, within 2 ulp (the compiler may fuse the multiply-add or not); bad
    indices leave the tensor alone.  decay = 0.9 is rounded to the tensor's type on entry; 1 - decay is then exact."""
    g = torch.Generator().manual_seed(num + 1)
    N = num + 50
    x = torch.rand(N, generator=g, dtype=dtype)
    idx = torch.randperm(N, generator=g)[:num].to(torch.int32)
    idx[::7] = -1
    idx[3::11] = N
    idx[5::13] = N + 12345
    v = torch.rand(num, generator=g, dtype=dtype)
    res = x.clone().to(device)
    tn.scatter_ema_uint32_(res, 0, idx.to(device), 0.9, v.to(device))
    d = torch.tensor(0.9, dtype=dtype)
    ok = (idx >= 0) & (idx < N)
    k = idx[ok].long()
    want = x.clone()
    want[k] = x[k] * d + (1 - d) * v[ok]
    got = res.cpu()
    touched = torch.zeros(N, dtype=torch.bool)
    touched[k] = True
    assert torch.equal(got[~touched], x[~touched])
    npd = np.float32 if dtype == torch.float32 else np.float64
    err = (got.double() - want.double()).abs().numpy()
    assert (err <= 2 * _ulp(want.numpy(), npd)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scatter_ema_uint32_repeated_index(tn, device, dtype):
    """An index repeated m times with ONE value v: v + (x - v) decay^m whatever the order of the compare-and-swap updates.
    x and v lie in [0.5, 1), so every intermediate does and one ulp is one number; a step rounds two products and a sum to
    within 1.5 ulp in total and the next step scales the error by decay: (m + 2) ulp covers it for every m."""
    npd = np.float32 if dtype == torch.float32 else np.float64
    ms = (2, 64, 300)
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(len(ms), generator=g, dtype=dtype) / 2 + 0.5)
    vt = (torch.rand(len(ms), generator=g, dtype=dtype) / 2 + 0.5)
    idx = torch.cat([torch.full((m,), j, dtype=torch.int32) for j, m in enumerate(ms)])
    idx = idx[torch.randperm(len(idx), generator=g)]
    res = x.clone().to(device)
    tn.scatter_ema_uint32_(res, 0, idx.to(device), 0.9, vt[idx.long()].to(device))
    d = float(npd(0.9))
    for j, m in enumerate(ms):
        want = float(vt[j]) + (float(x[j]) - float(vt[j])) * d ** m
        assert abs(float(res[j]) - want) <= (m + 2) * float(_ulp(want, npd)), (m, float(res[j]), want)
