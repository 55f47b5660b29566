"""The RAdam step on the GPU: k_radam_field and k_radam_flat (csrc/tn_optim.hip) and optim.FusedRAdam around them.

The reference of every kernel comparison is the CPU statement (optim.radam_statement) on copies of (p, g, m, v) taken before the
step; the comparison is BIT FOR BIT (int32 views) on p, exp_avg, exp_avg_sq and the vertex-major shadow.  Inputs come from
tests/radam_cases.py (|g| in {0} U [1e-6, 1]: no fp32 denormals).  Buffers the kernels write sit inside patterned buffers whose
other words must not change."""
import ctypes
import importlib

import pytest
import torch

import radam_cases as rc

pytestmark = pytest.mark.gpu

PAD = 64                 # floats of pattern on either side of a tensor the kernels write
PATTERN = -123.25
FIELD_V = [1, 3, 63, 64, 65, 127, 128, 129, 4099, 4100]
FLAT_N = [1, 3, 4, 5, 255, 256, 257, 128 * 155, 65537]


@pytest.fixture(scope="module")
def optim():
    return rc.optim()


@pytest.fixture(scope="module")
def render():
    return importlib.import_module("tetra-nerf_amd.render")


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same(x, y):
    return torch.equal(_bits(x.cpu()), _bits(y.cpu()))


class _Embedded:
    """`value` (a CPU tensor) uploaded `offset` floats into a patterned buffer"""

    def __init__(self, value, device, offset=PAD):
        self.n, self.offset = value.numel(), offset
        self.buf = torch.full((offset + self.n + PAD,), PATTERN, device=device)
        self.view = self.buf[offset:offset + self.n].view(value.shape)
        self.view.copy_(value)

    def intact(self):
        return bool((self.buf[:self.offset] == PATTERN).all()) and bool((self.buf[self.offset + self.n:] == PATTERN).all())


def _hyper(optim, decay, lr=rc.LR, betas=rc.BETAS, eps=rc.EPS):
    return optim._Hyper(*optim.hyper_scalars(lr, betas, eps, decay[1], decay[2]))


def _field_step(tn, optim, device, V, p, g, m, v, shadow, step, decay):
    a, adaptive = optim.radam_scalars(step, rc.LR, rc.BETAS)
    hyper = _hyper(optim, decay)
    lib = tn.cpp._lib.load()
    tn.cpp._lib.check(lib.tn_radam_step_field(V, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                              None if shadow is None else shadow.data_ptr(), a, int(adaptive),
                                              ctypes.addressof(hyper), tn.cpp._stream(device)))


# ---- 1: the field kernel ---------------------------------------------------------------------------------------------------------

def _field_case(tn, optim, device, V, decay, with_shadow, offset=PAD, steps=8):
    shape = (64, V)
    p_ref, m_ref, v_ref = rc.parameter(shape, V), torch.zeros(shape), torch.zeros(shape)
    p, m, v = (_Embedded(x, device, offset) for x in (p_ref, m_ref, v_ref))
    shadow = _Embedded(torch.full((V, 64), 7.5), device, offset) if with_shadow else None
    branches = set()
    for step in range(1, steps + 1):
        g_cpu = rc.gradient(shape, V, step)
        g = g_cpu.to(device)
        p_ref, m_ref, v_ref = rc.statement_step(p_ref, g_cpu, m_ref, v_ref, step, decay)
        _field_step(tn, optim, device, V, p.view, g, m.view, v.view, None if shadow is None else shadow.view, step, decay)
        branches.add(optim.radam_scalars(step, rc.LR, rc.BETAS)[1])
        what = (V, decay[0], with_shadow, offset, step)
        assert _same(p.view, p_ref), ("p",) + what
        assert _same(m.view, m_ref), ("exp_avg",) + what
        assert _same(v.view, v_ref), ("exp_avg_sq",) + what
        assert _same(g, g_cpu), ("the gradient was written",) + what
        assert p.intact() and m.intact() and v.intact(), ("a word outside p / exp_avg / exp_avg_sq changed",) + what
        if shadow is not None:
            assert _same(shadow.view, p_ref.t().contiguous()), ("shadow",) + what
            assert torch.equal(_bits(shadow.view), _bits(tn.cpp._transpose_field(p.view))), ("shadow vs tn_transpose_f32",) + what
            assert shadow.intact(), ("a word outside the shadow changed",) + what
    assert branches == {False, True}


@pytest.mark.parametrize("V", FIELD_V)
def test_field_kernel_bit_equal_to_the_statement(tn, device, optim, V):
    """8 steps (steps 1-5 plain, 6-8 adaptive) at every tile edge, with and without the shadow, weight decay off / coupled /
    decoupled.  V % 4 == 0 takes the 16-byte form, every other V the 4-byte form.  launch_radam_field does not cap its grid
    (optim.FIELD_GRID_CAP is None), so there is no capped size to add."""
    assert optim.FIELD_GRID_CAP is None
    for decay in rc.DECAYS:
        for with_shadow in (True, False):
            _field_case(tn, optim, device, V, decay, with_shadow)


@pytest.mark.parametrize("V", [64, 4100])
def test_field_kernel_with_bases_off_the_16_byte_grid(tn, device, optim, V):
    """V % 4 == 0, but p / exp_avg / exp_avg_sq / the shadow start 4 bytes into a 16-byte line: the 4-byte form must take over."""
    _field_case(tn, optim, device, V, rc.DECAYS[1], True, offset=PAD + 1, steps=6)


# ---- 2: the flat kernel ----------------------------------------------------------------------------------------------------------

def _flat_case(tn, optim, device, sizes, offsets, steps, decay, rounds=2, lr=rc.LR, betas=rc.BETAS):
    """One tn_radam_step over len(sizes) tensors, tensor i at step count steps[i] (+ round); `rounds` calls."""
    lib = tn.cpp._lib.load()
    ref = [(rc.parameter((n,), 100 + i),) + rc.moments((n,), 100 + i) for i, n in enumerate(sizes)]
    dev = [tuple(_Embedded(x, device, off) for x in r) for r, off in zip(ref, offsets)]
    hyper = _hyper(optim, decay, lr, betas)
    branches = set()
    for rnd in range(rounds):
        table = (optim._Tensor * len(sizes))()
        grads = []
        for i, n in enumerate(sizes):
            g_cpu = rc.gradient((n,), 100 + i, rnd + 1)
            g = _Embedded(g_cpu, device, offsets[i])
            grads.append((g_cpu, g))
            a, adaptive = optim.radam_scalars(steps[i] + rnd, lr, betas)
            branches.add(adaptive)
            slot = table[i]
            slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq = (dev[i][0].view.data_ptr(), g.view.data_ptr(),
                                                                    dev[i][1].view.data_ptr(), dev[i][2].view.data_ptr())
            slot.count, slot.step_size, slot.adaptive = n, a, int(adaptive)
        tn.cpp._lib.check(lib.tn_radam_step(len(sizes), ctypes.addressof(table), ctypes.addressof(hyper), tn.cpp._stream(device)))
        for i, n in enumerate(sizes):
            ref[i] = optim.radam_statement(ref[i][0], grads[i][0], ref[i][1], ref[i][2], steps[i] + rnd, lr, betas, rc.EPS, decay[1], decay[2])
            what = (i, n, offsets[i], steps[i] + rnd, decay[0])
            for name, got, want in zip(("p", "exp_avg", "exp_avg_sq"), dev[i], ref[i]):
                assert _same(got.view, want), (name,) + what
                assert got.intact(), ("a word outside " + name + " changed",) + what
            assert _same(grads[i][1].view, grads[i][0]) and grads[i][1].intact(), ("the gradient was written",) + what
    return branches


@pytest.mark.parametrize("decay", rc.DECAYS, ids=[d[0] for d in rc.DECAYS])
def test_flat_kernel_bit_equal_to_the_statement(tn, device, optim, decay):
    """All sizes in ONE launch, each tensor at a step count of its own (both branches in one table), 16-byte aligned starts."""
    steps = [1 + (3 * i) % 9 for i in range(len(FLAT_N))]
    branches = _flat_case(tn, optim, device, FLAT_N, [PAD] * len(FLAT_N), steps, decay)
    assert branches == {False, True}


def test_flat_kernel_with_starts_off_the_16_byte_grid(tn, device, optim):
    """Every tensor starts 4, 8 or 12 bytes into a 16-byte line (p, g, exp_avg, exp_avg_sq alike), beside aligned ones."""
    offsets = [PAD + (i % 4) for i in range(len(FLAT_N))]
    steps = [6 - (i % 2) for i in range(len(FLAT_N))]
    _flat_case(tn, optim, device, FLAT_N, offsets, steps, rc.DECAYS[1])


def test_flat_kernel_one_more_tensor_than_the_table_holds(tn, device, optim):
    count = optim.TABLE_SIZE + 1
    sizes = [(5, 257, 4097, 1, 4096)[i % 5] for i in range(count)]
    _flat_case(tn, optim, device, sizes, [PAD] * count, [1 + i % 8 for i in range(count)], rc.DECAYS[2], rounds=1)


# ---- 3: FusedRAdam ---------------------------------------------------------------------------------------------------------------

def _snapshot(opt, params):
    """CPU copies of (p, g, exp_avg, exp_avg_sq, step) of every parameter, before a step"""
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append((p.detach().cpu().clone(), None if p.grad is None else p.grad.cpu().clone(),
                    st["exp_avg"].cpu().clone() if st else torch.zeros(p.shape), st["exp_avg_sq"].cpu().clone() if st else torch.zeros(p.shape),
                    int(st["step"]) if st else 0))
    return out


def _check_step(optim, opt, params, before, hypers, tag=""):
    """every parameter of `params` against one statement step from its snapshot; hypers[i] = (lr, betas, eps, wd, decoupled)"""
    for i, (p, (p0, g0, m0, v0, t0)) in enumerate(zip(params, before)):
        st = opt.state.get(p, {})
        if g0 is None:
            assert _same(p, p0), (tag, i, "a parameter without a gradient was written")
            assert (int(st["step"]) if st else 0) == t0, (tag, i, "the step of a parameter without a gradient advanced")
            if st:
                assert _same(st["exp_avg"], m0) and _same(st["exp_avg_sq"], v0)
            continue
        lr, betas, eps, wd, decoupled = hypers[i]
        want = optim.radam_statement(p0, g0, m0, v0, t0 + 1, lr, betas, eps, wd, decoupled)
        assert int(st["step"]) == t0 + 1 and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"
        for name, got, w in zip(("p", "exp_avg", "exp_avg_sq"), (p, st["exp_avg"], st["exp_avg_sq"]), want):
            assert _same(got, w), (tag, i, name, t0 + 1)


def test_optimizer_groups_missing_gradients_and_step_counts(tn, device, optim):
    """Two groups with different lr and betas; a parameter whose gradient is None in some iterations, between others: it is
    untouched and its step does not advance, so the parameters of one group sit at different step counts (and, around step 6,
    on different branches) in one launch."""
    shapes = [(128, 64), (128,), (3, 128), (257,), (5,)]
    params = [rc.parameter(s, 40 + i).to(device).requires_grad_(True) for i, s in enumerate(shapes)]
    groups = [{"params": params[:3]}, {"params": params[3:], "lr": 3e-3, "betas": (0.5, 0.9), "weight_decay": 1e-2}]
    opt = optim.FusedRAdam(groups, lr=rc.LR, eps=rc.EPS)
    hypers = [(rc.LR, rc.BETAS, rc.EPS, 0, False)] * 3 + [(3e-3, (0.5, 0.9), rc.EPS, 1e-2, False)] * 2
    for it in range(1, 10):
        versions = [p._version for p in params]
        for i, p in enumerate(params):
            skip = (i == 1 and it % 2 == 0) or (i == 4 and it in (3, 4))
            p.grad = None if skip else rc.gradient(p.shape, 40 + i, it).to(device)
        before = _snapshot(opt, params)
        opt.step()
        _check_step(optim, opt, params, before, hypers, tag=it)
        for p, ver, (_, g0, _, _, _) in zip(params, versions, before):
            assert (p._version > ver) == (g0 is not None)
    assert [int(opt.state[p]["step"]) for p in params] == [9, 5, 9, 9, 7]


def test_optimizer_refuses_what_it_cannot_step(tn, device, optim):
    p = torch.zeros(8, 4, device=device, requires_grad=True)
    opt = optim.FusedRAdam([p])
    p.grad = torch.zeros(8, 4, device=device).to_sparse()
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        opt.step()
    p.grad = torch.zeros(4, 8, device=device).t()
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        opt.step()
    opt.param_groups[0]["maximize"] = True
    p.grad = torch.zeros(8, 4, device=device)
    with pytest.raises(ValueError, match="maximize=True is not supported"):
        opt.step()
    assert not opt.state[p] or int(opt.state[p]["step"]) == 0
    assert float(p.detach().abs().max()) == 0


def test_step_neither_synchronises_nor_allocates(tn, device, optim):
    """After a parameter's first step (which makes its state and, for a registered field, its shadow): no host synchronisation
    (torch.cuda.set_sync_debug_mode("error")) and no device allocation in step() or in the field_vertex_major that follows."""
    cpp = tn.cpp
    field = rc.parameter((64, 130), 5).to(device).requires_grad_(True)
    others = [rc.parameter(s, 80 + i).to(device).requires_grad_(True) for i, s in enumerate([(128, 64), (128,), (3, 128)])]
    cpp.register_field(field)
    try:
        opt = optim.FusedRAdam([field] + others, weight_decay=1e-2)
        for p in [field] + others:
            p.grad = rc.gradient(p.shape, 5, 1).to(device)
        opt.step()
        cpp.field_vertex_major(field)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(device)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(6):
                opt.step()
                cpp.field_vertex_major(field)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(device) == before
        assert int(opt.state[field]["step"]) == 7
    finally:
        cpp.unregister_field(field)


@pytest.mark.parametrize("check_caches", [False, True], ids=["plain", "TETRANERF_HIP_CHECK_CACHES"])
@pytest.mark.parametrize("V", [129, 4100])
def test_cache_hand_over(tn, device, optim, monkeypatch, V, check_caches):
    """After step() on a registered field, field_vertex_major(field) launches no transposition and returns the shadow the step
    wrote -- also under TETRANERF_HIP_CHECK_CACHES=1, which compares it with the field.  An unregistered [64, V] tensor takes the
    flat kernel and gets no shadow."""
    cpp = tn.cpp
    monkeypatch.setattr(cpp, "_CHECK_CACHES", check_caches)
    field = rc.parameter((64, V), 3).to(device).requires_grad_(True)
    plain = field.detach().clone().requires_grad_(True)
    cpp.register_field(field)
    try:
        real, calls = cpp._transpose_field, []
        first = cpp.field_vertex_major(field)                      # the ordinary route: one transposition
        opt = optim.FusedRAdam([field, plain], weight_decay=1e-2)
        monkeypatch.setattr(cpp, "_transpose_field", lambda f: (calls.append(f.shape), real(f))[1])
        for step in range(1, 8):
            g = rc.gradient((64, V), 3, step).to(device)
            field.grad, plain.grad = g, g.clone()
            version = field._version
            opt.step()
            assert field._version > version
            shadow = cpp.field_vertex_major(field)
            assert calls == [], "field_vertex_major transposed after the fused step"
            assert shadow.data_ptr() == opt._shadows[id(field)][1].data_ptr() and shadow.data_ptr() != first.data_ptr()
            assert torch.equal(_bits(shadow), _bits(field.detach().t().contiguous()))
            assert torch.equal(_bits(shadow), _bits(real(field)))
            assert torch.equal(_bits(field), _bits(plain)), "the field kernel and the flat kernel disagree"
        assert id(plain) not in opt._shadows
        cpp.field_vertex_major(plain)
        assert len(calls) == 1                                     # the unregistered tensor still transposes per call
        # an in-place write by someone else is still seen: the cache re-transposes
        with torch.no_grad():
            field.mul_(2.0)
        again = cpp.field_vertex_major(field)
        assert len(calls) == 2 and torch.equal(_bits(again), _bits(field.detach().t().contiguous()))
    finally:
        cpp.unregister_field(field)


def _renderer(tn, scenes, render, device, pts, cells, S, S_fine, biased, M, seed):
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    torch.manual_seed(seed)
    mlp = render.TetraMLP().to(device)
    field = ((torch.rand(64, len(pts), device=device) * 2 - 1) * 0.5).requires_grad_(True)
    rd = render.TetraRenderer(tr, field, mlp, S, M, fused=True, num_fine_samples=S_fine, biased=biased)
    return tr, mlp, field, rd


def test_nothing_goes_stale(tn, device, optim, scenes, render):
    """Two render_train iterations with FusedRAdam on the smallest scene, then render() is bit-equal to the render() of a fresh
    renderer built on clones of the stepped parameters: neither the cached field shadow nor the packed MLP weights -- both cached
    per tensor version, both written through raw pointers here -- is stale.  The version of every stepped tensor has moved."""
    pts, cells = scenes.cube_mesh()
    tr, mlp, field, rd = _renderer(tn, scenes, render, device, pts, cells, 32, 32, False, 16, 5)
    o, d = scenes.outside_in_rays(64, 3)
    o, d = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    target = torch.rand(64, 3, device=device)
    params = [field] + list(mlp.parameters())
    opt = optim.FusedRAdam(params, lr=1e-2)
    try:
        rd.render(o, d)                                            # caches filled before the first step
        for _ in range(2):
            versions = [p._version for p in params]
            state_versions = [(opt.state[p]["exp_avg"]._version, opt.state[p]["exp_avg_sq"]._version) for p in params if opt.state.get(p)]
            opt.zero_grad(set_to_none=True)
            out = rd.render_train(o, d)
            ((out["rgb"] - target) ** 2).mean().backward()
            assert all(p.grad is not None for p in params)
            opt.step()
            assert all(p._version > ver for p, ver in zip(params, versions))
            if state_versions:
                assert all(opt.state[p]["exp_avg"]._version > a and opt.state[p]["exp_avg_sq"]._version > b
                           for p, (a, b) in zip(params, state_versions))
        got = rd.render(o, d)
        mlp2 = render.TetraMLP().to(device)
        mlp2.load_state_dict({k: v.detach().clone() for k, v in mlp.state_dict().items()})
        fresh = render.TetraRenderer(tr, field.detach().clone(), mlp2, 32, 16, fused=True, num_fine_samples=32, cache_field=False)
        want = fresh.render(o, d)
        assert int(got["ray_mask"].sum()) > 32
        for k in ("rgb", "accumulation", "depth"):
            assert torch.equal(_bits(got[k]), _bits(want[k])), (k, float((got[k] - want[k]).abs().max()))
    finally:
        tn.cpp.unregister_field(field)


@pytest.mark.parametrize("config", [(24, 24, False, False), (16, 16, True, True)], ids=["tetra-nerf-original", "tetra-nerf"])
def test_in_the_training_loop(tn, device, optim, scenes, render, config):
    """8 real render_train iterations (64 rays, small S, the sampler settings of both shipped configurations): every step on its
    own is bit-equal to the CPU statement on the (p, g, exp_avg, exp_avg_sq) it started from.  (The atomic gather adjoint makes
    trajectories irreproducible; single steps are not.)"""
    S, S_fine, biased, scaling = config
    pts, cells = scenes.random_mesh(500, 3)
    tr, mlp, field, rd = _renderer(tn, scenes, render, device, pts, cells, S, S_fine, biased, 256, 7)
    o, d = scenes.outside_in_rays(64, 4)
    o, d = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    target = torch.rand(64, 3, device=device)
    params = [field] + list(mlp.parameters())
    opt = optim.FusedRAdam(params, lr=1e-2, weight_decay=1e-3)
    hypers = [(1e-2, rc.BETAS, 1e-8, 1e-3, False)] * len(params)
    try:
        for it in range(1, 9):
            opt.zero_grad(set_to_none=True)
            out = rd.render_train(o, d, gradient_scaling=scaling)
            ((out["rgb"] - target) ** 2).mean().backward()
            before = _snapshot(opt, params)
            assert all(b[1] is not None and bool(torch.isfinite(b[1]).all()) for b in before)
            assert float(before[0][1].abs().max()) > 0
            opt.step()
            _check_step(optim, opt, params, before, hypers, tag=it)
            assert torch.equal(_bits(tn.cpp.field_vertex_major(field)), _bits(field.detach().t().contiguous()))
    finally:
        tn.cpp.unregister_field(field)


# ---- 4: state interchange with torch.optim.RAdam -----------------------------------------------------------------------------------

def test_state_dict_from_torch_continues_bit_equal(tn, device, optim):
    """3 steps of torch.optim.RAdam on the device -> state_dict -> FusedRAdam.load_state_dict -> 5 more steps, each bit-equal to the
    statement continued from that state.  Keys and dtypes of the two state_dicts are the same."""
    shapes = [(64, 130), (128, 155), (7,)]
    params = [rc.parameter(s, 60 + i).to(device).requires_grad_(True) for i, s in enumerate(shapes)]
    theirs = torch.optim.RAdam(params, lr=rc.LR, weight_decay=1e-2)
    for it in range(1, 4):
        for i, p in enumerate(params):
            p.grad = rc.gradient(p.shape, 60 + i, it).to(device)
        theirs.step()
    sd = theirs.state_dict()
    ours = optim.FusedRAdam(params, lr=5e-4)
    ours.load_state_dict(sd)
    assert ours.param_groups[0]["lr"] == rc.LR and ours.param_groups[0]["weight_decay"] == 1e-2
    hypers = [(rc.LR, rc.BETAS, rc.EPS, 1e-2, False)] * len(params)
    for it in range(4, 9):
        for i, p in enumerate(params):
            p.grad = rc.gradient(p.shape, 60 + i, it).to(device)
        before = _snapshot(ours, params)
        assert all(b[4] == it - 1 for b in before)
        ours.step()
        _check_step(optim, ours, params, before, hypers, tag=it)
    mine, torchs = ours.state_dict(), theirs.state_dict()
    assert mine.keys() == torchs.keys()
    assert [sorted(g) for g in mine["param_groups"]] == [sorted(g) for g in torchs["param_groups"]]
    assert mine["state"].keys() == torchs["state"].keys()
    for k in mine["state"]:
        a, b = mine["state"][k], torchs["state"][k]
        assert a.keys() == b.keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a:
            assert a[name].dtype == b[name].dtype and a[name].device == b[name].device and a[name].shape == b[name].shape, (k, name)


def test_state_dict_to_torch_continues_within_4y_of_float64(tn, device, optim):
    """The other direction: 3 steps of FusedRAdam -> state_dict -> torch.optim.RAdam.load_state_dict -> 5 more steps of torch.
    Per step of the continuation the error against torch's float64 RAdam over all 8 steps stays within 4 y, y = the same figure of
    torch's fp32 RAdam over all 8 steps (tests/test_radam.py's rule)."""
    shape, seed, decay = (64, 130), 70, rc.DECAYS[1]
    p0 = rc.parameter(shape, seed)
    grads = [rc.gradient(shape, seed, it) for it in range(1, 9)]
    ref = rc.torch_trajectory(p0, grads, torch.float64, decay)
    y = rc.torch_trajectory(p0, grads, torch.float32, decay)
    p = p0.to(device).requires_grad_(True)
    ours = optim.FusedRAdam([p], lr=rc.LR, weight_decay=decay[1])
    for it in range(1, 4):
        p.grad = grads[it - 1].to(device)
        ours.step()
    theirs = torch.optim.RAdam([p], lr=1.0)
    theirs.load_state_dict(ours.state_dict())
    assert theirs.param_groups[0]["lr"] == rc.LR and int(theirs.state[p]["step"]) == 3
    failures = []
    for it in range(4, 9):
        p.grad = grads[it - 1].to(device)
        theirs.step()
        st = theirs.state[p]
        for name, got, r, yy in zip(("p", "exp_avg", "exp_avg_sq"), (p, st["exp_avg"], st["exp_avg_sq"]), ref[it - 1], y[it - 1]):
            e, f = rc.error(got.detach().cpu(), r), rc.error(yy, r)
            print(f"RATIO radam interchange step={it} {name}: fused-then-torch {e:.3e} torch-fp32 {f:.3e}", flush=True)
            if not e <= 4 * f:
                failures.append((it, name, e, f))
    assert not failures, failures
