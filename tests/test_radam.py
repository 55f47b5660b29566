"""The RAdam step without a GPU: the host scalars and the element-wise statement of tetra-nerf_amd/optim.py against
torch.optim.RAdam, the C-ABI additions, the nerfstudio adapter switch and what FusedRAdam refuses.  tests/test_radam_gpu.py holds
the kernels to the statement bit for bit.

Statement vs torch: three trajectories of 12 steps on the gradients of tests/radam_cases.py -- torch.optim.RAdam (foreach=False)
in float64 (the reference), the same in fp32 (the yardstick) and the statement.  Per tensor and step the error is
max |d| / max |reference|; the statement's must stay within 4 y, y = the same figure of torch's own fp32 RAdam.  `RATIO` lines
(pytest -s) are what profiles/radam_errors.txt records."""
import ctypes
import importlib
import inspect
import math
import re
import sys
from pathlib import Path

import pytest
import torch

import radam_cases as rc

ROOT = Path(__file__).resolve().parents[1]
NEW = ("tn_radam_step_field", "tn_radam_step")


@pytest.fixture(scope="module")
def optim():
    return rc.optim()


def _torch_scalars(step, lr, beta1, beta2):
    """torch/optim/radam.py, _single_tensor_radam, written out: (factor of exp_avg, adaptive)"""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    rho_inf = 2 / (1 - beta2) - 1
    rho_t = rho_inf - 2 * step * (beta2 ** step) / bias_correction2
    if rho_t > 5.0:
        rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5
        return lr * rect * (bias_correction2 ** 0.5) / bias_correction1, True, rho_t
    return lr / bias_correction1, False, rho_t


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9), (0.9, 0.99)])
def test_radam_scalars_match_torch_formulas(optim, betas):
    flips = []
    for step in list(range(1, 21)) + [1000, 300000]:
        want_a, want_adaptive, rho_t = _torch_scalars(step, 1e-3, *betas)
        a, adaptive = optim.radam_scalars(step, 1e-3, betas)
        assert adaptive is want_adaptive and adaptive == (rho_t > 5.0), (step, betas, rho_t)
        assert math.isclose(a, want_a, rel_tol=1e-14, abs_tol=0), (step, betas, a, want_a)
        flips.append(adaptive)
    assert not flips[0] and flips[-1] and flips == sorted(flips), flips      # one flip, from the plain to the adaptive branch
    if betas == (0.9, 0.999):
        assert flips[:5] == [False] * 5 and flips[5]                          # step 6 is the first adaptive one
    with pytest.raises(ValueError):
        optim.radam_scalars(0, 1e-3, betas)


@pytest.mark.parametrize("decay", rc.DECAYS, ids=[d[0] for d in rc.DECAYS])
def test_statement_vs_torch_float64(optim, decay):
    p0 = rc.parameter((rc.N,), 1)
    grads = [rc.gradient((rc.N,), 1, t) for t in range(1, rc.STEPS + 1)]
    assert all(float(g.abs().max()) <= 1 and float(g[g != 0].abs().min()) >= 1e-6 and bool((g == 0).any()) for g in grads)
    ref = rc.torch_trajectory(p0, grads, torch.float64, decay)
    t32 = rc.torch_trajectory(p0, grads, torch.float32, decay)
    got = rc.statement_trajectory(p0, grads, decay)
    failures, worst = [], {}
    for step, (r, y, s) in enumerate(zip(ref, t32, got), 1):
        for name, rr, yy, ss in zip(("p", "exp_avg", "exp_avg_sq"), r, y, s):
            assert ss.dtype == torch.float32
            e, f = rc.error(ss, rr), rc.error(yy, rr)
            ratio = e / f if f > 0 else (0.0 if e == 0 else math.inf)
            worst[name] = max(worst.get(name, 0.0), ratio)
            print(f"RATIO radam statement decay={decay[0]} step={step} {name}: statement {e:.3e} torch-fp32 {f:.3e} ratio {ratio:.2f}", flush=True)
            if not e <= 4 * f:
                failures.append((step, name, e, f))
    print(f"RATIO radam statement decay={decay[0]} worst ratios: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()), flush=True)
    assert not failures, failures


def test_statement_branches_and_purity(optim):
    """Steps 1-5 move p by a * m alone (no division), later ones by the adaptive form; the inputs are not written."""
    p, g = rc.parameter((257,), 2), rc.gradient((257,), 2, 1)
    m, v = rc.moments((257,), 2)
    keep = [x.clone() for x in (p, g, m, v)]
    for step, adaptive in ((5, False), (6, True)):
        a, is_adaptive = optim.radam_scalars(step, rc.LR, rc.BETAS)
        assert is_adaptive is adaptive
        p1, m1, v1 = optim.radam_statement(p, g, m, v, step, rc.LR, rc.BETAS, rc.EPS)
        a32 = torch.tensor(a, dtype=torch.float32)
        want = p - (a32 * m1) / (optim._sqrt_rn(v1) + torch.tensor(rc.EPS, dtype=torch.float32)) if adaptive else p - a32 * m1
        assert torch.equal(p1, want)
    assert all(torch.equal(x, k) for x, k in zip((p, g, m, v), keep))
    with pytest.raises(ValueError):
        optim.radam_statement(p.double(), g, m, v, 1, rc.LR, rc.BETAS)


def test_statement_square_root_is_correctly_rounded(optim):
    """The statement's square root against float64 (sqrt in float64, rounded to fp32, is the correctly rounded fp32 root): bit-equal
    on 2^18 values over 24 decades.  torch.sqrt on the CPU is off by an ulp on a fraction of a percent of them, which is why the
    statement does not use it; the fraction is printed, not asserted (it depends on the processor)."""
    x = (10.0 ** (-24 * torch.rand(1 << 18, generator=torch.Generator().manual_seed(3), dtype=torch.float64))).float()
    want = x.double().sqrt().float()
    assert torch.equal(optim._sqrt_rn(x).view(torch.int32), want.view(torch.int32))
    assert optim._sqrt_rn(x.reshape(512, 512).t()).shape == (512, 512)
    off = int((torch.sqrt(x).view(torch.int32) != want.view(torch.int32)).sum())
    print(f"RATIO radam statement: torch.sqrt (CPU, fp32) differs from the correctly rounded root on {off} of {x.numel()} values", flush=True)


def test_abi_additions_keep_version_6():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/tetranerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the shared library"
        assert name in _lib.SYMBOLS
    comment = header[:header.index("typedef struct tn_radam_hyper")].rsplit("/*", 1)[1]
    assert "registration.py:37-45" in comment and "torch/optim/radam.py" in comment
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header)
    lib.tn_abi_version.restype = ctypes.c_int
    assert _lib.ABI_VERSION == 6 and lib.tn_abi_version() == 6
    loaded = _lib.load()
    assert len(loaded.tn_radam_step_field.argtypes) == 10 and len(loaded.tn_radam_step.argtypes) == 4
    assert (ROOT / "tetra-nerf_amd" / "csrc" / "tn_optim.hip").exists()
    assert "tn_optim.hip" in (ROOT / "tetra-nerf_amd" / "csrc" / "Makefile").read_text()


def test_entries_refuse_bad_arguments_on_the_host(optim):
    """Argument errors go through tn_last_error before anything is launched (no GPU needed)."""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    lib = _lib.load()
    hyper = optim._Hyper(0.1, 0.999, 0.001, 1e-8, 0.0, 0)
    with pytest.raises(RuntimeError, match="hyper is null"):
        _lib.check(lib.tn_radam_step(0, None, None, None))
    with pytest.raises(RuntimeError, match="decay_mode"):
        _lib.check(lib.tn_radam_step(0, None, ctypes.addressof(optim._Hyper(0.1, 0.999, 0.001, 1e-8, 0.0, 3)), None))
    with pytest.raises(RuntimeError, match="table is null"):
        _lib.check(lib.tn_radam_step(2, None, ctypes.addressof(hyper), None))
    table = (optim._Tensor * 2)()
    table[1].count = 5
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(lib.tn_radam_step(2, ctypes.addressof(table), ctypes.addressof(hyper), None))
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(lib.tn_radam_step_field(8, None, None, None, None, None, 1e-3, 0, ctypes.addressof(hyper), None))
    _lib.check(lib.tn_radam_step(0, None, ctypes.addressof(hyper), None))            # nothing to do is not an error
    _lib.check(lib.tn_radam_step_field(0, None, None, None, None, None, 1e-3, 0, ctypes.addressof(hyper), None))
    assert ctypes.sizeof(optim._Tensor) == 48 and ctypes.sizeof(optim._Hyper) == 24   # tn_radam_tensor / tn_radam_hyper on LP64


class _OptimizerConfig:
    def __init__(self, target):
        self._target = target
        self.lr, self.eps, self.weight_decay, self.max_norm = 1e-3, 1e-8, 0, None


class _TrainerConfig:
    def __init__(self, optimizers):
        self.optimizers = optimizers


def test_use_fused_radam_on_stand_in_configs(optim):
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    fields, cameras, other = _OptimizerConfig(torch.optim.RAdam), _OptimizerConfig(torch.optim.Adam), _OptimizerConfig(torch.optim.RAdam)
    cfg = _TrainerConfig({"fields": {"optimizer": fields, "scheduler": object()}, "camera_opt": {"optimizer": cameras, "scheduler": None},
                          "more": {"optimizer": other}, "empty": {}})
    assert fields._target is torch.optim.RAdam                                       # nothing is installed by default
    assert plugin.use_fused_radam(cfg) == ["fields", "more"]
    assert fields._target is optim.FusedRAdam and other._target is optim.FusedRAdam and cameras._target is torch.optim.Adam
    assert plugin.use_fused_radam(cfg) == []                                         # idempotent
    assert plugin.use_fused_radam(_TrainerConfig({})) == [] and plugin.use_fused_radam(object()) == []
    assert not any(m.split(".")[0] == "nerfstudio" for m in sys.modules)           # duck typing: no nerfstudio import


def test_constructor_takes_torchs_names_and_defaults(optim):
    ours = inspect.signature(optim.FusedRAdam.__init__).parameters
    theirs = inspect.signature(torch.optim.RAdam.__init__).parameters
    assert list(ours) == list(theirs)
    for name, par in theirs.items():
        assert ours[name].default == par.default and ours[name].kind == par.kind, name


def test_refusals(optim):
    cpu = torch.zeros(8, requires_grad=True)
    with pytest.raises(RuntimeError, match="must be on a GPU"):              # no CPU fallback
        optim.FusedRAdam([cpu])
    with pytest.raises(RuntimeError, match="dense fp32"):
        optim.FusedRAdam([torch.zeros(8, dtype=torch.float64, requires_grad=True)])
    with pytest.raises(RuntimeError, match="contiguous"):
        optim.FusedRAdam([torch.zeros(8, 8).t()[1:].requires_grad_(True)])
    for key in ("maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=f"{key}=True is not supported"):
            optim.FusedRAdam([cpu], **{key: True})
    with pytest.raises(ValueError, match="tensor lr is not supported"):
        optim.FusedRAdam([cpu], lr=torch.tensor(1e-3))
    # torch's own validation, in torch's words
    for kwargs, msg in (({"lr": -1.0}, "Invalid learning rate: -1.0"), ({"eps": -1.0}, "Invalid epsilon value: -1.0"),
                        ({"betas": (1.0, 0.9)}, "Invalid beta parameter at index 0: 1.0"),
                        ({"betas": (0.9, 1.0)}, "Invalid beta parameter at index 1: 1.0"),
                        ({"weight_decay": -1.0}, "Invalid weight_decay value: -1.0")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            optim.FusedRAdam([cpu], **kwargs)
        with pytest.raises(ValueError, match=re.escape(msg)):
            torch.optim.RAdam([cpu], **kwargs)
