"""What the nine training entries of the fused MLP answer to arguments they refuse, through the C-ABI: which counts return 0
without work, which check fires first when two apply, and every message word for word.  The entries share their host code per
stage (csrc/tn_api_mlp.hip: forward_train, backward, param_grads, ray_head_grad); their answers stay their own.  No call here
gets as far as a launch: every one returns early or is refused."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

R, S, N = 2, 4, 8
MODE_2 = ("mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA) here: mode 2 (plain bf16 MFMA) is an arithmetic of tn_mlp_forward and "
          "tn_mlp_forward_gather only")
MODE_2_TRAIN_INDEXED = ("mlp_forward_gather_train_indexed: mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA): the plain-bf16 kernel "
                        "(mode 2) has neither a training nor an indexed form")
MODE_7 = "mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA)"
NULL = "null pointer"
N_MULTIPLE = "n must be a multiple of samples_per_ray"
N_SAMPLES_POSITIVE = "n_samples must be a positive multiple of samples_per_ray"
N_SAMPLES_MULTIPLE = "n_samples must be a multiple of samples_per_ray"


class _Args:
    """the arguments of the entries over 2 rays x 4 samples, every buffer 8 columns wide; `buffers(without=...)` and
    `grads(without=...)` build the two structs with one null member"""

    def __init__(self, tn, device):
        cpp = self.cpp = tn.cpp
        self.lib = cpp._lib.load()
        g = torch.Generator().manual_seed(1)
        self.weights = [torch.randn(shp, generator=g).to(device) * 0.1 for shp in cpp._WEIGHT_SHAPES]
        self.h = cpp.fused_mlp(self.weights).handle
        self.vi = torch.zeros(N, 4, dtype=torch.int32, device=device)
        self.bc = torch.full((N, 3), 0.25, device=device)
        self.field_vm = torch.zeros(5, 64, device=device)
        self.dirs = torch.nn.functional.normalize(torch.ones(R, 3, device=device), dim=-1)
        self.sigma, self.rgb = torch.zeros(N, device=device), torch.zeros(N, 3, device=device)
        self.d_sigma, self.d_rgb = torch.zeros(N, device=device), torch.zeros(N, 3, device=device)
        self.live = torch.arange(N, dtype=torch.int32, device=device)
        self.d_ray = torch.zeros(R, 128, device=device)
        self.acts = torch.zeros(576, N, device=device)
        self.masks = torch.zeros(4, N, 2, dtype=torch.int64, device=device)
        self.chain = torch.zeros(516, N, device=device)
        self.dx0 = torch.zeros(N, 64, device=device)
        self.grad_tensors = [torch.zeros(shp, device=device) for shp in cpp._WEIGHT_SHAPES]
        torch.cuda.synchronize()
        self.unchanged = [t.clone() for t in self._outputs()]

    def _outputs(self):
        return [self.sigma, self.rgb, self.acts, self.masks, self.chain, self.dx0, self.d_ray] + self.grad_tensors

    def nothing_was_written(self):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(self._outputs(), self.unchanged))

    def buffers(self, without=None):
        a, c = self.acts, self.chain
        ptr = dict(x0=a[0:64], h1=a[64:192], h2=a[192:320], h3=a[320:448], h4=a[448:576], masks=self.masks, d1=c[0:128], d2=c[128:256],
                   d3=c[256:384], d4=c[384:512], dhead=c[512:516], dx0=self.dx0)
        self._bs = self.cpp._MlpBackwardBuffers(*[None if k == without else t.data_ptr() for k, t in ptr.items()])
        return C.byref(self._bs)

    def grads(self, without=None):
        names = [k for k, _ in self.cpp._MlpWeightsStruct._fields_]
        self._gs = self.cpp._MlpWeightsStruct(*[None if k == without else t.data_ptr() for k, t in zip(names, self.grad_tensors)])
        return C.byref(self._gs)

    def refused(self, rc, text):
        got = self.lib.tn_last_error().decode()
        assert rc != 0 and got == text, (rc, got)

    def accepted(self, rc):
        assert rc == 0 and self.lib.tn_last_error() == b""


@pytest.fixture(scope="module")
def args(tn, device):
    return _Args(tn, device)


def _p(t):
    return None if t is None else t.data_ptr()


def _forward_train(a, entry, n=N, samples_per_ray=S, mode=0, vi="vi", without=None, b=True, n_live=N, live="live", dirs="dirs"):
    lib, get = a.lib, lambda k: _p(getattr(a, k)) if k else None
    head = (get(vi), _p(a.bc), _p(a.field_vm), get(dirs))
    tail = (_p(a.sigma), _p(a.rgb), a.buffers(without) if b else None, None, None)
    if entry == "tn_mlp_forward_gather_train":
        return lib.tn_mlp_forward_gather_train(a.h, n, samples_per_ray, *head, *tail)
    if entry == "tn_mlp_forward_gather_train_ex":
        return lib.tn_mlp_forward_gather_train_ex(a.h, n, samples_per_ray, *head, mode, *tail)
    return lib.tn_mlp_forward_gather_train_indexed(a.h, n_live, n, samples_per_ray, get(live), *head, mode, *tail)


@pytest.mark.parametrize("entry", ["tn_mlp_forward_gather_train", "tn_mlp_forward_gather_train_ex"])
def test_dense_training_forward(args, entry):
    a, has_mode = args, entry.endswith("_ex")
    a.accepted(_forward_train(a, entry, n=0))
    a.accepted(_forward_train(a, entry, n=0, samples_per_ray=0, vi=None, b=False))       # (an empty call is not looked at)
    a.refused(_forward_train(a, entry, samples_per_ray=0), N_MULTIPLE)
    a.refused(_forward_train(a, entry, n=7), N_MULTIPLE)
    a.refused(_forward_train(a, entry, vi=None), NULL)
    a.refused(_forward_train(a, entry, dirs=None), NULL)                                 # (no density-only form)
    a.refused(_forward_train(a, entry, b=False), NULL)
    a.refused(_forward_train(a, entry, without="masks"), NULL)
    a.refused(_forward_train(a, entry, without="h3"), NULL)
    a.accepted(_forward_train(a, entry, n=0, without="dx0"))
    a.refused(_forward_train(a, entry, samples_per_ray=0, vi=None), NULL)                # pointers before sizes
    a.refused(_forward_train(a, entry, n=7, without="x0"), NULL)
    a.refused(a.lib.tn_mlp_forward_gather_train(None, 0, S, *[None] * 9) if not has_mode else
              a.lib.tn_mlp_forward_gather_train_ex(None, 0, S, *[None] * 4, 7, *[None] * 5), "mlp handle is null")
    if has_mode:
        a.refused(_forward_train(a, entry, mode=2), MODE_2)
        a.refused(_forward_train(a, entry, mode=7), MODE_7)
        a.refused(_forward_train(a, entry, mode=-1), MODE_7)
        a.refused(_forward_train(a, entry, mode=7, n=0), MODE_7)                         # the mode before the empty call
        a.refused(_forward_train(a, entry, mode=2, n=7, vi=None), MODE_2)                # ... and before everything else
    assert a.nothing_was_written()


def test_indexed_training_forward(args):
    a, entry = args, "tn_mlp_forward_gather_train_indexed"
    a.accepted(_forward_train(a, entry, n_live=0))
    a.accepted(_forward_train(a, entry, n_live=0, n=0, samples_per_ray=0, live=None, b=False))
    a.refused(_forward_train(a, entry, mode=2), MODE_2_TRAIN_INDEXED)
    a.refused(_forward_train(a, entry, mode=7), MODE_7)
    a.refused(_forward_train(a, entry, mode=2, n_live=0), MODE_2_TRAIN_INDEXED)          # the mode before the empty list
    a.refused(_forward_train(a, entry, mode=7, n_live=0), MODE_7)
    a.refused(_forward_train(a, entry, samples_per_ray=0), N_SAMPLES_POSITIVE)
    a.refused(_forward_train(a, entry, n=7, n_live=5), N_SAMPLES_POSITIVE)
    a.refused(_forward_train(a, entry, n=0, n_live=5), N_SAMPLES_POSITIVE)               # a list into no samples
    a.refused(_forward_train(a, entry, live=None), NULL)
    a.refused(_forward_train(a, entry, vi=None), NULL)
    a.refused(_forward_train(a, entry, without="masks"), NULL)
    a.refused(_forward_train(a, entry, samples_per_ray=0, live=None), NULL)              # pointers before sizes
    a.refused(_forward_train(a, entry, n=7, without="h1"), NULL)
    a.refused(_forward_train(a, entry, n=2 ** 32, samples_per_ray=1), "too many samples for one call")
    assert a.nothing_was_written()


def _backward(a, entry, n=N, mode=0, sigma="sigma", without=None, b=True):
    head = (a.h, n, _p(getattr(a, sigma)) if sigma else None, _p(a.rgb), _p(a.d_sigma), _p(a.d_rgb), a.buffers(without) if b else None)
    if entry == "tn_mlp_backward":
        return a.lib.tn_mlp_backward(*head, None)
    return a.lib.tn_mlp_backward_ex(*head, mode, None)


@pytest.mark.parametrize("entry", ["tn_mlp_backward", "tn_mlp_backward_ex"])
def test_backward(args, entry):
    a = args
    a.accepted(_backward(a, entry, n=0))
    a.accepted(_backward(a, entry, n=0, sigma=None, b=False))
    a.refused(_backward(a, entry, sigma=None), NULL)
    a.refused(_backward(a, entry, b=False), NULL)
    for member in ("masks", "d1", "d4", "dhead", "dx0"):
        a.refused(_backward(a, entry, without=member), NULL)
    if entry.endswith("_ex"):
        a.accepted(_backward(a, entry, n=0, mode=1))
        a.refused(_backward(a, entry, mode=2), MODE_2)
        a.refused(_backward(a, entry, mode=7), MODE_7)
        a.refused(_backward(a, entry, mode=7, n=0), MODE_7)                              # the mode before the empty call
        a.refused(_backward(a, entry, mode=2, sigma=None), MODE_2)
    assert a.nothing_was_written()


def _param_grads(a, entry, n=N, samples_per_ray=S, mode=0, dirs="dirs", without=None, b=True, no_grad=None, grads=True, n_live=N,
                 live="live"):
    d = _p(getattr(a, dirs)) if dirs else None
    bs, gs = a.buffers(without) if b else None, a.grads(no_grad) if grads else None
    if entry == "tn_mlp_param_grads":
        return a.lib.tn_mlp_param_grads(a.h, n, samples_per_ray, d, bs, gs, None)
    if entry == "tn_mlp_param_grads_ex":
        return a.lib.tn_mlp_param_grads_ex(a.h, n, samples_per_ray, d, bs, gs, mode, None)
    return a.lib.tn_mlp_param_grads_indexed(a.h, n_live, n, samples_per_ray, _p(getattr(a, live)) if live else None, d, bs, gs, mode, None)


@pytest.mark.parametrize("entry", ["tn_mlp_param_grads", "tn_mlp_param_grads_ex"])
def test_dense_param_grads(args, entry):
    a = args
    a.accepted(_param_grads(a, entry, n=0))
    a.accepted(_param_grads(a, entry, n=0, samples_per_ray=0, dirs=None, b=False, grads=False))
    a.refused(_param_grads(a, entry, samples_per_ray=0), N_MULTIPLE)
    a.refused(_param_grads(a, entry, n=7), N_MULTIPLE)
    a.refused(_param_grads(a, entry, dirs=None), NULL)
    a.refused(_param_grads(a, entry, b=False), NULL)
    a.refused(_param_grads(a, entry, grads=False), NULL)
    a.refused(_param_grads(a, entry, no_grad="w1"), NULL)
    a.refused(_param_grads(a, entry, no_grad="br"), NULL)
    for member in ("x0", "h4", "d1", "dhead"):
        a.refused(_param_grads(a, entry, without=member), NULL)
    a.refused(_param_grads(a, entry, samples_per_ray=0, dirs=None), NULL)                # the three arguments before the size ...
    a.refused(_param_grads(a, entry, samples_per_ray=0, no_grad="wd"), N_MULTIPLE)       # ... the members of the structs after it
    a.refused(_param_grads(a, entry, n=7, without="h2"), N_MULTIPLE)
    if entry.endswith("_ex"):
        a.accepted(_param_grads(a, entry, n=0, mode=1))
        a.refused(_param_grads(a, entry, mode=2), MODE_2)
        a.refused(_param_grads(a, entry, mode=7), MODE_7)
        a.refused(_param_grads(a, entry, mode=7, n=0), MODE_7)                           # the mode before the empty call
        a.refused(_param_grads(a, entry, mode=2, samples_per_ray=0, dirs=None), MODE_2)
    assert a.nothing_was_written()


def test_indexed_param_grads(args):
    a, entry = args, "tn_mlp_param_grads_indexed"
    a.accepted(_param_grads(a, entry, n_live=0))
    a.accepted(_param_grads(a, entry, n_live=0, n=0, samples_per_ray=0, live=None, b=False, grads=False))
    a.refused(_param_grads(a, entry, mode=2), MODE_2)                                    # (this entry has no wording of its own)
    a.refused(_param_grads(a, entry, mode=7), MODE_7)
    a.refused(_param_grads(a, entry, mode=2, n_live=0), MODE_2)                          # the mode before the empty list
    a.refused(_param_grads(a, entry, samples_per_ray=0), N_SAMPLES_POSITIVE)
    a.refused(_param_grads(a, entry, n=7, n_live=5), N_SAMPLES_POSITIVE)
    a.refused(_param_grads(a, entry, n=0, n_live=5), N_SAMPLES_POSITIVE)
    a.refused(_param_grads(a, entry, live=None), NULL)
    a.refused(_param_grads(a, entry, dirs=None), NULL)
    a.refused(_param_grads(a, entry, no_grad="bh"), NULL)
    a.refused(_param_grads(a, entry, without="d3"), NULL)
    a.refused(_param_grads(a, entry, samples_per_ray=0, live=None), NULL)                # the four arguments before the size ...
    a.refused(_param_grads(a, entry, samples_per_ray=0, no_grad="w2"), N_SAMPLES_POSITIVE)   # ... the structs' members after it
    a.refused(_param_grads(a, entry, n=2 ** 32, samples_per_ray=1), "too many samples for one call")
    assert a.nothing_was_written()


def test_indexed_ray_head_grad(args):
    a, lib = args, args.lib

    def call(n_live=N, n=N, samples_per_ray=S, live="live", b=True, without=None, d_ray="d_ray"):
        return lib.tn_mlp_ray_head_grad_indexed(n_live, n, samples_per_ray, _p(getattr(a, live)) if live else None,
                                                a.buffers(without) if b else None, _p(getattr(a, d_ray)) if d_ray else None, None)

    a.accepted(call(n=0))                  # no rays: nothing to write (an EMPTY LIST over some rays writes their zeros: not run here)
    a.accepted(call(n=0, n_live=0, samples_per_ray=0, live=None, b=False, d_ray=None))
    a.refused(call(samples_per_ray=0), N_SAMPLES_MULTIPLE)
    a.refused(call(n=7, n_live=5), N_SAMPLES_MULTIPLE)
    a.refused(call(d_ray=None), NULL)
    a.refused(call(live=None), NULL)
    a.refused(call(b=False), NULL)
    a.refused(call(without="d4"), NULL)
    a.refused(call(n_live=0, d_ray=None), NULL)          # an empty list reads neither the list nor d4, but still has rows to write
    a.refused(call(samples_per_ray=0, live=None), NULL)                                  # pointers before sizes
    a.refused(call(n_live=0, live=None, b=False, samples_per_ray=0), N_SAMPLES_MULTIPLE)
    a.refused(call(n=2 ** 32, samples_per_ray=1), "too many samples for one call")
    assert a.nothing_was_written()
