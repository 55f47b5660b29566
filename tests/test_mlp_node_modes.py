"""The trailing arithmetic modes of the two fused-MLP autograd nodes, CPU side: render._FusedMlpFunction and
render._FusedMlpCulledFunction take the 12 weights followed by zero to three modes -- the forward's, the dX chain's, the
weight-gradient GEMMs' -- and an absent one is "fp32".  The ops the nodes call (cpp.mlp_forward_gather_train[_indexed],
cpp.mlp_backward) are replaced by recorders that return CPU tensors of the right shapes, so the test states what the nodes hand
on and that autograd accepts the number of gradients they return; no kernel runs."""
import importlib

import pytest
import torch

R, S, V = 2, 3, 5
N = R * S
TRAILING = [(), ("bf16x3",), ("bf16x3", "bf16x3"), ("bf16x3", "bf16x3", "bf16x3"), ("fp32", "bf16x3"), ("fp32", "fp32", "bf16x3"),
            ("bf16x3", "fp32", "fp32"), ("fp32", "bf16x3", "fp32")]


def install_recorders(cpp, monkeypatch):
    """replace the three ops by recorders; -> {"forward": [(node, mode)], "backward": [(adjoint_mode, dw_mode)]}"""
    calls = {"forward": [], "backward": []}

    def saved_of(cls, **attrs):
        sv = cls()
        sv.n, sv.S, sv.acts, sv.masks = N, S, None, None
        for k, v in attrs.items():
            setattr(sv, k, v)
        return sv

    def forward(vi, bc, field, dirs, weights, samples_per_ray, ray_head_bias=None, mode="fp32"):
        assert len(weights) == 12 and all(isinstance(w, torch.Tensor) for w in weights) and samples_per_ray == S
        calls["forward"].append(("dense", mode))
        sv = saved_of(cpp.MlpSaved, sigma=torch.rand(N), rgb=torch.rand(N, 3))
        return sv.sigma, sv.rgb, sv

    def forward_indexed(live, n_live, vi, bc, field, dirs, weights, samples_per_ray, ray_head_bias=None, mode="fp32", sigma=None,
                        rgb=None):
        assert len(weights) == 12 and all(isinstance(w, torch.Tensor) for w in weights) and samples_per_ray == S
        assert tuple(sigma.shape) == (N,) and tuple(rgb.shape) == (N, 3)
        calls["forward"].append(("indexed", mode))
        sv = saved_of(cpp.MlpSavedIndexed, sigma=sigma, rgb=rgb, n_samples=N, live=live)
        sv.n = n_live
        return sigma, rgb, sv

    def backward(saved, vi, bc, field, dirs, weights, sigma, rgb, d_sigma, d_rgb, want_ray_head_grad=False, want_bary_grad=False,
                 adjoint_mode="fp32", dw_mode="fp32"):
        assert saved.sigma is None and saved.rgb is None      # (the node holds its outputs through save_for_backward)
        assert len(weights) == 12 and tuple(d_sigma.shape) == (N,) and tuple(d_rgb.shape) == (N, 3)
        calls["backward"].append((adjoint_mode, dw_mode))
        res = (torch.ones(64, V), [torch.ones(shp) for shp in cpp._WEIGHT_SHAPES])
        if want_ray_head_grad:
            res += (torch.ones(R, 128),)
        if want_bary_grad:
            res += (torch.ones(N, 3),)
        return res

    monkeypatch.setattr(cpp, "mlp_forward_gather_train", forward)
    monkeypatch.setattr(cpp, "mlp_forward_gather_train_indexed", forward_indexed)
    monkeypatch.setattr(cpp, "mlp_backward", backward)
    return calls


@pytest.fixture
def recorded(tn, monkeypatch):
    return install_recorders(tn.cpp, monkeypatch)


def _inputs(tn, bias):
    g = torch.Generator().manual_seed(3)
    vi = torch.randint(0, V, (R, S, 4), generator=g, dtype=torch.int32)
    bc = torch.rand(R, S, 3, generator=g)
    field = torch.randn(64, V, generator=g).requires_grad_(True)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    hb = torch.randn(R, 128, generator=g).requires_grad_(True) if bias else None
    w = [torch.randn(shp, generator=g).requires_grad_(True) for shp in tn.cpp._WEIGHT_SHAPES]
    return vi, bc, field, dirs, hb, w


@pytest.mark.parametrize("bias", [False, True], ids=["no_bias", "ray_head_bias"])
@pytest.mark.parametrize("trailing", TRAILING, ids=["+".join(t) or "none" for t in TRAILING])
@pytest.mark.parametrize("node", ["dense", "indexed"])
def test_nodes_read_their_trailing_modes_by_position(tn, recorded, node, trailing, bias):
    run_node(tn, recorded, node, trailing, bias)


def run_node(tn, recorded, node, trailing, bias):
    """one forward and backward of a node with `trailing` modes behind its weights -> the (mode, adjoint_mode, dw_mode) the ops got"""
    render = importlib.import_module("tetra-nerf_amd.render")
    vi, bc, field, dirs, hb, w = _inputs(tn, bias)
    if node == "dense":
        sigma, rgb = render._FusedMlpFunction.apply(vi, bc, field, dirs, S, hb, *w, *trailing)
    else:
        live = torch.arange(N, dtype=torch.int32)
        sigma, rgb = render._FusedMlpCulledFunction.apply(live, 4, (torch.zeros(N), torch.zeros(N, 3)), vi, bc, field, dirs, S, hb, *w,
                                                          *trailing)
    assert tuple(sigma.shape) == (N,) and tuple(rgb.shape) == (N, 3)
    want = tuple(trailing) + ("fp32",) * (3 - len(trailing))
    assert recorded["forward"] == [(node, want[0])]
    assert recorded["backward"] == []
    (sigma.sum() + rgb.sum()).backward()          # (raises when the node returns another number of gradients than it has inputs)
    assert recorded["backward"] == [(want[1], want[2])]
    assert torch.equal(field.grad, torch.ones(64, V))
    assert all(torch.equal(x.grad, torch.ones_like(x)) for x in w)
    if bias:
        assert torch.equal(hb.grad, torch.ones(R, 128))
    got = (recorded["forward"].pop()[1],) + recorded["backward"].pop()
    assert got == want
    return got
