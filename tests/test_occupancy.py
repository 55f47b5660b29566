"""The per-tetrahedron occupancy field on the CPU: the ABI additions, the two PyTorch statements everything else is tested against
(render.occupancy_update_statement, render.cull_mask_statement), the culled render_reference on the oracle tracer, and the
plugin's opt-in wiring.  The kernels themselves: tests/test_occupancy_gpu.py."""
import ctypes
import importlib
import math
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
render = importlib.import_module("tetra-nerf_amd.render")
NEW = ("tn_occupancy_update", "tn_cull_samples", "tn_mlp_forward_gather_indexed")


def test_abi_additions_keep_version_6():
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/tetranerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the shared library"
        assert name in _lib.SYMBOLS
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header)
    assert _lib.ABI_VERSION == 6 and lib.tn_abi_version() == 6
    # every new entry point's comment says where the reference declares the field, and that it leaves it unused
    for name in NEW:
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "model.py:98-99,256-265" in comment and "unused" in comment, name


def _update_loop(occ, cells, sigma, decay):
    """the update statement as a scalar loop over float32 values"""
    T = len(occ)
    d = np.float32(decay)
    out = [np.float32(d * np.float32(x)) for x in occ]
    for c, s in zip(cells, sigma):
        c = int(c)
        if c < 0 or c >= T:                 # unmatched (-1 / 0xFFFFFFFF) or beyond the field
            continue
        s = np.float32(s)
        if not s >= 0:                      # NaN, negative
            continue
        if math.isnan(out[c]):
            continue
        out[c] = max(out[c], s)
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("unmatched", [-1, 0xFFFFFFFF])
def test_update_statement_equals_scalar_loop(unmatched):
    occ = torch.tensor([0.5, 2.0, 0.0, 7.0, 1.0, float("nan")], dtype=torch.float32)
    # duplicates (cell 1 three times, cell 0 twice), an unmatched id, ids >= T, a NaN and a negative sigma, +inf, a NaN occupancy
    cells = [1, 1, 0, unmatched, 6, 1, 0, 3, 4, 4, 1000, 5, 2]
    sigma = [0.25, 3.5, 0.1, 99.0, 99.0, 3.0, 0.75, float("nan"), -5.0, float("inf"), 1.0, 4.0, 0.0]
    decay = 0.95
    dtype = torch.int32 if unmatched < 0 else torch.int64
    got = render.occupancy_update_statement(occ, torch.tensor(cells, dtype=dtype), torch.tensor(sigma), decay)
    want = _update_loop(occ.numpy(), cells, sigma, decay)
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.numpy(), want)          # (NaN == NaN for numpy's array_equal of arrays: position 5)
    # spelled out: cell 1 takes its largest sample, cell 0 too, cell 2 is only touched by sigma 0 and decays, cell 3 (NaN sample)
    # only decays, cell 4 ignores the negative sample and takes +inf, the NaN occupancy stays
    f = np.float32
    assert got[1] == 3.5 and got[0] == 0.75 and got[2] == 0.0 and got[3] == f(f(0.95) * f(7.0)) and got[4] == float("inf")
    assert math.isnan(got[5])
    # order-independent
    perm = torch.randperm(len(cells), generator=torch.Generator().manual_seed(0))
    got2 = render.occupancy_update_statement(occ, torch.tensor(cells, dtype=dtype)[perm], torch.tensor(sigma)[perm], decay)
    np.testing.assert_array_equal(got2.numpy(), got.numpy())
    # the input is not modified, shapes other than flat are accepted
    assert occ[1] == 2.0
    got3 = render.occupancy_update_statement(occ, torch.tensor(cells + [unmatched], dtype=dtype).view(2, 7),
                                             torch.tensor(sigma + [1.0]).view(2, 7), decay)
    np.testing.assert_array_equal(got3.numpy(), got.numpy())


def test_update_statement_single_tetrahedron():
    occ = torch.tensor([1.0])
    cells = torch.tensor([0, 0, 1, -1, 0], dtype=torch.int32)
    sigma = torch.tensor([0.5, 0.25, 9.0, 9.0, float("nan")])
    np.testing.assert_array_equal(render.occupancy_update_statement(occ, cells, sigma, 0.25).numpy(), np.float32([0.5]))
    np.testing.assert_array_equal(render.occupancy_update_statement(occ, cells, sigma, 0.75).numpy(), np.float32([0.75]))
    np.testing.assert_array_equal(render.occupancy_update_statement(occ, cells[:0], sigma[:0], 0.5).numpy(), np.float32([0.5]))


def test_cull_mask_statement():
    occ = torch.tensor([0.0, 0.5, 1.0, float("nan")])
    cells = torch.tensor([[0, 1, 2, 3], [-1, 4, 1, 0]], dtype=torch.int32)
    got = render.cull_mask_statement(cells, occ, 0.75)
    # below the threshold: cells 0 and 1; NaN occupancy, the unmatched sample and the id >= T are live
    assert got.tolist() == [[True, True, False, False], [False, False, True, True]]
    assert got.shape == cells.shape and got.dtype == torch.bool
    assert not render.cull_mask_statement(cells, occ, 0.0).any()          # threshold <= 0 culls nothing
    assert not render.cull_mask_statement(cells, -occ, -1.0).any()
    u = torch.tensor([0, 0xFFFFFFFF, 1], dtype=torch.int64)                # the matcher's uint32 "unmatched"
    assert render.cull_mask_statement(u, occ, 10.0).tolist() == [True, False, True]
    assert not render.cull_mask_statement(cells, occ[:0], 1.0).any()


@pytest.fixture(scope="module")
def scene(oracle, scenes):
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import reference_model as rm

    pts, cells = scenes.random_mesh(500, 5)
    tracer = rm.OracleTorchTracer(oracle, pts, cells)
    o, d = scenes.outside_in_rays(96, 6)
    o, d = np.concatenate([o, o[:8] + 50.0]), np.concatenate([d, d[:8]])      # + rays that miss the mesh
    torch.manual_seed(0)
    mlp = render.TetraMLP()
    field = torch.rand(64, len(pts)) * 2 - 1
    return SimpleNamespace(tracer=tracer, interp=rm.einsum_interpolate_values, mlp=mlp, field=field, T=len(cells),
                           o=torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32)),
                           d=torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)))


@pytest.mark.parametrize("S,S_fine", [(13, 0), (9, 7)])
def test_render_reference_culled(scene, S, S_fine):
    sc = scene

    def run(tracer=sc.tracer, mlp=sc.mlp, **kw):
        with torch.no_grad():
            return render.render_reference(tracer, sc.interp, sc.field, mlp, sc.o, sc.d, S, 256, num_fine_samples=S_fine, **kw)

    plain = run()
    hit = plain["ray_mask"]
    assert 0 < int(hit.sum()) < len(sc.o)
    occ = torch.rand(sc.T, generator=torch.Generator().manual_seed(1))
    with pytest.raises(RuntimeError, match="both or neither"):
        run(occupancy=occ)
    # threshold 0: the unculled result, exactly
    zero = run(occupancy=occ, occupancy_threshold=0.0)
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(zero[k], plain[k]), k
    # a threshold above every occupancy: nothing accumulates, every ray shows the background (an unmatched sample would stay live:
    # the bin centres of rays through a convex mesh all lie inside it)
    empty = run(occupancy=occ, occupancy_threshold=2.0)
    assert torch.all(empty["accumulation"] == 0.0) and torch.all(empty["rgb"] == 1.0)
    assert torch.equal(empty["ray_mask"], hit)
    # mixed: equal to the same function with the densities / colours masked by cull_mask_statement by hand, through a tracer that
    # records the matched cells of each pass and an MLP adapter that masks with them
    thr = 0.5
    seen = []

    class Recording:
        def trace_rays(self, *a):
            return sc.tracer.trace_rays(*a)

        def find_visited_cells(self, *a):
            out = sc.tracer.find_visited_cells(*a)
            seen.append(render.cull_mask_statement(out["cell_indices"], occ, thr))
            return out

    class Masked:
        def coarse_sigma(self, feats):
            return torch.where(seen[-1], torch.zeros(()), render.coarse_sigma(sc.mlp, feats))

        def __call__(self, feats, dirs):
            sigma, col = sc.mlp(feats, dirs)
            m = seen[-1][..., None]
            return torch.where(m, torch.zeros(()), sigma), torch.where(m, torch.zeros(()), col)

    by_hand = run(tracer=Recording(), mlp=Masked())
    mixed = run(occupancy=occ, occupancy_threshold=thr)
    assert len(seen) == (2 if S_fine else 1) and all(0 < int(m.sum()) < m.numel() for m in seen)
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(mixed[k], by_hand[k]), k
    assert not torch.equal(mixed["rgb"], plain["rgb"])


class _RecordingRenderer:
    def __init__(self, tracer, field):
        self.tracer, self.field, self.calls = tracer, field, []
        self.mlp = SimpleNamespace(ray_head_bias=lambda ray_bundle: None)

    def render(self, o, d, **kw):
        self.calls.append(("render", kw))
        return {}

    def render_train(self, o, d, **kw):
        self.calls.append(("render_train", kw))
        return {}


def _stub_model(config, occupancy):
    tracer = object()
    model = SimpleNamespace(config=SimpleNamespace(background_color="white", **config), mlp_base=object(), training=False,
                            tetrahedra_field=torch.zeros(64, 4), get_tetrahedra_tracer=lambda: tracer)
    if occupancy is not None:
        model.tetrahedra_occupancy = occupancy
    model._tn_renderer = _RecordingRenderer(tracer, model.tetrahedra_field)
    return model


def test_plugin_passes_the_occupancy_only_when_asked():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    rays = SimpleNamespace(origins=torch.zeros(3, 3), directions=torch.ones(3, 3))
    occ = torch.zeros(7)

    def calls(config, occupancy):
        model = _stub_model(config, occupancy)
        plugin.fused_get_outputs(model, rays)
        model.training = True
        plugin.fused_get_outputs(model, rays)
        (k0, kw0), (k1, kw1) = model._tn_renderer.calls
        assert (k0, k1) == ("render", "render_train")
        return kw0, kw1

    occ_keys = {"occupancy", "occupancy_threshold", "occupancy_decay"}
    # use_occupancy_field=True alone (the buffer exists, the two fields do not): exactly as today
    for config, occupancy in (({}, occ), ({}, None), ({"occupancy_threshold": 0.1, "occupancy_decay": 0.9}, None),
                              ({"occupancy_threshold": None, "occupancy_decay": None}, occ)):
        ev, tr = calls(config, occupancy)
        assert not occ_keys & set(ev) and not occ_keys & set(tr), (config, occupancy)
    ev, tr = calls({"occupancy_threshold": 0.1}, occ)
    assert ev["occupancy"] is occ and ev["occupancy_threshold"] == 0.1 and not occ_keys & set(tr)
    ev, tr = calls({"occupancy_decay": 0.9}, occ)
    assert not occ_keys & set(ev) and tr["occupancy"] is occ and tr["occupancy_decay"] == 0.9
    ev, tr = calls({"occupancy_threshold": 0.1, "occupancy_decay": 0.9}, occ)
    assert set(ev) & occ_keys == {"occupancy", "occupancy_threshold"} and set(tr) & occ_keys == {"occupancy", "occupancy_decay"}


def test_renderer_argument_rules(scene):
    sc = scene
    rd = render.TetraRenderer(sc.tracer, sc.field, sc.mlp, 8, 256, cache_field=False, device_samplers=False)
    occ = torch.zeros(sc.T)
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render(sc.o, sc.d, occupancy=occ)
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render(sc.o, sc.d, occupancy_threshold=0.5)
    with pytest.raises(RuntimeError, match="bf16"):
        rd.render(sc.o, sc.d, occupancy=occ, occupancy_threshold=0.5, mlp_mode="bf16")
    with pytest.raises(RuntimeError, match="both or neither"):
        rd.render_train(sc.o, sc.d, occupancy=occ)
    assert rd._one_launch_ok("fp32", culled=True) is False
