"""The vertex step limiter without a GPU (tn_tet_quality / tn_limit_vertex_step, csrc/tn_vertex_guard.hip; the rule: DESIGN.md
section 4.11).  Three layers: the geometry the rule rests on (the width is a lower bound of every extent and the bound w / 2 is
tight), the torch statement on the seven meshes of tests/vertex_guard_cases.py (inside the bound nothing flips, the same step
limited to a whole width flips tetrahedra on every mesh), and tests/host/vertex_guard_emul.cpp, which drives the element
functions of csrc/tn_vertex_guard_core.h -- the bodies of the kernels -- and must equal the statement bit for bit.  Then the
entries' declarations and the adapter's call sequence on a tracer that only records calls.  (The kernels themselves:
tests/test_vertex_guard_gpu.py.)"""
import ctypes
import importlib
import re
import shutil
import struct
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import vertex_guard_cases as vc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"


# ------------------------------------------------------------------------------------------------------------------ geometry
def _squeezed_tets(n, seed):
    """float64 [n, 4, 3]: random tetrahedra, squeezed by up to 1e-3 along two axes and turned"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, size=(n, 4, 3))
    scale = 10.0 ** rng.uniform(-3, 0, size=(n, 1, 3))
    scale[:, :, 0] = 1.0
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return np.einsum("nij,nkj->nki", q, p * scale)


def test_width_is_a_lower_bound_of_every_extent():
    g = vc.geometry()
    tets = _squeezed_tets(30, 3)
    p = torch.from_numpy(tets)
    w = g.tet_width64(p).numpy()
    vol6, norms = (x.numpy() for x in g.tet_slabs(p))
    assert np.all(w > 0) and w.min() < 1e-2 * w.max()                        # the squeeze did something
    np.testing.assert_array_equal(w, (np.abs(vol6)[:, None] / norms).min(1))
    rng = np.random.default_rng(4)
    d = rng.normal(size=(400_000, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    for i in range(len(tets)):
        proj = d @ tets[i].T
        extent = proj.max(1) - proj.min(1)
        assert extent.min() >= w[i] * (1 - 1e-12), (i, extent.min(), w[i])
        # each of the seven slabs contains the tetrahedron: along the slab's normal its extent IS the slab's thickness
        for k, (a, b, c, e) in enumerate(g._SLABS):
            n = np.cross(tets[i, b] - tets[i, a], tets[i, e] - tets[i, c])
            proj_k = tets[i] @ (n / np.linalg.norm(n))
            thickness = abs(vol6[i]) / norms[i, k]
            assert abs((proj_k.max() - proj_k.min()) - thickness) <= 1e-9 * max(thickness, np.abs(tets[i]).max()), (i, k)


@pytest.mark.parametrize("tet", [0, 1, 2, 3, 4, 5])
def test_half_a_width_is_tight(tet):
    """pushed along the thinnest slab's normal towards each other, the two sides keep the orientation at 0.45 w each and lose
    it at 0.55 w each"""
    g = vc.geometry()
    p = _squeezed_tets(6, 9)[tet]
    vol6, norms = (x.numpy()[0] for x in g.tet_slabs(torch.from_numpy(p[None])))
    w = float(g.tet_width64(torch.from_numpy(p[None]))[0])
    a, b, c, e = g._SLABS[int(np.argmax(norms))]
    n = np.cross(p[b] - p[a], p[e] - p[c])
    n /= np.linalg.norm(n)
    proj = p @ n
    upper = proj > 0.5 * (proj.max() + proj.min())
    assert 1 <= upper.sum() <= 3 and abs((proj.max() - proj.min()) - w) < 1e-9
    cells = torch.tensor([[0, 1, 2, 3]])
    before = int(g.tet_orient(torch.from_numpy(p), cells)[0])
    assert before != 0

    def pushed(f):
        return torch.from_numpy(p + np.where(upper, -1.0, 1.0)[:, None] * (f * w) * n)

    assert int(g.tet_orient(pushed(0.45), cells)[0]) == before
    assert int(g.tet_orient(pushed(0.55), cells)[0]) in (0, -before)


# ----------------------------------------------------------------------------------------------------------------- statement
@pytest.mark.parametrize("mesh", vc.CPU_MESHES)
def test_statement_keeps_every_orientation(scenes, mesh):
    old, new, cells = vc.case(scenes, mesh)
    s = vc.statement(scenes, mesh, 0.45)
    out, star = s["xyz"].numpy(), s["star_width"].numpy()
    frozen, clamped = s["frozen"].numpy(), s["clamped"].numpy()
    counters = s["counters"].tolist()
    print(mesh, "V", len(old), "T", len(cells), "counters", counters, "frozen", int(frozen.sum()))
    assert counters[2] == 0 and counters[3] == 0
    assert counters[0] == clamped.sum() > 0
    kept = ~frozen & ~clamped
    np.testing.assert_array_equal(vc.bits(out[frozen]), vc.bits(old[frozen]))
    np.testing.assert_array_equal(vc.bits(out[kept]), vc.bits(new[kept]))
    finite = np.isfinite(star)
    assert np.all(~finite <= kept)                                            # a vertex no tetrahedron names is never limited
    move = np.linalg.norm(out.astype(np.float64) - old.astype(np.float64), axis=1)
    limit = np.float32(0.45) * star
    rho = 2.0 ** -22 * np.abs(old).max(1).astype(np.float64)
    live = finite & ~frozen
    assert np.all(move[live] <= limit[live].astype(np.float64) * (1 + 2.0 ** -20) + rho[live])
    # the freeze rule as the issue states it, and its consequence: rho <= star / 32 for every vertex that may move
    np.testing.assert_array_equal(frozen, ~(star >= np.float32(2.0 ** -17) * np.abs(old).max(1)))
    assert np.all(rho[live] <= star[live].astype(np.float64) / 32)
    # independent of torch: the signed volumes in numpy float64
    vol = lambda x: np.einsum("ij,ij->i", np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]), x[:, 3] - x[:, 0])
    before, after = vol(old.astype(np.float64)[cells]), vol(out.astype(np.float64)[cells])
    assert not np.any(before * after < 0) and not np.any((before != 0) & (after == 0))


@pytest.mark.parametrize("mesh", vc.CPU_MESHES)
def test_the_same_step_limited_to_a_whole_width_flips(scenes, mesh):
    """the power of the check above: the inputs break a limiter that allows twice the bound"""
    s = vc.statement(scenes, mesh, 1.0, check_range=False)
    print(mesh, "counters at 1.0 w, freeze rule off", s["counters"].tolist())
    assert int(s["counters"][2]) > 0
    assert not s["frozen"].any()


def test_statement_refuses_fractions_outside_the_bound(scenes):
    g = vc.geometry()
    old, new, cells = (torch.from_numpy(x) for x in vc.case(scenes, "cube"))
    for f in (0.0, -0.1, 0.4500001, 1.0, float("nan")):
        with pytest.raises(ValueError):
            g.limit_vertex_step_statement(old, new, cells, f)


# ------------------------------------------------------------------------------------------------------------ host emulation
@pytest.fixture(scope="module")
def guard_emul(tmp_path_factory):
    if shutil.which("g++") is None or not Path("/opt/rocm/include/hip/hip_runtime.h").exists():
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path_factory.mktemp("host") / "vertex_guard_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "vertex_guard_emul.cpp")]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


def _run_emul(exe, tmp_path, old, new, cells, fraction, flags=0):
    V, T = len(old), len(cells)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<QQfI", V, T, fraction, flags))
        f.write(np.ascontiguousarray(old, np.float32).tobytes())
        f.write(np.ascontiguousarray(new, np.float32).tobytes())
        f.write(np.ascontiguousarray(cells).astype(np.uint32).tobytes())
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = dst.read_bytes()
    assert len(raw) == 4 * V + 5 * T + 12 * V + 16
    star, raw = np.frombuffer(raw[:4 * V], np.uint32), raw[4 * V:]
    width, raw = np.frombuffer(raw[:4 * T], np.uint32), raw[4 * T:]
    orient, raw = np.frombuffer(raw[:T], np.int8), raw[T:]
    xyz, raw = np.frombuffer(raw[:12 * V], np.uint32).reshape(V, 3), raw[12 * V:]
    return star, width, orient, xyz, np.frombuffer(raw, np.uint32)


@pytest.mark.parametrize("mesh", vc.KERNEL_MESHES)
def test_emulated_kernels_equal_the_statement(guard_emul, tmp_path, scenes, mesh):
    old, new, cells = vc.case(scenes, mesh)
    s = vc.statement(scenes, mesh, 0.45)
    w, o, star_s = vc.quality(scenes, mesh)
    star, width, orient, xyz, counters = _run_emul(guard_emul, tmp_path, old, new, cells, 0.45)
    np.testing.assert_array_equal(width, vc.bits(w.numpy()))
    np.testing.assert_array_equal(orient, o.numpy())
    np.testing.assert_array_equal(star, vc.bits(star_s.numpy()))
    np.testing.assert_array_equal(star, vc.bits(s["star_width"].numpy()))
    np.testing.assert_array_equal(xyz, vc.bits(s["xyz"].numpy()))
    assert counters.tolist() == s["counters"].tolist()
    # another fraction, and the verify pass switched off
    s25 = vc.statement(scenes, mesh, 0.25)
    _, _, _, xyz, counters = _run_emul(guard_emul, tmp_path, old, new, cells, 0.25, flags=1)
    np.testing.assert_array_equal(xyz, vc.bits(s25["xyz"].numpy()))
    assert counters.tolist() == s25["counters"].tolist()[:2] + [0, 0]


def test_emulated_clamp_on_non_finite_and_unreferenced_vertices(guard_emul, tmp_path, scenes):
    """a NaN and an inf coordinate go back to the old position and count as clamped; a vertex no cell names has star width
    +inf and is never limited; an unmoved mesh is untouched"""
    old, new, cells = vc.case(scenes, "random_1500")
    old = np.concatenate([old, [[5.0, 6.0, 7.0]]]).astype(np.float32)            # vertex 1500: named by no cell
    new = np.concatenate([new, [[50.0, -60.0, 70.0]]]).astype(np.float32)
    new[3, 1], new[7, 0] = np.nan, np.inf
    g = vc.geometry()
    s = g.limit_vertex_step_statement(torch.from_numpy(old), torch.from_numpy(new), torch.from_numpy(cells), 0.45)
    assert not s["frozen"][[3, 7]].any() and s["clamped"][[3, 7]].all() and not s["clamped"][1500]
    np.testing.assert_array_equal(vc.bits(s["xyz"].numpy()[[3, 7]]), vc.bits(old[[3, 7]]))
    np.testing.assert_array_equal(vc.bits(s["xyz"].numpy()[1500]), vc.bits(new[1500]))
    star, _, _, xyz, counters = _run_emul(guard_emul, tmp_path, old, new, cells, 0.45)
    assert star[1500] == 0x7F800000
    np.testing.assert_array_equal(xyz, vc.bits(s["xyz"].numpy()))
    assert counters.tolist() == s["counters"].tolist()
    _, _, _, xyz, counters = _run_emul(guard_emul, tmp_path, old, old, cells, 0.45)
    np.testing.assert_array_equal(xyz, vc.bits(old))
    assert counters.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------- entries
def test_guard_entries_are_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_tet_quality\(tn_tracer_t tracer, size_t num_vertices, const float \*xyz, float \*width, int8_t \*orient,\s*"
                     r"float \*star_width,\s*void \*stream\);", header)
    assert re.search(r"int\s+tn_limit_vertex_step\(tn_tracer_t tracer, size_t num_vertices, const float \*xyz_old, float \*xyz_new,\s*"
                     r"float fraction,\s*float \*star_width, uint32_t \*counters, uint32_t flags, void \*stream\);", header)
    assert re.search(r"#define\s+TN_LIMIT_STEP_NO_VERIFY\s+1u", header)
    lib = _lib.load()
    for name in ("tn_tet_quality", "tn_limit_vertex_step"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert len(lib.tn_tet_quality.argtypes) == 7 and len(lib.tn_limit_vertex_step.argtypes) == 9
    assert lib.tn_limit_vertex_step.argtypes[4] is ctypes.c_float
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.supports_vertex_step_limit is True
    assert hasattr(ext.TetrahedraTracer, "tet_quality") and hasattr(ext.TetrahedraTracer, "limit_vertex_step")
    # the grid cap the GPU tests step over is the kernels' own
    src = (CSRC / "tn_vertex_guard.hip").read_text()
    blocks = int(re.search(r"constexpr unsigned GUARD_BLOCKS = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr int BT = (\d+);", src).group(1))
    assert ext.TetrahedraTracer.VERTEX_GUARD_GRID_LANES == blocks * threads
    g = vc.geometry()
    core = (CSRC / "tn_vertex_guard_core.h").read_text()
    assert g.MAX_STEP_FRACTION == 0.45 and "MAX_FRACTION = 0.45f" in core
    assert g.FREEZE_RATIO == 1.0 / 131072 and "FREEZE_RATIO = 1.0f / 131072.f" in core


# ------------------------------------------------------------------------------------------------------------------- adapter
class _RecordingTracer:
    """what _follow_vertices touches of a TetrahedraTracer, recording every call"""
    supports_refit = True
    supports_vertex_step_limit = True

    def __init__(self, vertices, cells):
        self.tetrahedra_vertices, self.tetrahedra_cells = vertices, cells
        self._refittable = False
        self.calls = []

    def load_tetrahedra(self, xyz, cells, refittable=False):
        self.calls.append(("load", refittable))
        self._refittable = refittable
        self.tetrahedra_vertices = xyz

    def update_vertices(self, xyz):
        self.calls.append(("update", xyz.detach().clone()))
        self.tetrahedra_vertices = xyz

    def limit_vertex_step(self, xyz_old, xyz_new, fraction=0.25, verify=True):
        self.calls.append(("limit", xyz_old.clone(), xyz_new.clone(), fraction, xyz_new.data_ptr()))
        xyz_new.copy_(0.5 * (xyz_old + xyz_new))          # any in-place write: here half the way
        return torch.tensor([3, 1, 0, 0], dtype=torch.int32), torch.ones(len(xyz_old))


def _names(tracer):
    return [c[0] for c in tracer.calls]


def test_adapter_limits_then_refits_then_snapshots():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.nn.Parameter(torch.arange(12, dtype=torch.float32).reshape(4, 3))
    tracer, model = _RecordingTracer(v, torch.zeros(1, 4, dtype=torch.int32)), types.SimpleNamespace()
    a = v.detach().clone()
    plugin._follow_vertices(tracer, model, 0.3)
    assert tracer.calls == [("load", True)]
    assert torch.equal(tracer._tn_vertex_snapshot, a) and tracer._tn_vertex_snapshot.data_ptr() != v.data_ptr()
    plugin._follow_vertices(tracer, model, 0.3)                       # nothing moved
    assert _names(tracer) == ["load"]
    with torch.no_grad():
        v += 2.0                                                      # an optimiser step: bumps the version counter
    plugin._follow_vertices(tracer, model, 0.3)
    assert _names(tracer) == ["load", "limit", "update"]
    _, old, new, fraction, ptr = tracer.calls[1]
    assert torch.equal(old, a) and torch.equal(new, a + 2.0) and fraction == 0.3 and ptr == v.data_ptr()
    assert torch.equal(v.detach(), a + 1.0)                           # the parameter itself holds the limited positions ...
    assert torch.equal(tracer.calls[2][1], a + 1.0)                   # ... the refit saw them ...
    assert torch.equal(tracer._tn_vertex_snapshot, a + 1.0)           # ... and the snapshot followed
    assert tracer._tn_vertex_key == (v._version, v.data_ptr())        # the key of AFTER the in-place write:
    plugin._follow_vertices(tracer, model, 0.3)                       # the next call sees nothing new
    assert _names(tracer) == ["load", "limit", "update"]
    assert model._tn_vertex_step_counters.dtype == torch.int64 and model._tn_vertex_step_counters.tolist() == [3, 1, 0, 0]
    with torch.no_grad():
        v -= 1.0
    plugin._follow_vertices(tracer, model, 0.3)
    assert _names(tracer) == ["load", "limit", "update", "limit", "update"]
    assert torch.equal(tracer.calls[3][1], a + 1.0) and model._tn_vertex_step_counters.tolist() == [6, 2, 0, 0]


def test_adapter_without_a_fraction_calls_what_it_called():
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.nn.Parameter(torch.zeros(4, 3))
    tracer = _RecordingTracer(v, torch.zeros(1, 4, dtype=torch.int32))
    for args in ((tracer,), (tracer, types.SimpleNamespace(), None)):
        tracer.calls.clear()
        tracer._refittable = False
        plugin._follow_vertices(*args)
        plugin._follow_vertices(*args)
        with torch.no_grad():
            v += 1.0
        plugin._follow_vertices(*args)
        assert _names(tracer) == ["load", "update"]
        assert not hasattr(tracer, "_tn_vertex_snapshot")


def test_adapter_refuses_a_fraction_without_refit():
    """fused_get_outputs: vertex_step_fraction without refit_vertices is an error, raised before anything is traced"""
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    v = torch.zeros(4, 3)
    tracer = _RecordingTracer(v, torch.zeros(1, 4, dtype=torch.int32))
    model = types.SimpleNamespace(config=types.SimpleNamespace(vertex_step_fraction=0.25), mlp_base=object(),
                                  get_tetrahedra_tracer=lambda: tracer)
    with pytest.raises(ValueError, match="refit_vertices"):
        plugin.fused_get_outputs(model, None)
    assert tracer.calls == []
