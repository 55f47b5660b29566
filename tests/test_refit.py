"""The refit (tn_update_vertices, csrc/tn_refit.hip) without a GPU: tests/host/refit_emul.cpp drives the element functions of
csrc/tn_build_core.h -- the bodies of the refit's kernels -- from CPU loops.  It builds on vertices A, refits to B and compares
with a build on B: pn and the thin exponent of every (caller tet id, entry face) are a fresh build's bytes, every other byte of
every record is untouched, the face BVH keeps the invariants tests/test_build_gpu.py::_check_bvh states, the hull triangles are
a fresh build's, and a refit back to A restores every table byte for byte.  (The kernels themselves: tests/test_refit_gpu.py.)"""
import ctypes
import importlib
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import refit_cases

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tetra-nerf_amd" / "csrc"


@pytest.fixture(scope="module")
def refit_emul(tmp_path_factory):
    if shutil.which("g++") is None or not Path("/opt/rocm/include/hip/hip_runtime.h").exists():
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path_factory.mktemp("host") / "refit_emul"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}", "-o", str(exe),
           str(ROOT / "tests" / "host" / "refit_emul.cpp"), str(CSRC / "tn_mesh.cpp")]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("mesh", ["random_1500", "grid_12_jitter", "grid_16", "cube"])
def test_refit_emulated_equals_fresh_build(refit_emul, tmp_path, scenes, mesh):
    pts, cells = refit_cases.meshes(scenes)[mesh]
    b = refit_cases.moved(pts, cells)
    path = tmp_path / "mesh.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(pts), len(cells)))
        f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        f.write(np.ascontiguousarray(b, np.float32).tobytes())
        f.write(np.ascontiguousarray(cells).astype(np.uint32).tobytes())
    for leaf_width in (16, 64):
        r = subprocess.run([str(refit_emul), str(path), str(leaf_width)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK"), (leaf_width, r.stdout, r.stderr)
        assert f"records {4 * len(cells)}" in r.stdout
        assert int(re.search(r"\((\d+) moved\)", r.stdout).group(1)) > 0


def test_the_move_is_what_the_checks_assume(scenes):
    """the displacement itself: interior vertices move, hull vertices only through the affine map, no tetrahedron flips (asserted
    inside `moved`)"""
    pts, cells = refit_cases.meshes(scenes)["random_1500"]
    b = refit_cases.moved(pts, cells)
    hull = refit_cases.hull_vertices(cells)
    assert 0 < len(hull) < len(pts)
    np.testing.assert_array_equal(b[hull], refit_cases.affine(pts[hull]))
    interior = np.setdiff1d(np.arange(len(pts)), hull)
    assert np.any(b[interior] != refit_cases.affine(pts[interior]))


def test_refit_entry_is_declared_bound_and_exported():
    """additive entries: the ABI number stays, the header declares them, the binding binds them, the library exports them"""
    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (ROOT / "include" / "tetranerf_hip.h").read_text()
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(r"int\s+tn_update_vertices\(tn_tracer_t tracer, size_t num_vertices, const float \*xyz, void \*stream\);", header)
    assert '"refit_tables"' in header
    lib = _lib.load()
    for name in ("tn_update_vertices", "tn_refit_table_bytes"):
        assert name in _lib.SYMBOLS and hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), name)
    assert len(lib.tn_update_vertices.argtypes) == 4
    ext = importlib.import_module("tetra-nerf_amd.tetranerf_cpp_extension")
    assert ext.TetrahedraTracer.supports_refit is True and hasattr(ext.TetrahedraTracer, "update_vertices")
