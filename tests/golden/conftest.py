"""The reference's own tests staged under tests/golden/ref/tests, when the suite collects them: they import `tetranerf`
(the reference's op layer on the one-file shim) and `trimesh` (the stand-in) from tests/golden/ref, as the staged
pytest.ini's `pythonpath = .` does for tests/test_reference_suite_gpu.py's subprocess run; the modules that call CUDA
are marked gpu; each test runs in a temporary working directory (the triangles variant exports a point cloud into its
working directory)."""
import sys
from pathlib import Path

import pytest

REF = Path(__file__).resolve().parent / "ref"
if str(REF) not in sys.path:
    sys.path.insert(0, str(REF))

GPU_MODULES = {"test_uint32.py", "test_tetrahedra_tracer.py", "test_tetrahedra_tracer_triangles.py"}


@pytest.hookimpl(tryfirst=True)
def pytest_collection_modifyitems(config, items):
    for item in items:
        p = Path(str(item.fspath))
        if p.parent == REF / "tests" and p.name in GPU_MODULES:
            item.add_marker(pytest.mark.gpu)


@pytest.fixture(autouse=True)
def _in_tmp_dir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
