"""bench.py's plain run (no --full): the headline alone, the contract keys of its one line, and --dump-outputs -- the
arrays the last timed step returned, for a fixed sample of rays, equal to what trace_rays returns on the same inputs."""
import importlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_and_dumped_outputs(tn, scenes, device, tmp_path):
    import torch

    W, H, P, M = 320, 200, 3000, 512
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--mesh-points", str(P),
                        "--full-json", str(tmp_path / "full.json"), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    short = json.loads(lines[0])
    assert short["metric"] == "ray_tet_intersections_per_s" and short["unit"] == "ray-tet intersections/s"
    assert short["higher_is_better"] is True and short["dtype"] == "f32" and short["steps"] == 3
    assert short["value"] > 0 and short["ms_per_step"] > 0
    line = json.loads((tmp_path / "full.json").read_text())
    for leg in ("cpu_baseline", "configs", "render", "sharded_render", "segments_only"):
        assert leg not in line, leg                      # secondary legs run with --full only
    assert short["value"] * short["ms_per_step"] * 1e-3 == pytest.approx(line["config"]["intersections_per_frame"], rel=1e-6)

    bench = importlib.import_module("bench")
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(got) == {"num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices"}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    pts, cells = scenes.random_mesh(P, 0)
    o, d = bench.frame_rays(scenes, 0, W, H)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    want = tr.trace_rays(torch.from_numpy(o).to(device), torch.from_numpy(d).to(device), M)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(len(o), size=bench.DUMP_ROWS, replace=False))
    np.testing.assert_array_equal(got["num_visited_cells"], want["num_visited_cells"].cpu().numpy().astype(np.float64))
    for k in ("visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices"):
        w = want[k].cpu().numpy()[idx]
        np.testing.assert_array_equal(got[k], w.astype(np.float32 if w.dtype == np.float32 else np.float64), err_msg=k)
