"""The size-edge cases of the device build and the refit (tests/build_edge_cases.py) without a GPU: every case goes through the
CPU emulations of the two kernel files (tests/host/gpu_build_emul.cpp at leaf widths 16, 32 and 64, tests/host/refit_emul.cpp)
and through the host build's check; the conditions the GPU tests (tests/test_build_edges_gpu.py) rely on are asserted here on the
oracle alone -- the aimed rays hit, the oracle's two paths agree on them -- so that no GPU test can pass by comparing two empty
results; `check_median_splits` is shown to reject a wrong split axis and a pair of faces swapped across a median; and the classes
of face and tet counts the cases are meant to meet are computed from the emulation's own report and asserted non-empty."""
import re
import struct
import subprocess

import numpy as np
import pytest

import build_edge_cases as bec
from test_host_build import _run as _run_host_check, emul_check, host_check  # noqa: F401  (fixtures: the compile lines)
from test_refit import refit_emul  # noqa: F401

KEYS = ("num_visited_cells", "visited_cells", "vertex_indices", "hit_distances", "barycentric_coordinates")
N_RAYS, M = 512, 64
_ROWS = {}


def _write(path, cells, *vertex_tables):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(vertex_tables[0]), len(cells)))
        for v in vertex_tables:
            f.write(np.ascontiguousarray(v, np.float32).tobytes())
        f.write(np.ascontiguousarray(cells).astype(np.uint32).tobytes())


def _row(emul_check, tmp_path_factory, scenes, name):
    """one line of the case table, from the emulation's OK lines (run once per case and session)"""
    if name in _ROWS:
        return _ROWS[name]
    pts, cells = bec.cases(scenes)[name]
    path = tmp_path_factory.mktemp("edge") / "mesh.bin"
    _write(path, cells, pts)
    F, hull = bec.face_counts(cells)
    row = {"case": name, "T": len(cells), "F": F, "hull": hull, "unused": len(bec.unreferenced(pts, cells))}
    for lw in bec.LEAF_WIDTHS:
        r = subprocess.run([str(emul_check), str(path), str(lw)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK"), (name, lw, r.stdout, r.stderr)
        got = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", r.stdout)}
        assert got["variants"] == 4 * len(cells) and got["faces"] == F and got["hull"] == hull, (name, lw, r.stdout)
        assert got["leaves"] == len(bec.leaf_counts(F, lw)), (name, lw, r.stdout)
        row[lw] = (got["leaves"], got["wide_nodes"], got["wide_levels"])
    _ROWS[name] = row
    return row


@pytest.mark.parametrize("name", bec.NAMES)
def test_device_build_emulated_equals_host_build(emul_check, host_check, tmp_path, tmp_path_factory, oracle, scenes, name):
    pts, cells = bec.cases(scenes)[name]
    _row(emul_check, tmp_path_factory, scenes, name)                    # gpu_build_emul at the three leaf widths
    out, faces, face_tets = _run_host_check(host_check, tmp_path, pts, cells)
    want_faces, want_ft = oracle.build_faces(cells)
    np.testing.assert_array_equal(faces, want_faces)
    np.testing.assert_array_equal(face_tets, want_ft)
    assert f"variants {4 * len(cells)}" in out


@pytest.mark.parametrize("name", bec.NAMES)
def test_refit_emulated_equals_fresh_build(refit_emul, tmp_path, scenes, name):
    pts, b, cells = bec.case_ab(scenes, name)
    path = tmp_path / "mesh.bin"
    _write(path, cells, pts, b)
    for leaf_width in bec.LEAF_WIDTHS:
        r = subprocess.run([str(refit_emul), str(path), str(leaf_width)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK"), (name, leaf_width, r.stdout, r.stderr)
        assert f"records {4 * len(cells)}" in r.stdout
        assert int(re.search(r"\((\d+) moved\)", r.stdout).group(1)) > 0


def test_the_move_keeps_unreferenced_vertices_and_moves_interior_ones(scenes):
    all_cases = bec.cases(scenes)
    pts, cells = all_cases["nan_unused"]
    b = bec.moved(pts, cells)
    un = bec.unreferenced(pts, cells)
    assert len(un) and np.isnan(b[un]).all() and np.isfinite(b[bec.referenced(cells)]).all()
    pts, cells = all_cases["prefix_2049"]
    b = bec.moved(pts, cells)
    un, hull = bec.unreferenced(pts, cells), bec.hull_vertices(cells)
    assert len(un) and np.array_equal(b[un], bec.affine(pts[un])) and np.array_equal(b[hull], bec.affine(pts[hull]))
    interior = np.setdiff1d(bec.referenced(cells), hull)
    assert len(interior) and np.any(b[interior] != bec.affine(pts[interior]))
    # the whole, convex mesh: what refit_cases.moved gives
    import refit_cases

    pts, cells = all_cases["prefix_whole"]
    assert np.array_equal(bec.moved(pts, cells), refit_cases.moved(pts, cells))


@pytest.mark.parametrize("name", bec.NAMES)
def test_aimed_rays_hit_and_the_oracle_paths_agree(oracle, scenes, name):
    """the condition of the GPU traces, on the oracle alone: at least 90 % of the aimed rays report a hit (no condition on
    `flat`), before and after the move; the BVH path and the all-faces path of the oracle agree bit for bit"""
    pts, b, cells = bec.case_ab(scenes, name)
    for p in (pts, b):
        o, d = bec.aimed_rays(p, cells, N_RAYS, 70)
        bvh, plain = oracle.OracleTracer(use_bvh=True), oracle.OracleTracer()
        bvh.load_tetrahedra(p, cells)
        plain.load_tetrahedra(p, cells)
        a, b = bvh.trace_rays(o, d, M), plain.trace_rays(o, d, M)
        for k in KEYS:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), (name, k)
        share = float((a["num_visited_cells"] > 0).mean())
        if name != "flat":            # (a zero-volume tetrahedron: a hit on a handful of rays at most; bit equality is its whole bar)
            assert share >= 0.9, (name, share)


# ---------------------------------------------------------------------------------------------------------------- the tree check
def _numpy_tree(faces, points, leaf_w, narrowest=False):
    """leaf rows [n_leaves, leaf_w] of a median-split tree over `faces`, built with numpy sorts"""
    p = np.asarray(points, np.float32)
    tri = p[np.asarray(faces, np.int64)]
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * (np.float32(1.0) / np.float32(3.0))
    rows = []

    def build(ids):
        if len(ids) <= leaf_w:
            rows.append(np.concatenate([ids, np.full(leaf_w - len(ids), 0xFFFFFFFF)]))
            return
        ext = cen[ids].max(0) - cen[ids].min(0)
        ax = 0
        for a in (1, 2):
            if (ext[a] < ext[ax]) if narrowest else (ext[a] > ext[ax]):
                ax = a
        ids = ids[np.argsort(cen[ids, ax], kind="stable")]
        build(ids[:len(ids) // 2])
        build(ids[len(ids) // 2:])

    build(np.arange(len(faces), dtype=np.int64))
    return np.array(rows, np.int64).astype(np.uint32), cen


def test_check_median_splits_rejects_wrong_trees(oracle, scenes):
    pts, cells = bec.cases(scenes)["prefix_65"]
    faces, _ = oracle.build_faces(cells)
    leaf_w = 16
    assert len(faces) > 4 * leaf_w
    good, cen = _numpy_tree(faces, pts, leaf_w)
    assert bec.check_median_splits(faces, good, pts, leaf_w) == len(good) - 1
    with pytest.raises(AssertionError, match="not split at the median"):
        bec.check_median_splits(faces, _numpy_tree(faces, pts, leaf_w, narrowest=True)[0], pts, leaf_w)
    # one pair of faces swapped across the root's median: the lowest of the lower half against the highest of the upper half
    order, _ = bec.final_face_order(good)
    ext = cen.max(0) - cen.min(0)
    ax = int(np.argmax(ext))
    half = len(order) // 2
    i, j = int(np.argmin(cen[order[:half], ax])), half + int(np.argmax(cen[order[half:], ax]))
    assert cen[order[i], ax] < cen[order[j], ax]
    flat = good.reshape(-1).copy()
    slots = np.nonzero(flat != 0xFFFFFFFF)[0]
    flat[slots[i]], flat[slots[j]] = flat[slots[j]], flat[slots[i]]
    with pytest.raises(AssertionError, match="not split at the median"):
        bec.check_median_splits(faces, flat.reshape(good.shape), pts, leaf_w)
    # a face moved from the emptiest row to the fullest one that has room: other leaf counts than the median-split tree's
    rows = good.copy()
    count = (rows != 0xFFFFFFFF).sum(1)
    assert count.max() < leaf_w
    a, b = int(np.argmax(count)), int(np.argmin(count))
    rows[a, count[a]], rows[b, count[b] - 1] = rows[b, count[b] - 1], 0xFFFFFFFF
    with pytest.raises(AssertionError, match="leaf counts"):
        bec.check_median_splits(faces, rows, pts, leaf_w)


def _split_rounds_like_the_device(faces, points, leaf_w, swap_axis_args=False, lane63=True):
    """The split rounds of device_build (csrc/tn_build.hip) restated with their wave structure: per round, k_seg_bounds reduces
    the centroid bounds of every segment from the runs of equal segment ids inside each 64-lane wave -- a run adds its result
    when its last lane is lane 63 or the next lane holds another id (__shfl_down past the wave returns the lane's own id; an
    inactive lane holds 0xFFFFFFFF) --, k_seg_keys takes core::split_axis of those bounds, and a stable sort by (segment,
    coordinate) orders the positions.  Returns the leaf rows.  swap_axis_args: split_axis(chi, clo); lane63=False: the
    `lane == 63 ||` of k_seg_bounds dropped -- two ways the kernels can be wrong and still give a valid tree."""
    p = np.asarray(points, np.float32)
    tri = p[np.asarray(faces, np.int64)]
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * (np.float32(1.0) / np.float32(3.0))
    F = len(cen)
    order = np.arange(F)
    segs = [(0, F)]
    while any(count > leaf_w for _, count in segs):
        seg_of = np.concatenate([np.full(count, s) for s, (_, count) in enumerate(segs)])
        lo = np.full((len(segs), 3), np.inf, np.float32)
        hi = np.full((len(segs), 3), -np.inf, np.float32)
        for wave in range(0, F, 64):
            i = wave
            while i < min(wave + 64, F):
                s, j = seg_of[i], i
                while j + 1 < min(wave + 64, F) and seg_of[j + 1] == s:
                    j += 1
                # j = the last lane of the run: lane 63, or the next lane holds another id (or is inactive)
                if lane63 or (j - wave) != 63:
                    c = cen[order[i:j + 1]]
                    lo[s], hi[s] = np.minimum(lo[s], c.min(0)), np.maximum(hi[s], c.max(0))
                i = j + 1
        with np.errstate(invalid="ignore"):
            ext = (lo - hi) if swap_axis_args else (hi - lo)
        ax = np.zeros(len(segs), np.int64)
        for a in (1, 2):
            ax = np.where(ext[:, a] > ext[np.arange(len(segs)), ax], a, ax)
        value = cen[order, ax[seg_of]]
        order = order[np.lexsort((value, seg_of))]            # stable, like the radix sort
        segs = [piece for first, count in segs
                for piece in (((first, count // 2), (first + count // 2, count - count // 2)) if count > leaf_w else ((first, count),))]
    return np.array([np.concatenate([order[f:f + c], np.full(leaf_w - c, 0xFFFFFFFF)]) for f, c in segs], np.int64).astype(np.uint32)


def test_check_median_splits_catches_the_two_kernel_mutations(oracle, scenes):
    """The mutation check of the split rounds, on the restatement above (a kernel made wrong on purpose is not something to run on
    a GPU): with split_axis's arguments swapped in k_seg_keys (negated extents: the NARROWEST axis wins) and with `lane == 63 ||`
    dropped from k_seg_bounds (every run that ends at a wave's last lane loses its bounds, so at the root only the last, partly
    filled wave counts) the tree stays a valid partition with tight boxes -- _check_bvh passes and every trace is bit-identical
    -- and check_median_splits rejects it."""
    caught = {"swap_axis_args": [], "lane63": []}
    for name in ("prefix_33", "prefix_65", "prefix_257", "shuffled", "prefix_1025"):
        pts, cells = bec.cases(scenes)[name]
        faces, _ = oracle.build_faces(cells)
        for lw in bec.LEAF_WIDTHS:
            if len(faces) <= lw:
                continue
            good = _split_rounds_like_the_device(faces, pts, lw)
            assert bec.check_median_splits(faces, good, pts, lw) == len(good) - 1
            for what, kw in (("swap_axis_args", dict(swap_axis_args=True)), ("lane63", dict(lane63=False))):
                bad = _split_rounds_like_the_device(faces, pts, lw, **kw)
                assert np.array_equal(np.sort(bad[bad != 0xFFFFFFFF]), np.arange(len(faces)))      # still a partition
                try:
                    bec.check_median_splits(faces, bad, pts, lw)
                except AssertionError as e:
                    assert "not split at the median" in str(e)
                    caught[what].append((name, lw))
    print(caught)
    # the bar: each mutation fails the check on at least one case (with the meshes this was written on: the swapped arguments on
    # all 15 (case, leaf width) pairs, the dropped lane-63 term on the 12 whose root segment spans more than two waves)
    assert caught["swap_axis_args"] and caught["lane63"], caught


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_every_size_class_is_met(emul_check, tmp_path_factory, scenes):
    table = [_row(emul_check, tmp_path_factory, scenes, name) for name in bec.NAMES]
    print("\n" + bec.format_table(table))
    met = bec.classes(table)
    for what, names in met.items():
        print(f"{what}: {' '.join(names)}")
    empty = [what for what, names in met.items() if not names]
    assert not empty, f"no case meets: {empty}"
    for r in table:                                   # the restated topology agrees with the emulation
        for lw in bec.LEAF_WIDTHS:
            assert (r[lw][0] == 1) == (r["F"] <= lw) == (bec.split_rounds(r["F"], lw) == 0)
