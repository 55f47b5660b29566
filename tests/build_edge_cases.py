"""The meshes, the move, the rays and the tree check of the size-edge tests of the device build (csrc/tn_build.hip) and the refit
(csrc/tn_refit.hip), stated once for tests/test_build_edge_cases.py (CPU) and tests/test_build_edges_gpu.py.

The kernels of both files dispatch on the tet count T (n4 = 4T lanes against 256-lane blocks, the partly filled last wave of
k_tet_bounds, the grid cap of k_refit_records at 1024 x 256 lanes) and on the face count F (F <= leaf width: the root is a leaf
and no split round runs; the shuffle-segmented reduction of k_seg_bounds with runs ending at lane 63 or starting mid-wave; one,
two and three levels of 64-wide nodes).  The cases put T on those edges; which F classes they meet is computed, not assumed
(`classes`), because Qhull may triangulate the same points differently between installations.

A prefix cells[:T] of a face-manifold mesh is face-manifold (no face gains a third tet); it is non-convex and may be
disconnected.  The vertex table is left whole, so the small cases carry vertices that no cell references."""
import numpy as np

from refit_cases import affine, affine_dirs, hull_vertices, signed_volumes, star_min_height  # noqa: F401  (re-exported)

PREFIX_T = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
            1023, 1024, 1025, 2047, 2048, 2049)
STRIDE_T = (65535, 65536, 65537)       # 4T = one block short of the grid cap of k_refit_records, the cap, the second trip
REFIT_GRID_LANES = 1024 * 256          # tn_refit.hip: RECORD_BLOCKS * BT
LEAF_WIDTHS = (16, 32, 64)

SMALL = tuple(f"prefix_{t}" for t in PREFIX_T) + ("prefix_whole", "single", "pair", "disjoint", "flat", "shuffled", "nan_unused")
STRIDE = tuple(f"stride_{t}" for t in STRIDE_T) + ("stride_tail",)      # stride_tail: `_tail_variant`
NAMES = SMALL + STRIDE

_CACHE = {}


def referenced(cells):
    return np.unique(np.asarray(cells, np.int64))


def unreferenced(points, cells):
    return np.setdiff1d(np.arange(len(points)), referenced(cells))


def cases(scenes):
    """name -> (points float32 [V,3], cells int32 [T,4]); every mesh is generated once per session"""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = {}
    pts, cells = scenes.random_mesh(400, 3)           # 2,387 tets with the Qhull this was written with
    pts, cells = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(cells, np.int32)
    assert len(cells) > max(PREFIX_T), len(cells)
    for t in PREFIX_T:
        out[f"prefix_{t}"] = (pts, np.ascontiguousarray(cells[:t]))
    out["prefix_whole"] = (pts, cells)                # the whole, convex mesh: no unreferenced vertex
    unit = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    out["single"] = (0.1 + 0.8 * unit, np.array([[0, 1, 2, 3]], np.int32))
    out["pair"] = (np.concatenate([0.1 + 0.6 * unit, [[0.8, 0.7, 0.9]]]).astype(np.float32), np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int32))
    out["disjoint"] = (np.concatenate([0.1 + 0.3 * unit, 0.6 + 0.3 * unit]).astype(np.float32), np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32))
    out["flat"] = (np.array([[0.1, 0.1, 0], [0.9, 0.2, 0], [0.3, 0.8, 0], [0.7, 0.9, 0]], np.float32), np.array([[0, 1, 2, 3]], np.int32))
    rng = np.random.default_rng(257)
    c = cells[:257][rng.permutation(257)]
    rot = rng.integers(0, 4, 257)
    c = np.stack([np.roll(row, int(r)) for row, r in zip(c, rot)])      # (a rotation by 1 or 3 is odd: the orientation flips too)
    out["shuffled"] = (pts, np.ascontiguousarray(c, np.int32))
    p = pts.copy()
    unused = unreferenced(pts, cells[:65])
    assert len(unused) >= 1
    p[unused] = np.nan
    out["nan_unused"] = (p, np.ascontiguousarray(cells[:65]))
    big_pts, big_cells = scenes.random_mesh(10500, 3)  # 69,559 tets with the Qhull this was written with
    big_pts, big_cells = np.ascontiguousarray(big_pts, np.float32), np.ascontiguousarray(big_cells, np.int32)
    assert len(big_cells) >= 65537, len(big_cells)
    for t in STRIDE_T:
        sub = np.ascontiguousarray(big_cells[:t])
        assert len(unreferenced(big_pts, sub)) >= 1, f"stride_{t}: every vertex is referenced"
        out[f"stride_{t}"] = (big_pts, sub)
    a, c, b = _tail_variant(*out["stride_65536"])
    out["stride_tail"] = (a, c)
    _CACHE["moved stride_tail"] = b
    assert tuple(out) == NAMES
    _CACHE["cases"] = out
    return out


def zeroed_unused(points, cells):
    """the same mesh with every vertex that no cell references set to 0"""
    p = np.array(points, np.float32)
    p[unreferenced(points, cells)] = 0.0
    return p


# ---------------------------------------------------------------------------------------------------------------- topology
_FACES = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))


def face_counts(cells):
    """(F, hull faces) of a mesh, from the sorted vertex triples"""
    c = np.asarray(cells, np.int64)
    tri = np.sort(np.concatenate([c[:, f] for f in _FACES], 0), axis=1)
    _, count = np.unique(tri, axis=0, return_counts=True)
    assert count.max() <= 2
    return len(count), int(np.count_nonzero(count == 1))


def leaf_counts(n, leaf_w):
    """build_bin_topology (csrc/tn_mesh.cpp) restated: the face counts of the leaves of the median-split tree over n faces,
    in position order; a range of count > leaf_w splits into count // 2 and the rest"""
    if n <= leaf_w:
        return [n] if n else []
    return leaf_counts(n // 2, leaf_w) + leaf_counts(n - n // 2, leaf_w)


def split_rounds(n, leaf_w):
    r = 0
    while n > leaf_w:
        n, r = n - n // 2, r + 1
    return r


def wide_levels(child):
    """levels of 64-wide nodes of a child table uint32 [n_wide, 64] (table 5; children have larger indices than their parent)"""
    child = np.asarray(child).reshape(-1, 64)
    depth = np.ones(len(child), np.int64)
    for w in range(len(child)):
        for ch in child[w]:
            if ch != 0xFFFFFFFF and not (int(ch) >> 31):
                depth[int(ch)] = depth[w] + 1
    return int(depth.max())


def classes(table):
    """table: rows {case, T, F, hull, leaf_w -> (leaves, wide_nodes, wide_levels)} (the emulation's OK lines).  Returns
    class name -> the cases that meet it; test_build_edge_cases.py asserts that none is empty."""
    out = {}
    for lw in LEAF_WIDTHS:
        out[f"F <= {lw} (the root is a leaf, no split round)"] = [r["case"] for r in table if r["F"] <= lw]
        out[f"F in ({lw}, {2 * lw}] (exactly one split round at leaf width {lw})"] = [r["case"] for r in table if lw < r["F"] <= 2 * lw]
        for levels in (1, 2, 3):
            out[f"{levels} level(s) of wide nodes at leaf width {lw}"] = [r["case"] for r in table if r[lw][2] == levels]
    out["4T < 256 (one partly filled block)"] = [r["case"] for r in table if 4 * r["T"] < 256]
    out["4T a multiple of 256"] = [r["case"] for r in table if 4 * r["T"] % 256 == 0]
    out["T not a multiple of 64, T > 64 (k_tet_bounds: full waves and a partly filled one)"] = [r["case"] for r in table if r["T"] > 64 and r["T"] % 64]
    out["F not a multiple of 64, F > 64 (k_seg_bounds: inactive tail lanes)"] = [r["case"] for r in table if r["F"] > 64 and r["F"] % 64]
    out["4T > the grid cap of k_refit_records"] = [r["case"] for r in table if 4 * r["T"] > REFIT_GRID_LANES]
    out["4T = the grid cap of k_refit_records"] = [r["case"] for r in table if 4 * r["T"] == REFIT_GRID_LANES]
    out["an unreferenced vertex"] = [r["case"] for r in table if r["unused"] > 0]
    return out


def format_table(table):
    lines = ["case             T       F    hull  unused | (leaves, wide nodes, wide levels) at leaf width 16 / 32 / 64"]
    for r in table:
        lines.append(f"{r['case']:<14}{r['T']:>6}{r['F']:>8}{r['hull']:>8}{r['unused']:>8} | " +
                     " / ".join(f"{r[lw][0]:>5} {r[lw][1]:>4} {r[lw][2]}" for lw in LEAF_WIDTHS))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- the move
def moved(points, cells, scale=0.1, seed=11):
    """float32 [V,3]: refit_cases.moved for meshes with unreferenced (and NaN) vertices and without interior ones.  Every vertex
    goes through the same affine map (an unreferenced vertex stays unreferenced, a NaN stays NaN); interior vertices -- referenced
    and on no hull face -- first move by a tenth of the smallest height over their star.  Asserted in float64: no tetrahedron's
    signed volume changes sign."""
    pts = np.asarray(points, np.float32)
    rng = np.random.default_rng(seed)
    step = np.zeros(len(pts))
    ref = referenced(cells)
    step[ref] = scale * star_min_height(pts, cells)[ref]        # over referenced vertices only: no inf
    step[hull_vertices(cells)] = 0.0
    assert np.all(np.isfinite(step))
    v = rng.normal(size=pts.shape)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    out = affine(pts.astype(np.float64) + step[:, None] * v)
    before, after = signed_volumes(pts, cells), signed_volumes(out, cells)
    flips = int(np.count_nonzero(before * after < 0))
    assert flips == 0, f"{flips} tetrahedra changed orientation: the moved mesh overlaps itself"
    assert np.all(np.isfinite(out[ref])) and not np.array_equal(out[ref], pts[ref])
    un = unreferenced(pts, cells)
    assert np.array_equal(np.isnan(out[un]), np.isnan(pts[un]))
    return np.ascontiguousarray(out)


TAIL_B = np.array([[-40.0, -50.0, 70.0], [-40.0, 60.0, 70.0], [50.0, -50.0, 70.0], [-40.0, -50.0, -60.0]], np.float32)


def _tail_variant(pts, cells):
    """(A, cells, B) of `stride_tail`, from the points and cells of stride_65536: the variant of stride_65537 whose refit reductions come from the second grid-stride trip
    of k_refit_records ALONE.  No vertex of the tetrahedra that end the kept (Morton) order of stride_65537 can be moved out of
    the mesh without a flip (they are interior), so the variant brings its own last tetrahedron: the first 65,536 cells plus one
    small tetrahedron on four unreferenced vertices, placed beyond the (1, 1, 1) corner in A -- its centroid is the largest on
    every axis, so its Morton code is the largest and its four records are 262,144 ... 262,147 (the GPU test reads the tet-id
    word of those records to assert it).  In B = moved(A) its vertices go to TAIL_B: a large tetrahedron beside the mesh (it does
    not contain the mesh: asserted) that holds max |coordinate| and spans the box of the referenced vertices on all six sides."""
    un = unreferenced(pts, cells)[:4]
    assert len(un) == 4
    a = pts.copy()
    a[un] = np.float32(1.2) + np.float32(0.1) * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    c = np.ascontiguousarray(np.concatenate([cells, un[None].astype(np.int32)]))
    assert len(c) == 65537 and 4 * len(c) - REFIT_GRID_LANES == 4
    cen = a[c.astype(np.int64)].astype(np.float64).mean(1)
    assert np.all(cen[-1] > cen[:-1].max(0))
    b = moved(a, c)
    b[un] = TAIL_B
    before, after = signed_volumes(a, c), signed_volumes(b, c)
    assert np.count_nonzero(before * after < 0) == 0 and after[-1] != 0
    ref = referenced(c)
    rest = np.setdiff1d(ref, un)
    # barycentric coordinates of the rest of the mesh in the large tetrahedron: none inside
    t = TAIL_B.astype(np.float64)
    w = np.linalg.solve((t[1:] - t[0]).T, (b[rest].astype(np.float64) - t[0]).T).T
    assert not np.any((w.min(1) >= 0) & (w.sum(1) <= 1)), "the large tetrahedron contains a vertex of the mesh"
    q = b[ref]
    assert np.abs(q).max() == np.abs(TAIL_B).max() and np.abs(b[rest]).max() < 10
    assert np.array_equal(q.min(0), TAIL_B.min(0)) and np.array_equal(q.max(0), TAIL_B.max(0))
    assert np.all(b[rest].min(0) > TAIL_B.min(0)) and np.all(b[rest].max(0) < TAIL_B.max(0))
    return a, c, np.ascontiguousarray(b)


def case_ab(scenes, name):
    """(A, B, cells) of a case: the loaded vertices, the moved ones (`moved`; stride_tail: its own B), made once per session"""
    a, cells = cases(scenes)[name]
    key = f"moved {name}"
    if key not in _CACHE:
        _CACHE[key] = moved(a, cells)
    return a, _CACHE[key], cells


# ---------------------------------------------------------------------------------------------------------------- rays
def ref_box(points, cells):
    q = np.asarray(points, np.float32)[referenced(cells)]
    return q.min(0), q.max(0)


def aimed_rays(points, cells, n, seed):
    """(origins, directions) float32 [n,3]: origins on a sphere around the box of the referenced vertices (radius 1.5 x the box
    diagonal + 0.5, seeded directions), each ray aimed at a seeded Dirichlet(1,1,1,1) point of a seeded tetrahedron of `cells`.
    The condition the tests rely on (asserted on the oracle by tests/test_build_edge_cases.py): the oracle reports a hit on at
    least 90 % of them, on every case but `flat`."""
    rng = np.random.default_rng(seed)
    lo, hi = ref_box(points, cells)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    centre, radius = 0.5 * (lo + hi), 1.5 * np.linalg.norm(hi - lo) + 0.5
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    o = centre + radius * v
    tet = rng.integers(0, len(cells), n)
    w = rng.dirichlet((1.0, 1.0, 1.0, 1.0), n)
    target = (np.asarray(points, np.float64)[np.asarray(cells, np.int64)[tet]] * w[..., None]).sum(1)
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.ascontiguousarray(o.astype(np.float32)), np.ascontiguousarray(d.astype(np.float32))


def locate_points(points, cells, n, seed):
    """n points in the referenced box scaled by 1.2 about its centre, the referenced vertices, the centroids of the first 64 tets"""
    rng = np.random.default_rng(seed)
    lo, hi = ref_box(points, cells)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    q = 0.5 * (lo + hi) + 1.2 * (rng.random((n, 3)) - 0.5) * (hi - lo)
    p = np.asarray(points, np.float32)
    cen = p[np.asarray(cells, np.int64)[:64]].astype(np.float64).mean(1)
    return np.ascontiguousarray(np.concatenate([q, p[referenced(cells)], cen]).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the tree
def final_face_order(leaf_id):
    """Leaf rows are in position order in both builds: the device build numbers its leaves from the last frontier
    (build_bin_topology, csrc/tn_mesh.cpp), the host build (build_wide_bvh) numbers them in the pre-order of a recursion that
    descends into the lower half first.  So the ids of the rows, concatenated, are the final face order."""
    rows = [row[row != 0xFFFFFFFF] for row in np.asarray(leaf_id)]
    return np.concatenate(rows).astype(np.int64), [len(r) for r in rows]


def check_median_splits(faces, leaf_id, points, leaf_w):
    """What the build promises of the face BVH, stated plainly: the final face order (the leaf rows of `leaf_id` [n_leaves,
    leaf_w], 0xFFFFFFFF = empty slot) is the order of a median-split tree.  Recursing as build_bin_topology does, every range of
    count > leaf_w splits into count // 2 and the rest, along the axis core::split_axis takes from the float32 bounds of the
    float32 centroids ((a + b + c) * (1.0f / 3.0f) on the stored triple, core::face_box): widest extent, ties to the lower
    axis; no centroid of the lower part may lie above one of the upper part on that axis.  Ties cannot fail this.  The leaf
    counts of the restated tree must be the row occupancies.  Returns the number of split ranges checked."""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    order, occupancy = final_face_order(np.asarray(leaf_id).reshape(-1, leaf_w))
    F = len(faces)
    assert len(order) == F and np.array_equal(np.sort(order), np.arange(F)), "the leaf rows are not a permutation of the faces"
    assert occupancy == leaf_counts(F, leaf_w), "the row occupancies are not the leaf counts of the median-split tree"
    p = np.asarray(points, np.float32)
    third = np.float32(1.0) / np.float32(3.0)
    tri = p[faces]
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * third
    assert cen.dtype == np.float32
    cen = cen[order]
    checked, todo = 0, [(0, F)]
    while todo:
        first, count = todo.pop()
        if count <= leaf_w:
            continue
        c = cen[first:first + count]
        ext = c.max(0) - c.min(0)                     # float32, as split_axis computes it
        ax = 0
        if ext[1] > ext[ax]:
            ax = 1
        if ext[2] > ext[ax]:
            ax = 2
        half = count // 2
        left, right = c[:half, ax].max(), c[half:, ax].min()
        assert left <= right, (f"range [{first}, {first + count}) is not split at the median of axis {ax}: "
                               f"max of the lower part {left} > min of the upper part {right}")
        checked += 1
        todo += [(first, half), (first + half, count - half)]
    return checked
