"""The vertex move every refit test uses (tests/test_refit.py, tests/test_refit_gpu.py), stated once.

Interior vertices (those on no hull face) move in a random direction by 0.1 x the smallest tet height over their star; then
every vertex is mapped by x -> A x + b.  The affine map keeps the hull convex and changes max |coordinate|, the mesh box and
every Morton code; the interior move changes the shape of every tetrahedron that has an interior vertex.  `moved` asserts in
float64 that no tetrahedron's signed volume changes sign, i.e. that the moved mesh is still a non-overlapping one (what the
walk's certification assumes of any mesh, freshly loaded or refitted)."""
import numpy as np

AFFINE_A = np.array([[1.3, 0.2, 0.0], [-0.1, 0.9, 0.3], [0.05, -0.2, 1.6]])     # det 1.985
AFFINE_B = np.array([0.7, -1.1, 2.3])

_FACES = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))      # local face k is opposite local vertex k


def meshes(scenes):
    """name -> (points, cells): the four meshes of the refit checks"""
    return {
        "random_1500": scenes.random_mesh(1500, 1),
        "grid_12_jitter": scenes.grid_mesh(12, 0.2),
        "grid_16": scenes.grid_mesh(16),          # 2,700 hull faces: the threaded hull tree; thousands of zero-volume tets
        "cube": scenes.cube_mesh(),               # one interior vertex
    }


def signed_volumes(pts, cells):
    p = np.asarray(pts, np.float64)[np.asarray(cells, np.int64)]
    return np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])


def hull_vertices(cells):
    c = np.asarray(cells, np.int64)
    tri = np.sort(np.concatenate([c[:, f] for f in _FACES], 0), axis=1)
    uniq, count = np.unique(tri, axis=0, return_counts=True)
    return np.unique(uniq[count == 1])


def star_min_height(pts, cells):
    """per vertex: the smallest height of any tetrahedron around it (0 next to a zero-volume tetrahedron)"""
    p = np.asarray(pts, np.float64)[np.asarray(cells, np.int64)]
    vol6 = np.abs(signed_volumes(pts, cells))
    h = np.full(len(cells), np.inf)
    for f in _FACES:
        area2 = np.linalg.norm(np.cross(p[:, f[1]] - p[:, f[0]], p[:, f[2]] - p[:, f[0]]), axis=1)
        h = np.minimum(h, np.where(area2 > 0, vol6 / np.where(area2 > 0, area2, 1.0), 0.0))
    out = np.full(len(pts), np.inf)
    np.minimum.at(out, np.asarray(cells, np.int64).reshape(-1), np.repeat(h, 4))
    return out


def affine(x):
    return (np.asarray(x, np.float64) @ AFFINE_A.T + AFFINE_B).astype(np.float32)


def affine_dirs(d):
    v = np.asarray(d, np.float64) @ AFFINE_A.T
    return np.ascontiguousarray((v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32))


def moved(pts, cells, scale=0.1, seed=11):
    """float32 [V,3]: the vertices after the move (same cells)"""
    pts = np.asarray(pts, np.float32)
    rng = np.random.default_rng(seed)
    step = scale * star_min_height(pts, cells)
    step[hull_vertices(cells)] = 0.0
    v = rng.normal(size=pts.shape)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    out = affine(pts.astype(np.float64) + step[:, None] * v)
    before, after = signed_volumes(pts, cells), signed_volumes(out, cells)     # det A > 0: the map keeps the sign
    flips = int(np.count_nonzero(before * after < 0))
    assert flips == 0, f"{flips} tetrahedra changed orientation: the moved mesh overlaps itself"
    assert step.max() > 0 and not np.array_equal(out, pts)
    return np.ascontiguousarray(out)
