"""Sizes, inputs, float64 references and error bounds of the tests of k_sample_positions_bwd (csrc/tn_position_grad.hip), part (B)
of the position gradients: tests/test_position_grad_edges_gpu.py uploads the cases, tests/test_position_grad_cases.py holds the
torch statement (geometry.sample_positions_backward) and the cases themselves to the references below, so that a failure on the
GPU is not the test's own error.  tests/test_position_gradients_gpu.py takes its reference and bound helpers from here too.
No kernel runs here and the library is not loaded.

THE LAUNCHER, restated (test_position_grad_cases.py reads the three numbers back from the source): one wavefront owns a ray,
RAYS_PER_BLOCK = 4 wavefronts per block, at most MAX_BLOCKS = 8192 blocks, so IN_FLIGHT = 32,768 rays per trip of the ray loop; the
lane is the sample in chunks of CHUNK = 64, a lane adding samples lane, lane + 64, ... before a butterfly sum.  `loop_model` states
which (ray, sample) each (wave, trip, chunk, lane) visits.

THE LIVENESS RULE: a sample with an id that is EMPTY or >= V, a zero determinant or a non-finite m contributes exact zeros to every
output; an id-dead sample does so whatever its barycentrics, distance and gradient hold.  In float64 "non-finite m" has to name the
float32 range: the reference calls a sample dead when max |m64| >= 2^128, and the cases keep every sample out of
2^110 <= max |m64| <= 2^148 (`check_gap`), so that no rounding of the code under test can change which side a sample is on.

TWO FILLS.  `exact`: integer vertex coordinates in [-8, 8]; every tetrahedron is x0, x0 + s_k 2^a_k axis(pi(k)) (s_k = +-1, a_k in
{0, 1, 2}, pi a permutation of the axes), so T is a signed, scaled permutation and det = +- a power of two; g integers in [-4, 4]
derived from (ray, sample), no two samples of a ray alike; barycentrics multiples of 1/8 in [-1/8, 1]; t multiples of 1/4 in [0, 16].
Then m has at most two fractional bits, every term -w_k m is a multiple of 1/32 and t m of 1/16, and every partial sum is exact in
fp32 while 32 sum |terms| < 2^24 (`exactness_margin`): the correct result has ONE bit pattern, whatever the order of the additions.
`random`: cells of scenes.random_mesh(1500, 1), barycentrics inside the cell, g ~ N(0, 1), t increasing along the ray; bounds
(u = 2^-24), all a priori, none with exclusions:
  per sample  ||m32 - m64|| <= 8 u cond2(T) ||m64||     the backward error of a 3 x 3 solve in fp32 (m64: a float64 solve on the
              kernel's own fp32 inputs);
  sums        the per-sample bounds times |w_k| (vertices), 1 (origins), |t| (directions), plus n_terms u sum |terms| for the fp32
              summation of n_terms terms in any order.  The weights are the forward's own fp32 bits, w0 = 1 - ((b0 + b1) + b2).

DEAD CLASSES, mixed into every case of both fills at about 1/16 each (seeded), present at least once from R S >= 64 on:
  1 ALL_EMPTY     four EMPTY ids                      2 ONE_EMPTY   one EMPTY id, in each of the four slots
  3 OUT_OF_RANGE  one id V, V + 5 or 0x7FFFFFFF       4 FLAT        det exactly 0: a flat quadruple of integer vertices, a repeated id
  5 NONFINITE     g = +inf / -inf / NaN, or a tetrahedron with an edge of 2^-149 so that |m64| >= 2^149 for |g| >= 1
  (6) poison      NaN barycentrics, NaN t and NaN g on every other id-dead sample (classes 1-3), the first of each class included
  CONTROL         LIVE: the tetrahedron 0, 2^-100 x, y, z, where m_x = 2^100 g_0 must come through (exactly in the exact fill, where
                  it only appears on a ray of its own: 2^100 g_0 plus small integers is not exact).
"""
import functools

import numpy as np
import torch

from gather_cases import weights32

U = 2.0 ** -24
RAYS_PER_BLOCK = 4
CHUNK = 64
MAX_BLOCKS = 8192
IN_FLIGHT = RAYS_PER_BLOCK * MAX_BLOCKS

S_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 257)
R_SMALL = (1, 3, 4, 5, 9)
R_EDGES = (1, 3, 4, 5, 32767, 32768, 32769, 65537)
S_AT_R_EDGES = (1, 3)
EDGE_SHAPES = sorted({(R, S) for S in S_EDGES for R in R_SMALL} | {(R, S) for R in R_EDGES for S in S_AT_R_EDGES})
RANDOM_SHAPES = [(R, S) for S in S_EDGES for R in (5, 300)]
ONE_TET_SHAPE = (157, 127)            # 19,939 samples in ONE tetrahedron: every vertex atomic lands on 12 addresses
CLASS_RAY_S = (1, 65, 129)
CHAIN_S = (1, 65)

LIVE, ALL_EMPTY, ONE_EMPTY, OUT_OF_RANGE, FLAT, NONFINITE, CONTROL = 0, 1, 2, 3, 4, 5, 6
DEAD_CLASSES = (ALL_EMPTY, ONE_EMPTY, OUT_OF_RANGE, FLAT, NONFINITE)
ID_DEAD = (ALL_EMPTY, ONE_EMPTY, OUT_OF_RANGE)
# rays of the class-ray case: a live ray between two all-dead rays, one ray made entirely of each class, the control, a mixed ray
CLASS_RAYS = (ALL_EMPTY, LIVE, ONE_EMPTY, OUT_OF_RANGE, FLAT, NONFINITE, CONTROL, None)
F32_RANGE = 2.0 ** 128
GAP = (2.0 ** 110, 2.0 ** 148)
TINY = 2.0 ** -149

# rows appended to every vertex table, each quadruple with rows of its own: only samples of that class name them
_SPECIAL = dict(
    flat=[(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)],                          # four coplanar points, all different
    spare=[(2, 1, 0), (3, 1, 2), (1, -2, 1), (0, 3, 1)],                        # a healthy tetrahedron, named with a repeated id
    tiny=[(0, 0, 0), (TINY, 0, 0), (0, TINY, 0), (0, 0, TINY)],                 # m64 = 2^149 g
    needle=[(0, 0, 0), (TINY, 0, 0), (0, 2.0 ** 60, 0), (0, 0, 2.0 ** 60)],     # m64_x = 2^149 g_0, det32 = 2^-29 or 0
    control=[(0, 0, 0), (2.0 ** -100, 0, 0), (0, 1, 0), (0, 0, 1)],             # LIVE: m = (2^100 g_0, g_1, g_2)
)


# ---- the kernel's loops ----------------------------------------------------------------------------------------------------
def launch(R):
    """(grid, waves) of launch_sample_positions_backward"""
    grid = min(-(-R // RAYS_PER_BLOCK), MAX_BLOCKS)
    return grid, grid * RAYS_PER_BLOCK


def trips(R):
    """how many rays wave 0 takes"""
    return -(-R // launch(R)[1])


def loop_model(R, S, whole_chunks_only=False, stride_off=0, ray_end_off=0):
    """Which (ray, sample) the loops of k_sample_positions_bwd visit:
        for (r = wave0; r < R; r += nwaves)  for (s0 = 0; s0 < S; s0 += 64)  { s = s0 + lane; if (s >= S) continue; ... }
    -> visits int [R, S] (how often each sample is taken), lane int [R, S] (the lane whose sum it lands in, -1: none),
    writers int [R] (how many waves write the ray's two rows).  The three keywords make the MODEL wrong the way a slip in the
    kernel would: `s0 + 64 <= S`, a stride of nwaves + stride_off, `r < R + ray_end_off`."""
    nwaves = launch(R)[1]
    visits = np.zeros((R, S), np.int64)
    lane = np.full((R, S), -1, np.int64)
    writers = np.zeros(R, np.int64)
    lanes = np.arange(CHUNK)
    r = np.arange(nwaves)                 # wave0 = block * RAYS_PER_BLOCK + wave in block
    while True:
        rr = r[r < R + ray_end_off]
        if len(rr) == 0:
            break
        s0 = 0
        while (s0 + CHUNK <= S) if whole_chunks_only else (s0 < S):
            s = s0 + lanes
            ok = s < S
            np.add.at(visits, (rr[:, None], s[ok][None, :]), 1)
            lane[rr[:, None], s[ok][None, :]] = lanes[ok][None, :]
            s0 += CHUNK
        np.add.at(writers, rr, 1)
        r = r + (nwaves + stride_off)
    return visits, lane, writers


# ---- references and bounds (torch, any device; shared with tests/test_position_gradients_gpu.py) -----------------------------
def ids_in_table(vi, V):
    """vi integer [..., 4] (EMPTY = -1 as int32) -> (int64 ids with 0 where the id is not in [0, V), bool `present` [...])"""
    ids = vi.long()
    ok = (ids >= 0) & (ids < V)
    return torch.where(ok, ids, torch.zeros_like(ids)), ok.all(-1)


def m64_and_cond(vi, verts, grad_bary, present=None):
    """float64 solve T m = g on the fp32 inputs and cond2(T), on the CPU, for the samples in `present` (default: those whose four
    ids are in the table); -> (m64 [n,3] (zeros elsewhere), cond [n] (1 elsewhere), present [n]) on grad_bary's device."""
    dev = grad_bary.device
    V = verts.shape[0]
    ids, in_table = ids_in_table(vi.reshape(-1, 4).cpu(), V)
    present = in_table if present is None else present.reshape(-1).cpu()
    n = ids.shape[0]
    m64 = torch.zeros(n, 3, dtype=torch.float64)
    cond = torch.ones(n, dtype=torch.float64)
    if bool(present.any()):
        v64 = verts.cpu().double()
        x = v64[ids[present]]
        T = x[:, 1:] - x[:, :1]
        g = grad_bary.reshape(-1, 3).cpu().double()[present]
        m64[present] = torch.linalg.solve(T, g.unsqueeze(-1)).squeeze(-1)
        uniq, inv = torch.unique(ids[present], dim=0, return_inverse=True)
        xu = v64[uniq]
        sv = torch.linalg.svdvals(xu[:, 1:] - xu[:, :1])
        cond[present] = (sv[:, 0] / sv[:, -1])[inv]
    return m64.to(dev), cond.to(dev), present.to(dev)


def sample_bound(cond, m64):
    """8 u cond2(T) ||m64|| per sample"""
    return 8 * U * cond * m64.norm(dim=-1)


def sums_and_bounds(vi, weights, m64, bound_s, live, t, R, S, V):
    """The float64 sums over w32_k m64 (vertices), m64 (origins) and t m64 (directions) of the `live` samples, and their bounds
    (module docstring).  vi [n, 4] or [R, S, 4]; weights [n, 4]: the forward's own fp32 weights; t [n] or [R, S] or None.
    What a sample that is not live holds is never multiplied in.  -> dict want_v / bound_v [V, 3], want_o / bound_o [R, 3],
    want_d / bound_d [R, 3] (with t), count_v [V] (live samples naming the vertex)."""
    dev = m64.device
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    live = live.reshape(-1).to(dev)
    ids = ids_in_table(vi.reshape(-1, 4).to(dev), V)[0].reshape(-1)
    w = torch.where(live[:, None], weights.to(dev).double(), zero)
    m = torch.where(live[:, None], m64, zero)
    bs = torch.where(live, bound_s, zero)
    lv = live.double()

    def at_vertices(rows):
        return torch.zeros((V,) + tuple(rows.shape[2:]), dtype=torch.float64, device=dev).index_add_(0, ids, rows.flatten(0, 1))

    terms = -(w[:, :, None] * m[:, None, :])                                             # [n, 4, 3]
    out = dict(want_v=at_vertices(terms), count_v=at_vertices(lv[:, None].expand(-1, 4)))
    out["bound_v"] = at_vertices(w.abs() * bs[:, None])[:, None] + out["count_v"][:, None] * U * at_vertices(terms.abs())
    n_live = lv.reshape(R, S).sum(1)[:, None]
    out["want_o"] = m.reshape(R, S, 3).sum(1)
    out["bound_o"] = bs.reshape(R, S).sum(1)[:, None] + n_live * U * m.abs().reshape(R, S, 3).sum(1)
    if t is not None:
        tt = torch.where(live, t.reshape(-1).to(dev).double(), zero)
        tm = tt[:, None] * m
        out["want_d"] = tm.reshape(R, S, 3).sum(1)
        out["bound_d"] = (tt.abs() * bs).reshape(R, S).sum(1)[:, None] + n_live * U * tm.abs().reshape(R, S, 3).sum(1)
    return out


def closed_form64(vi, verts, grad_bary):
    """The closed form of m in float64 on the fp32 inputs, for the liveness rule -> (m [n, 3] (nan / inf where it is), det [n],
    in_table [n]); numpy."""
    V = len(verts)
    ids = vi.reshape(-1, 4).astype(np.int64)
    ok = (ids >= 0) & (ids < V)
    x = verts.astype(np.float64)[np.where(ok, ids, 0)]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    det = (e1 * c23).sum(1)
    g = grad_bary.reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        m = (g[:, 0:1] * c23 + g[:, 1:2] * c31 + g[:, 2:3] * c12) / det[:, None]
    return m, det, ok.all(1)


def liveness64(vi, verts, grad_bary):
    """-> (live bool [n], largest |m64| per sample with 0 where m is not finite or the sample has no tetrahedron)"""
    m, det, in_table = closed_form64(vi, verts, grad_bary)
    finite = np.isfinite(m).all(1)
    size = np.where(finite & in_table & (det != 0), np.abs(np.where(np.isfinite(m), m, 0.0)).max(1), 0.0)
    return in_table & (det != 0) & finite & (size < F32_RANGE), size


def check_gap(size):
    return not bool(((size >= GAP[0]) & (size <= GAP[1])).any())


def reference(c, bounds):
    """float64 reference of a case `c` (numpy arrays): points, origins, directions, vertices, live, named (vertices that a live
    sample names); with `bounds` also bound_points [n], bound_o, bound_d, bound_v."""
    R, S, V = c["R"], c["S"], c["V"]
    live_np, size = liveness64(c["vi"], c["verts"], c["gb"])
    live = torch.from_numpy(live_np)
    vi, verts, gb = (torch.from_numpy(np.array(c[k])) for k in ("vi", "verts", "gb"))
    m64, cond, _ = m64_and_cond(vi, verts, gb, present=live)
    if not bounds:
        cond = torch.ones_like(cond)
    bs = sample_bound(cond, m64)
    w = torch.from_numpy(weights32(c["bc"].reshape(-1, 3)))
    s = sums_and_bounds(vi, w, m64, bs, live, torch.from_numpy(np.array(c["t"])), R, S, V)
    out = dict(points=m64.reshape(R, S, 3), origins=s["want_o"], directions=s["want_d"], vertices=s["want_v"],
               live=live.reshape(R, S), named=s["count_v"] > 0, size=torch.from_numpy(size))
    if bounds:
        out.update(bound_points=bs.reshape(R, S), bound_o=s["bound_o"], bound_d=s["bound_d"], bound_v=s["bound_v"], cond=cond)
    return out


def exactness_margin(c, ref):
    """the largest 32 sum |terms| over all outputs of an exact case, in units of 2^24 (< 1: every partial sum of multiples of
    1/32 is exact in fp32 in any order).  The control's m_x = 2^100 g_0 is counted as g_0: it shares no sum with another scale."""
    live = ref["live"].reshape(-1)
    m = ref["points"].reshape(-1, 3).abs().clone()
    m[torch.from_numpy(c["cls"].reshape(-1) == CONTROL), 0] *= 2.0 ** -100
    one = torch.ones_like(m[:, 0])
    s = sums_and_bounds(torch.from_numpy(np.array(c["vi"])), torch.from_numpy(weights32(c["bc"].reshape(-1, 3))).abs().neg(), m, one,
                        live, torch.from_numpy(np.array(c["t"])).abs(), c["R"], c["S"], c["V"])
    return 32 * max(float(s["want_v"].abs().max()), float(s["want_o"].abs().max()), float(s["want_d"].abs().max())) / 2.0 ** 24


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _exact_mesh(rng, ntets):
    """-> verts float64 [4 ntets, 3] integers in [-8, 8], cells int64 [ntets, 4]; the rows of the table are shuffled"""
    x0 = rng.integers(-4, 5, (ntets, 3)).astype(np.float64)
    a = rng.integers(0, 3, (ntets, 3))
    sgn = rng.choice([-1.0, 1.0], (ntets, 3))
    perm = rng.permuted(np.tile(np.arange(3), (ntets, 1)), axis=1)
    x = np.repeat(x0[:, None, :], 4, axis=1)
    for k in range(3):
        x[np.arange(ntets), k + 1, perm[:, k]] += sgn[:, k] * 2.0 ** a[:, k]
    row = rng.permutation(4 * ntets)
    verts = np.zeros((4 * ntets, 3))
    verts[row] = x.reshape(-1, 3)
    return verts, row.reshape(ntets, 4)


@functools.lru_cache(maxsize=None)
def _mesh(fill, ntets):
    """-> verts float32 [V, 3] (the special rows last), cells int64 [T, 4], special: name -> int64 [4] ids"""
    if fill == "exact":
        verts, cells = _exact_mesh(np.random.default_rng([7, ntets]), ntets)
    else:
        import importlib

        pts, cells = importlib.import_module("tetra-nerf_amd.scenes").random_mesh(1500, 1)
        verts, cells = pts.astype(np.float64), cells.astype(np.int64)
    special, rows = {}, [verts]
    V = len(verts)
    for name, quad in _SPECIAL.items():
        special[name] = np.arange(V, V + 4)
        rows.append(np.asarray(quad, np.float64))
        V += 4
    verts = np.concatenate(rows).astype(np.float32)
    assert np.array_equal(verts.astype(np.float64), np.concatenate(rows))        # (2^-149, 2^60 and 2^-100 are fp32 numbers)
    return verts, cells, special


def draw_classes(rng, n):
    """int8 [n]: each dead class with probability 1/16; from n >= 64 on every class at least once; at least half live (a small n
    whose draw says otherwise gets its last dead samples back)"""
    u = rng.random(n)
    cls = np.where(u < len(DEAD_CLASSES) / 16, np.floor(u * 16).astype(np.int64) + 1, LIVE)
    if n >= 64:
        cls[rng.permutation(n)[:len(DEAD_CLASSES)]] = DEAD_CLASSES
    dead = np.flatnonzero(cls != LIVE)
    cls[dead[len(dead) - max(0, len(dead) - n // 2):]] = LIVE
    return cls.astype(np.int8)


def _assemble(rng, fill, cls, ntets):
    verts, cells, special = _mesh(fill, ntets)
    R, S = cls.shape
    n, V = R * S, len(verts)
    c = cls.reshape(-1)
    vi = cells[rng.integers(0, len(cells), n)].copy()
    if fill == "exact":
        r, s = np.divmod(np.arange(n), S)
        k = (37 * r + s) % 729                       # three base-9 digits: no two samples of a ray (S < 729) share a g
        gb = (np.stack([k % 9, (k // 9) % 9, k // 81], 1) - 4).astype(np.float32)
        bc = (rng.integers(-1, 9, (n, 3)) / 8).astype(np.float32)
        t = (rng.integers(0, 65, (R, S)) / 4).astype(np.float32)
    else:
        gb = rng.standard_normal((n, 3)).astype(np.float32)
        bc = rng.dirichlet(np.ones(4), n)[:, 1:].astype(np.float32)
        t = np.cumsum(0.05 + 0.5 * rng.random((R, S)), axis=1).astype(np.float32)
    t = t.reshape(-1)

    def members(k):
        return np.flatnonzero(c == k)

    vi[members(ALL_EMPTY)] = -1
    for j, i in enumerate(members(ONE_EMPTY)):
        vi[i, j % 4] = -1
    for j, i in enumerate(members(OUT_OF_RANGE)):
        vi[i, (j // 3) % 4] = (V, V + 5, 0x7FFFFFFF)[j % 3]
    f, sp = special["flat"], special["spare"]
    flat = (f, sp[[0, 0, 1, 2]], sp[[0, 1, 2, 0]], sp[[1, 2, 2, 3]])
    for j, i in enumerate(members(FLAT)):
        vi[i] = flat[j % 4]
    for j, i in enumerate(members(NONFINITE)):
        if j % 5 < 3:
            gb[i, j % 3] = (np.inf, -np.inf, np.nan)[j % 5]
        else:
            vi[i] = special["tiny" if j % 5 == 3 else "needle"]
            gb[i] = (1 + j % 3, -(1 + j % 2), 2)           # |g_k| >= 1: |m64| >= 2^149
    vi[members(CONTROL)] = special["control"]
    for k in ID_DEAD:
        poisoned = members(k)[::2]
        bc[poisoned] = np.nan
        gb[poisoned] = np.nan
        t[poisoned] = np.nan
    case = dict(fill=fill, R=R, S=S, V=V, cls=cls, vi=vi.astype(np.int32).reshape(R, S, 4), bc=bc.reshape(R, S, 3),
                gb=gb.reshape(R, S, 3), t=t.reshape(R, S), verts=verts, special=special)
    case["ref"] = reference(case, bounds=fill == "random")
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _seed(fill, *key):
    return [11, 1 if fill == "exact" else 0] + list(key)


@functools.lru_cache(maxsize=None)
def mixed_case(fill, R, S, ntets=200):
    """R rays of S samples, the dead classes mixed in by `draw_classes`"""
    rng = np.random.default_rng(_seed(fill, 0, R, S, ntets))
    return _assemble(rng, fill, draw_classes(rng, R * S).reshape(R, S), ntets)


@functools.lru_cache(maxsize=None)
def class_ray_case(fill, S):
    """CLASS_RAYS: ray 1 is live between the all-dead rays 0 and 2; rays 0, 2, 3, 4, 5 are made entirely of one dead class each, ray
    6 of the control, ray 7 is mixed"""
    rng = np.random.default_rng(_seed(fill, 1, S))
    cls = np.stack([draw_classes(rng, S) if k is None else np.full(S, k, np.int8) for k in CLASS_RAYS])
    return _assemble(rng, fill, cls, 200)


def one_tet_case():
    """the exact fill with every live sample in ONE tetrahedron"""
    return mixed_case("exact", *ONE_TET_SHAPE, ntets=1)


def shares(c):
    """-> dict class -> number of samples, plus "live" (by the reference) and "poisoned" """
    out = {k: int((c["cls"] == k).sum()) for k in (LIVE,) + DEAD_CLASSES + (CONTROL,)}
    out["live"] = int(c["ref"]["live"].sum())
    out["poisoned"] = int(np.isnan(c["bc"]).any(-1).sum())
    return out


# ---- (A) then (B): the gather's barycentric adjoint feeding the sample-position adjoint ------------------------------------------
CHAIN_R, CHAIN_F = 37, 16


@functools.lru_cache(maxsize=None)
def chain_case(S):
    """Samples that DO sit where the forward statement puts them: rays o + t d through the unit cube, every sample in a cell of the
    random mesh (any cell: the barycentrics of a point are defined inside and outside it), bc = fl32(solve(T^T, o + t d - x0)) in
    float64 on the fp32 rays and vertices.  Dead classes ALL_EMPTY and ONE_EMPTY only, no poison (the forward gather runs on these
    ids and barycentrics).  field [F, V], G [R, S, F] ~ N(0, 1)."""
    rng = np.random.default_rng(_seed("random", 2, S))
    verts, cells, _ = _mesh("random", 200)
    R, V = CHAIN_R, len(verts)
    n = R * S
    o = rng.random((R, 3)).astype(np.float32)
    d = rng.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    t = np.cumsum(0.02 + 0.1 * rng.random((R, S)), axis=1).astype(np.float32)
    t *= np.float32(0.5) / t[:, -1:].clip(0.5)                    # the samples stay within 0.5 of the origin
    vi = cells[rng.integers(0, len(cells), n)].copy()
    p = (o.astype(np.float64)[:, None] + t.astype(np.float64)[..., None] * d.astype(np.float64)[:, None]).reshape(n, 3)
    x = verts.astype(np.float64)[vi]
    T = x[:, 1:] - x[:, :1]
    bc = np.linalg.solve(np.swapaxes(T, 1, 2), (p - x[:, 0])[..., None])[..., 0].astype(np.float32)
    cls = np.where(rng.random(n) < 1 / 8, rng.integers(1, 3, n), LIVE).astype(np.int8)
    vi[cls == ALL_EMPTY] = -1
    for j, i in enumerate(np.flatnonzero(cls == ONE_EMPTY)):
        vi[i, j % 4] = -1
    case = dict(R=R, S=S, V=V, F=CHAIN_F, cls=cls.reshape(R, S), vi=vi.astype(np.int32).reshape(R, S, 4), bc=bc.reshape(R, S, 3), t=t,
                o=o, d=d, verts=verts, field=rng.standard_normal((CHAIN_F, V)).astype(np.float32),
                G=rng.standard_normal((R, S, CHAIN_F)).astype(np.float32))
    case["ref"] = chain_reference(case)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def chain_reference(c):
    """float64 autograd of  L = sum over the live samples of G . phi,  phi = the gather statement on b = solve(T^T, o + t d - x0)
    (geometry.barycentrics_of), w.r.t. o, d and the vertex table -> origins, directions, vertices and their tolerances.

    THE TOLERANCE.  a_k = (2F + 2) u sum_c |G_c| (|F[v_{k+1},c]| + |F[v_0,c]|) bounds the error of (A)'s g_k in fp32 (the dot-product
    bound of tests/test_position_gradients_gpu.py).  (B) then solves T m = g32: ||m32 - T^-1 g32|| <= 8 u cond ||T^-1 g32|| and
    ||T^-1 (g32 - g64)|| <= ||a|| / sigma_min(T), so per sample, to first order,
        ||m32 - m64|| <= bs = 8 u cond (||m64|| + ||a|| / sigma_min) + ||a|| / sigma_min,
    and the three sums get the bounds of (B) (`sums_and_bounds`) with bs as the per-sample bound.  The vertex terms of the reference
    carry w64 = (1 - sum b64, b64) where the kernels carry the fp32 weights of bc = fl32(b64): |w32_k - w64_k| <= 4 u (1 + sum |b|)
    (the rounding of b, two additions and a subtraction), which adds 4 u (1 + sum |b|) |m64| per term."""
    R, S, V, F = c["R"], c["S"], c["V"], c["F"]
    n = R * S
    ids, live = ids_in_table(torch.from_numpy(np.array(c["vi"])).reshape(n, 4), V)
    o, d, verts = (torch.from_numpy(np.array(c[k])).double().requires_grad_(True) for k in ("o", "d", "verts"))
    t = torch.from_numpy(np.array(c["t"])).double()
    fvm = torch.from_numpy(np.array(c["field"])).double().t()
    G = torch.from_numpy(np.array(c["G"])).double().reshape(n, F)
    p = (o[:, None, :] + t[..., None] * d[:, None, :]).reshape(n, 3)[live]
    p.retain_grad()
    x = verts[ids[live]]
    T = x[:, 1:] - x[:, :1]
    b = torch.linalg.solve(T.transpose(-1, -2), (p - x[:, 0]).unsqueeze(-1)).squeeze(-1)
    rows = fvm[ids[live]]
    phi = b[:, 0:1] * rows[:, 1] + b[:, 1:2] * rows[:, 2] + b[:, 2:3] * rows[:, 3] + (1 - b.sum(-1, keepdim=True)) * rows[:, 0]
    (phi * G[live]).sum().backward()
    m64 = torch.zeros(n, 3, dtype=torch.float64)
    m64[live] = p.grad
    # the tolerance
    r = fvm[ids].abs()                                                           # live samples only are used below
    a = (2 * F + 2) * U * torch.einsum("nc,nkc->nk", G.abs(), r[:, 1:] + r[:, :1]).norm(dim=-1)
    sv = torch.linalg.svdvals(T.detach())
    smin, cond = torch.ones(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    smin[live], cond[live] = sv[:, -1], sv[:, 0] / sv[:, -1]
    bs = 8 * U * cond * (m64.norm(dim=-1) + a / smin) + a / smin
    bc = torch.from_numpy(np.array(c["bc"])).reshape(n, 3)
    w32 = torch.from_numpy(weights32(c["bc"].reshape(n, 3)))
    s = sums_and_bounds(ids, w32, m64, bs, live, torch.from_numpy(np.array(c["t"])), R, S, V)
    dw = torch.where(live, 4 * U * (1 + bc.double().abs().sum(-1)), torch.zeros(1, dtype=torch.float64))
    extra_v = torch.zeros(V, 3, dtype=torch.float64).index_add_(0, ids.reshape(-1), (dw[:, None] * m64.abs()).repeat_interleave(4, 0))
    return dict(origins=o.grad, directions=d.grad, vertices=verts.grad, live=live, bound_o=s["bound_o"], bound_d=s["bound_d"],
                bound_v=s["bound_v"] + extra_v, cond=cond)
