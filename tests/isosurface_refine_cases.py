"""The edges, densities and levels every test of the isosurface refinement uses (tests/test_isosurface_refine.py,
tests/test_isosurface_refine_gpu.py), stated once.  Nothing here needs a GPU or the library.

Two groups.  CRAFTED: N independent mesh edges (2 i, 2 i + 1), edge i following pattern i mod len(PATTERNS): its two vertex values
and, per round, the seven densities the "network" answers whatever it is asked -- so that the selection rule is driven through
every branch (a candidate equal to the level, several sign changes, NaN / inf / 2^126 candidates, both orientations, values on
one side, an id past the table).  ANALYTIC: the surfaces of the sphere cases of tests/isosurface_cases.py with the density
-(|p|^2) evaluated in float32 along the edge, for which the distance of a refined vertex from the sphere has an a-priori bound."""
import numpy as np

import isosurface_cases as ic

U = ic.U
C = 7
LEVEL = 0.125
L = np.float32(LEVEL)
NAN, INF, BIG = np.float32(np.nan), np.float32(np.inf), np.float32(2.0 ** 126)
ROUNDS = 4                            # rounds of a crafted case

# name -> (values[a], values[b], [the seven densities of round 0, of round 1, ...]; the last row repeats)
PATTERNS = {
    # a inside, densities falling through the level between candidates 4 and 5
    "a_inside": (1.0, -1.0, [[0.9, 0.7, 0.5, 0.3, 0.1, -0.2, -0.5]]),
    # b inside, rising through it between 2 and 3
    "b_inside": (-1.0, 1.0, [[-0.9, 0.0, 0.25, 0.5, 0.6, 0.7, 0.8]]),
    # a candidate exactly at the level counts as inside: the crossing is behind it, and q = 0 puts the vertex on the candidate
    "candidate_at_level": (1.0, -1.0, [[1.0, 1.0, LEVEL, -1.0, -1.0, -1.0, -1.0]]),
    "candidate_at_level_b_inside": (-1.0, 1.0, [[-1.0, -1.0, LEVEL, 1.0, 1.0, 1.0, 1.0]]),
    # two sign changes among the candidates (and the third against the far end): the first from a wins
    "two_changes": (1.0, -1.0, [[1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0]]),
    # three among the candidates
    "three_changes": (-1.0, 1.0, [[-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0], [-1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0]]),
    # the first interval and the last one
    "first_interval": (1.0, -1.0, [[-1.0] * 7]),
    "last_interval": (1.0, -1.0, [[1.0] * 7]),
    # a candidate out of range freezes the edge where it stands, for good: the later rows would move it
    "nan_in_round_1": (1.0, -1.0, [[0.9, 0.7, 0.5, 0.3, 0.1, -0.2, -0.5], [1.0, 1.0, 1.0, NAN, -1.0, -1.0, -1.0], [1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0]]),
    "inf_in_round_0": (-1.0, 1.0, [[-1.0, -1.0, 1.0, 1.0, 1.0, 1.0, INF], [-1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]]),
    "big_in_round_2": (1.0, -1.0, [[1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0], [1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], [-BIG, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], [1.0] * 7]),
    "below_big_is_kept": (1.0, -1.0, [[np.nextafter(BIG, np.float32(0)), 1.0, -1.0, -1.0, -1.0, -1.0, -1.0]]),
    # a NaN behind which the only sign change of the candidates would sit if it counted as outside
    "nan_hides_a_change": (1.0, -1.0, [[1.0, 1.0, NAN, 1.0, 1.0, 1.0, 1.0]]),
    # the caller changed `values` since the extraction: both on one side; the edge starts frozen and the vertex stays on the edge
    "values_on_one_side": (1.0, 0.5, [[0.9, 0.7, 0.5, 0.3, 0.1, -0.2, -0.5]]),
    "value_out_of_range": (NAN, -1.0, [[0.9, 0.7, 0.5, 0.3, 0.1, -0.2, -0.5]]),
    # a value at the level: inside; the extraction's t = -0 (a) and 1 (b)
    "value_at_level_a": (LEVEL, -1.0, [[0.9, 0.7, 0.5, 0.3, 0.1, -0.2, -0.5]]),
    "value_at_level_b": (-1.0, LEVEL, [[-0.9, -0.7, -0.5, -0.3, -0.2, -0.1, 0.0]]),
    # an id past the table
    "bad_id": (1.0, -1.0, [[0.9, 0.7, 0.5, 0.3, 0.1, -0.2, -0.5]]),
}
NAMES = list(PATTERNS)


def crafted(N, rounds=ROUNDS, only=None):
    """(xyz f32 [2 N, 3], edge_vertices i32 [N, 2], values f32 [2 N], level, densities f32 [rounds, N, 7]): edge i = (2 i, 2 i + 1)
    follows pattern NAMES[i % len(NAMES)] (only: that one pattern on every edge); a bad_id edge is (2 i, 2 N + 5)"""
    names = [only] * N if only else [NAMES[i % len(NAMES)] for i in range(N)]
    xyz = np.random.default_rng(N + 1).random((2 * N, 3)).astype(np.float32) * 2 - 1
    ev = np.stack([2 * np.arange(N), 2 * np.arange(N) + 1], 1).astype(np.int32).reshape(N, 2)
    values = np.zeros(2 * N, np.float32)
    dens = np.zeros((rounds, N, C), np.float32)
    for i, name in enumerate(names):
        va, vb, rows = PATTERNS[name]
        values[2 * i], values[2 * i + 1] = va, vb
        for r in range(rounds):
            dens[r, i] = rows[min(r, len(rows) - 1)]
        if name == "bad_id":
            ev[i, 1] = 2 * N + 5
    return xyz, ev, values, LEVEL, dens


def replay(dens):
    """the density_fn of the numpy statement that answers round r with dens[r], whatever it is asked"""
    state = {"round": 0}

    def fn(a, b, t):
        r = state["round"]
        state["round"] += 1
        assert len(t) == dens[r].size
        return dens[r].reshape(-1)

    return fn


# ---- analytic: the density -(|p|^2) in float32, summed x, y, z in that order (kind 1 of the emulation)
def radial_density(xyz):
    xyz = np.asarray(xyz, np.float32)

    def fn(a, b, t):
        t = np.asarray(t, np.float32)[:, None]
        p = xyz[a] + t * (xyz[b] - xyz[a])
        return -(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])

    return fn


def radial64(p):
    p = np.asarray(p, np.float64)
    return -(p * p).sum(-1)


def sphere_surface(scenes, name):
    """(xyz, cells, values, level, the extraction's statement) of a sphere case"""
    xyz, cells, values, level, _ = ic.case(scenes, name)
    return xyz, cells, values, level, ic.statement(scenes, name)


def residual_bound(xyz, edge_vertices, rounds):
    """An a-priori bound, per vertex, on |D(p) - L| for D(x) = -(|x|^2) in exact arithmetic, p the float32 vertex the refinement
    returns after `rounds` rounds on the float32 density above, L the float32 level.  u = 2^-24; R = the larger norm of the edge's
    two ends (|x| is convex along the edge, so it bounds |p(t)|); d = |xb - xa|.
      position: p = fl(xa + fl(t fl(xb - xa))) per coordinate, three roundings: |p_k - p_k(t)| <= u (2.01 |d_k| + 1.01 max(|xa_k|,
        |xb_k|)) <= 3.02 u R (|d_k| <= 2 R), so e_p = |p - p(t)|_2 <= 3.02 sqrt(3) u R.
      density: s = fl of three squares and two sums of the float32 point: |s - D(p_fl)| <= 3.01 u R'^2 with R' = R + e_p; and
        |D(p_fl) - D(p(t))| <= (2 R + e_p) e_p.  Together e_s, the error of a density the selection saw against D at the parameter.
      bracket: its ends are floats t_lo < t_hi whose densities, as seen, lie on the two sides of L: D(t_lo) and D(t_hi) are within
        e_s of being on those sides, so some t* in the bracket has |D(t*) - L| <= e_s.  The width is W <= 8^-rounds + 4 u (each
        round divides by 8 with at most two roundings of numbers <= 1; the brackets from (0, 1) are in fact exact).
      vertex: t is in the bracket, |D(p(t)) - L| <= e_s + Lip W with Lip = max |dD/dt| <= 2 R d; the returned p is a float32 point
        again: + (2 R + e_p) e_p.
    rounds = 0: W = 1."""
    x = np.asarray(xyz, np.float64)
    a, b = x[edge_vertices[:, 0]], x[edge_vertices[:, 1]]
    R = np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1))
    d = np.linalg.norm(b - a, axis=1)
    e_p = 3.02 * np.sqrt(3.0) * U * R
    move = (2 * R + e_p) * e_p
    e_s = 3.01 * U * (R + e_p) ** 2 + move
    W = 8.0 ** -rounds + (4 * U if rounds else 0.0)
    return e_s + 2 * R * d * W + move, W


# ---- brackets for the candidate order: random, adjacent floats, equal ends, the ends of [0, 1]
def order_brackets():
    rng = np.random.default_rng(8)
    lo = rng.random(200000).astype(np.float32)
    hi = np.maximum(lo, rng.random(200000).astype(np.float32))
    narrow = (lo + rng.random(200000).astype(np.float32) * np.float32(1e-6)).astype(np.float32).clip(0, 1)
    adj = np.nextafter(lo, np.float32(2))
    for k in range(9):
        adj = np.concatenate([adj, np.nextafter(adj[-200000:], np.float32(2))])
    adj = adj.clip(0, 1)
    tiny = np.float32(2.0) ** -rng.integers(1, 149, 200000).astype(np.float32)
    los = [lo, lo, np.tile(lo, 10), lo, np.zeros(200000, np.float32), tiny, 1 - lo * np.float32(1e-3)]
    his = [hi, np.maximum(lo, narrow), np.maximum(np.tile(lo, 10), adj), lo, tiny, np.nextafter(tiny, np.float32(1)), np.ones(200000, np.float32)]
    return np.concatenate(los).astype(np.float32), np.concatenate(his).astype(np.float32)
