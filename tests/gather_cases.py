"""Inputs and float64 references of the gather tests (the barycentric gather, its adjoints, the barycentric adjoint), built on the
CPU from seeds: tests/test_gather_edges_gpu.py uploads them, tests/test_gather_cases.py holds the CPU oracle and the inputs
themselves to the references below, so that a failure on the GPU is not the test's own error.  No kernel runs here.

Index streams are RAY-LIKE (walk_stream): a tuple of D distinct vertices is held for a run of samples, then ONE slot is replaced
and the slots are permuted -- the neighbour tetrahedron, which shares D - 1 vertices in any order -- and after some steps a fresh
tuple starts the next ray.  That is what the register carries of k_interp_fwd64 and k_interp_bwd (tn_interp.hip) are written for
and what uniform random ids reach about once in fifty samples, never in the permuted form.

Two fills.  `random`: standard normal fp32.  `exact`: g and field integers in [-8, 8], barycentrics multiples of 1/8 with sum at
most (D - 1)/8, so every weight is a multiple of 1/8 in [1/8, 1], every product a multiple of 1/8 of magnitude <= 8, and every
partial sum of c products exact in fp32 while 8 * 64 * c < 2^24: the correct adjoint then has ONE bit pattern, whatever the order
of the additions.

The weights are the kernels' own: w0 = 1 - ((b0 + b1) + ...) is ONE fp32 expression (weights32, numpy fp32 = IEEE single);
everything after it is float64.  Error bounds (u = 2^-24, the fp32 unit round-off):
  forward   |fl - exact| <= (D + 1) u A,  A = sum_k |w_k| |field[v_k]|: D products, D additions (the first one to zero is exact)
            -- gamma_D A to first order; the CPU oracle measures 0.97 of D u A on these streams, hence D + 1;
  adjoint   |fl - exact| <= (c + 1) u A,  A = sum over the c contributions to the element of |w| |g|: one product and at most
            c additions per term in ANY order (the sequential oracle, the atomic kernel's run-length partial sums, the
            deterministic kernel's quarters), to first order in u.  The bound is only as sharp as 1 / c: above c ~ 1000 one
            dropped term hides under it, so every case keeps max c <= MAX_COUNT.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
MAX_COUNT = 1024
EDGES = (8, 64, 256)          # a tuple change is forced between samples e - 1 and e: the 8-sample batch of k_interp_bwd /
                              # the 8-sample lane group of k_interp_fwd64, the 64-sample tile, the 256-sample block


def walk_stream(rng, n, V, D, exact=False):
    """-> vi int32 [n, D] (EMPTY = -1), bc float32 [n, D - 1].  Runs of 1..12 samples of one tuple; between runs one slot
    is replaced by a new vertex and the slots are permuted; after 1..40 such steps a fresh tuple of D distinct vertices.
    Overlaid, each on a few per cent of the samples (at least once, twice for the single EMPTY slot, from n >= 24 on): whole
    samples EMPTY, samples with exactly one EMPTY slot (slot 0 and slot D - 1 both occur), samples whose slot 1 repeats
    slot 0.  A run boundary (= a tuple change) is forced at every EDGES index below n, and the samples on either side of it
    stay clear of the overlays."""
    assert V >= 2 * D and n >= 1
    # run boundaries
    K = n // 6 + 8
    lens = rng.integers(1, 13, K)
    while int(lens.sum()) < n:
        lens = np.concatenate([lens, rng.integers(1, 13, K)])
    cuts = np.unique(np.concatenate([[0], np.cumsum(lens), [e for e in EDGES if e < n]]).astype(np.int64))
    cuts = cuts[cuts < n]
    K = len(cuts)
    run_len = np.diff(np.concatenate([cuts, [n]]))
    # one tuple per run (plain Python on pre-drawn numbers: n / 6.5 steps)
    slot = rng.integers(0, D, K).tolist()
    newv = rng.integers(0, V, (K, D)).tolist()
    perm = rng.permuted(np.tile(np.arange(D), (K, 1)), axis=1).tolist()
    ray = rng.integers(1, 41, K).tolist()
    tuples = []
    cur, left = None, 0
    for i in range(K):
        if left == 0:
            cur = rng.choice(V, D, replace=False).tolist()
            left = ray[i]
        else:
            v = newv[i][0]
            while v in cur:
                v = int(rng.integers(0, V))
            cur = list(cur)
            cur[slot[i]] = v
            cur = [cur[j] for j in perm[i]]
            left -= 1
        tuples.append(cur)
    vi = np.repeat(np.asarray(tuples, dtype=np.int32).reshape(K, D), run_len, axis=0)
    assert vi.shape == (n, D)
    # overlays
    keep = np.ones(n, bool)
    keep[0] = False
    for e in EDGES:
        keep[max(e - 1, 0):e + 1] = False
    free = rng.permutation(np.flatnonzero(keep))

    def take(frac, least):
        nonlocal free
        k = min(len(free), max(least if n >= 24 else 0, int(round(frac * n))))
        out, free = free[:k], free[k:]
        return out

    vi[take(0.03, 1)] = -1
    one = take(0.04, 2)
    which = rng.integers(0, D, len(one))
    which[:2] = (0, D - 1)[:len(one)]
    vi[one, which] = -1
    dup = take(0.03, 1)
    vi[dup, 1] = vi[dup, 0]
    if exact:
        # eighths: a total of at most D - 1, spread over the D - 1 coordinates
        total = rng.integers(0, D, n)
        eighths = np.zeros((n, D - 1), np.int64)
        for t in range(D - 1):
            eighths[np.arange(n), rng.integers(0, D - 1, n)] += t < total      # (one element per row: no repeated index)
        bc = eighths.astype(np.float32) / np.float32(8)
    else:
        bc = rng.random((n, D - 1)).astype(np.float32) / np.float32(D)
    return np.ascontiguousarray(vi), np.ascontiguousarray(bc.astype(np.float32))


def run_length_stream(rng, V, D, lengths, exact=False):
    """A stream in which vertex j (j < len(lengths)) is sampled exactly lengths[j] times (in slot j % D) and every other
    vertex is a filler drawn from [len(lengths), V): the run of vertex j in the sorted pair list of the deterministic adjoint
    (k_interp_bwd_det splits it into quarters by len * wave / 4) has exactly that length.  Samples are shuffled."""
    m = len(lengths)
    assert V - m >= 2 * D
    rows = []
    for j, L in enumerate(lengths):
        t = np.stack([rng.choice(V - m, D, replace=False) + m for _ in range(L)]).astype(np.int32)
        t[:, j % D] = j
        rows.append(t)
    vi = np.concatenate(rows)
    vi = vi[rng.permutation(len(vi))]
    n = len(vi)
    if exact:
        bc = (rng.integers(0, 2, (n, D - 1)).astype(np.float32)) / np.float32(8)
    else:
        bc = rng.random((n, D - 1)).astype(np.float32) / np.float32(D)
    return np.ascontiguousarray(vi), np.ascontiguousarray(bc)


def stream_stats(vi):
    """What a stream contains, as counts: permuted-slot carries (a vertex of sample s that sample s - 1 of the same 8-sample
    group -- the span of k_interp_fwd64's register carry -- held in ANOTHER slot), single-EMPTY-slot samples by slot, duplicates (slot 1 == slot 0, live), forced edges present."""
    n, D = vi.shape
    live = vi >= 0
    moved = np.zeros(n, bool)
    for k in range(D):
        for c in range(D):
            if c != k:
                moved[1:] |= live[1:, k] & (vi[1:, k] == vi[:-1, c])
    moved[::8] = False
    single = live.sum(1) == D - 1
    full = live.all(1)
    edges = [e for e in EDGES if e < n and full[e - 1] and full[e]
             and sorted(vi[e - 1].tolist()) != sorted(vi[e].tolist())]
    return dict(permuted_carry=int(moved.sum()), single_empty=int(single.sum()),
                single_empty_slot0=int((single & ~live[:, 0]).sum()), single_empty_last=int((single & ~live[:, D - 1]).sum()),
                all_empty=int((~live.any(1)).sum()), duplicate=int((live[:, 0] & (vi[:, 0] == vi[:, 1])).sum()),
                edges=edges, expected_edges=[e for e in EDGES if e < n])


def fills(rng, n, V, Fd, exact=False):
    """-> g float32 [n, Fd] (gradient rows), field float32 [Fd, V]"""
    if exact:
        return (rng.integers(-8, 9, (n, Fd)).astype(np.float32), rng.integers(-8, 9, (Fd, V)).astype(np.float32))
    return rng.standard_normal((n, Fd)).astype(np.float32), rng.standard_normal((Fd, V)).astype(np.float32)


def weights32(bc):
    """[n, D] fp32: (1 - ((b0 + b1) + ...), b0, b1, ...) with the sum and the subtraction in fp32, left to right from zero,
    as every kernel of tn_interp.hip and the CPU oracle form them."""
    bc = np.asarray(bc, np.float32)
    s = np.zeros(bc.shape[0], np.float32)
    for k in range(bc.shape[1]):
        s = (s + bc[:, k]).astype(np.float32)
    return np.concatenate([(np.float32(1) - s).astype(np.float32)[:, None], bc], axis=1)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))      # (a writable float64 copy of a read-only case array)


def forward_ref(vi, bc, field):
    """-> value float64 [n, Fd], A float64 [n, Fd] = sum_k |w_k| |field[:, v_k]| (EMPTY slots skipped)"""
    w = _t64(weights32(bc))
    ft = _t64(field.T)
    ids = torch.from_numpy(vi.astype(np.int64))
    val = torch.zeros(vi.shape[0], field.shape[0], dtype=torch.float64)
    A = torch.zeros_like(val)
    for k in range(vi.shape[1]):
        live = (ids[:, k] >= 0).double()[:, None]
        rows = ft[ids[:, k].clamp_min(0)]
        val += live * w[:, k:k + 1] * rows
        A += live * w[:, k:k + 1].abs() * rows.abs()
    return val.numpy(), A.numpy()


def adjoint_ref(vi, bc, g, V):
    """-> vertex-major float64 sum [V, Fd], A float64 [V, Fd] = sum over contributions of |w_k| |g|, count int64 [V]"""
    w = _t64(weights32(bc))
    g64 = _t64(g)
    ids = torch.from_numpy(vi.astype(np.int64))
    out = torch.zeros(V, g.shape[1], dtype=torch.float64)
    A = torch.zeros_like(out)
    cnt = np.zeros(V, np.int64)
    for k in range(vi.shape[1]):
        live = ids[:, k] >= 0
        t = w[live, k:k + 1] * g64[live]
        out.index_add_(0, ids[live, k], t)
        A.index_add_(0, ids[live, k], t.abs())
        cnt += np.bincount(vi[live.numpy(), k], minlength=V)
    return out.numpy(), A.numpy(), cnt


def bary_adjoint_ref(vi, g, field):
    """The statement of include/tetranerf_hip.h: grad_bary[s, k] = sum_c g[s, c] (F[c, v_{k+1}] - F[c, v_0]), the row of an
    EMPTY id a zero row -> float64 [n, D - 1], and A = sum_c |g| (|F[v_{k+1}]| + |F[v_0]|)."""
    ft = _t64(field.T)
    g64 = _t64(g)
    ids = torch.from_numpy(vi.astype(np.int64))
    rows = [ft[ids[:, k].clamp_min(0)] * (ids[:, k] >= 0).double()[:, None] for k in range(vi.shape[1])]
    val = torch.stack([(g64 * (r - rows[0])).sum(1) for r in rows[1:]], 1)
    A = torch.stack([(g64.abs() * (r.abs() + rows[0].abs())).sum(1) for r in rows[1:]], 1)
    return val.numpy(), A.numpy()


# ---- the cases both test files use -------------------------------------------------------------------------------------
DIMS = (2, 3, 4, 6)
FWD64_N = (1, 7, 8, 9, 63, 64, 65, 252, 256, 260, 1028)
FWD_FD = (1, 3, 4, 31, 32, 33, 36, 60, 63, 65, 96, 128, 130, 192)
FWD_N_D4 = (1, 31, 32, 33, 127, 128, 129)
ADJ_FD = (1, 3, 63, 64, 65, 128, 130)
ADJ_N = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000)
DET_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 700)
DET_GRID = 16384                # k_interp_bwd_det's grid cap: run_bwd_det (tn_interp.hip), 256 * 64 blocks, one vertex each

FORWARD64_CASES = [(D, 64, n) for D in DIMS for n in FWD64_N]
FORWARD_CASES = [(D, Fd, 1000) for D in DIMS for Fd in FWD_FD] + [(4, Fd, n) for Fd in FWD_FD for n in FWD_N_D4]
ADJOINT_CASES = [(D, Fd, 1000) for D in DIMS for Fd in ADJ_FD] + [(4, 64, n) for n in ADJ_N if n != 1000]
BARY_CASES = [(D, Fd, 1000) for D in DIMS for Fd in (36, 64)]


def num_vertices(n):
    """few enough vertices that they repeat across rays, enough that no vertex collects more than MAX_COUNT terms"""
    return 97 if n <= 65 else 301 if n <= 260 else 777


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(D, Fd, n, fill, V=None):
    """One case, built once and shared (read-only arrays): the walk stream, both operands, all three references."""
    V = V or num_vertices(n)
    rng = np.random.default_rng([D, Fd, n, V, 1 if fill == "exact" else 0])
    vi, bc = walk_stream(rng, n, V, D, exact=fill == "exact")
    g, field = fills(rng, n, V, Fd, exact=fill == "exact")
    return _finish(vi, bc, g, field, V)


def _finish(vi, bc, g, field, V):
    fwd, fwd_A = forward_ref(vi, bc, field)
    adj, adj_A, cnt = adjoint_ref(vi, bc, g, V)
    return _freeze(dict(vi=vi, bc=bc, g=g, field=field, V=V, fwd=fwd, fwd_A=fwd_A, adj=adj, adj_A=adj_A, count=cnt))


@functools.lru_cache(maxsize=None)
def run_length_case(fill, D=4, Fd=64, V=600):
    rng = np.random.default_rng([D, Fd, V, 2, 1 if fill == "exact" else 0])
    vi, bc = run_length_stream(rng, V, D, DET_LENGTHS, exact=fill == "exact")
    g, field = fills(rng, len(vi), V, Fd, exact=fill == "exact")
    return _finish(vi, bc, g, field, V)


@functools.lru_cache(maxsize=None)
def last_vertices_case(fill, D=4, Fd=64, n=1200, tail=37):
    """V = DET_GRID + tail with only the last `tail` vertices sampled: the second trip of k_interp_bwd_det's vertex loop"""
    V = DET_GRID + tail
    rng = np.random.default_rng([D, Fd, n, 3, 1 if fill == "exact" else 0])
    vi, bc = walk_stream(rng, n, tail, D, exact=fill == "exact")
    vi = np.where(vi >= 0, vi + (V - tail), -1).astype(np.int32)
    g, field = fills(rng, n, V, Fd, exact=fill == "exact")
    return _finish(vi, bc, g, field, V)


def adjoint_bound(c):
    """(c + 1) u A + c 2^-126 per element, from A [V, Fd] and the counts [V]; the last term allows a flushed subnormal per
    addition (hardware float atomics flush denormals)"""
    cnt = c["count"].astype(np.float64)[:, None]
    return (cnt + 1) * U * c["adj_A"] + cnt * 2.0 ** -126
