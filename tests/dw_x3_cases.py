"""Operand tensors of the bf16x3 weight-gradient tests, built on the CPU from seeds: tests/test_dw_x3_gpu.py uploads them into the
caller-allocated buffers of tn_mlp_param_grads(_ex), tests/test_dw_x3.py emulates the arithmetic on the very same tensors.

A fill is a dict of float32 CPU tensors in plain [n, F] feature order -- d1..d4, h1..h4 [n, 128], x0 [n, 64], dhead [4, n] -- plus
dirs [R, 3].  The GEMMs multiply A = d4, d3, d2, d1 with B = h3, h2, h1, x0 over the sample axis (PAIRS)."""
import torch

# rays x samples per ray: the smallest sizes at which the kernel changes path (slices of 32 samples, at most 512 blocks)
SHAPES = [(3, 7), (37, 97), (257, 64), (300, 257)]
PAIRS = [("d4", "h3"), ("d3", "h2"), ("d2", "h1"), ("d1", "x0")]
KINDS = ("small", "a_mid", "b_mid", "mid_mid", "one_last", "one_inner", "random")
WIDTH = dict(d1=128, d2=128, d3=128, d4=128, h1=128, h2=128, h3=128, h4=128, x0=64)
EXACT_LIMIT = 2 ** 24


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def fill(kind, R, S, seed=0):
    """small:    every operand an integer in [-8, 8]: one bf16 piece only
    a_mid:    A in +-[0, 4095] (hi and mid pieces), B in {-1, 0, 1};  b_mid: the mirror image
    mid_mid:  both in +-[0, 1023]: mid x mid products
    one_last / one_inner: a single sample row nonzero (the last sample; one inside the chunk): A[s, f] = f + 1, B[s, g] = g + 1 --
              a wrong sample-to-K mapping or a stale lane beyond n is a wrong entry of an outer product
    random:   A ~ 1e-3 N(0, 1) with half of its entries zeroed (a ReLU mask), B = relu(N(0, 1)) (x0: N(0, 1) 0.7): the
              magnitudes of a training step
    dhead (d sigma_raw and the three d rgb_raw rows) and h4 stay small integers in the integer fills."""
    assert kind in KINDS
    n = R * S
    g = torch.Generator().manual_seed(1000 * seed + 7 * KINDS.index(kind) + n)
    a_names, b_names = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    out = {}
    if kind == "random":
        for k in a_names:
            out[k] = torch.randn(n, WIDTH[k], generator=g) * 1e-3 * (torch.rand(n, WIDTH[k], generator=g) < 0.5)
        for k in ("h1", "h2", "h3", "h4"):
            out[k] = torch.relu(torch.randn(n, WIDTH[k], generator=g))
        out["x0"] = torch.randn(n, 64, generator=g) * 0.7
        out["dhead"] = torch.randn(4, n, generator=g) * 1e-3
    elif kind in ("one_last", "one_inner"):
        s = n - 1 if kind == "one_last" else n // 2 + 1
        for k, width in WIDTH.items():
            out[k] = torch.zeros(n, width)
            out[k][s] = torch.arange(1, width + 1).float()
        out["dhead"] = torch.zeros(4, n)
        out["dhead"][:, s] = torch.tensor([3.0, -2.0, 5.0, 7.0])
    else:
        ra, rb = {"small": (8, 8), "a_mid": (4095, 1), "b_mid": (1, 4095), "mid_mid": (1023, 1023)}[kind]
        for k in a_names:
            out[k] = _ints(g, (n, WIDTH[k]), -ra, ra)
        for k in b_names:
            out[k] = _ints(g, (n, WIDTH[k]), -rb, rb)
        out["h4"] = _ints(g, (n, 128), -8, 8)
        out["dhead"] = _ints(g, (4, n), -8, 8) if kind == "small" else _ints(g, (4, n), -1, 1)
    out = {k: v.float().contiguous() for k, v in out.items()}
    out["dirs"] = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).contiguous()
    return out


def exact_in_fp32(f):
    """True when every partial sum of every product of the fill, in any order and in any split of the operands into pieces
    (|hi| + |mid| + |lo| <= (1 + 2^-7) |x|), is an integer below 2^24: sum_s |a| |b| (1 + 2^-7)^2 < 2^24, also for the bias sums
    and the density vector"""
    slack = (1 + 2.0 ** -7) ** 2
    for a, b in PAIRS:
        if float((f[a].double().abs().t() @ f[b].double().abs()).max()) * slack >= EXACT_LIMIT:
            return False
        if float(f[a].double().abs().sum(0).max()) >= EXACT_LIMIT:
            return False
    return float((f["dhead"][0].double().abs()[None] @ f["h3"].double().abs()).max()) < EXACT_LIMIT


def split3(x):
    """the three bf16 pieces of fp32 values as x3::split8 forms them: round to nearest even, residuals in fp32"""
    hi = x.bfloat16().float()
    r1 = x - hi
    mid = r1.bfloat16().float()
    r2 = r1 - mid
    lo = r2.bfloat16().float()
    return hi, mid, lo


def six_products(a, b):
    """float64 sum of the six partial products the kernels form for a * b (broadcasting), small terms first"""
    ah, am, al = (t.double() for t in split3(a))
    bh, bm, bl = (t.double() for t in split3(b))
    return ((((al * bh + ah * bl) + am * bm) + am * bh) + ah * bm) + ah * bh
