"""Inputs and float64 statements of the fused MLP training chain at the sizes where its launchers change form, built on the CPU
from seeds: tests/test_mlp_edges_gpu.py runs the kernels on them, tests/test_mlp_edge_cases.py checks them without a GPU (the
fills are exact where they claim to be, the single rows sit where they claim to, the fp32 PyTorch evaluation of every statement
meets the bound the GPU test applies, both ReLU branches are live at every edge).

The launcher constants are restated here from csrc/ (tn_mlp_common.h: mlp_forward_grid; tn_mlp_grad.hip: slicing, DW_GRID;
tn_mlp_bwd.hip / tn_occupancy_train.hip: the ray-sum and compact grids).  A change of one of them moves an edge away from the
sizes below: test_mlp_edge_cases.py::test_sizes_sit_on_the_edges then says which.

Statements take tensors on any device and return float64 values with the bound of their arithmetic:
  a saved layer    |h - h64| <= 2^-21 (|W| |x| + |b| [+ |bias|]) + 4e-7 |h64|      (tests/test_train_x3_gpu.py)
  a dX layer       |d - d64| <= 2^-21 (|d_in| |W| [+ |d sigma_raw| |wd|]) + 4e-7 |d64|, 0 under a clear mask bit
                                                                                  (tests/test_adjoint_x3_gpu.py)
  an fp32 sum      |g - g64| <= (c + 1) 2^-24 sum |terms| for c terms in any order  (tests/gather_cases.py)"""
import importlib

import torch

import dw_x3_cases as dw
from gather_cases import U
from test_dw_x3_gpu import ACTS, DS, _references, _to_quad_major

render = importlib.import_module("tetra-nerf_amd.render")

# ---- the launchers' constants (csrc/) ----------------------------------------------------------------------------------
FWD_GROUP, DX_GROUP, GROUP_GRID = 256, 128, 256      # samples per group of k_mlp_forward* / k_mlp_backward*, blocks at most
DW_GRID, DW_UNIT, RGB_UNIT = 512, 32, 128           # slices at most; slices are multiples of 32 (GEMMs) / 128 (rgb head) samples
RAY_GRID, RAY_SUB = 2048, 8                         # one block per ray, at most; sub-lanes per quad
COMPACT_GRID, COMPACT_BLOCK = 2048, 256             # k_compact_rows: blocks at most, rows per block
NOT_A_SAMPLE = 0x7F7F7F7F

# (R, S, the edge the size names); S shares no factor with 32 wherever the edge allows it
SIZES = [
    (1, 1, "one lane"),
    (127, 1, "dX group tail of 127"), (8, 16, "dX group tail of 0"), (43, 3, "dX group tail of 1"),
    (85, 3, "forward group tail of 255"), (16, 16, "forward group tail of 0"), (1, 257, "forward group tail of 1"),
    (127, 129, "dW slices of 32, last grid of 512"), (2048, 8, "dW slices of 32, 512 full; rays = the ray-sum grid, S = 8"),
    (113, 145, "dW slices of 64, 257 blocks, the last one holds one sample"),
    (217, 151, "dX: every block one group, the last partial"), (4096, 8, "dX: 256 full groups; the shipped ray count"),
    (331, 99, "dX: block 0 runs a second group of one sample"),
    (255, 257, "forward: every block one group; rgb-head slices of 128"), (4096, 16, "forward: 256 full groups; rgb head 512 x 128"),
    (65537, 1, "forward second trip and carry; rgb-head slices of 256; S = 1 at scale"),
    (1, 65537, "the same with one ray across all slices"),
    (273, 241, "a full group followed by a one-sample group on different blocks"),
    (257, 257, "the same one group later: three blocks run a second group"),
]
IDS = [f"{R}x{S}" for R, S, _ in SIZES]
FORWARD_EDGES = [(R, S) for R, S, _ in SIZES if R * S in (1, 255, 256, 257, 65535, 65536, 65537, 65793, 66049)]
DX_EDGES = [(R, S) for R, S, _ in SIZES if R * S in (127, 128, 129, 32767, 32768, 32769, 65537)]
RAY_SUM_SIZES = [(R, S) for R in (1, 2047, 2048, 2049, 4097) for S in (1, 7, 8, 9, 17)]
COMPACT_ROWS = [524287, 524288, 524289]


def slicing(n, unit):
    """(grid, slice) of tn_mlp_grad.hip: at most DW_GRID slices, each a multiple of `unit` samples"""
    slice_ = -(-n // DW_GRID)
    slice_ = -(-slice_ // unit) * unit
    return -(-n // slice_), slice_


def second_owner_rows(n):
    """the first sample that a second grid trip (forward, dX) or a second slice (the GEMMs, the rgb head) owns, where there is one"""
    rows = {}
    if n > FWD_GROUP * GROUP_GRID:
        rows["fwd"] = FWD_GROUP * GROUP_GRID
    if n > DX_GROUP * GROUP_GRID:
        rows["dx"] = DX_GROUP * GROUP_GRID
    for name, unit in (("dw", DW_UNIT), ("rgb", RGB_UNIT)):
        grid, slice_ = slicing(n, unit)
        if grid > 1:
            rows[name] = slice_
    return rows


def edge_samples(n):
    """first and last sample of every group or slice edge a size can name: the ends, the last group of each kind, both sides of
    every second-trip / second-slice start and of the last slice's start"""
    s = {0, n - 1}
    for group in (DX_GROUP, FWD_GROUP):
        s |= {(n - 1) // group * group, (n - 1) // group * group - 1}
    for row in second_owner_rows(n).values():
        s |= {row - 1, row}
    for unit in (DW_UNIT, RGB_UNIT):
        grid, slice_ = slicing(n, unit)
        s |= {(grid - 1) * slice_ - 1, (grid - 1) * slice_}
    return sorted(x for x in s if 0 <= x < n)


# ---- fills of the caller-allocated buffers (tests/dw_x3_cases.py: plain [n, F] CPU tensors, dhead [4, n], dirs [R, 3]) -------------
KINDS = ("small", "one_last", "one_first_of_second_trip", "random")


def exactness_condition(n):
    """operands in [-8, 8]: every partial sum of every output, in any order and in any split into bf16 pieces, is an integer
    below 2^24"""
    return n * 64 * (1 + 2.0 ** -7) ** 2 < 2 ** 24


def single_row(R, S, row):
    """dw_x3_cases.fill("one_last") with the nonzero sample row at `row`"""
    f = dw.fill("one_last", R, S)
    n = R * S
    for k in dw.WIDTH:
        f[k][row] = f[k][n - 1]
        if row != n - 1:
            f[k][n - 1] = 0
    f["dhead"][:, row] = f["dhead"][:, n - 1]
    if row != n - 1:
        f["dhead"][:, n - 1] = 0
    return f


def fill(kind, R, S, unit=DW_UNIT):
    """small / random / one_last: dw_x3_cases.fill; one_first_of_second_trip: the single row at the first sample of the second slice
    of `unit` samples (DW_UNIT: the GEMMs', RGB_UNIT: the rgb head's)"""
    assert kind in KINDS
    if kind != "one_first_of_second_trip":
        return dw.fill(kind, R, S)
    grid, slice_ = slicing(R * S, unit)
    assert grid > 1
    return single_row(R, S, slice_)


def one_ray(R, S, ray):
    """the small fill with every sample outside `ray` zeroed: the head layer's encoding columns then hold that ray's encoding only"""
    f = dw.fill("small", R, S)
    keep = torch.zeros(R * S, dtype=torch.bool)
    keep[ray * S:(ray + 1) * S] = True
    for k in dw.WIDTH:
        f[k][~keep] = 0
    f["dhead"][:, ~keep] = 0
    return f


def nonzero_rows(f):
    rows = torch.zeros(f["dhead"].shape[1], dtype=torch.bool)
    for k in dw.WIDTH:
        rows |= f[k].ne(0).any(1)
    return torch.nonzero(rows | f["dhead"].ne(0).any(0))[:, 0].tolist()


def quad_buffers(f, device="cpu"):
    """a fill as the buffers the C entry takes (tests/test_dw_x3_gpu.py::_upload)"""
    b = {k: _to_quad_major(f[k].to(device)) for k in ACTS + DS}
    b["dhead"] = f["dhead"].to(device).contiguous()
    return b


def ray_d4(kind, rays, S):
    """d4 [n, 128] of the per-ray sums: integers in [-8, 8] (a sum of S of them is exact) or 1e-3 N(0, 1) with half of the entries
    zeroed"""
    n = rays * S
    g = torch.Generator().manual_seed(31 * rays + S + (0 if kind == "small" else 1))
    if kind == "small":
        return torch.randint(-8, 9, (n, 128), generator=g).float()
    return (torch.randn(n, 128, generator=g) * 1e-3 * (torch.rand(n, 128, generator=g) < 0.5)).float()


def dropping_list(rays, S):
    """ascending list of the samples of all rays but those with r % 7 == 3; of the last remaining ray only its first sample"""
    r = torch.arange(rays)
    kept = r[r % 7 != 3]
    s = (kept[:, None] * S + torch.arange(S)[None]).reshape(-1)
    return s[:len(s) - (S - 1)].to(torch.int32), int(kept[-1])


# ---- a real problem per size (tests/test_train_culled_gpu.py::_problem, on the CPU) -------------------------------------------
_PROBLEMS = {}


def _model(seed, scale):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        mlp = render.TetraMLP()
    for p in mlp.parameters():
        p.data.mul_(scale)
    return mlp


def problem(R, S, default_init=False):
    """seeded TetraMLP x 1.5 (every ReLU / softplus / sigmoid branch live; default_init: as initialised), field, vertex ids with EMPTY
    entries, barycentrics, directions, a per-ray bias and upstream gradients at a realistic loss scale -- CPU tensors, built once"""
    key = (R, S, default_init)
    if key not in _PROBLEMS:
        n = R * S
        V = 200 if n < 4096 else 5000
        mlp = _model(R + S, 1.0 if default_init else 1.5)
        g = torch.Generator().manual_seed(7 * R + S)
        vi = torch.randint(0, V, (n, 4), generator=g, dtype=torch.int32)
        vi[::17, 2] = -1
        _PROBLEMS[key] = dict(
            R=R, S=S, n=n, V=V, mlp=mlp, w=[x.detach() for x in render.mlp_weights(mlp)], field=torch.randn(64, V, generator=g) * 0.7,
            vi=vi, bc=(torch.rand(n, 3, generator=g) / 3).contiguous(),
            dirs=torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).contiguous(),
            bias=torch.randn(R, 128, generator=g) * 0.7, d_sigma=torch.randn(n, generator=g) * 1e-3,
            d_rgb=torch.randn(n, 3, generator=g) * 1e-3)
    return _PROBLEMS[key]


def on(p, device):
    """the tensors of a problem on `device`"""
    out = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in p.items() if k != "mlp"}
    out["w"] = [x.to(device) for x in p["w"]]
    return out


# ---- float64 statements ---------------------------------------------------------------------------------------------
def gather64(p, rows=None):
    """the gather in float64: x0 [m, 64] of the samples `rows` (all without it); EMPTY vertices are skipped"""
    vi, bc = (p["vi"], p["bc"]) if rows is None else (p["vi"][rows], p["bc"][rows])
    b64 = bc.double()
    wts = torch.cat([1 - b64.sum(-1, keepdim=True), b64], -1)
    wts = torch.where(vi < 0, torch.zeros_like(wts), wts)
    return (p["field"].double().t()[vi.long().clamp_min(0)] * wts[..., None]).sum(1)


def layer(x, W, b, extra=None, dtype=torch.float64):
    """relu(x W^T + b [+ extra]) in `dtype` and the float64 bound a stored fp32 / bf16x3 output is held to"""
    x64, W64, b64 = x.double(), W.double(), b.double()
    e64 = None if extra is None else extra.double()
    pre = x.to(dtype) @ W.to(dtype).t() + b.to(dtype) + (0 if extra is None else extra.to(dtype))
    h64 = (x64 @ W64.t() + b64 + (0 if e64 is None else e64)).clamp_min(0)
    bound = 2.0 ** -21 * (x64.abs() @ W64.abs().t() + b64.abs() + (0 if e64 is None else e64.abs())) + 4e-7 * h64
    return pre.clamp_min(0), bound


def dx_layer(d_in, W, mask=None, extra=None, dtype=torch.float64):
    """(d_in W [+ extra]) [* mask] in `dtype` and its float64 bound; extra = d sigma_raw wd, the density term of d3"""
    d64, W64 = d_in.double(), W.double()
    e64 = None if extra is None else extra.double()
    out = d_in.to(dtype) @ W.to(dtype) + (0 if extra is None else extra.to(dtype))
    o64 = d64 @ W64 + (0 if e64 is None else e64)
    bound = 2.0 ** -21 * (d64.abs() @ W64.abs() + (0 if e64 is None else e64.abs()))
    if mask is not None:
        out, o64 = out * mask, o64 * mask
    return out, bound + 4e-7 * o64.abs()


def head_input(p, acts3, rows=None):
    """[direction encoding 27 (fp32: the kernel's statement, an INPUT of the layer) | h3] and the per-sample bias rows"""
    n, S = p["n"], p["S"]
    ray = torch.div(torch.arange(n, device=acts3.device) if rows is None else rows, S, rounding_mode="floor")
    enc = render.direction_encoding(p["dirs"].float()).double()[ray]
    return torch.cat([enc, acts3.double()], -1), p["bias"].double()[ray]


def network(p, x0, rows=None, biased=True, dtype=torch.float64):
    """the whole network from x0 in `dtype`: {h1..h4, sigma, rgb, and the dX chain d4..d1, dhead, dx0 under its own masks}"""
    w = [t.to(dtype) for t in p["w"]]
    out = {"x0": x0.to(dtype)}
    x = out["x0"]
    for l in range(3):
        x = out[f"h{l + 1}"] = torch.relu(x @ w[2 * l].t() + w[2 * l + 1])
    hin, bias = head_input(p, x, rows)
    pre = hin.to(dtype) @ w[8].t() + w[9] + (bias.to(dtype) if biased else 0)
    out["h4"] = torch.relu(pre)
    out["sigma"] = torch.nn.functional.softplus(x @ w[6].t() + w[7])[:, 0]
    out["rgb"] = torch.sigmoid(out["h4"] @ w[10].t() + w[11])
    d_sigma = p["d_sigma"] if rows is None else p["d_sigma"][rows]
    d_rgb = p["d_rgb"] if rows is None else p["d_rgb"][rows]
    dsr = d_sigma.to(dtype) * (1 - torch.exp(-out["sigma"]))
    drr = d_rgb.to(dtype) * out["rgb"] * (1 - out["rgb"])
    out["dhead"] = torch.cat([dsr[None], drr.t()], 0)
    out["d4"] = (drr @ w[10]) * (out["h4"] > 0)
    out["d3"] = (out["d4"] @ w[8][:, 27:] + dsr[:, None] * w[6]) * (out["h3"] > 0)
    out["d2"] = (out["d3"] @ w[4]) * (out["h2"] > 0)
    out["d1"] = (out["d2"] @ w[2]) * (out["h1"] > 0)
    out["dx0"] = out["d1"] @ w[0]
    return out


def rgb_head_sums(dhead, h4):
    """what k_rgb_head_grad sums, from dhead [4, n] and h4 [n, 128]: {name: (float64 value, sum of the magnitudes of its terms)}"""
    d, h = dhead.double(), h4.double()
    return {"wr": (d[1:4] @ h, d[1:4].abs() @ h.abs()), "bd": (d[0].sum()[None], d[0].abs().sum()[None]),
            "br": (d[1:4].sum(1), d[1:4].abs().sum(1))}


def param_sums(b, dirs, S):
    """all twelve parameter sums from quad-major buffers (quad_buffers; any device): tests/test_dw_x3_gpu.py::_references extended
    with wr, bd, br.  Every element is a sum of c = n terms."""
    from test_adjoint_x3_gpu import _quad_major

    n = b["dhead"].shape[1]
    ref = _references(None, b, dirs, S)
    ref.update(rgb_head_sums(b["dhead"], _quad_major(b["h4"], n)))
    return ref


def param_sums_in(f, dtype):
    """the same sums from a plain fill evaluated in `dtype` (float32: one fp32 order of each sum, what the bound must admit)"""
    S = f["dhead"].shape[1] // f["dirs"].shape[0]
    enc = render.direction_encoding(f["dirs"].float()).to(dtype).repeat_interleave(S, dim=0)
    t = {k: f[k].to(dtype) for k in list(dw.WIDTH) + ["dhead"]}
    out = {}
    for name, bias, a, x in (("wh", "bh", t["d4"], torch.cat([enc, t["h3"]], 1)), ("w3", "b3", t["d3"], t["h2"]), ("w2", "b2", t["d2"], t["h1"]),
                             ("w1", "b1", t["d1"], t["x0"])):
        out[name], out[bias] = a.t() @ x, a.sum(0)
    out["wd"] = (t["dhead"][0][:, None] * t["h3"]).sum(0)[None]
    out["wr"], out["bd"], out["br"] = t["dhead"][1:4] @ t["h4"], t["dhead"][0].sum()[None], t["dhead"][1:4].sum(1)
    return out


def sum_bound(mag, c):
    return (c + 1) * U * mag


def ray_sums(d4, S, listed=None, rays=None):
    """per-ray sums of d4 [m, 128] (row i belongs to sample listed[i]; all samples in order without a list): float64 value
    [rays, 128], sum of the magnitudes, number of terms per ray"""
    m = d4.shape[0]
    s = torch.arange(m, device=d4.device) if listed is None else listed.long().to(d4.device)
    rays = m // S if rays is None else rays
    ray = torch.div(s, S, rounding_mode="floor")
    val = torch.zeros(rays, 128, dtype=torch.float64, device=d4.device).index_add_(0, ray, d4.double())
    mag = torch.zeros_like(val).index_add_(0, ray, d4.double().abs())
    return val, mag, torch.bincount(ray, minlength=rays)
