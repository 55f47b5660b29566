"""Forward render path of the Tetra-NeRF model on top of the HIP ops (inference / evaluation).

Mirrors TetrahedraNerf.get_outputs (/root/reference/tetranerf/nerfstudio/model.py:520-662) in
evaluation mode for both shipped configurations (`tetra-nerf-original`: uniform 256 + PDF 256;
`tetra-nerf`: biased TetrahedraSampler 128 + PDF 128, registration.py:55-57):

    trace_rays -> nears/fars (:531-544) -> coarse samples: nerfstudio UniformSampler (eval:
    bins = linspace(0,1,S+1), euclidean = near + bins*(far-near)) or the biased TetrahedraSampler
    (:111-192) -> find_visited_cells (:560-567) -> interpolate_values (:569-573)
    [num_fine_samples > 0 (:575-600): mlp_base + density head -> get_weights -> PDFSampler
     (include_original: S + S_fine + 1 samples) -> find_visited_cells -> interpolate_values]
    -> mlp_base 64->128->128->128 ReLU (+ReLU out) (:414-455, 602-603)
    -> density head 128->1 + softplus, direction encoding (NeRFEncoding 3->27) ++ base -> mlp_head
    155->128 ReLU -> rgb head 128->3 + sigmoid (:605-621) -> weights = alpha * transmittance
    (RaySamples.get_weights) -> rgb over white background, accumulation, median depth (:632-662).

nerfstudio is not installed in this environment: layer shapes and activations are taken from the
call sites above plus nerfstudio 0.3.4's public API as recalled (SURVEY.md 8c caveat).  The
arithmetic below is therefore *our* definition; `render_reference` is its plain-PyTorch fp32
statement (runs on CPU tensors with any tracer-like object), `render` the GPU pipeline, and
`use_fused_mlp=True` swaps the PyTorch MLP for the fp32-MFMA HIP kernel (tn_mlp.hip).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

FIELD_DIM = 64
SYNC_FREE_MIN_HITS = 0.85     # render_train: below this (last known) fraction of hitting rays the batch is compacted instead
HIDDEN = 128
DIR_ENC = 27


def direction_encoding(d: torch.Tensor) -> torch.Tensor:
    """NeRFEncoding(in_dim=3, num_frequencies=4, min_freq_exp=0, max_freq_exp=4, include_input=True)
    (model.py:428-434): sin(2*pi*x*f) and sin(2*pi*x*f + pi/2) for f = 2**linspace(0,4,4), then x."""
    freqs = 2.0 ** torch.linspace(0.0, 4.0, 4, dtype=d.dtype, device=d.device)
    scaled = (2.0 * math.pi * d)[..., None] * freqs                      # [...,3,4]
    scaled = scaled.reshape(*d.shape[:-1], 12)
    enc = torch.sin(torch.cat([scaled, scaled + math.pi / 2.0], dim=-1))  # [...,24]
    return torch.cat([enc, d], dim=-1)                                    # [...,27]


class TetraMLP(torch.nn.Module):
    """The shallow MLP + heads of the model (model.py:414-455): default-initialised nn.Linear
    layers, exactly the parameter shapes a reference checkpoint holds."""

    def __init__(self, field_dim: int = FIELD_DIM, hidden: int = HIDDEN):
        super().__init__()
        self.base = torch.nn.ModuleList([torch.nn.Linear(field_dim, hidden), torch.nn.Linear(hidden, hidden),
                                         torch.nn.Linear(hidden, hidden)])
        self.density = torch.nn.Linear(hidden, 1)
        self.head = torch.nn.Linear(DIR_ENC + hidden, hidden)
        self.rgb = torch.nn.Linear(hidden, 3)

    def forward(self, feats: torch.Tensor, dirs: torch.Tensor):
        """feats [..., 64], dirs [..., 3] (per sample) -> sigma [..., 1], rgb [..., 3]."""
        x = feats
        for lin in self.base:
            x = torch.relu(lin(x))
        sigma = torch.nn.functional.softplus(self.density(x))
        h = torch.relu(self.head(torch.cat([direction_encoding(dirs), x], dim=-1)))
        rgb = torch.sigmoid(self.rgb(h))
        return sigma, rgb


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """x rounded to the nearest bf16 value (ties to even), in x's own dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def mlp_forward_bf16_statement(mlp, feats: torch.Tensor, dirs: torch.Tensor, ray_head_bias: Optional[torch.Tensor] = None,
                               dtype=torch.float64):
    """THE definition of the "bf16" arithmetic of the fused MLP kernels (mlp_mode="bf16", C-ABI mode 2; evaluation only).
    feats [..., 64] fp32, dirs [..., 3] per sample, ray_head_bias [..., 128] per sample or None -> sigma [..., 1], rgb [..., 3].

    In each of the four wide layers -- mlp_base layers 0, 1, 2 and mlp_head layer 0, whose input is [direction encoding 27 |
    base 128] -- BOTH operands of every product are rounded to bf16, round to nearest even: the weight (once, when the
    weights are packed) and the layer's input, which is the fp32 activation of the layer before, the fp32 features, or the fp32
    direction encoding.  A product of two bf16 values is exact in fp32; the products are accumulated in fp32, bias and
    ray_head_bias are added in fp32, the ReLU is taken in fp32.  The narrow heads (density 128 -> 1 + softplus, rgb 128 -> 3 +
    sigmoid) read the fp32 activations and run in fp32 with unrounded weights.  Nothing else of the render path changes.

    `dtype` is the precision the SUMS are evaluated in: float64 gives the value every fp32 accumulation order approximates
    (what the tests compare the kernel with), float32 is one such order.  The roundings to bf16 start from fp32 values in
    both: an activation is brought to fp32 before it is rounded."""
    w1, b1, w2, b2, w3, b3, wd, bd, wh, bh, wr, br = (t.detach() for t in mlp_weights(mlp))

    def wide(x, w, b):
        return bf16_round(x.to(torch.float32)).to(dtype) @ bf16_round(w).to(dtype).t() + b.to(dtype)

    x = feats.to(torch.float32)
    for w, b in ((w1, b1), (w2, b2), (w3, b3)):
        x = torch.relu(wide(x, w, b))
    sigma = torch.nn.functional.softplus(x @ wd.to(dtype).t() + bd.to(dtype))
    pre = wide(torch.cat([direction_encoding(dirs.to(torch.float32)), x.to(torch.float32)], dim=-1), wh, bh)
    if ray_head_bias is not None:
        pre = pre + ray_head_bias.to(dtype)
    h = torch.relu(pre)
    rgb = torch.sigmoid(h @ wr.to(dtype).t() + br.to(dtype))
    return sigma, rgb


class Bf16StatementMLP:
    """mlp_forward_bf16_statement in the place of a TetraMLP of render_reference (evaluated in fp32): the whole render path
    with the "bf16" arithmetic stated in PyTorch, for the tests and measurements that need a frame and no kernel under test."""

    def __init__(self, mlp):
        self.mlp = mlp

    def __call__(self, feats, dirs):
        sigma, rgb = mlp_forward_bf16_statement(self.mlp, feats, dirs, dtype=torch.float32)
        return sigma, rgb

    def coarse_sigma(self, feats):
        w = [t.detach() for t in mlp_weights(self.mlp)]
        x = feats
        for l in range(3):
            x = torch.relu(bf16_round(x) @ bf16_round(w[2 * l]).t() + w[2 * l + 1])
        return torch.nn.functional.softplus(x @ w[6].t() + w[7])[..., 0]


def stratified_bins(num_samples: int, t_rand: torch.Tensor) -> torch.Tensor:
    """Train-mode spacing bins of TetrahedraSampler / nerfstudio's UniformSampler (model.py:166-175): every edge of
    linspace(0, 1, S+1) is jittered between the centres of its two neighbouring bins.  t_rand: U[0,1) [R, S+1]."""
    bins = torch.linspace(0.0, 1.0, num_samples + 1, dtype=t_rand.dtype, device=t_rand.device)[None]
    centers = (bins[..., 1:] + bins[..., :-1]) / 2.0
    upper = torch.cat([centers, bins[..., -1:]], -1)
    lower = torch.cat([bins[..., :1], centers], -1)
    return lower + (upper - lower) * t_rand


def spacing_bins(num_samples: int, t_rand: Optional[torch.Tensor], dtype, device) -> torch.Tensor:
    """[1 or R, S+1] spacing bins of the coarse samplers before the map to distances (model.py:166-174): linspace in
    evaluation mode, jittered with `t_rand` [R,S+1] in training mode."""
    if t_rand is None:
        return torch.linspace(0.0, 1.0, num_samples + 1, dtype=dtype, device=device)[None]
    return stratified_bins(num_samples, t_rand)


def uniform_sample_bins(nears: torch.Tensor, fars: torch.Tensor, num_samples: int, t_rand: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R,S+1] euclidean bin edges of nerfstudio's UniformSampler (eval mode; train mode with `t_rand` [R,S+1])."""
    bins = spacing_bins(num_samples, t_rand, nears.dtype, nears.device)
    return bins * fars + (1.0 - bins) * nears


def coarse_samples(nears, fars, num_samples, biased=False, num_visited_cells=None, hit_distances=None, t_rand=None):
    """(euclidean edges [R,S+1], spacing edges [R,S+1]) of the model's coarse sampler as the reference hands them on to
    the PDF sampler and the GradientScaler (`spacing_starts / spacing_ends` of its RaySamples): the UniformSampler keeps
    the spacing bins it drew, the TetrahedraSampler re-derives them from the re-mapped distances (model.py:182)."""
    bins = spacing_bins(num_samples, t_rand, nears.dtype, nears.device)
    edges = bins * fars + (1.0 - bins) * nears
    if biased:
        edges = map_to_biased(num_visited_cells, hit_distances, edges)
        return edges, (edges - nears) / (fars - nears)
    return edges, bins.expand(nears.shape[0], -1)


def biased_sample_bins(nears: torch.Tensor, fars: torch.Tensor, num_samples: int, num_visited_cells: torch.Tensor,
                       hit_distances: torch.Tensor, t_rand: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R,S+1] euclidean bin edges of the biased TetrahedraSampler in eval mode (model.py:111-192):
    the uniform edges are re-mapped so that every visited tetrahedron receives the same share of the
    samples, placed proportionally inside its [t_in, t_out] segment (the mapping stacks the segment
    lengths from the first entry point; negative lengths -- the cell -1 closing segments -- count 0)."""
    return map_to_biased(num_visited_cells, hit_distances, uniform_sample_bins(nears, fars, num_samples, t_rand))


def map_to_biased(num_visited_cells: torch.Tensor, hit_distances: torch.Tensor, uni: torch.Tensor) -> torch.Tensor:
    """map_from_real_distances_to_biased_with_bounds (model.py:111-122) without the in-place clamps."""
    nb = num_visited_cells.long()
    lengths = (hit_distances[..., 1] - hit_distances[..., 0]).clamp_min(0)
    start = hit_distances[..., 0, 0]
    end = torch.gather(hit_distances[..., 1], 1, (nb[:, None] - 1).clamp_min(0)).squeeze(-1)
    rest = (uni - start[:, None]) / (end - start)[:, None] * nb[:, None]
    intervals = rest.floor().clamp_max(nb[:, None] - 1).clamp_min(0)
    rest = rest - intervals
    intervals = intervals.long()
    cum = torch.cumsum(torch.cat((start[:, None], lengths), 1), 1)
    return torch.gather(cum, 1, intervals) + torch.gather(lengths, 1, intervals) * rest


def pdf_sample_bins(spacing_edges: torch.Tensor, weights: torch.Tensor, num_fine: int, nears: torch.Tensor,
                    fars: torch.Tensor, histogram_padding: float = 0.01, eps: float = 1e-5,
                    u_rand: Optional[torch.Tensor] = None, return_spacing: bool = False):
    """[R, S + num_fine + 2] euclidean bin edges of nerfstudio's PDFSampler in eval mode with
    include_original=True (model.py:463,584): inverse-CDF samples of the padded coarse weights at the
    num_fine+1 bin-centred quantiles, merged with the coarse edges and sorted, then mapped back with
    spacing_to_euclidean (x*far + (1-x)*near, model.py:177).  spacing_edges [R,S+1] in [0,1], weights [R,S]."""
    num_bins = num_fine + 1
    w = weights + histogram_padding
    wsum = w.sum(-1, keepdim=True)
    padding = torch.relu(eps - wsum)
    w = w + padding / w.shape[-1]
    wsum = wsum + padding
    pdf = w / wsum
    cdf = torch.min(torch.ones_like(pdf), torch.cumsum(pdf, dim=-1))
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], dim=-1)
    u = torch.linspace(0.0, 1.0 - (1.0 / num_bins), steps=num_bins, dtype=cdf.dtype, device=cdf.device)
    if u_rand is None:   # eval: bin-centred quantiles
        u = (u + 1.0 / (2 * num_bins)).expand(*cdf.shape[:-1], num_bins).contiguous()
    else:                # train_stratified: one uniform draw per quantile bin, u_rand U[0,1) [R, num_fine+1]
        u = (u + u_rand / num_bins).contiguous()
    inds = torch.searchsorted(cdf.contiguous(), u, side="right")
    last = spacing_edges.shape[-1] - 1
    below, above = (inds - 1).clamp(0, last), inds.clamp(0, last)
    cdf0, cdf1 = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    b0, b1 = torch.gather(spacing_edges, -1, below), torch.gather(spacing_edges, -1, above)
    t = torch.clip(torch.nan_to_num((u - cdf0) / (cdf1 - cdf0), 0), 0, 1)
    bins = b0 + t * (b1 - b0)
    bins, _ = torch.sort(torch.cat([spacing_edges, bins], -1), -1)
    edges = bins * fars + (1.0 - bins) * nears
    return (edges, bins) if return_spacing else edges


def ray_weights(sigma: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """RaySamples.get_weights on [R,S] densities and [R,S+1] edges."""
    dd = (edges[:, 1:] - edges[:, :-1]) * sigma
    trans = torch.cumsum(dd[:, :-1], dim=-1)
    trans = torch.cat([torch.zeros_like(dd[:, :1]), trans], dim=-1)      # (of dd, not of trans: one sample leaves trans empty)
    return torch.nan_to_num((1.0 - torch.exp(-dd)) * torch.exp(-trans))


def background_tensor(background, device=None) -> torch.Tensor:
    """[3] fp32 tensor of a grey level (float) or an (r, g, b) triple."""
    if isinstance(background, torch.Tensor):
        return background.detach().reshape(3).to(device=device, dtype=torch.float32)
    if isinstance(background, (int, float)):
        background = (background,) * 3
    return torch.tensor([float(x) for x in background], dtype=torch.float32, device=device)


def composite(sigma: torch.Tensor, rgb: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor,
              background=1.0, clamp: bool = False):
    """RaySamples.get_weights + RGBRenderer(background) + AccumulationRenderer + DepthRenderer(median).
    sigma [R,S,1], rgb [R,S,3], starts/ends [R,S,1].  background: grey level or (r, g, b); clamp = the RGB renderer's
    evaluation mode (nerfstudio RGBRenderer.forward when not training: nan_to_num of the colours, result clamped to [0, 1])."""
    if clamp:
        rgb = torch.nan_to_num(rgb)
    deltas = ends - starts
    dd = deltas * sigma
    alphas = 1.0 - torch.exp(-dd)
    trans = torch.cumsum(dd[..., :-1, :], dim=-2)
    trans = torch.cat([torch.zeros_like(dd[..., :1, :]), trans], dim=-2)   # (of dd, not of trans: one sample leaves trans empty)
    weights = torch.nan_to_num(alphas * torch.exp(-trans))
    acc = weights.sum(-2)
    out_rgb = (weights * rgb).sum(-2) + background_tensor(background, rgb.device) * (1.0 - acc)
    if clamp:
        out_rgb = out_rgb.clamp(0.0, 1.0)
    steps = (starts + ends) / 2.0
    cum = torch.cumsum(weights[..., 0], dim=-1)
    split = torch.full_like(cum[..., :1], 0.5)
    idx = torch.searchsorted(cum.contiguous(), split, side="left").clamp(0, steps.shape[-2] - 1)
    depth = torch.gather(steps[..., 0], -1, idx)
    return out_rgb, acc, depth, weights


def composite_aux_statement(sigma: torch.Tensor, edges: torch.Tensor):
    """(depth_moment [R], distortion_raw [R]) of [R,S] densities on [R,S+1] non-decreasing edges, in the dtype of the inputs: the
    first moment of the ray's weights (the numerator of nerfstudio's DepthRenderer(method="expected")) and the distortion loss of
    mip-NeRF 360 (eq. 15; nerfstudio's losses.lossfun_distortion) on the edges as given, in the literal pairwise O(S^2) form --
    the oracle of tn_composite_aux / tn_composite_backward_aux, which evaluate it in linear time.  The weights are ray_weights'
    (= composite's).  The midpoints are taken RELATIVE TO THE FIRST EDGE, u'_i = ((e_i - e_0) + (e_{i+1} - e_0)) / 2, so that
    fp32 keeps its digits on a ray that starts far from the camera:
        depth_moment   = e_0 sum_i w_i + sum_i w_i u'_i                             (= sum_i w_i (e_i + e_{i+1}) / 2)
        distortion_raw = sum_i sum_j w_i w_j |u'_i - u'_j| + (1/3) sum_i w_i^2 delta_i.
    The edges are constants of the gradient wherever this is differentiated next to the kernels (pass them detached)."""
    w = ray_weights(sigma, edges)
    e0 = edges[:, :1]
    u = ((edges[:, :-1] - e0) + (edges[:, 1:] - e0)) / 2
    delta = edges[:, 1:] - edges[:, :-1]
    depth_moment = e0[:, 0] * w.sum(-1) + (w * u).sum(-1)
    pair = (w[:, :, None] * w[:, None, :] * (u[:, :, None] - u[:, None, :]).abs()).sum((-2, -1))
    return depth_moment, pair + (w * w * delta).sum(-1) / 3


def aux_outputs_of(depth_moment: torch.Tensor, distortion_raw: torch.Tensor, acc: torch.Tensor, edges: torch.Tensor):
    """(expected_depth [r,1], distortion [r,1]) of a ray from the two sums: expected_depth = depth_moment / (accumulation + 1e-10)
    (nerfstudio's "expected" depth without its global clip) and distortion = distortion_raw / (e_S - e_0), 0 where the span is 0
    -- the loss is translation invariant and homogeneous of degree 1, so this is lossfun_distortion on the normalised bins
    (e - e_0) / (e_S - e_0)."""
    span = (edges[:, -1] - edges[:, 0]).detach()
    expected = depth_moment.reshape(-1) / (acc.reshape(-1) + 1e-10)
    dist = torch.where(span > 0, distortion_raw.reshape(-1) / torch.where(span > 0, span, torch.ones_like(span)),
                       torch.zeros_like(span))
    return expected[:, None], dist[:, None]


def aux_start_values(depth: torch.Tensor, acc: torch.Tensor) -> Dict[str, torch.Tensor]:
    """{"expected_depth", "distortion"} [R,1] of rays that meet nothing, from the miss frame's depth and accumulation: the far
    plane and 0."""
    return {"expected_depth": depth.clone(), "distortion": torch.zeros_like(acc)}


TRACE_KEYS = ("num_visited_cells", "visited_cells", "barycentric_coordinates", "hit_distances", "vertex_indices")


def trace_rows(out) -> list:
    """The five row tensors of a trace_rays result, in the order find_visited_cells takes them."""
    return [out[k] for k in TRACE_KEYS]


def bin_centres(edges: torch.Tensor) -> torch.Tensor:
    """[R,S] sample distances of [R,S+1] bin edges: what find_visited_cells is asked to match."""
    return ((edges[:, 1:] + edges[:, :-1]) / 2).contiguous()


def hit_near_far(out, idx: torch.Tensor):
    """([r,1], [r,1]) first entry and last exit distance of the hitting rays `idx` (rows of empty rays are unwritten without
    dense tails: only those of hitting rays are read)."""
    hd = out["hit_distances"]
    return hd[idx, 0, 0][:, None], hd[idx, (out["num_visited_cells"][idx].long() - 1), 1][:, None]


def coarse_sigma(mlp, feats: torch.Tensor) -> torch.Tensor:
    """[R,S] densities of the coarse pass (model.py:577-581): mlp_base + density head + softplus, or the `coarse_sigma` of an
    adapter around other modules (nerfstudio_plugin.ModelMLP)."""
    if hasattr(mlp, "coarse_sigma"):
        return mlp.coarse_sigma(feats)
    x = feats
    for lin in mlp.base:
        x = torch.relu(lin(x))
    return torch.nn.functional.softplus(mlp.density(x))[..., 0]


def median_margin(weights: torch.Tensor) -> torch.Tensor:
    """[R,1] distance of a ray's cumulative weights from the median threshold 0.5: the median depth of a ray is DECIDED
    (independent of round-off in the weights) when this exceeds the accumulated rounding error of the cumulative sum."""
    cum = torch.cumsum(weights[..., 0] if weights.dim() == 3 else weights, dim=-1)
    return (cum - 0.5).abs().min(dim=-1, keepdim=True).values


def _cell_ids(cells: torch.Tensor) -> torch.Tensor:
    """int64 tetrahedron ids of find_visited_cells' "cell_indices" (int32 with -1, or uint32 with 0xFFFFFFFF, for unmatched: both
    come out as invalid ids, negative or >= 2^32 - 1)."""
    return cells.to(torch.int64)


def occupancy_update_statement(occupancy: torch.Tensor, cells: torch.Tensor, sigma: torch.Tensor, decay: float) -> torch.Tensor:
    """Statement of the per-tetrahedron occupancy update (tn_occupancy_update computes it in place, bit for bit):
        occ_new[t] = max(fl32(decay * occupancy[t]), max{ sigma[i] : cells[i] == t })
    occupancy f32 [T]; cells: the matched tetrahedron of every sample (0xFFFFFFFF / -1 = unmatched); sigma: their densities.
    The inner maximum is over nothing -- absent -- for a tetrahedron no sample touches; samples whose cell is unmatched or >= T,
    or whose sigma is not >= 0 (NaN, negative), contribute nothing (an accepted -0 counts as +0); every tetrahedron decays on
    every update; a NaN occupancy stays NaN.  A maximum: the result does not depend on the order of the samples."""
    T = occupancy.numel()
    c = _cell_ids(cells).reshape(-1)
    s = sigma.detach().reshape(-1).to(torch.float32)
    ok = (c >= 0) & (c < T) & (s >= 0)
    decayed = occupancy.detach() * torch.tensor(float(decay), dtype=torch.float32, device=occupancy.device)
    top = torch.full_like(decayed, float("-inf")).scatter_reduce(0, c[ok], s[ok].abs(), "amax", include_self=True)
    return torch.maximum(decayed, top)


def tet_stats_statement(stats, cells, weights, ray_value=None, ray_index=None, count=None):
    """Statement of the per-tetrahedron training statistics (tn_tet_stats_accumulate computes it in place, byte for byte), in
    numpy integers.  Returns stats + the batch as a NEW int64 [T,3] array; `stats` is not changed.
    cells [rows,S]: the matched tetrahedron of every sample (int32 with -1 or uint32 with 0xFFFFFFFF = unmatched); weights f32
    [rows,S]: the COMPOSITE'S OWN weights of these samples (cpp.composite(..., out_weights): an input, because the host's expf is
    not the device's); row q belongs to ray ray_index[q] (None: q) of ray_value f32 [rays] (None: every value 1); only rows
    q < count are read (None: all).
        w^ = w >= 0 ? min(w, 1) : 0;   v^ = v >= 0 ? min(v, 256) : 0                       (NaN, negative, -0 -> 0)
        for every sample with 0 <= cell < T:   stats[cell] += (1, rint(w^ * 2^32), rint(fl32(w^ * v^) * 2^32))
    rint rounds half to even; w^ * 2^32 is exact in fp32; w^ * v^ is ONE fp32 multiply.  Integer sums: the order of the samples
    cannot matter."""
    import numpy as np

    def host(x, dtype=None):
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        return x if dtype is None else x.astype(dtype)

    out = host(stats, np.int64).copy()
    T = out.shape[0]
    c = host(cells)
    c = c.reshape(-1, c.shape[-1]) if c.ndim >= 2 else c.reshape(1, -1)
    if c.dtype.kind == "u":
        c = c.astype(np.int64)
    else:                                     # a signed id names the same 32 bits: -1 is 0xFFFFFFFF, never < T
        c = c.astype(np.int64) & 0xFFFFFFFF if c.dtype.itemsize == 4 else c.astype(np.int64)
    w = host(weights, np.float32).reshape(c.shape)
    rows = c.shape[0] if count is None else min(c.shape[0], int(host(count).reshape(-1)[0]))
    c, w = c[:rows], w[:rows]
    ray = np.arange(rows, dtype=np.int64) if ray_index is None else host(ray_index).reshape(-1)[:rows].astype(np.int64) & 0xFFFFFFFF
    v = np.ones(rows, np.float32) if ray_value is None else host(ray_value, np.float32).reshape(-1)[ray]
    with np.errstate(invalid="ignore"):
        wh = np.where(w >= 0, np.minimum(w, np.float32(1)), np.float32(0)).astype(np.float32)
        vh = np.where(v >= 0, np.minimum(v, np.float32(256)), np.float32(0)).astype(np.float32)
    scale = np.float32(2.0 ** 32)
    qw = np.rint(wh * scale).astype(np.int64)
    qe = np.rint((wh * vh[:, None]).astype(np.float32) * scale).astype(np.int64)
    ok = (c >= 0) & (c < T)
    np.add.at(out[:, 0], c[ok], 1)
    np.add.at(out[:, 1], c[ok], qw[ok])
    np.add.at(out[:, 2], c[ok], qe[ok])
    return out


def tet_stats_scores(stats: torch.Tensor, kind: str = "error") -> torch.Tensor:
    """Per-tetrahedron scores f32 [T] of the statistics i64 [T,3] (plain torch, float64 inside):
        "error"       sum of w^ v^        (stats[:,2] / 2^32)
        "mean_error"  sum of w^ v^ / sum of w^, 0 where the sum of weights is 0
        "weight"      sum of w^           (stats[:,1] / 2^32)
        "hits"        the number of samples matched to the tetrahedron"""
    st = stats.to(torch.float64)
    scale = 2.0 ** -32
    if kind == "error":
        out = st[:, 2] * scale
    elif kind == "mean_error":
        out = torch.where(stats[:, 1] != 0, st[:, 2] / st[:, 1].clamp_min(1.0), torch.zeros_like(st[:, 2]))
    elif kind == "weight":
        out = st[:, 1] * scale
    elif kind == "hits":
        out = st[:, 0]
    else:
        raise ValueError(f'tet_stats_scores: kind must be "error", "mean_error", "weight" or "hits", got {kind!r}')
    return out.to(torch.float32)


def cull_mask_statement(cells: torch.Tensor, occupancy: torch.Tensor, threshold: float) -> torch.Tensor:
    """bool mask, shape of `cells`: True = the sample is CULLED, i.e. its cell is a valid id < T and occupancy[cell] < threshold.
    Unmatched samples stay live (they are evaluated on zero features, as without a field), a NaN occupancy is live (the
    comparison fails), threshold <= 0 culls nothing.  A culled render is the unculled chain with sigma = 0 and rgb = 0 at the
    culled samples of both passes (tn_cull_samples writes the zeros, tn_mlp_forward_gather_indexed skips the samples)."""
    T = occupancy.numel()
    c = _cell_ids(cells)
    if T == 0 or not float(threshold) > 0:
        return torch.zeros(c.shape, dtype=torch.bool, device=cells.device)
    valid = (c >= 0) & (c < T)
    return valid & (occupancy.detach()[c.clamp(0, T - 1)] < float(threshold))


def live_lengths_statement(num_visited_cells: torch.Tensor, visited_cells: torch.Tensor, hit_distances: torch.Tensor,
                           occupancy: torch.Tensor, threshold: float) -> Dict[str, torch.Tensor]:
    """Statement of the LIVE LENGTHS of traced rays, the base of the occupancy-guided sampler (tn_sample_live / tn_live_to_distance
    compute it per ray; dtype-generic: it runs in the dtype of `hit_distances`).  Rows [r,M] / [r,M,2] of r rays, nb =
    num_visited_cells segments each:
        len_k = max(t_out_k - t_in_k, 0);  segment k is LIVE unless cull_mask_statement would cull its cell (invalid ids and a NaN
        occupancy are live, threshold <= 0 makes every segment live);  w_k = len_k for a live segment, else 0;
        cum_0 = 0, cum_{k+1} = cum_k + w_k, L = cum_nb, near = t_in_0.
    The prefix sums are made non-decreasing and exactly flat over every segment of weight 0 whatever the summation rounds to (a
    running maximum over the sums at the segments with w > 0: the identity in exact arithmetic), so that "the first k with
    cum_{k+1} > s" always names a segment with w_k > 0.  A ray with L == 0 (everything culled) counts every segment live: its
    samples are culled later anyway.  A row without a segment has near = 0, L = 1.
    Returns {"w" [r,M], "cum" [r,M+1], "near" [r,1], "length" [r,1] = L, "num_visited" [r,1] int64, "hit_distances"}."""
    hd = hit_distances
    nb = num_visited_cells.long()[:, None]
    M = hd.shape[1]
    inside = torch.arange(M, device=hd.device)[None] < nb
    zero = torch.zeros((), dtype=hd.dtype, device=hd.device)
    lengths = torch.where(inside, (hd[..., 1] - hd[..., 0]).clamp_min(0), zero)
    live = inside & ~cull_mask_statement(visited_cells, occupancy, threshold)

    def sums(w):
        top = torch.cummax(torch.where(w > 0, torch.cumsum(w, 1), zero), 1).values
        return torch.cat([torch.zeros_like(top[:, :1]), top], 1)

    w = torch.where(live, lengths, zero)
    cum = sums(w)
    dead = cum[:, -1:] == 0
    w, cum = torch.where(dead, lengths, w), torch.where(dead, sums(lengths), cum)
    hit = nb > 0
    return {"w": w, "cum": cum, "near": torch.where(hit, hd[:, 0, :1], zero), "length": torch.where(hit, cum[:, -1:], zero + 1),
            "num_visited": nb, "hit_distances": hd}


def live_to_distance_statement(s: torch.Tensor, live: Dict[str, torch.Tensor]):
    """The inverse map of the live-length coordinate (tn_live_to_distance): s [r,n] in [near, near + L] -> (t [r,n] distances,
    slot [r,n] int64 segment indices), `live` from live_lengths_statement:
        s' = clamp(s - near, 0, L);  k = the first segment with cum_{k+1} > s', or the last segment with w_k > 0 when there is none;
        frac = clamp((s' - cum_k) / w_k, 0, 1);  t = min(t_in_k + frac len_k, t_out_k);  slot = k.
    A mapped value lies inside a live segment.  A row without a segment: t = s, slot = 0."""
    w, cum, hd, nb = live["w"], live["cum"], live["hit_distances"], live["num_visited"]
    M = w.shape[1]
    sp = torch.minimum((s - live["near"]).clamp_min(0), live["length"])
    k = torch.searchsorted(cum[:, 1:].contiguous(), sp.contiguous(), right=True)
    last = ((w > 0) * torch.arange(M, device=w.device)[None]).max(1, keepdim=True).values
    k = torch.where(k >= nb, last.expand_as(k), k).clamp(0, M - 1)
    t_in, t_out = torch.gather(hd[..., 0], 1, k), torch.gather(hd[..., 1], 1, k)
    wk = torch.gather(w, 1, k)
    frac = torch.where(wk > 0, ((sp - torch.gather(cum, 1, k)) / wk).clamp(0, 1), torch.zeros_like(sp))
    t = torch.minimum(t_in + frac * (t_out - t_in).clamp_min(0), t_out)
    none = nb == 0
    return torch.where(none, s, t), torch.where(none, torch.zeros_like(k), k)


def live_sample_bins(live: Dict[str, torch.Tensor], num_samples: int, t_rand: Optional[torch.Tensor] = None):
    """The occupancy-guided coarse sampler (tn_sample_live): (s_edges [r,S+1], near_far_live = (near [r,1], near + L [r,1])) --
    the UniformSampler's bins (stratified with `t_rand` [r,S+1]) over the live-length span of every ray.  The edges are
    live-length coordinates: a pass locates live_to_distance_statement(bin_centres(s_edges)) and composites with s_edges, whose
    deltas are the live lengths inside the bins."""
    near, far = live["near"], live["near"] + live["length"]
    return uniform_sample_bins(near, far, num_samples, t_rand), (near, far)


def hit_far(out, idx: torch.Tensor) -> torch.Tensor:
    """[r,1] last exit distance of the rays `idx` of a trace result, read in place; 1 for a ray without a segment (the padded
    entries of a batch that misses altogether: their rows may be unwritten)."""
    nb = out["num_visited_cells"][idx].long()
    far = out["hit_distances"][idx, (nb - 1).clamp_min(0), 1]
    return torch.where(nb > 0, far, torch.ones_like(far))[:, None]


def occupancy_from_field(cells: torch.Tensor, field: torch.Tensor, mlp, mode: str = "fp32") -> torch.Tensor:
    """A starting occupancy f32 [T] for a checkpoint that has none: the maximum density over five probes per tetrahedron -- the
    centroid and the four vertices -- through the density-only gather + MLP kernel (cpp.mlp_forward_gather(dirs=None)).
    cells int [T, 4]: the vertex ids of the tetrahedra; field f32 [64, V]; mlp: a TetraMLP or an adapter (mlp_weights).
    A HEURISTIC, not a bound: the field is linear inside a tetrahedron but the density is a ReLU network of it, so the
    density can exceed all five probes in the interior; choose the threshold with a margin, and let training updates
    (render_train(occupancy=, occupancy_decay=)) take over."""
    from . import tetranerf_cpp_extension as cpp

    T, dev = cells.shape[0], field.device
    if T == 0:
        return torch.zeros((0,), dtype=torch.float32, device=dev)
    vi = cells.to(device=dev, dtype=torch.int32).reshape(T, 1, 4).expand(T, 5, 4).contiguous()
    # barycentrics (b1, b2, b3) of the probes, b0 = 1 - sum: centroid, vertex 0, 1, 2, 3
    probes = torch.tensor([[0.25, 0.25, 0.25], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
                          dtype=torch.float32, device=dev)
    bc = probes[None].expand(T, 5, 3).contiguous()
    with torch.no_grad():
        sigma = cpp.mlp_forward_gather(vi, bc, field.detach(), None, [x.detach() for x in mlp_weights(mlp)], 5, mode=mode)
    return sigma.view(T, 5).max(dim=1).values


def vertex_normals(positions: torch.Tensor, triangles: torch.Tensor) -> torch.Tensor:
    """f32 [N, 3]: the area-weighted normal of every mesh vertex -- the sum of (p1-p0) x (p2-p0) over its triangles, normalised;
    (0, 0, 1) where that sum is zero or not finite (a vertex of zero-area triangles only).  Plain torch."""
    p, t = positions, triangles.long()
    n = torch.linalg.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    total = torch.zeros_like(p).index_add_(0, t.reshape(-1), n.repeat_interleave(3, 0))
    length = total.norm(dim=-1, keepdim=True)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=p.dtype, device=p.device)
    return torch.where((length > 0) & torch.isfinite(length), total / length.clamp_min(1e-30), up)


def extract_mesh(xyz: torch.Tensor, cells: torch.Tensor, field: torch.Tensor, mlp, level: float,
                 occupancy: Optional[torch.Tensor] = None, occupancy_threshold: Optional[float] = None, colors: bool = True,
                 mode: str = "fp32", refine_rounds: int = 0) -> Dict[str, torch.Tensor]:
    """The density isosurface of a trained field as a triangle mesh, everything on the device:
    the density AT every vertex from the density-only fused forward on the [64, V] field as stored (cpp.mlp_forward(dirs=None));
    the level set { density = level } of its piecewise-linear interpolant by cpp.isosurface; with `occupancy` f32 [T] and
    `occupancy_threshold` (both or neither) the tetrahedra an evaluation render would cull (cull_mask_statement) are masked out.
    colors: per-vertex colours from the gathering forward (cpp.mlp_forward_gather) at the mesh vertices -- vertex_indices
    (a, b, a, a), barycentrics (t, 0, 0), one sample per ray -- looking AT the surface: dirs = minus the vertex normal.
    xyz f32 [V, 3], cells i32 [T, 4], mlp: a TetraMLP or an adapter (mlp_weights).  Runs under no_grad: nothing here has a gradient.
    NOT the level set of the network with refine_rounds = 0 (the default: nothing below runs and every output is what it was):
    inside a tetrahedron the density is an MLP of linearly interpolated features, the mesh interpolates the vertex densities
    linearly.  refine_rounds = 1..8: cpp.isosurface_refine moves every vertex along its mesh edge onto the network's own level
    set, bracketed to 8^-rounds of the edge (7 density-only samples per vertex and round, in `mode`), BEFORE the colour pass: the
    directions come from the refined normals and the colours are gathered at the refined edge_t; "edge_bracket" and "edge_frozen"
    are added.  Still not covered: a tetrahedron whose four vertex densities lie on one side is never visited (thin features
    between vertices stay missing); the triangles are chords of the surface (the enclosed volume can shrink); of several crossings
    on one edge the one nearest the smaller id is taken; zero-area triangles are kept.
    Open where the surface reaches the hull or a masked tetrahedron.
    Returns cpp.isosurface's dict plus "densities" f32 [V], "directions" f32 [N, 3] and "colors" f32 [N, 3] in [0, 1] (the last two
    None with colors=False).  Blocks on the two read-backs of cpp.isosurface."""
    from . import tetranerf_cpp_extension as cpp

    if (occupancy is None) != (occupancy_threshold is None):
        raise ValueError("extract_mesh: occupancy and occupancy_threshold come together (both or neither)")
    with torch.no_grad():
        w = [x.detach() for x in mlp_weights(mlp)]
        densities = cpp.mlp_forward(field.detach(), None, w, 1, mode=mode)
        mask = None
        if occupancy is not None and float(occupancy_threshold) > 0:
            mask = (~(occupancy.detach() < float(occupancy_threshold))).to(torch.uint8)
        out = cpp.isosurface(xyz.detach(), cells, densities, level, mask)
        if int(refine_rounds) != 0:
            out = cpp.isosurface_refine(out, xyz.detach(), densities, level, field.detach(), w, refine_rounds, mode=mode)
        out["densities"], out["directions"], out["colors"] = densities, None, None
        N = out["positions"].shape[0]
        if colors:
            dirs = -vertex_normals(out["positions"], out["triangles"])
            rgb = torch.zeros((0, 3), dtype=torch.float32, device=field.device)
            if N:
                ev = out["edge_vertices"]
                vi = torch.stack([ev[:, 0], ev[:, 1], ev[:, 0], ev[:, 0]], 1).contiguous()
                bc = torch.stack([out["edge_t"], torch.zeros_like(out["edge_t"]), torch.zeros_like(out["edge_t"])], 1).contiguous()
                rgb = cpp.mlp_forward_gather(vi, bc, field.detach(), dirs.contiguous(), w, 1, mode=mode)[1]
            out["directions"], out["colors"] = dirs, rgb
    return out


def render_reference(tracer, interpolate_values, field: torch.Tensor, mlp: TetraMLP, origins: torch.Tensor,
                     directions: torch.Tensor, num_samples: int = 256, max_ray_triangles: int = 512,
                     far_plane: float = 1000.0, num_fine_samples: int = 0, biased: bool = False,
                     background=1.0, occupancy: Optional[torch.Tensor] = None,
                     occupancy_threshold: Optional[float] = None, occupancy_sampler: bool = False,
                     aux_outputs: bool = False) -> Dict[str, torch.Tensor]:
    """Plain-PyTorch statement of the render path in EVALUATION mode (model.py:520-662 with `self.training == False`: the
    samplers do not jitter, the RGB renderer sanitises and clamps); `tracer` needs trace_rays / find_visited_cells
    returning tensors, `interpolate_values(vi, bc, field)` the gather.  Pinned by the reference's own `get_outputs`
    executed from its file (tests/test_reference_model.py).
    occupancy f32 [T] + occupancy_threshold (both or neither): the CULLED render -- sigma = 0 and rgb = 0 at the samples
    cull_mask_statement names, in both passes: the coarse weights, hence the PDF samples, see the masked densities, the final
    composite the masked final samples.
    occupancy_sampler (with an occupancy): the occupancy-guided coarse sampler in the place of the uniform / biased one --
    live_sample_bins places the S bins over the live length of every ray, both passes locate
    live_to_distance_statement(bin_centres(s_edges)), the PDF sampler and the composite run on the live-length edges, and the
    median depth is mapped back to a distance.
    aux_outputs: also "expected_depth" and "distortion" [R,1] of the final pass, from composite_aux_statement (far_plane and 0 on
    rays that meet nothing); refused together with occupancy_sampler, as in TetraRenderer.render."""
    if aux_outputs and occupancy_sampler:
        raise RuntimeError(AUX_WITH_LIVE_SAMPLER)
    if (occupancy is None) != (occupancy_threshold is None):
        raise RuntimeError("occupancy and occupancy_threshold go together: pass both or neither")
    if occupancy_sampler and occupancy is None:
        raise RuntimeError("occupancy_sampler needs occupancy and occupancy_threshold: the field the samples follow")
    out = tracer.trace_rays(origins.contiguous(), directions.contiguous(), max_ray_triangles)
    nv = out["num_visited_cells"]
    nears = out["hit_distances"][:, 0, 0][:, None]
    fars = torch.gather(out["hit_distances"][:, :, 1], 1, (nv[:, None].long() - 1).clamp_min(0))
    ray_mask = nv > 0
    R = origins.shape[0]
    rgb = background_tensor(background, origins.device).expand(R, 3).contiguous()   # get_background_color (model.py:504-518,642)
    acc = torch.zeros((R, 1), dtype=torch.float32, device=origins.device)
    depth = torch.full((R, 1), far_plane, dtype=torch.float32, device=origins.device)
    margin = torch.full((R, 1), 0.5, dtype=torch.float32, device=origins.device)   # test aid: see median_margin
    aux = aux_start_values(depth, acc) if aux_outputs else {}
    if bool(ray_mask.any()):
        lists = [x[ray_mask].contiguous() for x in trace_rows(out)]
        near_r, far_r = nears[ray_mask], fars[ray_mask]

        culled = None     # [r, S] of the current pass, with an occupancy

        live = live_lengths_statement(lists[0], lists[1], lists[3], occupancy, occupancy_threshold) if occupancy_sampler else None

        def features(edges):
            nonlocal culled
            centres = bin_centres(edges)
            if live is not None:
                centres = live_to_distance_statement(centres, live)[0].contiguous()
            traced = tracer.find_visited_cells(*lists, centres)
            if occupancy is not None:
                culled = cull_mask_statement(traced["cell_indices"], occupancy, occupancy_threshold)
            return interpolate_values(traced["vertex_indices"], traced["barycentric_coordinates"], field)

        if live is None:
            edges, spacing = coarse_samples(near_r, far_r, num_samples, biased, lists[0], lists[3])
        else:
            edges, (near_r, far_r) = live_sample_bins(live, num_samples)
            spacing = (edges - near_r) / (far_r - near_r)
        feats = features(edges)
        if num_fine_samples > 0:
            sigma_c = coarse_sigma(mlp, feats)
            if culled is not None:
                sigma_c = torch.where(culled, torch.zeros_like(sigma_c), sigma_c)
            edges = pdf_sample_bins(spacing, ray_weights(sigma_c, edges), num_fine_samples, near_r, far_r)
            feats = features(edges)
        starts, ends = edges[:, :-1, None], edges[:, 1:, None]
        dirs = directions[ray_mask][:, None, :].expand(-1, edges.shape[1] - 1, -1)
        sigma, col = mlp(feats, dirs)
        if culled is not None:
            sigma = torch.where(culled[..., None], torch.zeros_like(sigma), sigma)
            col = torch.where(culled[..., None], torch.zeros_like(col), col)
        rgb_r, acc_r, depth_r, w_r = composite(sigma, col, starts, ends, background=background, clamp=True)
        if live is not None:
            depth_r = live_to_distance_statement(depth_r, live)[0]
        rgb[ray_mask] = rgb_r
        acc[ray_mask] = acc_r
        depth[ray_mask] = depth_r
        margin[ray_mask] = median_margin(w_r)
        if aux_outputs:
            aux["expected_depth"][ray_mask], aux["distortion"][ray_mask] = aux_outputs_of(*composite_aux_statement(sigma[..., 0], edges), acc_r, edges)
    return {"rgb": rgb, "accumulation": acc, "depth": depth, "ray_mask": ray_mask, "depth_margin": margin, **aux}


class GradientScaler(torch.autograd.Function):
    """Radiance-field gradient scaling of the `tetra-nerf` configuration (model.py:195-205, applied :625-630):
    identity forward; the gradients of colours and densities are multiplied by clamp(ray_dist^2, 0, 1)."""

    @staticmethod
    def forward(ctx, colors, sigmas, ray_dist):
        ctx.save_for_backward(ray_dist)
        return colors, sigmas, ray_dist

    @staticmethod
    def backward(ctx, grad_colors, grad_sigmas, grad_ray_dist):
        (ray_dist,) = ctx.saved_tensors
        scaling = torch.square(ray_dist).clamp(0, 1)
        return grad_colors * scaling, grad_sigmas * scaling, grad_ray_dist


def _node_modes(weights):
    """(weights12, mode, adjoint_mode, dw_mode, num_modes) of what trails a fused MLP node's arguments: the 12 weight tensors,
    optionally followed by the forward's mode, then the dX chain's, then the weight-gradient GEMMs' ("fp32" when absent)."""
    num_modes = len(weights) - 12
    mode, adjoint_mode, dw_mode = (tuple(weights[12:]) + ("fp32",) * 3)[:3]
    return weights[:12], mode, adjoint_mode, dw_mode, num_modes


def _fused_mlp_forward(ctx, listed, vertex_indices, barycentric_coordinates, field, dirs, samples_per_ray, ray_head_bias, weights):
    """forward of both fused MLP nodes; listed: None, or the (live, n_live, out) of _FusedMlpCulledFunction"""
    from . import tetranerf_cpp_extension as cpp

    weights, mode, ctx.adjoint_mode, ctx.dw_mode, ctx.num_modes = _node_modes(weights)
    ctx.has_bias = ray_head_bias is not None
    if listed is None:
        sigma, rgb, saved = cpp.mlp_forward_gather_train(vertex_indices, barycentric_coordinates, field, dirs, list(weights),
                                                         int(samples_per_ray), ray_head_bias=ray_head_bias, mode=mode)
    else:
        live, n_live, out = listed
        sigma, rgb, saved = cpp.mlp_forward_gather_train_indexed(live, n_live, vertex_indices, barycentric_coordinates, field, dirs,
                                                                 list(weights), int(samples_per_ray), ray_head_bias=ray_head_bias,
                                                                 mode=mode, sigma=out[0], rgb=out[1])
    # the outputs go through save_for_backward (which knows how to hold a node's own outputs); `saved` must not
    # reference them: node -> saved -> output -> grad_fn -> node is a cycle no collector sees through, i.e. 5 GB
    # leaked per iteration
    saved.sigma = saved.rgb = None
    ctx.save_for_backward(vertex_indices, barycentric_coordinates, field, dirs, sigma, rgb, *weights)
    ctx.saved = saved
    return sigma, rgb


def _fused_mlp_backward(ctx, d_sigma, d_rgb, leading=0):
    """backward of both fused MLP nodes (cpp.mlp_backward tells the compact saves of a listed forward by their type); leading:
    how many inputs without a gradient the node has in front of vertex_indices"""
    from . import tetranerf_cpp_extension as cpp

    vi, bc, field, dirs, sigma, rgb, *weights = ctx.saved_tensors
    saved = ctx.saved          # (kept: a second backward through a retained graph reads the same activations)
    need_bary, need_dirs = ctx.needs_input_grad[leading + 1], ctx.needs_input_grad[leading + 3]
    res = cpp.mlp_backward(saved, vi, bc, field, dirs, list(weights), sigma, rgb, d_sigma.contiguous(), d_rgb.contiguous(),
                           want_ray_head_grad=ctx.has_bias or need_dirs, want_bary_grad=need_bary,
                           adjoint_mode=ctx.adjoint_mode, dw_mode=ctx.dw_mode)
    grad_field, grads = res[0], res[1]
    # the per-ray head bias (appearance embedding): its gradient = per-ray sums of the head pre-activation's gradient
    d_head = res[2] if (ctx.has_bias or need_dirs) else None
    grad_bary = res[-1].view_as(bc) if need_bary else None
    grad_dirs = None
    if need_dirs:
        # the view direction enters through the head layer's per-ray term Wh[:, :27] enc(dir): the same per-ray sums times
        # those columns, chained through the Jacobian of the encoding (recomputed: 27 values per ray)
        g_enc = d_head @ weights[8][:, :DIR_ENC]
        with torch.enable_grad():
            d_leaf = dirs.detach().requires_grad_(True)
            (grad_dirs,) = torch.autograd.grad(direction_encoding(d_leaf), d_leaf, g_enc)
    return ((None,) * leading + (None, grad_bary, grad_field, grad_dirs, None, d_head if ctx.has_bias else None, *grads)
            + (None,) * ctx.num_modes)


class _FusedMlpFunction(torch.autograd.Function):
    """gather + MLP + heads as ONE autograd node: forward = tn_mlp_forward_gather_train_ex (`mode`: "fp32" or "bf16x3"; saves the
    layer inputs and the ReLU masks, 2.3 KB per sample), backward = tn_mlp_backward_ex + tn_mlp_param_grads_ex +
    tn_interpolate_values_backward (dX chain and weight gradients on the fp32 matrix cores, nothing recomputed; with the adjoint
    mode "bf16x3" the four matrix products of the dX chain run on the bf16 matrix cores; with the weight-gradient mode "bf16x3" so
    do the four weight-gradient GEMMs, both operands split as they are staged).  Gradients flow to the field and the 12
    weight tensors, and -- when they require it -- to the barycentrics (tn_interpolate_values_backward_bary_vm on the same
    d x0 rows; the vertex indices are constants) and to the view directions (through the head layer's per-ray term).
    `weights`: the 12 tensors and up to three modes (_node_modes)."""

    @staticmethod
    def forward(ctx, vertex_indices, barycentric_coordinates, field, dirs, samples_per_ray, ray_head_bias, *weights):
        return _fused_mlp_forward(ctx, None, vertex_indices, barycentric_coordinates, field, dirs, samples_per_ray, ray_head_bias, weights)

    @staticmethod
    def backward(ctx, d_sigma, d_rgb):
        return _fused_mlp_backward(ctx, d_sigma, d_rgb)


class _FusedMlpCulledFunction(torch.autograd.Function):
    """_FusedMlpFunction on the listed samples only (occupancy-culled training): forward = tn_mlp_forward_gather_train_indexed over
    `live[:n_live]` (cpp.cull_samples' ascending list; n_live a host integer), which stores into `out` = (sigma [n], rgb [n, 3]) --
    the buffers cull_samples zeroed at the culled samples -- and saves 2.3 KB per LISTED sample; backward = the same adjoint kernels
    on compact columns (cpp.mlp_backward with an MlpSavedIndexed).  sigma = 0 and rgb = 0 are constants at the samples not listed:
    no gradient reaches or leaves them.  `live`, `n_live`, `out` lead the arguments of _FusedMlpFunction."""

    @staticmethod
    def forward(ctx, live, n_live, out, vertex_indices, barycentric_coordinates, field, dirs, samples_per_ray, ray_head_bias, *weights):
        return _fused_mlp_forward(ctx, (live, n_live, out), vertex_indices, barycentric_coordinates, field, dirs, samples_per_ray,
                                  ray_head_bias, weights)

    @staticmethod
    def backward(ctx, d_sigma, d_rgb):
        return _fused_mlp_backward(ctx, d_sigma, d_rgb, leading=3)


class _FusedCompositeFunction(torch.autograd.Function):
    """get_weights + RGB / accumulation / median-depth renderers as one node (tn_composite / tn_composite_backward)."""

    @staticmethod
    def forward(ctx, sigma, rgb, edges, background):
        from . import tetranerf_cpp_extension as cpp

        ctx.save_for_backward(sigma, rgb, edges)
        ctx.background = background     # grey level or (r, g, b); training mode: the RGB renderer does not clamp
        out_rgb, acc, depth = cpp.composite(sigma.detach(), rgb.detach(), edges, ctx.background)
        ctx.mark_non_differentiable(depth)
        return out_rgb, acc, depth

    @staticmethod
    def backward(ctx, d_rgb, d_acc, _d_depth):
        from . import tetranerf_cpp_extension as cpp

        sigma, rgb, edges = ctx.saved_tensors
        # (autograd hands over whatever layout the loss produced -- an expanded scalar after .sum() -- the op takes rows)
        d_sigma, d_col = cpp.composite_backward(sigma, rgb, edges, None if d_rgb is None else d_rgb.contiguous(),
                                                None if d_acc is None else d_acc.reshape(-1).contiguous(), ctx.background)
        return d_sigma, d_col, None, None


AUX_WITH_LIVE_SAMPLER = ("aux_outputs cannot be combined with occupancy_sampler: the composite then runs on live-length edges, and an "
                         "expected depth or a distortion measured in that coordinate is another quantity than the one in distances")


class _FusedCompositeAuxFunction(torch.autograd.Function):
    """_FusedCompositeFunction with two more per-ray outputs, depth_moment and distortion_raw (composite_aux_statement): forward =
    tn_composite + tn_composite_aux, backward = ONE tn_composite_backward_aux call (the cotangents of the two sums are further
    terms of dL/dw).  The edges are constants of the gradient."""

    @staticmethod
    def forward(ctx, sigma, rgb, edges, background):
        from . import tetranerf_cpp_extension as cpp

        ctx.save_for_backward(sigma, rgb, edges)
        ctx.background = background
        ctx.set_materialize_grads(False)      # an output the loss does not use hands None to backward, not a tensor of zeros
        sg = sigma.detach()
        out_rgb, acc, depth = cpp.composite(sg, rgb.detach(), edges, ctx.background)
        depth_moment, distortion_raw = cpp.composite_aux(sg, edges)
        ctx.mark_non_differentiable(depth)
        return out_rgb, acc, depth, depth_moment, distortion_raw

    @staticmethod
    def backward(ctx, d_rgb, d_acc, _d_depth, d_moment, d_dist):
        from . import tetranerf_cpp_extension as cpp

        sigma, rgb, edges = ctx.saved_tensors
        rows = [None if g is None else g.reshape(-1).contiguous() for g in (d_acc, d_moment, d_dist)]
        d_sigma, d_col = cpp.composite_backward(sigma, rgb, edges, None if d_rgb is None else d_rgb.contiguous(), rows[0],
                                                ctx.background, d_depth_moment=rows[1], d_distortion=rows[2])
        return d_sigma, d_col, None, None


def mlp_weights(mlp):
    """The 12 tensors the fused kernels take, in their order: of a TetraMLP, or of any object that provides
    `fused_weights()` (the nerfstudio adapter: nerfstudio_plugin.ModelMLP)."""
    if hasattr(mlp, "fused_weights"):
        return list(mlp.fused_weights())
    b = mlp.base
    return [b[0].weight, b[0].bias, b[1].weight, b[1].bias, b[2].weight, b[2].bias, mlp.density.weight,
            mlp.density.bias, mlp.head.weight, mlp.head.bias, mlp.rgb.weight, mlp.rgb.bias]


def _refuse_aux_with_live_sampler(aux_outputs, occupancy_sampler):
    """The refusal common to every call path; raised in front of everything: an argument error, whatever else the call holds."""
    if aux_outputs and occupancy_sampler:
        raise RuntimeError(AUX_WITH_LIVE_SAMPLER)


def _near_far_columns(near_far):
    """(near [r,1], far [r,1]) of what a coarse sampler returned: the columns of a device sampler's [r,2] tensor, the pair of
    a PyTorch statement as it is."""
    return near_far if isinstance(near_far, tuple) else (near_far[:, 0:1], near_far[:, 1:2])


def _uniform(rand, key, shape, device, generator):
    """The uniform draws `key` of a training call: the caller's (render_train(rand=)), or drawn HERE from `generator` -- the
    reference's order and shapes hold as long as "coarse" is asked for before "fine", and "fine" only when the PDF step runs."""
    given = rand.get(key)
    return torch.rand(shape, device=device, generator=generator) if given is None else given


# The scatters of per-ray rows (a dict by output name) into a frame, in the frame's key order.  They stay apart: the first works
# in place behind a composite that wrote its three outputs itself, the second is differentiable and never reads the count, the
# third follows a compaction on the host (training: differentiable; evaluation: in place).

def _scatter_counted_(frame, rows, order, count):
    """render(): rows [R, .] in the order of `order` (a permutation of the rays), of which the first count[0] (on the device)
    are real -- the others hold whatever their buffers held and are replaced by the frame's own values.  In place."""
    valid = (torch.arange(order.numel(), device=order.device) < count)[:, None]
    for key, row in rows.items():
        frame[key].index_copy_(0, order, torch.where(valid, row, frame[key]))


def _scatter_padded(frame, rows, order, valid):
    """Sync-free training: rows [R, .] of the hitting rays first, then padded entries (valid [R,1] False) that get the frame's
    miss values; `order` is a permutation of the rays, so every row is written once.  Differentiable: a frame of new tensors."""
    return {**frame, **{key: frame[key].index_copy(0, order, torch.where(valid, row, frame[key])) for key, row in rows.items()}}


def _scatter_compacted(frame, rows, idx):
    """Training after a compaction on the host: rows [r, .] of the hitting rays `idx`.  Differentiable: a frame of new tensors."""
    return {**frame, **{key: frame[key].index_copy(0, idx, row) for key, row in rows.items()}}


def _scatter_compacted_(frame, rows, idx):
    """Evaluation after a compaction on the host: an indexed store of the rows [r, .] of the hitting rays `idx`, in place."""
    for key, row in rows.items():
        frame[key][idx] = row


def _median_to_distance(depth_rows, to_distance, keep=False):
    """The median depth [r,1] of a call with the occupancy-guided sampler is a live-length coordinate: mapped to a distance
    per ray.  keep: the `out=` form of the map -- rows beyond the device-side count keep what `depth_rows` holds."""
    return to_distance(depth_rows.contiguous(), out=depth_rows.clone() if keep else None)


def _scale_gradients(sigma, col, spacing, capture):
    """GradientScaler on the final samples (model.py:625-630), ray_dist [r,S,1] from the spacing bins [r,S+1] of their edges
    -> (sigma, col) with scaled gradients; capture receives ray_dist."""
    ray_dist = (spacing[:, 1:] + spacing[:, :-1])[..., None]
    if capture is not None:
        capture["ray_dist"] = ray_dist
    col, sg, _ = GradientScaler.apply(col, sigma[..., None], ray_dist)
    return sg[..., 0], col


class _SyncFreeDecision:
    """Which form the next render_train batch takes, decided WITHOUT a host synchronisation.  The sync-free form pays for rays
    that miss (padded entries are computed and discarded), so the hit count of a sync-free batch is read back asynchronously --
    `pinned` (a one-element pinned int32 buffer) + `event`, never waited for -- and while the last known `fraction` of hitting
    rays lies below the renderer's threshold the batches take the compacting form, which knows its count on the host anyway,
    until the fraction recovers.  Rules: the decision is made on the last KNOWN fraction; there is no second copy while one is
    pending (the buffer is busy); the count of an older batch never overrides one the host has seen since."""

    def __init__(self):
        self.pinned, self.event, self.fraction = None, None, 1.0
        self.pending, self.host_id, self.batch_id = None, 0, 0     # (batch id, rays) of the copy in flight; last batch counted on the host

    def begin_batch(self, min_hits: float) -> bool:
        """A batch starts: take in a read-back that has landed -- whatever form this batch takes: a renderer that alternates
        between the forms must not decide on a stale fraction -- and tell whether the last known fraction allows the sync-free form."""
        self.batch_id += 1
        if self.pending is not None and self.event.query():
            (issued, rays), self.pending = self.pending, None
            if issued > self.host_id:
                self.fraction = float(self.pinned[0]) / max(float(rays), 1.0)   # of an EARLIER batch
        return self.fraction >= min_hits

    def start_copy(self, count, rays, stream):
        """Sync-free batch: `count` (a one-element device tensor, as the compaction left it) of `rays` goes to the pinned buffer
        as it is -- one copy on `stream` -- unless a copy is in flight."""
        if self.pinned is None:
            self.pinned, self.event = torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event()
        if self.pending is None:
            self.pinned.copy_(count, non_blocking=True)
            self.event.record(stream)
            self.pending = (self.batch_id, rays)

    def host_counted(self, hits, rays):
        """Compacting batch: the host knows the fraction."""
        self.fraction, self.host_id = hits / max(rays, 1), self.batch_id


class TetraRenderer:
    """GPU render path: HIP tracer/matcher/gather (+ optionally the fused fp32-MFMA MLP and the
    composite kernel).  With `fused=False` the MLP and the composite run in PyTorch on the GPU."""

    def __init__(self, tracer, field: torch.Tensor, mlp: TetraMLP, num_samples: int = 256,
                 max_ray_triangles: int = 512, fused: bool = True, far_plane: float = 1000.0,
                 num_fine_samples: int = 0, biased: bool = False, dense_tails: bool = False, fused_pass="auto",
                 mlp_mode: str = "fp32", background=1.0, cache_field: bool = True, device_samplers: bool = True,
                 interpolate_values=None, sync_free_train: bool = True, sync_free_min_hits: float = None,
                 bin_rays: bool = False, train_mlp_mode: str = "fp32", train_adjoint_mode: str = "fp32",
                 train_dw_mode: str = "fp32", train_occupancy_threshold: Optional[float] = None):
        from . import tetranerf_cpp_extension as cpp

        # render_train(occupancy=...) without an occupancy_threshold of its own culls below this one (None: training is not culled)
        self.train_occupancy_threshold = None if train_occupancy_threshold is None else float(train_occupancy_threshold)
        # incoherent batches (random pixels over many cameras): the tracer walks the rays in a locality order of its own
        # and still writes row r for ray r (trace_rays(bin_rays=True): the same rows, bit for bit)
        self.bin_rays = bool(bin_rays)

        # render_train without a host synchronisation (see there); False: compact the hitting rays with torch.nonzero
        self.sync_free_train = bool(sync_free_train)
        # below this last known fraction of hitting rays the next batches take the compacting form (_SyncFreeDecision)
        self._sync_free = _SyncFreeDecision()
        self.sync_free_min_hits = SYNC_FREE_MIN_HITS if sync_free_min_hits is None else float(sync_free_min_hits)

        self.cpp = cpp
        self.tracer, self.field, self.mlp = tracer, field, mlp
        # the gather of the UNFUSED statement (render_train(fused=False)): default = the product's autograd op; the CPU
        # tests pass the reference's einsum definition so that the statement runs next to the reference model's body
        self._interpolate_values = interpolate_values
        # arithmetic of the fused forward kernels, per renderer (not process-wide): "fp32" = exact fp32 MFMA chain (what
        # the parity tests pin), "bf16x3" = split-operand bf16 MFMA (opt-in), "bf16" = one bf16 MFMA per product (opt-in, render()
        # only, below the parity bar: mlp_forward_bf16_statement).  mlp_mode is render()'s; render_train has a
        # switch of its own, train_mlp_mode (so that a renderer built with mlp_mode="bf16x3" before the training forward had
        # that mode keeps training in fp32): the forward kernels of a training iteration -- the coarse density pass and the
        # fine forward, saving or not -- run in it.  The adjoint has an arithmetic of its own, train_adjoint_mode, independent of
        # the forward's (all four combinations are valid): "bf16x3" runs the dX chain's four matrix products on the bf16 matrix
        # cores (tn_mlp_backward_ex).  The four weight-gradient GEMMs have a third switch, train_dw_mode, independent of both
        # (all eight combinations are valid): "bf16x3" splits both streamed operands as they are staged and multiplies on the
        # bf16 matrix cores (tn_mlp_param_grads_ex); the bias sums, the rgb head and the gather adjoint are fp32 in all of them
        self.mlp_mode, self.train_mlp_mode, self.train_adjoint_mode, self.train_dw_mode = mlp_mode, train_mlp_mode, train_adjoint_mode, train_dw_mode
        for m in (train_mlp_mode, train_adjoint_mode, train_dw_mode):      # (an unknown mode fails here, not in the first training call)
            cpp._mode(m, inference=False)
        self.train_node_samples = 1 << 22      # render_train: samples per autograd node of the fused MLP (see there)
        # RGBRenderer background: grey level (1.0 white = default config, 0.0 black) or an (r, g, b) triple; render() /
        # render_train() take a per-call override (nerfstudio's BACKGROUND_COLOR_OVERRIDE, model.py:504-518)
        self.background = self._bg(background)
        # samplers as device kernels on the trace rows in place (tn_sample_coarse / tn_sample_pdf): a render is then
        # trace -> [sampler -> pass] x 2 with no PyTorch operator in between (False: the PyTorch statements above, ~15
        # small kernels per pass -- the parity definition, kept for tests and A/B)
        self.device_samplers = bool(device_samplers)
        if cache_field:
            # this renderer owns `field`: cached vertex-major shadow, refreshed per tensor version.  After a write through
            # `.data` call cpp.invalidate_field_cache(field) (see tetranerf_cpp_extension.register_field)
            cpp.register_field(field)
        self.S, self.M, self.fused, self.far_plane = int(num_samples), int(max_ray_triangles), fused, far_plane
        self.S_fine, self.biased = int(num_fine_samples), bool(biased)
        # the render path only reads the trace rows through num_visited_cells, so the constant tails of the
        # dense reference layout need not be written (non-materialising trace: 52 B per segment, not 52*M per ray)
        self.dense_tails = bool(dense_tails)
        # Everything after the trace as ONE persistent launch (tn_render_rays: samplers + match + gather + MLP + composite of both
        # passes) whenever its preconditions hold (_one_launch_ok).  True / "auto": use it; False: the chain of separate kernels
        # (sampler, matcher, gather + MLP, composite per pass), which takes the same device-side ray count -- neither form
        # synchronises with the host.  The persistent kernel separates the stages in time inside one launch and runs the chain's
        # own device functions, so its frame is bit-identical to the chain's (DESIGN.md 4.5 has the history of the forms).
        self.fused_pass = fused_pass if fused_pass == "auto" else bool(fused_pass)

    @property
    def _hit_fraction(self):
        """last known fraction of hitting rays of a render_train batch (_SyncFreeDecision)"""
        return self._sync_free.fraction

    def _trace(self, origins, directions):
        """trace_rays; compact rows (a PER-CALL flag of the op: the tracer may be shared with other threads) unless this
        renderer was asked for the dense reference rows."""
        o, d = origins.contiguous(), directions.contiguous()
        kw = {}
        if not self.dense_tails and getattr(self.tracer, "supports_compact_rows", False):
            kw["compact_rows"] = True
        if self.bin_rays and getattr(self.tracer, "supports_bin_rays", False):
            kw["bin_rays"] = True
        return self.tracer.trace_rays(o, d, self.M, **kw)

    @staticmethod
    def _background_rows(R, bg, dev):
        """[R,3] rows of the background colour (get_background_color, model.py:504-518,642) without a host->device copy."""
        if isinstance(bg, (int, float)):
            return torch.full((R, 3), float(bg), dtype=torch.float32, device=dev)
        rows = torch.empty((R, 3), dtype=torch.float32, device=dev)
        for c in range(3):
            rows[:, c].fill_(float(bg[c]))
        return rows

    def _bg(self, background):
        """A grey level as it is, a colour as an (r, g, b) tuple of floats; None: the renderer's own."""
        if background is None:
            return self.background
        return background if isinstance(background, (int, float)) else tuple(float(x) for x in background_tensor(background).tolist())

    def _miss_frame(self, R, bg, dev):
        """(rgb [R,3], accumulation [R,1], depth [R,1]) of R rays that meet nothing: background, 0, far plane."""
        return (self._background_rows(R, bg, dev), torch.zeros((R, 1), dtype=torch.float32, device=dev),
                torch.full((R, 1), self.far_plane, dtype=torch.float32, device=dev))

    def _frame(self, R, bg, dev, ray_mask, aux_outputs):
        """The result of a call whose rays all miss, in the key order of every result: the miss frame, ray_mask and, with
        aux_outputs, their start values.  The scatters (_scatter_*) write the rows of the hitting rays into it."""
        rgb, acc, depth = self._miss_frame(R, bg, dev)
        return {"rgb": rgb, "accumulation": acc, "depth": depth, "ray_mask": ray_mask, **(aux_start_values(depth, acc) if aux_outputs else {})}

    def _locate(self, lists, edges, ray_index, count=None, to_distance=None):
        """find_visited_cells of the bin centres of `edges` [r,S+1] on the trace rows in place: row i of the result belongs to
        trace row ray_index[i]; count: device-side number of rows to match.  to_distance (the occupancy-guided sampler): the
        edges are live-length coordinates and the centres go through this map first."""
        kw = {} if count is None else {"count": count}
        centres = bin_centres(edges)
        if to_distance is not None:
            centres = to_distance(centres)
        return self.tracer.find_visited_cells(*lists, centres, ray_index=ray_index, **kw)

    def _live_sampler(self, lists, ray_index, occ, t_rand=None, count=None):
        """The occupancy-guided coarse sampler of one call, occ = (occupancy, threshold): (s_edges [r,S+1] in the live-length
        coordinate, near_far_live, to_distance) -- to_distance(values [r,n], out=None) maps live-length values (bin centres,
        edges, a depth) to distances.  Device samplers: cpp.sample_live / cpp.live_to_distance on the trace rows in place
        (near_far_live [r,2]; count: device-side number of rows; `out`: a tensor to store into, so that rows beyond count keep
        what it holds); otherwise the PyTorch statements on the rows of `ray_index` (near_far_live: the pair (near, far))."""
        cpp = self.cpp
        if self.device_samplers:
            rows = (lists[0], lists[1], lists[3], ray_index)
            edges, near_far = cpp.sample_live(*rows, self.S, occ[0], occ[1], t_rand=t_rand, count=count)

            def to_distance(values, out=None):
                if out is not None:
                    out = (out, cpp._empty(tuple(out.shape), dtype=torch.int32, device=out.device))
                return cpp.live_to_distance(values.contiguous(), *rows, occ[0], occ[1], count=count, out=out)[0]
        else:
            idx = ray_index.long()
            live = live_lengths_statement(lists[0][idx], lists[1][idx], lists[3][idx], *occ)
            edges, near_far = live_sample_bins(live, self.S, t_rand)
            edges = edges.contiguous()

            def to_distance(values, out=None):
                return live_to_distance_statement(values, live)[0].contiguous()
        return edges, near_far, to_distance

    def _coarse_samples(self, out, lists, ridx, idx, occ, occupancy_sampler, t_rand=None, count=None):
        """The coarse sampler of a call on the trace `out` (lists = its rows), for the rays ridx i32 [r] (idx: the same as
        int64, read by the PyTorch statement only) -> (edges [r,S+1], near_far, spacing or None, to_distance or None).
        The choice: occupancy-guided (_live_sampler; to_distance: its map, the edges are live-length coordinates), the device
        kernel (cpp.sample_coarse), or the PyTorch statement.  near_far: what _near_far_columns and the PDF step (_pdf_step)
        take.  t_rand [r,S+1]: the stratified draws of a training call; count: device-side number of rows.  spacing: the
        spacing bins of the edges, exact only where the statement of a training call drew them -- an evaluation call carries
        none (its PDF step derives them from the edges)."""
        if occupancy_sampler:
            edges, near_far, to_distance = self._live_sampler(lists, ridx, occ, t_rand=t_rand, count=count)
            return edges, near_far, None, to_distance
        if self.device_samplers:
            return (*self.cpp.sample_coarse(lists[0], lists[3], ridx, self.S, biased=self.biased, t_rand=t_rand, count=count), None, None)
        near_far, spacing = hit_near_far(out, idx), None
        if t_rand is not None:
            edges, spacing = coarse_samples(*near_far, self.S, self.biased, lists[0][idx], lists[3][idx], t_rand)
        elif self.biased:
            edges = biased_sample_bins(*near_far, self.S, lists[0][idx], lists[3][idx])
        else:
            edges = uniform_sample_bins(*near_far, self.S)
        return edges.contiguous(), near_far, spacing, None

    def _pdf_step(self, edges, weights_c, near_far, carried, u_rand=None, count=None):
        """The PDF step of _chain_passes: coarse edges and weights -> the S + S_fine + 2 merged edges.  Device samplers:
        cpp.sample_pdf, over `count` rows (evaluation) or with the stratified draws u_rand [r,S_fine+1] (training).  Otherwise
        the PyTorch statement on spacing bins: those `carried["spacing"]` holds, or (None or absent) derived from the edges.
        The spacing bins of the returned edges are left in `carried` (a dict of the call), where a training call finds them:
        None after the device sampler, which keeps none."""
        if self.device_samplers:
            kw = {"count": count} if u_rand is None else {"u_rand": u_rand.contiguous()}
            edges, spacing = self.cpp.sample_pdf(edges, weights_c, near_far, self.S_fine, **kw), None
        else:
            near_r, far_r = _near_far_columns(near_far)
            spacing = carried.get("spacing")
            if spacing is None:
                spacing = (edges - near_r) / (far_r - near_r)
            edges, spacing = pdf_sample_bins(spacing, weights_c, self.S_fine, near_r, far_r, u_rand=u_rand, return_spacing=True)
        carried["spacing"] = spacing
        return edges.contiguous()

    def _culled_forward(self, traced, S, dirs, w, mode, hb, count, occ):
        """mlp_forward_gather of one pass with an occupancy (occ = (occupancy, threshold)): cull_samples on the pass's matched
        cells writes the zeros of the culled samples and lists the others, mlp_forward_gather_indexed runs the network on those."""
        cpp = self.cpp
        vi, bc, cells = traced["vertex_indices"], traced["barycentric_coordinates"], traced["cell_indices"]
        n, dev = cells.numel(), cells.device
        sigma = cpp._empty((n,), dtype=torch.float32, device=dev)
        rgb = None if dirs is None else cpp._empty((n, 3), dtype=torch.float32, device=dev)
        live, live_count = cpp.cull_samples(cells, occ[0], occ[1], sigma, rgb, samples_per_ray=S, count=count)
        cpp.mlp_forward_gather_indexed(live, live_count, vi, bc, self.field, dirs, w, S, mode=mode, ray_head_bias=hb, count=count,
                                       sigma=sigma, rgb=rgb)
        return sigma if dirs is None else (sigma, rgb)

    def _chain_passes(self, lists, edges, ray_index, w, mode, pdf, count=None, coarse_weights=None, occ=None, to_distance=None):
        """The sample placement of the kernel chain: locate -> [coarse weights -> pdf(edges, weights) -> locate] (the bracket
        with fine samples only).  Coarse weights: gather + mlp_base + density head in one kernel and get_weights in one more,
        unless `coarse_weights(traced, edges)` states them otherwise.  occ = (occupancy, threshold): the culled chain
        (_culled_forward).  to_distance: see _locate.  Returns (traced, final edges)."""
        traced = self._locate(lists, edges, ray_index, count, to_distance)
        if self.S_fine > 0:
            if coarse_weights is None:
                S = edges.shape[1] - 1
                if occ is None:
                    sigma_c = self.cpp.mlp_forward_gather(traced["vertex_indices"], traced["barycentric_coordinates"], self.field,
                                                          None, w, S, mode=mode, count=count)
                else:
                    sigma_c = self._culled_forward(traced, S, None, w, mode, None, count, occ)
                weights_c = self.cpp.composite(sigma_c.view(-1, S), None, edges, count=count)
            else:
                weights_c = coarse_weights(traced, edges)
            edges = pdf(edges, weights_c)
            traced = self._locate(lists, edges, ray_index, count, to_distance)
        return traced, edges

    def _final_forward(self, vi, bc, edges, dirs, w, mode, hb, count=None, occ=None, traced=None):
        """gather + MLP + heads of the final samples in one kernel (no [64, n] feature buffer): sigma [r,S], rgb [r,S,3].
        occ = (occupancy, threshold) with the pass's `traced`: culled (_culled_forward)."""
        S = edges.shape[1] - 1
        if occ is None:
            sigma, col = self.cpp.mlp_forward_gather(vi, bc, self.field, dirs, w, S, mode=mode, ray_head_bias=hb, count=count)
        else:
            sigma, col = self._culled_forward(traced, S, dirs, w, mode, hb, count, occ)
        return sigma.view(-1, S), col.view(-1, S, 3)

    def _render_args(self, background, mlp_mode, occupancy, threshold, occupancy_sampler, aux_outputs):
        """(bg, mode, occ) of a render() call, checked: the background of the call, the arithmetic of its MLP kernels, and
        occ = (occupancy, threshold) of a culled call, None without an occupancy."""
        _refuse_aux_with_live_sampler(aux_outputs, occupancy_sampler)
        bg = self._bg(background)
        mode = self.mlp_mode if mlp_mode is None else mlp_mode
        if (occupancy is None) != (threshold is None):
            raise RuntimeError("occupancy and occupancy_threshold go together: pass both or neither (there is no default "
                               "threshold: what counts as empty is the caller's decision)")
        occ = None
        if occupancy is not None:
            if not self.fused:
                raise RuntimeError("an occupancy is an input of the fused kernel chain (fused=True); the PyTorch statement is "
                                   "render_reference(..., occupancy=, occupancy_threshold=)")
            if self.cpp._mode(mode) == 2:
                raise RuntimeError('mlp_mode="bf16" cannot be combined with an occupancy: the plain-bf16 kernel has no indexed form')
            occ = (occupancy.detach(), float(threshold))
        if occupancy_sampler and occ is None:
            raise RuntimeError("occupancy_sampler needs occupancy and occupancy_threshold: the field the samples follow")
        return bg, mode, occ

    def _train_args(self, fused, position_gradients, mlp_mode, adjoint_mode, dw_mode, occupancy, occupancy_decay, occupancy_threshold,
                    occupancy_sampler, aux_outputs):
        """(occ, modes) of a render_train() call, checked: occ = (occupancy, threshold) of a culled batch (the threshold of
        the call, or the renderer's train_occupancy_threshold), None when training is not culled; modes = the arithmetic of
        the forward kernels, of the recorded node's dX chain and of its weight-gradient GEMMs."""
        _refuse_aux_with_live_sampler(aux_outputs, occupancy_sampler)
        thr = self.train_occupancy_threshold if occupancy_threshold is None and occupancy is not None else occupancy_threshold
        if thr is not None and occupancy is None:
            raise RuntimeError("occupancy_threshold needs the occupancy field it is compared with: pass occupancy=")
        if (occupancy is None) != (occupancy_decay is None) and thr is None:
            raise RuntimeError("occupancy and occupancy_decay go together: pass both or neither (occupancy with an "
                               "occupancy_threshold alone culls without updating)")
        if occupancy_decay is not None and not fused:
            raise RuntimeError("the occupancy update is a kernel of the fused path (fused=True); its statement is occupancy_update_statement")
        occ = None if thr is None else (occupancy.detach(), float(thr))
        if occupancy_sampler and occ is None:
            raise RuntimeError("occupancy_sampler needs occupancy and an occupancy threshold: the field the samples follow")
        if occupancy_sampler and position_gradients:
            raise RuntimeError("occupancy_sampler cannot be combined with position_gradients: the live-to-distance map has no adjoint")
        modes = tuple(own if given is None else given for given, own in
                      ((mlp_mode, self.train_mlp_mode), (adjoint_mode, self.train_adjoint_mode), (dw_mode, self.train_dw_mode)))
        for m in modes:
            self.cpp._mode(m, inference=False)
        return occ, modes

    def _composite_rows(self, sigma, col, edges, bg, how, aux_outputs, clamp=False, into=None):
        """Weights and renderers of the final samples -> the per-ray rows {"rgb" [r,3], "accumulation", "depth" [r,1]} and, with
        aux_outputs, {"expected_depth", "distortion"} [r,1] (aux_outputs_of).  how: "node" -- recorded, ONE autograd node backed
        by the forward / adjoint kernels (_FusedCompositeAuxFunction in the place of _FusedCompositeFunction with aux_outputs);
        "kernels" -- the forward kernels alone (clamp: the RGB renderer's evaluation mode), cpp.composite_aux behind the
        composite with aux_outputs only; "statement" -- composite / composite_aux_statement in PyTorch.
        into = (frame, order i32 [R], order as int64, count): render()'s form of "kernels" -- the composite stores the first
        count[0] (on the device) rows straight into the frame's three tensors at order[.] and only the aux rows, over all R, are
        returned: those from count on hold whatever their buffers held (_scatter_counted_ masks them)."""
        if how == "node":
            rgb, acc, depth, *sums = (_FusedCompositeAuxFunction if aux_outputs else _FusedCompositeFunction).apply(sigma, col, edges, bg)
        elif how == "kernels":
            sigma = sigma.contiguous()
            if into is None:
                rgb, acc, depth = self.cpp.composite(sigma, col.contiguous(), edges, background=bg, clamp=clamp)
            else:
                frame, order, order_l, count = into
                self.cpp.composite(sigma, col, edges, background=bg, clamp=clamp, out=(frame["rgb"], frame["accumulation"], frame["depth"]),
                                   ray_index=order, count=count)
                acc = frame["accumulation"].index_select(0, order_l) if aux_outputs else None
            sums = self.cpp.composite_aux(sigma, edges) if aux_outputs else ()
        else:
            rgb, acc, depth, _ = composite(sigma[..., None], col, edges[:, :-1, None], edges[:, 1:, None], background=bg)
            sums = composite_aux_statement(sigma, edges) if aux_outputs else ()
        rows = {} if into is not None else {"rgb": rgb, "accumulation": acc, "depth": depth}
        if aux_outputs:
            rows["expected_depth"], rows["distortion"] = aux_outputs_of(*sums, acc, edges)
        return rows

    def _one_launch_ok(self, mode, culled=False):
        """tn_render_rays' preconditions: device samplers, the per-wave LDS regions of its ray phases fit, "fp32" or "bf16x3"
        arithmetic (the bf16x3 mode runs x3::forward_group in the MLP phases).  `region` restates launch_render_rays'
        per-wave LDS region (csrc/tn_render_rays.hip).  culled: a call with an occupancy -- the persistent launch does not cull."""
        if culled:
            return False
        region = max(max(2 * self.M, 28) + self.S + 1, (max(2 * self.M, 3 * self.S + self.S_fine + 6) + 2 * self.S + self.S_fine + 2) if self.S_fine else 0) + 4
        return (self.fused_pass is not False and mode in ("fp32", "bf16x3") and self.device_samplers and 8 * 4 * region <= 160 * 1024
                and self.S + self.S_fine + 2 <= 8192)

    @torch.no_grad()
    def render(self, origins: torch.Tensor, directions: torch.Tensor, background=None, ray_head_bias=None,
               mlp_mode: Optional[str] = None, occupancy: Optional[torch.Tensor] = None,
               occupancy_threshold: Optional[float] = None, occupancy_sampler: bool = False, aux_outputs: bool = False,
               capture: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """Evaluation-mode render (model.py:520-662 with `self.training == False`: samplers without jitter, RGB renderer with
        nan_to_num + clamp) -> {"rgb" [R,3], "accumulation", "depth" [R,1], "ray_mask" [R]}.  NO HOST SYNCHRONISATION: the
        reference compacts the hitting rays with boolean indexing (model.py:540-567), a device -> host round trip per chunk
        during which the GPU idles; here they are compacted on the device (tn_compact_hits: their number stays there) and
        every kernel after the trace takes the address of that count.  The stages -- trace, coarse samples, sample placement
        of both passes, network, composite, scatter -- and the forms each call path takes of them: DESIGN.md 4.14.

        origins, directions f32 [R,3]: the rays.

        background: per-call override of the renderer's colour (grey level or (r, g, b)).

        ray_head_bias f32 [R,128] (fused path only): per-ray vector added to mlp_head's pre-activation -- the appearance
        embedding's share of the head layer, Wh[:, 155:] emb (model.py:608-620), made by the caller.

        mlp_mode (fused path; None: the renderer's mlp_mode): arithmetic of the MLP kernels of this call.  "bf16" -- both
        operands of every product of the four wide layers rounded to bf16, fp32 accumulation (mlp_forward_bf16_statement) --
        is the fast one and the only one that does NOT hold the 1e-5 parity bar; it renders through the kernel chain.

        occupancy f32 [num_cells] + occupancy_threshold (opt-in; both or neither, fused path, "fp32" / "bf16x3"): the
        per-tetrahedron occupancy field.  Samples whose tetrahedron lies below the threshold (cull_mask_statement) get
        sigma = rgb = 0 without running the network, in both passes; every other sample gets the bits it gets without an
        occupancy.  Such a call renders through the kernel chain (the persistent launch does not cull).

        occupancy_sampler (opt-in; needs occupancy and occupancy_threshold): the occupancy-GUIDED coarse sampler replaces the
        uniform / biased one of this call.  The S bins are spread over the LIVE length of every ray (cpp.sample_live), both
        passes locate cpp.live_to_distance of the bin centres with the unchanged matcher, the PDF sampler and the composite
        run on the live-length edges -- a delta is the live length inside its bin -- and the median depth is mapped back to a
        distance.  Matcher, cull, indexed forward and composite are the kernels of a culled call.

        aux_outputs (opt-in; off: nothing else changes, not a launch, not an allocation): the result also has
        "expected_depth" and "distortion" [R,1] of the final pass (see render_train; rays that meet nothing: far_plane and
        0), from one more kernel (cpp.composite_aux) behind the composite; a renderer built with fused=False evaluates
        composite_aux_statement.  Such a call renders through the kernel chain, as one with an occupancy does: the
        persistent launch is not touched.  Refused together with occupancy_sampler (AUX_WITH_LIVE_SAMPLER).

        capture (with aux_outputs): receives sigma [R,S], edges [R,S+1], order and count of the final pass (rows from count
        on are not written)."""
        bg, mode, occ = self._render_args(background, mlp_mode, occupancy, occupancy_threshold, occupancy_sampler, aux_outputs)
        cpp, S = self.cpp, self.S
        if not self.fused:
            if ray_head_bias is not None:
                raise RuntimeError("ray_head_bias is an input of the fused kernels; the PyTorch statement takes the model's own modules")
            return render_reference(self.tracer, cpp.interpolate_values, self.field, self.mlp, origins, directions,
                                    S, self.M, self.far_plane, self.S_fine, self.biased, background=bg, aux_outputs=bool(aux_outputs))
        cpp._mode(mode)
        if not self.device_samplers:
            return self._render_host_compaction(origins, directions, bg, ray_head_bias, mode, occ, bool(occupancy_sampler), bool(aux_outputs))
        out = self._trace(origins, directions)
        nv = out["num_visited_cells"]
        R = origins.shape[0]
        res = self._frame(R, bg, origins.device, nv > 0, aux_outputs)
        if R == 0:
            return res
        # the 26 KB trace rows of the hitting rays are NOT compacted (model.py:546-567 copies them with boolean indexing):
        # samplers, matcher and composite read them in place through the ray index
        lists = trace_rows(out)
        order, count = cpp.compact_hits(nv)          # hitting rays first, in ray order; their number stays on the device
        w = mlp_weights(self.mlp)
        d = directions.contiguous()
        if not aux_outputs and self._one_launch_ok(mode, culled=occ is not None):
            cpp.render_rays(lists, order, count, self.field, d, w, S, self.S_fine, self.biased, out=(res["rgb"], res["accumulation"], res["depth"]),
                            background=bg, clamp=True, ray_head_bias=ray_head_bias, mode=mode)
            return res
        # the chain of separate kernels: each is launched over R rows and processes the first `count` of them
        order_l = order.long()
        dirs_o = d.index_select(0, order_l)
        hb = None if ray_head_bias is None else ray_head_bias.index_select(0, order_l).contiguous()
        edges, near_far, _, to_distance = self._coarse_samples(out, lists, order, None, occ, occupancy_sampler, count=count)
        traced, edges = self._chain_passes(lists, edges, order, w, mode, count=count, occ=occ, to_distance=to_distance,
                                           pdf=lambda e, weights_c: self._pdf_step(e, weights_c, near_far, {}, count=count))
        sigma, col = self._final_forward(traced["vertex_indices"], traced["barycentric_coordinates"], edges, dirs_o, w, mode, hb, count,
                                         occ=occ, traced=traced)
        rows = self._composite_rows(sigma, col, edges, bg, "kernels", aux_outputs, clamp=True, into=(res, order, order_l, count))
        if aux_outputs:
            _scatter_counted_(res, rows, order_l, count)
            if capture is not None:
                capture.update(sigma=sigma, edges=edges, order=order, count=count)
        if to_distance is not None:      # (the rows beyond count keep the far plane)
            res["depth"].index_copy_(0, order_l, _median_to_distance(res["depth"].index_select(0, order_l), to_distance, keep=True))
        return res

    @torch.no_grad()
    def _render_host_compaction(self, origins, directions, bg, ray_head_bias, mode, occ, occupancy_sampler, aux_outputs):
        """render() with the PyTorch SAMPLER statements (device_samplers=False: the parity definition of tn_sample_coarse /
        tn_sample_pdf, ~15 small operators per pass) between the HIP kernels, on arguments render() has checked.  Sizes its
        work on the host (torch.nonzero), as the reference does; not the production path."""
        out = self._trace(origins, directions)
        ray_mask = out["num_visited_cells"] > 0
        res = self._frame(origins.shape[0], bg, origins.device, ray_mask, aux_outputs)
        idx = torch.nonzero(ray_mask)[:, 0]
        if idx.numel():
            lists = trace_rows(out)
            ridx = idx.to(torch.int32)
            w = mlp_weights(self.mlp)
            hb = None if ray_head_bias is None else ray_head_bias.index_select(0, idx).contiguous()
            edges, near_far, _, to_distance = self._coarse_samples(out, lists, ridx, idx, occ, occupancy_sampler)
            traced, edges = self._chain_passes(lists, edges, ridx, w, mode, occ=occ, to_distance=to_distance,
                                               pdf=lambda e, weights_c: self._pdf_step(e, weights_c, near_far, {}))
            sigma, col = self._final_forward(traced["vertex_indices"], traced["barycentric_coordinates"], edges,
                                             directions[idx].contiguous(), w, mode, hb, occ=occ, traced=traced)
            rows = self._composite_rows(sigma, col, edges, bg, "kernels", aux_outputs, clamp=True)
            if to_distance is not None:
                rows["depth"] = _median_to_distance(rows["depth"], to_distance)
            _scatter_compacted_(res, rows, idx)
        return res

    def _train_final_pass(self, vi, bc, edges, dirs, w, modes, hb, occ, traced, record, fused):
        """The network on the final samples of a training call -> (sigma [r,S], col [r,S,3]).  record: as autograd nodes backed by
        the saving forward and the adjoint kernels (fused, a graph is being recorded), several beyond train_node_samples; fused
        without a graph: the plain forward kernel; otherwise the PyTorch statement.  occ = (occupancy, threshold): culled."""
        cpp, S, r = self.cpp, edges.shape[1] - 1, vi.shape[0]
        if record and occ is not None:
            # culled: list the live samples (the zeros of the others are written here), read their number back -- the one host
            # synchronisation of a culled batch: it sizes the saves and the adjoint launches -- and run the node on the list;
            # lists beyond train_node_samples go through several nodes, one per range of SLOTS (slots are independent), each with
            # output buffers of its own that are zero wherever it stores nothing: their sum is exact (a softplus / sigmoid output
            # is never -0, the one value x + 0 would change); n_nodes full-size buffers, for the rare list beyond 2^22 samples
            n, dev = r * S, vi.device
            sigma = cpp._empty((n,), dtype=torch.float32, device=dev)
            col = cpp._empty((n, 3), dtype=torch.float32, device=dev)
            live, live_count = cpp.cull_samples(traced["cell_indices"], occ[0], occ[1], sigma, col, samples_per_ray=S)
            n_live = int(live_count.item())
            per_node = max(1, int(self.train_node_samples))
            if n_live > per_node:     # (cull_samples left the live positions unwritten: the first range needs zeros at the others')
                sigma, col = torch.zeros_like(sigma), torch.zeros_like(col)
            sigma, col = _FusedMlpCulledFunction.apply(live, min(n_live, per_node), (sigma, col), vi, bc, self.field, dirs, S, hb, *w, *modes)
            for a in range(per_node, n_live, per_node):
                part = _FusedMlpCulledFunction.apply(live[a:], min(n_live - a, per_node), (torch.zeros_like(sigma), torch.zeros_like(col)),
                                                     vi, bc, self.field, dirs, S, hb, *w, *modes)
                sigma, col = sigma + part[0], col + part[1]
        elif record:
            # the node keeps 2.3 KB per sample from forward to backward (and its backward writes as much again): batches
            # beyond 2^22 samples (nerfstudio trains on 4096 rays) go through several nodes, one per block of rays
            rays_per_node = max(1, int(self.train_node_samples) // S)
            if r <= rays_per_node:
                sigma, col = _FusedMlpFunction.apply(vi, bc, self.field, dirs, S, hb, *w, *modes)
            else:
                parts = [_FusedMlpFunction.apply(vi[a:a + rays_per_node], bc[a:a + rays_per_node], self.field,
                                                 dirs[a:a + rays_per_node], S, None if hb is None else hb[a:a + rays_per_node], *w, *modes)
                         for a in range(0, r, rays_per_node)]
                sigma, col = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        elif fused:               # no graph: the plain forward kernel, nothing saved
            return self._final_forward(vi, bc, edges, dirs, w, modes[0], hb, occ=occ, traced=traced)
        else:
            interpolate_values = self._interpolate_values
            if interpolate_values is None:
                from . import interpolate_values

            feats = interpolate_values(vi, bc, self.field)
            sg, col = self.mlp(feats, dirs[:, None, :].expand(-1, S, -1))
            sigma = sg[..., 0]
            if occ is not None:      # the statement of culled training: zeros as constants at the culled samples
                culled = cull_mask_statement(traced["cell_indices"], *occ)
                sigma = torch.where(culled, torch.zeros_like(sigma), sigma)
                col = torch.where(culled[..., None], torch.zeros_like(col), col)
            return sigma, col
        return sigma.view(-1, S), col.view(-1, S, 3)

    def render_train(self, origins: torch.Tensor, directions: torch.Tensor, gradient_scaling: bool = False,
                     generator: Optional[torch.Generator] = None, rand: Optional[Dict[str, torch.Tensor]] = None,
                     fused: bool = True, capture: Optional[dict] = None, background=None,
                     ray_head_bias: Optional[torch.Tensor] = None, position_gradients: bool = False,
                     vertices: Optional[torch.Tensor] = None, mlp_mode: Optional[str] = None,
                     adjoint_mode: Optional[str] = None, dw_mode: Optional[str] = None,
                     occupancy: Optional[torch.Tensor] = None, occupancy_decay: Optional[float] = None,
                     occupancy_threshold: Optional[float] = None, occupancy_sampler: bool = False,
                     aux_outputs: bool = False, tet_stats: bool = False) -> Dict[str, torch.Tensor]:
        """One training forward (TetrahedraNerf.get_outputs in training mode, model.py:520-662): stratified coarse samples
        (uniform or biased), optional PDF fine pass on the detached coarse weights (nerfstudio's PDFSampler detaches them),
        gather + MLP + heads, optional GradientScaler, weights and renderers (training mode: no clamp) -- differentiable
        w.r.t. the field and the MLP parameters.  Tet membership, the sample distances, near / far and the sampler draws are
        CONSTANTS of the gradient: the coarse pass and the samplers run under no_grad, nothing flows through the tracer's hit
        distances.  Returns render()'s dict.  The stages and the forms each call path takes of them: DESIGN.md 4.14.
        SYNC-FREE form (the renderer's sync_free_train, default for the fused path with device samplers; not with capture= or
        rand=): training batches are pixels of the object, nearly all of their rays hit, so the batch is processed at its
        full size R -- the hitting rays first, in ray order, the tail padded with copies of the first entry, whose (finite)
        results and gradients are masked out -- and nothing on the host ever waits for the ray count: no gap in the launch
        stream between the trace and the samplers.  While the last known fraction of hitting rays lies below
        sync_free_min_hits the batch is compacted with torch.nonzero instead, as the reference does (_SyncFreeDecision).

        origins, directions f32 [R,3]: the rays.

        gradient_scaling: GradientScaler of the `tetra-nerf` configuration on colours and densities (model.py:625-630).

        generator: the stratified draws come from it (None: torch's global generator) in the reference's order and shapes
        -- coarse [r,S+1] first, then fine [r,S_fine+1] when there is a fine pass -- so the same seed gives the reference
        body and this path the same draws.  In the sync-free form that holds when every ray hits (the bench batch, the parity
        tests); with misses the draws are the first `count` rows of an [R,S+1] draw instead of an [r,S+1] draw: the same
        distribution, another stream.

        rand: may carry the uniform draws ("coarse" [r,S+1], "fine" [r,S_fine+1] over the hitting rays) so that two calls see
        the same samples.

        fused=True: the MLP and the composite are single autograd nodes backed by the HIP forward / adjoint kernels (without a
        graph being recorded -- `torch.no_grad()` -- the non-saving forward kernels run instead); fused=False: the plain
        PyTorch statement (autograd through nn.Linear etc.; with device_samplers=False not one HIP kernel above the tracer's
        ops), which is what the parity tests compare against and what tests/test_reference_model.py pins with the
        reference's own get_outputs.

        capture: receives the (non-differentiable) sample placement -- idx, vertex_indices, barycentric_coordinates (the
        matcher's), edges, dirs, near, far, samples_per_ray, cell_indices -- and, with a threshold, culled [r,S]; with
        gradient scaling, ray_dist [r,S,1]; with position gradients, barycentric_positions.

        background: per-call override of the renderer's colour, as in render().

        ray_head_bias f32 [R,128] (fused path only): as in render(); differentiable w.r.t. the caller's tensor.

        position_gradients (opt-in; off: nothing else changes): the gradient also reaches WHERE the samples sit -- the
        `origins` and `directions` handed in (camera pose refinement) and `vertices`.  The final pass's barycentrics go
        through sample_positions_grad before the MLP node (fused) or the gather (fused=False), and the view directions of the
        head layer are differentiable too; everything the opening paragraph calls a constant stays one.  After the vertices
        moved the tracer must follow them: tracer.update_vertices(vertices) while the cells stay (a tracer loaded with
        refittable=True), load_tetrahedra after a re-triangulation, with the host build, and every so often over a long
        optimisation (records and BVH keep the order of the loaded positions).

        vertices f32 [V,3] (with position_gradients; default: the tracer's vertex table): receives a gradient when it
        requires one.

        mlp_mode (fused path; None: the renderer's train_mlp_mode, "fp32" unless chosen otherwise): "bf16x3" runs the forward
        kernels of this call -- the coarse density pass, the recorded fine node and the no-graph fine forward -- in the
        split-operand bf16 arithmetic (same 1e-5 bar against fp32 as in render()); the adjoints take that forward's
        activations and ReLU decisions.

        adjoint_mode (fused path; None: the renderer's train_adjoint_mode, "fp32" unless chosen otherwise; independent of
        mlp_mode): "bf16x3" runs the four matrix products of the recorded node's dX chain in the split-operand bf16
        arithmetic (tn_mlp_backward_ex); the outputs of the call do not depend on it.

        dw_mode (fused path; None: the renderer's train_dw_mode, "fp32" unless chosen otherwise; independent of the other
        two): "bf16x3" runs the four weight-gradient GEMMs of the recorded node in the split-operand bf16 arithmetic
        (tn_mlp_param_grads_ex); neither the outputs nor the field gradient depend on it.

        occupancy f32 [num_cells] (opt-in, fused path; with occupancy_decay, occupancy_threshold or both): the
        per-tetrahedron occupancy field.

        occupancy_decay (opt-in; needs `occupancy`): the field is UPDATED in place once per batch, after the forward, from the
        final pass's matched cells and the detached final densities (cpp.occupancy_update: occupancy[t] = max(decay
        occupancy[t], max sigma in t)); refused with fused=False (the update is a kernel; its statement is
        occupancy_update_statement).  Without a threshold training itself is not culled: the outputs and the gradients of the
        batch do not depend on the field.  (The padded duplicate rays of the sync-free form repeat samples of a real ray:
        harmless to a maximum.)

        occupancy_threshold (opt-in; None: the renderer's train_occupancy_threshold; needs `occupancy`, and makes
        occupancy_decay optional -- cull without update): CULLED training.  ONE definition: the unculled training forward
        with sigma = 0 and rgb = 0 as CONSTANTS at every culled sample of both passes, the culled samples being those
        cull_mask_statement(cells, occupancy, threshold) names -- render()'s rule.  No gradient reaches or leaves a culled
        sample; the samplers, GradientScaler, the composite node, the sync-free padding, position gradients and the three
        arithmetic switches are unchanged and see full-size [r,S] tensors.  Every live sample gets, bit for bit, the outputs
        and per-sample gradients of the unculled kernels; only sums over samples (field gradient, weight gradients, per-ray
        head-bias sums) run over a shorter list of terms.  Fused path: the coarse pass culls as render() does; the final pass
        runs cpp.cull_samples, READS THE LIVE COUNT BACK TO THE HOST -- one host synchronisation per culled batch, which
        sizes the saves (2.3 KB per live sample instead of per sample) and every adjoint launch -- and records a
        _FusedMlpCulledFunction; the update, when asked for, runs after the forward as without a threshold.  fused=False with
        a threshold and no decay is the PyTorch statement (torch.where on the mask in both passes): the oracle of the fused
        path.  A culled tetrahedron contributes sigma = 0, so an update can only decay it: a caller that wants it to come
        back runs some batches unculled (nerfstudio_plugin: occupancy_refresh_every).

        occupancy_sampler (opt-in; needs `occupancy` and a threshold, i.e. a culled batch): the occupancy-GUIDED coarse
        sampler replaces the uniform / biased one of this call, as in render(): stratified bins over the live length of every
        ray, both passes located through the live-to-distance map, PDF sampler and composite (node and statement alike) on
        the live-length edges, the depth mapped back; GradientScaler takes its spacing from the mapped edges,
        (t(s_edges) - near) / (far - near) with the ray's own far.  The sample placement stays a constant of the gradient;
        position_gradients=True is refused: the map has no adjoint.

        aux_outputs (opt-in; off: nothing else changes, not a launch, not an allocation): the result also has, each [R,1] and
        taken from the FINAL pass only,
            "expected_depth" = depth_moment / (accumulation + 1e-10), depth_moment = sum_i w_i (e_i + e_{i+1}) / 2: the first
                moment of the weights, nerfstudio's DepthRenderer(method="expected") without its global clip -- the depth that
                carries a gradient (the median depth does not), what a depth loss is written on;
            "distortion" = distortion_raw / (e_S - e_0), 0 where the span is 0: mip-NeRF 360's distortion loss (eq. 15;
                nerfstudio's losses.lossfun_distortion on the normalised bins (e - e_0) / (e_S - e_0)) of the ray, the
                regulariser against floaters;
        rays that meet nothing get far_plane and 0, and the padded rows of the sync-free form are masked like the other
        outputs.  composite_aux_statement states both sums in the literal pairwise form; fused=False evaluates it (the
        oracle).  Fused, with a graph: ONE node, _FusedCompositeAuxFunction, in the place of _FusedCompositeFunction -- the
        forward adds one kernel (tn_composite_aux, linear in S), the backward is still one kernel
        (tn_composite_backward_aux); the two divisions run in PyTorch on [r] tensors.  Without a graph the forward kernels
        alone run.  The edges stay constants of the gradient.  GradientScaler, culled training, position gradients and the
        three arithmetic switches need no change: the composite node sits behind them and sees full-size [r,S] tensors.
        occupancy_sampler=True is refused with aux_outputs: the composite's edges are then live-length coordinates, and a
        depth or a spread measured in them is another quantity.

        tet_stats (opt-in, fused path; off: nothing else changes, not a launch, not an allocation): the result also has
        "tet_stats_pending", what accumulate_tet_stats needs once the caller knows the error of every ray (the loss is formed
        outside this call, hence the two steps): the final pass's "cell_indices" [r,S], "sigma" [r,S] (detached, contiguous;
        after culling, before GradientScaler), "edges" [r,S+1], "ray_index" i32 [r] (row -> ray of the call) and "count" (the
        device-side number of real rows of the sync-free form, whose padded duplicates must not be counted; None in the
        compacting form); None when no ray hits.  Refused with fused=False (the accumulation is a kernel; its statement is
        tet_stats_statement) and with occupancy_sampler=True (the edges are live-length coordinates there, as for aux_outputs)."""
        if tet_stats and not fused:
            raise RuntimeError("tet_stats is a kernel of the fused path (fused=True); its statement is tet_stats_statement")
        if tet_stats and occupancy_sampler:
            raise RuntimeError("tet_stats cannot be combined with occupancy_sampler: the composite's edges are live-length coordinates there")
        occ, modes = self._train_args(fused, position_gradients, mlp_mode, adjoint_mode, dw_mode, occupancy, occupancy_decay,
                                      occupancy_threshold, occupancy_sampler, aux_outputs)
        cpp, S = self.cpp, self.S
        R, dev = origins.shape[0], origins.device
        rand = rand or {}
        # trace and ray set: the sync-free form (see sync_free_train) while the last known hit fraction allows it, else compaction
        allowed = self._sync_free.begin_batch(self.sync_free_min_hits)
        sync_free = self.sync_free_train and fused and self.device_samplers and capture is None and not rand and R > 0 and allowed
        with torch.no_grad():
            out = self._trace(origins, directions)
            nv = out["num_visited_cells"]
            ray_mask = nv > 0
            if sync_free:
                # order = the hitting rays in ray order, then the others; padded = order with the tail naming order[0]
                order32, count, padded = cpp.compact_hits(nv, want_padded=True)
                order = order32.long()
                valid = torch.arange(R, device=dev) < count     # (count is a one-element device tensor: no read-back)
                idx = padded.long()
                self._sync_free.start_copy(count, R, torch.cuda.current_stream(dev))
            else:
                idx = torch.nonzero(ray_mask)[:, 0]
                if self.sync_free_train:           # this form knows its count on the host anyway
                    self._sync_free.host_counted(idx.numel(), R)
        bg = self._bg(background)
        frame = self._frame(R, bg, dev, ray_mask, aux_outputs)
        if idx.numel() == 0:
            if tet_stats:
                frame["tet_stats_pending"] = None
            return frame
        lists = trace_rows(out)
        ridx = padded if sync_free else idx.to(torch.int32)
        r = idx.numel()
        record = fused and torch.is_grad_enabled()
        # (outside the no_grad block below: an adapter may hand over differentiable VIEWS of its parameters -- the first
        # 155 columns of an mlp_head widened by an appearance embedding, nerfstudio_plugin.ModelMLP.fused_weights)
        w = mlp_weights(self.mlp)
        # coarse samples and the sample placement of both passes: constants of the gradient
        with torch.no_grad():
            t_rand = _uniform(rand, "coarse", (r, S + 1), dev, generator)
            edges, near_far, spacing, to_distance = self._coarse_samples(out, lists, ridx, idx, occ, occupancy_sampler, t_rand=t_rand.contiguous())
            near_r, far_r = _near_far_columns(near_far)
            carried = {"spacing": spacing}     # spacing bins of the current edges (exact only on the PyTorch sampler path)
            traced, edges = self._chain_passes(
                lists, edges, ridx, w, modes[0], occ=occ if fused else None, to_distance=to_distance,
                coarse_weights=None if fused else (lambda traced_c, e: self._coarse_weights_statement(traced_c, e, occ)),
                pdf=lambda e, weights_c: self._pdf_step(e, weights_c, near_far, carried, u_rand=_uniform(rand, "fine", (r, self.S_fine + 1), dev, generator)))
            spacing, S = carried["spacing"], edges.shape[1] - 1
        # directions, per-ray bias of the head layer (appearance embedding; fused path only) and position gradients
        dirs = directions[idx].contiguous()      # (a differentiable index: the view term of position_gradients)
        hb = None if ray_head_bias is None else ray_head_bias.index_select(0, idx).contiguous()
        if hb is not None and not fused:
            raise RuntimeError("ray_head_bias is an input of the fused kernels; the PyTorch statement takes the model's own modules")
        vi, bc = traced["vertex_indices"], traced["barycentric_coordinates"]
        if position_gradients and torch.is_grad_enabled():
            from . import sample_positions_grad

            vertices = self.tracer.tetrahedra_vertices if vertices is None else vertices
            # (the distances `_locate` matched: held constant)
            bc = sample_positions_grad(bc, vi, vertices.reshape(-1, 3), origins[idx], dirs, bin_centres(edges))
            if capture is not None:
                capture["barycentric_positions"] = bc
        if capture is not None:   # the (non-differentiable) sample placement, for tests that restate the rest in float64
            capture.update(idx=idx, vertex_indices=vi, barycentric_coordinates=traced["barycentric_coordinates"], edges=edges, dirs=dirs,
                           near=near_r, far=far_r, samples_per_ray=S, cell_indices=traced["cell_indices"])
            if occ is not None:
                capture["culled"] = cull_mask_statement(traced["cell_indices"], *occ)
        sigma, col = self._train_final_pass(vi, bc, edges, dirs, w, modes, hb, occ, traced, record, fused)
        if occupancy_decay is not None:
            with torch.no_grad():
                cpp.occupancy_update(occupancy, traced["cell_indices"], sigma.detach().contiguous(), occupancy_decay)
        pending = None
        if tet_stats:
            pending = {"cell_indices": traced["cell_indices"], "sigma": sigma.detach().contiguous(), "edges": edges,
                       "ray_index": ridx, "count": count if sync_free else None}
        if gradient_scaling and torch.is_grad_enabled():
            if to_distance is not None:     # distances of the edges, over the ray's own [near, far]
                with torch.no_grad():
                    spacing = (to_distance(edges) - near_r) / (hit_far(out, idx) - near_r)
            sigma, col = _scale_gradients(sigma, col, (edges - near_r) / (far_r - near_r) if spacing is None else spacing, capture)
        rows = self._composite_rows(sigma, col, edges, bg, "node" if record else "kernels" if fused else "statement", aux_outputs)
        if to_distance is not None:
            rows["depth"] = _median_to_distance(rows["depth"], to_distance)
        res = _scatter_padded(frame, rows, order, valid[:, None]) if sync_free else _scatter_compacted(frame, rows, idx)
        if tet_stats:
            res["tet_stats_pending"] = pending
        return res

    def accumulate_tet_stats(self, stats: torch.Tensor, pending: Optional[dict], ray_value: Optional[torch.Tensor]) -> torch.Tensor:
        """Second step of render_train(tet_stats=True): add the batch to `stats` i64 [T,3] in place (cpp.tet_stats_accumulate,
        under no_grad; statement: tet_stats_statement).  pending: the result's "tet_stats_pending" (None -- no ray hit --
        adds nothing); ray_value f32 [R] over ALL rays of the call (e.g. the squared error of every rendered pixel; None: 1)."""
        if pending is None:
            return stats
        with torch.no_grad():
            rv = None if ray_value is None else ray_value.detach().to(torch.float32).reshape(-1).contiguous()
            return self.cpp.tet_stats_accumulate(stats, pending["cell_indices"], pending["sigma"], pending["edges"], ray_value=rv,
                                                 ray_index=pending["ray_index"], count=pending["count"])

    def _coarse_weights_statement(self, traced, edges, occ):
        """The coarse weights of a pass in PyTorch (model.py:577-582): gather, mlp_base + density head, get_weights; occ =
        (occupancy, threshold): zero density at the culled samples."""
        feats_c = (self._interpolate_values or self.cpp.interpolate_values)(traced["vertex_indices"], traced["barycentric_coordinates"], self.field)
        sigma_c = coarse_sigma(self.mlp, feats_c)
        if occ is not None:
            sigma_c = torch.where(cull_mask_statement(traced["cell_indices"], *occ), torch.zeros_like(sigma_c), sigma_c)
        return ray_weights(sigma_c, edges)


class TetraNerfModule(torch.nn.Module):
    """The model's trainable state -- `tetrahedra_field` [64,V] + the MLP -- and its forward as ONE nn.Module, i.e. the
    unit the reference wraps in `DistributedDataParallel(find_unused_parameters=True)` (pipeline.py:53-58: the model is
    replicated, every rank trains on its own rays, the gradients of the field and the MLP are all-reduced).
    `forward(origins, directions)` = TetraRenderer.render_train in training mode (the fused autograd nodes: their
    gradients reach the parameters through the autograd engine, so DDP's reducer hooks see them like any other) and
    TetraRenderer.render otherwise.  With a real nerfstudio the same role is played by the reference's TetrahedraNerf
    after nerfstudio_plugin.install()."""

    def __init__(self, tracer, num_vertices: int, num_samples: int = 256, max_ray_triangles: int = 512,
                 num_fine_samples: int = 256, biased: bool = False, gradient_scaling: bool = False,
                 train_mlp_mode: str = "fp32", train_adjoint_mode: str = "fp32", train_dw_mode: str = "fp32", **renderer_kw):
        super().__init__()
        field = (torch.rand(FIELD_DIM, num_vertices) * 2 - 1) * 1e-4      # model.py:269-271
        field[1:4] = torch.rand(3, num_vertices) * 2 - 1                  # colours, model.py:379-386
        self.tetrahedra_field = torch.nn.Parameter(field)
        self.mlp = TetraMLP()
        self.gradient_scaling = bool(gradient_scaling)
        self._tracer = tracer
        self._renderer_args = (int(num_samples), int(max_ray_triangles))
        self._renderer_kw = dict(num_fine_samples=int(num_fine_samples), biased=bool(biased), train_mlp_mode=train_mlp_mode,
                                 train_adjoint_mode=train_adjoint_mode, train_dw_mode=train_dw_mode, **renderer_kw)
        self._renderer = None

    def renderer(self) -> "TetraRenderer":
        rd = self._renderer
        if rd is None or rd.field is not self.tetrahedra_field:      # (.to(device) replaces the parameter's storage)
            rd = TetraRenderer(self._tracer, self.tetrahedra_field, self.mlp, *self._renderer_args, fused=True, **self._renderer_kw)
            object.__setattr__(self, "_renderer", rd)
        return rd

    def forward(self, origins: torch.Tensor, directions: torch.Tensor) -> Dict[str, torch.Tensor]:
        rd = self.renderer()
        if self.training:
            return rd.render_train(origins, directions, gradient_scaling=self.gradient_scaling)
        return rd.render(origins, directions)
