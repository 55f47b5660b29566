"""The occupancy-guided sampler on the GPU (csrc/tn_live_sampler.hip + ray_live_cum / ray_live_to_distance of csrc/tn_ray_ops.h):
tn_sample_live and tn_live_to_distance against the statements of render.py evaluated in FLOAT64 on the crafted rows of
tests/live_sampler_cases.py (tests/test_live_sampler.py checks those inputs and statements without a GPU), the agreement with the
unchanged matcher, the exact optical depth of a constant density, render(occupancy_sampler=True) bit for bit against the frame
assembled from the ops, render_train(occupancy_sampler=True) against the PyTorch statement under autograd, and the refusals.

Bounds: a multiple of the error `y` of the fp32 torch statement on the device in the same test, with the floor 2^-20 where the
rule of tests/test_ray_stages_gpu.py is used (8 y for a maximum over the rays of a sampler; two correct fp32 evaluations differ
in the order of their prefix sums).  Every check on the MAP is decision-free: a value on the boundary of two live runs may land on
either side of the gap, so (slot, t) is checked through the float64 FORWARD map, not against a reference slot.

Sizes at which the kernels change form: ray_live_cum scans 256 segments per step (4 chunks of 64: the counts 63 / 64 / 65 / 129 /
255 / 256 of the rows), ray_live_to_distance maps 256 values per step, 4 per lane (n = 63 / 64 / 65, 255 / 256 / 257, 513)."""
import importlib

import numpy as np
import pytest
import torch

import live_sampler_cases as cases
from test_occupancy_gpu import _assembled, small_scene            # noqa: F401  (the small Delaunay scene and the uniform culled chain)
from test_train_culled_gpu import GRADS, U, _quad_major, _record_backward, _term_magnitudes
from test_train_gpu import _decode_relu_masks

pytestmark = pytest.mark.gpu

render = importlib.import_module("tetra-nerf_amd.render")
THR = cases.THRESHOLD


def _report(*parts):
    print("live-sampler:", *parts, flush=True)


@pytest.fixture(scope="module")
def crafted(device):
    cpu = cases.live_rows()
    rows = cases.to_device(cpu, device)
    rows["ray_index"] = torch.arange(len(cpu["num_visited"]), dtype=torch.int32, device=device)
    return cpu, rows, cases.live_statement(cpu, torch.float64)


def _row_args(rows):
    return rows["num_visited"], rows["visited_cells"], rows["hit_distances"], rows["ray_index"]


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("S", cases.S_VALUES)
def test_sample_live_vs_float64_statement(tn, device, crafted, S, train):
    cpu, rows, live64 = crafted
    t_cpu = cases.draws(S + 1) if train else None
    want, (_, far64) = render.live_sample_bins(live64, S, None if t_cpu is None else t_cpu.double())
    t_rand = None if t_cpu is None else t_cpu.to(device)
    live32 = cases.live_statement(rows, torch.float32)
    y_edges, (_, y_far) = render.live_sample_bins(live32, S, t_rand)
    y = float(cases.edge_error(torch.cat([y_edges, y_far], 1).cpu(), torch.cat([want, far64], 1), live64).max())
    edges, nf = tn.cpp.sample_live(*_row_args(rows), S, rows["occupancy"], THR, t_rand=t_rand)
    assert edges.shape == (len(cpu["num_visited"]), S + 1) and nf.shape == (len(edges), 2) and bool(torch.isfinite(edges).all())
    hit = cpu["num_visited"] > 0
    first = torch.where(hit, cpu["hit_distances"][:, 0, 0], torch.zeros(()))
    assert torch.equal(nf[:, 0].cpu().view(torch.int32), first.view(torch.int32))            # the first t_in, bit for bit
    assert bool((edges[:, 1:] >= edges[:, :-1]).all())
    miss = torch.nonzero(~hit)[:, 0].to(device)      # rows without a segment: near = 0, L = 1, the plain spacing bins
    bins = render.uniform_sample_bins(torch.zeros(len(miss), 1, device=device), torch.ones(len(miss), 1, device=device), S,
                                      None if t_rand is None else t_rand[miss])
    assert torch.equal(edges[miss], bins.expand(len(miss), S + 1)) and bool((nf[miss] == torch.tensor([0.0, 1.0], device=device)).all())
    e = float(cases.edge_error(torch.cat([edges, nf[:, 1:]], 1).cpu(), torch.cat([want, far64], 1), live64).max())
    bound = max(8 * y, cases.FLOOR)
    _report(f"sample_live S={S} train={train}: err {e:.3e} y32 {y:.3e} bound {bound:.3e}")
    assert e <= bound, (e, y)


def _map_measure(live64, far, s, t, slot, hit):
    """max over the hitting rays of |forward_map64(slot, t) - clamp(s - near, 0, L)| / (L + |far|), far = the ray's last exit (t
    is a distance of up to far: that is the scale its fp32 rounding has)"""
    sp = torch.minimum((s.double() - live64["near"]).clamp_min(0), live64["length"])
    err = (cases.forward_map64(live64, slot, t) - sp).abs() / (live64["length"] + far.double().abs()[:, None])
    return float(err[hit].max())


def _check_map(tn, device, cpu, rows, live64, n, thr, label):
    """decision-free checks of tn_live_to_distance on n values per ray; returns (t, s) on the host"""
    hit = cpu["num_visited"] > 0
    s_cpu = cases.values_in_span(cases.live_statement(cpu, torch.float32, thr), cases.draws(n))
    s = s_cpu.to(device)
    t32, slot32 = render.live_to_distance_statement(s, cases.live_statement(rows, torch.float32, thr))
    far = cases.far_of(cpu)
    y = _map_measure(live64, far, s_cpu, t32.cpu(), slot32.cpu(), hit)
    t, slot = tn.cpp.live_to_distance(s, *_row_args(rows), rows["occupancy"], thr)
    assert t.shape == (len(hit), n) and slot.shape == (len(hit), n) and slot.dtype == torch.int32 and bool(torch.isfinite(t).all())
    t, slot = t.cpu(), slot.cpu().long()
    assert bool((slot[hit] >= 0).all()) and bool((slot[hit] < cpu["num_visited"][hit, None]).all())
    assert bool((torch.gather(live64["w"], 1, slot)[hit] > 0).all())                         # a live slot of positive length
    hd = cpu["hit_distances"]
    t_in, t_out = torch.gather(hd[..., 0], 1, slot), torch.gather(hd[..., 1], 1, slot)
    assert bool((t_in[hit] <= t[hit]).all()) and bool((t[hit] <= t_out[hit]).all())          # fp32 comparisons: bit-wise
    assert torch.equal(t[~hit], s_cpu[~hit]) and not bool(slot[~hit].any())                  # rows without a segment: t = s
    e = _map_measure(live64, far, s_cpu, t, slot, hit)
    bound = max(8 * y, cases.FLOOR)
    _report(f"live_to_distance {label} n={n}: err {e:.3e} y32 {y:.3e} bound {bound:.3e}")
    assert e <= bound, (e, y)
    return t, s_cpu, bound


@pytest.mark.parametrize("n", cases.N_VALUES)
def test_live_to_distance_decision_free(tn, device, crafted, n):
    cpu, rows, live64 = crafted
    _check_map(tn, device, cpu, rows, live64, n, THR, "crafted")
    # threshold 0 on exactly contiguous rows: the live-length coordinate is the distance
    flat_cpu = cases.contiguous(cpu)
    flat = dict(cases.to_device(flat_cpu, device), ray_index=rows["ray_index"])
    live0 = cases.live_statement(flat_cpu, torch.float64, 0.0)
    t, s, bound = _check_map(tn, device, flat_cpu, flat, live0, n, 0.0, "contiguous, threshold 0")
    hit = cpu["num_visited"] > 0
    scale = (live0["length"] + cases.far_of(flat_cpu).double().abs()[:, None])
    assert float(((t.double() - s.double()).abs() / scale)[hit].max()) <= bound


def test_count_is_honoured(tn, device, crafted, monkeypatch):
    cpu, rows, _ = crafted
    R, S, n, k = len(cpu["num_visited"]), 65, 257, 101
    count = torch.tensor([k], dtype=torch.int32, device=device)
    monkeypatch.setattr(tn.cpp, "_POISON", True)          # outputs start as NaN: an unwritten row shows
    edges, nf = tn.cpp.sample_live(*_row_args(rows), S, rows["occupancy"], THR, count=count)
    full, nf_full = tn.cpp.sample_live(*_row_args(rows), S, rows["occupancy"], THR)
    assert torch.equal(edges[:k], full[:k]) and torch.equal(nf[:k], nf_full[:k])
    assert bool(torch.isnan(edges[k:]).all()) and bool(torch.isnan(nf[k:]).all())
    s = full[:, :1].expand(R, n).contiguous()
    t = torch.full((R, n), float("nan"), device=device)
    slot = torch.full((R, n), -7, dtype=torch.int32, device=device)
    got = tn.cpp.live_to_distance(s, *_row_args(rows), rows["occupancy"], THR, count=count, out=(t, slot))
    assert got[0] is t and got[1] is slot
    t_full, slot_full = tn.cpp.live_to_distance(s, *_row_args(rows), rows["occupancy"], THR)
    assert torch.equal(t[:k], t_full[:k]) and torch.equal(slot[:k], slot_full[:k])
    assert bool(torch.isnan(t[k:]).all()) and bool((slot[k:] == -7).all())
    # a permuted ray index reads the rows it names
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3)).to(device)
    e2, nf2 = tn.cpp.sample_live(rows["num_visited"], rows["visited_cells"], rows["hit_distances"], perm.to(torch.int32), S, rows["occupancy"], THR)
    assert torch.equal(e2, full[perm]) and torch.equal(nf2, nf_full[perm])


def _matcher_disagreements(tn, device, tracer, lists, ray_index, occ, thr, edges):
    """samples whose matched cell differs from visited_cells[slot] and whose t is neither bit-equal to that slot's t_in or t_out nor
    in a zero-length slot -> (count of such samples, count of all differing samples)"""
    nv, cells, hd = lists[0], lists[1], lists[3]
    centres = render.bin_centres(edges)
    t, slot = tn.cpp.live_to_distance(centres, nv, cells, hd, ray_index, occ, thr)
    traced = tracer.find_visited_cells(*lists, t, ray_index=ray_index)
    rows = ray_index.long()[:, None].expand_as(slot)
    sl = slot.long()
    want_cell = cells[rows, sl]
    t_in, t_out = hd[rows, sl, 0], hd[rows, sl, 1]
    differ = (traced["cell_indices"] != want_cell) & (nv[ray_index.long()] > 0)[:, None]
    excused = (t == t_in) | (t == t_out) | (t_in == t_out)
    return int((differ & ~excused).sum()), int(differ.sum())


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_matcher_agrees_on_crafted_rows(tn, device, scenes, crafted, train):
    """Exactly contiguous rows (t_out of a segment IS t_in of the next, as a trace writes them; coarse_rows' own segments overlap
    or gap by an ulp of t_in + length, where "the" segment of a distance is not defined).  An exact condition, no tolerance."""
    cpu, rows, _ = crafted
    flat = cases.to_device(cases.contiguous(cpu), device)
    R, S = len(cpu["num_visited"]), 200
    g = torch.Generator().manual_seed(5)
    lists = [flat["num_visited"], flat["visited_cells"], torch.rand(R, cases.M, 2, 3, generator=g).to(device), flat["hit_distances"],
             torch.randint(0, 1000, (R, cases.M, 4), generator=g, dtype=torch.int32).to(device)]
    t_rand = cases.draws(S + 1).to(device) if train else None
    edges, _ = tn.cpp.sample_live(lists[0], lists[1], lists[3], rows["ray_index"], S, rows["occupancy"], THR, t_rand=t_rand)
    tracer = tn.TetrahedraTracer(device)        # (the matcher reads the rows alone; the tracer wants a mesh before any call)
    pts, cells = scenes.random_mesh(60, 1)
    tracer.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    bad, differ = _matcher_disagreements(tn, device, tracer, lists, rows["ray_index"], rows["occupancy"], THR, edges)
    _report(f"matcher agreement, crafted rows train={train}: {differ} samples matched to a neighbour of their slot, {bad} unexcused")
    assert bad == 0


@pytest.mark.parametrize("S", (1, 7, 200))
def test_constant_density_composites_to_the_exact_optical_depth(tn, device, crafted, S):
    cpu, rows, live64 = crafted
    sigma_v = 3.0
    edges, _ = tn.cpp.sample_live(*_row_args(rows), S, rows["occupancy"], THR)
    sigma = torch.full((len(edges), S), sigma_v, device=device)
    got = tn.cpp.composite(sigma, None, edges).sum(-1).cpu().double()
    want = 1 - torch.exp(-sigma_v * live64["length"][:, 0])
    y_edges, _ = render.live_sample_bins(cases.live_statement(rows, torch.float32), S)
    y = float((render.ray_weights(sigma, y_edges).sum(-1).cpu().double() - want).abs().max())
    e = float((got - want).abs().max())
    _report(f"constant density S={S}: err {e:.3e} y32 {y:.3e}")
    assert e <= 4 * y, (e, y)


# ---- frames ------------------------------------------------------------------------------------------------------------------

def _assembled_live(tn, rd, o, d, occ, thr, mode):
    """The frame of render(occupancy_sampler=True) from the ops: sample_live, live_to_distance, _locate, the masked forward,
    composite, sample_pdf, and the depth mapped."""
    cpp, S = tn.cpp, rd.S
    out = rd._trace(o, d)
    lists = render.trace_rows(out)
    rgb, acc, depth = rd._miss_frame(o.shape[0], rd.background, o.device)
    order, count = cpp.compact_hits(out["num_visited_cells"])
    n_hit = int(count)
    w = render.mlp_weights(rd.mlp)
    dirs_o = d.index_select(0, order.long())
    rows = (lists[0], lists[1], lists[3], order)

    def to_distance(values):
        return cpp.live_to_distance(values.contiguous(), *rows, occ, thr, count=count)[0]

    edges, near_far = cpp.sample_live(*rows, S, occ, thr, count=count)
    traced = rd._locate(lists, edges, order, count, to_distance=to_distance)
    if rd.S_fine:
        sigma_c = cpp.mlp_forward_gather(traced["vertex_indices"], traced["barycentric_coordinates"], rd.field, None, w, S, mode=mode,
                                         count=count).view(-1, S)
        sigma_c = torch.where(render.cull_mask_statement(traced["cell_indices"], occ, thr), torch.zeros_like(sigma_c), sigma_c)
        weights_c = cpp.composite(sigma_c.contiguous(), None, edges, count=count)
        edges = cpp.sample_pdf(edges, weights_c, near_far, rd.S_fine, count=count)
        traced = rd._locate(lists, edges, order, count, to_distance=to_distance)
    Sf = edges.shape[1] - 1
    sigma, col = cpp.mlp_forward_gather(traced["vertex_indices"], traced["barycentric_coordinates"], rd.field, dirs_o, w, Sf, mode=mode,
                                        count=count)
    culled = render.cull_mask_statement(traced["cell_indices"], occ, thr)
    sigma = torch.where(culled, torch.zeros_like(culled, dtype=torch.float32), sigma.view(-1, Sf)).contiguous()
    col = torch.where(culled[..., None], torch.zeros_like(col.view(-1, Sf, 3)), col.view(-1, Sf, 3)).contiguous()
    cpp.composite(sigma, col, edges, background=rd.background, clamp=True, out=(rgb, acc, depth), ray_index=order, count=count)
    hit = order.long()[:n_hit]
    depth[hit] = to_distance(depth[order.long()])[:n_hit]
    return {"rgb": rgb, "accumulation": acc, "depth": depth, "culled": int(culled[:n_hit].sum()), "samples": n_hit * Sf,
            "lists": lists, "order": order[:n_hit].contiguous(), "edges": edges[:n_hit].contiguous()}


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("S,S_fine", [(11, 7), (13, 0)])
def test_render_with_the_live_sampler(tn, device, small_scene, monkeypatch, mode, S, S_fine):
    sc = small_scene
    o, d = sc["o"], sc["d"]
    kw = dict(num_fine_samples=S_fine, mlp_mode=mode)
    chain = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], S, 256, fused_pass=False, **kw)
    rd = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], S, 256, **kw)        # fused_pass="auto"
    assert rd._one_launch_ok(mode)
    calls = []
    real = tn.cpp.render_rays
    monkeypatch.setattr(tn.cpp, "render_rays", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device)
    keys = ("rgb", "accumulation", "depth")
    for thr in (0.5, 2.0):
        got = rd.render(o, d, occupancy=occ, occupancy_threshold=thr, occupancy_sampler=True)
        want = _assembled_live(tn, chain, o, d, occ, thr, mode)
        for k in keys:
            assert torch.equal(got[k], want[k]), (thr, k)
        hit = got["ray_mask"]
        assert 0 < int(hit.sum()) < len(o)
        uniform = rd.render(o, d, occupancy=occ, occupancy_threshold=thr)
        if thr == 2.0:       # everything culled: the background frame
            assert torch.all(got["accumulation"] == 0) and torch.all(got["rgb"] == 1.0)
            assert want["culled"] == want["samples"]
        else:
            assert not torch.equal(got["rgb"], uniform["rgb"])
            uni = _assembled(tn, chain, o, d, occ, thr, mode)
            share, uni_share = want["culled"] / want["samples"], uni["culled"] / uni["samples"]
            _report(f"frame S={S}+{S_fine} {mode}: culled share of the final samples {share:.3f} (uniform sampler {uni_share:.3f})")
            assert share < uni_share
            # a mapped depth is a distance inside the ray's span
            nf = render.hit_near_far(rd._trace(o, d), torch.nonzero(hit)[:, 0])
            assert bool((got["depth"][hit] >= nf[0]).all()) and bool((got["depth"][hit] <= nf[1]).all())
            # the matcher agrees with the map's slots on real trace rows: an exact condition
            bad, differ = _matcher_disagreements(tn, device, sc["tr"], want["lists"], want["order"], occ, thr, want["edges"])
            _report(f"matcher agreement, traced rows S={S}+{S_fine}: {differ} samples matched to a neighbour of their slot, {bad} unexcused")
            assert bad == 0
    assert not calls                                                   # never the persistent launch
    # the PyTorch sampler statements between the kernels (device_samplers=False) render the same scene
    host = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], S, 256, device_samplers=False, **kw)
    got_host = host.render(o, d, occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True)
    dev_frame = rd.render(o, d, occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True)
    assert torch.equal(got_host["ray_mask"], dev_frame["ray_mask"]) and bool(torch.isfinite(got_host["rgb"]).all())
    close = ((got_host["rgb"] - dev_frame["rgb"]).abs().amax(1) <= 1e-4).float().mean()
    _report(f"statement samplers vs device samplers S={S}+{S_fine} {mode}: {float(close):.4f} of the rays within 1e-4")
    # the two frames differ in the samplers' last bits only (1e-5 parity of a frame, test_render_gpu.py; 1e-4 leaves room for the
    # ulp the edges move by); a sample on a cull boundary may flip between the two roundings: at most one ray in a hundred
    assert float(close) >= 0.99
    depth_close = ((got_host["depth"] - dev_frame["depth"]).abs() <= 1e-4 * dev_frame["depth"].abs()).float().mean()
    assert float(depth_close) >= 0.99, float(depth_close)


# ---- training ----------------------------------------------------------------------------------------------------------------

class _PinnedRelu:
    """TetraMLP's statement with the ReLU decisions GIVEN (bool [4, r, S, 128]: the three base layers and the head layer) instead of
    taken from its own pre-activations; the parameters are the wrapped module's."""

    def __init__(self, mlp, masks):
        self.mlp, self.masks = mlp, masks

    def fused_weights(self):
        return render.mlp_weights(self.mlp)

    def coarse_sigma(self, feats):
        return render.coarse_sigma(self.mlp, feats)

    def __call__(self, feats, dirs):
        m, x = self.mlp, feats
        for l, lin in enumerate(m.base):
            x = lin(x) * self.masks[l].to(x.dtype)
        sigma = torch.nn.functional.softplus(m.density(x))
        h = m.head(torch.cat([render.direction_encoding(dirs), x], dim=-1)) * self.masks[3].to(x.dtype)
        return sigma, torch.sigmoid(m.rgb(h))


def _train_run(tn, sc, S_fine, sync_free, fused, occ, thr, records, placement=None, replay=None, pin=None, watch=None):
    """one training batch with the live sampler -> (outputs, gradients of the field and the twelve MLP tensors).  placement: a list
    that receives what _chain_passes returned (the matched final samples and their edges); replay: such a pair, returned in the
    place of this run's own sample placement (its first `hit` rows: the rows of the hitting rays, padded or not); pin: ReLU
    decisions [4, rows, S, 128] for the statement's final pass (_PinnedRelu), likewise cut to the first `hit` rows; watch: a dict
    that receives, of a statement run, "decisions" (its own ReLU decisions of the final pass, [4, hit, S, 128]) and "weights" (the
    final composite's, [hit, S, 1])"""
    device = sc["field"].device
    S = 11
    mlp = render.TetraMLP().to(device)
    mlp.load_state_dict(sc["mlp"].state_dict())
    field = sc["field"].clone().requires_grad_(True)
    rd = render.TetraRenderer(sc["tr"], field, mlp, S, 256, num_fine_samples=S_fine, sync_free_train=sync_free, sync_free_min_hits=0.0)
    o, d = sc["o"], sc["d"]
    R = len(o)
    hit = int((rd._trace(o, d)["num_visited_cells"] > 0).sum())
    if pin is not None:
        rd.mlp = _PinnedRelu(mlp, pin[:, :hit])
    kw = {}
    torch.manual_seed(9)
    if not (sync_free and fused):
        # the draws of the sync-free form: the first `hit` rows of [R, .] draws, coarse first (render_train's docstring)
        coarse = torch.rand((R, S + 1), device=device)
        fine = torch.rand((R, S_fine + 1), device=device)
        kw["rand"] = {"coarse": coarse[:hit].contiguous(), "fine": fine[:hit].contiguous()}
    seen, hooks = [], []
    with pytest.MonkeyPatch.context() as mp:
        if records is not None:
            _record_backward(tn, mp, records)
        passes = rd._chain_passes
        if placement is not None:
            mp.setattr(rd, "_chain_passes", lambda *a, **k: (lambda res: (placement.append(res), res)[1])(passes(*a, **k)))
        if replay is not None:
            traced, edges = replay
            mp.setattr(rd, "_chain_passes", lambda *a, **k: ({key: v[:hit] for key, v in traced.items()}, edges[:hit]))
        if watch is not None:
            for lin in list(mlp.base) + [mlp.head]:
                hooks.append(lin.register_forward_hook(lambda _m, _i, pre: seen.append(pre.detach() > 0)))
            composite = render.composite
            mp.setattr(render, "composite", lambda *a, **k: (lambda res: (watch.__setitem__("weights", res[3].detach()), res)[1])(composite(*a, **k)))
        try:
            out = rd.render_train(o, d, gradient_scaling=True, fused=fused, occupancy=occ, occupancy_threshold=thr, occupancy_sampler=True, **kw)
        finally:
            for h in hooks:
                h.remove()
        target = torch.rand(R, 3, generator=torch.Generator().manual_seed(2)).to(device)
        (((out["rgb"] - target) ** 2).mean() + 0.1 * out["accumulation"].mean()).backward()
    if watch is not None:       # (the coarse pass runs the base layers first: the final pass's are the last three, then the head)
        final = [x for x in seen if x.dim() == 3 and x.shape[1] == S + S_fine + (1 if S_fine else 0)]
        watch["decisions"] = torch.stack(final[-4:])
    leaves = [field] + list(render.mlp_weights(mlp))
    return out, [x.grad.clone() for x in leaves]


# which ReLU layer (0 .. 3: base 0, 1, 2 and the head layer) a gradient tensor belongs to: a flipped unit of layer l changes d_l of its
# sample, hence w_l / b_l in the unit's own row and everything of the layers before it; the two narrow heads (4) sit behind no ReLU
LAYER_OF = {"field": -1, "w1": 0, "b1": 0, "w2": 1, "b2": 1, "w3": 2, "b3": 2, "wd": 4, "bd": 4, "wh": 3, "bh": 3, "wr": 4, "br": 4}


@pytest.mark.parametrize("S_fine,sync_free", [(7, True), (7, False), (0, True), (0, False)])
def test_render_train_with_the_live_sampler_vs_autograd_statement(tn, device, small_scene, monkeypatch, S_fine, sync_free):
    """Outputs and ALL gradients of the fused path (sync-free and compacting) against an independent render_train(fused=False): the
    PyTorch statement of the MLP, the cull mask and the composite under autograd, on the same sampler kernels and the same draws.
    Outputs: rgb and accumulation within 1e-5, the parity bar of the fused kernels against their statements (tests/test_train_gpu.py,
    test_render_gpu.py).  The depth is a median, i.e. a sample index: compared on EVERY ray whose cumulative weights stay further
    from 0.5 than 8 S u (the rounding of a sum of S <= 19 weights <= 1, with room for the weights' own last bits), read from the
    statement's own composite; the others are counted and printed.
    Gradients: the bar of tests/test_train_culled_gpu.py, 2 (n + 1) u sum |terms| per entry of the twelve MLP tensors, magnitudes from
    the fused run's own compact buffers, and for the field its PER-VERTEX bound, 2 (c + 1) u A_v over the c terms a vertex collects.
    There the two sides sum bit-equal terms; here a term d x0 comes from two arithmetics (the MFMA chain and torch's GEMMs: four
    layers of 128-term dot products each, every one within 128 u of the magnitudes it sums), so the field's bound is widened,
    explicitly, by 2 * 4 * 128 u A'_v, A'_v = sum |w| P0 with P0 = the magnitudes |d4|, |d sigma| pushed through |Wh|, |wd|, |W3|,
    |W2|, |W1|.
    One thing no rounding bound covers: a ReLU unit whose pre-activation rounds to the other side of 0 in torch's GEMM than in the
    MFMA chain hands a whole (sample, unit) term to w_l / b_l in the unit's row and to everything before its layer
    (tests/test_train_gpu.py: test_training_gradients_match_float64_under_the_saved_relu_masks).  So the statement's own decisions
    are read (forward hooks) and compared with the ones the fused forward saved, and an entry may exceed its bound ONLY where such a
    flip, or a sample the two runs matched to different vertices, reaches it: for a flip in layer l, row `unit` of w_l / b_l, every
    entry of the layers before l, and the field at the four vertices of the flipped SAMPLE -- everywhere else the bound holds
    unexcused.  The flips are counted, printed and must be fewer than 1e-5 of the decisions.
    Beside it, not instead of it: the statement once more on the fused run's placement with the fused run's decisions
    (_PinnedRelu) meets every bound with no excuse -- what is left then is the arithmetic of the adjoints alone."""
    sc = small_scene
    monkeypatch.setattr(tn.cpp, "DETERMINISTIC_FIELD_GRADIENT", True)
    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device)
    records, placement, plain_placement, watch = [], [], [], {}
    got, g_got = _train_run(tn, sc, S_fine, sync_free, True, occ, 0.5, records, placement=placement)
    want, g_plain = _train_run(tn, sc, S_fine, sync_free, False, occ, 0.5, None, placement=plain_placement, watch=watch)
    (placed,), (plain_placed,), (rec,) = placement, plain_placement, records
    saved = rec["saved"]
    S = 11 + S_fine + (1 if S_fine else 0)
    n, rows, hit = saved.n_samples, placed[1].shape[0], plain_placed[1].shape[0]
    assert 0 < saved.n <= n and n == rows * S     # (the sampler's point: nearly every sample is live -- here all of them)
    decisions = torch.zeros((4, n, 128), dtype=torch.bool, device=device)
    live_idx = saved.live[:saved.n].long()
    decisions[:, live_idx] = _decode_relu_masks(saved.masks.clone(), saved.n)
    decisions = decisions.view(4, rows, S, 128)
    on_same, g_pin = _train_run(tn, sc, S_fine, sync_free, False, occ, 0.5, None, replay=placed, pin=decisions)

    # ---- outputs
    assert torch.equal(got["ray_mask"], want["ray_mask"])
    for k in ("rgb", "accumulation"):
        e = float((got[k] - want[k]).abs().max())
        _report(f"train S_fine={S_fine} sync_free={sync_free} {k}: max |fused - statement| {e:.3e}")
        assert e <= 1e-5, (k, e)
    assert float((on_same["rgb"] - got["rgb"]).abs().max()) <= 1e-5
    margin = torch.full((len(sc["o"]), 1), 1.0, device=device)
    margin[torch.nonzero(want["ray_mask"])[:, 0]] = render.median_margin(watch["weights"])
    decided = (margin > 8 * S * U)[:, 0]
    _report(f"train S_fine={S_fine} sync_free={sync_free} depth: {int((~decided).sum())} of {len(decided)} rays within 8 S u of the median threshold")
    assert float((got["depth"] - want["depth"]).abs()[decided].max()) <= 1e-5

    # ---- where a bound may be exceeded: flipped decisions and samples matched to other vertices
    live_mask = torch.zeros(n, dtype=torch.bool, device=device)
    live_mask[live_idx] = True
    flips = (watch["decisions"] != decisions[:, :hit]) & live_mask.view(rows, S)[:hit][None, :, :, None]
    per_layer = flips.sum(dim=(1, 2, 3)).tolist()
    moved = (plain_placed[0]["vertex_indices"] != placed[0]["vertex_indices"][:hit]).any(-1)
    _report(f"train S_fine={S_fine} sync_free={sync_free}: ReLU decisions of the statement that differ from the fused forward's, per layer "
            f"{per_layer} of {flips[0].numel()} each; samples matched to other vertices {int(moved.sum())}")
    assert sum(per_layer) < 1e-5 * flips.numel()
    top = max([l for l in range(4) if per_layer[l]], default=-1)          # the last layer with a flip
    touched = flips.any(0).any(-1) | moved                                # [hit, S]: samples with a flip or other vertices
    V = sc["field"].shape[1]
    at_vertex = torch.zeros(V + 1, dtype=torch.bool, device=device)
    for vi_of in (placed[0]["vertex_indices"][:hit], plain_placed[0]["vertex_indices"]):
        at_vertex[vi_of[touched].long().clamp_min(-1).reshape(-1)] = True      # (-1, an empty id, lands in the spare last slot)
    excuse = {"field": at_vertex[:V][None, :].expand(64, V) if (top >= 0 or bool(moved.any())) else None}
    for name in GRADS:
        l = LAYER_OF[name]
        if bool(moved.any()) or l < top:
            excuse[name] = "all"
        elif l == top and l < 4:
            unit = flips[l].any(0).any(0)                                 # [128]: the units that flipped in this layer
            excuse[name] = unit if name.startswith("b") else unit[:, None]
        else:
            excuse[name] = None

    # ---- the bounds
    mags = _term_magnitudes(rec, S)
    gc = importlib.import_module("gather_cases")
    vi = rec["vi"].reshape(-1, 4)[live_idx].cpu().numpy()
    bc = rec["bc"].reshape(-1, 3)[live_idx].float().cpu().numpy()
    w = [x.detach().double().abs() for x in render.mlp_weights(sc["mlp"])]
    chain = rec["chain"]
    k_live = saved.n
    d4 = _quad_major(chain.d4, k_live).double().abs()                     # [k, 128]
    dsig = chain.dhead.double().abs()[0][:, None]                         # [k, 1]
    P = d4 @ w[8][:, render.DIR_ENC:] + dsig * w[6]                       # |d h3|   (wh [128, 155], wd [1, 128])
    P = ((P @ w[4]) @ w[2]) @ w[0]                                        # through |W3|, |W2|, |W1| -> [k, 64]
    _, adj_A, cnt = gc.adjoint_ref(vi, bc, rec["dx0"].detach().cpu().numpy(), rec["V"])
    _, adj_P, _ = gc.adjoint_ref(vi, bc, P.cpu().numpy(), rec["V"])
    field_bound = (2 * torch.from_numpy(gc.adjoint_bound(dict(count=cnt, adj_A=adj_A))) + 2 * 4 * 128 * U * torch.from_numpy(np.asarray(adj_P))).t().to(device)
    rel = 2 * (n + 1) * U
    failures = []
    for label, g_want, excuses in (("independent statement", g_plain, excuse), ("same placement and decisions", g_pin, {})):
        for name, g, want_g in zip(["field"] + GRADS, g_got, g_want):
            assert bool(torch.isfinite(g).all()) and float(want_g.abs().max()) > 0, name
            err = (g.double() - want_g.double()).abs()
            bound = field_bound if name == "field" else rel * mags[name].reshape(err.shape) + n * 2.0 ** -126
            over = err > bound
            ex = excuses.get(name)
            n_over = int(over.sum())
            if isinstance(ex, str):
                over = over & False
            elif ex is not None:
                over = over & ~ex.expand_as(err)
            _report(f"train S_fine={S_fine} sync_free={sync_free} {label} {name}: max err / bound = "
                    f"{float((err / bound.clamp_min(1e-300)).max()):.3f}; entries over their bound {n_over}, unexcused {int(over.sum())}")
            if bool(over.any()):
                failures.append((label, name))
    assert not failures, failures


@pytest.mark.parametrize("S_fine", [7, 0])
def test_gradient_scaler_spacing_vs_float64(tn, device, small_scene, S_fine):
    """The one new arithmetic of render_train with the sampler: GradientScaler's ray_dist = spacing_j + spacing_{j+1}, spacing =
    (live_to_distance(s_edges) - near) / (far - near) with the ray's own far.  Against the float64 statements on the call's own
    edges.  Decision-free like the map's own checks: an edge within eps = 2^-20 (L + |far|) (the floor of the map's bound above,
    whose y is far below it) of the end of a live run may land on either side of the gap behind it, and the map is monotone, so each
    ray_dist must lie between the float64 values at s - eps and s + eps, give or take 8 u: a difference, a division and a sum in fp32 on values of at most 2."""
    sc = small_scene
    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device)
    rd = render.TetraRenderer(sc["tr"], sc["field"].clone().requires_grad_(True), sc["mlp"], 11, 256, num_fine_samples=S_fine)
    cap = {}
    rd.render_train(sc["o"], sc["d"], gradient_scaling=True, fused=False, occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True,
                    capture=cap, generator=torch.Generator(device=device).manual_seed(1))
    out = rd._trace(sc["o"], sc["d"])
    idx = cap["idx"]
    live64 = render.live_lengths_statement(out["num_visited_cells"][idx], out["visited_cells"][idx], out["hit_distances"][idx].double(), occ, 0.5)
    near, far = (x.double() for x in render.hit_near_far(out, idx))
    assert torch.equal(cap["near"].double(), near) and bool((far > near).all())
    eps = cases.FLOOR * (live64["length"] + far.abs())

    def ray_dist64(s):
        t64, _ = render.live_to_distance_statement(s, live64)
        spacing = (t64 - near) / (far - near)
        return (spacing[:, 1:] + spacing[:, :-1])[..., None]

    s_edges = cap["edges"].double()
    lo, mid, hi = ray_dist64(s_edges - eps), ray_dist64(s_edges), ray_dist64(s_edges + eps)
    got = cap["ray_dist"].double()
    assert got.shape == mid.shape and float(mid.max()) > 1.0 and bool((lo >= 0).all()) and bool((hi <= 2 + 1e-9).all())
    _report(f"GradientScaler spacing S_fine={S_fine}: max |got - float64| {float((got - mid).abs().max()):.3e}; "
            f"entries beyond 2 eps / (far - near) of it {int(((got - mid).abs() > (2 * eps / (far - near))[..., None]).sum())} of {got.numel()}")
    assert bool((got >= lo - 8 * U).all()) and bool((got <= hi + 8 * U).all())


def test_refusals(tn, device, small_scene):
    sc = small_scene
    o, d = sc["o"], sc["d"]
    occ = torch.rand(sc["T"], generator=torch.Generator().manual_seed(3)).to(device)
    rd = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], 11, 256, num_fine_samples=7)
    with pytest.raises(RuntimeError, match="occupancy_sampler needs"):
        rd.render(o, d, occupancy_sampler=True)
    with pytest.raises(RuntimeError, match="occupancy_sampler needs"):
        rd.render_train(o, d, occupancy_sampler=True)
    with pytest.raises(RuntimeError, match="no adjoint"):
        rd.render_train(o, d, occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True, position_gradients=True)
    with pytest.raises(RuntimeError, match="bf16"):
        rd.render(o, d, occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True, mlp_mode="bf16")
    # the ops: no occupancy, wrong types, and a row length whose prefix sums do not fit the block's LDS
    nv = torch.ones(2, dtype=torch.int32, device=device)
    idx = torch.arange(2, dtype=torch.int32, device=device)
    for M, ok in ((4095, True), (4096, False)):
        cells = torch.zeros(2, M, dtype=torch.int32, device=device)
        hd = torch.rand(2, M, 2, device=device).sort(-1).values
        if ok:
            tn.cpp.sample_live(nv, cells, hd, idx, 5, occ, 0.5)
            tn.cpp.live_to_distance(torch.rand(2, 3, device=device), nv, cells, hd, idx, occ, 0.5)
            with pytest.raises(RuntimeError, match="occupancy"):
                tn.cpp.sample_live(nv, cells, hd, idx, 5, None, 0.5)
            with pytest.raises(RuntimeError, match="visited_cells"):
                tn.cpp.sample_live(nv, cells.long(), hd, idx, 5, occ, 0.5)
            with pytest.raises(RuntimeError, match="values"):
                tn.cpp.live_to_distance(torch.rand(3, 3, device=device), nv, cells, hd, idx, occ, 0.5)
            with pytest.raises(RuntimeError, match="count"):
                tn.cpp.live_to_distance(torch.rand(2, 3, device=device), nv, cells, hd, idx, occ, 0.5, count=torch.ones(1, device=device))
        else:
            with pytest.raises(RuntimeError, match="too large"):
                tn.cpp.sample_live(nv, cells, hd, idx, 5, occ, 0.5)
            with pytest.raises(RuntimeError, match="too large"):
                tn.cpp.live_to_distance(torch.rand(2, 3, device=device), nv, cells, hd, idx, occ, 0.5)
