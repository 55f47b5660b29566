"""The occupancy-guided sampler as stated in render.py (live_lengths_statement, live_sample_bins, live_to_distance_statement), on the
crafted rows of tests/live_sampler_cases.py, without a GPU: the inputs meet their own conditions, the statements have the
properties the kernels are then held to (tests/test_live_sampler_gpu.py), and the defect the sampler removes is there without it."""
import importlib

import pytest
import torch

import live_sampler_cases as cases

render = importlib.import_module("tetra-nerf_amd.render")


@pytest.fixture(scope="module")
def rows():
    return cases.live_rows()


@pytest.fixture(scope="module")
def live64(rows):
    return cases.live_statement(rows, torch.float64)


def _pattern(rows, name):
    return rows["pattern"] == cases.PATTERNS.index(name)


def test_inputs_meet_their_conditions(rows, live64):
    nv = rows["num_visited"]
    assert rows["hit_distances"].shape == (378, cases.M, 2) and rows["visited_cells"].dtype == torch.int32
    assert sorted(set(nv.tolist())) == [0, 1, 2, 63, 64, 65, 129, 255, 256]
    hd = rows["hit_distances"].double()
    inside = torch.arange(cases.M)[None] < nv[:, None]
    lengths = torch.where(inside, (hd[..., 1] - hd[..., 0]).clamp_min(0), 0.0)
    culled = inside & render.cull_mask_statement(rows["visited_cells"], rows["occupancy"], cases.THRESHOLD)
    raw_L = torch.where(culled, 0.0, lengths).sum(1)
    for p, name in enumerate(cases.PATTERNS):
        sel = (rows["pattern"] == p) & (nv > 0)
        assert int(sel.sum()) == 48
        if name == "all culled":
            assert bool((raw_L[sel] == 0).all()) and bool(culled[sel].sum(1).eq(nv[sel]).all())
        else:
            assert bool((raw_L[sel] > 0).all()), name
        if name == "all live":
            assert not bool(culled[sel].any())
        elif name not in ("ends culled",):
            assert bool(culled[sel & (nv > 2)].any(1).all()), name
    # the invalid ids and the NaN occupancies are there, and live
    inv = _pattern(rows, "invalid id") & (nv > 0)
    c = rows["visited_cells"][inv]
    assert bool((c[:, 0] >= rows["occupancy"].numel()).all()) and bool(((c == -1) & inside[inv]).any(1)[nv[inv] > 1].all())
    assert int(torch.isnan(rows["occupancy"]).sum()) >= 48
    # a zero-length and a backward segment per ray of four segments or more
    big = nv >= 4
    r = torch.nonzero(big)[:, 0]
    z, n = rows["zero_slot"][big], rows["neg_slot"][big]
    assert bool((hd[r, z, 1] == hd[r, z, 0]).all()) and bool((hd[r, n, 1] < hd[r, n, 0]).all())


def test_live_lengths_and_fall_backs(rows, live64):
    nv = rows["num_visited"].long()
    w, cum, near, L = live64["w"], live64["cum"], live64["near"][:, 0], live64["length"][:, 0]
    hd = rows["hit_distances"].double()
    inside = torch.arange(cases.M)[None] < nv[:, None]
    lengths = torch.where(inside, (hd[..., 1] - hd[..., 0]).clamp_min(0), 0.0)
    hit = nv > 0
    assert bool((cum[:, 0] == 0).all()) and bool((cum[:, 1:] >= cum[:, :-1]).all())
    assert bool((cum[:, 1:] - cum[:, :-1])[w == 0].eq(0).all())               # flat over every segment of weight 0
    assert torch.allclose(cum[:, -1], w.sum(1), rtol=1e-14, atol=0)
    assert torch.equal(near[hit], hd[hit, 0, 0]) and torch.equal(L[hit], cum[hit, -1])
    # everything culled (L == 0): every segment counts as live; all live and threshold <= 0: the lengths themselves
    for sel in (_pattern(rows, "all culled"), _pattern(rows, "all live")):
        assert torch.equal(w[sel], lengths[sel])
    for thr in (0.0, -1.0):
        assert torch.equal(cases.live_statement(rows, torch.float64, thr)["w"], lengths)
    # rows without a segment: near = 0, L = 1 and t = s
    miss = ~hit
    assert int(miss.sum()) == 6 * len(cases.PATTERNS) and bool((near[miss] == 0).all()) and bool((L[miss] == 1).all())
    s = torch.rand(len(nv), 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3 - 1
    t, slot = render.live_to_distance_statement(s, live64)
    assert torch.equal(t[miss], s[miss]) and not bool(slot[miss].any())


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("S", cases.S_VALUES)
def test_edges_ascend_and_span_the_live_length(rows, live64, S, train):
    t_rand = cases.draws(S + 1).double() if train else None
    edges, (near, far) = render.live_sample_bins(live64, S, t_rand)
    assert edges.shape == (378, S + 1)
    assert bool((edges[:, 1:] >= edges[:, :-1]).all())
    assert torch.equal(near, live64["near"]) and torch.equal(far, live64["near"] + live64["length"])
    assert bool((edges >= near - 1e-12).all()) and bool((edges <= far + 1e-12).all())
    if not train:
        assert torch.allclose(edges[:, 0], near[:, 0]) and torch.allclose(edges[:, -1], far[:, 0])
    # the spacing bins and the stratification are the uniform sampler's
    assert torch.equal(edges, render.uniform_sample_bins(near, far, S, t_rand))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", (1, 7, 200))
def test_mapped_values_lie_in_live_segments(rows, live64, n, dtype):
    live = cases.live_statement(rows, dtype)
    s = cases.values_in_span(live, cases.draws(n))
    t, slot = render.live_to_distance_statement(s, live)
    hit = rows["num_visited"] > 0
    hd = rows["hit_distances"].to(dtype)
    t_in, t_out = torch.gather(hd[..., 0], 1, slot), torch.gather(hd[..., 1], 1, slot)
    assert bool((slot[hit] < rows["num_visited"][hit, None]).all())
    assert bool((torch.gather(live["w"], 1, slot)[hit] > 0).all())            # a live slot of positive length
    assert bool((t_in[hit] <= t[hit]).all()) and bool((t[hit] <= t_out[hit]).all())
    # ... which cull_mask_statement does not cull, unless the whole ray is culled
    some_live = hit & ~_pattern(rows, "all culled")
    cells = torch.gather(rows["visited_cells"], 1, slot)
    assert not bool(render.cull_mask_statement(cells, rows["occupancy"], cases.THRESHOLD)[some_live].any())
    if dtype == torch.float64:
        # the forward map (live length before t) returns s - near
        back = cases.forward_map64(live64, slot, t)
        err = (back - (s - live["near"])).abs() / live["length"]
        assert float(err[hit].max()) <= 1e-12, float(err[hit].max())
        # exactly contiguous rows with every segment live (threshold 0): the coordinate IS the distance
        live0 = cases.live_statement(cases.contiguous(rows), torch.float64, 0.0)
        s0 = cases.values_in_span(live0, cases.draws(n))
        t0, _ = render.live_to_distance_statement(s0, live0)
        assert float(((t0 - s0).abs() / live0["length"])[hit].max()) <= 1e-12


def _uniform_culled_accumulation(rows, S, sigma):
    """accumulation of the uniform sampler + culling in float64: S bins over [near, far], a bin's density = sigma where its CENTRE
    lies in a live segment, times the whole bin width"""
    hd = rows["hit_distances"].double()
    nv = rows["num_visited"].long()
    near, far = hd[:, 0, :1], torch.gather(hd[..., 1], 1, (nv[:, None] - 1).clamp_min(0))
    edges = render.uniform_sample_bins(near, far, S)
    centres = render.bin_centres(edges)
    starts = torch.where(torch.arange(cases.M)[None] < nv[:, None], hd[..., 0], torch.full_like(hd[..., 0], float("inf")))
    slot = (torch.searchsorted(starts.contiguous(), centres.contiguous(), right=True) - 1).clamp_min(0)      # contiguous segments
    culled = render.cull_mask_statement(torch.gather(rows["visited_cells"], 1, slot), rows["occupancy"], cases.THRESHOLD)
    return render.ray_weights(torch.where(culled, 0.0, sigma), edges).sum(-1)


@pytest.mark.parametrize("S", (1, 7, 200))
def test_constant_density_is_exact_and_the_uniform_sampler_is_not(rows, live64, S):
    """Density sigma in every live tetrahedron, 0 in the culled ones: the optical depth of a ray is sigma L.  On s_edges every
    sample is live and every delta is the live length inside its bin, so the accumulation is 1 - exp(-sigma L) whatever S is;
    the uniform sampler with culling multiplies sigma by whole bin widths that reach into culled space (or skips live space whose
    bin centre is culled) and misses that value."""
    sigma = 3.0
    hit = (rows["num_visited"] > 0) & ~_pattern(rows, "all culled")
    for train in (False, True):
        edges, _ = render.live_sample_bins(live64, S, cases.draws(S + 1).double() if train else None)
        if train:        # (stratified bins cover the span only when the outer edges are pinned: jitter leaves them inside)
            edges[:, 0], edges[:, -1] = live64["near"][:, 0], (live64["near"] + live64["length"])[:, 0]
        _, slot = render.live_to_distance_statement(render.bin_centres(edges), live64)
        culled = render.cull_mask_statement(torch.gather(rows["visited_cells"], 1, slot), rows["occupancy"], cases.THRESHOLD)
        assert not bool(culled[hit].any())
        acc = render.ray_weights(torch.where(culled, 0.0, sigma), edges).sum(-1)
        want = 1 - torch.exp(-sigma * live64["length"][:, 0])
        assert float((acc - want).abs()[hit].max()) <= 1e-12
    uni = _uniform_culled_accumulation(rows, S, sigma)
    want = 1 - torch.exp(-sigma * live64["length"][:, 0])
    gaps = (rows["num_visited"] >= 63) & (_pattern(rows, "alternating") | _pattern(rows, "middle run") | _pattern(rows, "nan occupancy"))
    miss = (uni - want).abs()[gaps]
    assert float(miss.min()) > 1e-9 and float(miss.max()) > 1e-2       # no ray gets the value; some miss it by far
    # without culled space (exactly contiguous rows, every segment live) the two agree
    flat = cases.contiguous(rows)
    same = (rows["num_visited"] > 0) & _pattern(rows, "all live")
    want = 1 - torch.exp(-sigma * cases.live_statement(flat, torch.float64)["length"][:, 0])
    assert float((_uniform_culled_accumulation(flat, S, sigma) - want).abs()[same].max()) <= 1e-12


def test_render_reference_refuses_a_sampler_without_a_field():
    with pytest.raises(RuntimeError, match="occupancy_sampler needs"):
        render.render_reference(None, None, None, None, torch.zeros(1, 3), torch.zeros(1, 3), occupancy_sampler=True)


# ---- whole frames and a training call in PyTorch, on the oracle's CPU tracer ---------------------------------------------------

from test_occupancy import scene  # noqa: E402,F401  (the CPU scene of the occupancy tests)

NEW = ("tn_sample_live", "tn_live_to_distance")


def test_abi_additions_keep_version_6():
    import ctypes
    import re
    from pathlib import Path

    _lib = importlib.import_module("tetra-nerf_amd._lib")
    header = (Path(__file__).resolve().parents[1] / "include" / "tetranerf_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/tetranerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the shared library"
        assert name in _lib.SYMBOLS
        assert "%s (model.py:98-99,256-265)" % name in header, name
    comment = header[:header.index("int tn_sample_live(")].rsplit("/*", 1)[1]
    assert "model.py:98-99,256-265" in comment and "unused" in comment
    assert re.search(r"#define\s+TN_ABI_VERSION\s+6\b", header)
    assert _lib.ABI_VERSION == 6 and lib.tn_abi_version() == 6
    # the exports are the header's names
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", code)) - {"tn_rgb_background"}
    assert declared == set(_lib.SYMBOLS)


@pytest.mark.parametrize("S,S_fine", [(13, 0), (9, 7)])
def test_render_reference_with_the_live_sampler(scene, S, S_fine):
    sc = scene
    occ = torch.rand(sc.T, generator=torch.Generator().manual_seed(1))
    seen = []

    class Recording:
        def trace_rays(self, *a):
            self.out = sc.tracer.trace_rays(*a)
            return self.out

        def find_visited_cells(self, *a):
            out = sc.tracer.find_visited_cells(*a)
            seen.append((a[5], out["cell_indices"]))
            return out

    def run(**kw):
        del seen[:]
        tracer = Recording()
        with torch.no_grad():
            out = render.render_reference(tracer, sc.interp, sc.field, sc.mlp, sc.o, sc.d, S, 256, num_fine_samples=S_fine, **kw)
        culled = render.cull_mask_statement(seen[-1][1], occ, kw["occupancy_threshold"])
        return out, tracer.out, float(culled.float().mean())

    uniform, _, uni_share = run(occupancy=occ, occupancy_threshold=0.5)
    live, traced, share = run(occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True)
    hit = live["ray_mask"]
    assert torch.equal(hit, uniform["ray_mask"]) and 0 < int(hit.sum()) < len(sc.o)
    assert all(bool(torch.isfinite(live[k]).all()) for k in ("rgb", "accumulation", "depth"))
    assert not torch.equal(live["rgb"], uniform["rgb"])
    assert share < uni_share                          # the final samples sit in live tetrahedra (but for rays without any)
    # every located distance ascends along its ray and lies inside the ray's span; so does the mapped depth
    nv = traced["num_visited_cells"][hit].long()
    hd = traced["hit_distances"][hit]
    near, far = hd[:, 0, :1], torch.gather(hd[..., 1], 1, nv[:, None] - 1)
    for dist, _ in seen:
        assert bool((dist[:, 1:] >= dist[:, :-1]).all()) and bool((dist >= near).all()) and bool((dist <= far).all())
    assert bool((live["depth"][hit] >= near).all()) and bool((live["depth"][hit] <= far).all())
    assert bool((live["depth"][~hit] == 1000.0).all())
    # everything culled: the background frame
    empty, _, _ = run(occupancy=occ, occupancy_threshold=2.0, occupancy_sampler=True)
    assert torch.all(empty["accumulation"] == 0.0) and torch.all(empty["rgb"] == 1.0)


def test_unfused_training_call_with_the_live_sampler(scene):
    sc = scene
    occ = torch.rand(sc.T, generator=torch.Generator().manual_seed(1))
    field = sc.field.clone().requires_grad_(True)
    rd = render.TetraRenderer(sc.tracer, field, sc.mlp, 9, 256, num_fine_samples=7, cache_field=False, device_samplers=False,
                              interpolate_values=sc.interp)
    caps = {}
    for name, kw in (("uniform", {}), ("live", {"occupancy_sampler": True})):
        field.grad = None
        caps[name] = {}
        out = rd.render_train(sc.o, sc.d, fused=False, gradient_scaling=True, generator=torch.Generator().manual_seed(4),
                              occupancy=occ, occupancy_threshold=0.5, capture=caps[name], **kw)
        (out["rgb"].square().mean() + out["accumulation"].mean()).backward()
        assert bool(torch.isfinite(out["rgb"]).all()) and bool(torch.isfinite(field.grad).all()) and float(field.grad.abs().max()) > 0
    assert float(caps["live"]["culled"].float().mean()) < float(caps["uniform"]["culled"].float().mean())
    e = caps["live"]["edges"]
    assert e.shape[1] == 9 + 7 + 2 and bool((e[:, 1:] >= e[:, :-1]).all())
    # GradientScaler's ray_dist = spacing_j + spacing_{j+1}, spacing = (live_to_distance(s_edges) - near) / (far - near) with the
    # ray's own far, against the float64 statements on the call's own edges; decision-free: an edge within eps = 2^-20 (L + |far|) of
    # the end of a live run may land on either side of the gap, the map is monotone (8 u: three fp32 operations on values <= 2)
    cap = caps["live"]
    out = sc.tracer.trace_rays(sc.o, sc.d, 256)
    idx = cap["idx"]
    live64 = render.live_lengths_statement(out["num_visited_cells"][idx], out["visited_cells"][idx], out["hit_distances"][idx].double(), occ, 0.5)
    near, far = (x.double() for x in render.hit_near_far(out, idx))
    eps = 2.0 ** -20 * (live64["length"] + far.abs())

    def ray_dist64(s):
        spacing = (render.live_to_distance_statement(s, live64)[0] - near) / (far - near)
        return (spacing[:, 1:] + spacing[:, :-1])[..., None]

    got, s_edges = cap["ray_dist"].double(), cap["edges"].double()
    assert got.shape == (len(idx), 9 + 7 + 1, 1) and float(got.max()) > 1.0
    assert bool((got >= ray_dist64(s_edges - eps) - 8 * 2.0 ** -24).all()) and bool((got <= ray_dist64(s_edges + eps) + 8 * 2.0 ** -24).all())
    assert "ray_dist" in caps["uniform"] and not torch.equal(caps["uniform"]["ray_dist"], cap["ray_dist"])
    with pytest.raises(RuntimeError, match="occupancy_sampler needs"):
        rd.render_train(sc.o, sc.d, fused=False, occupancy_sampler=True)
    with pytest.raises(RuntimeError, match="no adjoint"):
        rd.render_train(sc.o, sc.d, fused=False, occupancy=occ, occupancy_threshold=0.5, occupancy_sampler=True, position_gradients=True)
