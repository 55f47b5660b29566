"""The per-tetrahedron training statistics on the GPU (tn_tet_stats_accumulate, csrc/tn_tet_stats.hip; cpp.tet_stats_accumulate,
TetraRenderer.render_train(tet_stats=True) / accumulate_tet_stats, the adapter's config.densify_stats, densify(stats=...)).

Bar: BIT-EQUAL INTEGERS everywhere, no tolerance.  The weights the statement (render.tet_stats_statement) takes are those
cpp.composite(sigma, None, edges) writes for the same sigma and edges -- the kernel must have formed the same bits in its LDS --
and `stats` starts from non-zero values, so that the entry is seen to accumulate."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import tet_stats_cases as tc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import reference_model as rm   # noqa: E402

render = importlib.import_module("tetra-nerf_amd.render")
GRID_CAP = 256 * 32                      # TS_MAX_GRID of tn_tet_stats.hip: from there on a wave strides over rows


def _dev(x, device):
    return None if x is None else torch.from_numpy(np.array(x)).to(device)


def _check(tn, device, T, cells, sigma, edges, ray_value=None, ray_index=None, count=None, what="", seed=0):
    """one call of the entry against the statement on the composite's own weights; returns (want, weights, stats0)"""
    stats0 = tc.stats0(np.random.default_rng(seed), T)
    d_cells, d_sigma, d_edges = _dev(cells, device), _dev(sigma, device), _dev(edges, device)
    weights = tn.cpp.composite(d_sigma, None, d_edges).cpu().numpy()
    want = render.tet_stats_statement(stats0, cells, weights, ray_value, ray_index, None if count is None else int(count))
    stats = _dev(stats0, device)
    d_count = None if count is None else torch.tensor([int(count)], dtype=torch.int32, device=device)
    got = tn.cpp.tet_stats_accumulate(stats, d_cells, d_sigma, d_edges, ray_value=_dev(ray_value, device), ray_index=_dev(ray_index, device),
                                      count=d_count)
    assert got is stats
    g = stats.cpu().numpy()
    bad = np.argwhere(g != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} sums differ (first at {bad[:1].tolist()}: {g[tuple(bad[0])]} vs {want[tuple(bad[0])]})"
    return want, weights, stats0


# ------------------------------------------------------------------------------------------- the entry against the statement
@pytest.mark.parametrize("S", [1, 63, 64, 65, 128, 129, 320, 321, 513])
@pytest.mark.parametrize("R", [1, 3, 64, 65, 257])
def test_entry_equals_the_statement(tn, device, S, R):
    """the chunk edges of ray_composite's three dispatch forms x the wave and block edges of the launch; runs of 1 .. 100 samples"""
    rng = np.random.default_rng(1000 * S + R)
    T = 211
    sigma, edges = tc.sigma_edges(rng, R, S)
    want, weights, stats0 = _check(tn, device, T, tc.run_cells(rng, R, S, T), sigma, edges, 4 * rng.random(R, dtype=np.float32),
                                   what=f"S={S} R={R}", seed=S + R)
    assert int((want - stats0)[:, 0].sum()) == R * S and weights.max() > 0


@pytest.mark.parametrize("S", [1, 65])
def test_first_row_count_beyond_the_grid_cap(tn, device, S):
    rng = np.random.default_rng(S)
    R, T = GRID_CAP + 1, 997
    sigma, edges = tc.sigma_edges(rng, R, S)
    _check(tn, device, T, tc.run_cells(rng, R, S, T), sigma, edges, rng.random(R, dtype=np.float32), what=f"R={R} S={S}")


@pytest.mark.parametrize("S, R", [(1025, 3), (8192, 2)])
def test_long_rows(tn, device, S, R):
    """beyond one pass of the composite's widest form (9 chunks = 576 samples), and the longest row the entry takes (32 KiB of LDS)"""
    rng = np.random.default_rng(S)
    T = 61
    sigma, edges = tc.sigma_edges(rng, R, S)
    _check(tn, device, T, tc.run_cells(rng, R, S, T), sigma, edges, rng.random(R, dtype=np.float32), what=f"S={S}")
    assert S <= tn.cpp.TET_STATS_MAX_SAMPLES
    if S == tn.cpp.TET_STATS_MAX_SAMPLES:                                      # one more is refused, not truncated
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)   # noqa: E731
        stats = z(T, 3, dtype=torch.int64)
        with pytest.raises(RuntimeError, match="8192"):
            tn.cpp.tet_stats_accumulate(stats, z(1, S + 1, dtype=torch.int32), z(1, S + 1), z(1, S + 2))
        assert not stats.any()


# ------------------------------------------------------------------------------------------------------------ named edge cases
def test_every_sample_in_one_tetrahedron(tn, device):
    """the largest contention, and T = 1: 64 x 513 samples into one row of three sums, checked exactly"""
    rng = np.random.default_rng(11)
    R, S = 64, 513
    sigma, edges = tc.sigma_edges(rng, R, S)
    v = 4 * rng.random(R, dtype=np.float32)
    want, weights, stats0 = _check(tn, device, 1, np.zeros((R, S), np.int32), sigma, edges, v, what="one tetrahedron")
    # the sums once more, without the statement: plain integer sums over all samples
    w64 = np.rint(weights.astype(np.float64) * 2.0 ** 32).astype(np.int64)
    e64 = np.rint((weights * v[:, None]).astype(np.float32).astype(np.float64) * 2.0 ** 32).astype(np.int64)
    assert (want - stats0)[0].tolist() == [R * S, int(w64.sum()), int(e64.sum())]
    assert 0 <= weights.min() and weights.max() <= 1 and v.max() <= 256       # (no clamp is active in this case)


def test_every_sample_in_its_own_tetrahedron(tn, device):
    rng = np.random.default_rng(12)
    R, S = 5, 129
    sigma, edges = tc.sigma_edges(rng, R, S)
    want, _, stats0 = _check(tn, device, R * S, rng.permutation(R * S).astype(np.int32).reshape(R, S), sigma, edges,
                             rng.random(R, dtype=np.float32), what="own tetrahedron")
    assert ((want - stats0)[:, 0] == 1).all()


@pytest.mark.parametrize("name", ["invalid_ids", "aba", "all_distinct", "single_sample"])
def test_named_cell_patterns(tn, device, name):
    """unmatched cells and ids = T and T + 1 contribute nothing; a tetrahedron that comes back on the ray (A B A) is folded run by run"""
    c = tc.case(name)
    rng = np.random.default_rng(13)
    sigma, edges = tc.sigma_edges(rng, *c["cells"].shape)
    want, _, stats0 = _check(tn, device, c["T"], c["cells"], sigma, edges, c["ray_value"], what=name)
    ok = (c["cells"] >= 0) & (c["cells"] < c["T"])
    assert int((want - stats0)[:, 0].sum()) == int(ok.sum())
    if name == "invalid_ids":
        assert 0 < ok.sum() < ok.size and (c["cells"] == c["T"]).any() and (c["cells"] == c["T"] + 1).any() and (c["cells"] == -1).any()


def test_ray_values_at_every_branch_of_the_clamp(tn, device):
    rng = np.random.default_rng(14)
    v = np.float32([np.nan, -1, -0.0, 0, 256, 257, np.inf, 1e-3])
    R, S, T = len(v), 70, 9
    sigma, edges = tc.sigma_edges(rng, R, S)
    cells = np.repeat(np.arange(R, dtype=np.int32)[:, None], S, 1)           # ray q alone feeds tetrahedron q
    want, weights, stats0 = _check(tn, device, T, cells, sigma, edges, v, what="ray values")
    add = want - stats0
    assert (add[:4, 2] == 0).all() and (add[:R, 1] > 0).all()                 # NaN, -1, -0, 0: no error, the weight still counts
    assert (add[4:R, 2] > 0).all()
    # 257 and inf are clamped to 256: what ray 4's weights would give -- checked through the statement on those weights
    for q in (5, 6):
        alone = render.tet_stats_statement(np.zeros((1, 3), np.int64), np.zeros((1, S), np.int32), weights[q:q + 1], np.float32([256]))
        assert add[q].tolist() == alone[0].tolist()
    # no ray_value at all: every value 1, the error channel is the weight channel
    want1, _, s1 = _check(tn, device, T, cells, sigma, edges, None, what="no ray value")
    assert ((want1 - s1)[:, 1] == (want1 - s1)[:, 2]).all()


def test_opaque_rays_zero_density_and_a_nan_weight(tn, device):
    rng = np.random.default_rng(15)
    R, S, T = 6, 130, 17
    sigma, edges = tc.sigma_edges(rng, R, S)
    edges[:2] = np.linspace(0.5, 6.5, S + 1, dtype=np.float32)                # delta = 0.046
    sigma[0] = 1.0e4                                                          # sigma delta in the hundreds from the first sample on
    sigma[1, :40] = 0.0
    sigma[1, 40:] = 2.0e4                                                     # ... and behind an empty stretch
    sigma[2] = 0.0                                                            # nothing at all
    edges[3, S] = np.inf                                                      # delta = inf: sigma 0 -> 0 * inf = NaN before nan_to_num
    sigma[3, S - 1] = 0.0
    edges[4, S] = np.inf                                                      # delta = inf with a density: the last weight takes all that is left
    sigma[5, ::2] = 0.0
    cells = tc.run_cells(rng, R, S, T, longest=30)
    want, weights, stats0 = _check(tn, device, T, cells, sigma, edges, 1 + rng.random(R, dtype=np.float32), what="opaque / empty / NaN")
    assert weights[0, 0] == 1.0 and not weights[0, 1:].any()                  # exactly 1, then exactly 0
    assert not weights[1, :40].any() and weights[1, 40] == 1.0 and not weights[1, 41:].any()
    assert not weights[2].any() and weights[3, S - 1] == 0.0 and np.isfinite(weights).all()
    assert int((want - stats0)[:, 0].sum()) == R * S                          # every sample is a hit, whatever it weighs


# ---------------------------------------------------------------------------------------------------- count and ray_index
def test_padded_rows_leave_no_trace(tn, device):
    """the sync-free form's inputs, built by compact_hits(want_padded=True) on a batch with misses"""
    rng = np.random.default_rng(16)
    R, S, T = 300, 65, 50
    nv = rng.integers(0, 3, R).astype(np.int32)                               # a third of the rays miss
    order, count, padded = tn.cpp.compact_hits(_dev(nv, device), want_padded=True)
    n = int(count.item())
    assert n == int((nv > 0).sum()) and 0 < n < R and (padded[n:] == padded[0]).all()
    sigma, edges = tc.sigma_edges(rng, R, S)
    sigma[n:] = 3.0                                                           # the padded rows would show
    cells = tc.run_cells(rng, R, S, T)
    v = 8 * rng.random(R, dtype=np.float32)
    stats0 = tc.stats0(rng, T)
    d = lambda a: _dev(a, device)   # noqa: E731
    weights = tn.cpp.composite(d(sigma), None, d(edges)).cpu().numpy()
    want = render.tet_stats_statement(stats0, cells, weights, v, padded.cpu().numpy(), n)
    stats = d(stats0)
    tn.cpp.tet_stats_accumulate(stats, d(cells), d(sigma), d(edges), ray_value=d(v), ray_index=padded, count=count)
    assert np.array_equal(stats.cpu().numpy(), want)
    assert int((want - stats0)[:, 0].sum()) == n * S
    every = render.tet_stats_statement(stats0, cells, weights, v, padded.cpu().numpy(), None)
    assert not np.array_equal(every, want)                                    # (they would have been seen)
    # count = 0: untouched
    order0, count0, padded0 = tn.cpp.compact_hits(torch.zeros(R, dtype=torch.int32, device=device), want_padded=True)
    assert int(count0.item()) == 0
    stats = d(stats0)
    tn.cpp.tet_stats_accumulate(stats, d(cells), d(sigma), d(edges), ray_value=d(v), ray_index=padded0, count=count0)
    assert np.array_equal(stats.cpu().numpy(), stats0)


# --------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bytes_and_batches_add_up(tn, device):
    rng = np.random.default_rng(17)
    R, S, T = 200, 257, 23                                                    # few tetrahedra: the atomics of many waves meet
    sigma, edges = tc.sigma_edges(rng, R, S)
    cells, v = tc.run_cells(rng, R, S, T), 16 * rng.random(R, dtype=np.float32)
    d = lambda a: _dev(a, device)   # noqa: E731
    args = (d(cells), d(sigma), d(edges))
    stats0 = tc.stats0(rng, T)
    runs = []
    for _ in range(2):
        stats = d(stats0)
        tn.cpp.tet_stats_accumulate(stats, *args, ray_value=d(v))
        runs.append(stats.clone())
    assert torch.equal(runs[0], runs[1])
    tn.cpp.tet_stats_accumulate(stats, *args, ray_value=d(v))                 # a second batch onto the first
    weights = tn.cpp.composite(args[1], None, args[2]).cpu().numpy()
    once = render.tet_stats_statement(stats0, cells, weights, v)
    assert np.array_equal(runs[0].cpu().numpy(), once)
    assert np.array_equal(stats.cpu().numpy(), render.tet_stats_statement(once, cells, weights, v))


# ------------------------------------------------------------------------------------------------------------- render_train
@pytest.fixture(scope="module")
def small_scene(tn, device, scenes):
    pts, cells = scenes.random_mesh(900, 12)
    tr = tn.TetrahedraTracer(device)
    tr.load_tetrahedra(torch.from_numpy(pts).to(device), torch.from_numpy(cells).to(device))
    o, d = scenes.outside_in_rays(330, 13)
    nv = tr.trace_rays(_dev(np.ascontiguousarray(o, np.float32), device), _dev(np.ascontiguousarray(d, np.float32), device), 256)["num_visited_cells"]
    o, d = o[(nv > 0).cpu().numpy()], d[(nv > 0).cpu().numpy()]              # an all-hit batch
    assert len(o) > 300
    hit = dict(o=_dev(np.ascontiguousarray(o, np.float32), device), d=_dev(np.ascontiguousarray(d, np.float32), device))
    o, d = np.concatenate([o, o[:37] + 40.0]), np.concatenate([d, d[:37]])       # + rays that miss
    perm = np.random.default_rng(1).permutation(len(o))
    torch.manual_seed(5)
    mlp = render.TetraMLP().to(device)
    field = (torch.randn(64, len(pts), device=device) * 0.5).requires_grad_(True)
    return dict(tr=tr, mlp=mlp, field=field, hit=hit, T=len(cells),
                mixed=dict(o=_dev(np.ascontiguousarray(o[perm], np.float32), device), d=_dev(np.ascontiguousarray(d[perm], np.float32), device)))


def _pending_equals_the_statement(tn, rd, out, T, device, seed):
    pending = out["tet_stats_pending"]
    assert set(pending) == {"cell_indices", "sigma", "edges", "ray_index", "count"}
    r, S = pending["cell_indices"].shape
    assert tuple(pending["sigma"].shape) == (r, S) and tuple(pending["edges"].shape) == (r, S + 1) and S == rd.S + rd.S_fine + 1
    assert not pending["sigma"].requires_grad and pending["sigma"].is_contiguous() and pending["ray_index"].dtype == torch.int32
    R = out["rgb"].shape[0]
    ray_value = 4 * torch.rand(R, generator=torch.Generator().manual_seed(seed)).to(device)
    stats0 = _dev(tc.stats0(np.random.default_rng(seed), T), device)
    stats = stats0.clone()
    assert rd.accumulate_tet_stats(stats, pending, ray_value) is stats
    weights = tn.cpp.composite(pending["sigma"], None, pending["edges"])
    count = None if pending["count"] is None else int(pending["count"].item())
    want = render.tet_stats_statement(stats0, pending["cell_indices"], weights, ray_value, pending["ray_index"], count)
    assert np.array_equal(stats.cpu().numpy(), want)
    rows = r if count is None else count
    cells = pending["cell_indices"][:rows]
    assert int((stats - stats0)[:, 0].sum()) == int(((cells >= 0) & (cells < T)).sum()) > 0
    return pending, count


def test_render_train_compacting_form_with_capture(tn, device, small_scene):
    """case A: an all-hit batch in the compacting form (capture= selects it)"""
    sc = small_scene
    rd = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], 11, 256, num_fine_samples=7)
    capture = {}
    torch.manual_seed(3)
    out = rd.render_train(sc["hit"]["o"], sc["hit"]["d"], capture=capture, tet_stats=True)
    assert bool(out["ray_mask"].all())
    pending, count = _pending_equals_the_statement(tn, rd, out, sc["T"], device, 21)
    assert count is None and torch.equal(pending["ray_index"].long(), torch.nonzero(out["ray_mask"])[:, 0])
    assert torch.equal(pending["edges"], capture["edges"]) and torch.equal(pending["cell_indices"], capture["cell_indices"])
    # tet_stats=False: the result and its tensors are what they were
    torch.manual_seed(3)
    plain = rd.render_train(sc["hit"]["o"], sc["hit"]["d"], capture={})
    assert set(plain) == set(out) - {"tet_stats_pending"}
    for k in plain:
        assert torch.equal(plain[k], out[k]), k
    with pytest.raises(RuntimeError, match="fused=True"):
        rd.render_train(sc["hit"]["o"], sc["hit"]["d"], fused=False, tet_stats=True)


@pytest.mark.parametrize("threshold", [None, 0.5])
def test_render_train_sync_free_form_with_misses(tn, device, small_scene, threshold):
    """case B: the sync-free form on a batch with misses; with a threshold the culled samples have sigma = 0 -- hits without weight"""
    sc = small_scene
    rd = render.TetraRenderer(sc["tr"], sc["field"], sc["mlp"], 11, 256, num_fine_samples=7, sync_free_train=True, sync_free_min_hits=0.0)
    kw = {}
    if threshold is not None:
        kw = dict(occupancy=torch.rand(sc["T"], generator=torch.Generator().manual_seed(4)).to(device), occupancy_threshold=threshold)
    torch.manual_seed(3)
    out = rd.render_train(sc["mixed"]["o"], sc["mixed"]["d"], tet_stats=True, **kw)
    pending, count = _pending_equals_the_statement(tn, rd, out, sc["T"], device, 22)
    n = int(out["ray_mask"].sum())
    assert count == n and 0 < n < out["ray_mask"].numel() and pending["cell_indices"].shape[0] == out["ray_mask"].numel()
    assert torch.equal(pending["ray_index"][:n].long(), torch.nonzero(out["ray_mask"])[:, 0])
    if threshold is not None:
        culled = render.cull_mask_statement(pending["cell_indices"][:n], kw["occupancy"], threshold)
        assert 0.2 * culled.numel() < int(culled.sum()) < 0.8 * culled.numel() and not pending["sigma"][:n][culled].any()
        with pytest.raises(RuntimeError, match="occupancy_sampler"):
            rd.render_train(sc["mixed"]["o"], sc["mixed"]["d"], tet_stats=True, occupancy_sampler=True, **kw)
    torch.manual_seed(3)
    plain = rd.render_train(sc["mixed"]["o"], sc["mixed"]["d"], **kw)
    assert set(plain) == set(out) - {"tet_stats_pending"}
    for k in plain:
        assert torch.equal(plain[k], out[k]), k


# ----------------------------------------------------------------------------------------------------------------- the adapter
def test_adapter_gathers_and_densify_selects_by_the_statistics(tn, device, scenes, monkeypatch):
    ref = rm.load()
    plugin = importlib.import_module("tetra-nerf_amd.nerfstudio_plugin")
    optim = importlib.import_module("tetra-nerf_amd.optim")
    plugin.install(ref.TetrahedraNerf)
    try:
        pts, cells = scenes.random_mesh(1500, 31)
        model = rm.build_model(ref, pts, cells, num_samples=48, num_fine_samples=48).to(device)
        V, T = len(pts), len(cells)
        o, d = scenes.outside_in_rays(1024, 33)
        rb = rm.ray_bundle(ref, o, d, device, camera_indices=np.arange(len(o)) % 3)
        target = torch.rand(len(o), 3, device=device)
        opt = optim.FusedRAdam([model.tetrahedra_field] + plugin.weights_from_model(model), lr=1e-3)
        keys = set(model.state_dict())

        def train_step():
            opt.zero_grad(set_to_none=True)
            out = model(rb)
            assert "tet_stats_pending" not in out
            loss = model.get_loss_dict(out, {"image": target})
            loss["rgb_loss"].backward()
            opt.step()
            return out, loss

        model.train()
        train_step()
        assert getattr(model, "_tn_tet_stats", None) is None                  # off unless asked for
        model.config.densify_stats = True
        recorded = []
        real = tn.cpp.tet_stats_accumulate
        monkeypatch.setattr(tn.cpp, "tet_stats_accumulate", lambda stats, *a, **kw: (recorded.append((stats.clone(), a, kw)), real(stats, *a, **kw))[1])
        out, loss = train_step()
        assert set(loss) == {"rgb_loss"} and len(recorded) == 1
        # the step's own numbers: the squared error of every pixel over the pending samples
        before, (cells_p, sigma_p, edges_p), kw = recorded[0]
        ray_value = ((out["rgb"] - target) ** 2).sum(-1).detach()
        assert torch.equal(kw["ray_value"], ray_value) and not before.any()
        want = render.tet_stats_statement(before, cells_p, tn.cpp.composite(sigma_p, None, edges_p), ray_value, kw["ray_index"],
                                          None if kw["count"] is None else int(kw["count"].item()))
        assert np.array_equal(model._tn_tet_stats.cpu().numpy(), want)
        train_step()
        stats = model._tn_tet_stats.clone()
        assert tuple(stats.shape) == (T, 3) and len(recorded) == 2 and int(stats[:, 0].sum()) > int(torch.from_numpy(want)[:, 0].sum())
        assert set(model.state_dict()) == keys and model._tn_tet_stats_pending is None
        # densify: the k highest scores among the tetrahedra with enough hits, ties to the lower id
        k, min_hits = 40, 3
        score = render.tet_stats_scores(stats, "error").cpu().numpy()
        eligible = np.nonzero(stats[:, 0].cpu().numpy() >= min_hits)[0]
        expected = sorted(sorted(eligible.tolist(), key=lambda t: (-float(score[t]), t))[:k])
        assert len(eligible) > 2 * k
        tracer = model.get_tetrahedra_tracer()
        asked = []
        split = tracer.split_tetrahedra
        monkeypatch.setattr(tracer, "split_tetrahedra", lambda mask, **kw: (asked.append(torch.nonzero(mask)[:, 0].tolist()), split(mask, **kw))[1])
        res = plugin.densify(model, stats=True, min_hits=min_hits, max_new=k, optimizer=opt)
        assert asked == [expected]
        K = res["num_new"]
        assert res["counters"].tolist()[0] == k and K == res["counters"].tolist()[1] and 0 < K <= k
        assert res["stats_reset"] is True and tuple(model._tn_tet_stats.shape) == (T + 3 * K, 3) and not model._tn_tet_stats.any()
        assert tuple(model.tetrahedra_field.shape) == (64, V + K) and set(model.state_dict()) == keys
        train_step()                                                          # the model trains on, and the children gather from zero
        assert tuple(model._tn_tet_stats.shape) == (T + 3 * K, 3) and int(model._tn_tet_stats[:, 0].sum()) > 0
        assert bool(torch.isfinite(model.tetrahedra_field).all())
    finally:
        plugin.uninstall(ref.TetrahedraNerf)
