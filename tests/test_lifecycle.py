"""Second- and later-generation meshes without a GPU: the split applied to its own output (tests/lifecycle_lib.py: cube_gen1..5,
region_gen1..4, random30_gen1..4), and the optimiser state carried through two grows.

Layers: the generations are what they are named for (sizes, no refusal); every generation is conforming, keeps the stored
orientations and the hull of generation 0 (the checks of tests/test_split.py, called, not copied); the host emulation of the kernels
equals the statement byte for byte on generation g - 1 input; the piecewise-linear field of generation g is the generation-0 field
within the section-4.18 bound summed over the ancestors; optim.grow_parameter twice in a row against a float64 RAdam written out in
numpy.  (The kernels on these meshes, and the adapter's model living through the same splits: tests/test_lifecycle_gpu.py.)"""
import importlib

import numpy as np
import pytest
import torch

import lifecycle_lib as ll
import radam_cases as rc
import split_cases as sc
import test_split as ts


def test_the_generations_are_what_they_are_named_for(scenes):
    assert set(ll.GENERATION_CELLS) == {f"{f}_gen{g}" for f, depth in ll.DEPTH.items() for g in range(depth + 1)}
    smallest = {}
    for name in ll.names():
        xyz, cells, select, s = ll.step(scenes, name)
        counters = s["counters"].tolist()
        # no tetrahedron is refused: a change of the rule that starts refusing shows here, not as a silent shrink of the other tests
        assert counters == [int(select.sum()), int(select.sum()), 0, 0] and counters[0] > 0, (name, counters)
        assert len(s["cells"]) == ll.GENERATION_CELLS[name] == len(cells) + 3 * s["num_new"], (name, len(s["cells"]))
        assert len(s["vertices"]) == len(xyz) + s["num_new"]
        smallest[name] = float(np.abs(sc.vol6(s["vertices"].astype(np.float64)[s["cells"]])).min() / 6)
    assert all(len(ll.mesh(scenes, n)[1]) == T for n, T in ll.GENERATION_CELLS.items())
    print("smallest volume per generation:", {k: f"{v:.2e}" for k, v in smallest.items()})
    for family, depth in ll.DEPTH.items():                                     # the smallest volume falls, by about 4 per generation
        v = [smallest[f"{family}_gen{g}"] for g in range(1, depth + 1)]
        assert all(b < a for a, b in zip(v, v[1:])), (family, v)
    assert smallest["region_gen4"] < 1e-6
    # generation 1 of random30 is the case the split's own tests use
    assert np.array_equal(ll.step(scenes, "random30_gen1")[2], sc.case(scenes, "random_300_30pct")[2])
    # region: the ball holds a growing share of the mesh, and every generation asks children of the one before
    for g in range(2, 5):
        _, cells, select, _ = ll.step(scenes, f"region_gen{g}")
        T_before = ll.GENERATION_CELLS[f"region_gen{g - 2}"]
        assert select[T_before:].any(), g                                      # (tetrahedra the split before appended: second generation)


def _boundary(cells):
    """(sorted vertex triples of the faces in exactly one tetrahedron, the largest number of tetrahedra sharing a face)"""
    c = np.asarray(cells).view(np.uint32).astype(np.int64)
    faces = np.sort(np.concatenate([c[:, [1, 2, 3]], c[:, [0, 2, 3]], c[:, [0, 1, 3]], c[:, [0, 1, 2]]]), 1)
    uniq, count = np.unique(faces, axis=0, return_counts=True)
    return uniq[count == 1], int(count.max())


@pytest.mark.parametrize("name", ll.names())
def test_every_generation_is_conforming_and_keeps_orientations(scenes, oracle, name):
    xyz, cells, _, s = ll.step(scenes, name)
    ts.check_structure(oracle, xyz, cells, s, name)
    # every interior face is shared by exactly two cells, and the boundary faces are those of generation 0
    hull, most = _boundary(s["cells"])
    hull0, _ = _boundary(ll.mesh(scenes, name.rsplit("_gen", 1)[0] + "_gen0")[1])
    assert most == 2 and np.array_equal(hull, hull0), name


@pytest.mark.parametrize("name", ll.DEEPEST)
def test_emulated_kernels_equal_the_statement_on_generation_input(split_emul, tmp_path, scenes, name):
    """tests/host/split_emul.cpp (the element functions of csrc/tn_split_core.h) on the deepest step of each family"""
    g = sc.geometry()
    xyz, cells, select, want = ll.step(scenes, name)
    values = sc.values_for(len(xyz), ts.ROWS, seed=len(cells))
    got = ts._run_emul(split_emul, tmp_path, xyz, cells, select, values, 0)
    ts._assert_equal(got, want, name)
    rows = g.split_vertex_rows_statement(values, want["vertex_parents"])
    assert np.array_equal(sc.bits(got["rows"]), sc.bits(rows)) and np.array_equal(sc.bits(got["rows_vm"]), sc.bits(np.ascontiguousarray(rows.T))), name


split_emul = ts.split_emul      # the module-scoped fixture that builds the emulation


@pytest.mark.parametrize("family", sorted(ll.DEPTH))
def test_field_is_preserved_across_generations(scenes, family):
    """At the four vertices and the centroid of EVERY generation-g tetrahedron, in float64 and with no sample skipped:
        |generation-g field - generation-0 interpolant|  <=  sum over k = 1 .. g of  |l_k| (3u max|F| + |grad P|_1 3u max|coordinate|).
    The argument of tests/test_split.py::test_split_field_is_the_parent_field holds for one split whatever its input: with P the
    affine interpolant of the generation-(k-1) field on the parent and l_k the barycentric weight of the vertex that split added in
    the generation-k tetrahedron that holds x, the two piecewise-linear fields differ at x by EXACTLY l_k (F~_c - P(c~)), and by
    nothing where that tetrahedron was not split.  The children of a tetrahedron tile it exactly (they share its corners and the
    one fp32 centroid inside it), so x lies in one tetrahedron of every generation -- the ancestors of its own -- and
        I_g(x) - I_0(x) = sum_k (I_k(x) - I_(k-1)(x))
    telescopes; each term has its own bound, with max|F|, grad P and max|coordinate| taken from the generation-(k-1) parent, P
    solved in float64.  Both sides are float64 evaluations of fp32 data; the generation-0 interpolant is evaluated through a
    3 x 3 solve, whose own error -- the only float64 rounding that is not scaled by l_k -- is allowed as 2^-40 (max|F| +
    |grad P_0|_1 max|coordinate|) of the generation-0 ancestor: 2^-16 u, four orders below anything the bound measures."""
    rows = 4
    F = ll.fields(scenes, family, rows)
    xyz0, cells0 = ll.mesh(scenes, f"{family}_gen0")
    P0 = sc.parent_interpolant(xyz0, cells0, F[0])
    worst = {}
    for g in range(1, ll.DEPTH[family] + 1):
        name = f"{family}_gen{g}"
        xyz, cells = ll.mesh(scenes, name)
        p = xyz.astype(np.float64)[cells]                                      # [T, 4, 3]
        x = np.concatenate([p, p.mean(1, keepdims=True)], 1)                   # [T, 5, 3]: the corners and the centroid
        f = F[g].astype(np.float64).T[cells]                                   # [T, 4, rows]
        value = np.concatenate([f, f.mean(1, keepdims=True)], 1)               # [T, 5, rows]: the generation-g field there
        bound = np.zeros_like(value)
        anc = np.arange(len(cells))
        for k in range(g, 0, -1):
            pxyz, pcells, _, s = ll.step(scenes, f"{family}_gen{k}")
            T_before, K = len(pcells), s["num_new"]
            accepted = np.nonzero(np.diff(s["offsets"].astype(np.int64)))[0]
            slot = np.full(len(s["cells"]), -1)                               # where the added vertex sits; -1: not split
            slot[accepted] = 0
            slot[T_before:] = 1 + np.arange(3 * K) % 3
            assert np.array_equal(s["cells"][slot >= 0, slot[slot >= 0]] >= len(pxyz), np.ones((slot >= 0).sum(), bool))
            child = np.nonzero(slot[anc] >= 0)[0]
            parent = s["cell_parent"].astype(np.int64)[anc]
            if len(child):
                lam = ll.barycentrics64(s["vertices"].astype(np.float64)[s["cells"][anc[child]]], x[child])
                l_k = np.abs(lam[np.arange(len(child)), :, slot[anc[child]]])              # [n, 5]
                par = parent[child]
                _, grad, _ = sc.parent_interpolant(pxyz, pcells[par], F[k - 1])
                maxF = np.abs(F[k - 1].astype(np.float64).T[pcells[par]]).max(1)           # [n, rows]
                M = np.abs(pxyz.astype(np.float64)[pcells[par]]).max((1, 2))               # [n]
                bound[child] += l_k[:, :, None] * (3 * sc.U * maxF + np.abs(grad).sum(2) * 3 * sc.U * M[:, None])[:, None]
            anc = parent
        assert np.array_equal(anc, ll.ancestors(scenes, name))
        F0, grad0, p0 = (a[anc] for a in P0)
        want = F0[:, None] + np.einsum("nra,nsa->nsr", grad0, x - p0[:, None])
        maxF0 = np.abs(F[0].astype(np.float64).T[cells0[anc]]).max(1)
        M0 = np.abs(xyz0.astype(np.float64)[cells0[anc]]).max((1, 2))
        slack = 2.0 ** -40 * (maxF0 + np.abs(grad0).sum(2) * M0[:, None])[:, None]
        diff = np.abs(value - want)
        worst[name] = float((diff / (bound + slack)).max())
        print(f"{name}: {diff.size} samples, largest difference {diff.max():.3e}, largest difference / bound {worst[name]:.3f}")
        assert np.all(diff <= bound + slack), (name, worst[name])
        assert bound.max() > 0


# ------------------------------------------------------------------------------------------------------ the optimiser's state
LR, BETAS, EPS = rc.LR, rc.BETAS, rc.EPS


def _radam64(p, g, m, v, step):
    """one step of RAdam (Liu et al. 2020, torch.optim.RAdam's formulas, no weight decay) in float64 numpy"""
    b1, b2 = BETAS
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    rho_inf = 2 / (1 - b2) - 1
    rho = rho_inf - 2 * step * b2 ** step / bc2
    if rho > 5:
        rect = np.sqrt((rho - 4) * (rho - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho))
        p = p - LR * (m / bc1) * rect * np.sqrt(bc2) / (np.sqrt(v) + EPS)
    else:
        p = p - LR * (m / bc1)
    return p, m, v


def _rows64(values, parents, new):
    """split_vertex_rows_statement's rule in float64: the new columns are the mean of the four parent columns, or 0"""
    fresh = values[:, parents].mean(2) if new == "mean" else np.zeros((values.shape[0], len(parents)))
    return np.concatenate([values, fresh], 1)


def _grow_trajectory(kind, parents, grads, p0, new):
    """(p, exp_avg, exp_avg_sq) after every step: three steps, a grow, three steps, a grow, three steps.
    kind: "float64" (the numpy reference), "torch" (torch.optim.RAdam + optim.grow_parameter), "fused" (FusedRAdam's host side +
    optim.grow_parameter; its step is a kernel, so the steps between run on torch.optim.RAdam through the two state dicts, the
    interchange tests/test_radam_gpu.py pins on the device), "rebuilt" (fp32 torch RAdam re-created at every grow with the
    statement's rows written into a new state: the yardstick y, which never calls grow_parameter)."""
    optim = importlib.import_module("tetra-nerf_amd.optim")
    g = sc.geometry()
    out, it = [], 0
    if kind == "float64":
        p, m, v = p0.astype(np.float64), np.zeros(p0.shape), np.zeros(p0.shape)
        for phase in range(3):
            for _ in range(3):
                it += 1
                p, m, v = _radam64(p, grads[it - 1].astype(np.float64), m, v, it)
                out.append((p, m, v))
            if phase < 2:
                p, m, v = _rows64(p, parents[phase], "mean"), _rows64(m, parents[phase], new), _rows64(v, parents[phase], new)
        return out
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    other = torch.nn.Parameter(torch.zeros(5))                                 # a second parameter of the group, never grown
    make = lambda ps: torch.optim.RAdam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=False)   # noqa: E731
    opt = make([param, other])
    fused = None
    if kind == "fused":
        fused = optim.FusedRAdam([param, other], lr=LR, betas=BETAS, eps=EPS)
    for phase in range(3):
        for _ in range(3):
            it += 1
            param.grad, other.grad = torch.from_numpy(grads[it - 1].copy()), torch.ones(5)
            opt.step()
            st = opt.state[param]
            out.append(tuple(t.detach().numpy().astype(np.float64) for t in (param, st["exp_avg"], st["exp_avg_sq"])))
        if phase == 2:
            break
        vp = parents[phase]
        st = opt.state[param]
        rows = [g.split_vertex_rows_statement(t.detach().numpy(), vp, new=mode)
                for t, mode in ((param, "mean"), (st["exp_avg"], new), (st["exp_avg_sq"], new))]
        grown = torch.nn.Parameter(torch.from_numpy(rows[0].copy()))
        if kind == "rebuilt":
            step = st["step"].clone()
            other_state = {k: (t.clone() if isinstance(t, torch.Tensor) else t) for k, t in opt.state[other].items()}
            opt = make([grown, other])
            opt.state[grown] = {"step": step, "exp_avg": torch.from_numpy(rows[1].copy()), "exp_avg_sq": torch.from_numpy(rows[2].copy())}
            opt.state[other] = other_state
        elif kind == "torch":
            assert optim.grow_parameter(opt, param, grown, torch.from_numpy(rows[1].copy()), torch.from_numpy(rows[2].copy())) is grown
        else:
            fused.load_state_dict(opt.state_dict())
            optim.grow_parameter(fused, param, grown, torch.from_numpy(rows[1].copy()), torch.from_numpy(rows[2].copy()))
            assert fused.param_groups[0]["params"][0] is grown and param not in fused.state
            opt = make([grown, other])
            opt.load_state_dict(fused.state_dict())
        param = grown
    return out


@pytest.mark.parametrize("new", ("mean", "zero"))
@pytest.mark.parametrize("kind", ("torch", "fused"))
def test_optimiser_state_through_two_grows(monkeypatch, kind, new):
    """optim.grow_parameter twice in a row, three steps before, between and after, on a [4, V] parameter whose columns grow as the
    vertices of two splits do.  Reference: float64 RAdam in numpy, the rows carried in float64.  Bar (tests/test_radam_gpu.py::
    test_state_dict_to_torch_continues_within_4y_of_float64): after every step the parameter and both moments are within 4 y of the
    float64 reference, y = the same figure of an fp32 torch.optim.RAdam that is re-created at every grow and never sees
    grow_parameter."""
    optim = importlib.import_module("tetra-nerf_amd.optim")
    if kind == "fused":
        monkeypatch.setattr(optim, "_check_param", lambda p: None)            # its host side runs without a device
    rng = np.random.default_rng(17)
    V = (37, 11, 23)
    parents = [rng.integers(0, V[0], (V[1], 4)).astype(np.int32), rng.integers(0, V[0] + V[1], (V[2], 4)).astype(np.int32)]
    widths = [V[0]] * 3 + [V[0] + V[1]] * 3 + [sum(V)] * 3
    grads = [rc.gradient((4, w), 90, it).numpy() for it, w in enumerate(widths, 1)]
    p0 = rc.parameter((4, V[0]), 90).numpy()
    ref = _grow_trajectory("float64", parents, grads, p0, new)
    y = _grow_trajectory("rebuilt", parents, grads, p0, new)
    got = _grow_trajectory(kind, parents, grads, p0, new)
    err = lambda a, r: float(np.abs(a - r).max() / np.abs(r).max())   # noqa: E731
    failures = []
    for it, (a, b, r) in enumerate(zip(got, y, ref), 1):
        for what, ga, yb, rr in zip(("p", "exp_avg", "exp_avg_sq"), a, b, r):
            assert ga.shape == rr.shape == (4, widths[it - 1])
            e, f = err(ga, rr), err(yb, rr)
            print(f"RATIO grow {kind} new={new} step={it} {what}: {e:.3e} rebuilt-fp32 {f:.3e}")
            if not e <= 4 * f:
                failures.append((it, what, e, f))
    assert not failures, failures
