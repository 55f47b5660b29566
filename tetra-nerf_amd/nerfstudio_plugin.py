"""Reference-side wiring of the fused MI355X kernels into `TetrahedraNerf` (the nerfstudio model of the reference).

With only the `tetranerf_cpp_extension` shim `ns-train tetra-nerf` runs the HIP tracer, matcher
and gather, but the MLP, the samplers and the renderers stay nerfstudio's PyTorch modules -- the fp32-MFMA MLP
(`tn_mlp_forward_gather`), the one-launch render (`tn_render_rays`) and the training adjoints (`tn_mlp_backward`,
`tn_composite_backward`) are never reached.  This module closes that gap without touching the reference's files:

    import tetranerf.nerfstudio.model as ref_model
    from tetranerf_amd.nerfstudio_plugin import install
    install(ref_model.TetrahedraNerf)            # get_outputs now runs TetraRenderer.render / render_train

or, without monkey-patching, `FusedTetrahedraNerf = make_fused_model_class(ref_model.TetrahedraNerf)` and point
`TetrahedraNerfConfig._target` at it (registration.py:20-67 builds the two method configs from that class).

What is mapped (reference: /root/reference/tetranerf/nerfstudio/model.py):

    get_outputs                                   :520-662   -> fused_get_outputs (below)
    mlp_base.layers[0..2]                         :436-441   -> w1,b1 / w2,b2 / w3,b3     [128,64] [128,128] [128,128]
    field_output_density.net                      :456       -> wd,bd                     [1,128]   (+ softplus)
    mlp_head.layers[0]  (in = [dir enc 27 | base 128]) :449-454 -> wh,bh                  [128,155]
    field_output_color.net                        :455       -> wr,br                     [3,128]   (+ sigmoid)
    tetrahedra_field                              :247-256   -> the [64,V] field (cached vertex-major shadow)
    sampler_uniform / TetrahedraSampler / sampler_pdf  :459-463,111-192 -> render.uniform/biased/pdf_sample_bins
    renderer_rgb(background) / accumulation / depth    :466-468  -> tn_composite (+ adjoint)
    GradientScaler                                :195-205,625-630 -> render.GradientScaler
    state dict keys                               :273-300   -> weights_from_state_dict

    appearance_embedding (appearance_embed_dim = E > 0) :437-447,608-620 -> the E extra columns of mlp_head collapse to a
                                                  per-RAY bias c = Wh[:, 155:] emb(camera) (training: the ray's camera; evaluation:
                                                  the mean embedding), made here in PyTorch ([R,E] x [E,128], differentiable) and
                                                  added by the kernels to the head pre-activation (`ray_head_bias`)

Fallback rule (the fused kernels hard-code the shipped architecture 64 -> 128^3 -> (27 + 128 [+ E]) -> 128 -> 3): any other
configuration -- `field_dim != 64`, `hidden_size != 128`, `num_density_layers != 3`, `num_color_layers != 1`,
`input_fourier_frequencies > 0`, a `background_color` that is not a constant on the call -- runs the
REFERENCE `get_outputs` unchanged (i.e. the HIP tracer / matcher / gather under nerfstudio's PyTorch MLP): same results as
the reference, just without the fused speed-up.  `fused_config_supported` states the rule; both method configs the
reference registers (`tetra-nerf-original`, `tetra-nerf`) are supported.

Opt-ins (fields the reference's config does not have; absent = off, read with getattr): `position_gradients` (gradients for
origins / directions / vertices), `train_mlp_mode` ("bf16x3": the forward kernels of a training iteration), `train_adjoint_mode`
("bf16x3": the dX chain of the MLP adjoint, independent of the forward's mode), `train_dw_mode` ("bf16x3": the four
weight-gradient GEMMs of the MLP adjoint, independent of both), `eval_mlp_mode` ("bf16x3" / "bf16"), and -- only for a model that
has the reference's own `tetrahedra_occupancy` buffer (`use_occupancy_field=True`, model.py:98-99,256-265: registered there, never
used) -- `occupancy_threshold` (evaluation renders skip the network in tetrahedra below it), `occupancy_decay` (training
batches update the buffer: max(decay occupancy, max density seen)) and `occupancy_train_threshold` (training batches skip the
network in tetrahedra below it, except every `occupancy_refresh_every`-th one, default 16, which runs unculled); and
`refit_vertices` (the tracer follows a vertex table an optimiser moves: `_follow_vertices` below) with `vertex_step_fraction`
(each followed move is first shortened so that no tetrahedron turns inside out: `TetrahedraTracer.limit_vertex_step`) and
`delaunay_check_every` / `retriangulate_above` (every so many followed iterations the interior faces that stopped being Delaunay
are counted, and above that fraction of them the vertices get new cells: `_monitor_delaunay` below; with `delaunay_repair =
"flip"` the violated faces are first flipped on the device and Qhull runs only for what is left above the threshold).

nerfstudio is not installed in this environment: the adapter is duck-typed (it only touches the attribute names listed
above) and is tested with stand-ins of nerfstudio's MLP / FieldHead / RayBundle (tests/golden/nerfstudio_standins.py).
"""
from __future__ import annotations

import sys
from typing import Dict, List, Tuple

import torch

# state-dict keys of the 12 kernel weight tensors, in kernel order (w1,b1,w2,b2,w3,b3,wd,bd,wh,bh,wr,br)
STATE_DICT_KEYS = (
    "mlp_base.layers.0.weight", "mlp_base.layers.0.bias",
    "mlp_base.layers.1.weight", "mlp_base.layers.1.bias",
    "mlp_base.layers.2.weight", "mlp_base.layers.2.bias",
    "field_output_density.net.weight", "field_output_density.net.bias",
    "mlp_head.layers.0.weight", "mlp_head.layers.0.bias",
    "field_output_color.net.weight", "field_output_color.net.bias",
)
FIELD_KEY = "tetrahedra_field"
_SHAPES = [(128, 64), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,), (128, 155), (128,), (3, 128), (3,)]


def weights_from_state_dict(state_dict, prefix: str = "") -> Tuple[List[torch.Tensor], torch.Tensor]:
    """(the 12 weight tensors in kernel order, the [64,V] field) out of a reference checkpoint's model state dict
    (`prefix` = "_model." for a nerfstudio pipeline checkpoint: ckpt["pipeline"]).  Shapes are checked: a checkpoint
    of a non-default architecture raises."""
    ws = []
    for k, shp in zip(STATE_DICT_KEYS, _SHAPES):
        t = state_dict[prefix + k]
        if tuple(t.shape) != shp:
            raise RuntimeError(f"{prefix + k}: shape {tuple(t.shape)} is not the shipped architecture's {shp} "
                               "(fused kernels: 64 -> 128^3 -> (27+128) -> 128 -> 3)")
        ws.append(t)
    field = state_dict[prefix + FIELD_KEY]
    if field.dim() != 2 or field.shape[0] != 64:
        raise RuntimeError(f"{prefix + FIELD_KEY}: expected [64, V], got {tuple(field.shape)}")
    return ws, field


def weights_from_model(model) -> List[torch.Tensor]:
    """The 12 live parameters of a TetrahedraNerf (model.py:436-456), in kernel order."""
    b, h = model.mlp_base.layers, model.mlp_head.layers
    if len(b) != 3 or len(h) != 1:
        raise RuntimeError("fused kernels need num_density_layers = 3 and num_color_layers = 1")
    d, c = model.field_output_density.net, model.field_output_color.net
    return [b[0].weight, b[0].bias, b[1].weight, b[1].bias, b[2].weight, b[2].bias, d.weight, d.bias,
            h[0].weight, h[0].bias, c.weight, c.bias]


class ModelMLP:
    """What TetraRenderer needs of an MLP, served by the reference model's own modules: `fused_weights()` for the
    kernels, `__call__` (the modules themselves, model.py:602-621) for the unfused path."""

    def __init__(self, model):
        self.model = model

    def fused_weights(self):
        """The 12 kernel tensors.  With an appearance embedding mlp_head's weight is [128, 155 + E]: the kernels take its
        first 155 columns (a differentiable slice while a graph is recorded; cached per parameter version otherwise, so
        that evaluation does not re-pack the weights on every call); the other E act through `ray_head_bias`."""
        ws = weights_from_model(self.model)
        wh = ws[8]
        if wh.shape[1] != 155:
            if torch.is_grad_enabled() and wh.requires_grad:
                ws[8] = wh[:, :155].contiguous()
            else:
                hit = getattr(self, "_wh_main", None)
                if hit is None or hit[0] != (wh._version, wh.data_ptr()):
                    hit = self._wh_main = ((wh._version, wh.data_ptr()), wh.detach()[:, :155].contiguous())
                ws[8] = hit[1]
        return ws

    def ray_head_bias(self, ray_bundle):
        """[R, 128] per-ray bias of the head layer = Wh[:, 155:] applied to the ray's appearance embedding, exactly the
        embedded_appearance of model.py:608-620 (training: the embedding of the ray's camera; evaluation: the mean
        embedding for every ray); None without an appearance embedding."""
        m = self.model
        E = int(getattr(m.config, "appearance_embed_dim", 0))
        if E <= 0:
            return None
        wa = m.mlp_head.layers[0].weight[:, 155:155 + E]
        R = ray_bundle.origins.reshape(-1, 3).shape[0]
        if m.training:
            assert ray_bundle.camera_indices is not None
            emb = m.appearance_embedding(ray_bundle.camera_indices.reshape(-1))       # [R, E]
            return (emb @ wa.t()).contiguous()
        mean = m.appearance_embedding.weight.mean(dim=0)                              # [E]
        return (mean @ wa.t())[None, :].expand(R, -1).contiguous()

    def coarse_sigma(self, feats):
        """density of the coarse pass (model.py:577-581) -> [..., S]"""
        m = self.model
        return m.field_output_density(m.mlp_base(m.position_encoding(feats)))[..., 0]

    def __call__(self, feats, dirs):
        m = self.model
        x = m.mlp_base(m.position_encoding(feats))
        sigma = m.field_output_density(x)
        h = m.mlp_head(torch.cat([m.direction_encoding(dirs), x], dim=-1))
        return sigma, m.field_output_color(h)


def fused_config_supported(config) -> Tuple[bool, str]:
    """The fallback rule of the module docstring: (True, "") or (False, reason)."""
    g = lambda k, dflt: getattr(config, k, dflt)   # noqa: E731
    checks = (
        (g("field_dim", 64) == 64, "field_dim != 64"),
        (g("hidden_size", 128) == 128, "hidden_size != 128"),
        (g("num_density_layers", 3) == 3, "num_density_layers != 3"),
        (g("num_color_layers", 1) == 1, "num_color_layers != 1"),
        (g("input_fourier_frequencies", 0) == 0, "input_fourier_frequencies > 0"),
        (g("appearance_embed_dim", 0) >= 0, "appearance_embed_dim < 0"),
        (g("background_color", "white") not in ("random", "last_sample"), "background_color is not a constant"),
        (g("num_samples", 256) >= 1, "num_samples < 1"),
    )
    for ok, why in checks:
        if not ok:
            return False, why
    return True, ""


def resolve_background(model):
    """The colour nerfstudio's RGB renderer will blend with on THIS call, resolved the way the reference does it
    (`get_background_color`, model.py:504-518; `RGBRenderer.combine_rgb`): `renderers.BACKGROUND_COLOR_OVERRIDE` when a
    `background_color_override_context` is active (the viewer / exporters use it), else `renderer_rgb.background_color`,
    else `config.background_color`.  Returns a grey level (float), an (r, g, b) tuple, or None when the colour is not a
    constant ("random", "last_sample": the fused kernels do not implement them -> reference body)."""
    renderers = sys.modules.get("nerfstudio.model_components.renderers")
    bg = getattr(renderers, "BACKGROUND_COLOR_OVERRIDE", None) if renderers is not None else None
    if bg is None:
        bg = getattr(getattr(model, "renderer_rgb", None), "background_color", None)
    if bg is None:
        bg = getattr(model.config, "background_color", "white")
    if isinstance(bg, str):
        if bg in ("white", "black"):
            return 1.0 if bg == "white" else 0.0
        colors = sys.modules.get("nerfstudio.utils.colors")
        if colors is None or bg not in getattr(colors, "COLORS_DICT", {}):
            return None
        bg = colors.COLORS_DICT[bg]
    # A colour TENSOR is read back once per (object, version, storage): get_outputs runs per batch, and a device tensor
    # (nerfstudio keeps its colours on the host, an override may not) would cost a host synchronisation every time -- in the
    # middle of the sync-free training path.  The key changes when the tensor is replaced or written in place.
    key = (id(bg), getattr(bg, "_version", None), bg.data_ptr()) if isinstance(bg, torch.Tensor) else None
    if key is not None and _BG_CACHE.get("key") == key and _BG_CACHE.get("ref", lambda: None)() is bg:
        return _BG_CACHE["value"]
    t = torch.as_tensor(bg).detach().to(dtype=torch.float32, device="cpu").reshape(-1)   # colours live on the host in nerfstudio
    if t.numel() != 3:
        value = None
    else:
        r, g, b = t.tolist()
        value = r if r == g == b else (r, g, b)
    if key is not None:
        import weakref

        _BG_CACHE.update(key=key, value=value, ref=weakref.ref(bg))
    return value


_BG_CACHE: dict = {}


def _renderer_for(model, tracer):
    from . import render

    rd = getattr(model, "_tn_renderer", None)
    if rd is not None and rd.tracer is tracer and rd.field is model.tetrahedra_field:
        return rd
    cfg = model.config
    rd = render.TetraRenderer(
        tracer, model.tetrahedra_field, ModelMLP(model), num_samples=int(cfg.num_samples),
        max_ray_triangles=int(cfg.max_intersected_triangles), fused=True, far_plane=float(model.collider.far_plane),
        num_fine_samples=int(getattr(cfg, "num_fine_samples", 0)), biased=bool(getattr(cfg, "use_biased_sampler", False)),
        background=1.0)     # every call passes the colour resolve_background() found
    # plain attribute (not a registered submodule / buffer): nothing of it enters the state dict
    object.__setattr__(model, "_tn_renderer", rd)
    return rd


def _accumulate(model, name, counters):
    """`counters` added to `model.<name>`, an int64 tensor on their device, created by the first call (and again on another
    device); without a model nothing is kept"""
    if model is None:
        return
    total = getattr(model, name, None)
    if total is None or total.device != counters.device:
        total = torch.zeros(4, dtype=torch.int64, device=counters.device)
        setattr(model, name, total)
    total += counters


def _adopt_mesh(model, tracer, cells, *, vertices=None, occupancy=None):
    """The model takes the mesh its tracer has just loaded, in the order of DESIGN.md section 4.18.1: (1) `tetrahedra_vertices`
    (where `vertices` is given; the tracer is re-pointed at it, the storage it borrows), `tetrahedra_cells` and
    `tetrahedra_occupancy` (where `occupancy` is given) REPLACED under their names, each of its kind (`_set_tensor`), so a state
    dict keeps its keys; (2) `config.num_tetrahedra_vertices` / `num_tetrahedra_cells` where the config has them; (3) the vertex
    snapshot refreshed iff the tracer keeps one, the vertex key taken again; (4) the statistics, where the model has any, zeros of
    the new size.  model None: (3) alone.  Returns the tracer's vertex table."""
    if model is not None:
        if vertices is not None:
            vertices = tracer.tetrahedra_vertices = _set_tensor(model, "tetrahedra_vertices", vertices, model.tetrahedra_vertices)
        _set_tensor(model, "tetrahedra_cells", cells)
        if occupancy is not None:
            _set_tensor(model, "tetrahedra_occupancy", occupancy)
        cfg = getattr(model, "config", None)
        if vertices is not None and hasattr(cfg, "num_tetrahedra_vertices"):
            cfg.num_tetrahedra_vertices = vertices.shape[0]
        if hasattr(cfg, "num_tetrahedra_cells"):
            cfg.num_tetrahedra_cells = cells.numel() // 4
    v = tracer.tetrahedra_vertices
    if getattr(tracer, "_tn_vertex_snapshot", None) is not None:
        tracer._tn_vertex_snapshot = v.detach().clone()
    tracer._tn_vertex_key = (v._version, v.data_ptr())
    if model is not None and getattr(model, "_tn_tet_stats", None) is not None:     # statistics of cells that no longer exist
        model_tet_stats(model, reset=True, num_cells=cells.numel() // 4)
    return v


def _monitor_delaunay(tracer, model, above, keep_snapshot):
    """One look at the Delaunay monitor (`config.delaunay_check_every`), and a re-triangulation where
    `config.retriangulate_above` asks for one.  The counters of `tracer.delaunay_check()` on the vertices the tracer follows
    (interior faces, violated, uncertain, violated with an inverted first tetrahedron) accumulate in
    `model._tn_delaunay_counters`, an int64 tensor on the device.  With a threshold the first two are read back -- the ONE host
    synchronisation of the monitor -- and when violated / interior exceeds it `tracer.retriangulate` gives the vertices new cells
    (blocking: Qhull on the CPU, then a load) and the model adopts them (`_adopt_mesh`): `tetrahedra_cells` and, where it has one,
    its `tetrahedra_occupancy` (carried over conservatively: `remap_tet_values`) are replaced, `_tn_retriangulations` counts the
    re-triangulation.  What is keyed by vertex -- the field, its optimiser state -- does not change.  keep_snapshot (the caller's
    vertex_step_fraction is set) decides nothing any more: `_follow_vertices` keeps a snapshot exactly then, and `_adopt_mesh`
    refreshes the one the tracer keeps.  With `config.delaunay_repair = "flip"` (opt-in) flips on the device are tried first and
    Qhull runs only for what they leave above the threshold (below).  Returns True after a re-triangulation or a repair by flips."""
    counters = tracer.delaunay_check()["counters"]
    _accumulate(model, "_tn_delaunay_counters", counters)
    if above is None:
        return False
    interior, violated = counters[:2].tolist()
    if interior == 0 or violated <= float(above) * interior:
        return False
    occupancy = getattr(model, "tetrahedra_occupancy", None) if model is not None else None
    repair = getattr(getattr(model, "config", None), "delaunay_repair", None)
    if repair is not None:
        # config.delaunay_repair = "flip" (opt-in; absent or None: the re-triangulation alone, call for call): flips of the violated
        # faces on the device first (`tracer.flip_to_delaunay`) -- no vertex moves, the occupancy is carried
        # by `flip_tet_values`, the model adopts the cells and `_tn_flip_repairs` counts the repair --, and Qhull only where the
        # violated share that flips could not remove is still above the threshold.
        if repair != "flip":
            raise ValueError('config.delaunay_repair must be "flip" or absent')
        if not getattr(tracer, "supports_flip", False):
            raise RuntimeError('config.delaunay_repair = "flip" needs a tracer with flip_to_delaunay (tetranerf_cpp_extension.TetrahedraTracer)')
        # config.delaunay_repair_reload = "once" (opt-in; absent or None: the call below with exactly the arguments it had): the
        # rounds read face tables built from the cells alone and the tracer is loaded once at the end
        reload = getattr(model.config, "delaunay_repair_reload", None)
        if reload is not None:
            if reload not in ("round", "once"):
                raise ValueError('config.delaunay_repair_reload must be "round", "once" or absent')
            if not getattr(tracer, "supports_face_table", False):
                raise RuntimeError("config.delaunay_repair_reload needs a tracer whose flip_to_delaunay takes reload= "
                                   "(tetranerf_cpp_extension.TetrahedraTracer)")
        tet_values = () if occupancy is None else (occupancy.detach(),)
        out = tracer.flip_to_delaunay(tet_values=tet_values) if reload is None else tracer.flip_to_delaunay(tet_values=tet_values, reload=reload)
        if out["num_rounds"]:
            _adopt_mesh(model, tracer, out["cells"], occupancy=None if occupancy is None else out["tet_values"][0])
            model._tn_flip_repairs = getattr(model, "_tn_flip_repairs", 0) + 1
            occupancy = getattr(model, "tetrahedra_occupancy", None)
        if out["violated"] <= float(above) * out["rounds"][-1][0]:
            return bool(out["num_rounds"])
    out = tracer.retriangulate(tracer.tetrahedra_vertices, () if occupancy is None else (occupancy.detach(),))
    _adopt_mesh(model, tracer, out["cells"], occupancy=None if occupancy is None else out["tet_values"][0])
    if model is not None:
        model._tn_retriangulations = getattr(model, "_tn_retriangulations", 0) + 1
    return True


def _follow_vertices(tracer, model=None, fraction=None, delaunay_check_every=None, retriangulate_above=None):
    """`config.refit_vertices` (opt-in; no such field in the reference's config): the tracer's tables follow the vertex table
    it borrows.  The (version counter, storage) of `tracer.tetrahedra_vertices` is remembered at load / refit and the tracer is
    refitted (`update_vertices`: the cells stay, everything that holds positions is recomputed) before the trace whenever
    either moved -- the rule the field shadow cache uses.  The model's own `get_tetrahedra_tracer` loads without the refit
    tables, so the first call loads once more with them.  A write through `.data` bumps no counter: call
    `tracer.update_vertices(v)` yourself after one.

    `config.vertex_step_fraction` (opt-in, with refit_vertices; absent or None: the route above, call for call): a snapshot of the
    vertices is kept at every load / refit, and a move is first shortened against it -- `limit_vertex_step(snapshot, v.data,
    fraction)` writes the vertex tensor in place, so the optimiser's parameter itself holds the limited positions -- then the
    tracer is refitted and the snapshot updated.  The key is taken again after the in-place write.  The call's counters
    (clamped, frozen but asked to move, flipped, collapsed) accumulate in `model._tn_vertex_step_counters`, an int64 tensor on
    the device; nothing is read back here.

    `config.delaunay_check_every` (opt-in, with refit_vertices; absent or None: nothing new runs) with `config.retriangulate_above`
    (a fraction of the interior faces; None: the monitor only counts): on every delaunay_check_every-th call, after the tracer
    has followed the vertices, `_monitor_delaunay` above."""
    if not getattr(tracer, "supports_refit", False):
        raise RuntimeError("config.refit_vertices needs a tracer with update_vertices (tetranerf_cpp_extension.TetrahedraTracer)")
    if delaunay_check_every is not None and not getattr(tracer, "supports_delaunay_check", False):
        raise RuntimeError("config.delaunay_check_every needs a tracer with delaunay_check (tetranerf_cpp_extension.TetrahedraTracer)")
    if fraction is not None and not getattr(tracer, "supports_vertex_step_limit", False):
        raise RuntimeError("config.vertex_step_fraction needs a tracer with limit_vertex_step (tetranerf_cpp_extension.TetrahedraTracer)")
    v = tracer.tetrahedra_vertices
    key = (v._version, v.data_ptr())
    snapshot = getattr(tracer, "_tn_vertex_snapshot", None) if fraction is not None else None
    if not getattr(tracer, "_refittable", False):
        tracer.load_tetrahedra(v, tracer.tetrahedra_cells, refittable=True)
        snapshot = None
    elif getattr(tracer, "_tn_vertex_key", None) != key:
        if snapshot is not None and snapshot.shape == v.shape:
            counters, _ = tracer.limit_vertex_step(snapshot, v.data, float(fraction))
            _accumulate(model, "_tn_vertex_step_counters", counters)
        else:
            snapshot = None          # first sight of a tracer someone else loaded: nothing valid to limit against
        tracer.update_vertices(v)
        if snapshot is not None:
            snapshot.copy_(v.detach())
        key = (v._version, v.data_ptr())
    if fraction is not None and snapshot is None:
        tracer._tn_vertex_snapshot = v.detach().clone()
    tracer._tn_vertex_key = key
    if delaunay_check_every is not None:
        calls = tracer._tn_follow_calls = getattr(tracer, "_tn_follow_calls", 0) + 1
        if int(delaunay_check_every) >= 1 and calls % int(delaunay_check_every) == 0:
            _monitor_delaunay(tracer, model, retriangulate_above, fraction is not None)


def fused_get_outputs(model, ray_bundle) -> Dict[str, torch.Tensor]:
    """Drop-in body of TetrahedraNerf.get_outputs (model.py:520-662) on the fused kernels: training mode = stratified
    samples + autograd through the HIP adjoints (`render_train`), evaluation = `render`; same output dictionary
    ("rgb", "accumulation", "depth", "ray_mask"; with config.aux_outputs or config.distortion_loss_mult also "expected_depth" and
    "distortion").  Unsupported configurations run the reference implementation (and have no such outputs)."""
    ok, _why = fused_config_supported(model.config)
    ref = getattr(type(model), "_tn_reference_get_outputs", None)
    bg = resolve_background(model) if ok else None
    if ok and bg is None:
        ok, _why = False, "background colour is not a constant on this call"
    if not ok:
        if ref is None:
            raise RuntimeError(f"fused path unsupported ({_why}) and no reference get_outputs to fall back to")
        return ref(model, ray_bundle)
    if model.mlp_base is None:
        raise ValueError("populate_fields() must be called before get_outputs")
    tracer = model.get_tetrahedra_tracer()          # lazy mesh initialisation + structure build (model.py:394-407)
    step_fraction = getattr(model.config, "vertex_step_fraction", None)
    check_every = getattr(model.config, "delaunay_check_every", None)
    if getattr(model.config, "refit_vertices", False):
        if check_every is None:
            _follow_vertices(tracer, model, step_fraction)
        else:
            _follow_vertices(tracer, model, step_fraction, check_every, getattr(model.config, "retriangulate_above", None))
    elif check_every is not None:
        raise ValueError("config.delaunay_check_every needs config.refit_vertices = True: the monitor looks at the vertices the "
                         "tracer follows, and a re-triangulation reloads that tracer")
    elif step_fraction is not None:
        raise ValueError("config.vertex_step_fraction needs config.refit_vertices = True: the limiter shortens a move against "
                         "the vertices of the last refit, and only a tracer that follows the vertices has one")
    rd = _renderer_for(model, tracer)
    o = ray_bundle.origins.reshape(-1, 3).contiguous()
    d = ray_bundle.directions.reshape(-1, 3).contiguous()
    hb = rd.mlp.ray_head_bias(ray_bundle)       # appearance embedding -> per-ray head bias (None without one)
    if model.training:
        # the reference's samplers stratify and its RGB renderer skips the clamp whenever `self.training` is set, with
        # or without autograd (model.py:169; nerfstudio RGBRenderer.forward); render_train skips the activation saves
        # when no graph is being recorded
        kw = {}
        if getattr(model.config, "position_gradients", False):
            # opt-in (no such field in the reference's config): gradients for ray bundles whose origins / directions require
            # them (nerfstudio's camera optimiser) and for a vertex table that does; see TetraRenderer.render_train
            kw["position_gradients"] = True
        train_mode = getattr(model.config, "train_mlp_mode", None)
        if train_mode is not None:
            # opt-in as well (an absent field: fp32): "bf16x3" = the forward kernels of a training iteration in the split-operand
            # bf16 arithmetic, fp32 adjoints (TetraRenderer.render_train: mlp_mode)
            kw["mlp_mode"] = str(train_mode)
        adjoint_mode = getattr(model.config, "train_adjoint_mode", None)
        if adjoint_mode is not None:
            # opt-in, independent of train_mlp_mode (an absent field: fp32): "bf16x3" = the matrix products of the dX chain in the
            # split-operand bf16 arithmetic (TetraRenderer.render_train: adjoint_mode)
            kw["adjoint_mode"] = str(adjoint_mode)
        dw_mode = getattr(model.config, "train_dw_mode", None)
        if dw_mode is not None:
            # opt-in, independent of the other two (an absent field: fp32): "bf16x3" = the weight-gradient GEMMs in the
            # split-operand bf16 arithmetic (TetraRenderer.render_train: dw_mode)
            kw["dw_mode"] = str(dw_mode)
        occupancy = getattr(model, "tetrahedra_occupancy", None)
        decay = getattr(model.config, "occupancy_decay", None)
        if occupancy is not None and decay is not None:
            # opt-in (no such field in the reference's config; the BUFFER is the reference's own, registered under
            # use_occupancy_field=True and left unused there): updated in place once per batch; training itself is not culled
            kw["occupancy"], kw["occupancy_decay"] = occupancy, float(decay)
        train_threshold = getattr(model.config, "occupancy_train_threshold", None)
        if occupancy is not None and train_threshold is not None:
            # opt-in, a field of its own (`occupancy_threshold` stays what it was: evaluation only): training batches skip the network
            # in tetrahedra below it (TetraRenderer.render_train: occupancy_threshold; one host synchronisation per culled batch).
            # A culled tetrahedron contributes sigma = 0, so the update can only decay it: every occupancy_refresh_every-th training
            # batch of the renderer (default 16; below 1: never) runs UNCULLED, which is what lets such a tetrahedron come back
            every = int(getattr(model.config, "occupancy_refresh_every", 16))
            batch = rd._tn_train_batches = getattr(rd, "_tn_train_batches", 0) + 1
            if every < 1 or batch % every != 0:
                kw["occupancy"], kw["occupancy_threshold"] = occupancy, float(train_threshold)
                if getattr(model.config, "occupancy_sampler", False):
                    # opt-in (an absent field: off): the culled batches place their samples in live tetrahedra only
                    # (TetraRenderer.render_train: occupancy_sampler); the unculled refresh batches keep the ordinary sampler, which is
                    # how a culled tetrahedron still gets seen
                    kw["occupancy_sampler"] = True
        if _wants_aux_outputs(model.config):
            kw["aux_outputs"] = True
        if not getattr(model.config, "densify_stats", False):
            return rd.render_train(o, d, gradient_scaling=bool(getattr(model.config, "use_gradient_scaling", False)), background=bg,
                                   ray_head_bias=hb, **kw)
        # opt-in (an absent field: off): per-tetrahedron training statistics for densify(stats=True).  The batch's sample
        # placement is kept on the model until fused_get_loss_dict knows the error of every ray -- a plain attribute, nothing of it
        # enters the state dict.  Batches of the occupancy-guided sampler are not counted (render_train refuses the combination:
        # their edges are live-length coordinates); the unculled refresh batches are.
        kw["tet_stats"] = not kw.get("occupancy_sampler", False)
        res = rd.render_train(o, d, gradient_scaling=bool(getattr(model.config, "use_gradient_scaling", False)), background=bg,
                              ray_head_bias=hb, **kw)
        pending = res.pop("tet_stats_pending", None)
        object.__setattr__(model, "_tn_tet_stats_pending", None if pending is None else (rd, pending))
        return res
    kw = {}
    if _wants_aux_outputs(model.config):
        kw["aux_outputs"] = True
    occupancy = getattr(model, "tetrahedra_occupancy", None)
    threshold = getattr(model.config, "occupancy_threshold", None)
    if occupancy is not None and threshold is not None:
        # opt-in as above: samples in tetrahedra whose occupancy is below the threshold skip the network (TetraRenderer.render)
        kw["occupancy"], kw["occupancy_threshold"] = occupancy, float(threshold)
        if getattr(model.config, "occupancy_sampler", False):
            kw["occupancy_sampler"] = True      # opt-in: the S samples go where something is (TetraRenderer.render)
    eval_mode = getattr(model.config, "eval_mlp_mode", None)
    if eval_mode is not None:
        # opt-in like train_mlp_mode (an absent field, as in the reference's config: the renderer's own fp32): "bf16" = the fast
        # evaluation arithmetic below the parity bar (TetraRenderer.render: mlp_mode)
        kw["mlp_mode"] = str(eval_mode)
    return rd.render(o, d, background=bg, ray_head_bias=hb, **kw)


def _wants_aux_outputs(config) -> bool:
    """opt-in (no such fields in the reference's config): `aux_outputs` truthy, or a `distortion_loss_mult`, adds "expected_depth"
    and "distortion" to the outputs (TetraRenderer.render_train / render: aux_outputs)."""
    return bool(getattr(config, "aux_outputs", None)) or getattr(config, "distortion_loss_mult", None) is not None


def fused_get_loss_dict(model, outputs, batch, metrics_dict=None):
    """The reference's get_loss_dict, its dictionary returned UNCHANGED unless config.distortion_loss_mult is set and the outputs
    carry "distortion" (a configuration that fell back to the reference body has no such output): then "distortion_loss" =
    mult * mean(distortion) is added -- what nerfstudio's models add from losses.distortion_loss; here the per-ray value comes out
    of the fused composite node.  A depth-supervision loss is the caller's: "expected_depth" is in the outputs."""
    ref = getattr(type(model), "_tn_reference_get_loss_dict", None)
    if ref is None:
        raise RuntimeError("no reference get_loss_dict to wrap: install() / make_fused_model_class() set it")
    loss_dict = ref(model, outputs, batch, metrics_dict)
    held = getattr(model, "_tn_tet_stats_pending", None)
    if held is not None:
        # config.densify_stats: the squared error of every rendered pixel, spread over the tetrahedra its ray's weights fell into
        object.__setattr__(model, "_tn_tet_stats_pending", None)
        rd, pending = held
        with torch.no_grad():
            rgb = outputs["rgb"]
            image = batch["image"].to(rgb.device)
            ray_value = ((rgb - image) ** 2).sum(-1).detach().reshape(-1)
            rd.accumulate_tet_stats(model_tet_stats(model), pending, ray_value)
    mult = getattr(model.config, "distortion_loss_mult", None)
    if mult is not None and "distortion" in outputs:
        loss_dict["distortion_loss"] = float(mult) * outputs["distortion"].mean()
    return loss_dict


def model_tet_stats(model, reset=False, num_cells=None):
    """The model's per-tetrahedron training statistics `model._tn_tet_stats`, i64 [T, 3] (cpp.tet_stats_new), created lazily and
    sized to the tracer's current cells (or num_cells); an array of another size (the mesh changed under it) or reset=True
    gives fresh zeros.  A plain attribute: no state-dict key."""
    from . import tetranerf_cpp_extension as cpp

    tracer = model.get_tetrahedra_tracer()
    T = tracer.tetrahedra_cells.numel() // 4 if num_cells is None else int(num_cells)
    stats = getattr(model, "_tn_tet_stats", None)
    if reset or stats is None or stats.size(0) != T or stats.device != tracer.tetrahedra_cells.device:
        stats = cpp.tet_stats_new(T, tracer.tetrahedra_cells.device)
        object.__setattr__(model, "_tn_tet_stats", stats)
    return stats


def densify_selection(stats, mask=None, score="error", min_hits=None, max_new=None):
    """The statistics' part of densify's selection, in plain torch (any device): bool [T].
        eligible = (hits >= min_hits) & mask            (min_hits None: 1 -- a tetrahedron no sample fell into has no evidence)
        max_new: of the eligible, the max_new with the highest render.tet_stats_scores(stats, score); equal scores go to the
        LOWER id (a stable descending sort keeps ids ascending among equals)."""
    from . import render

    hits = stats[:, 0]
    eligible = hits >= int(1 if min_hits is None else min_hits)
    if mask is not None:
        eligible = eligible & mask.to(eligible.device)
    if max_new is None or int(max_new) >= eligible.numel():
        return eligible
    scores = render.tet_stats_scores(stats, score)
    scores = torch.where(eligible, scores, scores.new_full((), -1.0))       # (scores are >= 0)
    keep = torch.sort(scores, descending=True, stable=True).indices[:max(0, int(max_new))]
    cut = torch.zeros_like(eligible)
    cut[keep] = True
    return eligible & cut


def install(model_cls=None):
    """Monkey-patch `model_cls.get_outputs` (default: the reference's TetrahedraNerf, imported here -- needs nerfstudio)
    with `fused_get_outputs`; the original stays reachable as `_tn_reference_get_outputs` (fallback rule).  `get_loss_dict`, where
    the class has one, is wrapped by `fused_get_loss_dict` the same way (`_tn_reference_get_loss_dict`).  Idempotent.
    Returns the class."""
    if model_cls is None:
        from tetranerf.nerfstudio.model import TetrahedraNerf as model_cls   # noqa: N813  (reference package)
    if getattr(model_cls, "_tn_reference_get_outputs", None) is None:
        model_cls._tn_reference_get_outputs = model_cls.get_outputs
        model_cls.get_outputs = fused_get_outputs
    if getattr(model_cls, "_tn_reference_get_loss_dict", None) is None and getattr(model_cls, "get_loss_dict", None) is not None:
        model_cls._tn_reference_get_loss_dict = model_cls.get_loss_dict
        model_cls.get_loss_dict = fused_get_loss_dict
    return model_cls


def uninstall(model_cls):
    ref = getattr(model_cls, "_tn_reference_get_outputs", None)
    if ref is not None:
        model_cls.get_outputs = ref
        model_cls._tn_reference_get_outputs = None
    ref = getattr(model_cls, "_tn_reference_get_loss_dict", None)
    if ref is not None:
        model_cls.get_loss_dict = ref
        model_cls._tn_reference_get_loss_dict = None
    return model_cls


def make_fused_model_class(base_cls):
    """Subclass of the reference model whose get_outputs runs the fused kernels (no monkey-patching): use it as
    `TetrahedraNerfConfig._target`."""

    class FusedTetrahedraNerf(base_cls):   # type: ignore[misc, valid-type]
        _tn_reference_get_outputs = base_cls.get_outputs

        def get_outputs(self, ray_bundle):
            return fused_get_outputs(self, ray_bundle)

        if getattr(base_cls, "get_loss_dict", None) is not None:
            _tn_reference_get_loss_dict = base_cls.get_loss_dict

            def get_loss_dict(self, outputs, batch, metrics_dict=None):
                return fused_get_loss_dict(self, outputs, batch, metrics_dict)

    FusedTetrahedraNerf.__name__ = "Fused" + base_cls.__name__
    return FusedTetrahedraNerf


def use_fused_radam(trainer_config) -> List[str]:
    """Opt in to the HIP optimiser step: every entry of `trainer_config.optimizers` (name -> {"optimizer": config, ...},
    registration.py:37-45: the one group "fields", RAdamOptimizerConfig) whose optimiser config's `_target` is torch.optim.RAdam
    gets `_target = optim.FusedRAdam` -- nerfstudio's `setup` calls `_target(params, lr=, eps=, weight_decay=)`, which FusedRAdam
    takes with torch's names and defaults.  Duck-typed: no nerfstudio import.  Returns the names it changed; nothing is installed
    unless this is called."""
    from .optim import FusedRAdam

    changed = []
    for name, entry in (getattr(trainer_config, "optimizers", None) or {}).items():
        cfg = entry.get("optimizer") if isinstance(entry, dict) else getattr(entry, "optimizer", None)
        if cfg is not None and getattr(cfg, "_target", None) is torch.optim.RAdam:
            try:
                cfg._target = FusedRAdam
            except AttributeError:           # (a frozen dataclass)
                object.__setattr__(cfg, "_target", FusedRAdam)
            changed.append(name)
    return changed


def load_reference_checkpoint(model, state_dict, prefix: str = ""):
    """Copy a reference checkpoint's parameters into a model through `copy_` (bumps the version counters the weight /
    field caches watch) after checking the architecture; returns the model."""
    ws, field = weights_from_state_dict(state_dict, prefix)
    with torch.no_grad():
        for dst, src in zip(weights_from_model(model), ws):
            dst.copy_(src)
        model.tetrahedra_field.copy_(field)
    return model


def extract_mesh(model, level, path=None, refine_rounds=0):
    """The density isosurface of a TetrahedraNerf as a coloured triangle mesh (render.extract_mesh on the model's own buffers:
    `tetrahedra_vertices`, `tetrahedra_cells`, `tetrahedra_field` and its modules' weights).  Where the
    model has the `tetrahedra_occupancy` buffer AND `config.occupancy_threshold`, the tetrahedra an evaluation render culls are
    masked out of the surface.  level: the density of the surface.  path: also written there as a binary PLY
    (tetrahedra_io.save_mesh_ply, colours as uint8).  The colours are the head's answer to a viewer looking at the surface along
    minus its normal, without the appearance-embedding term.  refine_rounds (0..8; 0: the linear placement, unchanged): the
    vertices move along their mesh edges onto the network's own level set first (render.extract_mesh).  Blocking (two small read-backs; the file).  Returns
    render.extract_mesh's dict."""
    from . import render, tetrahedra_io

    ok, why = fused_config_supported(model.config)
    if not ok:
        raise RuntimeError(f"extract_mesh needs the architecture of the fused kernels ({why})")
    occupancy = getattr(model, "tetrahedra_occupancy", None)
    threshold = getattr(model.config, "occupancy_threshold", None)
    if occupancy is None or threshold is None:
        occupancy = threshold = None
    field = model.tetrahedra_field
    mesh = render.extract_mesh(model.tetrahedra_vertices.detach().to(field.device), model.tetrahedra_cells.to(field.device).reshape(-1, 4),
                               field, ModelMLP(model), level, occupancy=None if occupancy is None else occupancy.detach(),
                               occupancy_threshold=threshold, **({"refine_rounds": refine_rounds} if refine_rounds else {}))
    if path is not None:
        tetrahedra_io.save_mesh_ply(path, mesh["positions"], mesh["triangles"],
                                    (mesh["colors"].clamp(0, 1) * 255.0).round().to(torch.uint8))
    return mesh


def _set_tensor(model, name, value, like=None):
    """`model.<name> = value` under the kind the attribute has: a Parameter stays one (requires_grad as before), a buffer a buffer"""
    if isinstance(like, torch.nn.Parameter):
        value = torch.nn.Parameter(value, requires_grad=like.requires_grad)
    setattr(model, name, value)
    return value


def _grow_moments(optimizer, old, vertex_parents, new_moments, vertex_major):
    """(exp_avg, exp_avg_sq) of `old` carried to the split mesh, or (None, None) where the optimiser holds none for it.
    vertex_major: the moments are [V, ...] (the vertex table's) and are carried in plain torch; else [rows, V] (the field's)."""
    from . import tetranerf_cpp_extension as cpp

    state = optimizer.state.get(old) if optimizer is not None else None
    if not state or "exp_avg" not in state:
        return None, None
    out = []
    for key in ("exp_avg", "exp_avg_sq"):
        m = state[key]
        if not vertex_major:
            out.append(cpp.split_vertex_rows(m, vertex_parents, new=new_moments))
            continue
        fresh = m.new_zeros((vertex_parents.size(0),) + tuple(m.shape[1:]))
        if new_moments == "mean":
            a, b, c, d = m[vertex_parents.long()].unbind(1)
            fresh = ((a + b) + (c + d)) * 0.25
        out.append(torch.cat([m, fresh], 0))
    return tuple(out)


def densify(model, select=None, *, stats=None, score="error", min_hits=None, occupancy_threshold=None, min_width=None, max_new=None,
            optimizer=None, new_moments="mean", retriangulate=False, method="centroid"):
    """Raise the resolution of a TetrahedraNerf's mesh where asked: the selected tetrahedra are split 1 -> 4 at their centroids
    (`tracer.split_tetrahedra`), the new vertices take the mean of their four parents' field columns, so
    the piecewise-linear field -- and with it the next frame and the next loss -- is the one of the unsplit mesh up to rounding.
    An explicit call, like extract_mesh, not a config switch: get_outputs cannot reach the trainer's optimisers.

    select: bool / uint8 [T] over the model's cells, or None: then the mask is occupancy >= occupancy_threshold (needs the
    `tetrahedra_occupancy` buffer) and width >= min_width (`tracer.tet_quality()`), whichever are given.  max_new: the mask is cut
    to the max_new widest tetrahedra (torch.topk).  The policy is the caller's; tetrahedra the rule refuses (flat, or so thin that
    the fp32 centroid lands on a face) stay as they are.
    stats: per-tetrahedron training statistics i64 [T, 3] (cpp.tet_stats_accumulate), or True: the model's own, gathered under
    `config.densify_stats`.  With select=None the mask is hits >= min_hits (None: 1) and the occupancy and width conditions
    where given; max_new then cuts to the highest SCORES -- render.tet_stats_scores(stats, score), score one of "error",
    "mean_error", "weight", "hits" -- with ties going to the lower id (a stable sort; densify_selection).  With `select` given
    the mask is the caller's and only the max_new cut uses the scores.  Selection is plain torch: it runs once per hundreds of
    iterations.  After a split or a re-triangulation the model's statistics (where it has any) are replaced by zeros of the new
    size -- children start from zero -- and the result has "stats_reset": True.
    optimizer: the optimiser that holds `tetrahedra_field` (and `tetrahedra_vertices`, where that is optimised): its state moves
    through optim.grow_parameter -- step kept, the moments of a new vertex the mean of its parents' (new_moments="mean") or 0
    ("zero").  Without it the caller re-creates its optimiser.
    retriangulate: afterwards `tracer.retriangulate` gives the grown vertex table Delaunay cells; the field is per vertex and
    survives, the occupancy goes through remap_tet_values.  This trades the exact preservation for a Delaunay mesh.

    The model adopts the split mesh, and after a re-triangulation that one (`_adopt_mesh`: `tetrahedra_vertices`,
    `tetrahedra_cells`, `tetrahedra_occupancy` where present and the config sizes replaced, what `_follow_vertices` remembers
    of the vertex table taken again, the statistics zeroed).  `tetrahedra_field` is REPLACED under its name as well (a new
    nn.Parameter: the old one leaves the field cache, the new one is registered iff the old was, with its vertex-major shadow
    already installed).  BLOCKS on the read-back of the number of accepted tetrahedra and on the load.  With nothing accepted
    nothing is touched.
    method: "centroid" (the default: the 1 -> 4 split above) or "edge": the best -- longest -- edge of every selected tetrahedron
    is bisected at its midpoint together with EVERY tetrahedron around it (`tracer.split_edges`), which
    halves the edge and the volumes where a centroid split never shortens an edge.  The new vertex takes the mean of the edge's
    two ends, in the centroid's own expression, so everything above holds as it stands.  One call bisects an independent set of
    edges: edges on the hull, edges that lose a tetrahedron to a longer selected edge and edges with a flat tetrahedron around
    them are refused, and what was left unsplit is split by calling again with the caller's own selection carried as
    cat(select & ~result["bisected"], zeros(num_cells - T)).
    Returns {"counters": int32 [4] on the device (asked, accepted, refused flat or inverted, refused for an id), "num_new",
    "num_vertices", "num_cells", "retriangulated"}; with method="edge" the counters are the ten of split_edges
    (geometry.EDGE_SPLIT_COUNTER_NAMES), "num_new" the new vertices K_v, "num_cells" T + K_t, and "bisected" uint8 [T] marks the
    rows that were bisected."""
    from . import optim as tn_optim
    from . import tetranerf_cpp_extension as cpp

    if new_moments not in ("mean", "zero"):
        raise ValueError('densify: new_moments must be "mean" or "zero"')
    if method not in ("centroid", "edge"):
        raise ValueError('densify: method must be "centroid" or "edge"')
    tracer = model.get_tetrahedra_tracer()
    if method == "edge" and not getattr(tracer, "supports_edge_split", False):
        raise RuntimeError("densify(method=\"edge\") needs a tracer with split_edges (tetranerf_cpp_extension.TetrahedraTracer)")
    if not getattr(tracer, "supports_split", False):
        raise RuntimeError("densify needs a tracer with split_tetrahedra (tetranerf_cpp_extension.TetrahedraTracer)")
    field, vertices = model.tetrahedra_field, model.tetrahedra_vertices
    occupancy = getattr(model, "tetrahedra_occupancy", None)
    T = tracer.tetrahedra_cells.numel() // 4
    if stats is True:
        stats = getattr(model, "_tn_tet_stats", None)
        if stats is None:
            raise ValueError("densify: stats=True needs the model's own statistics (config.densify_stats and at least one training step)")
    if stats is not None and (stats.dim() != 2 or tuple(stats.shape) != (T, 3) or stats.dtype != torch.int64):
        raise ValueError("densify: stats must be i64 [T, 3] over the model's current cells")
    if stats is None and min_hits is not None:
        raise ValueError("densify: min_hits needs stats")
    has_stats = stats is not None or getattr(model, "_tn_tet_stats", None) is not None
    with torch.no_grad():
        width = tracer.tet_quality()["width"] if (select is None and min_width is not None) or (max_new is not None and stats is None) else None
        if select is None:
            if occupancy_threshold is None and min_width is None and stats is None:
                raise ValueError("densify: give `select`, stats, or occupancy_threshold and / or min_width")
            mask = torch.ones(T, dtype=torch.bool, device=tracer.device)
            if occupancy_threshold is not None:
                if occupancy is None:
                    raise ValueError("densify: occupancy_threshold needs the model's tetrahedra_occupancy buffer")
                mask &= occupancy.detach() >= float(occupancy_threshold)
            if min_width is not None:
                mask &= width >= float(min_width)
        else:
            mask = select.to(tracer.device).reshape(-1) != 0
            if mask.numel() != T:
                raise ValueError("densify: select must have one entry per tetrahedron")
        if stats is not None:
            mask = densify_selection(stats.to(tracer.device), mask, score, min_hits if select is None else 0, max_new)
        elif max_new is not None and T:
            keep = torch.topk(torch.where(mask, width, width.new_full((), -1.0)), min(int(max_new), T)).indices
            cut = torch.zeros_like(mask)
            cut[keep] = True
            mask &= cut
        registered = cpp.field_is_registered(field)
        field_vm = cpp.field_vertex_major(field) if registered else None        # (before the load below forgets it)
        split = tracer.split_edges if method == "edge" else tracer.split_tetrahedra
        out = split(mask.contiguous(), tet_values=() if occupancy is None else (occupancy.detach(),))
        K = int(out["num_new"])
        result = {"counters": out["counters"], "num_new": K, "num_vertices": vertices.shape[0] + K,
                  "num_cells": T + (int(out["num_rows"]) if method == "edge" else 3 * K), "retriangulated": False}
        if method == "edge":
            result["bisected"] = out["bisected"]
        if has_stats:
            result["stats_reset"] = False
        if K == 0:
            return result
        parents = out["vertex_parents"]
        field_moments = _grow_moments(optimizer, field, parents, new_moments, False)
        vertex_moments = _grow_moments(optimizer, vertices, parents, new_moments, True)
        new_vertices = _adopt_mesh(model, tracer, out["cells"], vertices=out["vertices"],
                                   occupancy=None if occupancy is None else out["tet_values"][0])
        # the split's own: the field's new columns, its registration and shadow, the optimiser state of both tensors
        new_field, new_vm = cpp.split_vertex_rows(field.detach(), parents, "mean", values_vm=field_vm, want_vertex_major=True)
        new_field = _set_tensor(model, "tetrahedra_field", new_field, field)
        cpp.unregister_field(field)
        if registered:
            cpp.register_field(new_field)
            cpp.install_field_shadow(new_field, new_vm)
        if optimizer is not None:
            if field_moments[0] is not None or any(p is field for g in optimizer.param_groups for p in g["params"]):
                tn_optim.grow_parameter(optimizer, field, new_field, *field_moments)
            if any(p is vertices for g in optimizer.param_groups for p in g["params"]):
                tn_optim.grow_parameter(optimizer, vertices, new_vertices, *vertex_moments)
        if retriangulate:
            occ = getattr(model, "tetrahedra_occupancy", None)
            again = tracer.retriangulate(new_vertices, () if occ is None else (occ.detach(),))    # (the load borrows the Parameter)
            _adopt_mesh(model, tracer, again["cells"], occupancy=None if occ is None else again["tet_values"][0])
            result.update(num_cells=int(again["num_tetrahedra"]), retriangulated=True)
        if has_stats:
            result["stats_reset"] = getattr(model, "_tn_tet_stats", None) is not None
        return result


def _prune_moments(optimizer, old, kept_ids, vertex_major):
    """(exp_avg, exp_avg_sq) of `old` compacted to the kept vertices, or (None, None) where the optimiser holds none for it.
    vertex_major: the moments are [V, ...] (the vertex table's) and are carried in plain torch; else [rows, V] (the field's)."""
    from . import tetranerf_cpp_extension as cpp

    state = optimizer.state.get(old) if optimizer is not None else None
    if not state or "exp_avg" not in state:
        return None, None
    if vertex_major:
        return tuple(state[k][kept_ids.long()].contiguous() for k in ("exp_avg", "exp_avg_sq"))
    return tuple(cpp.prune_vertex_rows(state[k], kept_ids) for k in ("exp_avg", "exp_avg_sq"))


def prune(model, dead=None, *, stats=None, max_hits=0, occupancy_below=None, vertex_select=None, max_removed=None, optimizer=None):
    """Lower the resolution of a TetrahedraNerf's mesh where nothing is left: the vertices that only dead tetrahedra name, and that
    lie on no hull face, are removed and the rest get their Delaunay cells (`tracer.remove_vertices`).
    The field, its optimiser's moments and the vertex table are compacted; the occupancy goes through remap_tet_values.  An
    explicit call, like densify, not a config switch.

    dead: bool / uint8 [T] over the model's cells, or None: then the AND of the conditions given -- hits <= max_hits from
    `stats` (i64 [T, 3], cpp.tet_stats_accumulate, or True: the model's own) and occupancy < occupancy_below (needs the
    `tetrahedra_occupancy` buffer); ValueError if none is.  vertex_select: bool / uint8 [V], only these vertices are asked.
    max_removed: of the removable vertices, the max_removed with the LOWEST ids are removed (a second count with a cut
    vertex_select).  optimizer: the optimiser that holds `tetrahedra_field` (and `tetrahedra_vertices`, where that is
    optimised): its state moves through optim.grow_parameter -- step kept, the moments of every kept vertex kept bit for bit.
    Without it the caller re-creates its optimiser.

    The model adopts the pruned mesh (`_adopt_mesh`: `tetrahedra_vertices`, `tetrahedra_cells`, `tetrahedra_occupancy` where
    present and the config sizes replaced, what `_follow_vertices` remembers of the vertex table taken again, the statistics
    zeroed).  `tetrahedra_field` is REPLACED under its name (a new nn.Parameter: the old one leaves the field cache, the new one is
    registered iff the old was, with its vertex-major shadow already installed).  BLOCKS on the read-back of V' (twice with
    max_removed), the triangulation and the load.  With nothing removed nothing is touched.
    Returns {"counters": int32 [5] on the device (asked, removed, kept live, kept hull, kept unreferenced), "num_removed",
    "num_vertices", "num_cells"} and "stats_reset" where the model has statistics."""
    from . import optim as tn_optim
    from . import tetranerf_cpp_extension as cpp

    tracer = model.get_tetrahedra_tracer()
    if not getattr(tracer, "supports_prune", False):
        raise RuntimeError("prune needs a tracer with remove_vertices (tetranerf_cpp_extension.TetrahedraTracer)")
    field, vertices = model.tetrahedra_field, model.tetrahedra_vertices
    occupancy = getattr(model, "tetrahedra_occupancy", None)
    T, V, dev = tracer.tetrahedra_cells.numel() // 4, vertices.shape[0], tracer.device
    if stats is True:
        stats = getattr(model, "_tn_tet_stats", None)
        if stats is None:
            raise ValueError("prune: stats=True needs the model's own statistics (config.densify_stats and at least one training step)")
    if stats is not None and (stats.dim() != 2 or tuple(stats.shape) != (T, 3) or stats.dtype != torch.int64):
        raise ValueError("prune: stats must be i64 [T, 3] over the model's current cells")
    has_stats = stats is not None or getattr(model, "_tn_tet_stats", None) is not None
    with torch.no_grad():
        if dead is None:
            if stats is None and occupancy_below is None:
                raise ValueError("prune: give `dead`, stats, or occupancy_below")
            mask = torch.ones(T, dtype=torch.bool, device=dev)
            if stats is not None:
                mask &= stats[:, 0].to(dev) <= int(max_hits)
            if occupancy_below is not None:
                if occupancy is None:
                    raise ValueError("prune: occupancy_below needs the model's tetrahedra_occupancy buffer")
                mask &= occupancy.detach() < float(occupancy_below)
        else:
            mask = dead.to(dev).reshape(-1) != 0
            if mask.numel() != T:
                raise ValueError("prune: dead must have one entry per tetrahedron")
        mask = mask.contiguous()
        select = None
        if vertex_select is not None:
            select = (vertex_select.to(dev).reshape(-1) != 0).contiguous()
            if select.numel() != V:
                raise ValueError("prune: vertex_select must have one entry per vertex")
        if max_removed is not None:
            offsets, _ = tracer.prune_count(mask, select)
            removable = torch.nonzero(offsets[1:] == offsets[:-1]).reshape(-1)[:max(0, int(max_removed))]
            cut = torch.zeros(V, dtype=torch.bool, device=dev)
            cut[removable] = True
            select = cut
        registered = cpp.field_is_registered(field)
        field_vm = cpp.field_vertex_major(field) if registered else None        # (before the load below forgets it)
        out = tracer.remove_vertices(mask, select, tet_values=() if occupancy is None else (occupancy.detach(),))
        R = int(out["num_removed"])
        result = {"counters": out["counters"], "num_removed": R, "num_vertices": V - R, "num_cells": int(out["num_tetrahedra"])}
        if has_stats:
            result["stats_reset"] = False
        if R == 0:
            return result
        kept = out["kept_ids"]
        field_moments = _prune_moments(optimizer, field, kept, False)
        vertex_moments = _prune_moments(optimizer, vertices, kept, True)
        new_vertices = _adopt_mesh(model, tracer, out["cells"], vertices=out["vertices"],
                                   occupancy=None if occupancy is None else out["tet_values"][0])
        new_field, new_vm = cpp.prune_vertex_rows(field.detach(), kept, values_vm=field_vm, want_vertex_major=True)
        new_field = _set_tensor(model, "tetrahedra_field", new_field, field)
        cpp.unregister_field(field)
        if registered:
            cpp.register_field(new_field)
            cpp.install_field_shadow(new_field, new_vm)
        if optimizer is not None:
            if field_moments[0] is not None or any(p is field for g in optimizer.param_groups for p in g["params"]):
                tn_optim.grow_parameter(optimizer, field, new_field, *field_moments)
            if any(p is vertices for g in optimizer.param_groups for p in g["params"]):
                tn_optim.grow_parameter(optimizer, vertices, new_vertices, *vertex_moments)
        if has_stats:
            result["stats_reset"] = getattr(model, "_tn_tet_stats", None) is not None
        return result
