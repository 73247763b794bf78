"""NeRFRenderer: the prepared-field caches, the switches, run() / render() and the step renders of the stylisation step (models/instant_nsr.py:90-408)."""
import torch
import torch.nn as nn

from .. import nsr_ops
from .route import _keeps_stencil, render_route
from .guard import FiniteGuard

DEFAULT_GEO_THRESH = 0.05     # utils/constant.py:17


def near_far_from_bound(rays_o, rays_d, bound, type='cube'):
    """models/instant_nsr.py:58-77 (host-side helper kept for API parity; the fused kernel has its own copy)."""
    radius = rays_o.norm(dim=-1, keepdim=True)
    if type == 'sphere':
        return radius - bound, radius + bound
    tmin = (-bound - rays_o) / (rays_d + 1e-15)
    tmax = (bound - rays_o) / (rays_d + 1e-15)
    near = torch.where(tmin < tmax, tmin, tmax).max(dim=-1, keepdim=True)[0]
    far = torch.where(tmin > tmax, tmin, tmax).min(dim=-1, keepdim=True)[0]
    return torch.clamp(near, min=0.05), far


class SingleVarianceNetwork(nn.Module):
    def __init__(self, init_val):
        super().__init__()
        self.register_parameter('variance', nn.Parameter(torch.tensor(init_val)))

    def forward(self, x):
        return torch.ones([len(x), 1], device=self.variance.device) * torch.exp(self.variance * 10.0)


def _background(bg, n, device, ones=False):
    """a background colour as [n,3]: tensor [n,3] / [3] / scalar, broadcast without a copy; None stays None (the renderer's white), or with `ones` becomes
    the white it stands for (the training renders, whose backward reads it)"""
    if bg is None:
        return torch.ones((n, 3), dtype=torch.float32, device=device) if ones else None
    bg = torch.as_tensor(bg, dtype=torch.float32, device=device)
    bg = bg.reshape(-1, 3) if bg.numel() >= 3 else bg.reshape(1, 1).expand(1, 3)
    return bg.expand(n, 3) if bg.shape[0] == 1 else bg


def _draw_noise(dst):
    """jitter noise drawn straight into dst, a slice of a launch's noise buffer (torch.rand(out=...): no concatenation kernel)"""
    r = torch.rand(tuple(dst.shape), device=dst.device, out=dst)
    if r.data_ptr() != dst.data_ptr():                       # (a replaced torch.rand that ignores `out`: tests replaying recorded draws)
        dst.copy_(r)


def _flat_rays(rays_o, rays_d):
    """the rays as every launch takes them: [n,3] float32, contiguous"""
    return rays_o.reshape(-1, 3).float().contiguous(), rays_d.reshape(-1, 3).float().contiguous()


def _neus_alpha(sdf, inv_s, true_cos, deltas, cos_anneal_ratio):
    """the cos-annealed NeuS alpha in torch (:225-243), per sample: sdf, true_cos [M,1], deltas [M] (the section lengths) -> [M,1] in [0, 1]"""
    act = nn.Softplus(beta=100)
    iter_cos = -(act(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + act(-true_cos) * cos_anneal_ratio)
    half = iter_cos * deltas.reshape(-1, 1) * 0.5
    prev_cdf = torch.sigmoid((sdf - half) * inv_s)
    next_cdf = torch.sigmoid((sdf + half) * inv_s)
    return ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).clip(0.0, 1.0)


def _relaxed_ratio(relax, err):
    """a per-sample error averaged over the samples `relax` selects (the eikonal term :266-272, the curvature term :288)"""
    return (relax * err).sum() / (relax.sum() + 1e-5)


class NeRFRenderer(FiniteGuard, nn.Module):
    def __init__(self, cuda_ray=False, curvature_loss=False):
        super().__init__()
        self.cuda_ray = cuda_ray
        self.curvature_loss = curvature_loss
        if cuda_ray:   # extra state of the occupancy-grid marcher (instant_nsr.py:100-110)
            self.register_buffer('density_grid', torch.zeros([128 + 1] * 3))
            self.mean_density = 0
            self.iter_density = 0
            self.register_buffer('step_counter', torch.zeros(64, 2, dtype=torch.int32))
            self.mean_count = 0
            self.local_step = 0

    # ------------------------------------------------------------------ fused field handle
    # The prepared ac_field views (ctypes structs holding raw device pointers) and the outputs of the last training render are caches, not state:
    # they are left out of pickling / copy.deepcopy / torch.save(net) and rebuilt on the next render.  So are the variance keyed on the parameter's version
    # (forward_variance), the patch groups of the last whole-view training render, and the seed faces render_utils.render_instantnsr_naive keeps here from
    # one posed frame to the next (25 MB for a 256 x 256 view).  THE list: nothing else names what is cache.
    _CACHE_ATTRS = ("_pair_bg_cache", "_field_cache", "_field_sdf_cache", "_last_train", "_last_train_groups", "_offsets_cache", "_axis_cache",
                    "_inv_s_cache", "_warp_seed_rows")
    # not picklable (events, pinned words) but NOT a cache either: pending NaN flags survive invalidate_caches() and are resolved by check_finite()
    _UNPICKLED_ATTRS = _CACHE_ATTRS + ("_nan_pending",)

    def __getstate__(self):
        self.check_finite()             # a NaN recorded by an earlier training render must not vanish into a checkpoint / copy
        state = self.__dict__.copy()
        for k in self._UNPICKLED_ATTRS:
            state.pop(k, None)
        return state

    def __deepcopy__(self, memo):
        # (through pickling: the caches are dropped by __getstate__, and torch's own deepcopy refuses the non-leaf `weight` attribute that the
        # old-style weight_norm hook leaves on every layer -- the reference's networks cannot be deep-copied at all).
        # LIMITATION: only the module itself is registered in `memo`, not its parameters / buffers: deep-copying a CONTAINER that holds this net
        # and an optimizer over its parameters yields an optimizer that still points at the ORIGINAL parameters.  Copy the net, then build the
        # optimizer on the copy (what stylize.py / reconstruct.py do with their checkpoints: state_dicts, never live objects).
        import io
        buf = io.BytesIO()
        torch.save(self, buf)
        buf.seek(0)
        new = torch.load(buf, weights_only=False)
        memo[id(self)] = new
        return new

    def invalidate_caches(self):
        """Drop the prepared field views.  The caches are keyed by (data_ptr, tensor version) of every parameter and by the stream they were built
        on, so ordinary training / load_state_dict invalidate them by themselves; call this after writing parameters behind autograd's back
        (`param.data.copy_`, raw-pointer kernels, another stream) -- those do not bump the version counter."""
        for k in self._CACHE_ATTRS:
            self.__dict__.pop(k, None)
        from .. import ray_utils
        ray_utils.invalidate_caches()

    def _cache_key(self, prm):
        from .. import _lib as L
        return (int(L.current_stream(prm[0].device) or 0),) + tuple((t.data_ptr(), t._version) for t in prm)

    def _field(self):
        """ac_field view of the current parameters (effective = weight-normed matrices).  Cached while no parameter changes
        (tensor version counters): a frozen net (net_gt of stylize.py) builds it once, a training net once per optimizer step --
        not once per ray batch (7 weight-norm launches and a struct each time otherwise)."""
        enc = self.encoder
        prm = [enc.embeddings, self.sdf_net[0].bias, self.sdf_net[1].bias] + [t for l in list(self.sdf_net) + list(self.color_net)
                                                                             for t in (l.weight_v, l.weight_g)]
        key = self._cache_key(prm)
        cached = getattr(self, "_field_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        with torch.no_grad():
            W = self._effective_weights()
            Wc1, Wc1_sh = nsr_ops.split_viewdir_weight(W[2])          # use_viewdirs: [64,37] -> [x | n | feat] (21) + the 16 view-direction columns
            f = nsr_ops.Field(enc.embeddings.detach(), self._offsets_host(), enc.per_level_scale, enc.base_resolution,
                              W[0], self.sdf_net[0].bias.detach().contiguous(), W[1], self.sdf_net[1].bias.detach().contiguous(), Wc1, W[3], W[4],
                              Wc1_sh=Wc1_sh)
        f.prepare()                     # the weights in LDS order, once per parameter version (every render workgroup then copies them linearly)
        self._field_cache = (key, f)
        return f

    def _effective_weights(self):
        """weight-normed matrices of the five layers (torch.nn.utils.weight_norm: w = v g / ||v||_row), all in ONE launch"""
        layers = list(self.sdf_net) + list(self.color_net)
        dev = layers[0].weight_v.device
        shapes = [tuple(l.weight_v.shape) for l in layers]
        buf = torch.empty(sum(r * c for r, c in shapes), dtype=torch.float32, device=dev)
        outs, off = [], 0
        for r, c in shapes:
            outs.append(buf[off:off + r * c].view(r, c)); off += r * c
        return nsr_ops.weight_norm_forward([(l.weight_v.detach(), l.weight_g.detach()) for l in layers], outs)

    # ---- a training render WITHOUT autograd (stylize.sds_step): run() keeps the launch's per-sample outputs, backward_last() turns upstream
    # gradients of (image, weights_sum, gradient_error) into parameter gradients: ac_render_core_backward + ac_param_grads, accumulated into .grad
    _manual_backward = False

    def manual_backward_supported(self, num_steps=None, upsample_steps=None):
        # (not for cuda_ray nets: their render() is run_cuda's occupancy march -- the fixed-step pair / whole-view launches and backward_last() would render
        #  different samples than render_instantnsr_naive does for the same net; ADVICE round 5.  They train through run_cuda under autograd.)
        # With the counts: False also where the fused backward does not reach -- a field with view directions at a count that 16 does not divide (the
        # colour backward takes a tile of 16 samples as one ray's); such a step trains through autograd.
        ok = self.fused_training == "core" and self._fused_supported() and self.encoder.embeddings.is_cuda and not getattr(self, "cuda_ray", False)
        if ok and num_steps is not None and upsample_steps is not None and self.use_viewdirs:
            ok = (int(num_steps) + int(upsample_steps)) % 16 == 0
        return ok

    def _long_save_stencil(self, num_steps, upsample_steps):
        """_keeps_stencil with this model's long_step_extras"""
        return _keeps_stencil(self.long_step_extras, num_steps, upsample_steps)

    def _route(self, caller, num_steps, upsample_steps, full=None, posed=False, needs_grad=False, near_far=False, per_sample=True, opacity_only=False):
        """render_route() with this model's switches; full = None (the step renders): the default model on the GPU, for a training step not a cuda_ray net"""
        if full is None:
            full = self._fused_supported() and self.encoder.embeddings.is_cuda and not (caller != "view_nograd" and getattr(self, "cuda_ray", False))
        return render_route(caller, num_steps, upsample_steps, posed=posed, needs_grad=needs_grad, full=full, training=self.training, near_far=near_far,
                            per_sample=per_sample, opacity_only=opacity_only, fused_training=self.fused_training,
                            manual_backward=self._manual_backward, render_table_dtype=self.render_table_dtype,
                            skip_masked_samples=self.skip_masked_samples, posed_long_rays=self.posed_long_rays,
                            long_step_extras=self.long_step_extras, use_viewdirs=self.use_viewdirs)

    def render_step_pair(self, rays_o, rays_d, num_steps, upsample_steps, bound, bkg_fn, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0):
        """The two renders of net_style in one stylisation step (stylize.py:98-116 render_val, :143-152 the differentiable render of the same rays) as
        ONE launch (ac_render_rays_pair): the two copies of a ray share most table sectors and meet in L2.  Random draws, in the order the two renders
        make them: bkg_fn() -> background of render_val, jitter noise of render_val, bkg_fn() -> background of the training render, its jitter noise --
        i.e. the training render's draws come BEFORE whatever the guidance draws in between in the reference (stylize.py:128-152), which is why
        stylize.sds_step pairs the renders only for a guidance with `private_rng = True`.
        Returns (rgb_val [N,3], rgb [N,3], gradient_error, weight_sum [N,1]) of which the last three belong to the training render, whose
        per-sample outputs are kept for backward_last().  Every value equals what the two separate renders give, bit for bit."""
        route = self._route("step_pair", num_steps, upsample_steps)
        ro, rd = _flat_rays(rays_o, rays_d)
        N, device = ro.shape[0], ro.device
        # the two noise draws land in the two halves of one buffer (torch.rand(out=...): the same two calls, no concatenation kernel)
        noise2 = torch.empty((2 * N, num_steps), dtype=torch.float32, device=device)
        bg_a = _background(bkg_fn(), N, device, ones=True); _draw_noise(noise2[:N])
        bg_b = _background(bkg_fn(), N, device, ones=True); _draw_noise(noise2[N:])
        ck = (bg_a.data_ptr(), bg_b.data_ptr(), N)
        if bg_a is bg_b or (bg_a.data_ptr() == bg_b.data_ptr()):   # a constant background (cached on the device): its doubled copy is cached as well
            cache = self.__dict__.setdefault("_pair_bg_cache", {})
            if ck not in cache:
                cache.clear(); cache[ck] = (torch.cat([bg_a, bg_b]).contiguous(), bg_a)      # (bg_a kept alive: the key is its address)
            bg2 = cache[ck][0]
        else:
            bg2 = torch.cat([bg_a, bg_b]).contiguous()
        render = getattr(nsr_ops, route.entry)
        kw = dict(cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio, precision=self.render_precision)
        with torch.no_grad():
            field, inv_s = self._field(), self.forward_variance()
            if route.entry.endswith("_pair"):
                ra, rb = render(field, ro, rd, noise2, num_steps, upsample_steps, bound, inv_s, bg2=bg2, **kw, **route.options)
            else:           # two launches, the same draws: the route's options are the training copy's
                ra = render(field, ro, rd, num_steps, upsample_steps, bound, inv_s, bg=bg2[:N], noise=noise2[:N], **kw)
                rb = render(field, ro, rd, num_steps, upsample_steps, bound, inv_s, bg=bg2[N:], noise=noise2[N:], **route.options, **kw)
        self._last_train = (rb, ro, rd, bg2[N:], field)
        self._guard_finite(rb["eik_res"][0])
        return ra["image"], rb["image"], rb["eik_res"][0], rb["weights_sum"][:, None]

    def _render_view(self, caller, rays_o, rays_d, num_steps, upsample_steps, bound, draw, batch_size, cos_anneal_ratio, normal_epsilon_ratio, **how):
        """a whole view in ONE launch, its random draws exactly as the batch-by-batch loop makes them: per batch k of n rays draw(k, n) -> its background,
        then (a training render, or train mode) its jitter noise, into slices of one buffer.  -> (out, ro, rd, bg, field)"""
        train = caller == "view_train"
        route = self._route(caller, num_steps, upsample_steps, **how)
        ro, rd = _flat_rays(rays_o, rays_d)
        N, device = ro.shape[0], ro.device
        noise = torch.empty((N, num_steps), dtype=torch.float32, device=device) if train or self.training else None
        bgs = []
        for k, i in enumerate(range(0, N, batch_size)):
            n = min(batch_size, N - i)
            bgs.append(_background(draw(k, n), n, device, ones=train))
            if noise is not None:
                _draw_noise(noise[i:i + n])
        if all(b is None for b in bgs):
            bg = None
        elif len(bgs) == 1:
            bg = bgs[0].contiguous()
        else:
            bg = torch.cat([b if b is not None else _background(None, min(batch_size, N - k * batch_size), device, ones=True)
                            for k, b in enumerate(bgs)]).contiguous()
        with torch.no_grad():
            field = self._field()
            out = getattr(nsr_ops, route.entry)(field, ro, rd, num_steps, upsample_steps, bound, self.forward_variance(), bg=bg, noise=noise,
                                                cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio,
                                                precision=self.render_precision, **route.options)
        return out, ro, rd, bg, field

    def render_view_nograd(self, rays_o, rays_d, num_steps, upsample_steps, bound, bkg_fn, batch_size, opacity_only=False, cos_anneal_ratio=1.0,
                           normal_epsilon_ratio=0.0):
        """A whole view rendered WITHOUT gradients in ONE launch where the harness (render_instantnsr_naive) makes one launch per `batch_size` rays:
        render_val of a fine-stage stylisation view (stylize.py:98-116: 256 x 256 = 16 batches) and the frozen avatar of its opacity loss (:176-190).
        Rays are independent, so every pixel equals the batch-by-batch render bit for bit -- provided the random draws are the same: they are made here
        exactly as the harness makes them, batch by batch and in its order (bkg_fn(n) -> background of the next n rays; then, in train mode, the jitter
        noise of those rays), into slices of one buffer.  -> (rgb [N,3], weight_sum [N,1]); 11.5 ms per 65 536 rays against 16 x 0.92."""
        out = self._render_view("view_nograd", rays_o, rays_d, num_steps, upsample_steps, bound, lambda k, n: bkg_fn(n), batch_size, cos_anneal_ratio,
                                normal_epsilon_ratio, opacity_only=bool(opacity_only))[0]
        return out["image"], out["weights_sum"][:, None]

    def render_view_train(self, rays_o, rays_d, num_steps, upsample_steps, bound, draw_fn, batch_size, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0):
        """The TRAINING render of a whole view (stylize.py:143-152 renders it patch by patch: 256 x 256 = 16 patches of 4096 rays) as ONE launch that keeps
        its per-sample outputs for ONE backward_last() over all patches -- the patches' gradients add up before the single optimizer.step() anyway
        (stylize.py:199).  Random draws exactly as the patch loop makes them, patch by patch: draw_fn(k, n) -> the background of patch k's n rays (it may make
        further draws of its own there, e.g. the frozen avatar's background), then the jitter noise of those rays.  The eikonal term stays a ratio PER PATCH
        (instant_nsr.py:266-272): eik [P] are the patches' gradient_errors (the bits a launch of the patch alone reports), and backward_last takes one g_eik
        per patch.  -> (rgb [N,3], eik [P], weight_sum [N,1]); pixels equal the patch-by-patch renders bit for bit."""
        out, ro, rd, bg, field = self._render_view("view_train", rays_o, rays_d, num_steps, upsample_steps, bound, draw_fn, batch_size, cos_anneal_ratio,
                                                   normal_epsilon_ratio)
        with torch.no_grad():
            groups = nsr_ops.eikonal_groups(out["eik"], int(batch_size))
        self._last_train = (out, ro, rd, bg, field)
        self._last_train_groups = (int(batch_size), groups)
        self._guard_finite(groups[:, 0].sum())
        return out["image"], groups[:, 0], out["weights_sum"][:, None]

    def backward_last(self, g_image=None, g_weights_sum=None, g_eik=None, split=None):
        """split = (level, side stream): see nsr_ops.render_core_backward (the gradient of table levels >= level is final when the side stream runs)"""
        out, ro, rd, bg, field = self._last_train
        self._last_train = None
        eik_groups = self.__dict__.pop("_last_train_groups", None)
        enc = self.encoder
        prm = [enc.embeddings, self.deviation_net.variance] + [t for l in self.sdf_net for t in (l.weight_v, l.weight_g, l.bias)] + \
              [t for l in self.color_net for t in (l.weight_v, l.weight_g)]
        for t in prm:
            if t.grad is None:
                t.grad = torch.zeros_like(t)
        g_sdf_p, g_col_p, g_invs, *g_vd = nsr_ops.render_core_backward(field, out.opts, out, ro, rd, bg, g_image, g_weights_sum, None, None, g_eik,
                                                                       enc.embeddings.grad, split=split, eik_groups=eik_groups)
        S, K = nsr_ops.SDF_PARAM_GRADS, nsr_ops.COLOR_PARAM_GRADS          # where each matrix lies in the two packed vectors
        s0, s1, c0, c1, c2 = self.sdf_net[0], self.sdf_net[1], self.color_net[0], self.color_net[1], self.color_net[2]
        WN, ADD, VAR = nsr_ops.PG_WEIGHT_NORM, nsr_ops.PG_ADD, nsr_ops.PG_VARIANCE
        var = self.deviation_net.variance
        with torch.no_grad():
            inv_s = self.forward_variance()
        wn = lambda src, at, l: (WN, (src, at.offset), at.stride, l.weight_v.shape[0], l.weight_v.shape[1], l.weight_v.detach(), l.weight_g.detach(),
                                 l.weight_v.grad, l.weight_g.grad)
        add = lambda src, at, l: (ADD, (src, at.offset), at.stride, at.shape[0], 1, None, None, l.bias.grad, None)
        wn_c0 = wn(g_col_p, K["Wc1"], c0)
        if g_vd:                                                 # use_viewdirs: the gradient of the [64,37] effective matrix, columns in the reference's order
            g37 = nsr_ops.join_viewdir_grad(nsr_ops.split_color_param_grads(g_col_p)[0], g_vd[0]).contiguous()
            wn_c0 = wn(g37, nsr_ops.PackedSlot(0, 37, (64, 37)), c0)
        nsr_ops.param_grads([
            wn(g_sdf_p, S["W1"], s0), add(g_sdf_p, S["b1"], s0), wn(g_sdf_p, S["W2"], s1), add(g_sdf_p, S["b2"], s1),
            wn_c0, wn(g_col_p, K["Wc2"], c1), wn(g_col_p, K["Wc3"], c2),
            (VAR, g_invs, 1, g_invs.shape[0], 1, None, inv_s.reshape(-1), var.grad.reshape(-1), None)], ro.device)
        # the kernels wrote the gradients through raw pointers: bump their version counters, so that anything keyed on them -- stylize.Adam.grads_cleared --
        # sees that the buffers are no longer what they were (views of one flat buffer share a counter: one bump per distinct base is enough)
        seen = set()
        for t in prm:
            key = t.grad.untyped_storage().data_ptr()
            if key not in seen:
                seen.add(key)
                torch.autograd.graph.increment_version(t.grad)

    # How a render WITH gradients runs (stylize.py / reconstruct.py):
    #   "core": one operator -- forward = the fused renderer itself (the launch an inference render makes, bit for bit), backward =
    #           ac_render_core_backward (nsr_ops.render_core);
    #   "ops" (or True): sampling launch + the fused SDF-query / colour / compositing operators with torch glue between them (round 1;
    #           kept as the cross-check of "core");
    #   False : sampling launch + torch autograd over the stencil hash encoder (any model configuration).
    fused_training = "core"
    # arithmetic of the fused renderer (ac_render_opts.precision): "exact" (default since round 3: the mode that is pinned bit for bit) = every
    # product an fp32 fma in the oracle's order, GPU == CPU oracle; "fast" (opt-in) = the six finite-difference evaluations of a sample as
    # split-bf16 corrections of the centre's layer 1 and the colour network in split bf16 (normals within 6e-5 of "exact", sample positions /
    # indices / sdf bit-identical).  A training render's backward differentiates the formulation its forward ran.
    render_precision = "exact"
    # the hash table the fused renderer gathers from in inference: "float" (default) = the fp32 parameters; "half" (opt-in) = their fp16 copy
    # (nsr_ops.Field.half_table: 4 bytes per entry instead of 8, made once per parameter version), bit-identical to a render of a model whose table is
    # embeddings.half().float().  "half" applies to run() only in eval() mode and when no gradient is wanted -- canonical and posed renders inside the
    # fused renderer's window; there a long sample count raises NotImplementedError (the long renderer has no half-table form: no silent mix of
    # tables).  Training mode, renders under autograd, run_cuda and everything else read the fp32 table whatever this says.
    render_table_dtype = "float"
    # posed-space inference (render_can=False): samples the SMPL warp masks out contribute alpha * 0 = nothing.  True: tiles of 16 such samples are
    # not evaluated (pixels, depth, normals, weights unchanged bit for bit; the per-sample sdf / colour of skipped samples are 0 and gradient_error,
    # which no inference driver reads, covers the evaluated samples only).  False (default): every output as the reference computes it.
    # drivers.render_animation (render_warp.py's loop, which keeps rgb only) switches it on.
    skip_masked_samples = False
    # posed-space inference at the sample counts outside the fused renderer's window (nsr_ops.in_short_window): False (default) = run(render_can=False)
    # raises NotImplementedError there; True = a no-grad posed render goes to the long renderer (nsr_ops.render_rays_long(warp=...): any num_steps >= 2,
    # upsample_steps a multiple of 16, at most 512 samples).  drivers.render_animation switches it on for its duration.
    posed_long_rays = False
    # the stylisation step without autograd (stylize.sds_step) at the sample counts outside the fused renderer's window, canonical space.  False (default):
    # every route is what it was -- two launches of the long renderer on the one-patch route, no stencil features (ac_render_core_backward gathers the table
    # again), the frozen avatar of the opacity loss renders its colours.  True (opt-in; set it on net_style AND on the frozen net_gt): the step structure of
    # the window -- the one-patch route is ONE launch (nsr_ops.render_rays_long_pair); the one-patch and patch-by-patch training renders keep the stencil
    # features (feat7) where 16 divides num_steps + upsample_steps (other counts keep re-gathering); no-grad renders asked for opacity_only (the frozen
    # avatar: run(), render_view_nograd) skip the colour network.  The whole-view training render (render_view_train) keeps re-gathering either way: 0.9 KB
    # of features per sample is 15 GB for 65 536 rays x 256 samples.  Results: the pair launch and opacity_only change no bit; the saved features change the
    # SDF-network gradient by what the two forms of its backward differ.
    long_step_extras = False
    # posed-space inference through the harness (render_utils.render_instantnsr_naive): the closest-face searches of a frame start from the faces the previous
    # frame found for the same (ray, sample slot) -- an upper bound from a real face, so the same pixels bit for bit, with tighter culling (ac_warp_mesh.seed_faces)
    warp_temporal_seeds = True
    supports_opacity_only = True       # render(..., opacity_only=True) exists (no colour network: the frozen avatar of the opacity loss)
    supports_lean_render = True        # render(..., per_sample=False) exists (render_utils.render_instantnsr_naive asks before passing it)

    def _offsets_host(self):
        oh = getattr(self, "_offsets_cache", None)
        if oh is None:
            oh = self._offsets_cache = self.encoder.offsets.tolist()
        return oh

    def _sdf_supported(self):
        """the SDF side of the default model (16-level, 2-feature hash grid + the 35-64-16 SDF network): what the fused sampling stage needs"""
        enc = getattr(self, "encoder", None)
        return (self.include_input and self.num_layers == 2 and self.hidden_dim == 64 and self.geo_feat_dim == 15 and hasattr(enc, "embeddings")
                and enc.num_levels == 16 and enc.level_dim == 2 and enc.input_dim == 3)

    def _viewdirs_supported(self):
        """use_viewdirs=True as the reference builds it: the degree-4 spherical-harmonics encoder of the ray direction (16 values) in front of the
        colour network (models/instant_nsr.py:565-569: in_dim_color = 16 + 15 + 6 = 37)"""
        e = getattr(self, "encoder_dir", None)
        return getattr(e, "degree", None) == 4 and getattr(e, "output_dim", None) == 16 and self.in_dim_color == 37

    def _fused_supported(self, ignore_curvature=False):
        """the default model (colour net 21-64-64-3), or the same with view directions (37-64-64-3: the renderer folds the 16 spherical harmonics of the ray
        direction into a per-ray bias of colour layer 1, ac_field.Wc1_sh); no curvature term"""
        return (self._sdf_supported() and (not self.use_viewdirs or self._viewdirs_supported()) and self.num_layers_color == 3
                and self.hidden_dim_color == 64 and (ignore_curvature or not self.curvature_loss))

    def _field_sdf_only(self):
        """ac_field with the SDF side only (zero colour matrices): the sampling stage of a model whose colour net the fused renderer does not cover"""
        enc = self.encoder
        prm = [enc.embeddings, self.sdf_net[0].bias, self.sdf_net[1].bias] + [t for l in self.sdf_net for t in (l.weight_v, l.weight_g)]
        key = self._cache_key(prm)
        cached = getattr(self, "_field_sdf_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        with torch.no_grad():
            W = nsr_ops.weight_norm_all(list(self.sdf_net))
            f = nsr_ops.Field.sdf_only(enc.embeddings.detach(), self._offsets_host(), enc.per_level_scale, enc.base_resolution, W[0],
                                       self.sdf_net[0].bias.detach().contiguous(), W[1], self.sdf_net[1].bias.detach().contiguous())
        self._field_sdf_cache = (key, f)
        return f

    def _field_for(self, ignore_curvature=False):
        """the full field where the fused code covers this model's colour side, else the SDF-only field"""
        return self._field() if self._fused_supported(ignore_curvature=ignore_curvature) else self._field_sdf_only()

    def _records_graph(self):
        """would autograd record a render of this model: grad mode on, and a parameter that requires grad"""
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    # ------------------------------------------------------------------ run == reference :133-299
    def run(self, rays_o, rays_d, num_steps, bound, upsample_steps, bg_color, cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0,
            render_can=True, verts=None, faces=None, Ts=None, perturb_overwrite: bool = False, use_mesh_guide: bool = True, per_sample: bool = True,
            opacity_only: bool = False):
        """opacity_only = True (no-grad renders only; what stylize.sds_step asks of the frozen avatar): the colour network is skipped, `rgb` is meaningless,
        weight_sum / depth / normal / gradient_error are unchanged bit for bit.
        per_sample = False (not in the reference's signature; what render_instantnsr_naive passes for its no-grad renders): the per-sample
        results (weights, pts_color, pts_alpha, z_vals) are not produced -- None in the returned tuple -- and the launch runs the renderer's
        lean instantiation (no optional outputs compiled in: no register spills, 12.6 MB less to write per 4096 rays)."""
        if not self._sdf_supported():
            raise NotImplementedError("the MI355X renderer needs the default SDF side of NeRFNetwork (16-level hash grid, include_input, "
                                      "SDF network 35-64-16); other widths / depths have no sampling kernel")
        B, N = rays_o.shape[:2]
        device = rays_o.device
        ro, rd = _flat_rays(rays_o, rays_d)
        inv_s_t = self.forward_variance()
        noise = torch.rand((N, num_steps), device=device) if self.training and perturb_overwrite else None      # :161-162
        bg = None if bg_color is None else _background(bg_color, N, device).contiguous()      # None -> 1 (white), :291-294
        full = self._fused_supported()
        guided = render_can and verts is not None and use_mesh_guide
        needs_grad = self._records_graph()
        route = self._route("run", num_steps, upsample_steps, full, not render_can, needs_grad, guided, bool(per_sample), bool(opacity_only))
        warp = near_far = None
        if not render_can:                                       # SMPL inverse warp :166-172,198-203 (inference path of render_warp.py)
            if verts is None or (not isinstance(verts, nsr_ops.WarpMesh) and (faces is None or Ts is None)):     # (a WarpMesh carries its faces and transforms)
                raise RuntimeError("render_can=False needs verts, faces and Ts")
            warp = verts if isinstance(verts, nsr_ops.WarpMesh) else nsr_ops.WarpMesh(verts, faces, Ts, device, DEFAULT_GEO_THRESH,
                                                                                      DEFAULT_GEO_THRESH, use_mesh_guide)
        elif guided:                                             # canonical render inside the mesh-guided range :147-153
            from ..ray_utils import geometry_guided_near_far
            v = verts.verts if isinstance(verts, nsr_ops.WarpMesh) else verts
            near_far = geometry_guided_near_far(ro, rd, v, DEFAULT_GEO_THRESH)
        launch = getattr(nsr_ops, route.entry)
        if route.then == "autograd":
            # only the sample positions come from the fused (no-grad) stage (:176-184); the render core runs under autograd: through the fused
            # operators for the default model, through torch MLPs over the HIP hash encoder for any colour-net variant (use_viewdirs, curvature)
            z_vals = launch(self._field_for(), ro, rd, num_steps, upsample_steps, bound, noise=noise, near_far=near_far)
            return self._render_core_autograd(ro, rd, z_vals, num_steps, upsample_steps, bound, bg, cos_anneal_ratio, normal_epsilon_ratio, B, N,
                                              near_far=near_far)
        if route.then == "guard":                                # the fused training operator
            W = nsr_ops.weight_norm_all(list(self.sdf_net) + list(self.color_net))
            enc = self.encoder
            (image, wsum, depth, nmap, gerr, weights, alpha, color, z_vals) = launch(
                enc.embeddings, W[0], self.sdf_net[0].bias, W[1], self.sdf_net[1].bias, W[2], W[3], W[4], inv_s_t, ro, rd, bg, noise, self._offsets_host(), enc.per_level_scale, enc.base_resolution,
                num_steps, upsample_steps, bound, cos_anneal_ratio, normal_epsilon_ratio, precision=self.render_precision, warp=warp)
            self._guard_finite(gerr)
            return depth.reshape(B, N), weights, wsum[:, None], image.reshape(B, N, 3), nmap, gerr, 0.0, color, alpha, z_vals
        kw = dict(bg=bg, noise=noise, cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio, precision=self.render_precision, **route.options)
        if route.then == "last_train":                           # a training render without autograd: its per-sample outputs wait for backward_last()
            with torch.no_grad():
                field = self._field()
                out = launch(field, ro, rd, num_steps, upsample_steps, bound, self.forward_variance(), **kw)
            self._last_train = (out, ro, rd, bg, field)
            self._guard_finite(out["eik_res"][0])
        else:
            out = launch(self._field(), ro, rd, num_steps, upsample_steps, bound, inv_s_t, warp=warp, near_far=near_far, **kw)
        return (out["depth"].reshape(B, N), out.get("weights"), out["weights_sum"][:, None], out["image"].reshape(B, N, 3),
                out["normal_map"], out["gradient_error"], 0.0, out.get("color"), out.get("alpha"), out.get("z_vals"))

    def _render_core_autograd(self, rays_o, rays_d, z_vals, num_steps0, upsample_steps, bound, bg_color, cos_anneal_ratio,
                              normal_epsilon_ratio, B, N, near_far=None):
        """The differentiable part of run() (reference :190-299) on the sample positions delivered by the fused kernel."""
        near, far = near_far_from_bound(rays_o, rays_d, bound, type='cube')
        if near_far is not None:                                 # :148-153
            nm, fm = near_far[0].reshape(-1, 1), near_far[1].reshape(-1, 1)
            near = torch.where(torch.isinf(nm), near, nm)
            far = torch.where(torch.isinf(fm), far, fm)
        # (the stand-alone colour operator has no direction input: a model with view directions keeps torch's colour network on this path)
        # (the curvature term does not change the operators of the render core: it adds one more stencil query, below)
        fused_ops = bool(self.fused_training) and self._fused_supported(ignore_curvature=True) and near_far is None and not self.use_viewdirs
        sample_dist = (far - near) / num_steps0
        T = num_steps0 + upsample_steps
        deltas = z_vals[:, 1:] - z_vals[:, :-1]
        deltas = torch.cat([deltas, sample_dist * torch.ones_like(deltas[:, :1])], dim=-1)
        z_mid = torch.cat([z_vals[:, :-1] + 0.5 * deltas[:, :-1], z_vals[:, -1:]], dim=-1)
        pts = (rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z_mid.unsqueeze(-1)).clamp(-bound, bound).float()
        dirs = rays_d.unsqueeze(-2).expand_as(pts)
        flat = pts.reshape(-1, 3)
        fd_eps = nsr_ops.FD_STEP * (1.0 - normal_epsilon_ratio)
        if fd_eps > 0.0 and hasattr(self.encoder, "forward_stencil"):
            sdf_out, gradient = self.forward_sdf_stencil(flat, bound, fd_eps)      # 1 encoder launch + 1 MLP pass for the 7 points
        else:
            sdf_out = self.forward_sdf(flat, bound)
            gradient = self.gradient(flat, bound, fd_eps).squeeze()
        sdf, feat = sdf_out[:, :1], sdf_out[:, 1:]
        normal = gradient / (1e-5 + torch.linalg.norm(gradient, ord=2, dim=-1, keepdim=True))
        if fused_ops and flat.is_cuda:
            color = self.forward_color_fused(flat, normal.reshape(-1, 3), sdf_out)
        else:
            color = self.forward_color(flat, dirs.reshape(-1, 3), normal.reshape(-1, 3), feat, bound)
        pts_norm = torch.linalg.norm(flat, ord=2, dim=-1, keepdim=True).reshape(N, T)
        relax = (pts_norm < 1.2).float().detach()
        gerr = (torch.linalg.norm(gradient.reshape(N, T, 3), ord=2, dim=-1) - 1.0) ** 2
        gradient_error = _relaxed_ratio(relax, gerr)
        self._guard_finite(torch.linalg.norm(gradient.detach()) if gradient.is_cuda else gradient.detach().sum())    # :274 assert (gradient == gradient).all()
        curvature_error = 0.0
        if self.curvature_loss:                                  # :276-288
            draw = getattr(self, "curvature_noise", None)        # (tests replay the reference's recorded draw: a callable (shape, device) -> N(0, 1) values)
            random_vec = 2.0 * (draw(normal.shape, normal.device) if draw is not None else torch.randn_like(normal)) - 1.0
            random_vec_norm = random_vec / (1e-5 + torch.linalg.norm(random_vec, ord=2, dim=-1, keepdim=True))
            perturbed_pts = flat + torch.cross(normal, random_vec_norm, dim=-1) * 0.01 * (1.0 - normal_epsilon_ratio)
            if fd_eps > 0.0 and flat.is_cuda and self.fused_training and self._sdf_supported():
                # self.gradient(perturbed_pts) as ONE stencil query each way: the six offset evaluations in one launch, and in the backward the gradient w.r.t.
                # the perturbed positions themselves (they are a function of the normal: the reference's dy_dx path) -- nsr_ops._SdfStencil
                pg = self.forward_sdf_stencil(perturbed_pts, bound, fd_eps)[1]
            else:
                pg = self.gradient(perturbed_pts, bound, fd_eps).squeeze()
            pn = pg / (1e-5 + torch.linalg.norm(pg, ord=2, dim=-1, keepdim=True))
            cerr = (torch.sum(normal * pn, dim=-1) - 1.0) ** 2
            curvature_error = _relaxed_ratio(relax, cerr.reshape(N, T))
        if fused_ops and flat.is_cuda and T % 16 == 0 and T <= 128:
            # NeuS alpha + compositing as one fused op each way (same arithmetic as the inference renderer)
            bg = None if bg_color is None else _background(bg_color, N, flat.device).contiguous()
            image, wsum, depth, normal_map, weights, alpha = nsr_ops.composite(
                z_vals, sdf.reshape(N, T), normal.reshape(N, T, 3), color.reshape(N, T, 3), self.forward_variance(), rays_o, rays_d, bg, num_steps0,
                bound, cos_anneal_ratio)
            return (depth.reshape(B, N), weights, wsum[:, None], image.reshape(B, N, 3), normal_map, gradient_error, curvature_error, color.reshape(N, T, 3),
                    alpha, z_vals)
        inv_s = self.forward_variance().expand(N * T, 1)
        alpha = _neus_alpha(sdf, inv_s, (dirs.reshape(-1, 3) * normal).sum(-1, keepdim=True), deltas, cos_anneal_ratio).reshape(N, T)
        weights = alpha * torch.cumprod(torch.cat([torch.ones([N, 1], device=alpha.device), 1. - alpha + 1e-7], -1), -1)[:, :-1]
        weights_sum = weights.sum(dim=-1, keepdim=True)
        color = color.reshape(N, T, 3)
        image = (color * weights[:, :, None]).sum(dim=1)
        normal_map = torch.sum(normal.reshape(N, T, 3) * weights[:, :, None], dim=1)
        depth = torch.sum(weights * ((z_vals - near) / (far - near)).clamp(0, 1), dim=-1)
        if bg_color is None:
            bg_color = 1
        image = image + (1 - weights_sum) * bg_color
        return depth.reshape(B, N), weights, weights_sum, image.reshape(B, N, 3), normal_map, gradient_error, curvature_error, color, alpha, z_vals

    # ------------------------------------------------------------------ render == reference :358-408
    def render(self, rays_o, rays_d, num_steps, bound, upsample_steps, staged=False, max_ray_batch=4096, bg_color=None,
               cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0, render_can=True, verts=None, faces=None, Ts=None, perturb: bool = False,
               use_mesh_guide: bool = True, per_sample: bool = True, opacity_only: bool = False, **kwargs):
        B, N = rays_o.shape[:2]
        device = rays_o.device
        if staged and not self.cuda_ray:
            depth = torch.empty((B, N), device=device); image = torch.empty((B, N, 3), device=device)
            normal = torch.empty((B, N, 3), device=device)
            weights = weight_sum = pts_color = pts_alpha = z_vals = None
            gradient_error = curvature_error = 0.0
            for b in range(B):
                head = 0
                while head < N:
                    tail = min(head + max_ray_batch, N)
                    r = self.run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], num_steps, bound, upsample_steps, bg_color,
                                 cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio)
                    depth[b:b + 1, head:tail] = r[0].detach(); image[b:b + 1, head:tail] = r[3].detach()
                    normal[b, head:tail] = r[4].detach()
                    head += max_ray_batch
        else:
            _run = self.run_cuda if self.cuda_ray else self.run           # :360-363 (the reference has no run_cuda: see there)
            (depth, weights, weight_sum, image, normal, gradient_error, curvature_error, pts_color, pts_alpha, z_vals) = _run(
                rays_o, rays_d, num_steps, bound, upsample_steps, bg_color, cos_anneal_ratio, normal_epsilon_ratio, render_can=render_can,
                verts=verts, faces=faces, Ts=Ts, perturb_overwrite=perturb, use_mesh_guide=use_mesh_guide, per_sample=per_sample,
                **({"opacity_only": True} if (opacity_only and not self.cuda_ray) else {}))
        return {'depth': depth, 'weights': weights, 'weight_sum': weight_sum, 'rgb': image, 'normal': normal,
                'gradient_error': gradient_error, 'curvature_error': curvature_error, 'pts_color': pts_color, 'pts_alpha': pts_alpha,
                'z_vals': z_vals}


