"""Instant-NSR model + NeuS renderer behind the reference's model API (models/instant_nsr.py:90-726).

`NeRFNetwork()` has the reference's constructor, parameter names (state_dict keys: encoder.embeddings,
encoder.offsets, sdf_net.{0,1}.{bias,weight_g,weight_v}, color_net.{0,1,2}.{weight_g,weight_v},
deviation_net.variance -- SURVEY section 5) and `.render(...)` signature / result keys, so the reference's drivers
and checkpoints (bare_smpl.pth.tar) work unchanged.

Where the work happens:
  * no-grad rendering (render_canonical, render_val, the sampling stage of every training render) is ONE launch of
    the fused HIP kernel (nsr_ops.render_rays == NeRFRenderer.run :133-299);
  * rendering with gradients (stylize / reconstruct) takes the sample positions from the fused kernel (the reference
    computes them under no_grad, :176-184) and evaluates the differentiable "render core" (:190-299) with autograd
    over the HIP hash encoder; a fused backward kernel is the next step.
  * render_can=False (SMPL inverse warp, :166-172,198-203): no-grad only (render_warp.py), ac_render_rays_warped; at sample counts
    outside the fused renderer's window ac_render_rays_long_warped (opt-in: posed_long_rays).
"""
import collections
import math

import numpy as np

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import nsr_ops
from .encoder import get_encoder

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


# What render_route() decides: the nsr_ops entry to launch (looked up by name at call time), the keyword options that depend on the route, and what follows
# the launch -- None (an inference render), "last_train" (a training render without autograd: its outputs are kept for backward_last()), "guard" (the fused
# training operator: its gradient_error feeds the NaN guard) or "autograd" (the entry only samples: _render_core_autograd runs on its z_vals).
Route = collections.namedtuple("Route", "entry options then")
_TRAINS = dict(extras=True, train_extras=True)


def _keeps_stencil(long_step_extras, num_steps, upsample_steps):
    """a training render at a long count keeps the stencil features (feat7): the switch, and a count 16 divides"""
    return bool(long_step_extras) and (int(num_steps) + int(upsample_steps)) % 16 == 0


def render_route(caller, num_steps, upsample_steps, *, posed, needs_grad, full, training, near_far, per_sample, opacity_only, fused_training,
                 manual_backward, render_table_dtype, skip_masked_samples, posed_long_rays, long_step_extras, use_viewdirs):
    """THE routing decision of every render of NeRFRenderer: given the sample counts, the space, whether a gradient is wanted, the model's switches and
    the mode -> the Route to launch, or the error that names the rule.  Pure: no tensor, no device (DESIGN.md section 5.10 lists the outcomes).
    caller: "run" (run()), "step_pair" (render_step_pair), "view_nograd" (render_view_nograd), "view_train" (render_view_train).
    full: _fused_supported() for run(); for the three step renders "the default model, on the GPU".  near_far: a mesh-guided range is present.
    The step renders are canonical and know no gradient: they ignore posed / needs_grad / near_far / per_sample."""
    long_counts = not nsr_ops.in_short_window(num_steps, upsample_steps)
    render = "render_rays_long" if long_counts else "render_rays"
    if caller != "run":
        if caller == "view_nograd":
            if not full:
                raise RuntimeError("render_view_nograd: needs the default model on the GPU")
            # (at the long renderer's counts opacity_only renders the colour too unless long_step_extras is on: weight_sum is the same bits either way)
            return Route(render, dict(extras=False, opacity_only=opacity_only) if long_step_extras or not long_counts else dict(extras=False), None)
        # the two training renders of the stylisation step without autograd; with view directions the fused backward needs a count 16 divides
        if not (training and fused_training == "core" and full and not (use_viewdirs and (int(num_steps) + int(upsample_steps)) % 16)):
            raise RuntimeError(f"render_{caller}: needs the default model in train mode on the GPU")
        if caller == "view_train":          # (never the stencil features at a long count: 0.9 KB per sample of a whole view)
            return Route(render, _TRAINS, "last_train")
        if not long_counts:
            return Route("render_rays_pair", {}, "last_train")
        if long_step_extras:                # the long pair launch; the stencil features where 16 divides the count
            return Route("render_rays_long_pair", dict(save_stencil=_keeps_stencil(True, num_steps, upsample_steps)), "last_train")
        return Route(render, _TRAINS, "last_train")            # (long_step_extras off): two launches of the long renderer
    # counts outside the fused renderer's window go to the long renderer: canonical space, and posed space without gradients when posed_long_rays is on
    if long_counts:
        if posed and not posed_long_rays:
            raise NotImplementedError(f"posed-space rendering supports num_steps and upsample_steps that are multiples of 16 with "
                                      f"16 <= num_steps <= 64 and num_steps + upsample_steps <= 128 only (got {num_steps} + {upsample_steps}); "
                                      f"longer rays render in canonical space (render_can=True), or in posed space without gradients with "
                                      f"posed_long_rays = True")
        nsr_ops.check_long_counts(num_steps, upsample_steps)
    if render_table_dtype not in nsr_ops.TABLE_DTYPES:
        raise RuntimeError(f"render_table_dtype must be one of {nsr_ops.TABLE_DTYPES}, got {render_table_dtype!r}")
    # the half table: eval mode, no gradient wanted, the default model
    half = render_table_dtype == "half" and not needs_grad and not training and full
    if half and long_counts:
        raise NotImplementedError(f"render_table_dtype = 'half' renders inside the fused renderer's window only (multiples of 16, 16 <= num_steps <= 64, "
                                  f"at most 128 samples; got {num_steps} + {upsample_steps}): the long renderer reads the fp32 table, and an inference "
                                  f"render does not switch tables silently")
    if posed:
        if long_counts and needs_grad:
            raise NotImplementedError(f"posed-space training is built for the short window only (multiples of 16, 16 <= num_steps <= 64, at most 128 "
                                      f"samples; got {num_steps} + {upsample_steps}): the long posed renderer (posed_long_rays) runs under no_grad")
        if long_counts and opacity_only:
            raise NotImplementedError("opacity_only is not supported by the long renderer")
        if needs_grad and fused_training != "core":
            raise NotImplementedError("posed-space rendering under autograd runs through the fused operator only (fused_training = 'core')")
        if not full:
            raise NotImplementedError("posed-space rendering is built for the default NeRFNetwork (with or without view directions; no curvature term)")
    fused_op = needs_grad and full and fused_training == "core" and not near_far
    # only the sample positions come from the fused (no-grad) stage; the render core runs under autograd
    autograd = not posed and (needs_grad or not full)
    if fused_op and manual_backward and not posed:
        # (at the long counts the long renderer's launch: ac_render_core_backward takes its outputs as well)
        keep = long_counts and _keeps_stencil(long_step_extras, num_steps, upsample_steps)
        return Route(render, dict(_TRAINS, save_stencil=True) if keep else _TRAINS, "last_train")
    if long_counts:
        # (the fused training operator takes at most 128 samples: the long counts take the autograd render core, which handles any T)
        if autograd:
            return Route("sample_rays_long", {}, "autograd")
        return Route(render, dict(extras=per_sample, skip_masked=bool(skip_masked_samples) and posed,
                                  opacity_only=opacity_only and not posed and bool(long_step_extras)), None)
    if fused_op:
        return Route("render_core", {}, "guard")
    if autograd:
        return Route("sample_rays", {}, "autograd")
    return Route(render, dict(extras=per_sample, skip_masked=skip_masked_samples, opacity_only=opacity_only,
                              table_dtype="half" if half else "float"), None)


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


class NeRFRenderer(nn.Module):
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
    # they are left out of pickling / copy.deepcopy / torch.save(net) and rebuilt on the next render.
    _CACHE_ATTRS = ("_pair_bg_cache", "_field_cache", "_field_sdf_cache", "_last_train", "_offsets_cache", "_axis_cache")
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
        from . import ray_utils
        ray_utils.invalidate_caches()

    # The reference stops a training render on a NaN normal (`assert (gradient == gradient).all()`, instant_nsr.py:274), which costs it a host
    # round trip per render.  Here every training render leaves a one-word "gradient_error is not finite" flag in pinned host memory behind an
    # event; the flags of earlier renders are looked at (never waited for) on the next one, and check_finite() waits for all of them.
    # The step functions (stylize.sds_step, reconstruct.reconstruct_step) call check_finite() BEFORE optimizer.step(): the event is recorded right
    # behind the training forward, i.e. it has fired long before the host gets there (the backward is still queued), so a poisoned gradient raises
    # before Adam's state or the weights are touched -- the reference's order (assert, then backward, then step).  A caller that drives
    # render() + its own optimizer gets the flag on its next render, on check_finite(), or when the net is pickled / checkpointed / deep-copied.
    # nan_guard = False switches it off.
    nan_guard = True

    def _guard_finite(self, gerr):
        # a data-parallel step is collecting (stylize._collective_verdict): the flag is NOT judged on this rank -- neither now nor by a later render's
        # non-waiting poll (a rank whose patch k produced NaN raised inside patch k + 1's render, before the gradient collective, and the
        # healthy ranks hung in the all-reduce) -- it is folded into the guard word of the step's collective, whose verdict every rank sees
        defer = self.__dict__.get("_nan_deferred")
        if defer is not None:
            if self.nan_guard and isinstance(gerr, torch.Tensor):
                defer.append(gerr.detach().reshape(-1)[:1].float())
            return
        if not self.nan_guard or not isinstance(gerr, torch.Tensor) or not gerr.is_cuda:
            if self.nan_guard and isinstance(gerr, torch.Tensor) and not bool(torch.isfinite(gerr).all()):
                raise FloatingPointError("NaN / Inf in the finite-difference normals of a training render (reference: instant_nsr.py:274)")
            return
        pend = self.__dict__.setdefault("_nan_pending", [])
        self._poll_finite(wait=False)
        host = torch.zeros(1, dtype=torch.float32).pin_memory()      # the value itself travels (one 4-byte copy, no kernel); it is judged on the host
        host.copy_(gerr.detach().reshape(1), non_blocking=True)
        ev = torch.cuda.Event(); ev.record()
        pend.append((ev, host))

    def _poll_finite(self, wait):
        pend = self.__dict__.get("_nan_pending", [])
        while pend and (wait or pend[0][0].query()):
            ev, host = pend.pop(0)
            ev.synchronize()
            if not math.isfinite(float(host[0])):
                pend.clear()
                raise FloatingPointError("NaN / Inf in the finite-difference normals of a training render (reference: instant_nsr.py:274)")

    def check_finite(self):
        """wait for the NaN flags of every training render issued so far; raises FloatingPointError if one of them was set"""
        self._poll_finite(wait=True)

    def _cache_key(self, prm):
        from . import _lib as L
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
        """a training render at a long count keeps the stencil features: long_step_extras, and a count 16 divides"""
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
        ro = rays_o.reshape(-1, 3).float().contiguous()
        rd = rays_d.reshape(-1, 3).float().contiguous()
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
        ro = rays_o.reshape(-1, 3).float().contiguous()
        rd = rays_d.reshape(-1, 3).float().contiguous()
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
        ro = rays_o.reshape(-1, 3).float().contiguous()
        rd = rays_d.reshape(-1, 3).float().contiguous()
        inv_s_t = self.forward_variance()
        noise = torch.rand((N, num_steps), device=device) if self.training and perturb_overwrite else None      # :161-162
        bg = None if bg_color is None else _background(bg_color, N, device).contiguous()      # None -> 1 (white), :291-294
        full = self._fused_supported()
        guided = render_can and verts is not None and use_mesh_guide
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        route = self._route("run", num_steps, upsample_steps, full, not render_can, needs_grad, guided, bool(per_sample), bool(opacity_only))
        warp = near_far = None
        if not render_can:                                       # SMPL inverse warp :166-172,198-203 (inference path of render_warp.py)
            if verts is None or (not isinstance(verts, nsr_ops.WarpMesh) and (faces is None or Ts is None)):     # (a WarpMesh carries its faces and transforms)
                raise RuntimeError("render_can=False needs verts, faces and Ts")
            warp = verts if isinstance(verts, nsr_ops.WarpMesh) else nsr_ops.WarpMesh(verts, faces, Ts, device, DEFAULT_GEO_THRESH,
                                                                                      DEFAULT_GEO_THRESH, use_mesh_guide)
        elif guided:                                             # canonical render inside the mesh-guided range :147-153
            from .ray_utils import geometry_guided_near_far
            v = verts.verts if isinstance(verts, nsr_ops.WarpMesh) else verts
            near_far = geometry_guided_near_far(ro, rd, v, DEFAULT_GEO_THRESH)
        launch = getattr(nsr_ops, route.entry)
        if route.then == "autograd":
            # only the sample positions come from the fused (no-grad) stage (:176-184); the render core runs under autograd: through the fused
            # operators for the default model, through torch MLPs over the HIP hash encoder for any colour-net variant (use_viewdirs, curvature)
            z_vals = launch(self._field() if full else self._field_sdf_only(), ro, rd, num_steps, upsample_steps, bound, noise=noise, near_far=near_far)
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
        gradient_error = (relax * gerr).sum() / (relax.sum() + 1e-5)
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
            curvature_error = (relax * cerr.reshape(N, T)).sum() / (relax.sum() + 1e-5)
        if fused_ops and flat.is_cuda and T % 16 == 0 and T <= 128:
            # NeuS alpha + compositing as one fused op each way (same arithmetic as the inference renderer)
            bg = None if bg_color is None else _background(bg_color, N, flat.device).contiguous()
            image, wsum, depth, normal_map, weights, alpha = nsr_ops.composite(
                z_vals, sdf.reshape(N, T), normal.reshape(N, T, 3), color.reshape(N, T, 3), self.forward_variance(), rays_o, rays_d, bg, num_steps0,
                bound, cos_anneal_ratio)
            return (depth.reshape(B, N), weights, wsum[:, None], image.reshape(B, N, 3), normal_map, gradient_error, curvature_error, color.reshape(N, T, 3),
                    alpha, z_vals)
        inv_s = self.forward_variance().expand(N * T, 1)
        true_cos = (dirs.reshape(-1, 3) * normal).sum(-1, keepdim=True)
        act = nn.Softplus(beta=100)
        iter_cos = -(act(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + act(-true_cos) * cos_anneal_ratio)
        half = iter_cos * deltas.reshape(-1, 1) * 0.5
        prev_cdf = torch.sigmoid((sdf - half) * inv_s)
        next_cdf = torch.sigmoid((sdf + half) * inv_s)
        alpha = ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).reshape(N, T).clip(0.0, 1.0)
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

    # ------------------------------------------------------------------ occupancy-grid rendering (cuda_ray = True)
    occupancy_train_one_launch = True  # run_cuda's train() branch under no_grad (stylize.py's render_val of a cuda_ray net) as ONE launch (ac_render_rays_occupancy_train);
                                       # False: the chain of operators (march_rays_train / ac_field_samples / composite_rays_train x 2 / torch) -- same pixels
    occupancy_rounds = False           # True: run_cuda's eval() as the reference-shaped loop of compact / march / field / composite rounds (same results)
    occupancy_fused_shading = True     # run_cuda's train() branch UNDER AUTOGRAD: normal / NeuS alpha / eikonal terms of the packed samples as one launch each way
                                       # (nsr_ops.packed_shading); False: the torch formulation (kept as the cross-check of the tests)

    def run_cuda(self, rays_o, rays_d, num_steps, bound, upsample_steps, bg_color, cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0, render_can=True,
                 verts=None, faces=None, Ts=None, perturb_overwrite: bool = False, use_mesh_guide: bool = True, per_sample: bool = True, max_steps=1024):
        """The render path the reference dispatches to when cuda_ray=True (models/instant_nsr.py:358-363) and never defines: the chain its
        raymarching module and density grid exist for (raymarching/raymarching.py:21-188, update_extra_state :303-356), in the shape of the Instant-NSR
        code base the module was taken from --

          train():  march_rays_train (occupancy grid, perturb, align 128) -> field on the packed samples -> composite_rays_train (+ background)
          eval():   loop { compact_rays; march_rays (n_step = clamp(N / n_alive, 1, 8)); field; composite_rays } until no ray is alive or max_steps

        with the field evaluated per sample exactly like run()'s render core (:205-243): forward_sdf, finite-difference normal, forward_color and
        the NeuS alpha with the marcher's step as the section length (ac_field_samples: one fused launch; under autograd the SDF-query / colour
        operators with their fused backward).  composite_rays_train treats its first input as alpha (quirk C.4), so the chain is consistent.
        num_steps / upsample_steps are unused (the marcher decides the sampling).  Returns run()'s tuple; per-sample entries are None and the
        training depth is zero (the packed compositor has none)."""
        from . import raymarching
        if not self.cuda_ray:
            raise RuntimeError("run_cuda needs NeRFNetwork(cuda_ray=True) (density grid + step counters)")
        if not render_can:
            raise NotImplementedError("the occupancy grid lives in canonical space: cuda_ray renders render_can=True only")
        if not self._fused_supported():
            raise NotImplementedError("run_cuda is built for the default NeRFNetwork (with or without view directions; no curvature term)")
        fd_eps = nsr_ops.FD_STEP * (1.0 - normal_epsilon_ratio)
        if not fd_eps > 0.0:
            raise RuntimeError("run_cuda: normal_epsilon_ratio must be < 1 (finite-difference step 0.005 * (1 - ratio) > 0)")
        B, N = rays_o.shape[:2]
        device = rays_o.device
        ro = rays_o.reshape(-1, 3).float().contiguous()
        rd = rays_d.reshape(-1, 3).float().contiguous()
        n_rays = ro.shape[0]
        bg = 1.0
        if bg_color is not None:
            bg = torch.as_tensor(bg_color, dtype=torch.float32, device=device)
            bg = bg.reshape(-1, 3) if bg.numel() >= 3 else bg.reshape(1, 1)
        inv_s_t = self.forward_variance()
        if self.training:
            counter = self.step_counter[self.local_step % 64]
            counter.zero_()
            self.local_step += 1
            needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            budgeted = self.mean_count > 0
            if not needs_grad and budgeted and self.occupancy_train_one_launch:
                # no graph wanted (and a budget, so that the packed layout has a size before anything is counted): walk, packed samples, field, both composites,
                # the eikonal term and the background in one launch -- the same pixels as the chain below
                cap = raymarching.raymarching._round_up(int(self.mean_count), 128)                        # (march_rays_train's capacity: + 128 - n % 128)
                try:
                    o = nsr_ops.render_rays_occupancy_train(self._field(), ro, rd, self.density_grid, self.mean_density, bound, fd_eps, inv_s_t, cos_anneal_ratio,
                                                            perturb=bool(perturb_overwrite), capacity=cap, composite_capacity=cap, counter=counter, bg=bg)
                except nsr_ops.OccupancyBarrierTimeout:
                    # a grid barrier of the one launch timed out (compute units held by a foreign kernel for seconds): nothing was returned; the chain of
                    # operators below has no barriers and gives the same pixels.  The step counter may hold the failed launch's partial update.
                    o = None
                    counter.zero_()
                if o is not None:
                    gradient_error = o["gradient_error"][0]
                    self._guard_finite(gradient_error)
                    depth = torch.zeros(n_rays, dtype=torch.float32, device=device)
                    return (depth.reshape(B, N), None, o["weights_sum"][:, None], o["image"].reshape(B, N, 3), o["normal_map"], gradient_error, 0.0, None, None, None)
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(ro, rd, bound, self.density_grid, self.mean_density, self.iter_density, counter,
                                                                    self.mean_count, bool(perturb_overwrite), 128, False)
            M = xyzs.shape[0]
            if budgeted:
                # the rays the budget left out wrote nothing: the marched samples are a prefix of the layout that ends with the last ray that fitted
                # (rows behind it are zeros -- and would otherwise count as samples AT THE ORIGIN in the eikonal term)
                ends = rays[:, 1] + rays[:, 2]
                n_valid = (ends * ((rays[:, 2] > 0) & (ends < M))).max()
            else:
                n_valid = counter[0]
            valid = (torch.arange(M, device=device) < n_valid).float()             # rows past the marched samples are alignment padding (all-zero rows)
            if needs_grad:
                enc = self.encoder
                W = nsr_ops.weight_norm_all(list(self.sdf_net) + list(self.color_net))
                sdf_out, gradient = nsr_ops.sdf_stencil(xyzs, enc.embeddings, W[0], self.sdf_net[0].bias, W[1], self.sdf_net[1].bias, self._offsets_host(),
                                                        enc.per_level_scale, enc.base_resolution, bound, fd_eps)
                if self.occupancy_fused_shading:
                    # normal, the cos-annealed NeuS alpha and the per-sample eikonal terms as ONE launch each way (round 6: the ~40 torch kernels of the
                    # formulation in the else branch were 2.5 ms of forward + backward per 4096-ray batch against 0.5 ms for the no-grad launch)
                    nv = n_valid if isinstance(n_valid, torch.Tensor) else torch.tensor(int(n_valid), dtype=torch.int32, device=device)
                    alpha, normal, eik2 = nsr_ops.packed_shading(sdf_out, gradient, inv_s_t, xyzs, dirs, deltas, nv, cos_anneal_ratio)
                else:
                    normal = gradient / (1e-5 + torch.linalg.norm(gradient, ord=2, dim=-1, keepdim=True))
                if self.use_viewdirs:                            # (the stand-alone colour operator has no direction input: torch's colour network here)
                    rgbs = self.forward_color(xyzs, dirs, normal, sdf_out[:, 1:], bound)
                else:
                    rgbs = nsr_ops.color_mlp(xyzs, normal, sdf_out, W[2], W[3], W[4])
                if not self.occupancy_fused_shading:
                    true_cos = (dirs * normal).sum(-1, keepdim=True)
                    act = nn.Softplus(beta=100)
                    iter_cos = -(act(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + act(-true_cos) * cos_anneal_ratio)
                    half = iter_cos * deltas.reshape(-1, 1) * 0.5
                    sdf = sdf_out[:, :1]
                    prev_cdf, next_cdf = torch.sigmoid((sdf - half) * inv_s_t), torch.sigmoid((sdf + half) * inv_s_t)
                    alpha = ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).reshape(-1).clip(0.0, 1.0)
            else:
                fs = nsr_ops.field_samples(self._field(), xyzs, dirs, deltas, bound, fd_eps, inv_s_t, cos_anneal_ratio, want_gradient=True)
                alpha, rgbs, normal, gradient = fs["alpha"], fs["rgb"], fs["normal"], fs["gradient"]
            if needs_grad and self.occupancy_fused_shading:
                es = eik2.sum(0)
                gradient_error = es[0] / (es[1] + 1e-5)                                   # :266-272 over the packed samples
            else:
                relax = (torch.linalg.norm(xyzs, ord=2, dim=-1) < 1.2).float() * valid
                gerr = (torch.linalg.norm(gradient, ord=2, dim=-1) - 1.0) ** 2
                gradient_error = (relax * gerr).sum() / (relax.sum() + 1e-5)             # :266-272 over the packed samples
            self._guard_finite(gradient_error)
            weights_sum, image = raymarching.composite_rays_train(alpha, rgbs, deltas, rays, bound)
            with torch.no_grad():
                _, normal_map = raymarching.composite_rays_train(alpha.detach(), normal.detach().contiguous(), deltas, rays, bound)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg
            depth = torch.zeros(n_rays, dtype=torch.float32, device=device)
            return depth.reshape(B, N), None, weights_sum[:, None], image.reshape(B, N, 3), normal_map, gradient_error, 0.0, None, None, None
        # ---- inference.  Default: ONE launch (ac_render_rays_occupancy: march + field + composite per ray, a wave's 64 rays packed into tiles) -- the
        # same bits as the reference-shaped loop below without its rounds and host read-backs; occupancy_rounds = True selects the loop.  max_steps: the
        # one launch stops a ray after exactly max_steps samples, the loop after max_steps .. max_steps + 7 (it stops at the first round that brings its step
        # count to >= max_steps): the two agree bit for bit on every ray that needs fewer (tests/test_gpu_run_cuda.py checks both sides of that line).
        if not self.occupancy_rounds:
            with torch.no_grad():
                near, far = near_far_from_bound(ro, rd, bound, type='cube')
                near, far = near.reshape(-1), far.reshape(-1)
                o = nsr_ops.render_rays_occupancy(self._field(), ro, rd, self.density_grid, self.mean_density, bound, fd_eps, inv_s_t, cos_anneal_ratio,
                                                  max_steps=max_steps)
                self._last_cuda_rounds = 0
                image = o["image"] + (1 - o["weights_sum"]).unsqueeze(-1) * bg
                depth = torch.clamp(o["depth"] - near, min=0) / (far - near)
                return (depth.reshape(B, N), None, o["weights_sum"][:, None], image.reshape(B, N, 3), o["normal_map"],
                        torch.zeros((), dtype=torch.float32, device=device), 0.0, None, None, None)
        # ---- the loop: march / evaluate / composite in rounds, dead rays compacted away between rounds (one 4-byte D2H per round, like the reference's
        # `alive_counter.item()`: the next round's step count depends on it)
        with torch.no_grad():
            field = self._field()
            f32 = dict(dtype=torch.float32, device=device)
            weights_sum, depth = torch.zeros(n_rays, **f32), torch.zeros(n_rays, **f32)
            image, normal_map = torch.zeros(n_rays, 3, **f32), torch.zeros(n_rays, 3, **f32)
            near, far = near_far_from_bound(ro, rd, bound, type='cube')
            near, far = near.reshape(-1).contiguous(), far.reshape(-1).contiguous()
            n_alive = n_rays
            alive_counter = torch.zeros(1, dtype=torch.int32, device=device)
            rays_alive = torch.zeros(2, n_rays, dtype=torch.int32, device=device)
            rays_t = torch.zeros(2, n_rays, **f32)
            step = rnd = 0
            while step < max_steps:
                if step == 0:
                    rays_alive[0] = torch.arange(n_rays, dtype=torch.int32, device=device)
                    rays_t[0] = near
                else:
                    alive_counter.zero_()
                    raymarching.compact_rays(n_alive, rays_alive[rnd % 2], rays_alive[(rnd + 1) % 2], rays_t[rnd % 2], rays_t[(rnd + 1) % 2], alive_counter)
                    n_alive = int(alive_counter.item())
                if n_alive <= 0:
                    break
                n_step = max(min(n_rays // n_alive, 8), 1)
                xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, rays_alive[rnd % 2], rays_t[rnd % 2], ro, rd, bound, self.density_grid,
                                                            self.mean_density, near, far, 128, False)
                fs = nsr_ops.field_samples(field, xyzs, dirs, deltas, bound, fd_eps, inv_s_t, cos_anneal_ratio)
                raymarching.composite_rays(n_alive, n_step, rays_alive[rnd % 2], rays_t[rnd % 2], fs["alpha"], fs["rgb"], fs["normal"], deltas, weights_sum,
                                           depth, image, normal_map)
                step += n_step
                rnd += 1
            self._last_cuda_rounds = rnd
            image = image + (1 - weights_sum).unsqueeze(-1) * bg
            depth = torch.clamp(depth - near, min=0) / (far - near)
            return (depth.reshape(B, N), None, weights_sum[:, None], image.reshape(B, N, 3), normal_map, torch.zeros((), **f32), 0.0, None, None, None)

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


class NeRFNetwork(NeRFRenderer):
    """models/instant_nsr.py:478-718; the construction order (and therefore the RNG stream) follows the reference,
    so torch.manual_seed(s); NeRFNetwork() yields the same initial parameters."""

    def __init__(self, encoding="hashgrid", encoding_dir="sphere_harmonics", num_layers=2, hidden_dim=64, geo_feat_dim=15,
                 num_layers_color=3, hidden_dim_color=64, bound=1.0, geometric_init=True, weight_norm=True, cuda_ray=False,
                 include_input=True, curvature_loss=False, use_viewdirs=False):
        super().__init__(cuda_ray, curvature_loss)
        self.num_layers, self.hidden_dim, self.geo_feat_dim, self.include_input = num_layers, hidden_dim, geo_feat_dim, include_input
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.use_viewdirs = use_viewdirs
        pos_cfg = {"in_dim": 3, "freq_multires": 6, "hash_num_levels": 16, "hash_level_dim": 2, "hash_base_resolution": 16,
                   "hash_per_level_scale": 1.3819, "hash_log2_hashmap_size": 19, "hash_desired_resolution": 2048}
        dir_cfg = {"in_dim": 3, "freq_multires": 4}
        self.encoder, self.in_dim = get_encoder(encoding, pos_cfg)
        sdf_net = []
        for l in range(num_layers):
            in_dim = (self.in_dim + 3 if include_input else self.in_dim) if l == 0 else hidden_dim
            out_dim = 1 + geo_feat_dim if l == num_layers - 1 else hidden_dim
            lin = nn.Linear(in_dim, out_dim)
            if geometric_init:
                if l == num_layers - 1:
                    torch.nn.init.normal_(lin.weight, mean=np.sqrt(np.pi) / np.sqrt(in_dim), std=0.0001)
                    torch.nn.init.constant_(lin.bias, 0)
                elif l == 0 and include_input:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.normal_(lin.weight[:, :3], 0.0, np.sqrt(2) / np.sqrt(out_dim))
                    torch.nn.init.constant_(lin.weight[:, 3:], 0.0)
                else:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.normal_(lin.weight[:, :], 0.0, np.sqrt(2) / np.sqrt(out_dim))
            if weight_norm:
                lin = nn.utils.weight_norm(lin)
            sdf_net.append(lin)
        self.sdf_net = nn.ModuleList(sdf_net)
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        self.encoder_dir = None
        if use_viewdirs:
            self.encoder_dir, self.in_dim_color = get_encoder(encoding_dir, dir_cfg)
            self.in_dim_color = self.in_dim_color + geo_feat_dim + 6
        else:
            self.in_dim_color = geo_feat_dim + 6
        color_net = []
        for l in range(num_layers_color):
            lin = nn.Linear(self.in_dim_color if l == 0 else hidden_dim, 3 if l == num_layers_color - 1 else hidden_dim, bias=False)
            if weight_norm:
                lin = nn.utils.weight_norm(lin)
            color_net.append(lin)
        self.color_net = nn.ModuleList(color_net)
        self.deviation_net = SingleVarianceNetwork(0.3)
        self.activation = nn.Softplus(beta=100)

    # ---- differentiable field (autograd path: HIP hash encoder + torch MLP), reference :627-704
    def forward_sdf(self, x, bound):
        h = self.encoder(x, bound)
        if self.include_input:
            h = torch.cat([x, h], dim=-1)
        for l in range(self.num_layers):
            h = self.sdf_net[l](h)
            if l != self.num_layers - 1:
                h = self.activation(h)
        return h

    def forward_sdf_stencil(self, x, bound, epsilon):
        """forward_sdf(x) (:627-642) and finite_difference_normals_approximator(x) (:687-704) together: the seven hash encodings
        come from one stencil launch (encoder.forward_stencil) and the SDF MLP runs once over the 7B points.
        Returns (sdf_out [B,16], gradient [B,3])."""
        if self.fused_training and self._sdf_supported() and x.is_cuda:            # one kernel forward, two backward (csrc/sdf_stencil_train.hip)
            l0, l1, enc = self.sdf_net[0], self.sdf_net[1], self.encoder
            W = nsr_ops.weight_norm_all([l0, l1])                                   # the same effective matrices as every other fused path, bit for bit
            return nsr_ops.sdf_stencil(x, enc.embeddings, W[0], l0.bias, W[1], l1.bias, self._offsets_host(), enc.per_level_scale,
                                       enc.base_resolution, bound, epsilon)
        B = x.shape[0]
        h7 = self.encoder.forward_stencil(x, bound, epsilon)                       # [7,B,32]: x, +x, -x, +y, -y, +z, -z
        pts = x.unsqueeze(0).repeat(7, 1, 1)
        for k in range(3):
            pts[1 + 2 * k, :, k] = (x[:, k] + epsilon).clamp(-bound, bound)
            pts[2 + 2 * k, :, k] = (x[:, k] - epsilon).clamp(-bound, bound)
        h = torch.cat([pts, h7], dim=-1).reshape(7 * B, -1) if self.include_input else h7.reshape(7 * B, -1)
        for l in range(self.num_layers):
            h = self.sdf_net[l](h)
            if l != self.num_layers - 1:
                h = self.activation(h)
        h = h.view(7, B, -1)
        gradient = (0.5 * (h[1::2, :, 0] - h[2::2, :, 0]) / epsilon).t()
        return h[0], gradient

    def forward_color_fused(self, x, n, sdf_out):
        """forward_color on the outputs of forward_sdf (sdf_out [B,16] = [sdf, feat]) as one fused op with a fused backward"""
        W = nsr_ops.weight_norm_all(list(self.color_net))
        return nsr_ops.color_mlp(x, n, sdf_out, W[0], W[1], W[2])

    def forward_color(self, x, d, n, geo_feat, bound):
        if self.use_viewdirs:
            h = torch.cat([x, self.encoder_dir(d), n, geo_feat], dim=-1)
        else:
            h = torch.cat([x, n, geo_feat], dim=-1)
        for l in range(self.num_layers_color):
            h = self.color_net[l](h)
            if l != self.num_layers_color - 1:
                h = F.relu(h, inplace=True)
        return torch.sigmoid(h)

    def forward_variance(self):
        v = self.deviation_net.variance
        if not (torch.is_grad_enabled() and v.requires_grad):
            # no graph wanted: the value only changes with the parameter (five small launches per render otherwise; the frozen net_gt of the
            # stylisation step never changes at all)
            key = (v.data_ptr(), v._version, v.device)
            c = getattr(self, "_inv_s_cache", None)
            if c is None or c[0] != key:
                with torch.no_grad():
                    if v.is_cuda and v.dtype == torch.float32:
                        c = (key, nsr_ops.variance_forward(v))                       # one launch, the same bits (ac_variance_forward)
                    else:
                        c = (key, self.deviation_net(torch.zeros([1, 3]))[:, :1].clip(1e-6, 1e6))
                self._inv_s_cache = c
            return c[1]
        return self.deviation_net(torch.zeros([1, 3]))[:, :1].clip(1e-6, 1e6)

    def density(self, x, bound):
        """sdf only (reference :669-681); no-grad queries go through the fused field kernel"""
        if not torch.is_grad_enabled() and x.is_cuda and self._sdf_supported():
            f = self._field() if self._fused_supported() else self._field_sdf_only()
            return nsr_ops.field_sdf(f, x.reshape(-1, 3).float().contiguous(), bound)[:, 0].reshape(x.shape[:-1])
        return self.forward_sdf(x, bound)[..., 0]

    def gradient(self, x, bound, epsilon=0.0005):
        return self.finite_difference_normals_approximator(x, bound, epsilon)

    def finite_difference_normals_approximator(self, x, bound, epsilon=0.0005):
        outs = []
        for k in range(3):
            e = torch.zeros(1, 3, device=x.device); e[0, k] = epsilon
            pos = self.forward_sdf((x + e).clamp(-bound, bound), bound)[:, :1]
            neg = self.forward_sdf((x - e).clamp(-bound, bound), bound)[:, :1]
            outs.append(0.5 * (pos - neg) / epsilon)
        return torch.cat(outs, dim=-1)

    def _grid_axis(self, bound, resolution):
        """torch.linspace(-bound, bound, resolution) as the reference forms it (on the host, fp32: extract_fields :730-732, update_extra_state :312-314), on the
        device.  Cached: the axis of the density grid is asked for once per epoch, the mesh export's once per export."""
        dev = self.encoder.embeddings.device
        key = (float(bound), int(resolution), str(dev))
        c = self.__dict__.setdefault("_axis_cache", {})
        if key not in c:
            if len(c) > 8:
                c.clear()
            c[key] = torch.linspace(-bound, bound, resolution).to(dev)
        return c[key]

    def extract_fields_device(self, bound: float, resolution: int, negate: bool = False, slab_layers=None):
        """the SDF (negate: -SDF) on the resolution^3 grid over [-bound, bound]^3 as a device tensor [res, res, res]: ONE launch (ac_field_sdf_grid) -- the
        kernel forms the grid points from the axis table; no meshgrid / cat tensors, no 256^3 blocks, no host round trip.
        slab_layers is refused: a streamed volume (extract_geometry(slab_layers=...)) is never whole."""
        if slab_layers is not None:
            raise RuntimeError("extract_fields_device: slab_layers is refused here -- a streamed volume is never whole; extract_geometry(slab_layers=...) meshes it slab by slab")
        if not (self.encoder.embeddings.is_cuda and self._sdf_supported()):
            raise RuntimeError("extract_fields_device: needs the default SDF side of NeRFNetwork on the GPU")
        ax = self._grid_axis(bound, resolution)
        with torch.no_grad():
            f = self._field() if self._fused_supported() else self._field_sdf_only()
            return nsr_ops.field_sdf_grid(f, ax, ax, ax, bound, negate=negate)

    def extract_fields(self, bound: float, resolution: int):
        """the SDF on a resolution^3 grid over [-bound, bound]^3 (extract_fields, reference :728-745); returns a float32 numpy array
        [res, res, res] like the reference.  On the GPU: extract_fields_device + one copy to the host."""
        if self.encoder.embeddings.is_cuda and self._sdf_supported():
            return self.extract_fields_device(bound, resolution).cpu().numpy()
        N = 256
        dev = self.encoder.embeddings.device
        xs = torch.linspace(-bound, bound, resolution).split(N)
        u = torch.empty([resolution] * 3, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for xi, x in enumerate(xs):
                for yi, y in enumerate(xs):
                    for zi, z in enumerate(xs):
                        xx, yy, zz = torch.meshgrid(x, y, z, indexing="ij")
                        pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)
                        u[xi * N: xi * N + len(x), yi * N: yi * N + len(y), zi * N: zi * N + len(z)] = self.density(pts, bound).reshape(len(x), len(y), len(z))
        return u.cpu().numpy()

    def extract_geometry(self, bound: float, resolution: int, threshold: int = 0.0, device=None, mesher=None, return_torch=False, slab_layers=None, components=None,
                         decimate=None):
        """iso-surface of the SDF (reference :706-764; its one call is extract_geometry(NSR_BOUND, 512), stylize.py:267): vertices [V,3] float64 in world
        units, triangles [F,3].  The reference runs PyMCubes' marching_cubes on u = -sdf (third party, not in this image).
        mesher: "native" (default on the GPU) = ac_field_sdf_grid + ac_marching_cubes on the device: the volume never leaves it, one shared vertex per
                sign-changing grid edge at the linear zero crossing, the 256-case table of the definition, triangles oriented out of the body; only the
                finished mesh is copied to the host (return_torch=True: not even that -- device tensors);
                "mcubes" = the reference's own call when PyMCubes is installed; "tetra" = the marching-tetrahedra mesher of round 3 (geometry.py:
                the same vertex set, a different triangulation -- kept as the cross-check of the tests).
        slab_layers: None = the whole volume at once (9 bytes per grid point, fewer than 2^31 points: resolution <= 1290); an integer >= 2 = the native mesher
                STREAMED (nsr_ops.marching_cubes_streamed): the grid is evaluated slab_layers x-layers at a time into one window of slab_layers + 2 layers and
                meshed window by window -- the same mesh bit for bit, in the memory of one window, at any resolution whose window stays below 2^31 points
                (extract_geometry(1.6, 2048, slab_layers=64): the hash grid's own finest resolution, 0.92 s).  Multiples of 16 keep the x-tiles of the grid kernel
                full; other values are legal.  Needs mesher "native" (or None on the GPU).
        components: None = every connected component the field has, floaters included (as ever); a spec of geometry.select_components -- "largest",
                ("largest", k), ("min_faces", n), a bool mask or a callable on the size table -- = only those components, labelled and compacted on the device
                (geometry.clean_mesh: order preserved, so the dense and the streamed route give the same cleaned mesh).  Native mesher only.
        decimate: None = every marching-cubes triangle (as ever); a real k >= 1 = the vertices of every cluster cell of k marching-cubes cells merged on the device
                (mesh_decimate.cluster_grid / decimate_mesh: vertex clustering, order preserved, the same from run to run and on the dense and the streamed
                route), AFTER the components are cleaned, so that a floater never merges into the body.  This call has no field pass: with decimate the vertices
                are the clusters' MEAN vertices, near the level set and not on it (at most about one cluster cell off) -- extract_colored_mesh /
                extract_textured_mesh(decimate=k) project them back.  Triangles that lose a corner to a merge are dropped; duplicates are not removed and the
                result need not be manifold.  Native mesher only."""
        native_ok = self.encoder.embeddings.is_cuda and self._sdf_supported()
        if decimate is not None:
            from .mesh_decimate import cluster_grid, decimate_mesh
            if mesher not in (None, "native") or not native_ok:
                raise RuntimeError("extract_geometry(decimate=...) decimates the native mesher's mesh on the device: it needs mesher='native' and the default SDF side of NeRFNetwork on the GPU")
            decimate = cluster_grid(bound, resolution, decimate)                      # (a bad k raises before any device work)
        if components is not None and (mesher not in (None, "native") or not native_ok):
            raise RuntimeError("extract_geometry(components=...) cleans the native mesher's mesh on the device: it needs mesher='native' and the default SDF side of NeRFNetwork on the GPU")
        if slab_layers is not None:
            slab_layers = nsr_ops.check_slab_layers(slab_layers, "extract_geometry")
            if mesher not in (None, "native") or not native_ok:
                raise RuntimeError("extract_geometry(slab_layers=...) streams the native mesher: it needs mesher='native' and the default SDF side of NeRFNetwork on the GPU")
        if mesher is None:
            mesher = "native" if native_ok else "tetra"
        if mesher == "native":
            if not native_ok:
                raise RuntimeError("extract_geometry(mesher='native') needs the default SDF side of NeRFNetwork on the GPU")
            bmin, bmax = np.float32(-bound), np.float32(bound)                       # (the reference's bounds are float32 tensors, :712)
            xf = dict(den=resolution - 1.0, span=[float(bmax - bmin)] * 3, lo=[float(bmin)] * 3)
            if slab_layers is None:
                u = self.extract_fields_device(bound, resolution, negate=True)
                v, t = nsr_ops.marching_cubes(u, float(threshold), **xf)
            else:
                ax = self._grid_axis(bound, resolution)
                with torch.no_grad():
                    f = self._field() if self._fused_supported() else self._field_sdf_only()
                    fill = lambda x0, out: nsr_ops.field_sdf_grid(f, ax[x0:x0 + out.shape[0]], ax, ax, bound, negate=True, out=out)
                    v, t = nsr_ops.marching_cubes_streamed(fill, resolution, resolution, resolution, slab_layers=slab_layers, iso=float(threshold),
                                                           device=ax.device, **xf)
            if components is not None:
                from .geometry import clean_mesh
                m = clean_mesh(dict(vertices=v, triangles=t), components)
                v, t = m["vertices"], m["triangles"]
            if decimate is not None:
                m = decimate_mesh(dict(vertices=v, triangles=t), decimate)
                v, t = m["vertices"], m["triangles"]
            return (v, t) if return_torch else (v.cpu().numpy(), t.cpu().numpy())
        u = -1.0 * self.extract_fields(bound, resolution)
        if mesher == "mcubes":
            import mcubes
            vertices, triangles = mcubes.marching_cubes(u, threshold)
        elif mesher == "tetra":
            from .geometry import marching_tetrahedra
            v, t = marching_tetrahedra(torch.from_numpy(u).to(self.encoder.embeddings.device), float(threshold))
            vertices, triangles = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
        else:
            raise ValueError(f"extract_geometry: unknown mesher {mesher!r}")
        vertices = vertices / (resolution - 1.0) * (2 * bound) - bound
        return vertices, triangles

    def extract_colored_mesh(self, bound: float, resolution: int, threshold: float = 0.0, refine_steps: int = 3, tol: float = 1e-5, colors: bool = True,
                             return_torch=False, slab_layers=None, components=None, decimate=None):
        """the mesh of extract_geometry(mesher="native") with what a viewer wants on it (the reference's save_mesh, stylize.py:263-269, writes bare geometry):
        every vertex projected from the grid edge's linear zero crossing onto the level set sdf = -threshold (at most refine_steps Newton steps along the
        finite-difference gradient, never further than one grid cell), the field's normal and the colour network there -- one launch over the marching-cubes
        buffer (ac_mesh_vertex_attrs).  -> dict(vertices [V,3] float64, triangles [F,3] int32 (extract_geometry's), normals [V,3] float32, colors [V,3]
        float32 in [0, 1] (colors=True), sdf [V] at the final positions, status [V] uint8: 0 converged to tol, 1 all steps taken (sdf tells how close), 2 degenerate gradient,
        3 stopped by the one-cell limit); numpy arrays, or device tensors with return_torch=True.  With view directions the colour is the one seen along -normal.
        colors=True needs the default colour side (RuntimeError otherwise); colors=False works wherever extract_geometry(mesher="native") does.
        slab_layers: extract_geometry's (None: the whole volume at once; an integer: streamed, the same mesh in the memory of one window).
        components: extract_geometry's (None: every component).  The mesh is cleaned right after the geometry and BEFORE the vertices are shaded: a dropped vertex
        costs nothing, and a kept one gets what it would have got (the attributes are per vertex).  The dict then also carries component_sizes [C,2] (vertices,
        triangles of every component of the unfiltered mesh) and components_kept [C] bool.
        decimate: extract_geometry's (None: every triangle; k: clusters of k marching-cubes cells).  The mesh is decimated after the cleaning and BEFORE the
        vertices are shaded: no removed vertex is ever shaded, and every kept one is projected from its cluster's mean onto the level set, never further than one
        CLUSTER cell (k grid cells) instead of one grid cell.  The dict then also carries cluster_members [V] (how many marching-cubes vertices each vertex
        stands for)."""
        if slab_layers is not None:
            slab_layers = nsr_ops.check_slab_layers(slab_layers, "extract_colored_mesh")
        if decimate is not None:
            from .mesh_decimate import cluster_grid, decimate_mesh
            decimate = cluster_grid(bound, resolution, decimate)
        if not (self.encoder.embeddings.is_cuda and self._sdf_supported()):
            raise RuntimeError("extract_colored_mesh needs the default SDF side of NeRFNetwork on the GPU")
        if colors and not self._fused_supported(ignore_curvature=True):
            raise RuntimeError("extract_colored_mesh(colors=True): the colour side of this model is not the default one (colour net 21-64-64-3, or 37-64-64-3 "
                               "with the degree-4 view-direction encoder); colors=False exports positions and normals")
        v, t = self.extract_geometry(bound, resolution, threshold=threshold, mesher="native", return_torch=True, slab_layers=slab_layers)
        cleaned = None
        if components is not None:
            from .geometry import clean_mesh
            cleaned = clean_mesh(dict(vertices=v, triangles=t), components)
            v, t = cleaned["vertices"], cleaned["triangles"]
        max_move, members = 2.0 * bound / (resolution - 1.0), None
        if decimate is not None:
            dm = decimate_mesh(dict(vertices=v, triangles=t), decimate)
            v, t, members, max_move = dm["vertices"], dm["triangles"], dm["cluster_members"], decimate["h"]
        with torch.no_grad():
            f = self._field() if self._fused_supported(ignore_curvature=True) else self._field_sdf_only()
            a = nsr_ops.mesh_vertex_attrs(f, v, bound, nsr_ops.FD_STEP, refine_steps=refine_steps, tol=tol, max_move=max_move,
                                          target_sdf=-float(threshold), want_rgb=colors)
        out = dict(vertices=a["positions"].double(), triangles=t, normals=a["normals"], sdf=a["sdf"], status=a["status"])
        if colors:
            out["colors"] = a["rgb"]
        if cleaned is not None:
            out.update(component_sizes=cleaned["component_sizes"], components_kept=cleaned["components_kept"])
        if members is not None:
            out["cluster_members"] = members
        return out if return_torch else {k: x.cpu().numpy() for k, x in out.items()}

    def render_surface(self, rays_o, rays_d, bound, bg_color=None, normal_epsilon_ratio=0.0, max_ray_batch=None, **opts):
        """the image of the level set itself (ac_render_rays_surface) -- exactly the surface extract_colored_mesh / export_mesh write: per ray the first point with
        sdf = level, the field's normal and colour there, its METRIC distance and a hit mask, about 18 SDF evaluations per ray instead of the volumetric render's
        1008.  Rays as render() takes them ([B,N,3]); opts: level, tol, max_iters, step_scale, min_step, guard of nsr_ops.render_rays_surface, and want_rgb
        (False: no colour network, rgb = None; works wherever extract_colored_mesh(colors=False) does).
        -> dict with render()'s keys that make sense here, in its shapes -- rgb [B,N,3] (background where nothing is hit), depth [B,N] (the distance t along the
        ray, NOT normalised to near/far as run()'s; 0 where nothing is hit), weight_sum [B N,1] (1 or 0), normal [B N,3] -- plus position [B,N,3], sdf [B,N],
        status [B,N] uint8 (as nsr_ops.render_rays_surface; shaded = 0, 1 or 3), iters [B,N] uint8.
        No gradient flows through a root finder's iteration count: the call raises where autograd would record (grad mode on and a parameter that requires grad).
        It does not go through render() / render_route.  Same model requirements as extract_colored_mesh."""
        want_rgb = bool(opts.pop("want_rgb", True))
        if not (self.encoder.embeddings.is_cuda and self._sdf_supported()):
            raise RuntimeError("render_surface needs the default SDF side of NeRFNetwork on the GPU")
        if want_rgb and not self._fused_supported(ignore_curvature=True):
            raise RuntimeError("render_surface: the colour side of this model is not the default one (colour net 21-64-64-3, or 37-64-64-3 with the degree-4 "
                               "view-direction encoder); want_rgb=False renders geometry only")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("render_surface builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()")
        B, N = rays_o.shape[:2]
        n = B * N
        fd_eps = nsr_ops.FD_STEP * (1.0 - normal_epsilon_ratio)
        nsr_ops.surface_opts(bound, fd_eps, **opts)                                   # bad options raise before any device work
        with torch.no_grad():
            ro = rays_o.reshape(-1, 3).float().contiguous()
            rd = rays_d.reshape(-1, 3).float().contiguous()
            bg = None if bg_color is None else _background(bg_color, n, ro.device).contiguous()
            f = self._field() if self._fused_supported(ignore_curvature=True) else self._field_sdf_only()
            step = max(int(max_ray_batch or n), 1)                                    # (None: the whole view in one launch)
            parts = [nsr_ops.render_rays_surface(f, ro[h:h + step], rd[h:h + step], bound, fd_eps, bg=None if bg is None else bg[h:h + step], want_rgb=want_rgb,
                                                 **opts) for h in (range(0, n, step) or (0,))]
            o = parts[0] if len(parts) == 1 else {k: (None if parts[0][k] is None else torch.cat([p[k] for p in parts])) for k in parts[0]}
        return {"rgb": None if o["image"] is None else o["image"].reshape(B, N, 3), "depth": o["depth"].reshape(B, N), "weight_sum": o["weights_sum"][:, None],
                "normal": o["normal_map"], "position": o["position"].reshape(B, N, 3), "sdf": o["sdf"].reshape(B, N), "status": o["status"].reshape(B, N),
                "iters": o["iters"].reshape(B, N)}

    def render_surface_posed(self, rays_o, rays_d, bound, verts, faces, Ts, bg_color=None, max_ray_batch=None, normal_epsilon_ratio=0.0, **opts):
        """render_surface in the pose of one frame (ac_render_rays_surface_warped): per ray the first point of { p : sdf(W^-1(p)) = level } inside the warp's mask
        -- the set the posed volumetric render draws and pose_mesh moves the exported mesh onto -- about a dozen closest-face searches per ray where a posed
        volumetric frame takes 64.  verts [Vg,3], faces [F,3], Ts [>= Vg,4,4]: the frame's posed guide and transforms (calc_local_trans), or verts = an
        nsr_ops.WarpMesh of the frame (faces, Ts unused).  opts: level, tol, max_iters, step_scale, min_step, guard, w_tol of nsr_ops.render_rays_surface_warped,
        and want_rgb.
        -> render_surface's keys and shapes -- rgb [B,N,3], depth [B,N] (the ray parameter of the shaded point; 0 where nothing is hit), weight_sum [B N,1],
        normal [B N,3] (POSED), position [B,N,3] (posed), sdf, status (shaded = 0, 1, 3 or 6; 6 = the mask boundary cuts the body there), iters [B,N] -- plus
        canonical [B,N,3] (the shaded point in canonical space), normal_can [B N,3] and face_id [B,N] int32 (closest guide face, -1 where not shaded).
        Builds no autograd graph: the call raises where autograd would record.  It does not go through render() / render_route."""
        want_rgb = bool(opts.pop("want_rgb", True))
        if not (self.encoder.embeddings.is_cuda and self._sdf_supported()):
            raise RuntimeError("render_surface_posed needs the default SDF side of NeRFNetwork on the GPU")
        if want_rgb and not self._fused_supported(ignore_curvature=True):
            raise RuntimeError("render_surface_posed: the colour side of this model is not the default one (colour net 21-64-64-3, or 37-64-64-3 with the "
                               "degree-4 view-direction encoder); want_rgb=False renders geometry only")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("render_surface_posed builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()")
        B, N = rays_o.shape[:2]
        n = B * N
        fd_eps = nsr_ops.FD_STEP * (1.0 - normal_epsilon_ratio)
        nsr_ops.surface_warped_opts(bound, fd_eps, **opts)                            # bad options raise before any device work
        with torch.no_grad():
            ro = rays_o.reshape(-1, 3).float().contiguous()
            rd = rays_d.reshape(-1, 3).float().contiguous()
            wm = verts if isinstance(verts, nsr_ops.WarpMesh) else nsr_ops.WarpMesh(verts, faces, Ts, ro.device)
            bg = None if bg_color is None else _background(bg_color, n, ro.device).contiguous()
            f = self._field() if self._fused_supported(ignore_curvature=True) else self._field_sdf_only()
            step = max(int(max_ray_batch or n), 1)                                    # (None: the whole view in one call)
            parts = [nsr_ops.render_rays_surface_warped(f, ro[h:h + step], rd[h:h + step], bound, wm, fd_eps, bg=None if bg is None else bg[h:h + step],
                                                        want_rgb=want_rgb, **opts) for h in (range(0, n, step) or (0,))]
            o = parts[0] if len(parts) == 1 else {k: (None if parts[0][k] is None else torch.cat([p[k] for p in parts])) for k in parts[0]}
        return {"rgb": None if o["image"] is None else o["image"].reshape(B, N, 3), "depth": o["depth"].reshape(B, N), "weight_sum": o["weights_sum"][:, None],
                "normal": o["normal_map"], "position": o["position"].reshape(B, N, 3), "sdf": o["sdf"].reshape(B, N), "status": o["status"].reshape(B, N),
                "iters": o["iters"].reshape(B, N), "canonical": o["canonical"].reshape(B, N, 3), "normal_can": o["normal_can"],
                "face_id": o["face_id"].reshape(B, N)}

    def extract_textured_mesh(self, bound: float, resolution: int, texture_size: int = 2048, cell=None, threshold: float = 0.0, refine_steps: int = 3,
                              tol: float = 1e-5, return_torch=False, slab_layers=None, components=None, decimate=None):
        """extract_colored_mesh's mesh with the colour network baked into a texture instead of sampled at the vertices, so that colour detail no longer depends on
        the vertex density: every triangle gets half a cell of a closed-form texture_size^2 atlas (geometry.atlas_layout; cell=None: the largest that fits), every
        owned texel's point on its triangle is projected onto the level set like a vertex (never further than one grid cell) and shaded there, one launch
        (ac_mesh_bake_texture).  -> the dict of extract_colored_mesh plus uv [T,3,2] float64 (three corners per triangle, OBJ convention), texture [S,S,3] uint8
        (q = floor(clamp(x, 0, 1) 255 + 0.5), row 0 on top), owner [S,S] int32 (-1: nobody, texture 0), texel_sdf [S,S], texel_status [S,S] uint8.
        The atlas guarantees bilinear lookups only (no mip chain).  Same model requirements as extract_colored_mesh(colors=True).
        slab_layers: extract_geometry's; an atlas too small for the triangle count of a finer mesh raises as ever.
        components: extract_colored_mesh's.  The mesh is cleaned BEFORE the atlas is laid out, so the cells are sized for the kept triangles only: debris no longer
        lowers the texel density of the body.
        decimate: extract_colored_mesh's.  The mesh is decimated BEFORE the atlas is laid out, so the cells are sized for the decimated triangle count, and the
        texels carry the colour detail the removed vertices carried; a texel's point is projected never further than one CLUSTER cell."""
        from .geometry import atlas_layout
        m = self.extract_colored_mesh(bound, resolution, threshold=threshold, refine_steps=refine_steps, tol=tol, colors=True, return_torch=True,
                                      slab_layers=slab_layers, components=components, decimate=decimate)
        max_move = 2.0 * bound / (resolution - 1.0)
        if decimate is not None:
            from .mesh_decimate import cluster_grid
            max_move = cluster_grid(bound, resolution, decimate)["h"]
        T = m["triangles"].shape[0]
        try:
            lay = atlas_layout(T, texture_size, cell)
        except ValueError as e:
            raise RuntimeError(f"extract_textured_mesh: {e}") from e
        with torch.no_grad():
            b = nsr_ops.mesh_bake_texture(self._field(), m["vertices"].float(), m["triangles"], texture_size, lay["cell"], bound, nsr_ops.FD_STEP,
                                          refine_steps=refine_steps, tol=tol, max_move=max_move, target_sdf=-float(threshold))
            tex = torch.floor(b["rgb"].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
        m.update(texture=tex, owner=b["owner"], texel_sdf=b["sdf"], texel_status=b["status"])
        if not return_torch:
            m = {k: x.cpu().numpy() for k, x in m.items()}
        m["uv"] = torch.from_numpy(lay["uv"]).to(tex.device) if return_torch else lay["uv"]
        return m

    def pose_mesh(self, mesh, body_guide, verts, Ts=None, iters: int = 3, tol: float = 1e-5):
        """the exported mesh in the pose of one frame: the dict of extract_colored_mesh / extract_textured_mesh with its `vertices` moved to where the posed
        renderer draws them -- the p with W^-1(p) = vertex, W^-1 the SMPL-guided inverse warp of the frame (ac_mesh_pose: at most iters fixed-point steps from a
        start bound to the canonical guide, iters + 1 closest-face searches) -- and its `normals` carried along by the blended transform's cofactor matrix.
        body_guide: dict(faces [F,3] of the SMPL guide, and `canonical` [Vg,3], the guide in canonical space; absent: geometry.canonical_guide(verts, Ts), which
        is frame independent, is stored there).  The binding of the mesh to the guide (ac_mesh_bind: once per mesh, pose independent) is stored as
        body_guide["bind"] on the first call and reused: keep one body_guide per exported mesh.
        verts [Vg,3], Ts [>= Vg,4,4]: the frame's posed guide and transforms (calc_local_trans), or verts = an nsr_ops.WarpMesh of the frame (Ts unused).
        -> a shallow copy of `mesh` with vertices (float64, the input's convention), normals, and per vertex residual (float32: max-norm of W^-1(p) - vertex at
        the returned p), status (uint8: 0 within tol, 1 iters used up, 2 not finite) and mask (uint8: 0 = farther from the guide than the renderer's mask
        threshold, where it would draw nothing; kept and flagged); the export's own `status` (of the level-set projection) is replaced: read it from `mesh`.  triangles, uv, texture, colors and every other entry are the input's own objects.
        numpy in, numpy out; device tensors in, device tensors out."""
        from .geometry import canonical_guide
        dev = self.encoder.embeddings.device
        if dev.type != "cuda":
            raise RuntimeError("pose_mesh needs the model on the GPU (there is no CPU path)")
        as_torch = isinstance(mesh["vertices"], torch.Tensor)
        to_dev = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
        wm = verts if isinstance(verts, nsr_ops.WarpMesh) else None
        if "bind" not in body_guide:
            if "canonical" not in body_guide:
                if wm is not None:
                    raise RuntimeError("pose_mesh: body_guide needs `canonical` when the frame arrives as a WarpMesh")
                body_guide["canonical"] = canonical_guide(verts, Ts)
            body_guide["bind"] = nsr_ops.mesh_bind(to_dev(mesh["vertices"], torch.float32), to_dev(body_guide["canonical"], torch.float32),
                                                   to_dev(np.asarray(body_guide["faces"])[:, :3] if not isinstance(body_guide["faces"], torch.Tensor)
                                                          else body_guide["faces"][:, :3], torch.int32))
        if wm is None:
            wm = nsr_ops.WarpMesh(verts, body_guide["faces"], Ts, dev)
        n = mesh.get("normals")
        with torch.no_grad():
            a = nsr_ops.mesh_pose(to_dev(mesh["vertices"], torch.float32), None if n is None else to_dev(n, torch.float32), body_guide["bind"], wm,
                                  iters=iters, tol=tol)
        out = dict(mesh)
        new = dict(vertices=a["positions"].double(), residual=a["residual"], status=a["status"], mask=a["mask"])
        if n is not None:
            new["normals"] = a["normals"]
        out.update(new if as_torch else {k: x.cpu().numpy() for k, x in new.items()})
        return out

    # ------------------------------------------------------------------ occupancy grid of the ray marcher, reference :303-356
    def update_extra_state(self, bound, decay=0.95):
        """density grid for raymarching.march_rays_train / march_rays (only with cuda_ray=True, like the reference): the SDF on the 129^3
        grid -> a logistic density with inv_s = 512 (inv_s * sigmoid'(-|...|) written in two overflow-free branches), dilated by a 2^3 max
        pool, merged into the running grid with max(grid * decay, new); mean density and the step-counter bookkeeping.
        On the GPU the grid update is ONE launch (ac_density_grid_update, csrc/field_grid.hip; the grid is updated in place); the torch chain below
        is the formulation of the reference, kept for the CPU and as the cross-check of the tests (fused_density_grid = False)."""
        if not self.cuda_ray:
            return
        resolution = self.density_grid.shape[0]
        dev = self.density_grid.device
        inv_s = 512.0
        if self.fused_density_grid and self.density_grid.is_cuda and self._sdf_supported():
            with torch.no_grad():
                f = self._field() if self._fused_supported() else self._field_sdf_only()
                if not self.density_grid.is_contiguous():
                    self.density_grid = self.density_grid.contiguous()
                mean = nsr_ops.density_grid_update(f, self._grid_axis(bound, resolution), self.density_grid, bound, inv_s, decay)
        else:
            axes = torch.linspace(-bound, bound, resolution).split(128)
            tmp_grid = torch.zeros_like(self.density_grid)
            with torch.no_grad():
                for xi, xs in enumerate(axes):
                    for yi, ys in enumerate(axes):
                        for zi, zs in enumerate(axes):
                            lx, ly, lz = len(xs), len(ys), len(zs)
                            xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                            pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)
                            sdf = self.density(pts, bound).detach().float().reshape(-1)
                            mask = sdf > 0
                            density = torch.zeros_like(sdf)
                            density[mask] = inv_s * torch.exp(-inv_s * sdf[mask]) / (1 + torch.exp(-inv_s * sdf[mask]))
                            density[~mask] = inv_s * torch.exp(inv_s * sdf[~mask]) / (1 + torch.exp(inv_s * sdf[~mask]))
                            tmp_grid[xi * 128: xi * 128 + lx, yi * 128: yi * 128 + ly, zi * 128: zi * 128 + lz] = density.reshape(lx, ly, lz)
                tmp_grid = F.pad(tmp_grid, (0, 1, 0, 1, 0, 1))
                tmp_grid = F.max_pool3d(tmp_grid.unsqueeze(0).unsqueeze(0), kernel_size=2, stride=1).squeeze(0).squeeze(0)
                self.density_grid = torch.maximum(self.density_grid * decay, tmp_grid)
            mean = torch.mean(self.density_grid)
        # the two scalars the marcher takes as launch constants: ONE read-back for both
        total_step = min(64, self.local_step)
        if total_step > 0:
            both = torch.stack([mean.reshape(()).double(), self.step_counter[:total_step, 0].sum().double()]).tolist()
            self.mean_density = both[0]
            self.mean_count = int(both[1] / total_step)
        else:
            self.mean_density = mean.item()
        self.iter_density += 1
        self.local_step = 0

    fused_density_grid = True
