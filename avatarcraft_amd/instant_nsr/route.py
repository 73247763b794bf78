"""Which nsr_ops entry a render of NeRFRenderer launches.  Pure: no tensor, no device (DESIGN.md section 5.10 lists the outcomes)."""
import collections

from .. import nsr_ops

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
