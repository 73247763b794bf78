"""The launches of the fused renderer (NeRFRenderer.run, reference models/instant_nsr.py:133-299): render_rays / render_rays_long, their pair forms and
the sampling stage alone.  Host-side plumbing only: ac_render_opts / ac_render_out are built from torch CUDA tensors and the kernels enqueued on torch's
current stream; there is no eager fallback."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._args import _F32, _chk, _f32, _inv_s_arg, _ray_args

_LIN_CACHE = {}


def linspace_tables(num_steps, device):
    """lin_z = torch.linspace(0,1,num_steps), lin_u = torch.linspace(0.5/16, 1-0.5/16, 16), made on the
    CPU exactly as the reference makes them (instant_nsr.py:155, :34) and cached on the device."""
    key = (int(num_steps), str(device))
    if key not in _LIN_CACHE:
        lin_z = torch.linspace(0.0, 1.0, num_steps, dtype=_F32)
        lin_u = torch.linspace(0. + 0.5 / 16, 1. - 0.5 / 16, steps=16, dtype=_F32)
        _LIN_CACHE[key] = (lin_z.to(device), lin_u.to(device))
    return _LIN_CACHE[key]


PRECISIONS = {"exact": 0, "fast": 1}
TABLE_DTYPES = ("float", "half")


def check_table_dtype(who, table_dtype, long=False, pair=False, train_extras=False, opacity_only=False):
    """the rules of table_dtype (RuntimeError naming the rule, before any device work): "half" is the fused renderer's inference launch only"""
    if table_dtype not in TABLE_DTYPES:
        raise RuntimeError(f"{who}: table_dtype must be one of {TABLE_DTYPES}, got {table_dtype!r}")
    if table_dtype != "half":
        return
    if long:
        raise RuntimeError(f"{who}: table_dtype='half' is built for the fused renderer's window only (render_rays); the long renderer reads the fp32 table")
    if pair:
        raise RuntimeError(f"{who}: table_dtype='half' is not built for the pair launch (a training step's renders share the fp32 table)")
    if train_extras:
        raise RuntimeError(f"{who}: table_dtype='half' with train_extras: nothing trains from the half table (an inference option)")
    if opacity_only:
        raise RuntimeError(f"{who}: table_dtype='half' with opacity_only is not built (opacity_only serves the frozen avatar of a training step: fp32 table)")


class RenderResult(dict):
    """the tensors a render launch produced (a dict), plus `.opts`: the launch's ac_render_opts and the tensors its pointers refer to"""
    opts = None


def render_rays(field, rays_o, rays_d, num_steps=64, upsample_steps=64, bound=1.6, inv_s=1.0, bg=None, noise=None,
                cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, extras=False, debug_indices=False, out=None, events=None, warp=None,
                train_extras=False, near_far=None, precision="exact", skip_masked=False, opacity_only=False, table_dtype="float"):
    """One launch of the fused renderer for N rays.  Returns a dict of CUDA tensors:
    image[N,3] weights_sum[N] depth[N] normal_map[N,3] eik[N,2] gradient_error[] (+ z_vals, weights,
    alpha, color, sdf, gradient when extras; + ss_inds, sort_index when debug_indices; + sdf_out16 [N,T,16], pts [N,T,3] and
    eik_res = (gradient_error, eikonal denominator) when train_extras: what the render-core backward needs).
    inv_s: a float, or forward_variance() as a CUDA tensor (read on the device).
    near_far = (near [N], far [N]): per-ray sampling range that overrides the cube's where finite (the mesh-guided range of a canonical render).
    precision: "exact" (every product an fp32 fma, bit-identical to the CPU oracle) or "fast" (layer 1 of the six finite-difference
    evaluations as a split-bf16 correction of the centre's; sample positions, indices and sdf unchanged bit for bit; ac_render_opts.precision).
    warp = WarpMesh(...) renders in posed space (run(render_can=False)): + can_mid[N,T,3], mask[N,T] views of the scratch.
    opacity_only: the colour network is not evaluated (image = background over a black body); weights_sum, depth, normal_map, gradient_error unchanged.
    skip_masked (posed space only): tiles of 16 samples that the warp masks out entirely are not evaluated (ac_render_opts.skip_masked): image,
    weights_sum, depth, normal_map, weights and alpha unchanged bit for bit; sdf / color / gradient of skipped samples 0, gradient_error over the
    evaluated samples.
    table_dtype: "float" (default: the field's fp32 table) or "half" (opt-in, inference): the launch gathers from field.half_table() -- 4 bytes per
    entry instead of 8 -- through ac_render_rays_h16 / ac_render_rays_warped_h16; every output is bit-identical to this call on a field whose table is
    table.half().float().  "half" with train_extras or opacity_only raises RuntimeError."""
    check_table_dtype("render_rays", table_dtype, train_extras=train_extras, opacity_only=opacity_only)
    return _render(field, rays_o, rays_d, num_steps=num_steps, upsample_steps=upsample_steps, bound=bound, inv_s=inv_s, bg=bg, noise=noise,
                   cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio, extras=extras, debug_indices=debug_indices, out=out,
                   events=events, warp=warp, train_extras=train_extras, near_far=near_far, precision=precision, skip_masked=skip_masked,
                   opacity_only=opacity_only, long=False, half=table_dtype == "half")


LONG_MAX_SAMPLES = 512


def check_long_counts(num_steps, upsample_steps):
    """the envelope of the long renderer (ac_render_rays_long): RuntimeError naming the rule, before any device work"""
    ns, us = int(num_steps), int(upsample_steps)
    if ns < 2 or us < 0 or us % 16 or ns + us > LONG_MAX_SAMPLES:
        raise RuntimeError(f"render_rays_long: num_steps={ns} upsample_steps={us} unsupported (num_steps >= 2, upsample_steps >= 0 and a multiple "
                           f"of 16, num_steps + upsample_steps <= {LONG_MAX_SAMPLES})")


def check_save_stencil(who, num_steps, upsample_steps):
    """the rule of the long renderer's stencil features (ac_render_out.feat7): one block per tile of 16 samples of a ray"""
    T = int(num_steps) + int(upsample_steps)
    if T % 16:
        raise RuntimeError(f"{who}: save_stencil (feat7) needs num_steps + upsample_steps a multiple of 16, got {int(num_steps)} + {int(upsample_steps)} "
                           f"= {T}; at such a count leave it off: render_core_backward gathers the stencil features again")


def in_short_window(num_steps, upsample_steps):
    """the counts render_rays / sample_rays accept (multiples of 16, 16 <= num_steps <= 64, sum <= 128)"""
    ns, us = int(num_steps), int(upsample_steps)
    return ns % 16 == 0 and us % 16 == 0 and 16 <= ns <= 64 and us >= 0 and ns + us <= 128


def render_rays_long(field, rays_o, rays_d, num_steps=64, upsample_steps=64, bound=1.6, inv_s=1.0, bg=None, noise=None,
                     cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, extras=False, debug_indices=False, out=None, events=None, warp=None,
                     train_extras=False, near_far=None, precision="exact", skip_masked=False, opacity_only=False, table_dtype="float",
                     save_stencil=False):
    """render_rays for any sample count the reference accepts (ac_render_rays_long): num_steps >= 2, upsample_steps >= 0 a multiple of 16, at most
    512 samples per ray.  Same arguments and result dict as render_rays; bit-identical to it where both accept the counts.  train_extras gives
    sdf_out16 / pts; sort_index is [N, nup, T].
    save_stencil (opt-in, with train_extras, canonical space): + feat7, the stencil features render_core_backward otherwise gathers again -- only where 16
    divides num_steps + upsample_steps (RuntimeError naming the rule otherwise; such counts keep re-gathering).  Default: no feat7 in the result.
    opacity_only as in render_rays (canonical space; with a warp it raises).
    warp = WarpMesh(...) renders in posed space (ac_render_rays_long_warped): + can_mid [N,T,3], mask [N,T] views of the scratch as from
    render_rays(warp=...), with skip_masked as there; without a warp skip_masked is rejected (a posed-space option).
    table_dtype: "float" only ("half" raises: the long renderer has no half-table form)."""
    check_table_dtype("render_rays_long", table_dtype, long=True)
    check_long_counts(num_steps, upsample_steps)
    if opacity_only and warp is not None:
        raise RuntimeError("render_rays_long: opacity_only is not supported in posed space (warp=...): a canonical-space option of the long renderer")
    if skip_masked and warp is None:
        raise RuntimeError("render_rays_long: skip_masked is a posed-space option (pass warp=WarpMesh(...))")
    if save_stencil:
        check_save_stencil("render_rays_long", num_steps, upsample_steps)
        if warp is not None or not train_extras:
            raise RuntimeError("render_rays_long: save_stencil keeps the stencil features of a canonical training render (train_extras=True, no warp)")
    return _render(field, rays_o, rays_d, num_steps=num_steps, upsample_steps=upsample_steps, bound=bound, inv_s=inv_s, bg=bg, noise=noise,
                   cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio, extras=extras, debug_indices=debug_indices, out=out,
                   events=events, warp=warp, train_extras=train_extras, near_far=near_far, precision=precision, skip_masked=skip_masked,
                   opacity_only=opacity_only, long=True, save_stencil=bool(save_stencil))


FD_STEP = 0.005                        # finite-difference step of the normals at normal_epsilon_ratio = 0 (instant_nsr.py:687-704)


def _result_bufs(out, dev):
    """-> (res, buf): a launch's result dict (`out` again, or a new one) and buf(name, shape[, dtype]) -> res[name], kept where it fits, else allocated"""
    res = out if out is not None else RenderResult()

    def buf(name, shape, dtype=_F32):
        t = res.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=dev)
            res[name] = t
        return t
    return res, buf


def _render_opts(N, num_steps, upsample_steps, bound, has_noise, inv_s=1.0, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, near_far=None,
                 precision="exact", skip_masked=False, opacity_only=False):
    """-> (ac_render_opts, inv_s on the device or None, near [N] or None, far [N] or None): the struct and the tensors its pointers refer to"""
    inv_s_f, inv_s_t = _inv_s_arg(inv_s)
    nm = fm = None
    if near_far is not None:
        nm, fm = _chk(near_far[0].reshape(-1), "near", (N,)), _chk(near_far[1].reshape(-1), "far", (N,))
    op = L.ac_render_opts(N, int(num_steps), int(upsample_steps), float(bound), inv_s_f, float(cos_anneal_ratio),
                          float(np.float32(FD_STEP * (1.0 - normal_epsilon_ratio))), int(has_noise), L.ptr(inv_s_t), L.ptr(nm), L.ptr(fm),
                          PRECISIONS[precision], int(bool(skip_masked)), int(bool(opacity_only)))
    return op, inv_s_t, nm, fm


# the output buffers of ac_render_out by name, with the shape that follows [rays] (per ray) or [rays, samples] (per sample)
_PER_RAY_OUT = dict(image=(3,), weights_sum=(), depth=(), normal_map=(3,), eik=(2,))
_PER_SAMPLE_OUT = dict(z_vals=(), weights=(), alpha=(), color=(3,), sdf=(), gradient=(3,), sdf_out16=(16,), pts=(3,))
_OUT_TAIL = {**_PER_RAY_OUT, **_PER_SAMPLE_OUT}
_EXTRAS_OUT = ("z_vals", "weights", "alpha", "color", "sdf", "gradient")
_TRAIN_EXTRAS_OUT = ("sdf_out16", "pts")


def _feat7_shape(N, T):
    """ac_render_out.feat7: the hash features of every sample's 7-point stencil, one block per tile of 16 samples (0.9 KB per sample)"""
    return (N * T // 16, 14, 64, 4)


def _fill_out(o, buf, names, lead, prefix=""):
    """o.<name> = buf(prefix + name, lead + the name's trailing shape) for the given per-ray or per-sample names"""
    for k in names:
        setattr(o, k, buf(prefix + k, lead + _OUT_TAIL[k]).data_ptr())


def _render(field, rays_o, rays_d, *, num_steps, upsample_steps, bound, inv_s, bg, noise, cos_anneal_ratio, normal_epsilon_ratio, extras,
            debug_indices, out, events, warp, train_extras, near_far, precision, skip_masked, opacity_only, long, half=False, save_stencil=False):
    rays_o, rays_d = _ray_args(rays_o, rays_d)
    N = rays_o.shape[0]
    dev = rays_o.device
    T = num_steps + upsample_steps
    nup = upsample_steps // 16
    lin_z, lin_u = linspace_tables(num_steps, dev)
    res, buf = _result_bufs(out, dev)
    o = L.ac_render_out()
    _fill_out(o, buf, _PER_RAY_OUT, (N,))
    er = buf("eik_res", (2,))              # (gradient_error, its denominator): reduced by the render launch itself (ac_render_out.eik_reduced)
    o.eik_reduced = er.data_ptr()
    if N == 0:
        er.zero_()
    if extras:
        _fill_out(o, buf, _EXTRAS_OUT, (N, T))
    if train_extras:
        _fill_out(o, buf, _TRAIN_EXTRAS_OUT, (N, T))
        if not long or save_stencil:      # the backward streams the stencil features back instead of gathering them again
            o.feat7 = buf("feat7", _feat7_shape(N, T)).data_ptr()
        else:               # (the long renderer's default: render_core_backward gathers again; a reused result dict must not hand on another launch's)
            res.pop("feat7", None)
    if debug_indices:
        o.ss_inds = buf("ss_inds", (N, max(nup, 1), 16), torch.int32).data_ptr()
        o.sort_index = buf("sort_index", (N, max(nup, 1), T if long else 128), torch.int32).data_ptr()
    if bg is not None:
        bg = _chk(bg.reshape(-1, 3), "bg_color", (N, 3))
    if noise is not None:
        noise = _chk(noise.reshape(N, num_steps), "noise")
    opts = _render_opts(N, num_steps, upsample_steps, bound, noise is not None, inv_s, cos_anneal_ratio, normal_epsilon_ratio, near_far, precision,
                        skip_masked and warp is not None, opacity_only)
    op = opts[0]
    if isinstance(res, RenderResult):
        res.opts = opts
    st = L.current_stream(dev)
    h16 = field.half_table().data_ptr() if half else None          # (converted once per Field; before the events: not part of the render's time)
    if events is not None:          # (start, end) torch.cuda.Event pair around the render kernel only (bench.py roofline)
        events[0].record()
    who = ("render_rays_long" if long else "render_rays") + ("_warped" if warp is not None else "") + ("_h16" if half else "")
    args = (C.byref(field.c),) + ((h16,) if half else ()) + (C.byref(op), rays_o.data_ptr(), rays_d.data_ptr(), L.ptr(bg), L.ptr(noise),
                                                              lin_z.data_ptr(), lin_u.data_ptr())
    if warp is None:
        L.check(getattr(L.lib(), "ac_" + who)(*args, C.byref(o), st), who)
    else:
        offs = (C.c_size_t * 6)()
        nbytes = L.lib().ac_render_rays_warped_scratch(N, T, offs)
        scratch = buf("_warp_scratch", (max(int(nbytes), 1),), torch.uint8)
        L.check(getattr(L.lib(), "ac_" + who)(*args, C.byref(warp.c), scratch.data_ptr(), int(nbytes), C.byref(o), st), who)
        res["can_mid"] = scratch[offs[3]:offs[3] + N * T * 12].view(_F32).view(N, T, 3)
        res["mask"] = scratch[offs[4]:offs[4] + N * T].view(N, T)
        if skip_masked and warp.accel is not None and upsample_steps > 0:      # rays the cell grids proved masked out (never sampled): the scratch's last segment
            tail = (N + 255) & ~255
            res["ray_dead"] = scratch[int(nbytes) - tail:int(nbytes) - tail + N]
        if warp.use_mesh_guide:          # the mesh-guided range the launch sampled in (inf where the ray misses the body): what a backward pass needs
            res["near_m"] = scratch[offs[0]:offs[0] + N * 4].view(_F32)
            res["far_m"] = scratch[offs[1]:offs[1] + N * 4].view(_F32)
    if events is not None:
        events[1].record()
    res["gradient_error"] = er[0]
    return res


def handoff_timeouts(device=None):
    """segment hand-offs of the render launches on the CURRENT stream of `device` that timed out (ac_render_handoff_timeouts): 0 on a healthy run"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = C.c_uint32(0)
    with torch.cuda.device(dev):
        L.check(L.lib().ac_render_handoff_timeouts(L.current_stream(dev), C.addressof(n)), "render_handoff_timeouts")
    return int(n.value)


def render_rays_pair(field, rays_o, rays_d, noise2, num_steps=64, upsample_steps=64, bound=1.6, inv_s=1.0, bg2=None, cos_anneal_ratio=1.0,
                     normal_epsilon_ratio=0.0, precision="exact", out=None, events=None, keep_weights=False, table_dtype="float"):
    """ac_render_rays_pair: the same N rays rendered twice in ONE launch -- copy a with noise2[0] / bg2[0] (per-ray outputs only), copy b with
    noise2[1] / bg2[1] (+ everything the render-core backward needs: the training forward).  Returns (a, b): two RenderResult dicts whose tensors are
    the two halves of shared [2N, ...] buffers; b.opts is the N-ray ac_render_opts the backward takes.  Bit-identical to
    render_rays(..., noise=noise2[0]) and render_rays(..., noise=noise2[1], extras=True, train_extras=True).
    table_dtype: "float" only ("half" raises: the pair launch is a training launch)."""
    check_table_dtype("render_rays_pair", table_dtype, pair=True)
    return _render_pair(field, rays_o, rays_d, noise2=noise2, num_steps=num_steps, upsample_steps=upsample_steps, bound=bound, inv_s=inv_s, bg2=bg2,
                        cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio, precision=precision, out=out, events=events,
                        keep_weights=keep_weights, long=False, save_stencil=True)


def _render_pair(field, rays_o, rays_d, *, noise2, num_steps, upsample_steps, bound, inv_s, bg2, cos_anneal_ratio, normal_epsilon_ratio, precision,
                 out, events, keep_weights, long, save_stencil):
    rays_o, rays_d = _ray_args(rays_o, rays_d)
    N, dev, T = rays_o.shape[0], rays_o.device, num_steps + upsample_steps
    lin_z, lin_u = linspace_tables(num_steps, dev)
    res, buf = _result_bufs(out, dev)
    o = L.ac_render_out()
    _fill_out(o, buf, _PER_RAY_OUT, (2 * N,), prefix="pair_")
    er2 = buf("pair_eik_res", (2, 2))      # per copy: (gradient_error, its denominator), reduced by the launch itself
    o.eik_reduced = er2.data_ptr()
    if N == 0:
        er2.zero_()
    per_sample = ("z_vals", "color", "sdf", "gradient") + _TRAIN_EXTRAS_OUT + (("weights", "alpha") if keep_weights else ())      # what the backward reads
    _fill_out(o, buf, per_sample, (N, T))
    if save_stencil:
        o.feat7 = buf("feat7", _feat7_shape(N, T)).data_ptr()
        per_sample += ("feat7",)
    else:                   # (a reused result dict must not hand on another launch's)
        res.pop("feat7", None)
    noise2 = _chk(noise2.reshape(2 * N, num_steps), "noise2")
    if bg2 is not None:
        bg2 = _chk(bg2.reshape(-1, 3), "bg2", (2 * N, 3))
    opts = _render_opts(N, num_steps, upsample_steps, bound, True, inv_s, cos_anneal_ratio, normal_epsilon_ratio, precision=precision)
    op = opts[0]
    st = L.current_stream(dev)
    if events is not None:
        events[0].record()
    entry, who = (L.lib().ac_render_rays_long_pair, "render_rays_long_pair") if long else (L.lib().ac_render_rays_pair, "render_rays_pair")
    L.check(entry(C.byref(field.c), C.byref(op), rays_o.data_ptr(), rays_d.data_ptr(), L.ptr(bg2), noise2.data_ptr(),
                  lin_z.data_ptr(), lin_u.data_ptr(), C.byref(o), st), who)
    if events is not None:
        events[1].record()
    ra, rb = RenderResult(), RenderResult()
    for k in _PER_RAY_OUT:
        t = res["pair_" + k]
        ra[k], rb[k] = t[:N], t[N:]
    for k in per_sample:
        rb[k] = res[k]
    ra["eik_res"], rb["eik_res"] = er2[0], er2[1]
    ra["gradient_error"], rb["gradient_error"] = er2[0, 0], er2[1, 0]
    rb.opts = ra.opts = opts
    rb._keep = ra._keep = (noise2, bg2, res)
    return ra, rb


def render_rays_long_pair(field, rays_o, rays_d, noise2, num_steps=64, upsample_steps=64, bound=1.6, inv_s=1.0, bg2=None, cos_anneal_ratio=1.0,
                          normal_epsilon_ratio=0.0, precision="exact", out=None, events=None, keep_weights=False, table_dtype="float", save_stencil=False):
    """render_rays_pair at the long renderer's counts (ac_render_rays_long_pair): same arguments, same (a, b) result; bit-identical to
    render_rays_long(..., noise=noise2[0]) and render_rays_long(..., noise=noise2[1], extras=True, train_extras=True, save_stencil=...).
    save_stencil as in render_rays_long: True keeps copy b's feat7 and raises where 16 does not divide num_steps + upsample_steps; default: no feat7.
    table_dtype: "float" only."""
    check_table_dtype("render_rays_long_pair", table_dtype, long=True, pair=True)
    check_long_counts(num_steps, upsample_steps)
    if save_stencil:
        check_save_stencil("render_rays_long_pair", num_steps, upsample_steps)
    return _render_pair(field, rays_o, rays_d, noise2=noise2, num_steps=num_steps, upsample_steps=upsample_steps, bound=bound, inv_s=inv_s, bg2=bg2,
                        cos_anneal_ratio=cos_anneal_ratio, normal_epsilon_ratio=normal_epsilon_ratio, precision=precision, out=out, events=events,
                        keep_weights=keep_weights, long=True, save_stencil=bool(save_stencil))


def sample_rays(field, rays_o, rays_d, num_steps=64, upsample_steps=64, bound=1.6, noise=None, near_far=None):
    """the no-grad sampling stage of run() only -> z_vals [N, num_steps + upsample_steps] (identical to render_rays' z_vals)"""
    return _sample(field, rays_o, rays_d, num_steps=num_steps, upsample_steps=upsample_steps, bound=bound, noise=noise, near_far=near_far, long=False)


def sample_rays_long(field, rays_o, rays_d, num_steps=64, upsample_steps=64, bound=1.6, noise=None, near_far=None):
    """sample_rays for any count render_rays_long accepts (ac_sample_rays_long) -> z_vals [N, num_steps + upsample_steps], identical to
    render_rays_long's z_vals (and to sample_rays' where both accept the counts)"""
    check_long_counts(num_steps, upsample_steps)
    return _sample(field, rays_o, rays_d, num_steps=num_steps, upsample_steps=upsample_steps, bound=bound, noise=noise, near_far=near_far, long=True)


def _sample(field, rays_o, rays_d, *, num_steps, upsample_steps, bound, noise, near_far, long):
    rays_o, rays_d = _ray_args(rays_o, rays_d)
    N, dev = rays_o.shape[0], rays_o.device
    lin_z, lin_u = linspace_tables(num_steps, dev)
    if noise is not None:
        noise = _chk(noise.reshape(N, num_steps), "noise")
    z = _f32(dev, N, num_steps + upsample_steps)
    op, _, nm, fm = _render_opts(N, num_steps, upsample_steps, bound, noise is not None, near_far=near_far)
    name = "sample_rays_long" if long else "sample_rays"
    L.check(getattr(L.lib(), "ac_" + name)(C.byref(field.c), C.byref(op), rays_o.data_ptr(), rays_d.data_ptr(), L.ptr(noise), lin_z.data_ptr(),
                                           lin_u.data_ptr(), z.data_ptr(), L.current_stream(dev)), name)
    return z
