"""The training operators: the render core under autograd and from its saved state (ac_render_core_backward), weight norm of all layers as one
operator, and the operators of the step's glue (packed shading, SDF stencil, colour MLP, compositing), each a fused launch each way."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .._scratch import ScratchCache
from ._args import _F32, _dc, _f32
from .field import (COLOR_PARAM_GRADS_LEN, PG_WEIGHT_NORM, SDF_PARAM_GRADS_LEN, Field, join_viewdir_grad, param_grads, sh_bias, split_color_param_grads,
                    split_sdf_param_grads, split_viewdir_weight, weight_norm_forward)
from .render import render_rays

_CORE_SCRATCH = ScratchCache()


def core_scratch(field, N, T, dev):
    """device scratch of ac_render_core_backward, one buffer per (device, stream): grown to the largest batch seen, never shrunk
    (free_scratch() releases it).  Keyed by stream so that two streams never share queues.  -> (buffer, bytes needed); a batch of no rays that finds
    nothing cached gets an empty tensor (its data_ptr() is NULL), never None"""
    need = int(L.lib().ac_render_core_backward_scratch(C.byref(field.c), int(N), int(T)))
    buf = _CORE_SCRATCH.get((str(dev), int(L.current_stream(dev) or 0)), need, dev)
    return (buf if buf is not None else torch.empty(0, dtype=torch.uint8, device=dev)), need


def free_scratch():
    """drop the cached scratch of the render-core backward and of the hash encoder back end (multi-GB queues of the table-gradient scatter).  The small
    buffers of the occupancy renderers (they carry the barrier-failure counts) and of the density-grid update are not touched."""
    _CORE_SCRATCH.clear()
    from ..encoder.hashencoder import backend as BK
    BK.free_scratch()


class _RenderCore(torch.autograd.Function):
    """NeRFRenderer.run with gradients (reference models/instant_nsr.py:133-299 under torch.enable_grad) as ONE operator:
    forward  = the fused renderer itself (ac_render_rays: sampling + render core, the launch an inference render makes) with its
               per-sample outputs kept;
    backward = ac_render_core_backward: compositing -> colour MLP -> normal normalisation + eikonal -> SDF query -> table scatter.
    Differentiable w.r.t. the hash table, the EFFECTIVE MLP matrices (weight norm stays in torch) and inv_s; the sample positions
    are constants, as in the reference (they are computed under no_grad, :176-184)."""

    @staticmethod
    def forward(ctx, table, W1, b1, W2, b2, Wc1, Wc2, Wc3, inv_s, rays_o, rays_d, bg, noise, cfg):
        offsets, pls, H, T0, up, bound, car, ner, precision, warp = cfg
        ctx.set_materialize_grads(False)              # an output the loss does not use arrives as None -> a NULL upstream pointer
        Wc1_21, Wc1_sh = split_viewdir_weight(_dc(Wc1))           # use_viewdirs: [64,37] -> the 21 per-sample columns + the 16 view-direction columns
        field = Field(_dc(table), offsets, pls, H, _dc(W1), _dc(b1), _dc(W2), _dc(b2), Wc1_21, _dc(Wc2), _dc(Wc3), Wc1_sh=Wc1_sh).prepare()
        # warp = WarpMesh: posed space (run(render_can=False), instant_nsr.py:166-172,198-207,246-249) -- the launch sequence of an inference render
        # (sampling, SMPL inverse warp, final pass; every sample evaluated: skip_masked off) with the per-sample outputs kept.  The warped points,
        # the mask and the mesh-guided range are constants of the differentiation, as in the reference (the warp is numpy there).
        out = render_rays(field, rays_o, rays_d, T0, up, bound, inv_s, bg=bg, noise=noise, cos_anneal_ratio=car, normal_epsilon_ratio=ner,
                          extras=True, train_extras=True, precision=precision, warp=warp)
        ctx.field, ctx.cfg = field, cfg
        ctx.opts = out.opts                                        # the launch's ac_render_opts (+ the tensors its pointers refer to)
        ctx.posed = None
        if warp is not None:
            op_b = type(out.opts[0]).from_buffer_copy(out.opts[0])  # the backward's options: + the range the forward computed for itself
            if "near_m" in out:
                op_b.near_m, op_b.far_m = out["near_m"].data_ptr(), out["far_m"].data_ptr()
            ctx.opts = (op_b,) + tuple(out.opts[1:])
            ctx.posed = (out["mask"], out.get("near_m"), out.get("far_m"), out["_warp_scratch"], warp)
        ctx.has_bg = bg is not None
        # outputs among the saved tensors (z_vals, color) must go through save_for_backward (no reference cycle through ctx)
        ctx.save_for_backward(out["z_vals"], out["pts"], out["sdf"], out["sdf_out16"], out["gradient"], out["color"], out["eik_res"], rays_o, rays_d,
                              bg if bg is not None else rays_o, out["feat7"] if "feat7" in out else rays_o)
        ctx.has_feat = "feat7" in out
        ctx.table = table
        ctx.inv_s_shape = inv_s.shape
        ctx.mark_non_differentiable(out["weights"], out["alpha"], out["color"], out["z_vals"])
        return (out["image"], out["weights_sum"], out["depth"], out["normal_map"], out["eik_res"][0], out["weights"], out["alpha"], out["color"],
                out["z_vals"])

    @staticmethod
    def backward(ctx, g_image, g_wsum, g_depth, g_nmap, g_eik, *_unused):
        field = ctx.field
        z_vals, pts, sdf, sdf16, gradient, color, eik_res, rays_o, rays_d, bg, feat7 = ctx.saved_tensors
        if not ctx.has_bg:
            bg = None
        # The table gradient is RETURNED to autograd like every other gradient (torch.autograd.grad, backward(inputs=...), hooks and DDP-style
        # reducers see it); the step without autograd accumulates into its own buffer instead (render_core_backward's g_table).
        g_table = torch.zeros_like(ctx.table)                      # accumulated into, like hash_encode_backward (hashgrid.py:61-68)
        saved = (z_vals, pts, sdf, sdf16, gradient, color, eik_res[1:], feat7 if ctx.has_feat else None, ctx.posed[0] if ctx.posed else None)
        g_sdf_p, g_col_p, g_invs, g_sh = _core_backward(field, ctx.opts[0], saved, rays_o, rays_d, bg, (g_image, g_wsum, g_depth, g_nmap, g_eik), g_table)
        g_Wc1, g_Wc2, g_Wc3 = split_color_param_grads(g_col_p)
        if g_sh is not None:
            g_Wc1 = join_viewdir_grad(g_Wc1, g_sh)
        return (g_table, *split_sdf_param_grads(g_sdf_p), g_Wc1, g_Wc2, g_Wc3,
                g_invs.sum().reshape(ctx.inv_s_shape), None, None, None, None, None)


def render_core(table, W1, b1, W2, b2, Wc1, Wc2, Wc3, inv_s, rays_o, rays_d, bg, noise, offsets, per_level_scale, base_resolution, num_steps,
                upsample_steps, bound, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, precision="exact", warp=None):
    """-> image [N,3], weights_sum [N], depth [N], normal_map [N,3], gradient_error [], weights [N,T], alpha [N,T], color [N,T,3], z_vals [N,T]
    warp = WarpMesh(...): the posed-space render (run(render_can=False)) under autograd."""
    cfg = ([int(v) for v in offsets], per_level_scale, int(base_resolution), int(num_steps), int(upsample_steps), float(bound),
           float(cos_anneal_ratio), float(normal_epsilon_ratio), precision, warp)
    return _RenderCore.apply(table, W1, b1, W2, b2, Wc1, Wc2, Wc3, inv_s, rays_o, rays_d, bg, noise, cfg)


class _WeightNormAll(torch.autograd.Function):
    """torch.nn.utils.weight_norm (dim 0) of several layers as ONE operator: forward = ac_weight_norm_forward, backward = ac_param_grads -- the same
    effective matrices, bit for bit, for every path that renders a NeRFNetwork (inference, the training operators, the step without autograd)."""

    @staticmethod
    def forward(ctx, *vg):
        pairs = [(vg[2 * i].detach().contiguous(), vg[2 * i + 1].detach().contiguous()) for i in range(len(vg) // 2)]
        outs = [torch.empty_like(v) for v, _ in pairs]
        weight_norm_forward(pairs, outs)
        ctx.save_for_backward(*vg)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gw):
        vg = ctx.saved_tensors
        dev = vg[0].device
        flat = torch.zeros(sum(t.numel() for t in vg), dtype=_F32, device=dev)
        res, entries, off = [], [], 0
        for i in range(len(vg) // 2):
            v, g = vg[2 * i].detach().contiguous(), vg[2 * i + 1].detach().contiguous()
            gv = flat[off:off + v.numel()].view_as(v); off += v.numel()
            gg = flat[off:off + g.numel()].view_as(g); off += g.numel()
            if gw[i] is None:
                res += [None, None]
                continue
            gwi = gw[i].contiguous().to(_F32)
            entries.append((PG_WEIGHT_NORM, gwi, gwi.shape[1], v.shape[0], v.shape[1], v, g, gv, gg.reshape(-1)))
            res += [gv, gg]
        if entries:
            param_grads(entries, dev)
        return tuple(res)


def weight_norm_all(layers):
    """[W_l = weight_norm(l.weight_v, l.weight_g)] for the given nn.Linear-like modules, differentiable, one launch each way"""
    args = [t for l in layers for t in (l.weight_v, l.weight_g)]
    return list(_WeightNormAll.apply(*args))


def sds_upstream(weights_sum, weights_sum_gt, scale, want_grad=True):
    """opacity term of the stylisation loss: -> (d loss / d weights_sum [N] or None, loss [1]); loss = sum smooth_l1(clamp, clamp) * scale"""
    ws, wg = weights_sum.reshape(-1).contiguous(), weights_sum_gt.reshape(-1).contiguous()
    N, dev = ws.shape[0], ws.device
    g, loss = _f32(dev, N) if want_grad else None, _f32(dev, 1)
    L.check(L.lib().ac_sds_upstream(ws.data_ptr(), wg.data_ptr(), N, float(scale), L.ptr(g), loss.data_ptr(), L.current_stream(dev)), "sds_upstream")
    return g, loss


def _viewdir_args(field, rays_d, N, T, sv, gr):
    """a field with view directions: fill ac_core_saved.sh_bias / ac_core_grads.g_sh_tiles; returns what viewdir_weight_grad needs (None otherwise)"""
    if not getattr(field, "has_viewdirs", False):
        return None
    bias, sh = sh_bias(field, rays_d)
    tiles = _f32(rays_d.device, N * T // 16, 64)
    sv.sh_bias, gr.g_sh_tiles = bias.data_ptr(), tiles.data_ptr()
    return bias, sh, tiles


def _viewdir_weight_grad(vd, N, T):
    """d Wc1_sh [64,16] = sum over rays of (the ray's T / 16 tile rows of g_sh_tiles, summed) (x) sh(d_ray)"""
    if vd is None:
        return None
    _, sh, tiles = vd
    return tiles.view(N, T // 16, 64).sum(1).t().matmul(sh)


def eikonal_groups(eik, group_rays):
    """gradient_error (instant_nsr.py:266-272) per group of `group_rays` consecutive rays of a launch, from its per-ray partial sums eik [N,2]
    (ac_render_out.eik): [groups, 2] = (error, denominator), each by ac_eikonal_reduce2 -- the bits a launch of that group alone reports as eik_res"""
    N = eik.shape[0]
    G = (N + group_rays - 1) // group_rays
    res = _f32(eik.device, G, 2)
    st = L.current_stream(eik.device)
    for k in range(G):
        sl = eik[k * group_rays:(k + 1) * group_rays]
        L.check(L.lib().ac_eikonal_reduce2(sl.data_ptr(), sl.shape[0], res[k].data_ptr(), st), "eikonal_reduce2")
    return res


def render_core_backward(field, opts, out, rays_o, rays_d, bg, g_image, g_wsum, g_depth, g_nmap, g_eik, g_table, split=None, eik_groups=None):
    """ac_render_core_backward on the outputs of a render_rays(..., train_extras=True) launch (`out`, its .opts): the table gradient is accumulated
    into g_table; returns (g_sdf_params [SDF_PARAM_GRADS_LEN], g_color_params [COLOR_PARAM_GRADS_LEN], g_inv_s_per_ray [N][, g_Wc1_sh [64,16] for a field with view directions]) w.r.t. the
    EFFECTIVE matrices.
    split = (level, torch.cuda.Stream): the scatter completes the table gradient of levels >= level first and orders that stream behind exactly that
    (ac_core_grads.side_stream / split_level): work enqueued there afterwards (the all-reduce of that slice) overlaps the rest of the backward."""
    # eik_groups = (group_rays, res [G,2] from eikonal_groups): the launch holds G patches whose eikonal terms are separate ratios; g_eik is then [G]
    if eik_groups is not None and g_eik is not None and g_eik.numel() != eik_groups[1].shape[0]:
        raise RuntimeError("render_core_backward: one g_eik per group of rays")
    saved = (out["z_vals"], out["pts"], out["sdf"], out["sdf_out16"], out["gradient"], out["color"],
             out["eik_res"][1:] if eik_groups is None else eik_groups[1][:, 1:], out.get("feat7") if hasattr(out, "get") else None, None)
    g = _core_backward(field, opts[0], saved, rays_o, rays_d, bg, (g_image, g_wsum, g_depth, g_nmap, g_eik), g_table, split=split,
                       eik_group_rays=None if eik_groups is None else eik_groups[0])
    return g if g[3] is not None else g[:3]                                            # (+ d Wc1_sh [64,16] for a field with view directions)


def _core_backward(field, op, saved, rays_o, rays_d, bg, upstream, g_table, split=None, eik_group_rays=None):
    """THE ac_render_core_backward call.  saved = the forward's (z_vals, pts, sdf, sdf_out16, gradient, color, eikonal denominator(s), feat7 | None, posed
    mask | None); upstream = (g_image, g_wsum, g_depth, g_nmap, g_eik), tensors or None; eik_group_rays: patches of that many rays with one eikonal ratio
    each.  The table gradient is accumulated into g_table.  -> (g_sdf_params, g_color_params, g_inv_s_per_ray, g_Wc1_sh | None), as render_core_backward."""
    N, T = saved[0].shape
    dev = rays_o.device
    g_sdf_p, g_col_p, g_invs = _f32(dev, SDF_PARAM_GRADS_LEN), _f32(dev, COLOR_PARAM_GRADS_LEN), _f32(dev, N)
    sv = L.ac_core_saved(*[L.ptr(t) for t in saved])
    upstream = [None if g is None else g.contiguous().to(_F32) for g in upstream]        # (held until the launch is enqueued)
    upg = L.ac_core_upstream(*[L.ptr(g) for g in upstream], 0, 0)
    if eik_group_rays is not None:
        upg.eik_group_rays, upg.eik_den_stride = int(eik_group_rays), 2
    gr = L.ac_core_grads(g_table.data_ptr(), g_sdf_p.data_ptr(), g_col_p.data_ptr(), g_invs.data_ptr())
    if split is not None:
        gr.split_level, gr.side_stream = int(split[0]), int(split[1].cuda_stream)
    scratch, need = core_scratch(field, N, T, dev)
    vd = _viewdir_args(field, rays_d, N, T, sv, gr)
    L.check(L.lib().ac_render_core_backward(C.byref(field.c), C.byref(op), rays_o.data_ptr(), rays_d.data_ptr(), L.ptr(bg), C.byref(sv), C.byref(upg),
                                            C.byref(gr), scratch.data_ptr(), need, L.current_stream(dev)), "render_core_backward")
    return g_sdf_p, g_col_p, g_invs, _viewdir_weight_grad(vd, N, T)


class _PackedShading(torch.autograd.Function):
    """normal, cos-annealed NeuS alpha and the two per-sample eikonal terms of PACKED samples (ac_packed_shading_forward / _backward): the glue of
    NeRFRenderer.run_cuda's train() branch between the fused SDF query and the packed compositor, one launch each way.
    (sdf_out16 [M,16], gradient [M,3], inv_s) carry gradients; xyzs, dirs, deltas, n_valid (device int32) do not."""

    @staticmethod
    def forward(ctx, sdf16, gradient, inv_s, xyzs, dirs, deltas, n_valid, car):
        sdf16, gradient, xyzs, dirs, deltas = (t.contiguous() for t in (sdf16, gradient, xyzs, dirs, deltas))
        M, dev = sdf16.shape[0], sdf16.device
        stride = 1 if deltas.dim() == 1 else int(deltas.shape[1])
        inv_t = inv_s.detach().reshape(1).to(_F32).contiguous()
        nv = n_valid.detach().reshape(1).to(torch.int32).contiguous()
        alpha, normal, eik = _f32(dev, M), _f32(dev, M, 3), _f32(dev, M, 2)
        L.check(L.lib().ac_packed_shading_forward(sdf16.data_ptr(), gradient.data_ptr(), xyzs.data_ptr(), dirs.data_ptr(), deltas.data_ptr(), stride, M, nv.data_ptr(),
                                                  0.0, inv_t.data_ptr(), float(car), alpha.data_ptr(), normal.data_ptr(), eik.data_ptr(), L.current_stream(dev)),
                "packed_shading_forward")
        ctx.save_for_backward(sdf16, gradient, xyzs, dirs, deltas, inv_t, nv)
        ctx.meta = (stride, float(car), inv_s.shape)
        return alpha, normal, eik

    @staticmethod
    def backward(ctx, g_alpha, g_normal, g_eik):
        sdf16, gradient, xyzs, dirs, deltas, inv_t, nv = ctx.saved_tensors
        stride, car, inv_shape = ctx.meta
        M, dev = sdf16.shape[0], sdf16.device
        c = lambda g: None if g is None else g.contiguous().to(_F32)
        g_alpha, g_normal, g_eik = c(g_alpha), c(g_normal), c(g_eik)
        g_sdf16, g_grad, g_rows = _f32(dev, M, 16, zero=True), _f32(dev, M, 3), _f32(dev, M)
        L.check(L.lib().ac_packed_shading_backward(sdf16.data_ptr(), gradient.data_ptr(), xyzs.data_ptr(), dirs.data_ptr(), deltas.data_ptr(), stride, M, nv.data_ptr(),
                                                   0.0, inv_t.data_ptr(), car, L.ptr(g_alpha), L.ptr(g_normal), L.ptr(g_eik), g_sdf16.data_ptr(), g_grad.data_ptr(),
                                                   g_rows.data_ptr(), L.current_stream(dev)), "packed_shading_backward")
        return g_sdf16, g_grad, g_rows.sum().reshape(inv_shape), None, None, None, None, None


def packed_shading(sdf16, gradient, inv_s, xyzs, dirs, deltas, n_valid, cos_anneal_ratio=1.0):
    """-> (alpha [M], normal [M,3], eik [M,2] = (relax (|g| - 1)^2, relax)); see _PackedShading"""
    return _PackedShading.apply(sdf16, gradient, inv_s, xyzs, dirs, deltas, n_valid, float(cos_anneal_ratio))


class _SdfStencil(torch.autograd.Function):
    """forward_sdf(x) + finite_difference_normals_approximator(x) of the render core as one fused op with a fused backward
    (csrc/sdf_stencil_train.hip).  Inputs: x [B,3], the hash table, the EFFECTIVE sdf_net matrices (weight norm stays in torch).
    x may require grad (the curvature term's perturbed points, models/instant_nsr.py:276-288: positions that are a function of the normal): the backward then
    also returns d loss / d x = the share through the MLP's own xyz inputs (ac_sdf_stencil_backward_inputs) + the share through the encodings (the
    reference's dy_dx path, hashencoder.cu:177-220,311-337: ac_hash_stencil_input_backward)."""

    @staticmethod
    def forward(ctx, x, table, W1, b1, W2, b2, cfg):
        offsets, pls, H, bound, eps = cfg
        x = x.contiguous()
        dev = x.device
        field = Field.sdf_only(_dc(table), offsets, pls, H, _dc(W1), _dc(b1), _dc(W2), _dc(b2))
        B = x.shape[0]
        out16, grad = _f32(dev, B, 16), _f32(dev, B, 3)
        L.check(L.lib().ac_sdf_stencil_forward(C.byref(field.c), x.data_ptr(), B, float(bound), float(eps), out16.data_ptr(), grad.data_ptr(),
                                               L.current_stream(dev)), "sdf_stencil_forward")
        ctx.save_for_backward(x, table, W1, b1, W2, b2)
        ctx.field, ctx.cfg = field, cfg
        return out16, grad

    @staticmethod
    def backward(ctx, g_out, g_grad):
        x, table = ctx.saved_tensors[:2]                # (unpacking them all: autograd's check for a parameter modified in place since the forward)
        field = ctx.field
        offsets, pls, H, bound, eps = ctx.cfg
        dev = x.device
        B = x.shape[0]
        g_out = g_out.contiguous().float(); g_grad = g_grad.contiguous().float()
        gfeat = _f32(dev, 7, 16, B, 2)
        gparams = _f32(dev, SDF_PARAM_GRADS_LEN)
        nbytes = int(L.lib().ac_sdf_stencil_backward_scratch(B))
        scratch = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        st = L.current_stream(dev)
        oh = np.asarray(offsets, dtype=np.int32)
        g_x = None
        if ctx.needs_input_grad[0]:
            g_x = _f32(dev, B, 3)
            L.check(L.lib().ac_sdf_stencil_backward_inputs(C.byref(field.c), x.data_ptr(), g_out.data_ptr(), g_grad.data_ptr(), B, float(bound), float(eps),
                                                           gfeat.data_ptr(), gparams.data_ptr(), g_x.data_ptr(), scratch.data_ptr(), nbytes, st),
                    "sdf_stencil_backward_inputs")
            part = _f32(dev, (16 + 3) // 4, B, 3)
            L.check(L.lib().ac_hash_stencil_input_backward(gfeat.data_ptr(), x.data_ptr(), field.t["table"].data_ptr(), oh.ctypes.data, part.data_ptr(), B, 2, 16,
                                                           field.S, H, float(eps), float(bound), st), "hash_stencil_input_backward")
            g_x = g_x + part.sum(0)
        else:
            L.check(L.lib().ac_sdf_stencil_backward(C.byref(field.c), x.data_ptr(), g_out.data_ptr(), g_grad.data_ptr(), B, float(bound), float(eps),
                                                    gfeat.data_ptr(), gparams.data_ptr(), scratch.data_ptr(), nbytes, st), "sdf_stencil_backward")
        g_table = torch.zeros_like(table)
        from ..encoder.hashencoder.backend import stencil_scratch
        hs, hbytes = stencil_scratch(oh, 16, field.S, H, dev, B)
        L.check(L.lib().ac_hash_stencil_backward(gfeat.data_ptr(), x.data_ptr(), oh.ctypes.data, g_table.data_ptr(), B, 2, 16, field.S, H, float(eps),
                                                 float(bound), L.ptr(hs), hbytes, st), "hash_stencil_backward")
        g_W1, g_b1, g_W2, g_b2 = split_sdf_param_grads(gparams)
        return g_x, g_table, g_W1.contiguous(), g_b1.contiguous(), g_W2, g_b2, None


class _ColorMlp(torch.autograd.Function):
    """forward_color of the render core (use_viewdirs = False) as a fused op with a fused backward (csrc/color_train.hip).
    Inputs: x [B,3] (no grad), normal [B,3], sdf_out [B,16] (column 0 unused), the EFFECTIVE colour matrices."""

    @staticmethod
    def forward(ctx, x, normal, sdf_out, Wc1, Wc2, Wc3):
        x, normal, sdf_out = x.contiguous(), normal.contiguous(), sdf_out.contiguous()
        B, dev = x.shape[0], x.device
        field = Field.color_only(_dc(Wc1), _dc(Wc2), _dc(Wc3))
        rgb = _f32(dev, B, 3)
        L.check(L.lib().ac_color_forward(C.byref(field.c), x.data_ptr(), normal.data_ptr(), sdf_out.data_ptr(), B, rgb.data_ptr(), L.current_stream(dev)),
                "color_forward")
        ctx.save_for_backward(x, normal, sdf_out, Wc1, Wc2, Wc3)
        ctx.field = field
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        x, normal, sdf_out = ctx.saved_tensors[:3]      # (unpacking them all: autograd's check for a parameter modified in place since the forward)
        field = ctx.field
        B, dev = x.shape[0], x.device
        g_rgb = g_rgb.contiguous().float()
        g_n, g_s, gp = _f32(dev, B, 3), _f32(dev, B, 16), _f32(dev, COLOR_PARAM_GRADS_LEN)
        nbytes = int(L.lib().ac_color_backward_scratch(B))
        scratch = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        L.check(L.lib().ac_color_backward(C.byref(field.c), x.data_ptr(), normal.data_ptr(), sdf_out.data_ptr(), g_rgb.data_ptr(), B, g_n.data_ptr(),
                                          g_s.data_ptr(), gp.data_ptr(), scratch.data_ptr(), nbytes, L.current_stream(dev)), "color_backward")
        g_Wc1, g_Wc2, g_Wc3 = split_color_param_grads(gp)
        return None, g_n, g_s, g_Wc1.contiguous(), g_Wc2, g_Wc3.contiguous()


def color_mlp(x, normal, sdf_out, Wc1, Wc2, Wc3):
    """-> rgb [B,3]; differentiable w.r.t. normal, sdf_out[:, 1:], Wc1, Wc2, Wc3"""
    return _ColorMlp.apply(x, normal, sdf_out, Wc1, Wc2, Wc3)


class _Composite(torch.autograd.Function):
    """NeuS alpha + compositing of the render core as one fused op each way (csrc/composite.hip)"""

    @staticmethod
    def forward(ctx, z_vals, sdf, normal, color, inv_s, rays_o, rays_d, bg, num_steps, bound, car):
        N, T = z_vals.shape
        dev = z_vals.device
        z_vals, sdf, normal, color = z_vals.contiguous(), sdf.contiguous(), normal.contiguous(), color.contiguous()
        image, wsum, depth, nmap, weights, alpha = (_f32(dev, *sh) for sh in ((N, 3), (N,), (N,), (N, 3), (N, T), (N, T)))
        s = float(inv_s.detach().reshape(-1)[0])
        L.check(L.lib().ac_composite_forward(rays_o.data_ptr(), rays_d.data_ptr(), z_vals.data_ptr(), sdf.data_ptr(), normal.data_ptr(), color.data_ptr(),
                                             L.ptr(bg), N, int(num_steps), T, float(bound), s, float(car), image.data_ptr(), wsum.data_ptr(),
                                             depth.data_ptr(), nmap.data_ptr(), weights.data_ptr(), alpha.data_ptr(), L.current_stream(dev)),
                "composite_forward")
        ctx.save_for_backward(z_vals, sdf, normal, color, inv_s, rays_o, rays_d, bg if bg is not None else torch.empty(0, device=dev))
        ctx.cfg = (int(num_steps), float(bound), float(car), s, bg is not None)
        ctx.mark_non_differentiable(weights, alpha)
        return image, wsum, depth, nmap, weights, alpha

    @staticmethod
    def backward(ctx, g_image, g_wsum, g_depth, g_nmap, _gw, _ga):
        z_vals, sdf, normal, color, inv_s, rays_o, rays_d, bg = ctx.saved_tensors
        num_steps, bound, car, s, has_bg = ctx.cfg
        N, T = z_vals.shape
        dev = z_vals.device
        c = lambda g, *shape: (g.contiguous().float() if g is not None else _f32(dev, *shape, zero=True))
        g_image, g_wsum, g_depth, g_nmap = c(g_image, N, 3), c(g_wsum, N), c(g_depth, N), c(g_nmap, N, 3)
        g_sdf, g_nrm, g_col, g_s = (_f32(dev, *sh) for sh in ((N, T), (N, T, 3), (N, T, 3), (N,)))
        L.check(L.lib().ac_composite_backward(rays_o.data_ptr(), rays_d.data_ptr(), z_vals.data_ptr(), sdf.data_ptr(), normal.data_ptr(), color.data_ptr(),
                                              bg.data_ptr() if has_bg else None, N, num_steps, T, bound, s, car, g_image.data_ptr(), g_wsum.data_ptr(),
                                              g_depth.data_ptr(), g_nmap.data_ptr(), g_sdf.data_ptr(), g_nrm.data_ptr(), g_col.data_ptr(), g_s.data_ptr(),
                                              L.current_stream(dev)), "composite_backward")
        return None, g_sdf, g_nrm, g_col, g_s.sum().reshape(inv_s.shape), None, None, None, None, None, None


def composite(z_vals, sdf, normal, color, inv_s, rays_o, rays_d, bg, num_steps, bound, cos_anneal_ratio):
    """-> image [N,3], weights_sum [N], depth [N], normal_map [N,3], weights [N,T], alpha [N,T]; differentiable w.r.t. sdf, normal, color, inv_s"""
    return _Composite.apply(z_vals, sdf, normal, color, inv_s, rays_o, rays_d, bg, num_steps, bound, cos_anneal_ratio)


def sdf_stencil(x, table, W1, b1, W2, b2, offsets, per_level_scale, base_resolution, bound, eps):
    """-> (sdf_out [B,16], gradient [B,3]); differentiable w.r.t. table, W1, b1, W2, b2"""
    cfg = ([int(v) for v in offsets], per_level_scale, int(base_resolution), float(bound), float(eps))
    return _SdfStencil.apply(x, table, W1, b1, W2, b2, cfg)
