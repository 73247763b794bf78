"""First-hit surface rendering: the image of the level set itself, in canonical space and in the pose of a frame."""
import torch

from .. import nsr_ops
from .renderer import _background, _flat_rays
from .export import _check_model


def _first_hit(net, name, rays_o, rays_d, bound, bg_color, normal_epsilon_ratio, max_ray_batch, opts, warp=None):
    """THE body of render_surface (warp = None) and render_surface_posed (warp = (verts, faces, Ts) of the frame): the refusals, then the rays in batches of
    max_ray_batch through nsr_ops.render_rays_surface / render_rays_surface_warped, the parts joined (an entry that is None stays None)"""
    want_rgb = bool(opts.pop("want_rgb", True))
    kit = opts.pop("occlusion", None)
    if kit is not None:
        if warp is not None:
            raise RuntimeError(f"{name}: occlusion= is refused here -- occlusion in the pose of a frame is not built (render_surface has the canonical pose's)")
        from ..mesh_occlusion import field_occlusion, resolve_kit
        kit = resolve_kit(kit, bound, level=float(opts.get("level", 0.0)))            # a bad kit raises before any device work
    _check_model(net, f"{name} needs", colors=(name, "want_rgb=False renders geometry only") if want_rgb else None)
    if net._records_graph():
        raise RuntimeError(f"{name} builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()")
    B, N = rays_o.shape[:2]
    n = B * N
    fd_eps = nsr_ops.FD_STEP * (1.0 - normal_epsilon_ratio)
    (nsr_ops.surface_opts if warp is None else nsr_ops.surface_warped_opts)(bound, fd_eps, **opts)      # bad options raise before any device work
    with torch.no_grad():
        ro, rd = _flat_rays(rays_o, rays_d)
        if warp is None:
            launch, where = nsr_ops.render_rays_surface, (bound, fd_eps)
        else:
            wm = warp[0] if isinstance(warp[0], nsr_ops.WarpMesh) else nsr_ops.WarpMesh(*warp, ro.device)
            launch, where = nsr_ops.render_rays_surface_warped, (bound, wm, fd_eps)
        bg = None if bg_color is None else _background(bg_color, n, ro.device).contiguous()
        f = net._field_for(ignore_curvature=True)
        step = max(int(max_ray_batch or n), 1)                                    # (None: the whole view in one launch)
        parts = [launch(f, ro[h:h + step], rd[h:h + step], *where, bg=None if bg is None else bg[h:h + step], want_rgb=want_rgb, **opts)
                 for h in (range(0, n, step) or (0,))]
        if kit is not None:                                                       # at the hits: 1 where nothing is hit
            for p in parts:
                st = p["status"]
                shaded = (st == 0) | (st == 1) | (st == 3)
                p["occlusion"] = torch.where(shaded, field_occlusion(f, p["position"], p["normal_map"], bound, kit, active=shaded), torch.ones((), device=st.device))
        o = parts[0] if len(parts) == 1 else {k: (None if parts[0][k] is None else torch.cat([p[k] for p in parts])) for k in parts[0]}
    out = {"rgb": None if o["image"] is None else o["image"].reshape(B, N, 3), "depth": o["depth"].reshape(B, N), "weight_sum": o["weights_sum"][:, None],
           "normal": o["normal_map"], "position": o["position"].reshape(B, N, 3), "sdf": o["sdf"].reshape(B, N), "status": o["status"].reshape(B, N),
           "iters": o["iters"].reshape(B, N)}
    if kit is not None:
        out["occlusion"] = o["occlusion"].reshape(B, N)
    if warp is not None:
        out.update(canonical=o["canonical"].reshape(B, N, 3), normal_can=o["normal_can"], face_id=o["face_id"].reshape(B, N))
    return out


class SurfaceRendering:
    """mixed into NeRFNetwork"""

    def render_surface(self, rays_o, rays_d, bound, bg_color=None, normal_epsilon_ratio=0.0, max_ray_batch=None, **opts):
        """the image of the level set itself (ac_render_rays_surface) -- exactly the surface extract_colored_mesh / export_mesh write: per ray the first point with
        sdf = level, the field's normal and colour there, its METRIC distance and a hit mask, about 18 SDF evaluations per ray instead of the volumetric render's
        1008.  Rays as render() takes them ([B,N,3]); opts: level, tol, max_iters, step_scale, min_step, guard of nsr_ops.render_rays_surface, and want_rgb
        (False: no colour network, rgb = None; works wherever extract_colored_mesh(colors=False) does), and occlusion (None, True, occlusion_kit's keywords or a
        kit, as extract_colored_mesh takes it, at the rendered level: adds occlusion [B,N], mesh_occlusion.field_occlusion at the hit's position and normal, 1
        where nothing is hit).
        -> dict with render()'s keys that make sense here, in its shapes -- rgb [B,N,3] (background where nothing is hit), depth [B,N] (the distance t along the
        ray, NOT normalised to near/far as run()'s; 0 where nothing is hit), weight_sum [B N,1] (1 or 0), normal [B N,3] -- plus position [B,N,3], sdf [B,N],
        status [B,N] uint8 (as nsr_ops.render_rays_surface; shaded = 0, 1 or 3), iters [B,N] uint8.
        No gradient flows through a root finder's iteration count: the call raises where autograd would record (grad mode on and a parameter that requires grad).
        It does not go through render() / render_route.  Same model requirements as extract_colored_mesh."""
        return _first_hit(self, "render_surface", rays_o, rays_d, bound, bg_color, normal_epsilon_ratio, max_ray_batch, opts)

    def render_surface_posed(self, rays_o, rays_d, bound, verts, faces, Ts, bg_color=None, max_ray_batch=None, normal_epsilon_ratio=0.0, **opts):
        """render_surface in the pose of one frame (ac_render_rays_surface_warped): per ray the first point of { p : sdf(W^-1(p)) = level } inside the warp's mask
        -- the set the posed volumetric render draws and pose_mesh moves the exported mesh onto -- about a dozen closest-face searches per ray where a posed
        volumetric frame takes 64.  verts [Vg,3], faces [F,3], Ts [>= Vg,4,4]: the frame's posed guide and transforms (calc_local_trans), or verts = an
        nsr_ops.WarpMesh of the frame (faces, Ts unused).  opts: level, tol, max_iters, step_scale, min_step, guard, w_tol of nsr_ops.render_rays_surface_warped,
        and want_rgb.  occlusion= is refused: occlusion in the pose of a frame is not built.
        -> render_surface's keys and shapes -- rgb [B,N,3], depth [B,N] (the ray parameter of the shaded point; 0 where nothing is hit), weight_sum [B N,1],
        normal [B N,3] (POSED), position [B,N,3] (posed), sdf, status (shaded = 0, 1, 3 or 6; 6 = the mask boundary cuts the body there), iters [B,N] -- plus
        canonical [B,N,3] (the shaded point in canonical space), normal_can [B N,3] and face_id [B,N] int32 (closest guide face, -1 where not shaded).
        Builds no autograd graph: the call raises where autograd would record.  It does not go through render() / render_route."""
        return _first_hit(self, "render_surface_posed", rays_o, rays_d, bound, bg_color, normal_epsilon_ratio, max_ray_batch, opts, warp=(verts, faces, Ts))
