"""The first-hit renderers of the level set (csrc/surface_rays.hip): canonical space and through the inverse warp of a posed frame."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._args import _chk, _f32
from .render import FD_STEP
from .warp import WarpMesh


def surface_opts(bound, fd_eps, level=0.0, tol=1e-4, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125, who="render_rays_surface"):
    """ac_surface_opts from Python numbers; the checks of ac_render_rays_surface made here, before any device work (RuntimeError naming the option)"""
    try:
        mi = int(max_iters)
        bound, fd_eps, level, tol, step_scale, min_step, guard = (float(v) for v in (bound, fd_eps, level, tol, step_scale, min_step, guard))
    except (TypeError, ValueError) as e:
        raise RuntimeError(f"{who}: options must be numbers ({e})") from e
    if mi != max_iters or not 1 <= mi <= 255:
        raise RuntimeError(f"{who}: max_iters {max_iters!r} outside 1..255")
    if not tol >= 0.0:
        raise RuntimeError(f"{who}: tol {tol!r} not >= 0")
    for name, v in (("bound", bound), ("fd_eps", fd_eps), ("step_scale", step_scale), ("min_step", min_step)):
        if not (v > 0.0 and np.float32(v) > 0.0):
            raise RuntimeError(f"{who}: {name} {v!r} not > 0")
    if not (0.0 <= guard and np.float32(guard) < np.float32(0.5)):
        raise RuntimeError(f"{who}: guard {guard!r} outside [0, 0.5)")
    return L.ac_surface_opts(bound, fd_eps, level, tol, mi, step_scale, min_step, guard)


def render_rays_surface(field, rays_o, rays_d, bound, fd_eps, *, level=0.0, tol=1e-4, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125, bg=None,
                        want_rgb=True):
    """ac_render_rays_surface: the first-hit render of the level set sdf = level, one launch.  rays_o, rays_d [N,3] float32 on the device.  Per ray: sphere-tracing
    steps max(step_scale s, min_step) from the cube's near until the sign changes, then guarded false position inside the bracket until |sdf - level| <= tol, at
    most max_iters evaluations (the procedure operation by operation: include/avatarcraft_hip.h); then normal, sdf and colour at the point found, as field_samples
    gives them (view direction: the rays_d row as given, for a field with Wc1_sh).  bg [N,3] or None (white).  want_rgb=False: no colour network (an SDF-only
    field is enough), image = None.
    -> dict(image [N,3] | None, weights_sum [N] (1 or 0), depth [N] (metric t; 0 where not shaded), position [N,3], normal_map [N,3], sdf [N], status [N] uint8
    (0 hit, 1 out of iterations inside a bracket, 2 miss, 3 starts inside, 4 out of iterations without a bracket, 5 value not finite; shaded =
    0, 1 or 3), iters [N] uint8 = SDF evaluations of the root finder)"""
    opts = surface_opts(bound, fd_eps, level, tol, max_iters, step_scale, min_step, guard)
    N, dev, out, so = _surface_args("render_rays_surface", field, rays_o, rays_d, bg, want_rgb)
    L.check(L.lib().ac_render_rays_surface(C.byref(field.c), C.byref(opts), rays_o.data_ptr(), rays_d.data_ptr(), N, L.ptr(bg), C.byref(so),
                                           L.current_stream(dev)), "render_rays_surface")
    return out


def _surface_args(who, field, rays_o, rays_d, bg, want_rgb, posed=False, warp=None):
    """the tensor checks of the two surface renderers (rays_o, rays_d, bg are used as given: no copies), their result dict and its ac_surface_out ->
    (N, device, out, ac_surface_out).  posed: + the checks of the mesh `warp` and the three posed outputs."""
    _chk(rays_o, "rays_o")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3:
        raise RuntimeError(f"{who}: rays_o must be [N,3], got {tuple(rays_o.shape)}")
    if posed and not isinstance(warp, WarpMesh):
        raise RuntimeError(f"{who}: warp must be an nsr_ops.WarpMesh")
    N, dev = rays_o.shape[0], rays_o.device
    _chk(rays_d, "rays_d", (N, 3))
    if bg is not None:
        _chk(bg, "bg", (N, 3))
    if rays_d.device != dev or (bg is not None and bg.device != dev) or field.device != dev or (posed and warp.verts.device != dev):
        raise RuntimeError(f"{who}: field, rays_o, rays_d" + (", bg and the mesh" if posed else " and bg") + " must live on one device")
    if posed and warp.faces.shape[0] == 0:
        raise RuntimeError(f"{who}: a mesh without faces")
    u8 = lambda: torch.empty(N, dtype=torch.uint8, device=dev)
    out = dict(image=_f32(dev, N, 3) if want_rgb else None, weights_sum=_f32(dev, N), depth=_f32(dev, N), position=_f32(dev, N, 3),
               normal_map=_f32(dev, N, 3), sdf=_f32(dev, N), status=u8(), iters=u8())
    if posed:
        out.update(canonical=_f32(dev, N, 3), normal_can=_f32(dev, N, 3), face_id=torch.empty(N, dtype=torch.int32, device=dev))
    so = L.ac_surface_out(*[L.ptr(out[k]) for k in ("image", "weights_sum", "depth", "position", "normal_map", "sdf", "status", "iters")])
    return N, dev, out, so


def surface_warped_opts(bound, fd_eps, level=0.0, tol=1e-4, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125, w_tol=1e-4):
    """(ac_surface_opts, w_tol) from Python numbers; the checks of ac_render_rays_surface_warped made here, before any device work (RuntimeError naming the option)"""
    who = "render_rays_surface_warped"
    opts = surface_opts(bound, fd_eps, level, tol, max_iters, step_scale, min_step, guard, who=who)
    try:
        w_tol = float(w_tol)
    except (TypeError, ValueError) as e:
        raise RuntimeError(f"{who}: w_tol must be a number ({e})") from e
    if not (w_tol >= 0.0 and np.float32(w_tol) >= 0.0):
        raise RuntimeError(f"{who}: w_tol {w_tol!r} not >= 0")
    return opts, w_tol


def render_rays_surface_warped(field, rays_o, rays_d, bound, warp, fd_eps=FD_STEP, *, level=0.0, tol=1e-4, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125,
                               w_tol=1e-4, bg=None, want_rgb=True):
    """ac_render_rays_surface_warped: the first-hit render of the POSED level set { p : sdf(W^-1(p)) = level, p inside the mask }, W^-1 the inverse warp of the
    frame `warp` (an nsr_ops.WarpMesh) -- what the posed renderer draws and mesh_pose moves a mesh onto.  rays_o, rays_d [N,3] float32 on the device.  Per ray and
    trip one closest-face search at the posed point, then either the canonical SDF there (inside the mask) or the gap to the mask (outside: an exact safe step);
    sphere tracing to the sign change, guarded false position inside the bracket (bisection while its outer end is a masked point), at most max_iters trips (the
    procedure operation by operation: include/avatarcraft_hip.h).  One C call; the scratch is allocated here.
    -> dict(image [N,3] | None, weights_sum [N], depth [N] (the ray parameter of the shaded point), position [N,3] (posed), normal_map [N,3] (posed), sdf [N],
    status [N] uint8 (0 .. 5 as render_rays_surface, 6 = the bracket closed on the mask boundary to within w_tol; shaded = 0, 1, 3 or 6), iters [N] uint8 (searches
    of the root finder), canonical [N,3] (the shaded point in canonical space), normal_can [N,3], face_id [N] int32 (closest guide face; -1 where not shaded))"""
    who = "render_rays_surface_warped"
    opts, w_tol = surface_warped_opts(bound, fd_eps, level, tol, max_iters, step_scale, min_step, guard, w_tol)
    N, dev, out, so = _surface_args(who, field, rays_o, rays_d, bg, want_rgb, posed=True, warp=warp)
    sw = L.ac_surface_warped_out(*[L.ptr(out[k]) for k in ("canonical", "normal_can", "face_id")])
    need = int(L.lib().ac_render_rays_surface_warped_scratch(N))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    L.check(L.lib().ac_render_rays_surface_warped(C.byref(field.c), C.byref(opts), w_tol, rays_o.data_ptr(), rays_d.data_ptr(), N, L.ptr(bg), C.byref(warp.c),
                                                  scratch.data_ptr(), need, C.byref(so), C.byref(sw), L.current_stream(dev)), who)
    return out
