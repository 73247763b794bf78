"""Ambient occlusion for the exported mesh and the surface renders (csrc/mesh_occlusion.hip: ac_field_occlusion, ac_mesh_bake_maps): how open the space above a
point of the level set is, asked of the SDF that produced the mesh by taps along a cone of directions around the normal -- no light setup, no ray-triangle
machinery.  The quantity, operation by operation: include/avatarcraft_hip.h (ac_field_occlusion); its numpy fp32 restatement: tests/mesh_occlusion_cases.py.
A kit is the tap pattern: K directions in the normal's frame, K weights, J distances, a gain and a level (occlusion_kit).  The default radius (0.1 bound in the
export) and gain are a starting point: no trained avatar was at hand to tune them on.
The front end of extract_colored_mesh / extract_textured_mesh (under NeRFNetwork.export_occlusion) and render_surface(occlusion=...)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .nsr_ops._args import _chk, _chk_typed, _f32

MAX_DIRS, MAX_STEPS = 32, 16
BAKE_OUTPUTS = ("rgb", "normals", "positions", "sdf", "status")


def _table(x, shape, name):
    try:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    except (TypeError, ValueError) as e:
        raise ValueError(f"occlusion_kit: {name} must be an array of numbers ({e})") from e
    if a.ndim != len(shape) or any(s is not None and s != n for s, n in zip(shape, a.shape)):
        raise ValueError(f"occlusion_kit: {name} must have shape {list(shape)}, got {list(a.shape)}")
    return a


def check_kit(kit):
    """ValueError for what ac_field_occlusion / ac_mesh_bake_maps would refuse in a kit (the same rules in the same order); no device work.
    -> the kit with float32 tables: dict(dirs [K,3], weights [K], dists [J], gain, level)"""
    try:
        dirs, weights, dists = _table(kit["dirs"], (None, 3), "dirs"), _table(kit["weights"], (None,), "weights"), _table(kit["dists"], (None,), "dists")
        gain, level = float(kit["gain"]), float(kit["level"])
    except (TypeError, KeyError) as e:
        raise ValueError(f"occlusion_kit: a kit is a dict(dirs, weights, dists, gain, level) as occlusion_kit makes it ({e!r})") from e
    K, J = dirs.shape[0], dists.shape[0]
    if not 1 <= K <= MAX_DIRS or not 1 <= J <= MAX_STEPS or weights.shape[0] != K:
        raise ValueError(f"occlusion_kit: {K} directions outside 1..{MAX_DIRS}, {J} distances outside 1..{MAX_STEPS}, or {weights.shape[0]} weights for {K} directions")
    if not math.isfinite(np.float32(gain)) or not np.float32(gain) > 0 or not math.isfinite(np.float32(level)):
        raise ValueError(f"occlusion_kit: gain {gain!r} must be finite and > 0, level {level!r} finite")
    total = 0.0
    for i in range(K):
        l, w = [float(v) for v in dirs[i]], float(weights[i])
        if not all(math.isfinite(v) for v in l + [w]):
            raise ValueError(f"occlusion_kit: direction or weight {i} is not finite")
        if not l[2] >= float(np.float32(0.05)):
            raise ValueError(f"occlusion_kit: direction {i} has lz {l[2]} < 0.05")
        length = math.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])
        if not abs(length - 1.0) <= 1e-3:
            raise ValueError(f"occlusion_kit: direction {i} has length {length}, not within 1e-3 of 1")
        if not w >= 0.0:
            raise ValueError(f"occlusion_kit: weight {i} is negative")
        total += w
    if not abs(total - 1.0) <= 1e-5:
        raise ValueError(f"occlusion_kit: the weights sum to {total}, not within 1e-5 of 1")
    for j in range(J):
        t = float(dists[j])
        if not math.isfinite(t) or not t > 0.0 or (j and not t > float(dists[j - 1])):
            raise ValueError(f"occlusion_kit: the distances must be finite, > 0 and strictly ascending (distance {j})")
    return dict(dirs=dirs, weights=weights, dists=dists, gain=gain, level=level)


def occlusion_kit(radius=None, directions=8, steps=4, gain=1.0, level=0.0, dirs=None, weights=None, dists=None):
    """the tap pattern of the occlusion: -> dict(dirs [K,3], weights [K], dists [J] float32 numpy tables, gain, level).  By default K = directions
    cosine-weighted directions on a golden-angle spiral -- for i = 0 .. K-1, u = (i + 0.5) / K, phi = (i + 0.5) pi (3 - sqrt 5):
    l = (sqrt(u) cos phi, sqrt(u) sin phi, sqrt(1 - u)), in float64, then rounded -- with equal weights 1 / K, and J = steps distances
    t_j = radius (j + 1) / J.  Explicit dirs / weights / dists replace the table they name (weights default to 1 / K of the directions given).
    gain scales the test (r = gain sdf / h: above 1 forgives a field that under-reports distances), level is the level set the points lie on.
    ValueError for whatever the C entries would refuse (check_kit), before anything else."""
    if dirs is None:
        if isinstance(directions, bool) or not isinstance(directions, (int, np.integer)) or not 1 <= directions <= MAX_DIRS:
            raise ValueError(f"occlusion_kit: directions {directions!r} must be an integer in 1..{MAX_DIRS}")
        K = int(directions)
        i = np.arange(K, dtype=np.float64) + 0.5
        u, phi = i / K, i * (math.pi * (3.0 - math.sqrt(5.0)))
        dirs = np.stack([np.sqrt(u) * np.cos(phi), np.sqrt(u) * np.sin(phi), np.sqrt(1.0 - u)], 1)
    if weights is None:
        K = len(dirs)
        weights = np.full(K, 1.0 / K if K else 0.0, np.float64)
    if dists is None:
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= MAX_STEPS:
            raise ValueError(f"occlusion_kit: steps {steps!r} must be an integer in 1..{MAX_STEPS}")
        try:
            radius = float(radius)
        except (TypeError, ValueError) as e:
            raise ValueError(f"occlusion_kit: radius {radius!r} must be a number > 0") from e
        if not math.isfinite(radius) or not radius > 0:
            raise ValueError(f"occlusion_kit: radius {radius!r} must be finite and > 0")
        dists = radius * (np.arange(int(steps), dtype=np.float64) + 1.0) / int(steps)
    try:
        gain, level = float(gain), float(level)
    except (TypeError, ValueError) as e:
        raise ValueError(f"occlusion_kit: gain and level must be numbers ({e})") from e
    return check_kit(dict(dirs=dirs, weights=weights, dists=dists, gain=gain, level=level))


def resolve_kit(spec, bound, level=0.0):
    """NeRFNetwork.export_occlusion and the `occlusion=` argument of the drivers and the surface render -> a checked kit: True = the default kit with radius 0.1 bound at `level`; a dict with
    `dirs` = a kit, passed as is; any other dict = occlusion_kit's keywords (radius defaults to 0.1 bound, level to `level`).  ValueError otherwise."""
    if spec is True:
        return occlusion_kit(0.1 * float(bound), level=level)
    if isinstance(spec, dict):
        if "dirs" in spec and "weights" in spec and "dists" in spec and "gain" in spec and "level" in spec:
            return check_kit(spec)
        kw = dict(spec)
        if "dists" not in kw:
            kw.setdefault("radius", 0.1 * float(bound))
        kw.setdefault("level", level)
        try:
            return occlusion_kit(**kw)
        except TypeError as e:
            raise ValueError(f"occlusion: {e}") from e
    raise ValueError(f"occlusion: {spec!r} is neither None, True, a dict of occlusion_kit's keywords nor a kit")


def _kit_arg(kit):
    """(ac_occlusion_opts, what it points to) of a kit; ValueError for a kit the entry would refuse"""
    k = check_kit(kit)
    return L.ac_occlusion_opts(k["dirs"].shape[0], k["dists"].shape[0], k["dirs"].ctypes.data, k["weights"].ctypes.data, k["dists"].ctypes.data,
                               k["gain"], k["level"]), k


def field_occlusion(field, points, normals, bound, kit, active=None):
    """ac_field_occlusion: points [N,3] and their unit normals [N,3], float32 on the device (mesh_vertex_attrs' positions / normals, a surface render's hits) ->
    occlusion [N] float32 in [0, 1], 1 = open.  active [N] bool or uint8: rows to evaluate (None: all); an inactive row, and a row with a number that is not
    finite, stores 0 and costs nothing.  The kit is checked first (ValueError), then the tensors (RuntimeError), before any launch."""
    opts, keep = _kit_arg(kit)
    points = _chk(points, "field_occlusion: points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("field_occlusion: points must be [N,3]")
    N, dev = points.shape[0], points.device
    normals = _chk(normals, "field_occlusion: normals", (N, 3))
    if normals.device != dev:
        raise RuntimeError("field_occlusion: normals must live on the device of points")
    if active is not None:
        _chk_typed(active, (torch.bool, torch.uint8), (N,), "field_occlusion: active must be a bool or uint8 [N] tensor on the device of points",
                   cuda_msg="field_occlusion: active must be a CUDA tensor", device=dev, contiguous=False)
        active = active.to(torch.uint8).contiguous()
    out = _f32(dev, N)
    L.check(L.lib().ac_field_occlusion(C.byref(field.c), L.ptr(points), L.ptr(normals), L.ptr(active), N, float(bound), C.byref(opts), L.ptr(out),
                                       L.current_stream(dev)), "field_occlusion")
    del keep
    return out


def mesh_bake_maps(field, positions, triangles, size, cell, bound, eps=None, kit=None, want=BAKE_OUTPUTS, refine_steps=3, tol=1e-5, max_move=None, target_sdf=0.0):
    """ac_mesh_bake_maps: nsr_ops.mesh_bake_texture with more maps out of the same launch -- per owned texel the point on its triangle is refined and shaded as
    there (the colour network only when "rgb" is wanted), and with a kit the occlusion is taken at that refined point and normal: colour and occlusion share the
    texel's refine.  Arguments as mesh_bake_texture's; want: which of rgb, normals, positions, sdf, status to return (the others are None).
    -> dict(rgb [S,S,3], owner [S,S] int32, normals [S,S,3], positions [S,S,3] the refined points, sdf [S,S], status [S,S] uint8, occlusion [S,S] | None without
    a kit); unowned texels: owner -1, everything else 0.  What it shares with mesh_bake_texture has the same bits; occlusion has field_occlusion's on
    (positions, normals, owner >= 0).  The kit (ValueError), the tensors and the triangle indices (RuntimeError, checked on the device) are refused before the launch."""
    from .nsr_ops.mesh import _bake_args
    from .nsr_ops.render import FD_STEP
    opts_o, keep = _kit_arg(kit) if kit is not None else (None, None)
    unknown = set(want) - set(BAKE_OUTPUTS)
    if unknown:
        raise ValueError(f"mesh_bake_maps: unknown outputs {sorted(unknown)}")
    V, T, S, dev, atlas, opts = _bake_args("mesh_bake_maps", positions, triangles, size, cell, bound, FD_STEP if eps is None else eps, target_sdf, refine_steps,
                                           tol, max_move)
    img = lambda name, *tail: _f32(dev, S, S, *tail) if name in want else None
    out = dict(rgb=img("rgb", 3), owner=torch.empty((S, S), dtype=torch.int32, device=dev), normals=img("normals", 3), positions=img("positions", 3),
               sdf=img("sdf"), status=torch.empty((S, S), dtype=torch.uint8, device=dev) if "status" in want else None,
               occlusion=_f32(dev, S, S) if kit is not None else None)
    c_out = L.ac_bake_out(*(L.ptr(out[k]) for k in ("rgb", "owner", "normals", "positions", "sdf", "status", "occlusion")))
    L.check(L.lib().ac_mesh_bake_maps(C.byref(field.c), positions.data_ptr(), V, triangles.data_ptr(), T, C.byref(atlas), C.byref(opts),
                                      None if opts_o is None else C.byref(opts_o), C.byref(c_out), L.current_stream(dev)), "mesh_bake_maps")
    del keep
    return out
