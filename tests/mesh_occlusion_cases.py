"""The arithmetic of ac_field_occlusion (include/avatarcraft_hip.h) restated in numpy fp32: every operation rounds once, in the kernel's order, np.fmax / np.fmin
where the kernel uses fmaxf / fminf.  Around any sdf(points [M,3] float32) -> [M] callable: the CPU oracle's Field.sdf on the GPU tier, analytic distance
fields on the CPU tier.  No test in this file."""
import contextlib

import numpy as np

F = np.float32


@contextlib.contextmanager
def occluded(net, spec):
    """net.export_occlusion = spec inside the block (the way into extract_colored_mesh / extract_textured_mesh, whose signatures are frozen), None after"""
    prev = net.export_occlusion
    assert prev is None
    net.export_occlusion = spec
    try:
        yield net
    finally:
        net.export_occlusion = prev


def occlusion_reference(sdf, points, normals, bound, kit, active=None):
    """-> occlusion [N] float32.  points, normals [N,3]; kit: mesh_occlusion.occlusion_kit's dict; active [N] bool or None.  Inactive rows (masked out, or with a
    number that is not finite) store 0 and are never handed to `sdf`."""
    pts, nrm = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    N = len(pts)
    act = np.isfinite(pts).all(1) & np.isfinite(nrm).all(1)
    if active is not None:
        act &= np.asarray(active).astype(bool)
    out = np.zeros(N, F)
    if not act.any():
        return out
    bound, gain, level = F(bound), F(kit["gain"]), F(kit["level"])
    dirs, weights, dists = np.asarray(kit["dirs"], F), np.asarray(kit["weights"], F), np.asarray(kit["dists"], F)
    p = np.clip(pts[act], -bound, bound)
    n = nrm[act]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    one = F(1.0)
    sg = np.copysign(one, nz)
    a = -one / (sg + nz)
    b = (nx * ny) * a
    T = np.stack([one + sg * ((nx * nx) * a), sg * b, -(sg * nx)], 1)
    U = np.stack([b, sg + (ny * ny) * a, -ny], 1)
    acc = np.zeros(len(p), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(len(dirs)):
            lx, ly, lz = dirs[k]
            w = (lx * T + ly * U) + lz * n
            v = np.ones(len(p), F)
            for j in range(len(dists)):
                t = dists[j]
                q = np.fmin(np.fmax(p + t * w, -bound), bound)
                assert q.dtype == F
                s = np.asarray(sdf(q), F).reshape(-1) - level
                h = t * lz
                r = np.fmin(np.fmax((gain * s) / h, F(0.0)), one)
                v = np.fmin(v, r)
            acc = acc + weights[k] * v
    assert acc.dtype == F
    out[act] = np.fmin(acc, one)
    return out
