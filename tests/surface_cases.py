"""Shared by tests/test_surface_render_host.py (CPU) and tests/test_gpu_surface_render.py (-m gpu): the ray set of the first-hit surface render and `restate`,
the per-ray procedure of ac_render_rays_surface (include/avatarcraft_hip.h) in numpy fp32 -- every operation rounds once, in the kernel's order -- around the
unchanged CPU oracle: Field.sdf per iteration, _near_far_cube for the prologue, field_samples for the shading."""
import numpy as np

from tests.common import edge_case_rays

F = np.float32
BOUND, EPS, TOL = 1.6, 0.005, 1e-4
OUTPUTS = ("image", "weights_sum", "depth", "position", "normal_map", "sdf", "status", "iters")
# status histograms [0, 1, 2, 3, 4, 5] of `restate` on rays() over the golden field (bound 1.6, tol 1e-4), by max_iters; and the evaluations at the defaults
HIST = {64: [453, 0, 128, 1, 6, 0], 16: [354, 5, 26, 1, 202, 0], 1: [0, 0, 2, 1, 585, 0]}
EVALS_64 = 10569


def pinhole(eye, n=24, fov=0.3, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """n x n pixel centres of a pinhole camera at `eye` looking at `target`, full field of view `fov` rad: unit directions, formed in double, then fp32"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye; fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    c = ((np.arange(n) + 0.5) / n * 2.0 - 1.0) * np.tan(0.5 * fov)
    u, v = np.meshgrid(c, -c)                                               # row 0 on top
    d = fwd[None, None] + u[..., None] * right + v[..., None] * upv
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    return np.broadcast_to(eye, d.shape).astype(F), d.astype(F)


def rays():
    """576 camera rays + the 12 of edge_case_rays(): axis-parallel, a start inside the cube, a cube miss with far < near, grazing, an unnormalised direction"""
    o, d = pinhole((0.3, 0.4, 2.6))
    eo, ed = edge_case_rays()
    return np.ascontiguousarray(np.concatenate([o, eo]), F), np.ascontiguousarray(np.concatenate([d, ed]), F)


def restate(O, of, rays_o, rays_d, bound=BOUND, eps=EPS, level=0.0, tol=TOL, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125, bg=None, dirs=None):
    """-> the outputs of ac_render_rays_surface (OUTPUTS) + trace = dict(t, s, near, far, t_lo, t_hi, bracketed): the state every ray stopped in"""
    o, d = np.ascontiguousarray(rays_o, F).reshape(-1, 3), np.ascontiguousarray(rays_d, F).reshape(-1, 3)
    N = len(o)
    level, tol, step_scale, min_step, guard, lo, hi = F(level), F(tol), F(step_scale), F(min_step), F(guard), F(-bound), F(bound)
    near, far = O._near_far_cube(o, d, bound)
    pos = lambda t: np.clip(o + t[:, None] * d, lo, hi)
    t = near.copy()
    st, iters = np.full(N, 2, np.uint8), np.zeros(N, np.uint8)
    active = far > near
    have_lo, bracketed = np.zeros(N, bool), np.zeros(N, bool)
    t_lo, s_lo, t_hi, s_hi, s_last = (np.zeros(N, F) for _ in range(5))
    for it in range(1, int(max_iters) + 1):
        if not active.any():
            break
        s = np.zeros(N, F)
        s[active] = of.sdf(pos(t)[active], bound)[:, 0] - level
        s_last = np.where(active, s, s_last)
        iters[active] = it
        nonfin = active & ~np.isfinite(s)
        hit = active & ~nonfin & (np.abs(s) <= tol)
        rest = active & ~nonfin & ~hit
        outside = rest & ~bracketed & (s > 0)
        miss = outside & (t >= far)
        march = outside & ~miss
        inside = rest & ~bracketed & ~(s > 0) & ~have_lo
        opened = rest & ~bracketed & ~(s > 0) & have_lo
        inb = rest & bracketed
        st[nonfin] = 5; st[hit] = 0; st[miss] = 2; st[inside] = 3
        to_lo, to_hi = march | (inb & (s > 0)), opened | (inb & ~(s > 0))
        t_lo, s_lo = np.where(to_lo, t, t_lo), np.where(to_lo, s, s_lo)
        t_hi, s_hi = np.where(to_hi, t, t_hi), np.where(to_hi, s, s_hi)
        have_lo = have_lo | march
        bracketed = bracketed | opened
        fp = inb | opened
        with np.errstate(all="ignore"):
            w = t_hi - t_lo
            q = s_lo / (s_lo - s_hi)
            f = t_lo + w * q
            g = guard * w
            t_fp = np.minimum(np.maximum(f, t_lo + g), t_hi - g)                        # guarded false position
            t_out = np.minimum(t + np.maximum(step_scale * s, min_step), far)
        active = march | fp
        if it == int(max_iters):
            st[active & bracketed] = 1; st[active & ~bracketed] = 4
            active = np.zeros(N, bool)
        else:
            t = np.where(fp, t_fp, np.where(march, t_out, t))
    assert t.dtype == F and t_lo.dtype == F and s_lo.dtype == F
    shaded = np.isin(st, (0, 1, 3))
    p = pos(t)
    assert p.dtype == F
    z3 = np.zeros((N, 3), F)
    out = dict(image=np.ones((N, 3), F) if bg is None else np.array(bg, F).reshape(N, 3), weights_sum=shaded.astype(F), depth=np.where(shaded, t, F(0)),
               position=np.where(shaded[:, None], p, z3), normal_map=z3.copy(), sdf=np.zeros(N, F), status=st, iters=iters)
    if shaded.any():
        k = int(shaded.sum())
        fs = O.field_samples(of, p[shaded], (d if dirs is None else np.ascontiguousarray(dirs, F))[shaded], np.ones(k, F), bound, eps, 64.0)
        out["image"][shaded] = fs["rgb"]; out["normal_map"][shaded] = fs["normal"]; out["sdf"][shaded] = fs["sdf"]
    out["trace"] = dict(t=t, s=s_last, near=near, far=far, t_lo=t_lo, t_hi=t_hi, bracketed=bracketed)
    return out
