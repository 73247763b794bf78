"""Shared by tests/test_surface_posed_host.py (CPU) and tests/test_gpu_surface_posed.py (-m gpu): the case of the posed first-hit surface render and
`restate_posed`, the per-ray procedure of ac_render_rays_surface_warped (include/avatarcraft_hip.h) in numpy fp32 (fp64 where the header says so) -- every
operation rounds once, in the kernels' order -- around the unchanged CPU oracle: warp_samples per trip, Field.sdf at the unmasked points, _near_far_cube for the
prologue, field_samples for the shading, and the blended transform / cofactor normal of tests/mesh_pose_cases.py."""
import numpy as np

from tests import mesh_pose_cases as MP
from tests.common import edge_case_rays, make_body, make_rays

F = np.float32
BOUND, EPS, TOL, W_TOL, THRESHOLD = 1.6, 0.005, 1e-4, 1e-4, 0.05
OUTPUTS = ("image", "weights_sum", "depth", "position", "normal_map", "sdf", "status", "iters", "canonical", "normal_can", "face_id")
SHADED = (0, 1, 3, 6)
N_CAMERA = 400
# status histograms [0 .. 6] of `restate_posed` on the 400 camera rays of rays() (golden field, make_body(), the defaults), by max_iters; recorded from the
# restatement itself, like the searches and SDF evaluations of those rays at max_iters = 64
HIST_CAMERA = {64: [40, 0, 326, 0, 0, 0, 34], 16: [22, 10, 233, 0, 105, 0, 30], 1: [0, 0, 0, 0, 400, 0, 0]}
HIST_ALL = {64: [42, 0, 333, 3, 0, 0, 37], 16: [23, 10, 240, 3, 106, 0, 33], 1: [0, 0, 3, 3, 409, 0, 0]}
SEARCHES_64, SDF_EVALS_64 = 5211, 1126        # of the root finder on the camera rays: 13.0 searches and 2.8 SDF evaluations per ray
_CACHE = {}


def body():
    """make_body(): verts [3202,3] f32, faces [6400,3] i32, Ts [3202,4,4] f64 (read-only)"""
    if "body" not in _CACHE:
        b = make_body()
        for a in b:
            a.setflags(write=False)
        _CACHE["body"] = b
    return _CACHE["body"]


def rays():
    """415 rays: the 400 of make_rays(20, 20, dist=1.8, f=17.0, jitter_seed=9), the 12 of edge_case_rays(), two that start inside the posed body (their near
    point, t = 0.05, already has a negative traced value: status 3) and one with a NaN origin (its near and far are NaN, far > near is false: status 2, no search, on the device as in numpy)"""
    o, d = make_rays(20, 20, dist=1.8, f=17.0, jitter_seed=9)
    eo, ed = edge_case_rays()
    io = np.array([[0.0, 0.0, 0.0], [0.05, 0.3, 0.02], [np.nan, np.nan, np.nan]], F)
    idr = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 0.0, -1.0]], F)
    return np.ascontiguousarray(np.concatenate([o, eo, io]), F), np.ascontiguousarray(np.concatenate([d, ed, idr]), F)


def restate_posed(O, of, rays_o, rays_d, verts, faces, T, threshold=THRESHOLD, bound=BOUND, eps=EPS, level=0.0, tol=TOL, max_iters=64, step_scale=1.0, min_step=1e-3,
                  guard=0.125, w_tol=W_TOL, bg=None, dirs=None):
    """-> the outputs of ac_render_rays_surface_warped (OUTPUTS) + trace = dict(t, near, far, t_lo, s_lo, t_hi, s_hi, lo_masked, bracketed, mask_s: the mask at
    the shaded point, searches, sdf_evals)"""
    o, d = np.ascontiguousarray(rays_o, F).reshape(-1, 3), np.ascontiguousarray(rays_d, F).reshape(-1, 3)
    N = len(o)
    level, tol, step_scale, min_step, guard, w_tol, lo, hi = F(level), F(tol), F(step_scale), F(min_step), F(guard), F(w_tol), F(-bound), F(bound)
    rt = np.sqrt(F(threshold))
    assert rt.dtype == F
    near, far = O._near_far_cube(o, d, bound)
    with np.errstate(invalid="ignore"):
        pos = lambda t: np.clip(o + t[:, None] * d, lo, hi)
        t = near.copy()
        st, iters = np.full(N, 2, np.uint8), np.zeros(N, np.uint8)
        active = far > near
    have_lo, bracketed, lo_masked = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    t_lo, s_lo, t_hi, s_hi = (np.zeros(N, F) for _ in range(4))
    searches = sdf_evals = 0
    for it in range(1, int(max_iters) + 1):
        if not active.any():
            break
        idx = np.flatnonzero(active)
        can, _, d2, _, mk = O.warp_samples(pos(t)[idx], verts, faces, T, threshold)
        searches += len(idx)
        m = np.zeros(N, bool); m[idx] = mk
        s, k = np.zeros(N, F), np.ones(N, F)
        with np.errstate(all="ignore"):
            e = np.sqrt(d2.astype(F)) - rt
        bad_gap = np.zeros(N, bool); bad_gap[idx[~mk]] = ~np.isfinite(e[~mk])
        s[idx[~mk]] = np.maximum(e[~mk], min_step)
        if mk.any():
            c = np.clip(can.astype(F)[mk], lo, hi)
            s[idx[mk]] = of.sdf(c, bound)[:, 0] - level
            sdf_evals += int(mk.sum())
            k[idx[mk]] = step_scale
        iters[active] = it
        nonfin = active & (bad_gap | ~np.isfinite(s))
        hit = active & ~nonfin & m & (np.abs(s) <= tol)
        rest = active & ~nonfin & ~hit
        outside = rest & ~bracketed & (s > 0)
        miss = outside & (t >= far)
        march = outside & ~miss
        inside = rest & ~bracketed & ~(s > 0) & ~have_lo
        opened = rest & ~bracketed & ~(s > 0) & have_lo
        inb = rest & bracketed
        st[nonfin] = 5; st[hit] = 0; st[miss] = 2; st[inside] = 3
        to_lo, to_hi = march | (inb & (s > 0)), opened | (inb & ~(s > 0))
        t_lo, s_lo, lo_masked = np.where(to_lo, t, t_lo), np.where(to_lo, s, s_lo), np.where(to_lo, ~m, lo_masked)
        t_hi, s_hi = np.where(to_hi, t, t_hi), np.where(to_hi, s, s_hi)
        have_lo = have_lo | march
        bracketed = bracketed | opened
        fp = inb | opened
        with np.errstate(all="ignore"):
            w = t_hi - t_lo
            cut = fp & (w <= w_tol)
            q = np.where(lo_masked, F(0.5), s_lo / (s_lo - s_hi))
            f = t_lo + w * q
            g = guard * w
            t_fp = np.minimum(np.maximum(f, t_lo + g), t_hi - g)
            t_out = np.minimum(t + np.maximum(k * s, min_step), far)
        assert w.dtype == F and q.dtype == F and t_fp.dtype == F and t_out.dtype == F
        st[cut] = 6
        fp = fp & ~cut
        active = march | fp
        if it == int(max_iters):
            st[active & bracketed] = 1; st[active & ~bracketed] = 4
            active = np.zeros(N, bool)
        else:
            t = np.where(fp, t_fp, np.where(march, t_out, t))
    assert t.dtype == F and t_lo.dtype == F and s_lo.dtype == F
    shaded = np.isin(st, SHADED)
    t_s = np.where(np.isin(st, (1, 6)), t_hi, t)
    with np.errstate(invalid="ignore"):
        p = pos(t_s)
    assert p.dtype == F
    z3 = np.zeros((N, 3), F)
    out = dict(image=np.ones((N, 3), F) if bg is None else np.array(bg, F).reshape(N, 3), weights_sum=shaded.astype(F), depth=np.where(shaded, t_s, F(0)),
               position=np.where(shaded[:, None], p, z3), normal_map=z3.copy(), sdf=np.zeros(N, F), status=st, iters=iters, canonical=z3.copy(),
               normal_can=z3.copy(), face_id=np.full(N, -1, np.int32))
    mask_s = np.zeros(N, bool)
    if shaded.any():
        n = int(shaded.sum())
        can, clo, _, fid, mk = O.warp_samples(p[shaded], verts, faces, T, threshold)
        searches += n
        c = np.clip(can.astype(F), lo, hi)
        fs = O.field_samples(of, c, (d if dirs is None else np.ascontiguousarray(dirs, F))[shaded], np.ones(n, F), bound, eps, 64.0)
        tri = np.asarray(faces)[fid]
        M = MP.blend(np.asarray(T, np.float64), tri, MP.face_bary(clo, np.asarray(verts, F), tri))
        out["image"][shaded] = fs["rgb"]; out["normal_can"][shaded] = fs["normal"]; out["sdf"][shaded] = fs["sdf"]
        out["normal_map"][shaded] = MP.warp_normal(M, fs["normal"])
        out["canonical"][shaded] = c; out["face_id"][shaded] = fid
        mask_s[shaded] = mk
    out["trace"] = dict(t=t, near=near, far=far, t_lo=t_lo, s_lo=s_lo, t_hi=t_hi, s_hi=s_hi, lo_masked=lo_masked, bracketed=bracketed, mask_s=mask_s,
                        searches=searches, sdf_evals=sdf_evals)
    return out
