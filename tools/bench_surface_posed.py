"""Timing of ac_render_rays_surface_warped, the first-hit render of the POSED level set, on the benchmark's posed 256 x 256 frame (bench_legs/posed.py: the
synthetic field, make_body(83, 83), one static pose, the culling structure built once outside the timed region):
    a  surface_posed_one_call   the C call: prologue, max_iters x (closest-face search + trip kernel), shading search, shading kernel
    b  surface_posed_chain      the same arithmetic from what the library had before it: a Python loop of ac_warp_samples_accel launches at the active rays'
                                points and ac_field_sdf launches at their unmasked canonical points, torch element-wise updates between (host reads per trip:
                                which rays are active, which unmasked), then ONE search + ONE ac_field_samples at the shaded points and the blended transform /
                                cofactor normal in torch fp64.  The tool ASSERTS that every output of (a) is bit-identical to (b).
    c  volumetric_posed         the volumetric posed frame (ac_render_rays_warped, 32 + 32 samples, skip_masked) of the same rays in one batch -- a DIFFERENT
                                image (alpha-composited samples), the cost a preview of the surface had before
    d  all_rays_stopped         (a) on 65 536 rays that miss the cube: every ray is stopped by the prologue, so all 64 searches and trips are enqueued and
                                find nothing to do -- the price of the launch sequence itself; and (a) at max_iters = 16 and 32 (other images: more status 1 / 4)
HIP events around `inner` back-to-back calls, the forms alternating in one process, 3 warm-ups, median over the rounds.  Also printed: the status histogram,
searches and SDF evaluations per ray, the trips of the slowest ray, and the exact point-triangle tests of one frame of (a) and of (c) (ac_warp_accel_work).
One JSON line.
python tools/bench_surface_posed.py [--rounds 15] [--inner 2]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import _lib as L, nsr_ops
from avatarcraft_amd.synthetic import make_body, make_rays
from bench_legs.common import make_inputs

BOUND, EPS = 1.6, 0.005
OPTS = dict(level=0.0, tol=1e-4, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125, w_tol=1e-4)
OUTPUTS = ("image", "weights_sum", "depth", "position", "normal_map", "sdf", "status", "iters", "canonical", "normal_can", "face_id")


def search(p, wm, full=False):
    """one closest-face search through the public entry -> can [P,3] f32, dist2 [P] f64, mask [P] bool (+ closest [P,3] f64, face [P] i32 with `full`)"""
    P, dev = p.shape[0], p.device
    can, d2 = torch.empty((P, 3), device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    clo = torch.empty((P, 3), dtype=torch.float64, device=dev) if full else None
    fid = torch.empty(P, dtype=torch.int32, device=dev) if full else None
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    if P:
        L.check(L.lib().ac_warp_samples_accel(p.data_ptr(), wm.verts.data_ptr(), wm.faces.data_ptr(), wm.T.data_ptr(), P, wm.verts.shape[0], wm.faces.shape[0],
                                              float(wm.c.threshold), wm.accel.data_ptr(), None, can.data_ptr(), L.ptr(clo), d2.data_ptr(), L.ptr(fid), mask.data_ptr(),
                                              L.current_stream(dev)), "warp_samples_accel")
    return (can, d2, mask.bool(), clo, fid) if full else (can, d2, mask.bool())


def dot(u, v):
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]


def posed_normal(wm, clo, fid, n):
    """ac_mesh_pose's rules in torch fp64: M blended at the closest point, cofactor(A) n / (1e-30 + length), rounded to fp32"""
    tri = wm.faces.long()[fid.long()]
    a, b, c = (wm.verts[tri[:, j]].double() for j in range(3))
    v0, v1, v2 = b - a, c - a, clo - a
    d00, d01, d11, d20, d21 = dot(v0, v0), dot(v0, v1), dot(v1, v1), dot(v2, v0), dot(v2, v1)
    den = d00 * d11 - d01 * d01
    bv, bw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    bu = 1.0 - bv - bw
    M = wm.T[tri[:, 0]] * bu[:, None, None] + wm.T[tri[:, 1]] * bv[:, None, None] + wm.T[tri[:, 2]] * bw[:, None, None]
    A = lambda i, j: M[:, i, j]
    C = [[A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1), A(1, 2) * A(2, 0) - A(1, 0) * A(2, 2), A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0)],
         [A(2, 1) * A(0, 2) - A(2, 2) * A(0, 1), A(2, 2) * A(0, 0) - A(2, 0) * A(0, 2), A(2, 0) * A(0, 1) - A(2, 1) * A(0, 0)],
         [A(0, 1) * A(1, 2) - A(0, 2) * A(1, 1), A(0, 2) * A(1, 0) - A(0, 0) * A(1, 2), A(0, 0) * A(1, 1) - A(0, 1) * A(1, 0)]]
    n = n.double()
    w = [(C[r][0] * n[:, 0] + C[r][1] * n[:, 1]) + C[r][2] * n[:, 2] for r in range(3)]
    ln = 1e-30 + torch.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return torch.stack([w[r] / ln for r in range(3)], 1).float()


def sqrt32(x):
    """correctly rounded fp32 square root (through fp64: 53 bits are enough for the double rounding to be harmless)"""
    return torch.sqrt(x.double()).float()


def chain(field, o, d, wm, counts=None):
    """the arithmetic of ac_render_rays_surface_warped from stand-alone operators (every torch operation rounds once, in the kernels' order)"""
    N, dev = o.shape[0], o.device
    tmin, tmax = (-BOUND - o) / (d + 1e-15), (BOUND - o) / (d + 1e-15)
    near = torch.where(tmin < tmax, tmin, tmax).amax(1).clamp(min=0.05)
    far = torch.where(tmin > tmax, tmin, tmax).amin(1)
    pos = lambda t: (o + t[:, None] * d).clamp(-BOUND, BOUND)
    z, zb = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.bool, device=dev)
    t, t_lo, s_lo, t_hi, s_hi = near.clone(), z, z, z, z
    st, iters = torch.full((N,), 2, dtype=torch.uint8, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    active, have_lo, bracketed, lo_masked = far > near, zb, zb, zb
    u8 = lambda v: torch.full((N,), v, dtype=torch.uint8, device=dev)
    c32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)                # (fp32 constants, as the kernels hold them)
    tol, min_step, w_tol, half, rt = c32(OPTS["tol"]), c32(OPTS["min_step"]), c32(OPTS["w_tol"]), c32(0.5), sqrt32(c32(float(wm.c.threshold)))
    mi = OPTS["max_iters"]
    n_search = n_sdf = 0
    for it in range(1, mi + 1):
        idx = active.nonzero()[:, 0]
        if idx.shape[0] == 0:
            break
        can, d2, mk = search(pos(t)[idx].contiguous(), wm)
        n_search += idx.shape[0]
        m = zb.clone(); m[idx] = mk
        e = sqrt32(d2.float()) - rt
        s = torch.zeros(N, device=dev); k = torch.ones(N, device=dev)
        bad_gap = zb.clone(); bad_gap[idx[~mk]] = ~torch.isfinite(e[~mk])
        s[idx[~mk]] = torch.maximum(e[~mk], min_step)
        un = idx[mk]
        if un.shape[0]:
            s[un] = nsr_ops.field_sdf(field, can[mk].clamp(-BOUND, BOUND).contiguous(), BOUND)[:, 0] - OPTS["level"]
            k[un] = OPTS["step_scale"]
            n_sdf += un.shape[0]
        iters = torch.where(active, u8(it), iters)
        nonfin = active & (bad_gap | ~torch.isfinite(s))
        hit = active & ~nonfin & m & (s.abs() <= tol)
        rest = active & ~nonfin & ~hit
        outside = rest & ~bracketed & (s > 0)
        miss = outside & (t >= far)
        march = outside & ~miss
        inside = rest & ~bracketed & ~(s > 0) & ~have_lo
        opened = rest & ~bracketed & ~(s > 0) & have_lo
        inb = rest & bracketed
        for msk, v in ((nonfin, 5), (hit, 0), (miss, 2), (inside, 3)):
            st = torch.where(msk, u8(v), st)
        to_lo, to_hi = march | (inb & (s > 0)), opened | (inb & ~(s > 0))
        t_lo, s_lo, lo_masked = torch.where(to_lo, t, t_lo), torch.where(to_lo, s, s_lo), torch.where(to_lo, ~m, lo_masked)
        t_hi, s_hi = torch.where(to_hi, t, t_hi), torch.where(to_hi, s, s_hi)
        have_lo, bracketed = have_lo | march, bracketed | opened
        fp = inb | opened
        w = t_hi - t_lo
        cut = fp & (w <= w_tol)
        f = t_lo + w * torch.where(lo_masked, half, s_lo / (s_lo - s_hi))
        g = OPTS["guard"] * w
        t_fp = torch.minimum(torch.maximum(f, t_lo + g), t_hi - g)
        t_out = torch.minimum(t + torch.maximum(k * s, min_step), far)
        st = torch.where(cut, u8(6), st)
        fp = fp & ~cut
        active = march | fp
        if it == mi:
            st = torch.where(active & bracketed, u8(1), torch.where(active & ~bracketed, u8(4), st))
            active = zb
        else:
            t = torch.where(fp, t_fp, torch.where(march, t_out, t))
    shaded = (st == 0) | (st == 1) | (st == 3) | (st == 6)
    t_s = torch.where((st == 1) | (st == 6), t_hi, t)
    p = pos(t_s)
    idx = shaded.nonzero()[:, 0]
    can, _, _, clo, fid = search(p[idx].contiguous(), wm, full=True)
    n_search += idx.shape[0]
    c = can.clamp(-BOUND, BOUND).contiguous()
    fs = nsr_ops.field_samples(field, c, d[idx].contiguous(), torch.ones(idx.shape[0], device=dev), BOUND, EPS, 64.0, want_sdf=True)
    z3 = torch.zeros((N, 3), device=dev)
    out = dict(image=torch.ones((N, 3), device=dev), weights_sum=shaded.float(), depth=torch.where(shaded, t_s, z), position=torch.where(shaded[:, None], p, z3),
               normal_map=z3.clone(), sdf=z.clone(), status=st, iters=iters, canonical=z3.clone(), normal_can=z3.clone(),
               face_id=torch.full((N,), -1, dtype=torch.int32, device=dev))
    out["image"][idx] = fs["rgb"]; out["normal_can"][idx] = fs["normal"]; out["sdf"][idx] = fs["sdf"]; out["canonical"][idx] = c; out["face_id"][idx] = fid
    out["normal_map"][idx] = posed_normal(wm, clo, fid, fs["normal"])
    if counts is not None:
        counts.update(searches=n_search, sdf_evaluations=n_sdf)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_posed: needs a GPU (there is no CPU path to time)")
    if a.rounds < 10:
        raise SystemExit("bench_surface_posed: at least 10 rounds")
    dev = torch.device("cuda:0")
    p, field, _, _, _ = make_inputs(dev, 0)
    field.prepare()
    ro, rd = make_rays(256, 256, dist=1.8, f=443.405 / 2, yaw=0.3, pitch=-0.1)
    o, d = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    N = o.shape[0]
    inv_s = float(p["inv_s"])
    verts, faces, Ts = make_body(n_lat=83, n_lon=83)
    wm = nsr_ops.WarpMesh(verts, faces, Ts, dev, 0.05, 0.05, True)
    o_miss = torch.tensor([3.0, 3.0, 3.0], device=dev).expand(N, 3).contiguous()          # pointing away from the cube: far < near
    d_miss = torch.tensor([1.0, 1.0, 1.0], device=dev).div(3.0 ** 0.5).expand(N, 3).contiguous()
    capped = lambda mi: (lambda: nsr_ops.render_rays_surface_warped(field, o, d, BOUND, wm, EPS, **dict(OPTS, max_iters=mi)))
    with torch.no_grad():
        forms = {"surface_posed_one_call_ms": lambda: nsr_ops.render_rays_surface_warped(field, o, d, BOUND, wm, EPS, **OPTS),
                 "surface_posed_chain_ms": lambda: chain(field, o, d, wm),
                 "volumetric_posed_ms": lambda: nsr_ops.render_rays(field, o, d, 32, 32, BOUND, inv_s, warp=wm, skip_masked=True),
                 "all_rays_stopped_ms": lambda: nsr_ops.render_rays_surface_warped(field, o_miss, d_miss, BOUND, wm, EPS, **OPTS),
                 "max_iters_16_ms": capped(16), "max_iters_32_ms": capped(32)}
        for fn in forms.values():                                          # warm-up: code objects, the allocator's blocks of every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.inner)
        work = {}
        for k in ("surface_posed_one_call_ms", "volumetric_posed_ms"):
            w0 = wm.work_counters()
            forms[k]()
            w1 = wm.work_counters()
            work[k.replace("_ms", "")] = {x: w1[x] - w0[x] for x in w0}
        counts = {}
        one, ref = forms["surface_posed_one_call_ms"](), chain(field, o, d, wm, counts)
        torch.cuda.synchronize()
        for k in OUTPUTS:
            same = torch.equal(one[k].view(torch.int32), ref[k].view(torch.int32)) if one[k].dtype == torch.float32 else torch.equal(one[k], ref[k])
            assert same, f"bench_surface_posed: the one call and the chain of operators differ in {k}"
        st, it = one["status"], one["iters"].float()
        hist = torch.bincount(st.long(), minlength=7).tolist()
        assert bool((forms["all_rays_stopped_ms"]()["iters"] == 0).all())
        active_by_trip = [int((one["iters"] >= k).sum()) for k in (1, 8, 16, 24, 32, 48, 64)]
    res = {"tool": "bench_surface_posed", "rays": N, "rounds": a.rounds, "inner": a.inner, "opts": OPTS, "mesh": "synthetic 6891 verts / 13778 faces"}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_max_ms")] = [round(min(v), 4), round(max(v), 4)]
    res.update(status_histogram=hist, chain_equal=True, searches_per_ray=round(counts["searches"] / N, 3), sdf_evaluations_per_ray=round(counts["sdf_evaluations"] / N, 3),
               mean_trips_per_ray=round(float(it.mean()), 3), max_trips_seen=int(it.max()), trips_enqueued=OPTS["max_iters"],
               mean_tile_max_trips=round(float(it[:N - N % 16].reshape(-1, 16).amax(1).mean()), 3), active_rays_at_trip={str(k): v for k, v in zip((1, 8, 16, 24, 32, 48, 64), active_by_trip)}, accel_work_per_frame=work)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
