"""Timing of ac_render_rays_surface, the first-hit render of the level set, on the benchmark's 256 x 256 canonical view of the synthetic field:
    a  surface_one_launch   the kernel (root finder + stencil + colour per ray, one launch for the view)
    b  surface_chain        the same arithmetic from what the library had before it: a loop of ac_field_sdf launches with torch element-wise updates between
                            (one host read per trip: "is any ray still active"), then ONE ac_field_samples at the shaded points.  The tool ASSERTS that every
                            output of (a) is bit-identical to (b).
    c  volumetric_fused     the fused volumetric render (ac_render_rays, 64 + 64 samples) of the same rays, in the benchmark's 4096-ray batches
    d  occupancy_one_launch the occupancy-grid render (ac_render_rays_occupancy) of the same rays on a grid built for the same field (variance 512)
HIP events around `inner` back-to-back calls, the forms alternating in one process, median over the rounds.  Also printed: the status histogram, the mean number
of evaluations per ray, and the mean over tiles of 16 consecutive rays of the tile's largest count -- the trips a wave makes; the gap between the two means is
what regrouping rays between trips could win.  One JSON line.
python tools/bench_surface_render.py [--rounds 15] [--inner 4]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import nsr_ops
from bench_legs.common import make_inputs, make_net, RAYS_PER_BATCH

BOUND, EPS = 1.6, 0.005
OPTS = dict(level=0.0, tol=1e-4, max_iters=64, step_scale=1.0, min_step=1e-3, guard=0.125)
OUTPUTS = ("image", "weights_sum", "depth", "position", "normal_map", "sdf", "status", "iters")


def chain(field, o, d):
    """the arithmetic of ac_render_rays_surface from stand-alone operators (every torch operation rounds once, in the kernel's order)"""
    N, dev = o.shape[0], o.device
    tmin, tmax = (-BOUND - o) / (d + 1e-15), (BOUND - o) / (d + 1e-15)
    near = torch.where(tmin < tmax, tmin, tmax).amax(1).clamp(min=0.05)
    far = torch.where(tmin > tmax, tmin, tmax).amin(1)
    pos = lambda t: (o + t[:, None] * d).clamp(-BOUND, BOUND)
    z, zb = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.bool, device=dev)
    t, t_lo, s_lo, t_hi, s_hi = near.clone(), z, z, z, z
    st, iters = torch.full((N,), 2, dtype=torch.uint8, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    active, have_lo, bracketed = far > near, zb, zb
    u8 = lambda v: torch.full((N,), v, dtype=torch.uint8, device=dev)
    mi = OPTS["max_iters"]
    tol, min_step = (torch.tensor(OPTS[k], dtype=torch.float32, device=dev) for k in ("tol", "min_step"))      # (fp32 constants, as the kernel holds them)
    for it in range(1, mi + 1):
        if not bool(active.any()):
            break
        s = nsr_ops.field_sdf(field, pos(t), BOUND)[:, 0] - OPTS["level"]
        iters = torch.where(active, u8(it), iters)
        nonfin = active & ~torch.isfinite(s)
        hit = active & ~nonfin & (s.abs() <= tol)
        rest = active & ~nonfin & ~hit
        outside = rest & ~bracketed & (s > 0)
        miss = outside & (t >= far)
        march = outside & ~miss
        inside = rest & ~bracketed & ~(s > 0) & ~have_lo
        opened = rest & ~bracketed & ~(s > 0) & have_lo
        inb = rest & bracketed
        for m, v in ((nonfin, 5), (hit, 0), (miss, 2), (inside, 3)):
            st = torch.where(m, u8(v), st)
        to_lo, to_hi = march | (inb & (s > 0)), opened | (inb & ~(s > 0))
        t_lo, s_lo = torch.where(to_lo, t, t_lo), torch.where(to_lo, s, s_lo)
        t_hi, s_hi = torch.where(to_hi, t, t_hi), torch.where(to_hi, s, s_hi)
        have_lo, bracketed = have_lo | march, bracketed | opened
        fp = inb | opened
        w = t_hi - t_lo
        f = t_lo + w * (s_lo / (s_lo - s_hi))
        g = OPTS["guard"] * w
        t_fp = torch.minimum(torch.maximum(f, t_lo + g), t_hi - g)
        t_out = torch.minimum(t + torch.maximum(OPTS["step_scale"] * s, min_step), far)
        active = march | fp
        if it == mi:
            st = torch.where(active & bracketed, u8(1), torch.where(active & ~bracketed, u8(4), st))
        else:
            t = torch.where(fp, t_fp, torch.where(march, t_out, t))
    shaded = (st == 0) | (st == 1) | (st == 3)
    p = pos(t)
    idx = shaded.nonzero()[:, 0]
    fs = nsr_ops.field_samples(field, p[idx].contiguous(), d[idx].contiguous(), torch.ones(idx.shape[0], device=dev), BOUND, EPS, 64.0, want_sdf=True)
    z3 = torch.zeros((N, 3), device=dev)
    out = dict(image=torch.ones((N, 3), device=dev), weights_sum=shaded.float(), depth=torch.where(shaded, t, z), position=torch.where(shaded[:, None], p, z3),
               normal_map=z3.clone(), sdf=z.clone(), status=st, iters=iters)
    out["image"][idx] = fs["rgb"]; out["normal_map"][idx] = fs["normal"]; out["sdf"][idx] = fs["sdf"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_render: needs a GPU (there is no CPU path to time)")
    if a.rounds < 10:
        raise SystemExit("bench_surface_render: at least 10 rounds")
    dev = torch.device("cuda:0")
    p, field, table, ro, rd = make_inputs(dev, 0)
    field.prepare()
    o, d = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    N = o.shape[0]
    inv_s = float(p["inv_s"])
    with torch.no_grad():
        net = make_net(p, table, dev, False, cuda_ray=True)                      # the occupancy leg's grid: update_extra_state builds it for variance 512
        net.deviation_net.variance.fill_(float(np.log(512.0) / 10.0))
        net.update_extra_state(BOUND)
        occ = (net._field(), o, d, net.density_grid, net.mean_density, BOUND, EPS, net.forward_variance(), 1.0)

        def volumetric():
            for h in range(0, N, RAYS_PER_BATCH):
                nsr_ops.render_rays(field, o[h:h + RAYS_PER_BATCH], d[h:h + RAYS_PER_BATCH], 64, 64, BOUND, inv_s)

        forms = {"surface_one_launch_ms": lambda: nsr_ops.render_rays_surface(field, o, d, BOUND, EPS, **OPTS),
                 "surface_chain_ms": lambda: chain(field, o, d),
                 "volumetric_fused_ms": volumetric,
                 "occupancy_one_launch_ms": lambda: nsr_ops.render_rays_occupancy(*occ)}
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
        one, ref = forms["surface_one_launch_ms"](), forms["surface_chain_ms"]()
        torch.cuda.synchronize()
        for k in OUTPUTS:
            same = torch.equal(one[k].view(torch.int32), ref[k].view(torch.int32)) if one[k].dtype == torch.float32 else torch.equal(one[k], ref[k])
            assert same, f"bench_surface_render: the one launch and the chain of operators differ in {k}"
        st, it = one["status"], one["iters"].float()
        hist = torch.bincount(st.long(), minlength=6).tolist()
        hit = st == 0
    res = {"tool": "bench_surface_render", "rays": N, "rounds": a.rounds, "inner": a.inner, "opts": OPTS}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_max_ms")] = [round(min(v), 4), round(max(v), 4)]
    res.update(status_histogram=hist, chain_equal=True, mean_iters_per_ray=round(float(it.mean()), 3),
               mean_tile_max_iters=round(float(it[:N - N % 16].reshape(-1, 16).amax(1).mean()), 3), max_iters_seen=int(it.max()),
               max_abs_sdf_over_hits=float(one["sdf"][hit].abs().max()) if int(hit.sum()) else None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
