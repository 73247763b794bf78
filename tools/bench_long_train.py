#!/usr/bin/env python3
"""Stylisation step time at the long renderer's counts: one sds_step on a 64 x 64 patch (4096 rays, SyntheticGuidance: the pair route) and on a
256 x 256 view of 16 patches (the view routes), on the fused route (forward = the long renderer, backward = ac_render_core_backward) or on the
autograd route (NeRFNetwork.manual_backward_supported forced False: sampling launch + the autograd render core); and the backward alone.

    timeout -k 10 600 python tools/bench_long_train.py --what patch --counts 128+128 --route fused [--steps 5 --warmup 2]
    timeout -k 10 600 python tools/bench_long_train.py --what backward --counts 128+128
    timeout -k 10 600 python tools/bench_long_train.py --what extras --counts 128+128

--what backward times ac_render_core_backward alone on one 4096-ray patch: the long route with the stencil features gathered again and, where 16 divides
the count, on the features its forward kept (render_rays_long(save_stencil=True)); where the fused renderer also takes the counts, the short route too
(render_rays + the features its forward kept).
--what extras times the patch step (the one-patch pair route) with NeRFNetwork.long_step_extras on against the same step with it off -- the route
every earlier figure of this tool measured -- in ONE process and run: two pairs of nets, the off route timed before AND after the on route (the
difference between its two medians is the run-to-run spread the comparison has to beat).  One measurement per process, so that
each runs under its own time limit; prints one JSON line: median and min ms per step (host clock around steps that end in a device synchronise, or
event pairs around the backward), and the peak of torch.cuda.max_memory_allocated over the timed work.  The figures in DESIGN.md section 5.8 come
from this loop:

    for c in 64+64 128+128 100+64 256+0; do for w in patch view; do for r in fused autograd; do
        timeout -k 10 600 python tools/bench_long_train.py --what $w --counts $c --route $r || break 3; done; done; done
    timeout -k 10 600 python tools/bench_long_train.py --what backward --counts 128+128
    timeout -k 10 600 python tools/bench_long_train.py --what backward --counts 64+64
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _nets(dev, route):
    from bench_legs.common import make_net
    from avatarcraft_amd.synthetic import load_field_params, device_field
    p = load_field_params()
    _, table = device_field(p, device=dev)
    table = table if isinstance(table, np.ndarray) else table.cpu().numpy()
    net, net_gt = make_net(p, table, dev, True), make_net(p, table, dev, False)
    if route == "autograd":
        net.manual_backward_supported = lambda *a, **k: False
    return net, net_gt


def time_step(dev, what, T0, up, route, steps, warmup):
    import avatarcraft_amd.stylize as ST
    from bench_legs.common import sds_view
    from avatarcraft_amd.synthetic import make_rays
    net, net_gt = _nets(dev, route)
    if what == "patch":
        ro, rd = sds_view(0)
        hw = (64, 64)
    else:
        ro, rd = make_rays(256, 256, dist=1.8, f=200.0, yaw=0.0, pitch=0.0)
        hw = (256, 256)
    ro, rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    opt = ST.Adam(net.parameters(), lr=5e-3, zero_grad_in_step=True)
    flat = ST.flat_grad_view(net.parameters())
    guidance = ST.SyntheticGuidance(42)
    step = lambda: ST.sds_step(net, net_gt, ro, rd, hw, opt, guidance, batch_size=4096, flat_grad=flat, num_steps=T0, upsample_steps=up)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    net.check_finite()
    return ms


def time_extras(dev, T0, up, steps, warmup):
    """the patch step with long_step_extras off / on / off again, each a median of `steps` after `warmup`, one process"""
    import avatarcraft_amd.stylize as ST
    from bench_legs.common import sds_view
    ro, rd = (torch.from_numpy(a).to(dev) for a in sds_view(0))

    def make(on):
        net, net_gt = _nets(dev, "fused")
        net.long_step_extras = net_gt.long_step_extras = on
        opt = ST.Adam(net.parameters(), lr=5e-3, zero_grad_in_step=True)
        flat = ST.flat_grad_view(net.parameters())
        guidance = ST.SyntheticGuidance(42)
        return net, lambda: ST.sds_step(net, net_gt, ro, rd, (64, 64), opt, guidance, batch_size=4096, flat_grad=flat, num_steps=T0, upsample_steps=up)

    def run(step):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": round(float(np.median(ms)), 2), "ms_min": round(float(np.min(ms)), 2), "ms_max": round(float(np.max(ms)), 2),
                "peak_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
    (net_off, off), (net_on, on) = make(False), make(True)
    res = {"off (before)": run(off), "on": run(on), "off (after)": run(off)}
    net_off.check_finite(); net_on.check_finite()
    base = 0.5 * (res["off (before)"]["ms_median"] + res["off (after)"]["ms_median"])
    res["on / off"] = round(res["on"]["ms_median"] / base, 4)
    res["off spread"] = round(abs(res["off (before)"]["ms_median"] - res["off (after)"]["ms_median"]) / base, 4)
    res["stencil features kept"] = bool(net_on._long_save_stencil(T0, up))
    return res


def time_backward(dev, T0, up, steps, warmup):
    from avatarcraft_amd import nsr_ops
    from bench_legs.common import sds_view
    net, _ = _nets(dev, "fused")
    ro, rd = (torch.from_numpy(a).to(dev) for a in sds_view(0))
    N = ro.shape[0]
    g = torch.Generator(device=dev); g.manual_seed(3)
    noise = torch.rand((N, T0), device=dev, generator=g)
    g_img = torch.rand((N, 3), device=dev, generator=g) - 0.5
    g_eik = torch.full((1,), 0.01, device=dev)
    field = net._field()
    routes = [("long", nsr_ops.render_rays_long, {})]
    if (T0 + up) % 16 == 0:
        routes.append(("long saved", nsr_ops.render_rays_long, dict(save_stencil=True)))
    if nsr_ops.in_short_window(T0, up):
        routes.append(("short", nsr_ops.render_rays, {}))
    res = {}
    for name, render, kw in routes:
        with torch.no_grad():
            out = render(field, ro, rd, T0, up, 1.6, net.forward_variance(), noise=noise, extras=True, train_extras=True, **kw)
        g_table = torch.zeros_like(net.encoder.embeddings)
        bwd = lambda: nsr_ops.render_core_backward(field, out.opts, out, ro, rd, None, g_img, None, None, None, g_eik, g_table)
        for _ in range(warmup):
            bwd()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        ms = []
        for _ in range(steps):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(); bwd(); ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        res[name.split()[0] + (" (stencil features kept)" if "feat7" in out else " (stencil features gathered again)")] = {
            "ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3),
            "peak_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
        del out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["patch", "view", "backward", "extras"], required=True)
    ap.add_argument("--counts", default="128+128", help="num_steps+upsample_steps")
    ap.add_argument("--route", choices=["fused", "autograd"], default="fused")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_long_train times the GPU"
    T0, up = (int(v) for v in a.counts.split("+"))
    dev = torch.device("cuda:0")
    key = f"{a.what} {T0}+{up}"
    if a.what == "backward":
        print(json.dumps({key: time_backward(dev, T0, up, a.steps, a.warmup)}))
        return
    if a.what == "extras":
        print(json.dumps({key: time_extras(dev, T0, up, a.steps, a.warmup)}))
        return
    ms = time_step(dev, a.what, T0, up, a.route, a.steps, a.warmup)
    print(json.dumps({f"{key} {a.route}": {"ms_median": round(float(np.median(ms)), 2), "ms_min": round(float(np.min(ms)), 2),
                                            "peak_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}}))


if __name__ == "__main__":
    main()
