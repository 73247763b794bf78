#!/usr/bin/env python3
"""Rays per second of the long renderer (ac_render_rays_long) on a 256 x 256 view of the synthetic field, next to the fused renderer at 64 + 64.

    timeout -k 10 300 python tools/bench_long_rays.py [--iters 10] [--warmup 3]

Prints one JSON line: {"<entry> <num_steps>+<upsample_steps>": {"ms": median ms per view, "mrays_s": M rays/s}, ...}.  Each launch is timed
with a pair of events around it (the lean instantiations: no per-sample outputs).
Posed rows ("posed <entry> ..."): one 256 x 256 frame of the SMPL-sized synthetic body (6 891 vertices), mesh guide and skip_masked on, the whole
posed sequence (near / far, both closest-face searches, both render passes) between the events, median of 5 after 2 warm-ups; the short posed frame
at 32 + 32 from the same run is the yardstick of the long ones."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.synthetic import device_field, load_field_params, make_rays
    p = load_field_params()
    f, _ = device_field(p)
    f.prepare()
    ro, rd = make_rays(256, 256, dist=1.7, f=200.0)
    ro, rd = (torch.from_numpy(a).cuda() for a in (ro, rd))
    inv_s = float(p["inv_s"])
    cases = [("render_rays", 64, 64), ("render_rays_long", 64, 64), ("render_rays_long", 128, 128), ("render_rays_long", 100, 64),
             ("render_rays_long", 256, 0)]
    res = {}
    for entry, T0, up in cases:
        fn = getattr(nsr_ops, entry)
        out = None
        for _ in range(args.warmup):
            out = fn(f, ro, rd, T0, up, 1.6, inv_s, out=out)
        ms = []
        for _ in range(args.iters):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            out = fn(f, ro, rd, T0, up, 1.6, inv_s, out=out, events=ev)
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        assert torch.isfinite(out["image"]).all(), (entry, T0, up)
        m = float(np.median(ms))
        res[f"{entry} {T0}+{up}"] = {"ms": round(m, 3), "mrays_s": round(ro.shape[0] / m / 1e3, 3)}
    from avatarcraft_amd.synthetic import make_body
    verts, faces, Ts = make_body(n_lat=83, n_lon=83)
    pro, prd = make_rays(256, 256, dist=1.8, f=0.78125 * 256)
    pro, prd = (torch.from_numpy(a).cuda() for a in (pro, prd))
    wm = nsr_ops.WarpMesh(verts, faces, Ts, "cuda", use_mesh_guide=True)
    for entry, T0, up in (("render_rays", 32, 32), ("render_rays_long", 32, 32), ("render_rays_long", 128, 128), ("render_rays_long", 100, 64)):
        fn = getattr(nsr_ops, entry)
        out = None
        for _ in range(2):
            out = fn(f, pro, prd, T0, up, 1.6, inv_s, out=out, warp=wm, skip_masked=True)
        ms = []
        for _ in range(5):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            out = fn(f, pro, prd, T0, up, 1.6, inv_s, out=out, events=ev, warp=wm, skip_masked=True)
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        assert torch.isfinite(out["image"]).all(), ("posed", entry, T0, up)
        m = float(np.median(ms))
        res[f"posed {entry} {T0}+{up}"] = {"ms": round(m, 3), "mrays_s": round(pro.shape[0] / m / 1e3, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
