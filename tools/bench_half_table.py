"""Time the fused renderer from the fp32 hash table and from the half table (nsr_ops.render_rays(table_dtype=...)), in ONE process.

    python tools/bench_half_table.py [--rounds 15] [--warmup 3]

Workloads (both in exact precision, the synthetic field of bench.py):
  headline  the view of bench.py / README's first row: 256 x 256 rays, 64 + 64 samples, sixteen 4096-ray launches (lean outputs);
  posed     the 32 + 32 posed frame of bench_legs/posed.py: 256 x 256 rays in one batch, SMPL-sized synthetic body, mesh-guided range, skip_masked
            (mesh upload and culling structure outside the timed region: the two table formats share them).
Protocol: after the warm-ups every round times the fp32 table, then the half table (alternating, so that drift on a shared host hits both), each between
a pair of HIP events around its launches; the figure of a format is the median over the rounds.  The spread of the fp32 rounds themselves
((max - min) / median, and the inter-quartile range) is printed beside the ratio: a ratio inside that spread is no difference.  The largest pixel
difference between the two renders of each workload is reported as well (they are different fields by the fp16 rounding of the table).
Prints one JSON object.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def alternate(runs, rounds, warmup):
    """runs: {name: callable}; every round runs each once between its own pair of events -> {name: [ms per round]}"""
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        evs = {}
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k] = (e0, e1)
        torch.cuda.synchronize()
        for k, (e0, e1) in evs.items():
            ms[k].append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    f, h = np.asarray(ms["float"]), np.asarray(ms["half"])
    mf, mh = float(np.median(f)), float(np.median(h))
    q1, q3 = np.percentile(f, [25, 75])
    return {"float_ms": mf, "half_ms": mh, "half_over_float": mh / mf, "float_spread_max_min_over_median": float((f.max() - f.min()) / mf),
            "float_iqr_over_median": float((q3 - q1) / mf), "half_iqr_over_median": float(np.subtract(*np.percentile(h, [75, 25])) / mh),
            "inside_float_spread": bool(abs(mh - mf) <= (f.max() - f.min())), "rounds": int(len(f))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_table: needs the MI355X (no CPU fallback)")
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.synthetic import load_field_params, make_rays, make_body, device_field
    dev = "cuda:0"
    p = load_field_params()
    field, _ = device_field(p, device=dev)
    field.prepare()
    field.half_table()                                          # converted once, outside every timed region
    inv_s = float(p["inv_s"])
    res = {"table_bytes": {"float": int(field.t["table"].numel() * 4), "half": int(field.half_table().numel() * 4)}}

    # headline: sixteen 4096-ray launches of one 256 x 256 view, 64 + 64
    ro, rd = make_rays(256, 256, dist=1.7, f=200.0, yaw=0.0, pitch=0.0)
    ro, rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    outs = {k: [dict() for _ in range(16)] for k in ("float", "half")}

    def view(k):
        for b in range(16):
            sl = slice(b * 4096, (b + 1) * 4096)
            nsr_ops.render_rays(field, ro[sl], rd[sl], 64, 64, 1.6, inv_s, out=outs[k][b], table_dtype=k)
    r = summary(alternate({"float": lambda: view("float"), "half": lambda: view("half")}, a.rounds, a.warmup))
    r["float_ms_per_4096_rays"], r["half_ms_per_4096_rays"] = r["float_ms"] / 16, r["half_ms"] / 16
    r["image_linf_half_vs_float"] = max(float((x["image"] - y["image"]).abs().max()) for x, y in zip(outs["float"], outs["half"]))
    res["headline_256x256_64+64_16x4096"] = r

    # posed: one 65 536-ray frame, 32 + 32
    verts, faces, Ts = make_body(n_lat=83, n_lon=83)
    ro, rd = make_rays(256, 256, dist=1.8, f=443.405 / 2, yaw=0.3, pitch=-0.1)
    ro, rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    wm = nsr_ops.WarpMesh(verts, faces, Ts, dev, 0.05, 0.05, True)
    pouts = {"float": dict(), "half": dict()}

    def frame(k):
        nsr_ops.render_rays(field, ro, rd, 32, 32, 1.6, inv_s, out=pouts[k], warp=wm, skip_masked=True, table_dtype=k)
    r = summary(alternate({"float": lambda: frame("float"), "half": lambda: frame("half")}, a.rounds, a.warmup))
    r["image_linf_half_vs_float"] = float((pouts["float"]["image"] - pouts["half"]["image"]).abs().max())
    res["posed_256x256_32+32_one_batch"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
