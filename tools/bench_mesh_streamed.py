"""Dense against streamed mesh extraction (nsr_ops.marching_cubes_streamed, ac_marching_cubes_slab_*; csrc/marching_cubes.hip); does not touch bench.py.

    python tools/bench_mesh_streamed.py [--resolutions 512 1024 2048] [--dense-up-to 1024] [--slabs 16 32 64 128] [--rounds 7] [--out profiles/mesh_streamed.txt]

Field: the synthetic field (synthetic.device_field), -sdf on resolution^3 points over [-1.6, 1.6]^3.  Per resolution the forms
  dense       : field_sdf_grid of the whole volume + marching_cubes (what extract_geometry(slab_layers=None) runs; only up to --dense-up-to: 9 B per grid point,
                and 2^31 points are refused from 1291^3)
  streamed/S  : marching_cubes_streamed with fill = field_sdf_grid of S x-layers into the window (what extract_geometry(slab_layers=S) runs)
are warmed up once (where a dense form runs, the tool ASSERTS there that every streamed mesh equals the dense one bit for bit), run once more alone for their peak
of torch.cuda.max_memory_allocated above the level at entry, and then timed with HIP events on the current stream, alternating round by round in one process;
the report has the median and the spread of `rounds`.  One JSON line per resolution, appended to --out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import nsr_ops, synthetic

BOUND = 1.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--dense-up-to", type=int, default=1024)
    ap.add_argument("--slabs", type=int, nargs="+", default=[16, 32, 64, 128])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    field, _ = synthetic.device_field(device=a.device)
    span, lo = [float(np.float32(BOUND) - np.float32(-BOUND))] * 3, [float(np.float32(-BOUND))] * 3
    for R in a.resolutions:
        ax = torch.linspace(-BOUND, BOUND, R).to(dev)
        xf = dict(den=R - 1.0, span=span, lo=lo)

        def dense():
            u = nsr_ops.field_sdf_grid(field, ax, ax, ax, BOUND, negate=True)
            return nsr_ops.marching_cubes(u, 0.0, **xf)

        def streamed(S):
            fill = lambda x0, out: nsr_ops.field_sdf_grid(field, ax[x0:x0 + out.shape[0]], ax, ax, BOUND, negate=True, out=out)
            return lambda: nsr_ops.marching_cubes_streamed(fill, R, R, R, slab_layers=S, iso=0.0, device=dev, **xf)
        forms = {"dense": dense} if R <= a.dense_up_to else {}
        forms.update({f"streamed/{S}": streamed(S) for S in a.slabs if (min(S, R) + 2) * R * R < 2 ** 31})
        ref, counts, peak = None, None, {}
        for k, fn in forms.items():                              # warm-up + parity, then the peak of a run alone
            v, t = fn()
            torch.cuda.synchronize(dev)
            if k == "dense":
                ref = (v, t)
            elif ref is not None:
                assert v.shape == ref[0].shape and torch.equal(t, ref[1]) and torch.equal(v.view(torch.int64), ref[0].view(torch.int64)), \
                    f"{k} at {R}^3 is not the dense mesh bit for bit"
            assert counts in (None, (v.shape[0], t.shape[0])), f"{k} at {R}^3: {v.shape[0]} vertices / {t.shape[0]} triangles, the form before it {counts}"
            counts = (v.shape[0], t.shape[0])
            del v, t
            if k != "dense":
                torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            out = fn()
            torch.cuda.synchronize(dev)
            peak[k] = torch.cuda.max_memory_allocated(dev) - base
            del out
        ref = None
        torch.cuda.empty_cache()
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out = fn(); e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
                del out
        report = dict(resolution=R, grid_points=R ** 3, vertices=counts[0], triangles=counts[1], mesh_bytes=counts[0] * 24 + counts[1] * 12, rounds=a.rounds,
                      equal_to_dense_bit_for_bit=("dense" in forms) or None,
                      forms={k: dict(ms_median=float(np.median(x)), ms_min=float(min(x)), ms_max=float(max(x)), peak_bytes=int(peak[k]),
                                     windows=None if k == "dense" else len(nsr_ops.slab_windows(R, int(k.split("/")[1])))) for k, x in ms.items()})
        line = json.dumps(report)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
