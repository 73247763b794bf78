"""Timing of the ambient occlusion (csrc/mesh_occlusion.hip) on the mesh of the reference's one export call, extract_geometry(1.6, 512), of the golden net (the
synthetic field), projected onto the level set by extract_colored_mesh, with the default kit (8 directions x 4 taps, radius 0.1 bound):
    field_occlusion   ac_field_occlusion over the mesh's vertices (one launch: K J evaluations per tile)
    chain             the same arithmetic from operators the library had before: torch forms the frame and the taps, K J nsr_ops.field_sdf launches, torch takes
                      the min and the sum (`chain_equal`: bit-identical to field_occlusion -- asserted)
    bake_texture      ac_mesh_bake_texture, 4096^2 atlas, 3 Newton steps: the bake without occlusion
    bake_maps         ac_mesh_bake_maps with the kit: the same bake plus the occlusion of every owned texel, in one launch
HIP events around `inner` back-to-back calls, the forms alternating, median over the rounds; also the histogram of the vertices' occlusion in ten bins; one JSON
line.  python tools/bench_mesh_occlusion.py [--rounds 10] [--inner 1] [--resolution 512] [--size 4096]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import nsr_ops
from avatarcraft_amd.geometry import atlas_layout
from avatarcraft_amd.mesh_occlusion import field_occlusion, mesh_bake_maps, occlusion_kit
from bench_mesh_attrs import BOUND, EPS, TOL, golden_net


def chain_occlusion(field, points, normals, kit, bound):
    """ac_field_occlusion from what the library had before it: every operation one torch kernel (rounded once), the SDF through nsr_ops.field_sdf"""
    const = lambda v: torch.full((), float(v), device=points.device)
    lo, hi, zero, one = const(-bound), const(bound), const(0.0), const(1.0)
    p = points.clamp(-bound, bound)
    nx, ny, nz = normals.unbind(1)
    sg = torch.copysign(torch.ones_like(nz), nz)
    a = torch.full_like(nz, -1.0) / (sg + nz)
    b = (nx * ny) * a
    T = torch.stack([1.0 + sg * ((nx * nx) * a), sg * b, -(sg * nx)], 1)
    U = torch.stack([b, sg + (ny * ny) * a, -ny], 1)
    acc = torch.zeros_like(nz)
    gain, level = float(np.float32(kit["gain"])), float(np.float32(kit["level"]))
    for k in range(len(kit["dirs"])):
        lx, ly, lz = (float(v) for v in kit["dirs"][k])
        w = (lx * T + ly * U) + lz * normals
        v = torch.ones_like(nz)
        for j in range(len(kit["dists"])):
            t = kit["dists"][j]
            q = torch.fmin(torch.fmax(p + float(t) * w, lo), hi)
            s = nsr_ops.field_sdf(field, q.contiguous(), bound)[:, 0] - level
            h = const(t * kit["dirs"][k, 2])                                            # (the fp32 product; on the device: torch divides by a host scalar
            v = torch.fmin(v, torch.fmin(torch.fmax((gain * s) / h, zero), one))        #  by multiplying with its reciprocal, which rounds twice)
        acc = acc + float(kit["weights"][k]) * v
    return torch.fmin(acc, one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=1)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_occlusion: needs a GPU (there is no CPU path to time)")
    if a.rounds < 10:
        raise SystemExit("bench_mesh_occlusion: at least 10 rounds")
    dev = torch.device("cuda:0")
    net = golden_net(dev)
    kit = occlusion_kit(0.1 * BOUND)
    with torch.no_grad():
        m = net.extract_colored_mesh(BOUND, a.resolution, return_torch=True)
        pos, nrm, tris = m["vertices"].float(), m["normals"], m["triangles"]
        T, S = int(tris.shape[0]), a.size
        c = atlas_layout(T, S)["cell"]
        field = net._field()
        how = dict(refine_steps=3, tol=TOL, max_move=2.0 * BOUND / (a.resolution - 1.0))
        forms = {"field_occlusion_ms": lambda: field_occlusion(field, pos, nrm, BOUND, kit),
                 "chain_field_sdf_ms": lambda: chain_occlusion(field, pos, nrm, kit, BOUND),
                 "bake_texture_ms": lambda: nsr_ops.mesh_bake_texture(field, pos, tris, S, c, BOUND, EPS, **how),
                 "bake_maps_ms": lambda: mesh_bake_maps(field, pos, tris, S, c, BOUND, EPS, kit=kit, want=("rgb", "sdf", "status"), **how)}
        for fn in forms.values():                                          # warm-up: code objects, the allocator's blocks of every shape
            for _ in range(2):
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
        one, ref = forms["field_occlusion_ms"](), forms["chain_field_sdf_ms"]()
        equal = bool(torch.equal(one, ref))
        tex, maps = forms["bake_texture_ms"](), forms["bake_maps_ms"]()
        shared = all(torch.equal(tex[k], maps[k]) for k in ("rgb", "owner", "sdf", "status"))
        owned = maps["owner"] >= 0
        hist = torch.histc(one, bins=10, min=0.0, max=1.0).long().tolist()
        thist = torch.histc(maps["occlusion"][owned], bins=10, min=0.0, max=1.0).long().tolist()
    res = {"tool": "bench_mesh_occlusion", "resolution": a.resolution, "V": int(pos.shape[0]), "triangles": T, "size": S, "cell": int(c),
           "owned_texels": int(owned.sum()), "directions": int(len(kit["dirs"])), "taps": int(len(kit["dists"])), "radius": float(kit["dists"][-1]),
           "rounds": a.rounds, "inner": a.inner}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 3)
        res[k.replace("_ms", "_min_max_ms")] = [round(min(v), 3), round(max(v), 3)]
    res.update(chain_equal=equal, bake_shared_outputs_equal=bool(shared), vertex_occlusion_histogram=hist, vertex_occlusion_mean=round(float(one.mean()), 4),
               texel_occlusion_histogram=thist)
    print(json.dumps(res))
    assert equal, "bench_mesh_occlusion: the chained form and the kernel differ"
    assert shared, "bench_mesh_occlusion: ac_mesh_bake_maps and ac_mesh_bake_texture differ in what they share"
    assert res["field_occlusion_ms"] < res["chain_field_sdf_ms"], "bench_mesh_occlusion: the kernel is not faster than the chain of launches"


if __name__ == "__main__":
    main()
