"""Timing of ac_mesh_bake_texture on the mesh of the reference's one export call, extract_geometry(1.6, 512), of the golden net (the synthetic field), projected
onto the level set by extract_colored_mesh, in a 4096^2 atlas with the cell the layout picks itself:
    a      the kernel with 3 Newton steps (one launch: texel -> point, steps, normal, colour)
    chain  the same arithmetic from stand-alone operators: torch forms every owned texel's point from the same weights, then nsr_ops.field_samples four times with
           torch element-wise updates between, results scattered into the images (`chain_equal`: rgb, sdf, status and owner came out bit-identical to a -- asserted)
    c      the kernel with refine_steps = 0 (one stencil + colour per owned texel)
HIP events around `inner` back-to-back calls, the three forms alternating, median over the rounds; also the status histogram over the owned texels and the
owned fraction; one JSON line.
python tools/bench_texture_bake.py [--rounds 10] [--inner 1] [--resolution 512] [--size 4096]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import nsr_ops
from avatarcraft_amd.geometry import atlas_layout, atlas_owner, atlas_weights
from bench_mesh_attrs import BOUND, EPS, TOL, chain, golden_net


def chain_bake(field, pos, tris, owner, weights, cell, steps, max_move):
    """ac_mesh_bake_texture from what the library had before it.  owner [S,S] int32 and weights [c,c,3] are the closed-form layout (device copies of
    geometry.atlas_owner / atlas_weights); the points, the steps and the scatter are torch and ac_field_samples"""
    S = owner.shape[0]
    ys, xs = torch.nonzero(owner >= 0, as_tuple=True)
    t = owner[ys, xs].long()
    w = weights[ys % cell, xs % cell]
    P = pos[tris[t].long()]                                                           # [N,3 corners,3]
    p = (w[:, 0:1] * P[:, 0] + w[:, 1:2] * P[:, 1]) + w[:, 2:3] * P[:, 2]
    r = chain(field, p, steps, max_move)
    out = dict(rgb=torch.zeros((S, S, 3), device=pos.device), sdf=torch.zeros((S, S), device=pos.device), status=torch.zeros((S, S), dtype=torch.uint8, device=pos.device),
               owner=owner)
    for k in ("rgb", "sdf", "status"):
        out[k][ys, xs] = r[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=1)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture_bake: needs a GPU (there is no CPU path to time)")
    if a.rounds < 10:
        raise SystemExit("bench_texture_bake: at least 10 rounds")
    dev = torch.device("cuda:0")
    net = golden_net(dev)
    with torch.no_grad():
        m = net.extract_colored_mesh(BOUND, a.resolution, return_torch=True)
        pos, tris = m["vertices"].float(), m["triangles"]
        T, S = int(tris.shape[0]), a.size
        c = atlas_layout(T, S)["cell"]
        owner = torch.from_numpy(atlas_owner(T, S, c)).to(dev)
        weights = torch.from_numpy(atlas_weights(c)[1]).to(dev)
        field = net._field()
        cell = 2.0 * BOUND / (a.resolution - 1.0)
        bake = lambda steps: nsr_ops.mesh_bake_texture(field, pos, tris, S, c, BOUND, EPS, refine_steps=steps, tol=TOL, max_move=cell)
        forms = {"bake_3_steps_ms": lambda: bake(3),
                 "chain_4_field_samples_ms": lambda: chain_bake(field, pos, tris, owner, weights, c, 3, cell),
                 "bake_0_steps_ms": lambda: bake(0)}
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
        one, ref = forms["bake_3_steps_ms"](), forms["chain_4_field_samples_ms"]()
        equal = all(torch.equal(one[k], ref[k]) for k in ("rgb", "sdf", "status", "owner"))
        owned = one["owner"] >= 0
        hist = torch.bincount(one["status"][owned].long(), minlength=4).tolist()
        n_owned = int(owned.sum())
        max_sdf = float(one["sdf"][owned].abs().max())
    res = {"tool": "bench_texture_bake", "resolution": a.resolution, "V": int(pos.shape[0]), "triangles": T, "size": S, "cell": int(c), "texels": S * S,
           "owned_texels": n_owned, "owned_fraction": round(n_owned / float(S * S), 4), "rounds": a.rounds, "inner": a.inner}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 3)
        res[k.replace("_ms", "_min_max_ms")] = [round(min(v), 3), round(max(v), 3)]
    res.update(status_histogram=hist, chain_equal=bool(equal), max_abs_sdf=max_sdf)
    print(json.dumps(res))
    assert equal, "bench_texture_bake: the chained form and the kernel differ"


if __name__ == "__main__":
    main()
