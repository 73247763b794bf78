"""Cleaning the exported mesh on the device (nsr_ops.mesh_components / mesh_compact, ac_mesh_components / ac_mesh_compact_*; csrc/mesh_components.hip) against the
host route every mesh tool offers; does not touch bench.py.

    python tools/bench_mesh_components.py [--cases 512 2048/64] [--rounds 7] [--rough] [--contention 1000000] [--out profiles/mesh_components.txt]

Field: the synthetic field (synthetic.load_field_params; --rough: its rough table, which has floaters), in a NeRFNetwork.  A case is RES (the dense route) or RES/S
(extract_geometry(slab_layers=S)).  Per case, on the mesh of extract_geometry(1.6, RES):
  label      : nsr_ops.mesh_components -- union-find, ranks, the size table, its one 8-byte read-back
  compact    : nsr_ops.mesh_compact keeping the largest component -- flags, scans, ordered writes, its one 8-byte read-back
  host_scipy : the same labelling by scipy.sparse.csgraph.connected_components on the host INCLUDING both copies (triangles down, labels up), in this process
  export     : extract_colored_mesh(..., components=None) and (..., components="largest"), whole calls
The forms are warmed up once (the tool ASSERTS there that the device's partition equals scipy's), then timed alternating round by round: HIP events on the
current stream for the device forms, the wall clock between two device synchronisations for the host route and the whole exports.  The report has the median and
the spread of `rounds`, C and the five largest components.  One JSON line per case, appended to --out.
Before the cases, --contention N times the labelling alone on N triangles shaped as a fan (every hook on one word), a strip and disjoint triangles: what the
integer compare-exchange costs under contention on this chip."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import nsr_ops, synthetic
from avatarcraft_amd.geometry import select_components
from avatarcraft_amd.instant_nsr import NeRFNetwork

BOUND = 1.6


def make_net(dev, rough):
    p = synthetic.load_field_params()
    torch.manual_seed(0)
    net = NeRFNetwork()
    sd = {k: torch.from_numpy(np.asarray(p[k])) for k in p if k.startswith(("sdf_net", "color_net", "deviation_net"))}
    sd["encoder.embeddings"] = torch.from_numpy(synthetic.field_table(p, rough))
    sd["encoder.offsets"] = torch.from_numpy(np.asarray(p["offsets"]))
    net.load_state_dict(sd, strict=True)
    return net.to(dev).eval()


def host_labels(tris, V):
    """the host route: triangles to the host, scipy's connected components over their edges, the labels back to the device"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = tris.cpu().numpy()
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]])                                  # (two edges join a triangle's three vertices)
    n, lab = connected_components(coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(V, V)), directed=False)
    return n, torch.from_numpy(lab.astype(np.int32)).to(tris.device)


def stats(x):
    return dict(ms_median=round(float(np.median(x)), 4), ms_min=round(float(min(x)), 4), ms_max=round(float(max(x)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["512", "2048/64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rough", action="store_true")
    ap.add_argument("--contention", type=int, default=1000000, help="triangles of the synthetic contention meshes (0: skip them)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_components: needs a GPU (there is no CPU path to time)")
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    net = make_net(dev, a.rough)
    sync = lambda: torch.cuda.synchronize(dev)
    if a.contention:
        # what the integer compare-exchange costs under contention: the same number of triangles as a fan (every hook and every find lands on ONE word), a strip
        # (a wave hooks a chain, neighbours contend) and disjoint triangles (no two hooks share a word) -- label times, whole calls with their read-back
        n = a.contention
        i = torch.arange(n, dtype=torch.int32, device=dev)
        shapes = dict(fan=(torch.stack([torch.full_like(i, 2 * n), 2 * i, 2 * i + 1], dim=1).contiguous(), 2 * n + 1),
                      strip=(torch.stack([i, i + 1, i + 2], dim=1).contiguous(), n + 2),
                      strip_descending=((n + 1 - torch.stack([i, i + 1, i + 2], dim=1)).contiguous(), n + 2),
                      disjoint=(torch.arange(3 * n, dtype=torch.int32, device=dev).reshape(n, 3), 3 * n))
        times = {k: [] for k in shapes}
        for rnd in range(a.rounds + 1):                                                # (round 0: warm-up)
            for k, (t, V) in shapes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); r = nsr_ops.mesh_components(t, V); e1.record()
                e1.synchronize()
                assert r["n_components"] == (n if k == "disjoint" else 1)
                if rnd:
                    times[k].append(e0.elapsed_time(e1))
        line = json.dumps(dict(tool="bench_mesh_components", case="contention", triangles=n, rounds=a.rounds, label={k: stats(x) for k, x in times.items()}))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        del shapes
    for case in a.cases:
        R, S = (int(x) for x in case.split("/")) if "/" in case else (int(case), None)
        with torch.no_grad():
            verts, tris = net.extract_geometry(BOUND, R, return_torch=True, slab_layers=S)
        V, T = verts.shape[0], tris.shape[0]
        del verts
        cc = nsr_ops.mesh_components(tris, V)
        sizes = cc["sizes"].cpu().numpy()
        keep = torch.from_numpy(select_components(sizes, "largest")).to(dev)
        n_host, lab_host = host_labels(tris, V)                                       # warm-up + parity: the same partition
        pairs = torch.unique(torch.stack([lab_host.long(), cc["component"].long()], dim=1), dim=0)
        assert n_host == cc["n_components"] == pairs.shape[0], f"{case}: the device finds {cc['n_components']} components, scipy {n_host}, {pairs.shape[0]} label pairs"
        cm = nsr_ops.mesh_compact(tris, cc["component"], keep)
        kept = (int(cm["kept_vertices"].shape[0]), int(cm["triangles"].shape[0]))
        export = lambda spec: net.extract_colored_mesh(BOUND, R, return_torch=True, slab_layers=S, components=spec)
        for spec in (None, "largest"):
            export(spec)
        del lab_host, cm, pairs
        sync()
        ms = dict(label=[], compact=[], host_scipy=[], export_all=[], export_largest=[])

        def events(key, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = fn(); e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1))
            del out

        def wall(key, fn):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            ms[key].append((time.perf_counter() - t0) * 1e3)
            del out
        for _ in range(a.rounds):
            events("label", lambda: nsr_ops.mesh_components(tris, V))
            events("compact", lambda: nsr_ops.mesh_compact(tris, cc["component"], keep))
            wall("host_scipy", lambda: host_labels(tris, V))
            wall("export_all", lambda: export(None))
            wall("export_largest", lambda: export("largest"))
        order = np.argsort(-sizes[:, 1], kind="stable")[:5]
        report = dict(tool="bench_mesh_components", case=case, rough=bool(a.rough), vertices=V, triangles=T, components=int(cc["n_components"]),
                      largest=[[int(sizes[i, 0]), int(sizes[i, 1])] for i in order], kept_vertices=kept[0], kept_triangles=kept[1], rounds=a.rounds,
                      partition_equal_to_scipy=True, forms={k: stats(x) for k, x in ms.items()})
        report["host_over_device_label"] = round(report["forms"]["host_scipy"]["ms_median"] / report["forms"]["label"]["ms_median"], 2)
        line = json.dumps(report)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        del tris, cc, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
