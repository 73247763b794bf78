"""Decimating the exported mesh on the device (mesh_decimate.mesh_cluster, ac_mesh_cluster_count / _emit; csrc/mesh_cluster.hip) against the host route a user has
today, and what the decimated export costs and keeps; does not touch bench.py.

    python tools/bench_mesh_decimate.py [--cases 512 2048/64] [--k 2 4] [--rounds 7] [--rough] [--out profiles/mesh_decimate.txt]

Field: the synthetic field (synthetic.load_field_params; --rough: its rough table), in a NeRFNetwork.  A case is RES (the dense route) or RES/S
(extract_geometry(slab_layers=S)).  Per case and k, on the mesh of extract_geometry(1.6, RES), TIMED:
  cluster    : mesh_decimate.mesh_cluster -- table fill, scans, ordered writes, its one 16-byte read-back (count + emit), its scratch and outputs allocated in the call
  cluster_alone : the same call back to back, nothing in between (what it costs when the allocator's state is not disturbed by whole exports)
  count_entry / emit_entry : ac_mesh_cluster_count and ac_mesh_cluster_emit alone, on a scratch and outputs that are kept (the launches)
  host_numpy : the same clustering by numpy.unique on the host INCLUDING both copies (vertices down, cluster ids up), in this process
  export     : drivers.export_mesh(net, x.ply, resolution=RES) with decimate=None and decimate=k, whole calls, the file written to a temporary directory
The forms are warmed up once (the tool ASSERTS there that the device's partition equals numpy's), then timed alternating round by round: HIP events on the current
stream for the device form, the wall clock between two device synchronisations for the host route and the whole exports.  Median and spread of `rounds`.
NOT timed, per case and k: vertices and triangles before and after; the status histogram of the projection (extract_colored_mesh's status: 0 converged, 1 all steps
taken, 2 degenerate gradient, 3 stopped by the limit of one cell -- grid cell before, cluster cell after); max and median |sdf| at the triangle centroids of the
projected mesh before and after (what flat triangles of that size miss of the surface); the duplicate triangles left (same orientation, back to back).
One JSON line per case and k, appended to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import _lib as L
from avatarcraft_amd import drivers, mesh_decimate, nsr_ops, synthetic
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


def host_clusters(verts, grid):
    """the host route: vertices to the host, the cell of each by the header's arithmetic, numpy.unique, the cluster ids (in key order) back to the device"""
    v = verts.cpu().numpy()
    lo, n = np.asarray(grid["lo"]), np.asarray(grid["n"], np.int64)
    c = np.minimum(np.floor((v - lo) / grid["h"]), n - 1).astype(np.int64)
    uniq, inv = np.unique((c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2], return_inverse=True)
    return len(uniq), torch.from_numpy(inv.reshape(-1).astype(np.int32)).to(verts.device)


def duplicates(tris):
    """(triangles that repeat an earlier one up to a rotation, back-to-back pairs), on the device"""
    if not tris.shape[0]:
        return 0, 0
    t = tris.long()
    r = t.argmin(dim=1, keepdim=True)
    rot = torch.cat([t.gather(1, (r + k) % 3) for k in range(3)], dim=1)
    n = int(t.max()) + 1
    key = lambda x: (x[:, 0] * n + x[:, 1]) * n + x[:, 2]
    ku = torch.unique(key(rot))
    back = torch.unique(key(rot[:, [0, 2, 1]]))
    return int(rot.shape[0] - ku.shape[0]), int(torch.isin(ku, back).sum()) // 2


def centroid_sdf(net, mesh):
    """|sdf| at the triangle centroids of a projected mesh: (max, median)"""
    v, t = mesh["vertices"].float(), mesh["triangles"].long()
    c = v[t].mean(dim=1).contiguous()
    with torch.no_grad():
        s = nsr_ops.field_sdf(net._field(), c, BOUND)
    s = (s[0] if isinstance(s, (tuple, list)) else s).reshape(c.shape[0], -1)[:, 0].abs()
    return float(s.max()), float(s.median())


def stats(x):
    return dict(ms_median=round(float(np.median(x)), 4), ms_min=round(float(min(x)), 4), ms_max=round(float(max(x)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["512", "2048/64"])
    ap.add_argument("--k", nargs="+", type=float, default=[2.0, 4.0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rough", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_decimate: needs a GPU (there is no CPU path to time)")
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    net = make_net(dev, a.rough)
    sync = lambda: torch.cuda.synchronize(dev)
    tmp = tempfile.mkdtemp(prefix="bench_mesh_decimate_")
    for case in a.cases:
        R, S = (int(x) for x in case.split("/")) if "/" in case else (int(case), None)
        with torch.no_grad():
            verts, tris = net.extract_geometry(BOUND, R, return_torch=True, slab_layers=S)
        V, T = verts.shape[0], tris.shape[0]
        before = net.extract_colored_mesh(BOUND, R, return_torch=True, slab_layers=S)
        sdf_before = centroid_sdf(net, before)
        status_before = torch.bincount(before["status"].long(), minlength=4).tolist()
        del before
        for k in a.k:
            grid = mesh_decimate.cluster_grid(BOUND, R, k)
            r = mesh_decimate.mesh_cluster(verts, tris, grid)
            n_host, lab_host = host_clusters(verts, grid)                             # warm-up + parity: the same partition
            pairs = torch.unique(torch.stack([lab_host.long(), r["cluster"].long()], dim=1), dim=0)
            assert n_host == r["leader"].shape[0] == pairs.shape[0], f"{case} k={k}: the device finds {r['leader'].shape[0]} clusters, numpy {n_host}, {pairs.shape[0]} label pairs"
            after = net.extract_colored_mesh(BOUND, R, return_torch=True, slab_layers=S, decimate=k)
            assert after["triangles"].shape[0] == r["triangles"].shape[0]
            report = dict(tool="bench_mesh_decimate", case=case, k=k, rough=bool(a.rough), vertices=V, triangles=T, vertices_after=int(after["vertices"].shape[0]),
                          triangles_after=int(after["triangles"].shape[0]), largest_cluster=int(r["members"].max()), status_before=status_before,
                          status_after=torch.bincount(after["status"].long(), minlength=4).tolist())
            report["centroid_abs_sdf_before"] = dict(max=sdf_before[0], median=sdf_before[1])
            m, md = centroid_sdf(net, after)
            report["centroid_abs_sdf_after"] = dict(max=m, median=md)
            same, back = duplicates(after["triangles"])
            report.update(duplicate_triangles=same, back_to_back_pairs=back, grid_cell=2.0 * BOUND / (R - 1.0), cluster_cell=grid["h"])
            del after, lab_host, pairs, r
            export = lambda dec: drivers.export_mesh(net, os.path.join(tmp, "m.ply"), BOUND, R, slab_layers=S, decimate=dec)
            for dec in (None, k):
                export(dec)
            sync()
            ms = dict(cluster=[], cluster_alone=[], count_entry=[], emit_entry=[], host_numpy=[], export_all=[], export_decimated=[])

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
                events("cluster_alone", lambda: mesh_decimate.mesh_cluster(verts, tris, grid))
            need = int(L.lib().ac_mesh_cluster_scratch(V, T))
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
            scratch, cluster, counts = torch.empty(need, dtype=torch.uint8, device=dev), i32(V), i32(4)
            g = L.ac_cluster_grid((C.c_double * 3)(*grid["lo"]), grid["h"], (C.c_uint32 * 3)(*grid["n"]))
            head, st = (verts.data_ptr(), V, tris.data_ptr(), T, C.byref(g), scratch.data_ptr(), need), L.current_stream(dev)
            L.check(L.lib().ac_mesh_cluster_count(*head, cluster.data_ptr(), counts.data_ptr(), st), "mesh_cluster_count")
            nc, nt = counts.tolist()[:2]
            outs = (i32(nc).data_ptr(), i32(nc).data_ptr(), torch.empty((nc, 3), dtype=torch.float64, device=dev).data_ptr(), nc, i32(nt, 3).data_ptr(), i32(nt).data_ptr(), nt)
            for _ in range(a.rounds):
                events("count_entry", lambda: L.check(L.lib().ac_mesh_cluster_count(*head, cluster.data_ptr(), counts.data_ptr(), st), "mesh_cluster_count"))
                events("emit_entry", lambda: L.check(L.lib().ac_mesh_cluster_emit(*head, *outs, st), "mesh_cluster_emit"))
            sync()
            del scratch, cluster, counts, outs
            for _ in range(a.rounds):
                events("cluster", lambda: mesh_decimate.mesh_cluster(verts, tris, grid))
                wall("host_numpy", lambda: host_clusters(verts, grid))
                wall("export_all", lambda: export(None))
                wall("export_decimated", lambda: export(k))
            report.update(rounds=a.rounds, partition_equal_to_numpy=True, forms={f: stats(x) for f, x in ms.items()})
            report["host_over_device_cluster"] = round(report["forms"]["host_numpy"]["ms_median"] / report["forms"]["cluster"]["ms_median"], 2)
            report["scratch_bytes"] = need
            line = json.dumps(report)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
        del verts, tris
        torch.cuda.empty_cache()
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
