"""Welding the decimated mesh and reporting its topology on the device (mesh_weld.mesh_weld / mesh_topology, ac_mesh_weld_count / _emit, ac_mesh_topology;
csrc/mesh_weld.hip) against the host route a user has today, and what weld=True costs the whole export; does not touch bench.py.

    python tools/bench_mesh_weld.py [--cases 512 2048/64] [--k 2 4] [--rounds 7] [--rough] [--out profiles/mesh_weld.txt]

Field: the synthetic field (synthetic.load_field_params; --rough: its rough table), in a NeRFNetwork.  A case is RES (the dense route) or RES/S
(extract_geometry(slab_layers=S)).  Per case and k, on the triangles of extract_geometry(1.6, RES, decimate=k), TIMED:
  weld / topology        : mesh_weld.mesh_weld and mesh_weld.mesh_topology, whole calls -- the table fill, the flag pass, scans and ordered writes, the one 32-byte
                           read-back, scratch and outputs allocated in the call
  weld_count_entry / weld_emit_entry / topology_entry : the C entries alone, on a scratch and outputs that are kept (the launches)
  host_weld / host_topology : the same results by numpy.unique over sorted triples / (min, max) edge pairs on the host INCLUDING both copies (triangles down, the
                           result up), in this process
  export / export_weld   : drivers.export_mesh(net, x.ply, resolution=RES, decimate=k) without and with weld=True, whole calls, the file written to a temporary directory
The forms are warmed up once (the tool ASSERTS there that the device's survivors and counts equal numpy's), then timed alternating round by round: HIP events on the
current stream for the device forms, the wall clock between two device synchronisations for the host routes and the whole exports.  Median and spread of `rounds`.
NOT timed, per case and k: the weld's report, the topology before and after, the scratch bytes of both.
One JSON line per case and k, appended to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import _lib as L
from avatarcraft_amd import drivers, mesh_weld
from tools.bench_mesh_decimate import BOUND, make_net, stats


def host_weld(tris, V):
    """the host route of the weld: triangles to the host, groups by numpy.unique on sorted triples, the two leaders by minimum.at, the survivors' indices and the
    vertex map back to the device -> (kept_triangles, vertex_map) on the device"""
    t = tris.cpu().numpy().astype(np.int64)
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    idx = np.flatnonzero(ok)
    m = t[idx]
    r = np.argmin(m, axis=1)
    plus = np.take_along_axis(m, ((r + 1) % 3)[:, None], 1)[:, 0] < np.take_along_axis(m, ((r + 2) % 3)[:, None], 1)[:, 0]
    s = np.sort(m, axis=1)
    _, inv = np.unique((s[:, 0] * V + s[:, 1]) * V + s[:, 2], return_inverse=True)         # (V^3 < 2^63 up to V = 2 097 151: every mesh timed here)
    inv = inv.reshape(-1)
    G = int(inv.max()) + 1 if len(inv) else 0
    lead = np.full((2, G), len(t), np.int64)
    np.minimum.at(lead[0], inv[plus], idx[plus])
    np.minimum.at(lead[1], inv[~plus], idx[~plus])
    net = np.bincount(inv[plus], minlength=G) - np.bincount(inv[~plus], minlength=G)
    kept = np.sort(np.where(net > 0, lead[0], lead[1])[net != 0])
    used = np.zeros(V, bool)
    used[t[kept].reshape(-1)] = True
    vmap = np.full(V, -1, np.int32)
    vmap[used] = np.arange(int(used.sum()), dtype=np.int32)
    return torch.from_numpy(kept.astype(np.int32)).to(tris.device), torch.from_numpy(vmap).to(tris.device)


def host_topology(tris, V):
    """the host route of the report: triangles to the host, edges by numpy.unique on (min, max) -> (E, boundary, nonmanifold, misoriented)"""
    t = tris.cpu().numpy().astype(np.int64)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    fwd = e[:, 0] < e[:, 1]
    uniq, inv = np.unique(e.min(axis=1) * V + e.max(axis=1), return_inverse=True)
    inv = inv.reshape(-1)
    f, b = np.bincount(inv[fwd], minlength=len(uniq)), np.bincount(inv[~fwd], minlength=len(uniq))
    return len(uniq), int((f + b == 1).sum()), int((f + b > 2).sum()), int(((f + b == 2) & (f != b)).sum())


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
        raise SystemExit("bench_mesh_weld: needs a GPU (there is no CPU path to time)")
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    net = make_net(dev, a.rough)
    sync = lambda: torch.cuda.synchronize(dev)
    tmp = tempfile.mkdtemp(prefix="bench_mesh_weld_")
    for case in a.cases:
        R, S = (int(x) for x in case.split("/")) if "/" in case else (int(case), None)
        for k in a.k:
            with torch.no_grad():
                verts, tris = net.extract_geometry(BOUND, R, return_torch=True, slab_layers=S, decimate=k)
            V, T = verts.shape[0], tris.shape[0]
            r = mesh_weld.mesh_weld(tris, V)                                          # warm-up + parity: the same survivors, the same map, the same edge counts
            kept_host, vmap_host = host_weld(tris, V)
            assert torch.equal(kept_host, r["kept_triangles"]) and torch.equal(vmap_host, r["vertex_map"]), f"{case} k={k}: the device's weld differs from numpy's"
            before = mesh_weld.mesh_topology(tris, V)
            assert host_topology(tris, V) == tuple(before[x] for x in ("edges", "boundary", "nonmanifold", "misoriented")), f"{case} k={k}: the report differs from numpy's"
            after = mesh_weld.mesh_topology(r["triangles"], r["report"]["vertices"])
            report = dict(tool="bench_mesh_weld", case=case, k=k, rough=bool(a.rough), vertices=V, triangles=T, weld=r["report"], topology_before=before,
                          topology_after=after)
            del kept_host, vmap_host
            export = lambda weld: drivers.export_mesh(net, os.path.join(tmp, "m.ply"), BOUND, R, slab_layers=S, decimate=k, **(dict(weld=True) if weld else {}))
            for w in (False, True):
                export(w)
            sync()
            ms = dict(weld=[], topology=[], weld_count_entry=[], weld_emit_entry=[], topology_entry=[], host_weld=[], host_topology=[], export=[], export_weld=[])

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
            lib, st = L.lib(), L.current_stream(dev)
            need_w, need_t = int(lib.ac_mesh_weld_scratch(V, T)), int(lib.ac_mesh_topology_scratch(V, T))
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
            scratch, scratch_t, counts = torch.empty(need_w, dtype=torch.uint8, device=dev), torch.empty(need_t, dtype=torch.uint8, device=dev), i32(8)
            head = (tris.data_ptr(), T, V, scratch.data_ptr(), need_w)
            nv, nt = r["report"]["vertices"], r["report"]["triangles"]
            outs = (i32(V), i32(nv), i32(nt, 3), i32(nt))
            emit_args = (outs[0].data_ptr(), outs[1].data_ptr(), nv, outs[2].data_ptr(), outs[3].data_ptr(), nt)
            for _ in range(a.rounds):
                events("weld_count_entry", lambda: L.check(lib.ac_mesh_weld_count(*head, counts.data_ptr(), st), "mesh_weld_count"))
                events("weld_emit_entry", lambda: L.check(lib.ac_mesh_weld_emit(*head, *emit_args, st), "mesh_weld_emit"))
                events("topology_entry", lambda: L.check(lib.ac_mesh_topology(tris.data_ptr(), T, V, scratch_t.data_ptr(), need_t, counts.data_ptr(), st), "mesh_topology"))
            sync()
            del scratch, scratch_t, counts, outs
            for _ in range(a.rounds):
                events("weld", lambda: mesh_weld.mesh_weld(tris, V))
                events("topology", lambda: mesh_weld.mesh_topology(tris, V))
                wall("host_weld", lambda: host_weld(tris, V))
                wall("host_topology", lambda: host_topology(tris, V))
                wall("export", lambda: export(False))
                wall("export_weld", lambda: export(True))
            report.update(rounds=a.rounds, equal_to_numpy=True, forms={f: stats(x) for f, x in ms.items()}, weld_scratch_bytes=need_w, topology_scratch_bytes=need_t)
            f = report["forms"]
            report["host_over_device_weld"] = round(f["host_weld"]["ms_median"] / f["weld"]["ms_median"], 2)
            report["host_over_device_topology"] = round(f["host_topology"]["ms_median"] / f["topology"]["ms_median"], 2)
            line = json.dumps(report)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
            del verts, tris, r
            torch.cuda.empty_cache()
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
