"""Making the decimated, welded mesh manifold on the device (mesh_repair.mesh_repair, ac_mesh_repair_count / _emit; csrc/mesh_repair.hip) against the host route
-- the numpy restatement of tests/mesh_repair_cases.py -- and what manifold=True costs the whole export; does not touch bench.py.

    python tools/bench_mesh_repair.py [--cases 512 2048/64] [--k 2 4] [--rounds 7] [--rough] [--out profiles/mesh_repair.txt]

Field: the synthetic field (synthetic.load_field_params; --rough: its rough table), in a NeRFNetwork.  A case is RES (the dense route) or RES/S
(extract_geometry(slab_layers=S)).  Per case and k, on the mesh of extract_geometry(1.6, RES, decimate=k) with export_weld, TIMED:
  repair                 : mesh_repair.mesh_repair, the whole call -- the float32 copy of the positions, the table fill, the use lists, the hooking pass, the flatten, the
                           scans and ordered writes, the one 32-byte read-back, scratch and outputs allocated in the call
  count_entry / emit_entry : the C entries alone, on float32 positions, a scratch and outputs that are kept (the launches)
  host_repair            : the same result by the numpy restatement on the host INCLUDING both copies (positions and triangles down, triangles and source up)
  export_weld / export_manifold : drivers.export_mesh(net, x.ply, resolution=RES, decimate=k, weld=True) without and with manifold=True, whole calls, the file
                           written to a temporary directory
The forms are warmed up once (the tool ASSERTS there that the device's triangles, source and counts equal numpy's), then timed alternating round by round: HIP events
on the current stream for the device forms, the wall clock between two device synchronisations for the host route and the whole exports.  Median and spread of
`rounds`.  NOT timed, per case and k: the report, the topology before and after, the scratch bytes.
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
from avatarcraft_amd import drivers, mesh_repair, mesh_weld
from tests import mesh_repair_cases
from tools.bench_mesh_decimate import BOUND, make_net, stats


def host_repair(verts, tris):
    """the host route: positions and triangles to the host, the numpy restatement, the new triangles and `source` back to the device"""
    r = mesh_repair_cases.repair(verts.cpu().numpy(), tris.cpu().numpy())
    return torch.from_numpy(r["triangles"]).to(tris.device), torch.from_numpy(r["source"]).to(tris.device), r["report"]


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
        raise SystemExit("bench_mesh_repair: needs a GPU (there is no CPU path to time)")
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    net = make_net(dev, a.rough)
    sync = lambda: torch.cuda.synchronize(dev)
    tmp = tempfile.mkdtemp(prefix="bench_mesh_repair_")
    for case in a.cases:
        R, S = (int(x) for x in case.split("/")) if "/" in case else (int(case), None)
        for k in a.k:
            net.export_weld = True
            try:
                with torch.no_grad():
                    verts, tris = net.extract_geometry(BOUND, R, return_torch=True, slab_layers=S, decimate=k)
            finally:
                del net.export_weld
            V, T = verts.shape[0], tris.shape[0]
            r = mesh_repair.mesh_repair(verts, tris)                                    # warm-up + parity: the same triangles, the same source, the same counts
            t_host, s_host, rep_host = host_repair(verts, tris)
            assert torch.equal(t_host, r["triangles"]) and torch.equal(s_host, r["source"]) and rep_host == r["report"], f"{case} k={k}: the device's repair differs from numpy's"
            before = mesh_weld.mesh_topology(tris, V)
            after = mesh_weld.mesh_topology(r["triangles"], r["report"]["vertices"])
            report = dict(tool="bench_mesh_repair", case=case, k=k, rough=bool(a.rough), vertices=V, triangles=T, repair=r["report"], topology_before=before,
                          topology_after=after)
            del t_host, s_host
            export = lambda manifold: drivers.export_mesh(net, os.path.join(tmp, "m.ply"), BOUND, R, slab_layers=S, decimate=k, weld=True,
                                                          **(dict(manifold=True) if manifold else {}))
            for m in (False, True):
                export(m)
            sync()
            ms = dict(repair=[], count_entry=[], emit_entry=[], host_repair=[], export_weld=[], export_manifold=[])

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
            need = int(lib.ac_mesh_repair_scratch(V, T))
            v32 = verts.to(torch.float32)
            nv = r["report"]["vertices"]
            scratch, counts = torch.empty(need, dtype=torch.uint8, device=dev), torch.empty(8, dtype=torch.int32, device=dev)
            outs = (torch.empty((T, 3), dtype=torch.int32, device=dev), torch.empty(nv, dtype=torch.int32, device=dev))
            head = (v32.data_ptr(), tris.data_ptr(), T, V, scratch.data_ptr(), need)
            for _ in range(a.rounds):
                events("count_entry", lambda: L.check(lib.ac_mesh_repair_count(*head, counts.data_ptr(), st), "mesh_repair_count"))
                events("emit_entry", lambda: L.check(lib.ac_mesh_repair_emit(*head, outs[0].data_ptr(), outs[1].data_ptr(), nv, st), "mesh_repair_emit"))
            sync()
            assert torch.equal(outs[0], r["triangles"]) and torch.equal(outs[1], r["source"])
            del scratch, counts, outs, v32
            for _ in range(a.rounds):
                events("repair", lambda: mesh_repair.mesh_repair(verts, tris))
                wall("host_repair", lambda: host_repair(verts, tris))
                wall("export_weld", lambda: export(False))
                wall("export_manifold", lambda: export(True))
            report.update(rounds=a.rounds, equal_to_numpy=True, forms={f: stats(x) for f, x in ms.items()}, repair_scratch_bytes=need)
            f = report["forms"]
            report["host_over_device_repair"] = round(f["host_repair"]["ms_median"] / f["repair"]["ms_median"], 2)
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
