"""Per-frame cost of posing the exported mesh (ac_mesh_pose, csrc/mesh_pose.hip); does not touch bench.py.

    python tools/bench_mesh_pose.py [--resolution 512] [--frame 5] [--rounds 10] [--out profiles/mesh_pose.txt]

Mesh: the synthetic field's level set at resolution^3 (field_sdf_grid + marching_cubes + mesh_vertex_attrs, geometry only).  Guide: synthetic.make_body_sequence
(SMPL-sized capsule, 6 891 vertices / 13 778 faces).  NOTE its rest transforms carry make_body's per-vertex noise (3 cm translation jitter): the fixed-point
iteration does not contract on it (tests/mesh_pose_cases.py), so the status histogram printed here shows the work done, not the convergence a smooth
body gives; --smooth removes the two noise terms.  The frame's WarpMesh (upload + culling structure) is built outside the timed region: in
drivers.export_animation it is prepared on a side stream beside the previous frame.
Timed with HIP events, median of `rounds`, the three forms alternating round by round:
  (a) nsr_ops.mesh_pose at iters = 3 (four closest-face searches + the step kernels, one call);
  (b) the same arithmetic with the searches launched from Python (the call ray_utils.warp_samples_to_canonical makes, plus the face index it does not
      return) and the steps as torch fp64 tensor operations; the tool asserts that (b)'s positions equal (a)'s bit for bit;
  (c) nsr_ops.mesh_pose at iters = 0 (the bound start and one search)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from avatarcraft_amd import _lib as L, nsr_ops, synthetic
from avatarcraft_amd.geometry import canonical_guide

BOUND = 1.6


def search(p, wm):
    """one closest-face search as ray_utils.warp_samples_to_canonical launches it -> can [V,3] f64, closest [V,3] f64, face [V] i32, mask [V] u8"""
    V, dev = p.shape[0], p.device
    can, clo = torch.empty((V, 3), dtype=torch.float64, device=dev), torch.empty((V, 3), dtype=torch.float64, device=dev)
    fid, mask = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.uint8, device=dev)
    L.check(L.lib().ac_warp_samples_accel(p.data_ptr(), wm.verts.data_ptr(), wm.faces.data_ptr(), wm.T.data_ptr(), V, wm.verts.shape[0], wm.faces.shape[0],
                                          float(wm.c.threshold), wm.accel.data_ptr(), can.data_ptr(), None, clo.data_ptr(), None, fid.data_ptr(), mask.data_ptr(),
                                          L.current_stream(dev)), "warp_samples_accel")
    return can, clo, fid, mask


def dot(u, v):
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]


def blend(T, tri, bc):
    return T[tri[:, 0]] * bc[:, 0, None, None] + T[tri[:, 1]] * bc[:, 1, None, None] + T[tri[:, 2]] * bc[:, 2, None, None]


def fwd(M, c64):
    k = M[:, 3, 3]
    return torch.stack([(M[:, r, 0] * c64[:, 0] + M[:, r, 1] * c64[:, 1]) + M[:, r, 2] * c64[:, 2] + M[:, r, 3] / k for r in range(3)], 1).float()


def torch_pose(c, bind, wm, iters, tol):
    """ac_mesh_pose's positions and status in torch fp64 (include/avatarcraft_hip.h, operation for operation)"""
    faces = wm.faces.long()
    c64 = c.double()
    p = fwd(blend(wm.T, faces[bind["face_id"].long()], bind["bary"]), c64)
    running = torch.ones(c.shape[0], dtype=torch.bool, device=c.device)
    status = torch.full((c.shape[0],), 255, dtype=torch.uint8, device=c.device)
    for k in range(iters + 1):
        can, clo, fid, _ = search(p, wm)
        d = (can - c64).abs()
        finite = torch.isfinite(d).all(1)
        r = torch.nan_to_num(d, nan=0.0, posinf=0.0).max(1).values
        st = torch.where(~finite, 2, torch.where(r <= float(np.float32(tol)), 0, 1 if k == iters else 255)).to(torch.uint8)
        tri = faces[fid.long()]
        a, b, cc = (wm.verts[tri[:, j]].double() for j in range(3))
        v0, v1, v2 = b - a, cc - a, clo - a
        d00, d01, d11, d20, d21 = dot(v0, v0), dot(v0, v1), dot(v1, v1), dot(v2, v0), dot(v2, v1)
        den = d00 * d11 - d01 * d01
        bv, bw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        M = blend(wm.T, tri, torch.stack([1.0 - bv - bw, bv, bw], 1))
        stop = running & (st != 255)
        status = torch.where(stop, st, status)
        running = running & ~stop
        p = torch.where(running[:, None], fwd(M, c64), p)
    return p, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--frame", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--smooth", action="store_true", help="rest transforms without make_body's per-vertex noise")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    dev = torch.device(a.device)
    field, _ = synthetic.device_field(device=a.device)
    ax = torch.linspace(-BOUND, BOUND, a.resolution).to(dev)
    u = nsr_ops.field_sdf_grid(field, ax, ax, ax, BOUND, negate=True)
    v, tris = nsr_ops.marching_cubes(u, 0.0, den=a.resolution - 1.0, span=[float(np.float32(BOUND) - np.float32(-BOUND))] * 3, lo=[float(np.float32(-BOUND))] * 3)
    del u
    at = nsr_ops.mesh_vertex_attrs(field, v, BOUND, refine_steps=3, max_move=2.0 * BOUND / (a.resolution - 1.0), want_rgb=False)
    pts, nrm = at["positions"], at["normals"]
    V = pts.shape[0]
    vs, faces, Ts = synthetic.make_body_sequence(n_frames=a.frame + 1)
    if a.smooth:                                           # make_body's transform field without its two noise terms; the bend of the frame is B = T T0^-1
        v0 = synthetic.make_body(n_lat=83, n_lon=83)
        ang = 0.35 * np.sin(2.0 * v0[0][:, 1].astype(np.float64))
        S0 = np.tile(np.eye(4)[None], (len(ang), 1, 1))
        S0[:, 0, 0] = np.cos(ang); S0[:, 0, 1] = -np.sin(ang); S0[:, 1, 0] = np.sin(ang); S0[:, 1, 1] = np.cos(ang)
        S0 = S0 @ (np.eye(4) / 0.9)
        Ts = [T @ np.linalg.inv(v0[2]) @ S0 for T in Ts]
    guide = torch.from_numpy(canonical_guide(vs[0], Ts[0])).to(dev)
    wm = nsr_ops.WarpMesh(vs[a.frame], faces, Ts[a.frame], dev)
    bind = nsr_ops.mesh_bind(pts, guide, wm.faces)
    forms = {"a": lambda: nsr_ops.mesh_pose(pts, nrm, bind, wm, iters=a.iters, tol=a.tol),
             "b": lambda: torch_pose(pts, bind, wm, a.iters, a.tol),
             "c": lambda: nsr_ops.mesh_pose(pts, nrm, bind, wm, iters=0, tol=a.tol)}
    ra, rb = forms["a"](), forms["b"]()                   # warm-up of (a) and (b) + the parity check
    forms["c"]()
    torch.cuda.synchronize(dev)
    assert torch.equal(ra["positions"].view(torch.int32), rb[0].view(torch.int32)), "form (b) does not reproduce ac_mesh_pose's positions bit for bit"
    assert torch.equal(ra["status"], rb[1])
    ms = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    hist = torch.bincount(ra["status"].long(), minlength=3).tolist()
    res = ra["residual"].double()
    report = dict(vertices=V, triangles=int(tris.shape[0]), guide_faces=int(wm.faces.shape[0]), frame=a.frame, iters=a.iters, tol=a.tol, smooth=bool(a.smooth),
                  rounds=a.rounds, ms_mesh_pose=med["a"], ms_torch_steps=med["b"], ms_iters0=med["c"], status_hist=hist,
                  masked_out=int((ra["mask"] == 0).sum()), residual_median=float(res.median()), residual_p99=float(res.quantile(0.99)) if V <= 16_000_000 else None,
                  bitwise_equal_to_torch_form=True)
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
