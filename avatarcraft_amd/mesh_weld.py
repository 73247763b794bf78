"""Welding the decimated mesh on the device and reporting its topology (csrc/mesh_weld.hip: ac_mesh_weld_count / _emit, ac_mesh_topology).  Vertex clustering
(mesh_decimate) collapses a thin part onto itself: the same triangle twice, or a back-to-back pair.  The weld keeps one triangle of every group of triangles over
the same three vertices -- none where the two orientations cancel --, drops the vertices nobody names any more, and keeps the order of everything else; the report
counts distinct, boundary, non-manifold and misoriented edges, so that a caller can SEE whether a mesh is closed and manifold.  The definitions:
include/avatarcraft_hip.h.  Integer work on the index buffer alone: the result is the same from run to run and equals the numpy restatement of
tests/mesh_weld_cases.py exactly.  The front end of NeRFNetwork.export_weld and drivers.export_mesh / export_animation(weld=True)."""
import numpy as np
import torch

from . import _lib as L
from .nsr_ops._args import _chk_int, _chk_typed

REPORT_KEYS = ("vertices", "triangles", "invalid", "degenerate", "cancelled", "repeated", "excess")
TOPOLOGY_KEYS = ("edges", "boundary", "nonmanifold", "misoriented", "referenced", "faces", "invalid", "degenerate")
_NOT_PER_VERTEX = ("vertices", "triangles", "component_sizes", "components_kept", "cluster", "cluster_members")


def _head(triangles, V, who):
    """the checked arguments both calls share -> (T, V, device)"""
    _chk_typed(triangles, torch.int32, (None, 3), f"{who}: triangles must be a contiguous int32 [T,3] tensor",
               cuda_msg=f"{who}: triangles must be a CUDA tensor (there is no CPU path)")
    V = _chk_int(V, f"{who}: V {V!r} must be an integer in [0, 2^31)", 0, 2 ** 31)
    T = triangles.shape[0]
    if T >= 2 ** 31:
        raise RuntimeError(f"{who}: {T} triangles reach 2^31 (indices are int32)")
    if T and not V:
        raise RuntimeError(f"{who}: {T} triangles over no vertex")
    return T, V, triangles.device


def mesh_weld(triangles, V):
    """ac_mesh_weld_count + _emit: triangles [T,3] int32 on the device over V vertices.  -> dict(vertex_map [V] int32: new index or -1; kept_vertices [V'] int32:
    old indices, ascending; triangles [T',3] int32: one triangle of every group that does not cancel, re-indexed, in their order and orientation;
    kept_triangles [T'] int32: their old indices; report: a plain dict of the counts REPORT_KEYS -- vertices V', triangles T', invalid, degenerate, cancelled,
    repeated, excess).  One 32-byte read-back between count and emit.  Degenerate triangles are dropped and reported.  RuntimeError, giving the counts, if a
    triangle names an index outside [0, V): a mesh of this project never does."""
    T, V, dev = _head(triangles, V, "mesh_weld")
    need = int(L.lib().ac_mesh_weld_scratch(V, T))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    st = L.current_stream(dev)
    head = (L.ptr(triangles) if T else None, T, V, L.ptr(scratch) if V else None, need)
    L.check(L.lib().ac_mesh_weld_count(*head, counts.data_ptr(), st), "mesh_weld_count")
    report = dict(zip(REPORT_KEYS, (int(v) for v in counts.tolist())))
    if report["invalid"]:
        raise RuntimeError(f"mesh_weld: {report['invalid']} of {T} triangles name an index outside [0, {V}) (counts: {report})")
    nv, nt = report["vertices"], report["triangles"]
    out = dict(vertex_map=i32(V), kept_vertices=i32(nv), triangles=i32(nt, 3), kept_triangles=i32(nt), report=report)
    if V:
        L.check(L.lib().ac_mesh_weld_emit(*head, L.ptr(out["vertex_map"]), L.ptr(out["kept_vertices"]) if nv else None, nv,
                                          L.ptr(out["triangles"]) if nt else None, L.ptr(out["kept_triangles"]) if nt else None, nt, st), "mesh_weld_emit")
    return out


def mesh_topology(triangles, V):
    """ac_mesh_topology: triangles [T,3] int32 on the device over V vertices -> a dict of Python ints: the counts TOPOLOGY_KEYS -- edges E (distinct),
    boundary (used once), nonmanifold (used more than twice), misoriented (used twice in one direction), referenced vertices, faces F (valid, non-degenerate),
    invalid, degenerate -- plus euler = referenced - E + F and closed_manifold = (boundary == nonmanifold == misoriented == 0).  One 32-byte read-back.
    Non-manifold VERTICES (two fans that touch in a point) are not looked for (mesh_repair.mesh_repair splits them, and the non-manifold edges it can)."""
    T, V, dev = _head(triangles, V, "mesh_topology")
    need = int(L.lib().ac_mesh_topology_scratch(V, T))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    L.check(L.lib().ac_mesh_topology(L.ptr(triangles) if T else None, T, V, L.ptr(scratch) if V else None, need, counts.data_ptr(), L.current_stream(dev)),
            "mesh_topology")
    r = dict(zip(TOPOLOGY_KEYS, (int(v) for v in counts.tolist())))
    r["euler"] = r["referenced"] - r["edges"] + r["faces"]
    r["closed_manifold"] = r["boundary"] == 0 and r["nonmanifold"] == 0 and r["misoriented"] == 0
    return r


def weld_mesh(mesh):
    """the mesh welded on the device: mesh = dict(vertices [V,3], triangles [T,3] int32, ...) of device tensors, as mesh_decimate.decimate_mesh or
    geometry.clean_mesh gives them.  -> a new dict: vertices and every other per-vertex entry (a tensor with V rows) gathered through kept_vertices, triangles
    replaced, cluster (old vertex -> new, if present) remapped through vertex_map (-1 where the cluster was dropped), cluster_members gathered, weld = the
    report of mesh_weld; entries that are not per vertex (component_sizes, ...) are carried over.
    A dict with `uv` or `texture` is refused: the atlas addresses its cells by triangle index, so a textured mesh is welded before the bake
    (NeRFNetwork.export_weld), not after."""
    if "uv" in mesh or "texture" in mesh:
        raise RuntimeError("weld_mesh: a textured mesh cannot be welded (the atlas addresses cells by triangle index): set NeRFNetwork.export_weld "
                           "(drivers.export_mesh(weld=True)) so that the mesh is welded before the bake")
    v, t = mesh["vertices"], mesh["triangles"]
    if not isinstance(v, torch.Tensor) or not isinstance(t, torch.Tensor) or not v.is_cuda or not t.is_cuda:
        raise RuntimeError("weld_mesh: vertices and triangles must be CUDA tensors (there is no CPU path)")
    V = v.shape[0]
    r = mesh_weld(t, V)
    kept = r["kept_vertices"].long()
    out = {}
    for k, x in mesh.items():
        if k in ("vertices", "cluster_members") or (k not in _NOT_PER_VERTEX and isinstance(x, (torch.Tensor, np.ndarray)) and x.ndim >= 1 and x.shape[0] == V):
            out[k] = x[kept] if isinstance(x, torch.Tensor) else x[kept.cpu().numpy()]
        else:
            out[k] = x
    if "cluster" in mesh and V:                                 # (without a vertex every entry is -1 already)
        c = mesh["cluster"].long()
        new = r["vertex_map"][c.clamp(min=0)]
        out["cluster"] = torch.where(c >= 0, new, torch.full_like(new, -1))
    out.update(triangles=r["triangles"], weld=r["report"])
    return out
