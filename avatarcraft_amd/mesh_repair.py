"""Making the exported mesh manifold on the device (csrc/mesh_repair.hip: ac_mesh_repair_count / _emit).  Vertex clustering (mesh_decimate) pushes two sheets of
the surface onto one edge or one vertex; after the weld (mesh_weld) such an edge is shared by three or more different triangles and mesh_topology counts it as
non-manifold.  The repair orders the triangles around every such edge by their positions, pairs them by cyclic bracket matching -- each pair bounds one wedge of
solid --, and gives every fan of triangles around a vertex its own copy of that vertex: two bodies that touch along an edge or in a point come apart as two
bodies.  Nothing is removed, no triangle changes its place or its orientation, and the copies of a vertex start at one position.  What no vertex duplication can
separate -- a pinch: an edge where the surface touches itself while both end points keep a single fan -- stays and is counted by mesh_topology.  The definition:
include/avatarcraft_hip.h.  The result is the same from run to run and equals the numpy restatement of tests/mesh_repair_cases.py exactly.  The front end of
NeRFNetwork.export_manifold and drivers.export_mesh / export_animation(manifold=True)."""
import numpy as np
import torch

from . import _lib as L
from .nsr_ops._args import _chk_typed

REPORT_KEYS = ("vertices", "split", "nonmanifold", "paired", "cut", "crowded", "invalid", "degenerate")
_NOT_PER_VERTEX = ("vertices", "triangles", "component_sizes", "components_kept", "cluster", "cluster_members")


def mesh_repair(vertices, triangles):
    """ac_mesh_repair_count + _emit: vertices [V,3] float32 and triangles [T,3] int32 on the device; float64 vertices (the export's own) are rounded to float32
    first: the order around an edge is defined on fp32 positions.  -> dict(triangles [T,3] int32: the same triangles in the
    same order and orientation, every corner rewritten to the index of its fan; source [V'] int32: the original vertex of every output vertex, the identity on
    the first V, so vertices[source] are the output positions (the copies of a split vertex coincide); report: a plain dict of the counts REPORT_KEYS --
    vertices V', split (vertices with more than one fan), nonmanifold (edges with three or more uses), paired and cut (their uses), crowded (edges with more
    than 8 uses or a key that is not finite: all their uses are cut), invalid, degenerate -- plus added = V' - V).  One 32-byte read-back between count and
    emit.  Degenerate triangles are copied as they stand and reported.  RuntimeError, giving the counts, if a triangle names an index outside [0, V): a mesh
    of this project never does."""
    who = "mesh_repair"
    _chk_typed(vertices, (torch.float32, torch.float64), (None, 3), f"{who}: vertices must be a contiguous float32 or float64 [V,3] tensor",
               cuda_msg=f"{who}: vertices must be a CUDA tensor (there is no CPU path)")
    _chk_typed(triangles, torch.int32, (None, 3), f"{who}: triangles must be a contiguous int32 [T,3] tensor",
               cuda_msg=f"{who}: triangles must be a CUDA tensor (there is no CPU path)")
    V, T, dev = vertices.shape[0], triangles.shape[0], triangles.device
    if vertices.device != dev:
        raise RuntimeError(f"{who}: vertices on {vertices.device}, triangles on {dev}")
    if V >= 2 ** 31 or 3 * T >= 2 ** 31:
        raise RuntimeError(f"{who}: {V} vertices or 3 x {T} corners reach 2^31 (indices are int32)")
    if T and not V:
        raise RuntimeError(f"{who}: {T} triangles over no vertex")
    vertices = vertices.to(torch.float32)
    need = int(L.lib().ac_mesh_repair_scratch(V, T))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    st = L.current_stream(dev)
    head = (L.ptr(vertices) if V else None, L.ptr(triangles) if T else None, T, V, L.ptr(scratch) if V else None, need)
    L.check(L.lib().ac_mesh_repair_count(*head, counts.data_ptr(), st), "mesh_repair_count")
    report = dict(zip(REPORT_KEYS, (int(v) & 0xffffffff for v in counts.tolist())))
    if report["invalid"]:
        raise RuntimeError(f"mesh_repair: {report['invalid']} of {T} triangles name an index outside [0, {V}) (counts: {report})")
    nv = report["vertices"]
    if nv >= 2 ** 31:
        raise RuntimeError(f"mesh_repair: {nv} vertices after the repair reach 2^31 (indices are int32)")
    report["added"] = nv - V
    out = dict(triangles=torch.empty((T, 3), dtype=torch.int32, device=dev), source=torch.empty((nv,), dtype=torch.int32, device=dev), report=report)
    if V:
        L.check(L.lib().ac_mesh_repair_emit(*head, L.ptr(out["triangles"]) if T else None, L.ptr(out["source"]), nv, st), "mesh_repair_emit")
    return out


def repair_mesh(mesh):
    """the mesh made manifold on the device: mesh = dict(vertices [V,3] float64 or float32, triangles [T,3] int32, ...) of device tensors, as mesh_weld.weld_mesh,
    mesh_decimate.decimate_mesh or geometry.clean_mesh gives them.  -> a new dict: vertices, cluster_members and every other per-vertex entry (a tensor with V
    rows) gathered through `source` -- the copies of a split vertex hold the same values, the same position among them --, triangles replaced, repair = the
    report of mesh_repair; cluster (old vertex -> new, if present) is left as it is: old indices stay valid, the copies come after them; entries that are not
    per vertex (component_sizes, ...) are carried over.  geometry.clean_mesh accepts the result: whether a part that merely touched the body goes is the
    caller's decision, so the components are not re-run here.
    A dict with `uv` or `texture` is refused: the atlas addresses its cells by triangle index and its texels were baked for the vertices as they were, so a
    textured mesh is repaired before the bake (NeRFNetwork.export_manifold), not after."""
    if "uv" in mesh or "texture" in mesh:
        raise RuntimeError("repair_mesh: a textured mesh cannot be repaired (the atlas addresses cells by triangle index): set NeRFNetwork.export_manifold "
                           "(drivers.export_mesh(manifold=True)) so that the mesh is repaired before the bake")
    v, t = mesh["vertices"], mesh["triangles"]
    if not isinstance(v, torch.Tensor) or not isinstance(t, torch.Tensor) or not v.is_cuda or not t.is_cuda:
        raise RuntimeError("repair_mesh: vertices and triangles must be CUDA tensors (there is no CPU path)")
    V = v.shape[0]
    r = mesh_repair(v, t)
    src = r["source"].long()
    out = {}
    for k, x in mesh.items():
        if k in ("vertices", "cluster_members") or (k not in _NOT_PER_VERTEX and isinstance(x, (torch.Tensor, np.ndarray)) and x.ndim >= 1 and x.shape[0] == V):
            out[k] = x[src] if isinstance(x, torch.Tensor) else x[src.cpu().numpy()]
        else:
            out[k] = x
    out.update(triangles=r["triangles"], repair=r["report"])
    return out
