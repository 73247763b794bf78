"""Decimating the exported mesh on the device (csrc/mesh_cluster.hip: ac_mesh_cluster_count / _emit): vertex clustering on a grid.  The vertices of one grid cell
merge into one, triangles that lose a corner to a merge are dropped, everything else keeps its order.  The step decides WHICH vertices merge and gives a starting
point near the surface (the cell's mean vertex); positions, normals and colours are then restored from the field by the export's own projection
(nsr_ops.mesh_vertex_attrs / mesh_bake_texture), which is why no quadric is needed.  The definitions: include/avatarcraft_hip.h.  Everything computed is an integer
or a function of exact integer sums: the result is the same from run to run and equals the numpy restatement of tests/mesh_decimate_cases.py exactly.
The front end of NeRFNetwork.extract_geometry / extract_colored_mesh / extract_textured_mesh(decimate=k)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .nsr_ops._args import _chk_typed

MAX_CELLS = 2 ** 21                   # cells per axis: three of them fit the 64-bit cell key


def cluster_grid(bound, resolution, k):
    """the cluster grid over the marching-cubes grid of extract_geometry(bound, resolution), k marching-cubes cells per cluster cell (a finite real >= 1; k = 1
    merges only what shares a marching-cubes cell): -> dict(lo [3], h, n [3]) with lo = float32(-bound) on each axis (the export's own lower corner),
    h = k * (float32(bound) - float32(-bound)) / (resolution - 1), n = ceil((resolution - 1) / k).  ValueError for anything else, and for n > 2^21."""
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not math.isfinite(k) or k < 1:
        raise ValueError(f"cluster_grid: k {k!r} must be a finite real >= 1 (the cluster cell edge in marching-cubes cells)")
    if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or resolution < 2:
        raise ValueError(f"cluster_grid: resolution {resolution!r} must be an integer >= 2")
    try:
        bmin, bmax = np.float32(-bound), np.float32(bound)
    except (TypeError, ValueError) as e:
        raise ValueError(f"cluster_grid: bound {bound!r} must be a number") from e
    if not np.isfinite(bmax) or not bmax > 0:
        raise ValueError(f"cluster_grid: bound {bound!r} must be finite and > 0")
    k, cells = float(k), int(resolution) - 1
    n = int(math.ceil(cells / k))
    if n > MAX_CELLS:
        raise ValueError(f"cluster_grid: {n} cells per axis, more than 2^21: raise k ({k}) or lower the resolution ({resolution})")
    return dict(lo=[float(bmin)] * 3, h=k * float(bmax - bmin) / cells, n=[n] * 3)


def _grid_arg(grid, who):
    """ac_cluster_grid of a cluster_grid dict; ValueError for what the C entries would refuse"""
    try:
        lo, h, n = [float(v) for v in grid["lo"]], float(grid["h"]), [int(v) for v in grid["n"]]
    except (TypeError, KeyError, ValueError) as e:
        raise ValueError(f"{who}: grid must be a dict(lo [3], h, n [3]) as cluster_grid makes it ({e})") from e
    if len(lo) != 3 or len(n) != 3 or not math.isfinite(h) or h <= 0 or any(c < 1 or c > MAX_CELLS for c in n) or [float(v) for v in grid["n"]] != [float(c) for c in n]:
        raise ValueError(f"{who}: grid needs three lo, a finite h > 0 and three integer n in [1, 2^21], got {grid!r}")
    return L.ac_cluster_grid((C.c_double * 3)(*lo), h, (C.c_uint32 * 3)(*n))


def mesh_cluster(vertices, triangles, grid):
    """ac_mesh_cluster_count + _emit: vertices [V,3] float64 and triangles [T,3] int32 on one device (a mesh dict's own), grid = cluster_grid's dict.
    -> dict(cluster [V] int32: the cluster of every vertex; leader [V'] int32: the smallest old index of each cluster, ascending; members [V'] int32;
    positions [V',3] float64: the clusters' mean vertices; triangles [T',3] int32: the triangles that keep three different clusters, re-indexed, in their order and
    orientation; kept_triangles [T'] int32: their old indices).  One 16-byte read-back between count and emit.  RuntimeError, giving the counts, if a vertex is not
    finite or lies outside the grid, or a triangle names an index outside [0, V): a mesh of this project never has either."""
    _chk_typed(vertices, torch.float64, (None, 3), "mesh_cluster: vertices must be a contiguous float64 [V,3] tensor",
               cuda_msg="mesh_cluster: vertices must be a CUDA tensor (there is no CPU path)")
    _chk_typed(triangles, torch.int32, (None, 3), "mesh_cluster: triangles must be a contiguous int32 [T,3] tensor on the device of vertices",
               cuda_msg="mesh_cluster: triangles must be a CUDA tensor (there is no CPU path)", device=vertices.device)
    g = _grid_arg(grid, "mesh_cluster")
    V, T, dev = vertices.shape[0], triangles.shape[0], vertices.device
    if V >= 2 ** 31 or T >= 2 ** 31:
        raise RuntimeError(f"mesh_cluster: {V} vertices or {T} triangles reach 2^31 (indices are int32)")
    need = int(L.lib().ac_mesh_cluster_scratch(V, T))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    cluster = i32(V)
    st = L.current_stream(dev)
    head = (L.ptr(vertices) if V else None, V, L.ptr(triangles) if T else None, T, C.byref(g), L.ptr(scratch) if V or T else None, need)
    L.check(L.lib().ac_mesh_cluster_count(*head, L.ptr(cluster) if V else None, counts.data_ptr(), st), "mesh_cluster_count")
    nc, nt, bad_v, bad_t = (int(v) for v in counts.tolist())
    if bad_v or bad_t:
        raise RuntimeError(f"mesh_cluster: {bad_v} of {V} vertices are not finite or lie outside the grid, {bad_t} of {T} triangles name one of them or an index "
                           f"outside [0, {V})")
    out = dict(cluster=cluster, leader=i32(nc), members=i32(nc), positions=torch.empty((nc, 3), dtype=torch.float64, device=dev), triangles=i32(nt, 3),
               kept_triangles=i32(nt))
    if nc or nt:
        L.check(L.lib().ac_mesh_cluster_emit(*head, L.ptr(out["leader"]) if nc else None, L.ptr(out["members"]) if nc else None,
                                             L.ptr(out["positions"]) if nc else None, nc, L.ptr(out["triangles"]) if nt else None,
                                             L.ptr(out["kept_triangles"]) if nt else None, nt, st), "mesh_cluster_emit")
    return out


def decimate_mesh(mesh, grid):
    """the mesh with the vertices of every cell of `grid` (cluster_grid) merged, on the device: mesh = dict(vertices [V,3] float64, triangles [T,3] int32) of device
    tensors, as extract_geometry(return_torch=True) or geometry.clean_mesh gives them.  -> a new dict: vertices [V',3] float64 (the clusters' mean vertices: near
    the surface, NOT on it -- project them with nsr_ops.mesh_vertex_attrs, max_move = the grid's h), triangles [T',3] int32, cluster [V] int32 (old vertex -> new)
    and cluster_members [V'] int32; entries that are not per vertex (component_sizes, ...) are carried over.
    A dict with `uv` or `texture` is refused: the atlas addresses its cells by triangle index, so a textured mesh is decimated before the bake
    (extract_textured_mesh(decimate=...)), not after.  So is a dict with any other per-vertex entry (normals, colors, sdf, status, ...): after a merge they have to
    be recomputed from the field, not averaged -- decimate the bare geometry, then shade it."""
    if "uv" in mesh or "texture" in mesh:
        raise RuntimeError("decimate_mesh: a textured mesh cannot be decimated (the atlas addresses cells by triangle index): pass decimate= to extract_textured_mesh")
    v, t = mesh["vertices"], mesh["triangles"]
    if not isinstance(v, torch.Tensor) or not isinstance(t, torch.Tensor):
        raise RuntimeError("decimate_mesh: vertices and triangles must be CUDA tensors (there is no CPU path)")
    V = v.shape[0]
    per_vertex = sorted(k for k, x in mesh.items() if k not in ("vertices", "triangles") and isinstance(x, (torch.Tensor, np.ndarray)) and x.ndim >= 1 and x.shape[0] == V
                        and k not in ("component_sizes", "components_kept"))
    if per_vertex:
        raise RuntimeError(f"decimate_mesh: the mesh carries per-vertex entries {per_vertex}: merged vertices cannot average them, they are recomputed from the field -- "
                           "decimate dict(vertices, triangles) and shade the result (or pass decimate= to extract_colored_mesh)")
    if not v.is_cuda or not t.is_cuda:
        raise RuntimeError("decimate_mesh: vertices and triangles must be CUDA tensors (there is no CPU path)")
    r = mesh_cluster(v, t, grid)
    out = {k: x for k, x in mesh.items() if k not in ("vertices", "triangles")}
    out.update(vertices=r["positions"], triangles=r["triangles"], cluster=r["cluster"], cluster_members=r["members"])
    return out
