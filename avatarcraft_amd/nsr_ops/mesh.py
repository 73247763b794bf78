"""The mesh export on the device (csrc/field_grid.hip, marching_cubes.hip, mesh_shade.hip, mesh_pose.hip, mesh_components.hip): the SDF on a grid,
marching cubes whole and in slabs, per-vertex and per-texel attributes, binding to and posing with the guide, connected components and compaction."""
import ctypes as C

import torch

from .. import _lib as L
from ._args import _F32, _chk, _chk_cuda, _chk_int, _chk_typed, _f32
from .render import FD_STEP
from .warp import WarpMesh


def field_sdf_grid(field, axis_x, axis_y, axis_z, bound, negate=False, out=None):
    """ac_field_sdf_grid: forward_sdf(.)[0] on the grid axis_x x axis_y x axis_z (three 1-D float32 device tensors: the coordinates
    torch.linspace gives the reference's extract_fields, models/instant_nsr.py:728-745) -> [nx, ny, nz] float32 on the device; negate: -sdf"""
    ax, ay, az = _chk(axis_x.reshape(-1), "axis_x"), _chk(axis_y.reshape(-1), "axis_y"), _chk(axis_z.reshape(-1), "axis_z")
    nx, ny, nz = ax.shape[0], ay.shape[0], az.shape[0]
    if out is None:
        out = _f32(ax.device, nx, ny, nz)
    else:
        _chk_typed(out, _F32, (nx, ny, nz), "field_sdf_grid: out must be a contiguous float32 [nx, ny, nz] tensor")
    L.check(L.lib().ac_field_sdf_grid(C.byref(field.c), ax.data_ptr(), ay.data_ptr(), az.data_ptr(), nx, ny, nz, float(bound), int(bool(negate)),
                                      out.data_ptr(), L.current_stream(ax.device)), "field_sdf_grid")
    return out


def marching_cubes(volume, iso=0.0, den=1.0, span=(1.0, 1.0, 1.0), lo=(0.0, 0.0, 0.0)):
    """ac_marching_cubes_count + _emit on a device volume [nx, ny, nz] (float32): the surface u = iso, corner flagged <=> u <= iso (PyMCubes' convention),
    one shared vertex per sign-changing grid edge.  -> (vertices [V,3] float64 = index / den * span + lo, triangles [F,3] int32), both on the device.
    One 8-byte device-to-host read between the two calls (the caller owns the output buffers, so it has to know their size)."""
    vol = _chk(volume, "volume")
    if vol.dim() != 3:
        raise RuntimeError("marching_cubes: volume must be [nx, ny, nz]")
    nx, ny, nz = vol.shape
    dev = vol.device
    need = int(L.lib().ac_marching_cubes_scratch(nx, ny, nz))
    if need == 0:
        raise RuntimeError(f"marching_cubes: grid {nx} x {ny} x {nz} unsupported (every side >= 2, fewer than 2^31 points)")
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    st = L.current_stream(dev)
    L.check(L.lib().ac_marching_cubes_count(vol.data_ptr(), nx, ny, nz, float(iso), scratch.data_ptr(), need, counts.data_ptr(), st), "marching_cubes_count")
    nv, nt = (int(v) for v in counts.tolist())
    verts = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    span_c, lo_c = (C.c_double * 3)(*[float(v) for v in span]), (C.c_double * 3)(*[float(v) for v in lo])
    if nv or nt:
        L.check(L.lib().ac_marching_cubes_emit(vol.data_ptr(), nx, ny, nz, float(iso), scratch.data_ptr(), need, float(den), span_c, lo_c,
                                               L.ptr(verts) if nv else None, nv, L.ptr(tris) if nt else None, nt, st), "marching_cubes_emit")
    return verts, tris


def check_slab_layers(slab_layers, who):
    """slab_layers of the streamed mesh export as an int >= 2 (RuntimeError naming it otherwise); no device work"""
    return _chk_int(slab_layers, f"{who}: slab_layers {slab_layers!r} must be an integer >= 2", 2)


def slab_windows(nx, slab_layers):
    """the windows in which marching_cubes_streamed walks nx grid layers: [(x0, n, first, last, new_lo, new_n)], window = layers [x0, x0 + n) of the grid, of which
    [new_lo, new_lo + new_n) (window-relative) are new and the ones before them carried from the previous window.  The first window has min(slab_layers, nx)
    layers, all new; every later one carries 2 and adds up to slab_layers: x0' = x0 + n - 2, no window longer than slab_layers + 2.  A window emits the vertices
    of its layers 1 .. n-2 (and 0 if first, n-1 if last) and the triangles of its cell layers 0 .. n-3 (and n-2 if last): a partition of the grid.  Pure Python."""
    slab_layers = check_slab_layers(slab_layers, "slab_windows")
    _chk_int(nx, f"slab_windows: nx {nx!r} must be an integer >= 2", 2)
    end = min(slab_layers, int(nx))
    wins = [(0, end, True, end == nx, 0, end)]
    while end < nx:
        new = min(slab_layers, nx - end)
        wins.append((end - 2, new + 2, False, end + new == nx, 2, new))
        end += new
    return wins


def marching_cubes_streamed(fill, nx, ny, nz, slab_layers=64, iso=0.0, den=1.0, span=(1.0, 1.0, 1.0), lo=(0.0, 0.0, 0.0), device="cuda"):
    """marching_cubes of an [nx, ny, nz] volume that is never whole (ac_marching_cubes_slab_count / _emit): the volume is produced slab by slab along x into ONE
    window buffer of slab_layers + 2 layers, each window is meshed with the shared-edge vertex indices carried across its border, and the pieces are joined --
    bit for bit and in order the mesh marching_cubes gives for the whole volume, in the memory of one window (9 bytes per point of the window instead of the
    grid), and for grids of 2^31 points and more (only a window has to stay below that).
    fill(x0, out) writes grid layers [x0, x0 + out.shape[0]) into out, a contiguous float32 [m, ny, nz] view of the window buffer on `device`; every layer is
    asked for exactly once, slab_layers at a time (the last call: what is left).  Per window: two carried layers copied to the front, fill, count, one 16-byte
    read-back, emit into the window's own piece.  slab_layers: any integer >= 2 (slab_windows); the default is the fastest of 16 / 32 / 64 / 128 at 512^3
    (profiles/mesh_streamed.txt: 15.20 ms beside the dense route's 15.65), and multiples of 16 keep the x-tiles of field_sdf_grid full.
    -> (vertices [V,3] float64 = index / den * span + lo, triangles [F,3] int32), both on the device.  Options are checked before any device work."""
    slab_layers = check_slab_layers(slab_layers, "marching_cubes_streamed")
    if not callable(fill):
        raise RuntimeError("marching_cubes_streamed: fill must be callable: fill(x0, out)")
    for name, v in (("nx", nx), ("ny", ny), ("nz", nz)):
        _chk_int(v, f"marching_cubes_streamed: {name} {v!r} must be an integer, 2 <= {name} < 2^32", 2, 2 ** 32)
    nx, ny, nz = int(nx), int(ny), int(nz)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"marching_cubes_streamed: device {device!r} is not a GPU (there is no CPU path)")
    try:
        iso, den, span, lo = float(iso), float(den), [float(v) for v in span], [float(v) for v in lo]
    except (TypeError, ValueError) as e:
        raise RuntimeError(f"marching_cubes_streamed: iso, den, span and lo must be numbers ({e})") from e
    if len(span) != 3 or len(lo) != 3 or not den != 0.0:
        raise RuntimeError("marching_cubes_streamed: span and lo take 3 numbers each, den != 0")
    wins = slab_windows(nx, slab_layers)
    layers = max(3, max(w[1] for w in wins))
    if layers * ny * nz >= 2 ** 31:
        raise RuntimeError(f"marching_cubes_streamed: a window of {layers} x {ny} x {nz} points reaches 2^31: lower slab_layers ({slab_layers})")
    need = int(L.lib().ac_marching_cubes_slab_scratch(layers, ny, nz))
    buf = torch.empty((layers, ny, nz), dtype=_F32, device=dev)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    span_c, lo_c = (C.c_double * 3)(*span), (C.c_double * 3)(*lo)
    st = L.current_stream(dev)
    vparts, tparts, vbase, prev_n, top = [], [], 0, 0, None
    for x0, n, first, last, new_lo, new_n in wins:
        if new_lo:
            tail = buf[prev_n - 2:prev_n]
            buf[:2].copy_(tail.clone() if prev_n < 4 else tail)                          # (source and target overlap in a window of 3 layers)
        fill(x0 + new_lo, buf[new_lo:new_lo + new_n])
        prev_n = n
        if n == 2 and not last:
            continue                  # (slab_layers = 2: no layer of this window has both neighbours yet; the next one starts at x0 = 0 as well and is meshed as the first)
        first = x0 == 0
        L.check(L.lib().ac_marching_cubes_slab_count(buf.data_ptr(), n, ny, nz, iso, int(first), int(last), scratch.data_ptr(), need, counts.data_ptr(), st),
                "marching_cubes_slab_count")
        nv, nt, carried, new_top = (int(v) for v in counts.tolist())
        if not first and carried != top:
            raise RuntimeError(f"marching_cubes_streamed: the window at x0 = {x0} finds {carried} vertices in its carried layer, the window before it emitted {top} "
                               f"there: fill({x0}, .) and the call before it disagree, or the carry is broken")
        top = new_top
        if vbase + nv > 2 ** 31 - 1:
            raise RuntimeError(f"marching_cubes_streamed: more than {2 ** 31 - 1} vertices: triangle indices are int32")
        verts = torch.empty((nv, 3), dtype=torch.float64, device=dev)
        tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        if nv or nt:
            L.check(L.lib().ac_marching_cubes_slab_emit(buf.data_ptr(), n, ny, nz, iso, int(first), int(last), scratch.data_ptr(), need, x0, vbase, den, span_c, lo_c,
                                                        L.ptr(verts) if nv else None, nv, L.ptr(tris) if nt else None, nt, st), "marching_cubes_slab_emit")
            vparts.append(verts); tparts.append(tris)
        vbase += nv
    join = lambda parts, dt: parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.empty((0, 3), dtype=dt, device=dev)
    verts = join(vparts, torch.float64)
    del vparts
    return verts, join(tparts, torch.int32)


def _mesh_attr_opts(bound, eps, target_sdf, refine_steps, tol, max_move):
    """ac_mesh_attr_opts of mesh_vertex_attrs and mesh_bake_texture"""
    return L.ac_mesh_attr_opts(float(bound), float(eps), float(target_sdf), int(refine_steps), float(tol), float(_max_move(bound, max_move)))


def _max_move(bound, max_move):
    """max_move None: one cell of a 512^3 grid over the bound"""
    return 2.0 * float(bound) / 511.0 if max_move is None else max_move


def mesh_vertex_attrs(field, vertices, bound, eps=FD_STEP, refine_steps=3, tol=1e-5, max_move=None, target_sdf=0.0, dirs=None, want_rgb=True):
    """ac_mesh_vertex_attrs: what a coloured export needs per vertex, in one launch.  vertices [V,3] float64 on the device (marching_cubes' buffer as it is);
    every vertex takes at most refine_steps Newton steps along the finite-difference gradient onto sdf = target_sdf (never further than max_move per
    coordinate from where it started; None: one cell of a 512^3 grid over the bound), then the normal and the colour network are evaluated at the final position.
    dirs [V,3] float32: view directions for a field with Wc1_sh (None: -normal).  want_rgb=False: no colour network (an SDF-only field is enough).
    -> dict(positions [V,3], normals [V,3], rgb [V,3] | None, sdf [V], status [V] uint8, why the steps ended: 0 a step found |sdf - target| <= tol, 1 all steps taken (the last is
    not tested: read sdf), 2 degenerate gradient, 3 max_move)"""
    _chk_typed(vertices, torch.float64, (None, 3), "mesh_vertex_attrs: vertices must be a contiguous float64 [V,3] tensor",
               cuda_msg="vertices must be a CUDA tensor")
    V, dev = vertices.shape[0], vertices.device
    if dirs is not None:
        dirs = _chk(dirs, "dirs", (V, 3))
    opts = _mesh_attr_opts(bound, eps, target_sdf, refine_steps, tol, max_move)
    out = dict(positions=_f32(dev, V, 3), normals=_f32(dev, V, 3), rgb=_f32(dev, V, 3) if want_rgb else None, sdf=_f32(dev, V),
               status=torch.empty(V, dtype=torch.uint8, device=dev))
    L.check(L.lib().ac_mesh_vertex_attrs(C.byref(field.c), vertices.data_ptr(), V, L.ptr(dirs), C.byref(opts), out["positions"].data_ptr(),
                                         out["normals"].data_ptr(), L.ptr(out["rgb"]), out["sdf"].data_ptr(), out["status"].data_ptr(),
                                         L.current_stream(dev)), "mesh_vertex_attrs")
    return out


def _bake_args(who, positions, triangles, size, cell, bound, eps, target_sdf, refine_steps, tol, max_move):
    """what the launches over the atlas' texels (mesh_bake_texture, mesh_occlusion.mesh_bake_maps) check before any device work, `who` naming the caller
    -> (V, T, S, device, ac_atlas_opts, ac_mesh_attr_opts)"""
    _chk_cuda(f"{who}: positions and triangles must be CUDA tensors", positions, triangles)
    _chk_typed(positions, _F32, (None, 3), f"{who}: positions must be a contiguous float32 [V,3] tensor")
    _chk_typed(triangles, torch.int32, (None, 3), f"{who}: triangles must be a contiguous int32 [T,3] tensor on the device of positions",
               device=positions.device)
    V, T, S, dev = positions.shape[0], triangles.shape[0], int(size), positions.device
    if cell is None:
        from ..geometry import atlas_layout
        try:
            cell = atlas_layout(T, S)["cell"]
        except ValueError as e:
            raise RuntimeError(f"{who}: {e}") from e
    if T and (int(triangles.min()) < 0 or int(triangles.max()) >= V):
        raise RuntimeError(f"{who}: a triangle index outside [0, {V}); nothing was launched")
    max_move = _max_move(bound, max_move)             # (here, so that a bound that is no number is refused before the size, as it always was)
    if not 0 < S <= 32768:
        raise RuntimeError(f"{who}: size {S} outside 1 .. 32768")
    return V, T, S, dev, L.ac_atlas_opts(S, max(int(cell), 0)), _mesh_attr_opts(bound, eps, target_sdf, refine_steps, tol, max_move)


def mesh_bake_texture(field, positions, triangles, size, cell, bound, eps=FD_STEP, refine_steps=3, tol=1e-5, max_move=None, target_sdf=0.0, want_normals=False):
    """ac_mesh_bake_texture: mesh_vertex_attrs' work per TEXEL of the closed-form atlas (geometry.atlas_layout), in one launch.  positions [V,3] float32 on the
    device (mesh_vertex_attrs' `positions`: vertices on the level set), triangles [T,3] int32, size x size texels in cells of `cell` (None: the largest that fits).
    Every owned texel's point on its triangle takes at most refine_steps Newton steps (max_move from that point; None: one cell of a 512^3 grid), then normal, sdf and
    the colour seen along -normal are evaluated there.  -> dict(rgb [S,S,3], owner [S,S] int32 (-1: nobody; everything else is 0 there), normals [S,S,3] | None,
    sdf [S,S], status [S,S] uint8 as mesh_vertex_attrs').  The triangle indices are checked on the device BEFORE the launch (the kernel reads through them unchecked):
    RuntimeError for one outside [0, V)."""
    V, T, S, dev, atlas, opts = _bake_args("mesh_bake_texture", positions, triangles, size, cell, bound, eps, target_sdf, refine_steps, tol, max_move)
    out = dict(rgb=_f32(dev, S, S, 3), owner=torch.empty((S, S), dtype=torch.int32, device=dev), normals=_f32(dev, S, S, 3) if want_normals else None,
               sdf=_f32(dev, S, S), status=torch.empty((S, S), dtype=torch.uint8, device=dev))
    L.check(L.lib().ac_mesh_bake_texture(C.byref(field.c), positions.data_ptr(), V, triangles.data_ptr(), T, C.byref(atlas), C.byref(opts), out["rgb"].data_ptr(),
                                         out["owner"].data_ptr(), L.ptr(out["normals"]), out["sdf"].data_ptr(), out["status"].data_ptr(),
                                         L.current_stream(dev)), "mesh_bake_texture")
    return out


def mesh_bind(points, guide_verts, faces, accel=True):
    """ac_mesh_bind: once per exported mesh, pose independent.  points [V,3] float32 (the mesh's canonical vertices), guide_verts [Vg,3] float32 (the SMPL guide
    in canonical space: geometry.canonical_guide), faces [F,3] int32, all on one device.  -> dict(face_id [V] int32 the closest guide face, bary [V,3] float64 of
    the closest point on it, dist2 [V] float64).  accel: search through the culling structure (built here) where it covers the guide; the same bits either way."""
    _chk_cuda("mesh_bind: points, guide_verts and faces must be CUDA tensors", points, guide_verts, faces)
    points, guide_verts = _chk(points, "points"), _chk(guide_verts, "guide_verts")
    if points.dim() != 2 or points.shape[1] != 3 or guide_verts.dim() != 2 or guide_verts.shape[1] != 3:
        raise RuntimeError("mesh_bind: points and guide_verts must be [N,3]")
    _chk_typed(faces, torch.int32, (None, 3), "mesh_bind: faces must be a contiguous int32 [F,3] tensor on the device of points", device=points.device)
    V, Vg, F, dev = points.shape[0], guide_verts.shape[0], faces.shape[0], points.device
    if F == 0 or Vg == 0 or int(faces.min()) < 0 or int(faces.max()) >= Vg:
        raise RuntimeError(f"mesh_bind: an empty guide or a face index outside [0, {Vg}); nothing was launched")
    st = L.current_stream(dev)
    acc = None
    nbytes = int(L.lib().ac_warp_accel_bytes(F)) if accel else 0
    if nbytes and V:
        acc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(L.lib().ac_warp_accel_build(guide_verts.data_ptr(), faces.data_ptr(), Vg, F, acc.data_ptr(), nbytes, st), "warp_accel_build")
    out = dict(face_id=torch.empty(V, dtype=torch.int32, device=dev), bary=torch.empty((V, 3), dtype=torch.float64, device=dev),
               dist2=torch.empty(V, dtype=torch.float64, device=dev))
    need = int(L.lib().ac_mesh_bind_scratch(V, Vg))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.lib().ac_mesh_bind(points.data_ptr(), V, guide_verts.data_ptr(), Vg, faces.data_ptr(), F, L.ptr(acc), out["face_id"].data_ptr(),
                                 out["bary"].data_ptr(), out["dist2"].data_ptr(), scratch.data_ptr(), need, st), "mesh_bind")
    return out


def mesh_pose(points, normals, bind, mesh, iters=3, tol=1e-5, want=("residual", "status", "mask")):
    """ac_mesh_pose: once per frame.  points [V,3] float32 canonical vertices, normals [V,3] float32 canonical normals or None, bind = mesh_bind's dict (face_id,
    bary), mesh = the frame's WarpMesh (posed guide, faces, Ts, culling structure or none).  Every vertex iterates p <- A(p) c + t(p) / kappa(p) from the bound
    start until W^-1(p) is within tol of c (max norm), at most iters times (iters + 1 closest-face searches).
    -> dict(positions [V,3], normals [V,3] | None, residual [V], status [V] uint8: 0 within tol, 1 iters used up (read residual), 2 not finite, mask [V] uint8:
    0 = farther from the guide than the renderer's mask threshold -- kept and flagged); `want` names the optional ones to return (the others are None).
    The binding's faces are checked on the device BEFORE the launch: RuntimeError for one outside [0, F)."""
    if not isinstance(mesh, WarpMesh):
        raise RuntimeError("mesh_pose: mesh must be an nsr_ops.WarpMesh")
    face_id, bary = bind["face_id"], bind["bary"]
    _chk_cuda("mesh_pose: points, normals and the binding must be CUDA tensors", *(t for t in (points, normals, face_id, bary) if t is not None))
    points = _chk(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("mesh_pose: points must be [V,3]")
    V, dev = points.shape[0], points.device
    if normals is not None:
        normals = _chk(normals, "normals", (V, 3))
    _chk_typed(face_id, torch.int32, (V,), "mesh_pose: bind['face_id'] must be a contiguous int32 [V] tensor")
    _chk_typed(bary, torch.float64, (V, 3), "mesh_pose: bind['bary'] must be a contiguous float64 [V,3] tensor")
    if any(t is not None and t.device != mesh.verts.device for t in (points, normals, face_id, bary)):
        raise RuntimeError("mesh_pose: every tensor must live on the mesh's device")
    F = mesh.faces.shape[0]
    if V and (int(face_id.min()) < 0 or int(face_id.max()) >= F):
        raise RuntimeError(f"mesh_pose: a binding face outside [0, {F}); nothing was launched")
    unknown = set(want) - {"residual", "status", "mask"}
    if unknown:
        raise ValueError(f"mesh_pose: unknown outputs {sorted(unknown)}")
    opts = L.ac_mesh_pose_opts(int(iters), float(tol))
    out = dict(positions=_f32(dev, V, 3), normals=_f32(dev, V, 3) if normals is not None else None, residual=_f32(dev, V) if "residual" in want else None,
               status=torch.empty(V, dtype=torch.uint8, device=dev) if "status" in want else None,
               mask=torch.empty(V, dtype=torch.uint8, device=dev) if "mask" in want else None)
    need = int(L.lib().ac_mesh_pose_scratch(V))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.lib().ac_mesh_pose(points.data_ptr(), L.ptr(normals), V, face_id.data_ptr(), bary.data_ptr(), C.byref(mesh.c), C.byref(opts), scratch.data_ptr(),
                                 need, out["positions"].data_ptr(), L.ptr(out["normals"]), L.ptr(out["residual"]), L.ptr(out["status"]), L.ptr(out["mask"]),
                                 L.current_stream(dev)), "mesh_pose")
    return out


def _chk_triangles(who, triangles):
    return _chk_typed(triangles, torch.int32, (None, 3), f"{who}: triangles must be a contiguous int32 [T,3] tensor",
                      cuda_msg=f"{who}: triangles must be a CUDA tensor (there is no CPU path)")


def mesh_components(triangles, n_vertices):
    """ac_mesh_components: the connected components of a mesh, triangles [T,3] int32 on the device over n_vertices vertices (the definitions:
    include/avatarcraft_hip.h).  -> dict(root [V] int32: the smallest vertex index of the vertex's component, component [V] int32: the rank of that root among the
    roots, sizes [C,2] (vertices, triangles per component; int64 on the device), n_components = C).  One 8-byte read-back: the two counts (C, invalid triangles).
    RuntimeError, giving the count, for triangles with an index outside [0, V): a mesh of this project never has one."""
    tris = _chk_triangles("mesh_components", triangles)
    V = _chk_int(n_vertices, f"mesh_components: n_vertices {n_vertices!r} must be an integer in [0, 2^31)", 0, 2 ** 31)
    T, dev = tris.shape[0], tris.device
    if V == 0 and T:
        raise RuntimeError(f"mesh_components: {T} triangles over no vertex")
    root = torch.empty(V, dtype=torch.int32, device=dev)
    comp = torch.empty(V, dtype=torch.int32, device=dev)
    sizes = torch.empty((V, 2), dtype=torch.int32, device=dev)                       # (uint32 rows; a count stays below 2^31)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    need = int(L.lib().ac_mesh_components_scratch(V, T))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.lib().ac_mesh_components(L.ptr(tris) if T else None, T, V, L.ptr(root) if V else None, L.ptr(comp) if V else None, L.ptr(sizes) if V else None, V,
                                       counts.data_ptr(), L.ptr(scratch) if need else None, need, L.current_stream(dev)), "mesh_components")
    n_comp, n_bad = (int(v) for v in counts.tolist())
    if n_bad:
        raise RuntimeError(f"mesh_components: {n_bad} of {T} triangles have an index outside [0, {V})")
    return dict(root=root, component=comp, sizes=sizes[:n_comp].to(torch.int64), n_components=n_comp)


def mesh_compact(triangles, component, keep):
    """ac_mesh_compact_count + _emit: the mesh restricted to the components with keep[c] != 0, order preserved.  triangles [T,3] int32, component [V] int32
    (mesh_components'), keep [C] bool or uint8, all on one device.  -> dict(vertex_map [V] int32: new index or -1, kept_vertices [V'] int32: old indices
    ascending, triangles [T',3] int32 re-indexed, kept_triangles [T'] int32: old triangle indices ascending).  One 8-byte read-back between count and emit."""
    tris = _chk_triangles("mesh_compact", triangles)
    for t, name in ((component, "component"), (keep, "keep")):
        _chk_cuda(f"mesh_compact: {name} must be a CUDA tensor (there is no CPU path)", t)
    _chk_typed(component, torch.int32, (None,), "mesh_compact: component must be a contiguous int32 [V] tensor on the device of triangles", device=tris.device)
    _chk_typed(keep, (torch.bool, torch.uint8), (None,), "mesh_compact: keep must be a bool or uint8 [C] tensor on the device of triangles",
               device=tris.device, contiguous=False)
    keep8 = keep.to(torch.uint8).contiguous()
    V, T, Cn, dev = component.shape[0], tris.shape[0], keep8.shape[0], tris.device
    if Cn > V:
        raise RuntimeError(f"mesh_compact: keep has {Cn} entries for {V} vertices")
    need = int(L.lib().ac_mesh_compact_scratch(V, T))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    st = L.current_stream(dev)
    head = (L.ptr(tris) if T else None, T, V, L.ptr(component) if V else None, L.ptr(keep8) if Cn else None, Cn, L.ptr(scratch) if need else None, need)
    L.check(L.lib().ac_mesh_compact_count(*head, counts.data_ptr(), st), "mesh_compact_count")
    nv, nt = (int(v) for v in counts.tolist())
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = dict(vertex_map=i32(V), kept_vertices=i32(nv), triangles=i32(nt, 3), kept_triangles=i32(nt))
    if V:
        L.check(L.lib().ac_mesh_compact_emit(*head, out["vertex_map"].data_ptr(), L.ptr(out["kept_vertices"]) if nv else None, nv,
                                             L.ptr(out["triangles"]) if nt else None, L.ptr(out["kept_triangles"]) if nt else None, nt, st), "mesh_compact_emit")
    return out
