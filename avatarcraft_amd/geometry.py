"""Iso-surface extraction for NeRFNetwork.extract_geometry when PyMCubes is not installed (reference models/instant_nsr.py:748-764 calls
mcubes.marching_cubes): marching tetrahedra on the device, torch only.

Every grid cell is split into the six tetrahedra that share the cell's main diagonal (Kuhn triangulation: neighbouring cells agree on the
diagonals of their common face, so the surface is watertight without a case table for the 256 cube configurations).  A tetrahedron with
1 or 3 corners above the level contributes one triangle, with 2 above a quad (two triangles).  Vertices sit on grid edges at the linear
zero crossing and are shared between the tetrahedra that touch the edge (one vertex per crossed edge), so the result is an indexed mesh.
Vertex coordinates are in grid units (0 .. res-1), like mcubes.marching_cubes; triangles wind counter-clockwise seen from the side of the
smaller values, i.e. normals point out of the body for the reference's `u = -sdf` volumes."""
import torch

# corners of the unit cube, bit k of the corner id = offset along axis k (x = bit 0)
_CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
# the 6 tetrahedra around the diagonal 0 -> 7: paths 0 -> a -> b -> 7 over the axis permutations
_TETS = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def marching_tetrahedra(u, level=0.0):
    """u: [X, Y, Z] float tensor (any device) -> (vertices [V,3] float32 in grid units, triangles [F,3] int64)"""
    assert u.dim() == 3
    X, Y, Z = u.shape
    dev = u.device
    u = u.float()
    inside = u > level                                                  # "inside" = above the level (u = -sdf: inside the body)
    ii, jj, kk = torch.meshgrid(torch.arange(X - 1, device=dev), torch.arange(Y - 1, device=dev), torch.arange(Z - 1, device=dev), indexing="ij")
    base = torch.stack([ii, jj, kk], -1).reshape(-1, 3)                 # [C,3] cell origins
    cid = [((base[:, 0] + c[0]) * Y + (base[:, 1] + c[1])) * Z + (base[:, 2] + c[2]) for c in _CORNERS]      # flat point ids of the 8 corners
    flat_in = inside.reshape(-1)
    cin = torch.stack([flat_in[c] for c in cid], 1)                     # [C,8]
    active = cin.any(1) & ~cin.all(1)                                   # cells the surface passes through
    cid = [c[active] for c in cid]
    cin = cin[active]
    tris = []                                                           # triangles as triples of (point a, point b) edge keys
    for tet in _TETS:
        p = torch.stack([cid[t] for t in tet], 1)                       # [A,4] point ids
        s = torch.stack([cin[:, t] for t in tet], 1)                    # [A,4] inside flags
        n_in = s.sum(1)
        # orientation of the tetrahedron (sign of det[p1-p0, p2-p0, p3-p0]) decides the winding; constant per tetrahedron of the pattern
        c0, c1, c2, c3 = (torch.tensor(_CORNERS[t], dtype=torch.float32) for t in tet)
        orient = torch.det(torch.stack([c1 - c0, c2 - c0, c3 - c0])).item() > 0
        for k in range(4):                                              # exactly one corner differs from the other three
            others = [m for m in range(4) if m != k]
            for flag, count in ((True, 1), (False, 3)):
                sel = (n_in == count) & (s[:, k] == flag)
                if not sel.any():
                    continue
                a = p[sel, k]
                e = [torch.stack([a, p[sel, m]], 1) for m in others]   # the three edges from the odd corner
                # even permutation parity of (k, others) relative to (0,1,2,3): k odd flips; an inside odd corner flips again; orientation flips again
                flip = (k % 2 == 1) ^ flag ^ orient
                tris.append(torch.stack([e[0], e[2], e[1]] if flip else [e[0], e[1], e[2]], 1))
        for (a0, a1) in ((0, 1), (0, 2), (0, 3)):                       # two inside, two outside: the pair (a0, a1) against the other pair
            b0, b1 = [m for m in range(4) if m not in (a0, a1)]
            for flag in (True, False):
                sel = (n_in == 2) & (s[:, a0] == flag) & (s[:, a1] == flag)
                if not sel.any():
                    continue
                q = p[sel]
                e00 = torch.stack([q[:, a0], q[:, b0]], 1); e01 = torch.stack([q[:, a0], q[:, b1]], 1)
                e10 = torch.stack([q[:, a1], q[:, b0]], 1); e11 = torch.stack([q[:, a1], q[:, b1]], 1)
                # quad e00 - e01 - e11 - e10; parity of the permutation (a0, a1, b0, b1)
                perm = [a0, a1, b0, b1]
                inv = sum(1 for i in range(4) for j in range(i + 1, 4) if perm[i] > perm[j])
                flip = (inv % 2 == 1) ^ flag ^ orient
                quad = [e00, e01, e11, e10]
                if flip:
                    quad = quad[::-1]
                tris.append(torch.stack([quad[0], quad[1], quad[2]], 1)); tris.append(torch.stack([quad[0], quad[2], quad[3]], 1))
    if not tris:
        return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev)
    T = torch.cat(tris, 0)                                              # [F,3,2] point-id pairs
    lo, hi = T.min(-1).values, T.max(-1).values
    key = lo * (X * Y * Z) + hi                                         # one key per crossed grid edge (or cell diagonal)
    uniq, inv = torch.unique(key.reshape(-1), return_inverse=True)
    faces = inv.reshape(-1, 3)
    pa, pb = uniq // (X * Y * Z), uniq % (X * Y * Z)
    ua, ub = u.reshape(-1)[pa], u.reshape(-1)[pb]
    t = ((level - ua) / (ub - ua)).clamp(0.0, 1.0)

    def coords(pid):
        return torch.stack([pid // (Y * Z), (pid // Z) % Y, pid % Z], 1).float()
    verts = coords(pa) + t[:, None] * (coords(pb) - coords(pa))
    return verts, faces


def save_ply(path, vertices, triangles, normals=None, colors=None, quality=None):
    """binary little-endian PLY: float32 x y z [nx ny nz], uchar red green blue (round(clip(c, 0, 1) * 255)), [float32 quality], faces as
    `list uchar int vertex_indices`.  vertices [V,3], triangles [F,3], normals [V,3], colors [V,3] in [0, 1], quality [V] (the per-vertex scalar viewers
    know by that name: the export's ambient occlusion): numpy arrays or tensors on any device."""
    import numpy as np
    arr = lambda a, dt: np.ascontiguousarray((a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)), dtype=dt)
    v, t = arr(vertices, "<f4").reshape(-1, 3), arr(triangles, "<i4").reshape(-1, 3)
    cols, props = [("xyz", "<f4", (3,))], ["float x", "float y", "float z"]
    if normals is not None:
        cols.append(("n", "<f4", (3,))); props += ["float nx", "float ny", "float nz"]
    if colors is not None:
        cols.append(("rgb", "u1", (3,))); props += ["uchar red", "uchar green", "uchar blue"]
    if quality is not None:
        cols.append(("q", "<f4")); props += ["float quality"]
    vert = np.empty(len(v), dtype=cols)
    vert["xyz"] = v
    if normals is not None:
        vert["n"] = arr(normals, "<f4").reshape(-1, 3)
    if colors is not None:
        vert["rgb"] = np.round(np.clip(arr(colors, "<f8").reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
    if quality is not None:
        vert["q"] = arr(quality, "<f4").reshape(len(v))
    face = np.empty(len(t), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    face["n"] = 3; face["idx"] = t
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + ["property " + p for p in props]
    head += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vert.tobytes()); fh.write(face.tobytes())


def canonical_guide(world_verts, Ts):
    """the SMPL guide in the canonical space of the field: (inv(Ts[i]) @ (v_i, 1))[:3] per vertex in fp64, cast to fp32 -- the point the inverse warp sends a
    posed guide vertex to (no homogeneous division, like ray_utils.warp_samples_to_canonical).  world_verts [Vg,3], Ts [>= Vg,4,4] of ANY one frame
    (smpl.calc_local_trans): the result does not depend on the frame.  numpy."""
    import numpy as np
    v = np.asarray(world_verts.detach().cpu().numpy() if isinstance(world_verts, torch.Tensor) else world_verts, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(Ts.detach().cpu().numpy() if isinstance(Ts, torch.Tensor) else Ts, dtype=np.float64).reshape(-1, 4, 4)
    if len(T) < len(v):
        raise ValueError("canonical_guide: Ts must hold one 4x4 per vertex")
    h = np.concatenate([v, np.ones((len(v), 1))], axis=1)
    return np.einsum("vij,vj->vi", np.linalg.inv(T[:len(v)]), h)[:, :3].astype(np.float32)


def skin_weights(bind, faces, lbs_weights):
    """a rig for users who pose the exported mesh elsewhere: per mesh vertex sum_k bary_k * lbs_weights[faces[face_id][k]] -> [V,J] float64.  bind: the dict of
    nsr_ops.mesh_bind (face_id [V], bary [V,3]; tensors or arrays), faces [F,3] of the guide, lbs_weights [Vg,J] (SMPL's `weights`).  Rows sum to what
    the guide's rows sum to (1) up to the rounding of the barycentrics.  numpy."""
    import numpy as np
    arr = lambda a, dt: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)
    fid, bc = arr(bind["face_id"], np.int64).reshape(-1), arr(bind["bary"], np.float64).reshape(-1, 3)
    f, w = arr(faces, np.int64)[:, :3], arr(lbs_weights, np.float64)
    if len(fid) and (fid.min() < 0 or fid.max() >= len(f)):
        raise ValueError("skin_weights: a binding face outside the guide's faces")
    return np.einsum("vk,vkj->vj", bc, w[f[fid]])


# ---------------------------------------------------------------------------------------------------- cleaning the mesh: which components stay (nsr_ops.mesh_components / mesh_compact)
def select_components(sizes, spec):
    """which components of a mesh stay: sizes [C,2] (vertices, triangles per component: nsr_ops.mesh_components' table; a tensor or an array) -> bool [C], numpy.
    spec: "largest" = the component with the most triangles, ties to the lower component id | ("largest", k) = the k largest by triangles, same tie rule (k >= C:
    all) | ("min_faces", n) = every component with at least n triangles | a bool array of length C, used as given | a callable sizes -> such a mask.
    ValueError for anything else and for a mask of the wrong length.  Selection by area or bounding box is not built: pass a mask."""
    import numpy as np
    s = np.asarray(sizes.detach().cpu().numpy() if isinstance(sizes, torch.Tensor) else sizes).astype(np.int64).reshape(-1, 2)
    n = len(s)
    if callable(spec):
        spec = spec(s)
        if isinstance(spec, (str, tuple)):
            raise ValueError("select_components: a callable spec must return a bool mask")
    if isinstance(spec, str):
        spec = (spec, 1) if spec == "largest" else (spec,)
    if isinstance(spec, tuple):
        if len(spec) != 2 or spec[0] not in ("largest", "min_faces") or isinstance(spec[1], bool) or not isinstance(spec[1], (int, np.integer)) or spec[1] < 0:
            raise ValueError(f"select_components: unknown spec {spec!r} ('largest', ('largest', k), ('min_faces', n), a bool mask or a callable)")
        if spec[0] == "min_faces":
            return s[:, 1] >= int(spec[1])
        mask = np.zeros(n, dtype=bool)
        mask[np.argsort(-s[:, 1], kind="stable")[:int(spec[1])]] = True                # (stable: equal counts stay in component order -- ties to the lower id)
        return mask
    if isinstance(spec, torch.Tensor):
        spec = spec.detach().cpu().numpy()
    if not isinstance(spec, (np.ndarray, list)):
        raise ValueError(f"select_components: unknown spec {spec!r} ('largest', ('largest', k), ('min_faces', n), a bool mask or a callable)")
    mask = np.asarray(spec)
    if mask.dtype != bool or mask.shape != (n,):
        raise ValueError(f"select_components: a mask must be a bool array of length {n}, got {mask.dtype} {mask.shape}")
    return mask.copy()


def clean_mesh(mesh, spec):
    """the mesh without the components `spec` drops (select_components), on the device: mesh = the dict of NeRFNetwork.extract_colored_mesh(return_torch=True) or
    dict(vertices, triangles) of extract_geometry -- device tensors.  -> a new dict: vertices and every other per-vertex entry (first dimension V: normals, colors,
    sdf, status, ...) gathered through the kept vertices in their order, triangles re-indexed, plus component_sizes [C,2] int64 (of the INPUT mesh) and
    components_kept [C] bool.  A dict with `uv` or `texture` is refused: the atlas addresses its cells by triangle index, so a textured mesh is cleaned before
    the bake (extract_textured_mesh(components=...)), not after."""
    from . import nsr_ops
    if "uv" in mesh or "texture" in mesh:
        raise RuntimeError("clean_mesh: a textured mesh cannot be cleaned (the atlas addresses cells by triangle index): pass components= to extract_textured_mesh")
    v, t = mesh["vertices"], mesh["triangles"]
    if not isinstance(v, torch.Tensor) or not isinstance(t, torch.Tensor) or not v.is_cuda or not t.is_cuda:
        raise RuntimeError("clean_mesh: vertices and triangles must be CUDA tensors (there is no CPU path)")
    V = v.shape[0]
    cc = nsr_ops.mesh_components(t, V)
    keep = select_components(cc["sizes"], spec)
    keep_dev = torch.from_numpy(keep).to(t.device)
    cm = nsr_ops.mesh_compact(t, cc["component"], keep_dev)
    idx = cm["kept_vertices"].long()
    out = {}
    for k, x in mesh.items():
        if k == "triangles":
            out[k] = cm["triangles"]
        elif isinstance(x, torch.Tensor) and x.dim() >= 1 and x.shape[0] == V:
            out[k] = x.index_select(0, idx)
        else:
            out[k] = x
    out["component_sizes"] = cc["sizes"]
    out["components_kept"] = keep_dev
    return out


# ---------------------------------------------------------------------------------------------------- texture atlas (closed form; the kernel restates it in integers)
# The S x S texture is cut into R x R square cells of c x c texels (R = S // c; texels beyond R c belong to nobody).  Triangle t lives in cell k = t >> 1, at
# column k % R and row k // R, in half h = t & 1: texel (i, j) of a cell -- i along x, centre at (i + 0.5, j + 0.5) -- belongs to half 0 iff i + j <= c - 2.
# The UV corners sit ON texel centres, in the triangle's vertex order: half 0 at (1, 1), (c - 4, 1), (1, c - 4), half 1 at (c - 2, c - 2), (3, c - 2), (c - 2, 3);
# legs of L = c - 5 texels, three texel diagonals between the two hypotenuses -- a bilinear lookup inside a UV triangle reads texels of its own half only
# (tests/test_texture_atlas_host.py, exact arithmetic).  Nothing wider (mip levels, anisotropic filters) is guaranteed.
ATLAS_MIN_CELL = 8


def _atlas_cell(n_triangles, size, cell):
    n_triangles, size = int(n_triangles), int(size)
    if n_triangles < 0 or size < 1:
        raise ValueError("atlas: n_triangles >= 0 and size >= 1")
    if cell is None:                                                     # the largest cell whose grid still holds every triangle
        cell = next((c for c in range(size, ATLAS_MIN_CELL - 1, -1) if 2 * (size // c) ** 2 >= n_triangles), None)
        if cell is None:
            raise ValueError(f"atlas: {n_triangles} triangles do not fit a {size} x {size} texture with cells of {ATLAS_MIN_CELL} texels or more")
        return cell
    cell = int(cell)
    if cell < ATLAS_MIN_CELL:
        raise ValueError(f"atlas: cell {cell} < {ATLAS_MIN_CELL}")
    if size < cell or 2 * (size // cell) ** 2 < n_triangles:
        raise ValueError(f"atlas: {n_triangles} triangles, but a {size} x {size} texture of {cell}-texel cells holds 2 (size // cell)^2 = {2 * (size // cell) ** 2}")
    return cell


def atlas_weights(cell):
    """per texel of one cell: (half [c,c] int32, weights [c,c,3] float32), both indexed [j, i] -- the barycentric weights (w0, w1, w2) of the texel in the triangle
    of ITS half, every operation in fp32 and rounded once (ac_mesh_bake_texture's arithmetic); texels outside the UV triangle get a point on it"""
    import numpy as np
    F = np.float32
    c = int(cell)
    j, i = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    half = (i + j > c - 2).astype(np.int32)
    L = F(c - 5)
    w1 = np.maximum(np.where(half == 0, i - 1, c - 2 - i).astype(F) / L, F(0))
    w2 = np.maximum(np.where(half == 0, j - 1, c - 2 - j).astype(F) / L, F(0))
    s = w1 + w2
    over = s > F(1)
    sd = np.where(over, s, F(1))
    w1, w2 = np.where(over, w1 / sd, w1), np.where(over, w2 / sd, w2)
    w0 = np.where(over, F(0), F(1) - s)
    w = np.stack([w0, w1, w2], -1)
    assert w.dtype == F
    return half, w


def atlas_layout(n_triangles, size, cell=None):
    """-> dict(cell, per_row, uv [T,3,2] float64).  cell=None: the largest cell >= 8 with 2 (size // cell)^2 >= n_triangles; ValueError when nothing fits.
    uv in the OBJ convention (u = (x + 0.5) / size, v = 1 - (y + 0.5) / size for the texel centre (x, y), image row 0 on top), one row per triangle corner in the
    triangle's vertex order.  Both halves wind the same way: counter-clockwise in texel coordinates (x, y)."""
    import numpy as np
    c = _atlas_cell(n_triangles, size, cell)
    R = int(size) // c
    t = np.arange(int(n_triangles))
    k, h = t >> 1, t & 1
    corners = np.array([[[1, 1], [c - 4, 1], [1, c - 4]], [[c - 2, c - 2], [3, c - 2], [c - 2, 3]]], np.int64)[h]          # [T,3,2] texel (i, j)
    x = (k % R * c)[:, None] + corners[..., 0]
    y = (k // R * c)[:, None] + corners[..., 1]
    uv = np.stack([(x + 0.5) / float(size), 1.0 - (y + 0.5) / float(size)], -1)
    return dict(cell=c, per_row=R, uv=uv.reshape(-1, 3, 2))


def atlas_owner(n_triangles, size, cell):
    """-> int32 [S,S], indexed [y, x]: the triangle that owns each texel, -1 for nobody (the margin beyond R cell, cells past the last triangle, the second half
    of the last cell of an odd count)"""
    import numpy as np
    c = _atlas_cell(n_triangles, size, cell)
    S = int(size)
    R = S // c
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    cx, cy = x // c, y // c
    i, j = x - cx * c, y - cy * c
    t = 2 * (cy * R + cx) + (i + j > c - 2)
    return np.where((cx < R) & (cy < R) & (t < int(n_triangles)), t, -1).astype(np.int32)


def save_png(path, rgb8):
    """8-bit RGB PNG from a uint8 [H,W,3] array, row 0 on top: one IDAT chunk, filter 0 on every row (zlib and struct only)"""
    import struct
    import zlib
    import numpy as np
    a = np.asarray(rgb8.detach().cpu().numpy() if isinstance(rgb8, torch.Tensor) else rgb8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("save_png: a uint8 [H,W,3] array")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    rows[:, 1:] = a.reshape(H, 3 * W)
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
                 + chunk(b"IEND", b""))


def save_mtl(path, texture, occlusion_texture=None):
    """the material file save_obj references: one material `baked` whose diffuse map is the image `texture` (a file name next to the .mtl);
    occlusion_texture: the file name of the ambient-occlusion image, referenced as the ambient map (map_Ka)"""
    with open(path, "w") as fh:
        fh.write(f"newmtl baked\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {texture}\n")
        if occlusion_texture is not None:
            fh.write(f"map_Ka {occlusion_texture}\n")


def save_obj(path, vertices, triangles, uv, normals=None, texture=None, mtllib=None, occlusion_texture=None):
    """Wavefront OBJ: `v` per vertex, `vt` three per triangle (uv [T,3,2], atlas_layout's), `vn` per vertex, `f a/ta/na b/tb/nb c/tc/nc` (`a/ta` without normals),
    1-based; triangle t uses vt 3t+1 .. 3t+3.  texture: the image's file name -- then a sibling .mtl (same stem) with map_Kd is written and referenced.
    occlusion_texture: with texture, the ambient-occlusion image's file name: the material gets a map_Ka line.
    mtllib: instead, the file name of a material file that exists already (save_mtl) and is only referenced -- the frames of an animation share one.
    Numbers are written with repr, so they read back to the same doubles."""
    import os
    import numpy as np
    arr = lambda a, dt: np.ascontiguousarray((a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)), dtype=dt)
    v, t, w = arr(vertices, np.float64).reshape(-1, 3), arr(triangles, np.int64).reshape(-1, 3), arr(uv, np.float64).reshape(-1, 2)
    if len(w) != 3 * len(t):
        raise ValueError("save_obj: uv must be [T,3,2]")
    out = []
    stem = os.path.splitext(path)[0]
    if texture is not None and mtllib is not None:
        raise ValueError("save_obj: texture (write a sibling .mtl) or mtllib (reference an existing one), not both")
    if occlusion_texture is not None and texture is None:
        raise ValueError("save_obj: occlusion_texture goes into the material that texture= writes")
    if texture is not None:
        save_mtl(stem + ".mtl", texture, occlusion_texture)
        out += [f"mtllib {os.path.basename(stem)}.mtl", "usemtl baked"]
    if mtllib is not None:
        out += [f"mtllib {mtllib}", "usemtl baked"]
    out += ["v %r %r %r" % tuple(r) for r in v.tolist()]
    out += ["vt %r %r" % tuple(r) for r in w.tolist()]
    if normals is not None:
        n = arr(normals, np.float64).reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError("save_obj: one normal per vertex")
        out += ["vn %r %r %r" % tuple(r) for r in n.tolist()]
        out += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a + 1, 3 * k + 1, a + 1, b + 1, 3 * k + 2, b + 1, c + 1, 3 * k + 3, c + 1) for k, (a, b, c) in enumerate(t.tolist())]
    else:
        out += ["f %d/%d %d/%d %d/%d" % (a + 1, 3 * k + 1, b + 1, 3 * k + 2, c + 1, 3 * k + 3) for k, (a, b, c) in enumerate(t.tolist())]
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")
