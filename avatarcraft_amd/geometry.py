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


def save_ply(path, vertices, triangles, normals=None, colors=None):
    """binary little-endian PLY: float32 x y z [nx ny nz], uchar red green blue (round(clip(c, 0, 1) * 255)), faces as `list uchar int vertex_indices`.
    vertices [V,3], triangles [F,3], normals [V,3], colors [V,3] in [0, 1]: numpy arrays or tensors on any device."""
    import numpy as np
    arr = lambda a, dt: np.ascontiguousarray((a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)), dtype=dt)
    v, t = arr(vertices, "<f4").reshape(-1, 3), arr(triangles, "<i4").reshape(-1, 3)
    cols, props = [("xyz", "<f4", (3,))], ["float x", "float y", "float z"]
    if normals is not None:
        cols.append(("n", "<f4", (3,))); props += ["float nx", "float ny", "float nz"]
    if colors is not None:
        cols.append(("rgb", "u1", (3,))); props += ["uchar red", "uchar green", "uchar blue"]
    vert = np.empty(len(v), dtype=cols)
    vert["xyz"] = v
    if normals is not None:
        vert["n"] = arr(normals, "<f4").reshape(-1, 3)
    if colors is not None:
        vert["rgb"] = np.round(np.clip(arr(colors, "<f8").reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
    face = np.empty(len(t), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    face["n"] = 3; face["idx"] = t
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + ["property " + p for p in props]
    head += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vert.tobytes()); fh.write(face.tobytes())
