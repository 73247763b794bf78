"""Mesh export on the device: the SDF grid, its iso-surface, the coloured and the textured mesh, and the exported mesh in the pose of a frame."""
import collections

import numpy as np
import torch

from .. import nsr_ops


def _native_ok(net):
    """the native mesher, the vertex shading and the first-hit renderers run the fused field code: the default SDF side, on the GPU"""
    return net.encoder.embeddings.is_cuda and net._sdf_supported()


def _check_model(net, needs, colors=None, ok=True):
    """THE model requirement of the export and the surface renders.  needs: the caller's message up to the requirement; ok: what else the caller asks for
    in the same breath (its mesher); colors: None, or (the caller's name, what it offers without colours) where the colour side is wanted too."""
    if not (ok and _native_ok(net)):
        raise RuntimeError(f"{needs} the default SDF side of NeRFNetwork on the GPU")
    if colors is not None and not net._fused_supported(ignore_curvature=True):
        raise RuntimeError(f"{colors[0]}: the colour side of this model is not the default one (colour net 21-64-64-3, or 37-64-64-3 with the degree-4 "
                           f"view-direction encoder); {colors[1]}")


# what the native pipeline hands on: the mesh, and what its steps learned (None where a step did not run); max_move: how far a vertex may be projected
_NativeMesh = collections.namedtuple("_NativeMesh", "vertices triangles component_sizes components_kept cluster_members max_move weld repair")


def _native_mesh(net, bound, resolution, threshold, slab_layers, components, grid):
    """THE native mesh pipeline, device tensors throughout: marching cubes on the whole volume or streamed in slabs -> geometry.clean_mesh (components) ->
    mesh_decimate.decimate_mesh (grid: cluster_grid's result, made by the public call before any device work) -> mesh_weld.weld_mesh (net.export_weld) ->
    mesh_repair.repair_mesh (net.export_manifold)"""
    bmin, bmax = np.float32(-bound), np.float32(bound)                       # (the reference's bounds are float32 tensors, :712)
    xf = dict(den=resolution - 1.0, span=[float(bmax - bmin)] * 3, lo=[float(bmin)] * 3)
    if slab_layers is None:
        u = net.extract_fields_device(bound, resolution, negate=True)
        v, t = nsr_ops.marching_cubes(u, float(threshold), **xf)
    else:
        ax = net._grid_axis(bound, resolution)
        with torch.no_grad():
            f = net._field_for()
            fill = lambda x0, out: nsr_ops.field_sdf_grid(f, ax[x0:x0 + out.shape[0]], ax, ax, bound, negate=True, out=out)
            v, t = nsr_ops.marching_cubes_streamed(fill, resolution, resolution, resolution, slab_layers=slab_layers, iso=float(threshold),
                                                   device=ax.device, **xf)
    sizes = kept = members = weld = repair = None
    max_move = 2.0 * bound / (resolution - 1.0)
    if components is not None:
        from ..geometry import clean_mesh
        m = clean_mesh(dict(vertices=v, triangles=t), components)
        v, t, sizes, kept = m["vertices"], m["triangles"], m["component_sizes"], m["components_kept"]
    if grid is not None:
        from ..mesh_decimate import decimate_mesh
        m = decimate_mesh(dict(vertices=v, triangles=t), grid)
        v, t, members, max_move = m["vertices"], m["triangles"], m["cluster_members"], grid["h"]
    if net.export_weld:
        from ..mesh_weld import weld_mesh
        m = weld_mesh(dict(vertices=v, triangles=t) if members is None else dict(vertices=v, triangles=t, cluster_members=members))
        v, t, members, weld = m["vertices"], m["triangles"], m.get("cluster_members"), m["weld"]
    if net.export_manifold:
        from ..mesh_repair import repair_mesh
        m = repair_mesh(dict(vertices=v, triangles=t) if members is None else dict(vertices=v, triangles=t, cluster_members=members))
        v, t, members, repair = m["vertices"], m["triangles"], m.get("cluster_members"), m["repair"]
    return _NativeMesh(v, t, sizes, kept, members, max_move, weld, repair)


def _host(mesh):
    """the mesh dict with its device tensors as numpy arrays (the weld report, a plain dict, stays what it is)"""
    return {k: x.cpu().numpy() if isinstance(x, torch.Tensor) else x for k, x in mesh.items()}


def _occlusion_kit(occlusion, bound, threshold):
    """occlusion (None, True, occlusion_kit's keywords or a kit) -> None, or the checked kit at the export's level; a bad one raises here, before any device work"""
    if occlusion is None:
        return None
    from ..mesh_occlusion import resolve_kit
    return resolve_kit(occlusion, bound, level=-float(threshold))


def _cluster_grid(bound, resolution, decimate):
    """decimate (None, or the k of mesh_decimate.cluster_grid) -> None, or the cluster grid; a bad k raises here, before any device work"""
    if decimate is None:
        return None
    from ..mesh_decimate import cluster_grid
    return cluster_grid(bound, resolution, decimate)


class MeshExport:
    """mixed into NeRFNetwork"""

    # opt-in switch of extract_colored_mesh / extract_textured_mesh (their signatures are frozen: tests/test_instant_nsr_package_host.py): None = what they always
    # returned; True = ambient occlusion from the default kit (mesh_occlusion.occlusion_kit, radius 0.1 bound); a dict = occlusion_kit's keywords, or a kit, passed
    # as is.  drivers.export_mesh / export_animation(occlusion=...) set it for the length of their call.
    export_occlusion = None

    # opt-in switch of extract_geometry / extract_colored_mesh / extract_textured_mesh (same reason): False = what they always returned; True = the mesh is
    # welded on the device (mesh_weld.weld_mesh) after the decimation -- after the cleaning without one -- and before anything is shaded, laid out or baked:
    # repeated triangles and back-to-back pairs of a collapsed thin part go, and so do the vertices nobody names any more.  The dicts then carry `weld`, the
    # report of mesh_weld.mesh_weld.  Native mesher only.  drivers.export_mesh / export_animation(weld=True) set it for the length of their call.
    export_weld = False

    # opt-in switch of the same three (same reason): False = what they always returned; True = the mesh is made manifold on the device
    # (mesh_repair.repair_mesh) after the weld -- after the decimation or the cleaning when the weld is off -- and before anything is shaded, laid out or baked:
    # where clustering pushed two sheets of the surface onto one edge or one vertex, every sheet gets its own copy of the vertex.  No triangle is added, dropped
    # or turned; the copies of a split vertex start at one position and the export's own projection moves them identically, so the result holds COINCIDENT
    # vertices that the index buffer keeps apart.  The dicts then carry `repair`, the report of mesh_repair.mesh_repair.  Native mesher only.
    # drivers.export_mesh / export_animation(manifold=True) set it for the length of their call.
    export_manifold = False

    def _grid_axis(self, bound, resolution):
        """torch.linspace(-bound, bound, resolution) as the reference forms it (on the host, fp32: extract_fields :730-732, update_extra_state :312-314), on the
        device.  Cached: the axis of the density grid is asked for once per epoch, the mesh export's once per export."""
        dev = self.encoder.embeddings.device
        key = (float(bound), int(resolution), str(dev))
        c = self.__dict__.setdefault("_axis_cache", {})
        if key not in c:
            if len(c) > 8:
                c.clear()
            c[key] = torch.linspace(-bound, bound, resolution).to(dev)
        return c[key]

    def extract_fields_device(self, bound: float, resolution: int, negate: bool = False, slab_layers=None):
        """the SDF (negate: -SDF) on the resolution^3 grid over [-bound, bound]^3 as a device tensor [res, res, res]: ONE launch (ac_field_sdf_grid) -- the
        kernel forms the grid points from the axis table; no meshgrid / cat tensors, no 256^3 blocks, no host round trip.
        slab_layers is refused: a streamed volume (extract_geometry(slab_layers=...)) is never whole."""
        if slab_layers is not None:
            raise RuntimeError("extract_fields_device: slab_layers is refused here -- a streamed volume is never whole; extract_geometry(slab_layers=...) meshes it slab by slab")
        _check_model(self, "extract_fields_device: needs")
        ax = self._grid_axis(bound, resolution)
        with torch.no_grad():
            return nsr_ops.field_sdf_grid(self._field_for(), ax, ax, ax, bound, negate=negate)

    def extract_fields(self, bound: float, resolution: int):
        """the SDF on a resolution^3 grid over [-bound, bound]^3 (extract_fields, reference :728-745); returns a float32 numpy array
        [res, res, res] like the reference.  On the GPU: extract_fields_device + one copy to the host."""
        if _native_ok(self):
            return self.extract_fields_device(bound, resolution).cpu().numpy()
        N = 256
        dev = self.encoder.embeddings.device
        xs = torch.linspace(-bound, bound, resolution).split(N)
        u = torch.empty([resolution] * 3, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for xi, x in enumerate(xs):
                for yi, y in enumerate(xs):
                    for zi, z in enumerate(xs):
                        xx, yy, zz = torch.meshgrid(x, y, z, indexing="ij")
                        pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)
                        u[xi * N: xi * N + len(x), yi * N: yi * N + len(y), zi * N: zi * N + len(z)] = self.density(pts, bound).reshape(len(x), len(y), len(z))
        return u.cpu().numpy()

    def extract_geometry(self, bound: float, resolution: int, threshold: int = 0.0, device=None, mesher=None, return_torch=False, slab_layers=None, components=None,
                         decimate=None):
        """iso-surface of the SDF (reference :706-764; its one call is extract_geometry(NSR_BOUND, 512), stylize.py:267): vertices [V,3] float64 in world
        units, triangles [F,3].  The reference runs PyMCubes' marching_cubes on u = -sdf (third party, not in this image).
        mesher: "native" (default on the GPU) = ac_field_sdf_grid + ac_marching_cubes on the device: the volume never leaves it, one shared vertex per
                sign-changing grid edge at the linear zero crossing, the 256-case table of the definition, triangles oriented out of the body; only the
                finished mesh is copied to the host (return_torch=True: not even that -- device tensors);
                "mcubes" = the reference's own call when PyMCubes is installed; "tetra" = the marching-tetrahedra mesher of round 3 (geometry.py:
                the same vertex set, a different triangulation -- kept as the cross-check of the tests).
        slab_layers: None = the whole volume at once (9 bytes per grid point, fewer than 2^31 points: resolution <= 1290); an integer >= 2 = the native mesher
                STREAMED (nsr_ops.marching_cubes_streamed): the grid is evaluated slab_layers x-layers at a time into one window of slab_layers + 2 layers and
                meshed window by window -- the same mesh bit for bit, in the memory of one window, at any resolution whose window stays below 2^31 points
                (extract_geometry(1.6, 2048, slab_layers=64): the hash grid's own finest resolution, 0.92 s).  Multiples of 16 keep the x-tiles of the grid kernel
                full; other values are legal.  Needs mesher "native" (or None on the GPU).
        components: None = every connected component the field has, floaters included (as ever); a spec of geometry.select_components -- "largest",
                ("largest", k), ("min_faces", n), a bool mask or a callable on the size table -- = only those components, labelled and compacted on the device
                (geometry.clean_mesh: order preserved, so the dense and the streamed route give the same cleaned mesh).  Native mesher only.
        decimate: None = every marching-cubes triangle (as ever); a real k >= 1 = the vertices of every cluster cell of k marching-cubes cells merged on the device
                (mesh_decimate.cluster_grid / decimate_mesh: vertex clustering, order preserved, the same from run to run and on the dense and the streamed
                route), AFTER the components are cleaned, so that a floater never merges into the body.  This call has no field pass: with decimate the vertices
                are the clusters' MEAN vertices, near the level set and not on it (at most about one cluster cell off) -- extract_colored_mesh /
                extract_textured_mesh(decimate=k) project them back.  Triangles that lose a corner to a merge are dropped; duplicates are not removed and the
                result need not be manifold (self.export_weld, the switch above, removes them).  Native mesher only."""
        native = mesher in (None, "native")
        grid = None
        if decimate is not None:
            _check_model(self, "extract_geometry(decimate=...) decimates the native mesher's mesh on the device: it needs mesher='native' and", ok=native)
            grid = _cluster_grid(bound, resolution, decimate)
        if self.export_weld:
            _check_model(self, "extract_geometry with export_weld welds the native mesher's mesh on the device: it needs mesher='native' and", ok=native)
        if self.export_manifold:
            _check_model(self, "extract_geometry with export_manifold repairs the native mesher's mesh on the device: it needs mesher='native' and", ok=native)
        if components is not None:
            _check_model(self, "extract_geometry(components=...) cleans the native mesher's mesh on the device: it needs mesher='native' and", ok=native)
        if slab_layers is not None:
            slab_layers = nsr_ops.check_slab_layers(slab_layers, "extract_geometry")
            _check_model(self, "extract_geometry(slab_layers=...) streams the native mesher: it needs mesher='native' and", ok=native)
        if mesher is None:
            mesher = "native" if _native_ok(self) else "tetra"
        if mesher == "native":
            _check_model(self, "extract_geometry(mesher='native') needs")
            v, t = _native_mesh(self, bound, resolution, threshold, slab_layers, components, grid)[:2]
            return (v, t) if return_torch else (v.cpu().numpy(), t.cpu().numpy())
        u = -1.0 * self.extract_fields(bound, resolution)
        if mesher == "mcubes":
            import mcubes
            vertices, triangles = mcubes.marching_cubes(u, threshold)
        elif mesher == "tetra":
            from ..geometry import marching_tetrahedra
            v, t = marching_tetrahedra(torch.from_numpy(u).to(self.encoder.embeddings.device), float(threshold))
            vertices, triangles = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
        else:
            raise ValueError(f"extract_geometry: unknown mesher {mesher!r}")
        vertices = vertices / (resolution - 1.0) * (2 * bound) - bound
        return vertices, triangles

    def _colored_mesh(self, bound, resolution, threshold, refine_steps, tol, colors, slab_layers, components, decimate, kit=None):
        """extract_colored_mesh on the device -> (its dict of device tensors, the max_move its vertices were projected with: the bake's as well)"""
        if slab_layers is not None:
            slab_layers = nsr_ops.check_slab_layers(slab_layers, "extract_colored_mesh")
        grid = _cluster_grid(bound, resolution, decimate)
        _check_model(self, "extract_colored_mesh needs",
                     colors=("extract_colored_mesh(colors=True)", "colors=False exports positions and normals") if colors else None)
        m = _native_mesh(self, bound, resolution, threshold, slab_layers, components, grid)
        with torch.no_grad():
            a = nsr_ops.mesh_vertex_attrs(self._field_for(ignore_curvature=True), m.vertices, bound, nsr_ops.FD_STEP, refine_steps=refine_steps, tol=tol,
                                          max_move=m.max_move, target_sdf=-float(threshold), want_rgb=colors)
        out = dict(vertices=a["positions"].double(), triangles=m.triangles, normals=a["normals"], sdf=a["sdf"], status=a["status"])
        if colors:
            out["colors"] = a["rgb"]
        if kit is not None:
            from ..mesh_occlusion import field_occlusion
            with torch.no_grad():                     # (a vertex without a gradient, status 2, has no normal to open a cone around)
                out["occlusion"] = field_occlusion(self._field_for(ignore_curvature=True), a["positions"], a["normals"], bound, kit, active=a["status"] != 2)
        if m.component_sizes is not None:
            out.update(component_sizes=m.component_sizes, components_kept=m.components_kept)
        if m.cluster_members is not None:
            out["cluster_members"] = m.cluster_members
        if m.weld is not None:
            out["weld"] = m.weld
        if m.repair is not None:
            out["repair"] = m.repair
        return out, m.max_move

    def extract_colored_mesh(self, bound: float, resolution: int, threshold: float = 0.0, refine_steps: int = 3, tol: float = 1e-5, colors: bool = True,
                             return_torch=False, slab_layers=None, components=None, decimate=None):
        """the mesh of extract_geometry(mesher="native") with what a viewer wants on it (the reference's save_mesh, stylize.py:263-269, writes bare geometry):
        every vertex projected from the grid edge's linear zero crossing onto the level set sdf = -threshold (at most refine_steps Newton steps along the
        finite-difference gradient, never further than one grid cell), the field's normal and the colour network there -- one launch over the marching-cubes
        buffer (ac_mesh_vertex_attrs).  -> dict(vertices [V,3] float64, triangles [F,3] int32 (extract_geometry's), normals [V,3] float32, colors [V,3]
        float32 in [0, 1] (colors=True), sdf [V] at the final positions, status [V] uint8: 0 converged to tol, 1 all steps taken (sdf tells how close), 2 degenerate gradient,
        3 stopped by the one-cell limit); numpy arrays, or device tensors with return_torch=True.  With view directions the colour is the one seen along -normal.
        colors=True needs the default colour side (RuntimeError otherwise); colors=False works wherever extract_geometry(mesher="native") does.
        slab_layers: extract_geometry's (None: the whole volume at once; an integer: streamed, the same mesh in the memory of one window).
        components: extract_geometry's (None: every component).  The mesh is cleaned right after the geometry and BEFORE the vertices are shaded: a dropped vertex
        costs nothing, and a kept one gets what it would have got (the attributes are per vertex).  The dict then also carries component_sizes [C,2] (vertices,
        triangles of every component of the unfiltered mesh) and components_kept [C] bool.
        decimate: extract_geometry's (None: every triangle; k: clusters of k marching-cubes cells).  The mesh is decimated after the cleaning and BEFORE the
        vertices are shaded: no removed vertex is ever shaded, and every kept one is projected from its cluster's mean onto the level set, never further than one
        CLUSTER cell (k grid cells) instead of one grid cell.  The dict then also carries cluster_members [V] (how many marching-cubes vertices each vertex
        stands for).
        self.export_occlusion (the switch above; None: nothing more, as ever) adds ambient occlusion.  The kit's level is -threshold.  The dict then also carries
        occlusion [V] float32 in [0, 1], 1 = open: mesh_occlusion.field_occlusion at the final positions and normals (after cleaning and decimation), 0 at a
        status-2 vertex.  The colours are unlit albedo; a viewer multiplies.
        self.export_weld (the switch above; False: nothing more, as ever) welds the mesh after the decimation and BEFORE the vertices are shaded: a vertex that no
        surviving triangle names is never projected, coloured or posed.  The dict then also carries weld (the report, a plain dict of counts).
        self.export_manifold (the switch above; False: nothing more, as ever) splits non-manifold edges and vertices after the weld and BEFORE the vertices are
        shaded: the copies of a split vertex start at one position, are projected identically and so stay COINCIDENT -- the same position, normal and colour under
        different indices.  The dict then also carries repair (the report of mesh_repair.mesh_repair)."""
        kit = _occlusion_kit(self.export_occlusion, bound, threshold)
        out = self._colored_mesh(bound, resolution, threshold, refine_steps, tol, colors, slab_layers, components, decimate, kit)[0]
        return out if return_torch else _host(out)

    def extract_textured_mesh(self, bound: float, resolution: int, texture_size: int = 2048, cell=None, threshold: float = 0.0, refine_steps: int = 3,
                              tol: float = 1e-5, return_torch=False, slab_layers=None, components=None, decimate=None):
        """extract_colored_mesh's mesh with the colour network baked into a texture instead of sampled at the vertices, so that colour detail no longer depends on
        the vertex density: every triangle gets half a cell of a closed-form texture_size^2 atlas (geometry.atlas_layout; cell=None: the largest that fits), every
        owned texel's point on its triangle is projected onto the level set like a vertex (never further than one grid cell) and shaded there, one launch
        (ac_mesh_bake_texture).  -> the dict of extract_colored_mesh plus uv [T,3,2] float64 (three corners per triangle, OBJ convention), texture [S,S,3] uint8
        (q = floor(clamp(x, 0, 1) 255 + 0.5), row 0 on top), owner [S,S] int32 (-1: nobody, texture 0), texel_sdf [S,S], texel_status [S,S] uint8.
        The atlas guarantees bilinear lookups only (no mip chain).  Same model requirements as extract_colored_mesh(colors=True).
        slab_layers: extract_geometry's; an atlas too small for the triangle count of a finer mesh raises as ever.
        components: extract_colored_mesh's.  The mesh is cleaned BEFORE the atlas is laid out, so the cells are sized for the kept triangles only: debris no longer
        lowers the texel density of the body.
        decimate: extract_colored_mesh's.  The mesh is decimated BEFORE the atlas is laid out, so the cells are sized for the decimated triangle count, and the
        texels carry the colour detail the removed vertices carried; a texel's point is projected never further than one CLUSTER cell.
        self.export_occlusion: as in extract_colored_mesh.  The dict then also carries occlusion [V], texel_occlusion [S,S] float32 (0 at unowned texels) and occlusion_map [S,S]
        uint8 (the texture's quantisation rule), the texels' from ONE launch (ac_mesh_bake_maps) in place of the bake's: colour and occlusion share a texel's refine.
        self.export_weld: as in extract_colored_mesh.  The mesh is welded BEFORE the atlas is laid out: the cells are sized for the welded triangle count.
        self.export_manifold: as in extract_colored_mesh (coincident copies of the split vertices); the repair keeps every triangle and its place, so the atlas
        is the one the unrepaired mesh would get."""
        from ..geometry import atlas_layout
        kit = _occlusion_kit(self.export_occlusion, bound, threshold)
        m, max_move = self._colored_mesh(bound, resolution, threshold, refine_steps, tol, True, slab_layers, components, decimate, kit)
        T = m["triangles"].shape[0]
        try:
            lay = atlas_layout(T, texture_size, cell)
        except ValueError as e:
            raise RuntimeError(f"extract_textured_mesh: {e}") from e
        quantise = lambda x: torch.floor(x.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
        with torch.no_grad():
            how = dict(refine_steps=refine_steps, tol=tol, max_move=max_move, target_sdf=-float(threshold))
            if kit is None:
                b = nsr_ops.mesh_bake_texture(self._field(), m["vertices"].float(), m["triangles"], texture_size, lay["cell"], bound, nsr_ops.FD_STEP, **how)
            else:
                from ..mesh_occlusion import mesh_bake_maps
                b = mesh_bake_maps(self._field(), m["vertices"].float(), m["triangles"], texture_size, lay["cell"], bound, nsr_ops.FD_STEP, kit=kit,
                                   want=("rgb", "sdf", "status"), **how)
            tex = quantise(b["rgb"])
        m.update(texture=tex, owner=b["owner"], texel_sdf=b["sdf"], texel_status=b["status"])
        if kit is not None:
            m.update(texel_occlusion=b["occlusion"], occlusion_map=quantise(b["occlusion"]))
        if not return_torch:
            m = _host(m)
        m["uv"] = torch.from_numpy(lay["uv"]).to(tex.device) if return_torch else lay["uv"]
        return m

    def pose_mesh(self, mesh, body_guide, verts, Ts=None, iters: int = 3, tol: float = 1e-5):
        """the exported mesh in the pose of one frame: the dict of extract_colored_mesh / extract_textured_mesh with its `vertices` moved to where the posed
        renderer draws them -- the p with W^-1(p) = vertex, W^-1 the SMPL-guided inverse warp of the frame (ac_mesh_pose: at most iters fixed-point steps from a
        start bound to the canonical guide, iters + 1 closest-face searches) -- and its `normals` carried along by the blended transform's cofactor matrix.
        body_guide: dict(faces [F,3] of the SMPL guide, and `canonical` [Vg,3], the guide in canonical space; absent: geometry.canonical_guide(verts, Ts), which
        is frame independent, is stored there).  The binding of the mesh to the guide (ac_mesh_bind: once per mesh, pose independent) is stored as
        body_guide["bind"] on the first call and reused: keep one body_guide per exported mesh.
        verts [Vg,3], Ts [>= Vg,4,4]: the frame's posed guide and transforms (calc_local_trans), or verts = an nsr_ops.WarpMesh of the frame (Ts unused).
        -> a shallow copy of `mesh` with vertices (float64, the input's convention), normals, and per vertex residual (float32: max-norm of W^-1(p) - vertex at
        the returned p), status (uint8: 0 within tol, 1 iters used up, 2 not finite) and mask (uint8: 0 = farther from the guide than the renderer's mask
        threshold, where it would draw nothing; kept and flagged); the export's own `status` (of the level-set projection) is replaced: read it from `mesh`.  triangles, uv, texture, colors and every other entry are the input's own objects --
        `occlusion` among them: it is the CANONICAL pose's, carried to every frame (per-frame occlusion is not built).
        numpy in, numpy out; device tensors in, device tensors out."""
        from ..geometry import canonical_guide
        dev = self.encoder.embeddings.device
        if dev.type != "cuda":
            raise RuntimeError("pose_mesh needs the model on the GPU (there is no CPU path)")
        as_torch = isinstance(mesh["vertices"], torch.Tensor)
        to_dev = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
        wm = verts if isinstance(verts, nsr_ops.WarpMesh) else None
        if "bind" not in body_guide:
            if "canonical" not in body_guide:
                if wm is not None:
                    raise RuntimeError("pose_mesh: body_guide needs `canonical` when the frame arrives as a WarpMesh")
                body_guide["canonical"] = canonical_guide(verts, Ts)
            body_guide["bind"] = nsr_ops.mesh_bind(to_dev(mesh["vertices"], torch.float32), to_dev(body_guide["canonical"], torch.float32),
                                                   to_dev(np.asarray(body_guide["faces"])[:, :3] if not isinstance(body_guide["faces"], torch.Tensor)
                                                          else body_guide["faces"][:, :3], torch.int32))
        if wm is None:
            wm = nsr_ops.WarpMesh(verts, body_guide["faces"], Ts, dev)
        n = mesh.get("normals")
        with torch.no_grad():
            a = nsr_ops.mesh_pose(to_dev(mesh["vertices"], torch.float32), None if n is None else to_dev(n, torch.float32), body_guide["bind"], wm,
                                  iters=iters, tol=tol)
        out = dict(mesh)
        new = dict(vertices=a["positions"].double(), residual=a["residual"], status=a["status"], mask=a["mask"])
        if n is not None:
            new["normals"] = a["normals"]
        out.update(new if as_torch else {k: x.cpu().numpy() for k, x in new.items()})
        return out
