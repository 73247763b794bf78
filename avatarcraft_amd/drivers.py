"""The two inference drivers of the reference as functions (no file I/O, no option parsing): the main loops of render_canonical.py:38-99
(360-degree views of the canonical avatar, body and head rings) and render_warp.py:40-125 (SMPL-driven animation / shape
interpolation through the posed-space renderer), plus the camera of the latter, SMPLDataset.gen_rays_pose (utils/SMPLDataset.py:86-103); and the one
drivers that do write files: export_mesh, the coloured form of the trainer's extract_geometry + save_mesh (stylize.py:263-269), and export_animation, the
same mesh posed frame by frame (render_warp.py's sequence as geometry instead of pixels)."""
import contextlib

import numpy as np
import torch

from .render_utils import (default_360_path, pose2cap, cap2rays, render_instantnsr_naive, WHITE_BKG, BLACK_BKG, NSR_BOUND)
from .smpl import calc_local_trans

CANONICAL_CAMERA_DIST_VAL = 1.7         # render_canonical.py:35 (overrides utils/constant.py for the supplementary video)
CAN_HEAD_OFFSET = 0.47 * 0.9            # utils/constant.py:35,43
CAN_HEAD_CAMERA_DIST = 0.5 * 0.9        # utils/constant.py:36,42


def gen_rays_pose(pose, resolution_level=1, H=512, W=512, camera_angle_x=np.pi / 3, device="cuda"):
    """rays of the 512x512 dataset camera with field of view camera_angle_x (focal = 0.5 W / tan(0.5 fov)) for a camera-to-world
    `pose` [4,4], sub-sampled on linspace(0, W-1, W // level): -> rays_o, rays_d [H//level, W//level, 3] fp32"""
    focal = .5 * W / np.tan(.5 * camera_angle_x)
    pose = torch.as_tensor(np.asarray(pose, dtype=np.float32) if not isinstance(pose, torch.Tensor) else pose).to(device=device, dtype=torch.float32)
    l = resolution_level
    tx = torch.linspace(0, W - 1, int(W // l))
    ty = torch.linspace(0, H - 1, int(H // l))
    px, py = torch.meshgrid(tx, ty, indexing="ij")
    px, py = px.t().to(device), py.t().to(device)
    K = torch.tensor([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]], dtype=torch.float64)
    p = torch.stack([(px - K[0][2]) / K[0][0], -(py - K[1][2]) / K[1][1], -torch.ones_like(px)], -1).float()
    v = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
    v = torch.sum(v[..., None, :] * pose[:3, :3], -1)
    o = pose[None, None, :3, 3].expand(v.shape)
    return o, v


def _rank_world(rank, world):
    """(rank, world) of this process: explicit arguments win, else the default process group, else (0, 1)"""
    if rank is None or world is None:
        on = torch.distributed.is_available() and torch.distributed.is_initialized()
        rank = (torch.distributed.get_rank() if on else 0) if rank is None else rank
        world = (torch.distributed.get_world_size() if on else 1) if world is None else world
    rank, world = int(rank), int(world)
    if not (world >= 1 and 0 <= rank < world):
        raise ValueError(f"rank {rank} / world {world}: need 0 <= rank < world")
    return rank, world


def shard_indices(n, rank=None, world=None):
    """Multi-GPU inference ("partition the views across ranks", every rank a full replica of the 49 MB table + MLPs, no collective on
    the data path): the view / frame indices rank `rank` of `world` renders -- round robin (rank, rank + world, ...), so that consecutive frames of
    an animation land on different GPUs and the ranks finish together whatever n % world is.  Defaults: the default process group, else everything."""
    rank, world = _rank_world(rank, world)
    return list(range(rank, int(n), world))


def render_canonical_360(net, n_views=100, render_hw=(256, 256), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), white_bkg=True, with_head=True,
                         rays_per_batch=4096, device="cuda", rank=None, world=None, table_dtype=None, surface=False):
    """yields (ring name, view index, rgb [H,W,3] float32 in [0,1], depth [H,W]) for the body ring and, with_head, the head ring.
    surface=True: the same tuple from net.render_surface -- the first-hit render of the level set (the surface export_mesh writes) instead of the volumetric one,
    a view in one launch; its depth is the METRIC distance along the ray (0 where nothing is hit), not the near/far-normalised depth of the default.
    table_dtype does not apply to it.
    table_dtype: None (default) leaves net.render_table_dtype as the caller set it; "float" / "half" sets it around each view's render and restores it
    (also when the consumer abandons the generator).  "half" takes effect for a net in eval() mode (NeRFNetwork.render_table_dtype).
    rank / world: this process renders the views shard_indices(n_views, rank, world) of every ring (default: its rank in the default process group;
    without one, all views) -- the view index yielded is the GLOBAL one, so the ranks' outputs interleave into the reference's file sequence."""
    center, up = np.asarray(center, dtype=np.float64), np.asarray(up, dtype=np.float64)
    mine = set(shard_indices(n_views, rank, world))
    rings = [("body", default_360_path(center, up, CANONICAL_CAMERA_DIST_VAL, n_views)[0])]
    if with_head:
        rings.append(("head", default_360_path(center + up * CAN_HEAD_OFFSET, up, CAN_HEAD_CAMERA_DIST, n_views)[0]))
    h, w = render_hw
    for name, poses in rings:
        for i, pose in enumerate(poses):
            if i not in mine:
                continue
            ro, rd = cap2rays(pose2cap([h, w], pose), device=device)
            if surface:
                with torch.no_grad():
                    r = net.render_surface(ro.reshape(1, -1, 3), rd.reshape(1, -1, 3), NSR_BOUND, bg_color=None if white_bkg else 0.0)
                yield name, i, r["rgb"].reshape(h, w, 3), r["depth"].reshape(h, w)
                continue
            prev_table = getattr(net, "render_table_dtype", None)
            if table_dtype is not None and prev_table is not None:
                net.render_table_dtype = table_dtype
            try:
                rgb, _, extra = render_instantnsr_naive(net, ro, rd, rays_per_batch, requires_grad=False, bkg_key=WHITE_BKG if white_bkg else BLACK_BKG,
                                                        return_torch=True, perturb=False, return_raw=True, render_can=True)
            finally:
                if table_dtype is not None and prev_table is not None:
                    net.render_table_dtype = prev_table
            yield name, i, rgb.reshape(h, w, 3), extra["depth"].reshape(h, w)


def render_animation(net, body_model, cam_pose, poses=None, render_type="animate", shape_from=None, shape_to=None, resolution=256, max_frames=100,
                     white_bkg=True, rays_per_batch=None, device="cuda", rank=None, world=None, num_steps=32, upsample_steps=32, table_dtype=None, surface=False):
    """yields (frame index, rgb [res,res,3]) for an SMPL pose sequence (render_type "animate", poses [F,72]) or a shape interpolation
    ("interp_shape", shape_from / shape_to [1,10]), seen from the dataset camera `cam_pose` [4,4]; 32 + 32 samples per ray like the reference.
    num_steps / upsample_steps: render_warp.py's two command-line counts; outside the fused renderer's window (multiples of 16, num_steps <= 64, at most 128
    samples) the frames go to the long posed renderer (num_steps >= 2, upsample_steps a multiple of 16, at most 512 samples): net.posed_long_rays is
    switched on for the duration, like skip_masked_samples.
    table_dtype: None (default) leaves net.render_table_dtype alone; "float" / "half" sets it around each frame's render and restores it, like the two
    switches above ("half": a net in eval() mode, counts inside the fused renderer's window -- NeRFNetwork.render_table_dtype).
    rays_per_batch: the reference cuts a frame into 64 * 128 = 8192-ray batches (render_warp.py) to bound its memory; the default here is the whole
    frame in one batch (0.13 GB of scratch at 256 x 256): same pixels, and the launches are full when the body covers a fraction of the image.
    surface=True: every frame is the first-hit render of the posed level set instead (net.render_surface_posed, one call per frame at its default
    options, on the GPU only) and the generator yields (frame index, rgb [res,res,3], depth [res,res]: the distance along the ray, 0 where nothing is hit);
    the sample counts, rays_per_batch and table_dtype do not apply.
    rank / world: this process renders the frames shard_indices(n_frames, rank, world) (default: its rank in the default process group; without one,
    every frame); the frame index yielded is the global one.  The SMPL forward of the sequence (calc_local_trans: a few ms) runs on every rank."""
    if rays_per_batch is None:
        rays_per_batch = resolution * resolution
    world_verts, Ts, n_frames = calc_local_trans(body_model, render_type=render_type, poses=poses, shape_from=shape_from, shape_to=shape_to,
                                                 max_frames=max_frames)
    faces = np.asarray(body_model.faces)
    ro, rd = gen_rays_pose(cam_pose, int(512 / resolution), device=device)
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    mine = list(shard_indices(n_frames, rank, world))
    # one WarpMesh per frame, the next frame's upload + culling structure prepared beside the current frame's render (nsr_ops.warp_mesh_sequence)
    if torch.device(device).type == "cuda":
        from . import nsr_ops
        meshes = nsr_ops.warp_mesh_sequence(((world_verts[i], Ts[i]) for i in mine), faces, device)
    else:
        meshes = (None for _ in mine)
    for i, mesh in zip(mine, meshes):
        if surface:
            if mesh is None:
                raise RuntimeError("render_animation(surface=True) needs the GPU (there is no CPU path)")
            with torch.no_grad():
                r = net.render_surface_posed(ro[None], rd[None], NSR_BOUND, mesh, faces, Ts[i], bg_color=None if white_bkg else 0.0)
            yield i, r["rgb"].reshape(resolution, resolution, 3), r["depth"].reshape(resolution, resolution)
            continue
        # the loop keeps rgb only: samples the warp masks out (alpha * 0) need no field evaluation (bit-identical pixels).  The switch is set around
        # each frame's render and restored (also when the consumer abandons the generator): the caller's net keeps its documented default
        prev = getattr(net, "skip_masked_samples", None)
        prev_long = getattr(net, "posed_long_rays", None)
        if prev is not None:
            net.skip_masked_samples = True
        if prev_long is not None:
            net.posed_long_rays = True
        prev_table = getattr(net, "render_table_dtype", None)
        if table_dtype is not None and prev_table is not None:
            net.render_table_dtype = table_dtype
        try:
            rgb, _, _ = render_instantnsr_naive(net, ro, rd, rays_per_batch, requires_grad=False, bkg_key=WHITE_BKG if white_bkg else BLACK_BKG,
                                                return_torch=True, perturb=False, return_raw=True, render_can=False,
                                                verts=mesh if mesh is not None else world_verts[i], faces=faces, Ts=Ts[i], num_steps=num_steps,
                                                upsample_steps=upsample_steps, bound=NSR_BOUND)
        finally:
            if prev is not None:
                net.skip_masked_samples = prev
            if prev_long is not None:
                net.posed_long_rays = prev_long
            if table_dtype is not None and prev_table is not None:
                net.render_table_dtype = prev_table
        yield i, rgb.reshape(resolution, resolution, 3)


def export_mesh(net, path, bound=NSR_BOUND, resolution=512, **kw):
    """the canonical avatar as a binary PLY with per-vertex normals and colours: net.extract_colored_mesh(bound, resolution, **kw) -> geometry.save_ply;
    the reference's counterpart (extract_geometry(NSR_BOUND, 512) + save_mesh, stylize.py:263-269) writes vertices and faces only.  Returns the mesh dict.
    A path ending in .obj writes a TEXTURED mesh instead: net.extract_textured_mesh(bound, resolution, **kw) -> name.obj, name.mtl (geometry.save_obj) and
    name.png (geometry.save_png).  components="largest" (or any spec of geometry.select_components, forwarded like every keyword) drops the field's floaters on
    the device before anything is shaded or baked: export_mesh(net, "avatar.obj", components="largest") writes the body alone.  decimate=k (forwarded as well)
    merges the vertices of every cluster cell of k marching-cubes cells on the device, after the cleaning and before the shading and the atlas layout:
    export_mesh(net, "avatar.obj", components="largest", decimate=4) writes a body of about a sixteenth of the triangles, its texture baked from the field.
    occlusion=True (or occlusion_kit's keywords, or a kit: net.export_occlusion for the length of this call) adds ambient occlusion: the PLY gets a
    `float quality` property per vertex, the OBJ a grey image name_ao.png that its material references as map_Ka.
    weld=True (net.export_weld for the length of this call) welds the mesh on the device after the decimation and before anything is shaded or baked
    (mesh_weld.weld_mesh): repeated triangles, back-to-back pairs of a collapsed thin part and the vertices nobody names any more are not written.  The dict
    then carries weld (what was removed) and topology (mesh_weld.mesh_topology of the written triangles: its closed_manifold says whether the file is one).
    manifold=True (net.export_manifold for the length of this call) makes the mesh manifold on the device after the weld -- after the decimation or the cleaning
    when weld is off -- and before anything is shaded or baked (mesh_repair.repair_mesh): where clustering pushed two sheets of the surface onto one edge or one
    vertex, every sheet gets its own copy of the vertex.  The copies are projected identically, so the file holds COINCIDENT vertices that its faces keep apart;
    no face is added, dropped or turned.  The dict then carries repair (what was split, paired and cut) and topology of the written triangles: what it still
    counts as nonmanifold are pinched edges, which no vertex duplication separates, and its boundary is at most repair["cut"]."""
    import os
    from .geometry import save_obj, save_ply, save_png
    if "occlusion" in kw:
        with _export_occlusion(net, kw.pop("occlusion")):
            return export_mesh(net, path, bound, resolution, **kw)
    if "weld" in kw:
        weld = kw.pop("weld")
        with _export_weld(net, weld):
            mesh = export_mesh(net, path, bound, resolution, **kw)
        return _with_topology(net, mesh) if weld and "topology" not in mesh else mesh
    if "manifold" in kw:
        manifold = kw.pop("manifold")
        with _export_flag(net, "export_manifold", manifold):
            mesh = export_mesh(net, path, bound, resolution, **kw)
        return _with_topology(net, mesh) if manifold else mesh
    if str(path).lower().endswith(".obj"):
        mesh = net.extract_textured_mesh(bound, resolution, **kw)
        png = os.path.splitext(str(path))[0] + ".png"
        save_png(png, mesh["texture"])
        save_obj(str(path), mesh["vertices"], mesh["triangles"], mesh["uv"], normals=mesh["normals"], texture=os.path.basename(png),
                 occlusion_texture=_save_ao(png, mesh))
        return mesh
    mesh = net.extract_colored_mesh(bound, resolution, **kw)
    save_ply(path, mesh["vertices"], mesh["triangles"], normals=mesh["normals"], colors=mesh.get("colors"), quality=mesh.get("occlusion"))
    return mesh


@contextlib.contextmanager
def _export_occlusion(net, occlusion):
    """net.export_occlusion = occlusion inside the block, what it was afterwards"""
    prev = net.export_occlusion
    net.export_occlusion = occlusion
    try:
        yield
    finally:
        net.export_occlusion = prev


@contextlib.contextmanager
def _export_flag(net, name, value):
    """the model's opt-in switch `name` (export_weld, export_manifold) = value inside the block, what it was afterwards"""
    prev = getattr(net, name)
    setattr(net, name, bool(value))
    try:
        yield
    finally:
        setattr(net, name, prev)


def _export_weld(net, weld):
    return _export_flag(net, "export_weld", weld)


def _with_topology(net, mesh):
    """mesh["topology"] = mesh_weld.mesh_topology of the mesh's final triangles (numpy or device) -> mesh"""
    from .mesh_weld import mesh_topology
    t = mesh["triangles"]
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32))
    mesh["topology"] = mesh_topology(t.to(device=net.encoder.embeddings.device, dtype=torch.int32).contiguous(), int(mesh["vertices"].shape[0]))
    return mesh


def _save_ao(png, mesh):
    """the occlusion map of a textured mesh as a grey RGB image next to its texture `png` (stem_ao.png) -> its file name, or None for a mesh without one"""
    import os
    from .geometry import save_png
    if "occlusion_map" not in mesh:
        return None
    ao = os.path.splitext(png)[0] + "_ao.png"
    m = mesh["occlusion_map"]
    m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    save_png(ao, np.repeat(m[:, :, None], 3, axis=2))
    return os.path.basename(ao)


def animation_paths(out_pattern):
    """the files of export_animation for a pattern like "out/frame_%04d.obj": (kind "obj" | "ply", frame path function, shared .mtl path, shared .png path).
    The shared material / texture take the pattern's stem without its frame directive and the separators around it ("out/frame.mtl", "out/frame.png";
    "texture" if nothing is left); a .ply sequence has neither (None)."""
    import os
    import re
    pat = str(out_pattern)
    try:
        differ = pat % 0 != pat % 1
    except (TypeError, ValueError):
        differ = False
    if not differ:
        raise ValueError(f"export_animation: out_pattern {pat!r} needs one integer directive such as %04d")
    ext = os.path.splitext(pat)[1].lower()
    if ext not in (".obj", ".ply"):
        raise ValueError(f"export_animation: out_pattern {pat!r} must end in .obj (textured) or .ply (vertex colours)")
    frame = lambda i: pat % int(i)
    if ext == ".ply":
        return "ply", frame, None, None
    d, base = os.path.split(os.path.splitext(pat)[0])
    stem = re.sub(r"%[0-9]*d", "", base).strip("_-. ") or "texture"
    return "obj", frame, os.path.join(d, stem + ".mtl"), os.path.join(d, stem + ".png")


def export_animation(net, body_model, poses=None, shape_from=None, shape_to=None, out_pattern="frame_%04d.obj", render_type=None, bound=NSR_BOUND,
                     resolution=512, iters=3, tol=1e-5, max_frames=100, device="cuda", rank=None, world=None, **kw):
    """the animated avatar as GEOMETRY: the canonical mesh extracted (and, for .obj, its texture baked) ONCE, bound to the SMPL guide once, then only its
    vertices and normals moved per frame of calc_local_trans (net.pose_mesh: ac_mesh_pose) -- every frame has the same triangles, UVs and texture.
    poses [F,72] (render_type "animate") or shape_from / shape_to [1,10] ("interp_shape"; render_type None picks by which is given).
    out_pattern ending in .obj: frame files (geometry.save_obj) that all reference ONE material and ONE texture image, written before the first frame
    (animation_paths names them); ending in .ply: binary PLYs with vertex normals and colours.  **kw goes to extract_textured_mesh / extract_colored_mesh
    (texture_size, threshold, refine_steps, components, decimate ...: components="largest" keeps the floaters out of every frame, decimate=k poses the
    decimated mesh; occlusion=... adds the CANONICAL pose's ambient occlusion, one shared name_ao.png or a quality property in every frame; weld=True welds
    the mesh before it is shaded, so no orphan vertex is posed, and every frame's dict carries weld and topology as export_mesh's does; manifold=True
    makes it manifold as export_mesh's does: the copies of a split vertex are bound and posed like any vertex and stay coincident in every frame, and every
    frame's dict carries repair and topology); iters / tol to pose_mesh.
    yields (frame index, posed mesh dict of pose_mesh); rank / world: this process writes the frames shard_indices(n_frames, rank, world) like
    render_animation (the shared files are written by every rank with the same content)."""
    import os
    from .geometry import canonical_guide, save_mtl, save_obj, save_ply, save_png
    kind, frame_path, mtl, png = animation_paths(out_pattern)
    if render_type is None:
        render_type = "animate" if poses is not None else "interp_shape"
    world_verts, Ts, n_frames = calc_local_trans(body_model, render_type=render_type, poses=poses, shape_from=shape_from, shape_to=shape_to,
                                                 max_frames=max_frames)
    faces = np.asarray(body_model.faces)[:, :3]
    mine = list(shard_indices(n_frames, rank, world))
    weld, manifold = kw.pop("weld", None), kw.pop("manifold", None)
    with _export_occlusion(net, kw.pop("occlusion")) if "occlusion" in kw else contextlib.nullcontext(), \
            _export_weld(net, weld) if weld is not None else contextlib.nullcontext(), \
            _export_flag(net, "export_manifold", manifold) if manifold is not None else contextlib.nullcontext():
        mesh = net.extract_textured_mesh(bound, resolution, **kw) if kind == "obj" else net.extract_colored_mesh(bound, resolution, **kw)
    if weld or manifold:
        _with_topology(net, mesh)
    if kind == "obj":
        save_png(png, mesh["texture"])
        save_mtl(mtl, os.path.basename(png), _save_ao(png, mesh))             # (the occlusion is the canonical pose's: one image for every frame)
    guide = dict(faces=faces, canonical=canonical_guide(world_verts[0], Ts[0])) if n_frames else None
    # one WarpMesh per frame, the next frame's upload + culling structure prepared beside the current frame's searches (nsr_ops.warp_mesh_sequence)
    if torch.device(device).type == "cuda":
        from . import nsr_ops
        meshes = nsr_ops.warp_mesh_sequence(((world_verts[i], Ts[i]) for i in mine), faces, device)
    else:
        meshes = (None for _ in mine)
    for i, wm in zip(mine, meshes):
        posed = net.pose_mesh(mesh, guide, wm if wm is not None else world_verts[i], Ts[i], iters=iters, tol=tol)
        if kind == "obj":
            save_obj(frame_path(i), posed["vertices"], posed["triangles"], posed["uv"], normals=posed.get("normals"), mtllib=os.path.basename(mtl))
        else:
            save_ply(frame_path(i), posed["vertices"], posed["triangles"], normals=posed.get("normals"), colors=posed.get("colors"),
                     quality=posed.get("occlusion"))
        yield i, posed
