"""Does a change to the Python front end (avatarcraft_amd/nsr_ops, instant_nsr.py, stylize.py) leave every launch's outputs as they were?  For changes that
touch no kernel: the tree before and the tree after load the SAME built library (AC_LIB_PATH), each runs the sequence below in a process of its own, and the
two records must agree byte for byte.

  python tools/frontend_compare.py dump out.npz       one seeded sequence in the tree this file lies in: every output tensor's raw bytes, shape, dtype and
                                                      strides, every result dict's keys in order
  python tools/frontend_compare.py compare a.npz b.npz  -> "COMPARE entries E tensors T differing D"; exit status 1 unless D == 0

Only public names are used, each spelled nsr_ops.<name>, so the file runs unchanged in an older tree: copy it there.  A section that raises is recorded
with the exception's text (and compared like any other entry); dump then ends with status 2.  256 rays (a 16 x 16 view), 2 000 samples for the operators.
The second half (model_sections) drives NeRFNetwork's own methods: render() in eval and with gradients, the step renders, a cuda_ray net, the mesh export
on a 24^3 grid (texture_size 256: the atlas of its ~1 000 triangles), pose_mesh and the first-hit renders.
"""
import os
import sys
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV, BOUND, N_SAMPLES = "cuda:0", 1.6, 2000


class Record:
    def __init__(self):
        self.items, self.errors = {}, 0

    def add(self, name, v):
        """a tensor, None, a number, or a dict / tuple / list of those (result dicts: + their keys in order; keys that start with _ are scratch: listed, not stored)"""
        if isinstance(v, dict):
            self.items[name + "#keys"] = np.array(list(v.keys()), dtype="U")
            for k, x in v.items():
                if not str(k).startswith("_"):
                    self.add(f"{name}.{k}", x)
        elif isinstance(v, (tuple, list)):
            self.items[name + "#len"] = np.array(len(v))
            for i, x in enumerate(v):
                self.add(f"{name}.{i}", x)
        elif isinstance(v, torch.Tensor):
            t = v.detach()
            self.items[name + "#meta"] = np.array([str(t.dtype), str(tuple(t.shape)), str(tuple(t.stride()))], dtype="U")
            self.items[name + "#bytes"] = t.cpu().contiguous().reshape(-1).view(torch.uint8).numpy().copy()
        elif isinstance(v, np.ndarray):
            self.add(name, torch.from_numpy(np.ascontiguousarray(v)))
        elif v is None or isinstance(v, (bool, int, float, str)):
            self.items[name + "#value"] = np.array(repr(v), dtype="U")
        else:                                               # an object (a WarpMesh): its device tensors
            self.items[name + "#type"] = np.array(type(v).__name__, dtype="U")
            self.add(name, {k: x for k, x in getattr(v, "__dict__", {}).items() if isinstance(x, torch.Tensor) and k != "accel"})

    def section(self, name, fn):
        """record fn()'s result under `name` and return it; an exception is recorded instead (-> None)"""
        try:
            v = fn()
            self.add(name, v)
            torch.cuda.synchronize()
            return v
        except Exception as e:
            traceback.print_exc()
            self.errors += 1
            self.items[name + "#error"] = np.array(f"{type(e).__name__}: {e}", dtype="U")


def golden_net(train):
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    from avatarcraft_amd.synthetic import make_table
    p = dict(np.load(os.path.join(ROOT, "tests", "golden", "nsr_params.npz"), allow_pickle=False))
    torch.manual_seed(0)
    net = NeRFNetwork()
    sd = {k: torch.from_numpy(np.asarray(p[k])) for k in p if k.startswith(("sdf_net", "color_net", "deviation_net"))}
    sd["encoder.embeddings"] = torch.from_numpy(make_table(int(p["offsets"][-1]), seed=int(p["table_seed"]), offsets=p["offsets"], level_amp=p["level_amp"]))
    sd["encoder.offsets"] = torch.from_numpy(p["offsets"])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).train(train)


def model(train, **ctor):
    """golden_net's parameters on a NeRFNetwork(**ctor): every entry whose shape the variant keeps (a view-direction colour layer 1 keeps its seeded start)"""
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    gold = golden_net(train).state_dict()
    torch.manual_seed(3)
    net = NeRFNetwork(**ctor)
    mine = net.state_dict()
    net.load_state_dict({k: v for k, v in gold.items() if k in mine and mine[k].shape == v.shape}, strict=False)
    return net.to(DEV).train(train)


def model_sections(rec, ro, rd, bg, up, body):
    """NeRFNetwork's own methods, public names only: render() in eval and with gradients, the step renders and backward_last, a cuda_ray net, the mesh export,
    pose_mesh, the first-hit renders.  256 rays, the synthetic body, a 24^3 grid, a 256^2 atlas."""
    from avatarcraft_amd import nsr_ops
    verts, faces, Ts = body
    N = ro.shape[0]
    ro3, rd3 = ro[None], rd[None]
    grads = lambda net: {k: v.grad for k, v in net.named_parameters()}
    common = dict(bg_color=bg, cos_anneal_ratio=0.5, normal_epsilon_ratio=0.0)

    # ---- render() in eval under no_grad
    net = golden_net(False)
    with torch.no_grad():
        rec.section("m_eval_64_64", lambda: net.render(ro3, rd3, 64, BOUND, 64, **common))
        rec.section("m_eval_lean", lambda: net.render(ro3, rd3, 64, BOUND, 64, per_sample=False, **common))
        rec.section("m_eval_opacity_only", lambda: net.render(ro3, rd3, 64, BOUND, 64, opacity_only=True, **common))
        rec.section("m_eval_long_40_16", lambda: net.render(ro3, rd3, 40, BOUND, 16, **common))
        net.render_table_dtype = "half"
        rec.section("m_eval_half", lambda: net.render(ro3, rd3, 64, BOUND, 64, **common))
        net.render_table_dtype = "float"
        rec.section("m_eval_staged", lambda: net.render(ro3, rd3, 64, BOUND, 64, staged=True, max_ray_batch=100, **dict(common, bg_color=bg[0])))      # (one colour: every batch gets bg_color whole)
        rec.section("m_eval_guided", lambda: net.render(ro3, rd3, 64, BOUND, 64, render_can=True, verts=torch.from_numpy(verts).to(DEV), **common))
        posed = dict(render_can=False, verts=verts, faces=faces, Ts=Ts, **common)
        rec.section("m_posed_32_32", lambda: net.render(ro3, rd3, 32, BOUND, 32, **posed))
        net.skip_masked_samples = True
        rec.section("m_posed_32_32_skip", lambda: net.render(ro3, rd3, 32, BOUND, 32, **posed))
        net.skip_masked_samples = False
        net.posed_long_rays = True
        rec.section("m_posed_long_40_16", lambda: net.render(ro3, rd3, 40, BOUND, 16, **posed))
        net.posed_long_rays = False

    # ---- render() in train mode with gradients: a fixed upstream, every .grad
    def trained(net, num_steps=64, upsample_steps=64, **kw):
        def f():
            net.zero_grad(set_to_none=True)
            torch.manual_seed(21)
            out = net.render(ro3, rd3, num_steps, BOUND, upsample_steps, perturb=True, **dict(common, **kw))
            loss = (out["rgb"].reshape(-1, 3) * up["image"]).sum() + (out["weight_sum"].reshape(-1) * up["wsum"]).sum() + 0.1 * out["gradient_error"]
            if isinstance(out["curvature_error"], torch.Tensor):
                loss = loss + 0.05 * out["curvature_error"]
            loss.backward()
            net.check_finite()
            return out, grads(net)
        return f
    net = golden_net(True)
    for how in ("core", "ops", False):
        net.fused_training = how
        rec.section(f"m_train_{how}", trained(net))
    net.fused_training = "core"
    rec.section("m_train_long_40_16", trained(net, 40, 16))
    rec.section("m_train_posed_32_32", trained(net, 32, 32, render_can=False, verts=verts, faces=faces, Ts=Ts))
    rec.section("m_train_viewdirs", trained(model(True, use_viewdirs=True)))
    rec.section("m_train_curvature", trained(model(True, curvature_loss=True)))
    nsr_ops.free_scratch()

    # ---- the step renders and backward_last
    def step_pair():
        net = golden_net(True)
        torch.manual_seed(31)
        out = net.render_step_pair(ro, rd, 64, 64, BOUND, lambda: torch.rand(N, 3, device=DEV))
        net.backward_last(g_image=up["image"], g_weights_sum=up["wsum"], g_eik=torch.tensor(0.1, device=DEV))
        net.check_finite()
        return out, grads(net)
    rec.section("m_step_pair", step_pair)

    def view_train():
        net = golden_net(True)
        torch.manual_seed(32)
        out = net.render_view_train(ro, rd, 64, 64, BOUND, lambda k, n: torch.rand(n, 3, device=DEV), 100)
        net.backward_last(g_image=up["image"], g_weights_sum=up["wsum"], g_eik=torch.linspace(0.05, 0.2, out[1].shape[0], device=DEV))
        net.check_finite()
        return out, grads(net)
    rec.section("m_view_train", view_train)
    net = golden_net(False)
    for oo in (False, True):
        def view_nograd():
            torch.manual_seed(33)
            with torch.no_grad():
                return net.render_view_nograd(ro, rd, 64, 64, BOUND, lambda n: torch.rand(n, 3, device=DEV), 100, opacity_only=oo)
        rec.section(f"m_view_nograd_opacity{int(oo)}", view_nograd)
    nsr_ops.free_scratch()

    # ---- a cuda_ray net: the density grid, run_cuda in eval (one launch / rounds), in train without and with a graph
    occ = model(False, cuda_ray=True)
    state = lambda: (occ.density_grid, occ.mean_density, occ.mean_count, occ.iter_density, occ.local_step)
    rec.section("m_occ_grid_1", lambda: (occ.update_extra_state(BOUND), state()))
    rec.section("m_occ_grid_2", lambda: (occ.update_extra_state(BOUND), state()))
    with torch.no_grad():
        rec.section("m_occ_eval", lambda: (occ.render(ro3, rd3, 64, BOUND, 64, **common), occ._last_cuda_rounds))
        occ.occupancy_rounds = True
        rec.section("m_occ_eval_rounds", lambda: (occ.render(ro3, rd3, 64, BOUND, 64, **common), occ._last_cuda_rounds > 0))
        occ.occupancy_rounds = False
        occ.train()
        torch.manual_seed(41)
        rec.section("m_occ_train_unbudgeted", lambda: occ.render(ro3, rd3, 64, BOUND, 64, perturb=True, **common))
        rec.section("m_occ_grid_3", lambda: (occ.update_extra_state(BOUND), state()))
        rec.section("m_occ_train_budgeted", lambda: (occ.render(ro3, rd3, 64, BOUND, 64, perturb=True, **common), occ.step_counter))
    for fused in (True, False):
        occ.occupancy_fused_shading = fused
        rec.section(f"m_occ_train_grad_fused{int(fused)}", trained(occ))
    occ.occupancy_fused_shading = True

    # ---- density, the SDF grid, the mesh export in each of its forms
    net = golden_net(False)
    G = 24
    with torch.no_grad():
        x = (torch.rand(500, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
        rec.section("m_density", lambda: net.density(x, BOUND))
    rec.section("m_extract_fields", lambda: net.extract_fields(BOUND, G))
    for name, kw in (("dense", {}), ("slab8", dict(slab_layers=8)), ("largest", dict(components="largest")), ("decimate2", dict(decimate=2)),
                     ("all", dict(slab_layers=8, components="largest", decimate=2)), ("tetra", dict(mesher="tetra"))):
        rec.section(f"m_geometry_{name}", lambda: net.extract_geometry(BOUND, G, **kw))
    rec.section("m_geometry_torch", lambda: net.extract_geometry(BOUND, G, return_torch=True))
    colored = rec.section("m_colored", lambda: net.extract_colored_mesh(BOUND, G))
    rec.section("m_colored_no_colors", lambda: net.extract_colored_mesh(BOUND, G, colors=False, return_torch=True))
    rec.section("m_colored_clean_decimate", lambda: net.extract_colored_mesh(BOUND, G, components="largest", decimate=2, slab_layers=8))
    rec.section("m_textured", lambda: net.extract_textured_mesh(BOUND, G, texture_size=256))
    rec.section("m_textured_clean_decimate", lambda: net.extract_textured_mesh(BOUND, G, texture_size=256, components="largest", decimate=2, return_torch=True))
    if colored is not None:
        rec.section("m_pose_numpy", lambda: net.pose_mesh(colored, dict(faces=faces), verts, Ts))
        on_dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in colored.items()}
        rec.section("m_pose_torch", lambda: net.pose_mesh(on_dev, dict(faces=torch.from_numpy(faces).to(DEV)), torch.from_numpy(verts).to(DEV),
                                                          torch.from_numpy(Ts).to(DEV)))

    # ---- the first-hit renders: whole, in three parts, without colours
    with torch.no_grad():
        for name, kw in (("whole", {}), ("parts", dict(max_ray_batch=100)), ("no_rgb", dict(want_rgb=False)), ("parts_no_rgb", dict(max_ray_batch=100, want_rgb=False))):
            rec.section(f"m_surface_{name}", lambda: net.render_surface(ro3, rd3, BOUND, bg_color=bg, **kw))
            rec.section(f"m_surface_posed_{name}", lambda: net.render_surface_posed(ro3, rd3, BOUND, verts, faces, Ts, bg_color=bg, **kw))


def dump(path):
    from avatarcraft_amd import geometry, nsr_ops
    from avatarcraft_amd.synthetic import device_field, load_field_params, make_body, make_rays
    rec = Record()
    t = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)
    p = load_field_params()
    f, _ = device_field(p)
    f.prepare()
    inv_s = float(p["inv_s"])
    ro, rd = (t(a) for a in make_rays(16, 16, dist=1.7, f=12.5))
    N = ro.shape[0]
    torch.manual_seed(1234)
    noise = {ns: torch.rand(N, ns, device=DEV) for ns in (32, 40, 64)}
    noise2 = {ns: torch.rand(2, N, ns, device=DEV) for ns in (32, 40, 64)}
    bg, bg2 = torch.rand(N, 3, device=DEV), torch.rand(2, N, 3, device=DEV)
    x = (torch.rand(N_SAMPLES, 3, device=DEV) * 2 - 1) * 0.9
    dirs = torch.nn.functional.normalize(torch.randn(N_SAMPLES, 3, device=DEV), dim=1)
    up = {k: torch.randn(*s, device=DEV) for k, s in dict(image=(N, 3), wsum=(N,), depth=(N,), nmap=(N, 3), out16=(N_SAMPLES, 16), grad=(N_SAMPLES, 3),
                                                          rgb=(N_SAMPLES, 3)).items()}
    kw = dict(bound=BOUND, inv_s=inv_s)

    # ---- the fused renderer and its pair / sample forms
    rec.section("render_64_64", lambda: nsr_ops.render_rays(f, ro, rd, 64, 64, bg=bg, noise=noise[64], extras=True, train_extras=True, **kw))
    rec.section("render_32_32_idx", lambda: nsr_ops.render_rays(f, ro, rd, 32, 32, debug_indices=True, **kw))
    rec.section("render_half", lambda: nsr_ops.render_rays(f, ro, rd, 64, 64, bg=bg, extras=True, table_dtype="half", **kw))
    rec.section("render_fast", lambda: nsr_ops.render_rays(f, ro, rd, 64, 64, precision="fast", **kw))
    rec.section("long_40_16", lambda: nsr_ops.render_rays_long(f, ro, rd, 40, 16, noise=noise[40], extras=True, train_extras=True, **kw))
    rec.section("long_32_32_stencil", lambda: nsr_ops.render_rays_long(f, ro, rd, 32, 32, noise=noise[32], extras=True, train_extras=True, save_stencil=True, **kw))
    for keep in (False, True):
        rec.section(f"pair_keep{int(keep)}", lambda: nsr_ops.render_rays_pair(f, ro, rd, noise2[64], 64, 64, bg2=bg2, keep_weights=keep, **kw))
    rec.section("long_pair_40_16", lambda: nsr_ops.render_rays_long_pair(f, ro, rd, noise2[40], 40, 16, bg2=bg2, **kw))
    rec.section("long_pair_32_32", lambda: nsr_ops.render_rays_long_pair(f, ro, rd, noise2[32], 32, 32, bg2=bg2, keep_weights=True, save_stencil=True, **kw))
    rec.section("sample", lambda: nsr_ops.sample_rays(f, ro, rd, 64, 64, BOUND, noise=noise[64]))
    rec.section("sample_long", lambda: nsr_ops.sample_rays_long(f, ro, rd, 40, 16, BOUND, noise=noise[40]))
    rec.section("handoff_timeouts", lambda: nsr_ops.handoff_timeouts(DEV))

    # ---- posed space and the surface renderers on the synthetic body
    verts, faces, Ts = make_body(n_lat=10, n_lon=12)
    wm = rec.section("warp_mesh", lambda: nsr_ops.WarpMesh(verts, faces, Ts, DEV))
    rec.section("render_warped", lambda: nsr_ops.render_rays(f, ro, rd, 32, 32, warp=wm, skip_masked=True, extras=True, **kw))
    rec.section("long_warped", lambda: nsr_ops.render_rays_long(f, ro, rd, 40, 16, warp=wm, extras=True, **kw))
    rec.section("surface", lambda: nsr_ops.render_rays_surface(f, ro, rd, BOUND, nsr_ops.FD_STEP, bg=bg))
    rec.section("surface_no_rgb", lambda: nsr_ops.render_rays_surface(f, ro, rd, BOUND, nsr_ops.FD_STEP, want_rgb=False))
    rec.section("surface_warped", lambda: nsr_ops.render_rays_surface_warped(f, ro, rd, BOUND, wm, bg=bg))

    # ---- the field alone and the training operators, forward and backward
    P = {k: t(p[k]).requires_grad_() for k in ("W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3")}
    table = f.t["table"].clone().requires_grad_()
    offsets, pls = [int(v) for v in p["offsets"]], float(p["per_level_scale"])
    sdf16 = rec.section("field_sdf", lambda: nsr_ops.field_sdf(f, x, BOUND))
    rec.section("field_color", lambda: nsr_ops.field_color(f, x, dirs, sdf16))
    rec.section("field_samples", lambda: nsr_ops.field_samples(f, x, dirs, torch.full((N_SAMPLES,), 0.01, device=DEV), BOUND, nsr_ops.FD_STEP, inv_s,
                                                               want_sdf=True, want_gradient=True))

    def stencil(x_grad):
        xs = x.clone().requires_grad_(x_grad)
        out = nsr_ops.sdf_stencil(xs, table, P["W1"], P["b1"], P["W2"], P["b2"], offsets, pls, 16, BOUND, nsr_ops.FD_STEP)
        ins = ([xs] if x_grad else []) + [table, P["W1"], P["b1"], P["W2"], P["b2"]]
        return out, torch.autograd.grad(out, ins, (up["out16"], up["grad"]))
    rec.section("sdf_stencil", lambda: stencil(False))
    rec.section("sdf_stencil_dx", lambda: stencil(True))

    def color():
        n, s = dirs.clone().requires_grad_(), sdf16.clone().requires_grad_()
        rgb = nsr_ops.color_mlp(x, n, s, P["Wc1"], P["Wc2"], P["Wc3"])
        return rgb, torch.autograd.grad(rgb, [n, s, P["Wc1"], P["Wc2"], P["Wc3"]], up["rgb"])
    rec.section("color_mlp", color)

    def core():
        s = torch.tensor([[inv_s]], device=DEV, requires_grad=True)
        out = nsr_ops.render_core(table, *(P[k] for k in ("W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3")), s, ro, rd, bg, noise[64], offsets, pls, 16, 64, 64, BOUND)
        loss = (out[0] * up["image"]).sum() + (out[1] * up["wsum"]).sum() + (out[2] * up["depth"]).sum() + (out[3] * up["nmap"]).sum() + 0.1 * out[4]
        return out, torch.autograd.grad(loss, [table, s] + list(P.values()))
    rec.section("render_core", core)

    def core_backward():
        out = nsr_ops.render_rays(f, ro, rd, 64, 64, bg=bg, noise=noise[64], extras=True, train_extras=True, **kw)
        g_table = torch.zeros_like(f.t["table"])
        g = nsr_ops.render_core_backward(f, out.opts, out, ro, rd, bg, up["image"], up["wsum"], up["depth"], up["nmap"], torch.tensor(0.1, device=DEV), g_table)
        return g, g_table, nsr_ops.split_sdf_param_grads(g[0]), nsr_ops.split_color_param_grads(g[1])
    rec.section("render_core_backward", core_backward)
    nsr_ops.free_scratch()

    # ---- the occupancy grid: its update, the two renderers
    H = 32
    axis = torch.linspace(-BOUND, BOUND, H, device=DEV)
    grid = torch.zeros(H, H, H, device=DEV)
    rec.section("density_grid_update", lambda: [nsr_ops.density_grid_update(f, axis, grid, BOUND) for _ in range(2)])
    rec.add("density_grid", grid)
    mean = float(grid.mean())
    occ = (f, ro, rd, grid, mean, BOUND, nsr_ops.FD_STEP, inv_s)
    for phased in (False, True):
        rec.section(f"occupancy_phased{int(phased)}", lambda: nsr_ops.render_rays_occupancy(*occ, count_samples=True, phased=phased))
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    rec.section("occupancy_train", lambda: nsr_ops.render_rays_occupancy_train(*occ, capacity=N * 64, counter=counter, bg=1.0))
    rec.add("occupancy_counter", counter)
    rec.section("occupancy_failures", lambda: (nsr_ops.occupancy_launch_failures(), nsr_ops.occupancy_fallbacks()))

    # ---- the mesh export: whole against streamed, attributes, bake, bind, pose, components, compact
    G = 24
    ax = torch.linspace(-BOUND, BOUND, G, device=DEV)
    mc_kw = dict(den=G - 1.0, span=(2 * BOUND,) * 3, lo=(-BOUND,) * 3)
    vol = rec.section("sdf_grid", lambda: nsr_ops.field_sdf_grid(f, ax, ax, ax, BOUND))
    mesh = rec.section("marching_cubes", lambda: nsr_ops.marching_cubes(vol, **mc_kw))
    for layers in (2, 3, 8):
        rec.section(f"marching_cubes_streamed_{layers}",
                    lambda: nsr_ops.marching_cubes_streamed(lambda x0, out: nsr_ops.field_sdf_grid(f, ax[x0:x0 + out.shape[0]], ax, ax, BOUND, out=out), G, G, G,
                                                            slab_layers=layers, device=DEV, **mc_kw))
    attrs = rec.section("mesh_vertex_attrs", lambda: nsr_ops.mesh_vertex_attrs(f, mesh[0], BOUND))
    rec.section("mesh_bake_texture", lambda: nsr_ops.mesh_bake_texture(f, attrs["positions"], mesh[1][:128].contiguous(), 64, None, BOUND, want_normals=True))
    bind = rec.section("mesh_bind", lambda: nsr_ops.mesh_bind(attrs["positions"], t(geometry.canonical_guide(verts, Ts)), wm.faces))
    rec.section("mesh_pose", lambda: nsr_ops.mesh_pose(attrs["positions"], attrs["normals"], bind, wm))
    c = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    two = torch.minimum((c - c.new_tensor([0.7, 0.0, 0.0])).norm(dim=-1) - 0.4, (c + c.new_tensor([0.7, 0.1, 0.0])).norm(dim=-1) - 0.5).contiguous()
    m2 = rec.section("marching_cubes_two", lambda: nsr_ops.marching_cubes(two, **mc_kw))
    comps = rec.section("mesh_components", lambda: nsr_ops.mesh_components(m2[1], m2[0].shape[0]))
    rec.section("mesh_compact", lambda: nsr_ops.mesh_compact(m2[1], comps["component"], torch.arange(comps["n_components"], device=DEV) == 0))

    # ---- a model: the sampling stage on its SDF-only field, two stylisation steps
    def steps():
        from avatarcraft_amd.stylize import SyntheticGuidance, flat_grad_view, sds_step
        net, net_gt = golden_net(True), golden_net(False)
        z = nsr_ops.sample_rays(net._field_sdf_only(), ro, rd, 64, 64, BOUND)
        opt = torch.optim.Adam(net.parameters(), lr=5e-3)
        flat = flat_grad_view(net.parameters())
        guide_fn = SyntheticGuidance(5)
        torch.manual_seed(11)
        stats = [sds_step(net, net_gt, ro, rd, (16, 16), opt, guide_fn, batch_size=4096, flat_grad=flat) for _ in range(2)]
        torch.cuda.synchronize()
        return (z, {k: v for k, v in net.named_parameters()}, {k: v.grad for k, v in net.named_parameters()}, flat,
                [{k: v for k, v in s.items() if isinstance(v, (int, float, torch.Tensor))} for s in stats])
    rec.section("sds_steps", steps)
    nsr_ops.free_scratch()
    model_sections(rec, ro, rd, bg, up, (verts, faces, Ts))

    np.savez_compressed(path, **rec.items)
    print(f"DUMP entries {len(rec.items)} tensors {sum(k.endswith('#bytes') for k in rec.items)} errors {rec.errors}", flush=True)
    return 2 if rec.errors else 0


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    names = sorted(set(a.files) | set(b.files))
    bad = [n for n in names if n not in a.files or n not in b.files or a[n].shape != b[n].shape or not np.array_equal(a[n], b[n])]
    for n in bad:
        print("differs:", n, *(str(z[n])[:200] if n in z.files and not n.endswith("#bytes") else "" for z in (a, b)))
    errors = [n for n in names if n.endswith("#error")]
    for n in errors:
        print("a section raised:", n)
    print(f"COMPARE entries {len(names)} tensors {sum(n.endswith('#bytes') for n in names)} differing {len(bad)}" + (f" sections that raised {len(errors)}" if errors else ""))
    return 1 if bad or errors else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
