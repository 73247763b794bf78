"""CPU: the instant_nsr package keeps what instant_nsr.py offered -- names, signatures, switches, every refusal's type, text and order -- its submodules
import only upwards, the one list of caches is complete, and the shared helpers choose what the written-out copies chose.  Needs neither the library nor a
GPU.  Everything but test_every_cache_is_dropped_and_unpickled and test_shared_helpers passes unedited in the tree where instant_nsr was one module."""
import ast
import copy
import importlib
import inspect
import os
import pickle
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# written from the one-module instant_nsr.py: {name: str(inspect.signature)} of the public methods of NeRFNetwork and of the private ones used outside the file
SIGNATURES = {
    '_field': '(self)',
    '_field_sdf_only': '(self)',
    '_fused_supported': '(self, ignore_curvature=False)',
    '_grid_axis': '(self, bound, resolution)',
    '_guard_finite': '(self, gerr)',
    '_long_save_stencil': '(self, num_steps, upsample_steps)',
    '_offsets_host': '(self)',
    '_poll_finite': '(self, wait)',
    '_render_core_autograd': '(self, rays_o, rays_d, z_vals, num_steps0, upsample_steps, bound, bg_color, cos_anneal_ratio, normal_epsilon_ratio, B, N, near_far=None)',
    'backward_last': '(self, g_image=None, g_weights_sum=None, g_eik=None, split=None)',
    'check_finite': '(self)',
    'density': '(self, x, bound)',
    'extract_colored_mesh': '(self, bound: float, resolution: int, threshold: float = 0.0, refine_steps: int = 3, tol: float = 1e-05, colors: bool = True, return_torch=False, slab_layers=None, components=None, decimate=None)',
    'extract_fields': '(self, bound: float, resolution: int)',
    'extract_fields_device': '(self, bound: float, resolution: int, negate: bool = False, slab_layers=None)',
    'extract_geometry': '(self, bound: float, resolution: int, threshold: int = 0.0, device=None, mesher=None, return_torch=False, slab_layers=None, components=None, decimate=None)',
    'extract_textured_mesh': '(self, bound: float, resolution: int, texture_size: int = 2048, cell=None, threshold: float = 0.0, refine_steps: int = 3, tol: float = 1e-05, return_torch=False, slab_layers=None, components=None, decimate=None)',
    'finite_difference_normals_approximator': '(self, x, bound, epsilon=0.0005)',
    'forward_color': '(self, x, d, n, geo_feat, bound)',
    'forward_color_fused': '(self, x, n, sdf_out)',
    'forward_sdf': '(self, x, bound)',
    'forward_sdf_stencil': '(self, x, bound, epsilon)',
    'forward_variance': '(self)',
    'gradient': '(self, x, bound, epsilon=0.0005)',
    'invalidate_caches': '(self)',
    'manual_backward_supported': '(self, num_steps=None, upsample_steps=None)',
    'pose_mesh': '(self, mesh, body_guide, verts, Ts=None, iters: int = 3, tol: float = 1e-05)',
    'render': '(self, rays_o, rays_d, num_steps, bound, upsample_steps, staged=False, max_ray_batch=4096, bg_color=None, cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0, render_can=True, verts=None, faces=None, Ts=None, perturb: bool = False, use_mesh_guide: bool = True, per_sample: bool = True, opacity_only: bool = False, **kwargs)',
    'render_step_pair': '(self, rays_o, rays_d, num_steps, upsample_steps, bound, bkg_fn, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0)',
    'render_surface': '(self, rays_o, rays_d, bound, bg_color=None, normal_epsilon_ratio=0.0, max_ray_batch=None, **opts)',
    'render_surface_posed': '(self, rays_o, rays_d, bound, verts, faces, Ts, bg_color=None, max_ray_batch=None, normal_epsilon_ratio=0.0, **opts)',
    'render_view_nograd': '(self, rays_o, rays_d, num_steps, upsample_steps, bound, bkg_fn, batch_size, opacity_only=False, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0)',
    'render_view_train': '(self, rays_o, rays_d, num_steps, upsample_steps, bound, draw_fn, batch_size, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0)',
    'run': '(self, rays_o, rays_d, num_steps, bound, upsample_steps, bg_color, cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0, render_can=True, verts=None, faces=None, Ts=None, perturb_overwrite: bool = False, use_mesh_guide: bool = True, per_sample: bool = True, opacity_only: bool = False)',
    'run_cuda': '(self, rays_o, rays_d, num_steps, bound, upsample_steps, bg_color, cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0, render_can=True, verts=None, faces=None, Ts=None, perturb_overwrite: bool = False, use_mesh_guide: bool = True, per_sample: bool = True, max_steps=1024)',
    'update_extra_state': '(self, bound, decay=0.95)',
}
SWITCHES = {
    '_manual_backward': False,
    'fused_density_grid': True,
    'fused_training': 'core',
    'long_step_extras': False,
    'nan_guard': True,
    'occupancy_fused_shading': True,
    'occupancy_rounds': False,
    'occupancy_train_one_launch': True,
    'posed_long_rays': False,
    'render_precision': 'exact',
    'render_table_dtype': 'float',
    'skip_masked_samples': False,
    'supports_lean_render': True,
    'supports_opacity_only': True,
    'warp_temporal_seeds': True,
}
# of those, what NeRFRenderer has by itself: everything it had but run_cuda and the three occupancy_* switches, which are the occupancy mixin's now
ON_RENDERER = ['_field', '_field_sdf_only', '_fused_supported', '_guard_finite', '_long_save_stencil', '_manual_backward', '_offsets_host', '_poll_finite',
               '_render_core_autograd', 'backward_last', 'check_finite', 'fused_training', 'invalidate_caches', 'long_step_extras', 'manual_backward_supported',
               'nan_guard', 'posed_long_rays', 'render', 'render_precision', 'render_step_pair', 'render_table_dtype', 'render_view_nograd', 'render_view_train',
               'run', 'skip_masked_samples', 'supports_lean_render', 'supports_opacity_only', 'warp_temporal_seeds']
ORDER = ["route", "guard", "renderer", "occupancy", "export", "surface", "network"]


def test_public_surface():
    from avatarcraft_amd import instant_nsr as M
    from avatarcraft_amd import nsr_ops
    for name in ("NeRFNetwork", "NeRFRenderer", "SingleVarianceNetwork", "near_far_from_bound", "render_route", "Route", "DEFAULT_GEO_THRESH", "nsr_ops"):
        assert hasattr(M, name), name
    assert M.nsr_ops is nsr_ops and M.DEFAULT_GEO_THRESH == 0.05 and M.Route._fields == ("entry", "options", "then")
    assert issubclass(M.NeRFNetwork, M.NeRFRenderer)
    static = lambda cls, k: inspect.getattr_static(cls, k)
    assert {k: str(inspect.signature(static(M.NeRFNetwork, k))) for k in SIGNATURES} == SIGNATURES
    assert {k: static(M.NeRFNetwork, k) for k in SWITCHES} == SWITCHES
    for k in ON_RENDERER:
        assert static(M.NeRFRenderer, k) is static(M.NeRFNetwork, k), k
    # the guard's methods are plain functions that a foreign class can borrow, and the private attributes other files name are still where they look
    for k in ("_guard_finite", "_poll_finite", "check_finite"):
        assert isinstance(static(M.NeRFRenderer, k), types.FunctionType), k
    assert "_nan_pending" in M.NeRFRenderer._UNPICKLED_ATTRS and "_nan_pending" not in M.NeRFRenderer._CACHE_ATTRS


def test_submodules_import_upwards_only():
    """each submodule's `from .x import` names only modules above it in ORDER (one module: nothing to order), and __init__ holds imports only"""
    from avatarcraft_amd import instant_nsr as M
    if not hasattr(M, "__path__"):
        return
    files = sorted(f[:-3] for f in os.listdir(M.__path__[0]) if f.endswith(".py") and f != "__init__.py")
    assert files == sorted(ORDER)
    for i, name in enumerate(ORDER):
        tree = ast.parse(open(os.path.join(M.__path__[0], name + ".py")).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 1:
                assert node.module in ORDER[:i], (name, node.module)
                if node.module is None:                                   # `from . import x`
                    assert all(a.name in ORDER[:i] for a in node.names), (name, [a.name for a in node.names])
            if isinstance(node, ast.ImportFrom) and node.level == 2:     # launches are spelled nsr_ops.<name>: nobody binds an entry of it
                assert node.module != "nsr_ops", (name, [a.name for a in node.names])
    assert not [n.id for n in ast.walk(ast.parse(open(M.__file__).read())) if isinstance(n, ast.Name)]
    for name in ("occupancy", "export", "surface"):                      # the mixins: plain classes, no __init__, no state of their own
        for cls in (v for v in vars(importlib.import_module(f"{M.__name__}.{name}")).values() if inspect.isclass(v) and v.__module__.endswith(name)):
            assert "__init__" not in vars(cls) and (cls.__bases__ == (object,) or issubclass(cls, tuple)), cls


def _net(**kw):
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    torch.manual_seed(0)
    return NeRFNetwork(**kw)


def test_every_cache_is_dropped_and_unpickled():
    """FAILS in the one-module tree, the one test of this file that does: there _inv_s_cache, _last_train_groups and _warp_seed_rows were missing from
    _CACHE_ATTRS, survived invalidate_caches() and went into every pickle and deep copy."""
    net = _net()
    names = type(net)._CACHE_ATTRS
    assert {"_inv_s_cache", "_last_train_groups", "_warp_seed_rows"} <= set(names)
    with torch.no_grad():
        net.forward_variance()                                            # a real one among the dummies
    assert "_inv_s_cache" in net.__dict__
    plant = lambda n: [n.__dict__.__setitem__(k, ("dummy", k)) for k in names if k != "_inv_s_cache"]
    plant(net)
    net.invalidate_caches()
    assert not [k for k in names if k in net.__dict__]
    plant(net)
    net.__dict__["_nan_pending"] = []
    net.__dict__["_inv_s_cache"] = ("dummy", None)
    state = net.__getstate__()
    assert not [k for k in names + ("_nan_pending",) if k in state]
    twin = copy.deepcopy(net)
    assert not [k for k in names + ("_nan_pending",) if k in twin.__dict__]
    assert all(k in net.__dict__ for k in names)                           # (copying took nothing from the original)
    net.invalidate_caches()
    bare = len(pickle.dumps(net))
    net.__dict__["_warp_seed_rows"] = {(256, 64): torch.arange(1000, dtype=torch.int32)}
    assert len(pickle.dumps(net)) <= bare
    with torch.no_grad():                                                  # the copy rebuilds what it needs: the same variance
        assert torch.equal(twin.forward_variance(), net.forward_variance())


class _Launched(Exception):
    pass


class _CudaNamedCpu(str):
    """a device torch takes for the CPU (tensors made "on" it are host tensors) that calls itself cuda"""
    type = "cuda"


def _gpu_like(net):
    """the model answers `is_cuda` like one on the GPU, so that a call gets past "on the GPU" to its later refusals; whatever would prepare a field raises
    _Launched instead (no refusal fired).  The encoder's facts stay the real encoder's."""
    enc = net.encoder
    fake = types.SimpleNamespace(embeddings=types.SimpleNamespace(is_cuda=True, device=_CudaNamedCpu("cpu")), num_levels=enc.num_levels,
                                 level_dim=enc.level_dim, input_dim=enc.input_dim)
    del net.encoder
    net.__dict__["encoder"] = fake

    def launched(*a, **kw):
        raise _Launched()
    net.__dict__["_field"] = net.__dict__["_field_sdf_only"] = launched
    return net


_SDF = "the default SDF side of NeRFNetwork on the GPU"
_COLOUR = "the colour side of this model is not the default one (colour net 21-64-64-3, or 37-64-64-3 with the degree-4 view-direction encoder)"
_NATIVE = "it needs mesher='native' and " + _SDF
R, N, V = RuntimeError, NotImplementedError, ValueError
_rays = lambda: (torch.zeros(1, 4, 3), torch.ones(1, 4, 3))


def _zero_volume(net):
    """(the hash encoder has no CPU path: the host volume of the non-native meshers is given, so that the call gets as far as naming its mesher)"""
    net.extract_fields = lambda bound, resolution: torch.zeros([resolution] * 3).numpy()
    return net


def _warp():
    from avatarcraft_amd import nsr_ops
    return object.__new__(nsr_ops.WarpMesh)                                 # (a WarpMesh by type only: nothing is built)


_mesh = lambda: dict(vertices=torch.zeros(3, 3, dtype=torch.float64))
# (label, constructor arguments, answers like a GPU model, grad mode, call, exception type, full message)
REFUSALS = [
    # ---- extract_fields_device
    ("fields_device slab", {}, False, False, lambda n: n.extract_fields_device(1.0, 8, slab_layers=4), R,
     "extract_fields_device: slab_layers is refused here -- a streamed volume is never whole; extract_geometry(slab_layers=...) meshes it slab by slab"),
    ("fields_device cpu", {}, False, False, lambda n: n.extract_fields_device(1.0, 8), R, "extract_fields_device: needs " + _SDF),
    ("fields_device sdf side", dict(hidden_dim=32), True, False, lambda n: n.extract_fields_device(1.0, 8), R, "extract_fields_device: needs " + _SDF),
    ("fields_device passes", {}, True, False, lambda n: n.extract_fields_device(1.0, 8), _Launched, ""),
    # ---- extract_geometry: decimate (mesher check before cluster_grid), then components, then slab_layers, then mesher='native'
    ("geometry decimate cpu", {}, False, False, lambda n: n.extract_geometry(1.0, 8, decimate=2), R,
     "extract_geometry(decimate=...) decimates the native mesher's mesh on the device: " + _NATIVE),
    ("geometry decimate nan cpu", {}, False, False, lambda n: n.extract_geometry(1.0, 8, decimate=float("nan")), R,
     "extract_geometry(decimate=...) decimates the native mesher's mesh on the device: " + _NATIVE),
    ("geometry decimate tetra", {}, True, False, lambda n: n.extract_geometry(1.0, 8, decimate=float("nan"), mesher="tetra"), R,
     "extract_geometry(decimate=...) decimates the native mesher's mesh on the device: " + _NATIVE),
    ("geometry decimate nan", {}, True, False, lambda n: n.extract_geometry(1.0, 8, decimate=float("nan"), components="largest", slab_layers=1), V,
     "cluster_grid: k nan must be a finite real >= 1 (the cluster cell edge in marching-cubes cells)"),
    ("geometry decimate first", {}, False, False, lambda n: n.extract_geometry(1.0, 8, decimate=2, components="largest", slab_layers=1), R,
     "extract_geometry(decimate=...) decimates the native mesher's mesh on the device: " + _NATIVE),
    ("geometry components cpu", {}, False, False, lambda n: n.extract_geometry(1.0, 8, components="largest"), R,
     "extract_geometry(components=...) cleans the native mesher's mesh on the device: " + _NATIVE),
    ("geometry components mcubes", {}, True, False, lambda n: n.extract_geometry(1.0, 8, components="largest", mesher="mcubes", slab_layers=1), R,
     "extract_geometry(components=...) cleans the native mesher's mesh on the device: " + _NATIVE),
    ("geometry components then slab", {}, True, False, lambda n: n.extract_geometry(1.0, 8, decimate=2, components="largest", slab_layers=1), R,
     "extract_geometry: slab_layers 1 must be an integer >= 2"),
    ("geometry slab value cpu", {}, False, False, lambda n: n.extract_geometry(1.0, 8, slab_layers=1), R, "extract_geometry: slab_layers 1 must be an integer >= 2"),
    ("geometry slab cpu", {}, False, False, lambda n: n.extract_geometry(1.0, 8, slab_layers=8), R,
     "extract_geometry(slab_layers=...) streams the native mesher: " + _NATIVE),
    ("geometry slab tetra", {}, True, False, lambda n: n.extract_geometry(1.0, 8, slab_layers=8, mesher="tetra"), R,
     "extract_geometry(slab_layers=...) streams the native mesher: " + _NATIVE),
    ("geometry native cpu", {}, False, False, lambda n: n.extract_geometry(1.0, 8, mesher="native"), R, "extract_geometry(mesher='native') needs " + _SDF),
    ("geometry native sdf side", dict(num_layers=3), True, False, lambda n: n.extract_geometry(1.0, 8, mesher="native"), R,
     "extract_geometry(mesher='native') needs " + _SDF),
    ("geometry bad mesher", {}, False, False, lambda n: _zero_volume(n).extract_geometry(1.0, 4, mesher="cubes"), V, "extract_geometry: unknown mesher 'cubes'"),
    ("geometry bad mesher last", {}, False, False, lambda n: _zero_volume(n).extract_geometry(1.0, 4, mesher="cubes", slab_layers=2), R,
     "extract_geometry(slab_layers=...) streams the native mesher: " + _NATIVE),
    ("geometry passes", {}, True, False, lambda n: n.extract_geometry(1.0, 8, decimate=2, components="largest", slab_layers=2), _Launched, ""),
    # ---- extract_colored_mesh / extract_textured_mesh: slab_layers, then cluster_grid, then "on the GPU", then the colour side
    ("colored slab first", {}, False, False, lambda n: n.extract_colored_mesh(1.0, 8, slab_layers=1, decimate=float("nan")), R,
     "extract_colored_mesh: slab_layers 1 must be an integer >= 2"),
    ("colored decimate nan cpu", {}, False, False, lambda n: n.extract_colored_mesh(1.0, 8, decimate=float("nan")), V,
     "cluster_grid: k nan must be a finite real >= 1 (the cluster cell edge in marching-cubes cells)"),
    ("colored cpu", {}, False, False, lambda n: n.extract_colored_mesh(1.0, 8, components="largest", decimate=2, slab_layers=2), R, "extract_colored_mesh needs " + _SDF),
    ("colored cpu no colours", dict(hidden_dim_color=32), False, False, lambda n: n.extract_colored_mesh(1.0, 8, colors=False), R, "extract_colored_mesh needs " + _SDF),
    ("colored gpu before colour", dict(hidden_dim_color=32), False, False, lambda n: n.extract_colored_mesh(1.0, 8), R, "extract_colored_mesh needs " + _SDF),
    ("colored colour side", dict(hidden_dim_color=32), True, False, lambda n: n.extract_colored_mesh(1.0, 8), R,
     "extract_colored_mesh(colors=True): " + _COLOUR + "; colors=False exports positions and normals"),
    ("colored colour side 4 layers", dict(num_layers_color=4), True, False, lambda n: n.extract_colored_mesh(1.0, 8, colors=True), R,
     "extract_colored_mesh(colors=True): " + _COLOUR + "; colors=False exports positions and normals"),
    ("colored no colours passes", dict(hidden_dim_color=32), True, False, lambda n: n.extract_colored_mesh(1.0, 8, colors=False), _Launched, ""),
    ("colored curvature passes", dict(curvature_loss=True), True, False, lambda n: n.extract_colored_mesh(1.0, 8), _Launched, ""),
    ("textured slab", {}, False, False, lambda n: n.extract_textured_mesh(1.0, 8, slab_layers=True), R, "extract_colored_mesh: slab_layers True must be an integer >= 2"),
    ("textured decimate", {}, False, False, lambda n: n.extract_textured_mesh(1.0, 8, decimate=0.5), V,
     "cluster_grid: k 0.5 must be a finite real >= 1 (the cluster cell edge in marching-cubes cells)"),
    ("textured cpu", {}, False, False, lambda n: n.extract_textured_mesh(1.0, 8, components="largest"), R, "extract_colored_mesh needs " + _SDF),
    ("textured colour side", dict(hidden_dim_color=32), True, False, lambda n: n.extract_textured_mesh(1.0, 8), R,
     "extract_colored_mesh(colors=True): " + _COLOUR + "; colors=False exports positions and normals"),
    # ---- render_surface / render_surface_posed: "on the GPU", the colour side, grad mode, the options
    ("surface cpu", {}, False, True, lambda n: n.render_surface(*_rays(), 1.0, max_iters=0), R, "render_surface needs " + _SDF),
    ("surface cpu no rgb", {}, False, False, lambda n: n.render_surface(*_rays(), 1.0, want_rgb=False), R, "render_surface needs " + _SDF),
    ("surface colour side", dict(hidden_dim_color=32), True, True, lambda n: n.render_surface(*_rays(), 1.0, max_iters=0), R,
     "render_surface: " + _COLOUR + "; want_rgb=False renders geometry only"),
    ("surface grad", {}, True, True, lambda n: n.render_surface(*_rays(), 1.0, max_iters=0), R,
     "render_surface builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()"),
    ("surface grad no rgb", dict(hidden_dim_color=32), True, True, lambda n: n.render_surface(*_rays(), 1.0, want_rgb=False), R,
     "render_surface builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()"),
    ("surface options", {}, True, False, lambda n: n.render_surface(*_rays(), 1.0, max_iters=0), R, "render_rays_surface: max_iters 0 outside 1..255"),
    ("surface options no rgb", dict(hidden_dim_color=32), True, False, lambda n: n.render_surface(*_rays(), 1.0, want_rgb=False, guard=0.5), R,
     "render_rays_surface: guard 0.5 outside [0, 0.5)"),
    ("surface fd step", {}, True, False, lambda n: n.render_surface(*_rays(), 1.0, normal_epsilon_ratio=1.0), R, "render_rays_surface: fd_eps 0.0 not > 0"),
    ("surface passes", {}, True, False, lambda n: n.render_surface(*_rays(), 1.0), _Launched, ""),
    ("posed cpu", {}, False, True, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, w_tol=-1), R, "render_surface_posed needs " + _SDF),
    ("posed cpu no rgb", {}, False, False, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, want_rgb=False), R, "render_surface_posed needs " + _SDF),
    ("posed colour side", dict(hidden_dim_color=32), True, True, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, w_tol=-1), R,
     "render_surface_posed: " + _COLOUR + "; want_rgb=False renders geometry only"),
    ("posed grad", {}, True, True, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, w_tol=-1), R,
     "render_surface_posed builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()"),
    ("posed grad no rgb", dict(hidden_dim_color=32), True, True, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, want_rgb=False), R,
     "render_surface_posed builds no autograd graph (the hit point is the result of a root finder): call it under torch.no_grad()"),
    ("posed options", {}, True, False, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, w_tol=-1), R, "render_rays_surface_warped: w_tol -1.0 not >= 0"),
    ("posed options of both", {}, True, False, lambda n: n.render_surface_posed(*_rays(), 1.0, None, None, None, w_tol=-1, tol=-1.0), R,
     "render_rays_surface_warped: tol -1.0 not >= 0"),
    ("surface option of the posed form", {}, True, False, lambda n: n.render_surface(*_rays(), 1.0, w_tol=0.0), TypeError, None),
    # ---- pose_mesh
    ("pose cpu", {}, False, False, lambda n: n.pose_mesh(_mesh(), dict(faces=None), None), R, "pose_mesh needs the model on the GPU (there is no CPU path)"),
    ("pose warp mesh without canonical", {}, True, False, lambda n: n.pose_mesh(_mesh(), dict(faces=None), _warp()), R,
     "pose_mesh: body_guide needs `canonical` when the frame arrives as a WarpMesh"),
    # ---- run_cuda, run
    ("run_cuda no grid", {}, False, False, lambda n: n.run_cuda(*_rays(), 64, 1.0, 64, None, render_can=False, normal_epsilon_ratio=1.0), R,
     "run_cuda needs NeRFNetwork(cuda_ray=True) (density grid + step counters)"),
    ("run_cuda posed", dict(cuda_ray=True, curvature_loss=True), False, False, lambda n: n.run_cuda(*_rays(), 64, 1.0, 64, None, render_can=False), N,
     "the occupancy grid lives in canonical space: cuda_ray renders render_can=True only"),
    ("run_cuda curvature", dict(cuda_ray=True, curvature_loss=True), False, False, lambda n: n.run_cuda(*_rays(), 64, 1.0, 64, None, normal_epsilon_ratio=1), N,
     "run_cuda is built for the default NeRFNetwork (with or without view directions; no curvature term)"),
    ("run_cuda fd step", dict(cuda_ray=True), False, False, lambda n: n.run_cuda(*_rays(), 64, 1.0, 64, None, normal_epsilon_ratio=1), R,
     "run_cuda: normal_epsilon_ratio must be < 1 (finite-difference step 0.005 * (1 - ratio) > 0)"),
    ("run_cuda fd step default", dict(cuda_ray=True), False, False, lambda n: n.render(*_rays(), 64, 1.0, 64), R,
     "run_cuda: normal_epsilon_ratio must be < 1 (finite-difference step 0.005 * (1 - ratio) > 0)"),
    ("run posed without faces", {}, False, False, lambda n: n.eval().run(*_rays(), 32, 1.0, 32, None, render_can=False, verts=torch.zeros(3, 3)), R,
     "render_can=False needs verts, faces and Ts"),
    ("run sdf side", dict(hidden_dim=32), False, False, lambda n: n.run(*_rays(), 64, 1.0, 64, None, render_can=False), N,
     "the MI355X renderer needs the default SDF side of NeRFNetwork (16-level hash grid, include_input, SDF network 35-64-16); other widths / depths have no "
     "sampling kernel"),
    ("render sdf side", dict(geo_feat_dim=7), False, False, lambda n: n.render(*_rays(), 64, 1.0, 64), N,
     "the MI355X renderer needs the default SDF side of NeRFNetwork (16-level hash grid, include_input, SDF network 35-64-16); other widths / depths have no "
     "sampling kernel"),
]


@pytest.mark.parametrize("label, ctor, gpu_like, grad, call, exc, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_model_refusals(label, ctor, gpu_like, grad, call, exc, message):
    """type, full text (anchored at both ends) and order of the refusals a model makes before any launch"""
    net = _net(**ctor)
    if gpu_like:
        _gpu_like(net)
    with torch.set_grad_enabled(grad):
        with pytest.raises(exc) as e:
            call(net)
    assert e.type is exc
    if message is not None and exc is not _Launched:
        assert re.fullmatch(re.escape(message), str(e.value)), str(e.value)


@pytest.fixture()
def chosen(monkeypatch):
    """default-SDF-side models on the CPU whose fields are recorders, the way test_half_table_host.py replaces them: which one did a call take?"""
    from avatarcraft_amd import instant_nsr as M
    took = []
    monkeypatch.setattr(M.NeRFNetwork, "_field", lambda self: took.append("full") or "full")
    monkeypatch.setattr(M.NeRFNetwork, "_field_sdf_only", lambda self: took.append("sdf_only") or "sdf_only")

    def sampled(field, *a, **kw):
        raise _Launched(field)
    for name in ("sample_rays", "sample_rays_long"):
        monkeypatch.setattr(M.nsr_ops, name, sampled)
    return took


@pytest.mark.parametrize("ctor, field", [({}, "full"), (dict(curvature_loss=True), "sdf_only"), (dict(hidden_dim_color=32), "sdf_only")])
def test_the_sampling_stage_takes_the_field_the_model_allows(chosen, ctor, field):
    """through run() alone (train mode, gradients wanted, fused_training off: the sampling launch gets the selected field)"""
    net = _net(**ctor)
    net.fused_training = False
    with pytest.raises(_Launched) as e:
        net.run(*_rays(), 64, 1.0, 64, None)
    assert chosen == [field] and e.value.args == (field,)


def test_shared_helpers(chosen):
    """the helpers by name (they exist since the split): the field selection, and "would autograd record" """
    for ctor, plain, ignoring in (({}, "full", "full"), (dict(curvature_loss=True), "sdf_only", "full"), (dict(hidden_dim_color=32), "sdf_only", "sdf_only"),
                                  (dict(use_viewdirs=True), "full", "full")):
        net = _net(**ctor)
        del chosen[:]
        assert (net._field_for(), net._field_for(ignore_curvature=True)) == (plain, ignoring) and chosen == [plain, ignoring]
    net = _net()
    assert net._records_graph() is True
    with torch.no_grad():
        assert net._records_graph() is False
    for p in net.parameters():
        p.requires_grad_(False)
    assert net._records_graph() is False
    from avatarcraft_amd.instant_nsr import renderer
    ro, rd = renderer._flat_rays(torch.zeros(2, 3, 3, dtype=torch.float64).transpose(0, 1), torch.ones(1, 6, 3))
    assert ro.shape == rd.shape == (6, 3) and ro.dtype == torch.float32 and ro.is_contiguous()
    assert net._long_save_stencil(32, 32) is False
    net.long_step_extras = True
    assert net._long_save_stencil(32, 32) is True and net._long_save_stencil(40, 17) is False
