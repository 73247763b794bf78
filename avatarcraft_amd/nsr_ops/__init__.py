"""Python front end of the fused Instant-NSR renderer (ac_render_rays & friends).

Host-side plumbing only: builds the ac_field / ac_render_opts / ac_render_out structs from torch
CUDA tensors and enqueues the HIP kernels on torch's current stream.  The numerical work of
NeRFRenderer.run (reference models/instant_nsr.py:133-299) is entirely inside
libavatarcraft_hip.so; there is no eager fallback.

No code here: the public names of the submodules, by concern, in the order of their imports (none imports one below it):
  _args      argument checks and forms every wrapper shares
  field      Field, the packed gradient layout, the launches on the field alone
  warp       WarpMesh, warp_mesh_sequence
  render     render_rays / render_rays_long, pair forms, sample_rays
  train      the autograd operators, render_core_backward, the scratch of the backward
  occupancy  the occupancy-grid renderers, their failure accounting, density_grid_update
  mesh       marching cubes, vertex / texel attributes, bind, pose, components, compact
  surface    the first-hit renderers
Callers spell every name nsr_ops.<name>; instant_nsr launches through getattr(nsr_ops, entry), so assigning to a name HERE redirects it.
"""
from ._args import _chk
from .field import (COLOR_PARAM_GRADS, COLOR_PARAM_GRADS_LEN, PG_ADD, PG_VARIANCE, PG_WEIGHT_NORM, SDF_PARAM_GRADS, SDF_PARAM_GRADS_LEN, VIEWDIR_COLS,
                    Field, PackedSlot, field_color, field_samples, field_sdf, join_viewdir_grad, param_grads, sh_bias, split_color_param_grads,
                    split_sdf_param_grads, split_viewdir_weight, variance_forward, weight_norm_forward)
from .warp import WarpMesh, warp_mesh_sequence
from .render import (FD_STEP, LONG_MAX_SAMPLES, PRECISIONS, TABLE_DTYPES, RenderResult, _render_opts, check_long_counts, check_save_stencil,
                     check_table_dtype, handoff_timeouts, in_short_window, linspace_tables, render_rays, render_rays_long, render_rays_long_pair,
                     render_rays_pair, sample_rays, sample_rays_long)
from .train import (_SdfStencil, color_mlp, composite, core_scratch, eikonal_groups, free_scratch, packed_shading, render_core, render_core_backward,
                    sdf_stencil, sds_upstream, weight_norm_all)
from .occupancy import (OCCUPANCY_PHASED_MIN_RAYS, OCCUPANCY_VERIFY, OccupancyBarrierTimeout, debug_hold_cus, density_grid_update,
                        occupancy_fallbacks, occupancy_launch_failures, render_rays_occupancy, render_rays_occupancy_train)
from .mesh import (check_slab_layers, field_sdf_grid, marching_cubes, marching_cubes_streamed, mesh_bake_texture, mesh_bind, mesh_compact,
                   mesh_components, mesh_pose, mesh_vertex_attrs, slab_windows)
from .surface import render_rays_surface, render_rays_surface_warped, surface_opts, surface_warped_opts
