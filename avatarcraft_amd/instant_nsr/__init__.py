"""Instant-NSR model + NeuS renderer behind the reference's model API (models/instant_nsr.py:90-726).

`NeRFNetwork()` has the reference's constructor, parameter names (state_dict keys: encoder.embeddings,
encoder.offsets, sdf_net.{0,1}.{bias,weight_g,weight_v}, color_net.{0,1,2}.{weight_g,weight_v},
deviation_net.variance -- SURVEY section 5) and `.render(...)` signature / result keys, so the reference's drivers
and checkpoints (bare_smpl.pth.tar) work unchanged.

Where the work happens:
  * no-grad rendering (render_canonical, render_val, the sampling stage of every training render) is ONE launch of
    the fused HIP kernel (nsr_ops.render_rays == NeRFRenderer.run :133-299);
  * rendering with gradients (stylize / reconstruct) takes the sample positions from the fused kernel (the reference
    computes them under no_grad, :176-184) and evaluates the differentiable "render core" (:190-299) with autograd
    over the HIP hash encoder; a fused backward kernel is the next step.
  * render_can=False (SMPL inverse warp, :166-172,198-203): no-grad only (render_warp.py), ac_render_rays_warped; at sample counts
    outside the fused renderer's window ac_render_rays_long_warped (opt-in: posed_long_rays).

No code here: the names of the submodules, by concern, in the order of their imports (none imports one below it):
  route      Route, render_route: which nsr_ops entry a render launches (pure: no tensor)
  guard      the NaN guard of the training renders
  renderer   NeRFRenderer: caches and pickling, the fields, the switches, run / render, the step renders and backward_last
  occupancy  run_cuda and update_extra_state (cuda_ray = True)
  export     extract_fields / extract_geometry / extract_colored_mesh / extract_textured_mesh, pose_mesh
  surface    render_surface, render_surface_posed
  network    NeRFNetwork = the three mixins above on NeRFRenderer, the reference's constructor and torch forward functions
Every launch is spelled nsr_ops.<name> or getattr(nsr_ops, route.entry) at call time, so assigning to a name of the nsr_ops package redirects it.
"""
from .. import nsr_ops
from .route import Route, render_route
from .renderer import DEFAULT_GEO_THRESH, NeRFRenderer, SingleVarianceNetwork, near_far_from_bound
from .network import NeRFNetwork
