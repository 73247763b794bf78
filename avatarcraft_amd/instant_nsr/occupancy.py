"""Occupancy-grid rendering (cuda_ray = True): run_cuda, the render path the reference dispatches to and never defines, and its density grid."""
import torch
import torch.nn.functional as F

from .. import nsr_ops
from .renderer import _flat_rays, _neus_alpha, _relaxed_ratio, near_far_from_bound


class OccupancyRendering:
    """mixed into NeRFNetwork; the density grid and the step counters are registered by NeRFRenderer.__init__, where the reference has them"""

    occupancy_train_one_launch = True  # run_cuda's train() branch under no_grad (stylize.py's render_val of a cuda_ray net) as ONE launch (ac_render_rays_occupancy_train);
                                       # False: the chain of operators (march_rays_train / ac_field_samples / composite_rays_train x 2 / torch) -- same pixels
    occupancy_rounds = False           # True: run_cuda's eval() as the reference-shaped loop of compact / march / field / composite rounds (same results)
    occupancy_fused_shading = True     # run_cuda's train() branch UNDER AUTOGRAD: normal / NeuS alpha / eikonal terms of the packed samples as one launch each way
                                       # (nsr_ops.packed_shading); False: the torch formulation (kept as the cross-check of the tests)
    fused_density_grid = True

    def run_cuda(self, rays_o, rays_d, num_steps, bound, upsample_steps, bg_color, cos_anneal_ratio=1.0, normal_epsilon_ratio=1.0, render_can=True,
                 verts=None, faces=None, Ts=None, perturb_overwrite: bool = False, use_mesh_guide: bool = True, per_sample: bool = True, max_steps=1024):
        """The render path the reference dispatches to when cuda_ray=True (models/instant_nsr.py:358-363) and never defines: the chain its
        raymarching module and density grid exist for (raymarching/raymarching.py:21-188, update_extra_state :303-356), in the shape of the Instant-NSR
        code base the module was taken from --

          train():  march_rays_train (occupancy grid, perturb, align 128) -> field on the packed samples -> composite_rays_train (+ background)
          eval():   loop { compact_rays; march_rays (n_step = clamp(N / n_alive, 1, 8)); field; composite_rays } until no ray is alive or max_steps

        with the field evaluated per sample exactly like run()'s render core (:205-243): forward_sdf, finite-difference normal, forward_color and
        the NeuS alpha with the marcher's step as the section length (ac_field_samples: one fused launch; under autograd the SDF-query / colour
        operators with their fused backward).  composite_rays_train treats its first input as alpha (quirk C.4), so the chain is consistent.
        num_steps / upsample_steps are unused (the marcher decides the sampling).  Returns run()'s tuple; per-sample entries are None and the
        training depth is zero (the packed compositor has none)."""
        from .. import raymarching
        if not self.cuda_ray:
            raise RuntimeError("run_cuda needs NeRFNetwork(cuda_ray=True) (density grid + step counters)")
        if not render_can:
            raise NotImplementedError("the occupancy grid lives in canonical space: cuda_ray renders render_can=True only")
        if not self._fused_supported():
            raise NotImplementedError("run_cuda is built for the default NeRFNetwork (with or without view directions; no curvature term)")
        fd_eps = nsr_ops.FD_STEP * (1.0 - normal_epsilon_ratio)
        if not fd_eps > 0.0:
            raise RuntimeError("run_cuda: normal_epsilon_ratio must be < 1 (finite-difference step 0.005 * (1 - ratio) > 0)")
        B, N = rays_o.shape[:2]
        device = rays_o.device
        ro, rd = _flat_rays(rays_o, rays_d)
        n_rays = ro.shape[0]
        bg = 1.0                                                 # (not renderer._background: a scalar stays [1,1] here)
        if bg_color is not None:
            bg = torch.as_tensor(bg_color, dtype=torch.float32, device=device)
            bg = bg.reshape(-1, 3) if bg.numel() >= 3 else bg.reshape(1, 1)
        inv_s_t = self.forward_variance()
        if self.training:
            counter = self.step_counter[self.local_step % 64]
            counter.zero_()
            self.local_step += 1
            needs_grad = self._records_graph()
            budgeted = self.mean_count > 0
            if not needs_grad and budgeted and self.occupancy_train_one_launch:
                # no graph wanted (and a budget, so that the packed layout has a size before anything is counted): walk, packed samples, field, both composites,
                # the eikonal term and the background in one launch -- the same pixels as the chain below
                cap = raymarching.raymarching._round_up(int(self.mean_count), 128)                        # (march_rays_train's capacity: + 128 - n % 128)
                try:
                    o = nsr_ops.render_rays_occupancy_train(self._field(), ro, rd, self.density_grid, self.mean_density, bound, fd_eps, inv_s_t, cos_anneal_ratio,
                                                            perturb=bool(perturb_overwrite), capacity=cap, composite_capacity=cap, counter=counter, bg=bg)
                except nsr_ops.OccupancyBarrierTimeout:
                    # a grid barrier of the one launch timed out (compute units held by a foreign kernel for seconds): nothing was returned; the chain of
                    # operators below has no barriers and gives the same pixels.  The step counter may hold the failed launch's partial update.
                    o = None
                    counter.zero_()
                if o is not None:
                    gradient_error = o["gradient_error"][0]
                    self._guard_finite(gradient_error)
                    depth = torch.zeros(n_rays, dtype=torch.float32, device=device)
                    return (depth.reshape(B, N), None, o["weights_sum"][:, None], o["image"].reshape(B, N, 3), o["normal_map"], gradient_error, 0.0, None, None, None)
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(ro, rd, bound, self.density_grid, self.mean_density, self.iter_density, counter,
                                                                    self.mean_count, bool(perturb_overwrite), 128, False)
            M = xyzs.shape[0]
            if budgeted:
                # the rays the budget left out wrote nothing: the marched samples are a prefix of the layout that ends with the last ray that fitted
                # (rows behind it are zeros -- and would otherwise count as samples AT THE ORIGIN in the eikonal term)
                ends = rays[:, 1] + rays[:, 2]
                n_valid = (ends * ((rays[:, 2] > 0) & (ends < M))).max()
            else:
                n_valid = counter[0]
            valid = (torch.arange(M, device=device) < n_valid).float()             # rows past the marched samples are alignment padding (all-zero rows)
            if needs_grad:
                enc = self.encoder
                W = nsr_ops.weight_norm_all(list(self.sdf_net) + list(self.color_net))
                sdf_out, gradient = nsr_ops.sdf_stencil(xyzs, enc.embeddings, W[0], self.sdf_net[0].bias, W[1], self.sdf_net[1].bias, self._offsets_host(),
                                                        enc.per_level_scale, enc.base_resolution, bound, fd_eps)
                if self.occupancy_fused_shading:
                    # normal, the cos-annealed NeuS alpha and the per-sample eikonal terms as ONE launch each way (round 6: the ~40 torch kernels of the
                    # formulation in the else branch were 2.5 ms of forward + backward per 4096-ray batch against 0.5 ms for the no-grad launch)
                    nv = n_valid if isinstance(n_valid, torch.Tensor) else torch.tensor(int(n_valid), dtype=torch.int32, device=device)
                    alpha, normal, eik2 = nsr_ops.packed_shading(sdf_out, gradient, inv_s_t, xyzs, dirs, deltas, nv, cos_anneal_ratio)
                else:
                    normal = gradient / (1e-5 + torch.linalg.norm(gradient, ord=2, dim=-1, keepdim=True))
                if self.use_viewdirs:                            # (the stand-alone colour operator has no direction input: torch's colour network here)
                    rgbs = self.forward_color(xyzs, dirs, normal, sdf_out[:, 1:], bound)
                else:
                    rgbs = nsr_ops.color_mlp(xyzs, normal, sdf_out, W[2], W[3], W[4])
                if not self.occupancy_fused_shading:
                    alpha = _neus_alpha(sdf_out[:, :1], inv_s_t, (dirs * normal).sum(-1, keepdim=True), deltas, cos_anneal_ratio).reshape(-1)
            else:
                fs = nsr_ops.field_samples(self._field(), xyzs, dirs, deltas, bound, fd_eps, inv_s_t, cos_anneal_ratio, want_gradient=True)
                alpha, rgbs, normal, gradient = fs["alpha"], fs["rgb"], fs["normal"], fs["gradient"]
            if needs_grad and self.occupancy_fused_shading:
                es = eik2.sum(0)
                gradient_error = es[0] / (es[1] + 1e-5)                                   # :266-272 over the packed samples
            else:
                relax = (torch.linalg.norm(xyzs, ord=2, dim=-1) < 1.2).float() * valid
                gerr = (torch.linalg.norm(gradient, ord=2, dim=-1) - 1.0) ** 2
                gradient_error = _relaxed_ratio(relax, gerr)                              # :266-272 over the packed samples
            self._guard_finite(gradient_error)
            weights_sum, image = raymarching.composite_rays_train(alpha, rgbs, deltas, rays, bound)
            with torch.no_grad():
                _, normal_map = raymarching.composite_rays_train(alpha.detach(), normal.detach().contiguous(), deltas, rays, bound)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg
            depth = torch.zeros(n_rays, dtype=torch.float32, device=device)
            return depth.reshape(B, N), None, weights_sum[:, None], image.reshape(B, N, 3), normal_map, gradient_error, 0.0, None, None, None
        # ---- inference.  Default: ONE launch (ac_render_rays_occupancy: march + field + composite per ray, a wave's 64 rays packed into tiles) -- the
        # same bits as the reference-shaped loop below without its rounds and host read-backs; occupancy_rounds = True selects the loop.  max_steps: the
        # one launch stops a ray after exactly max_steps samples, the loop after max_steps .. max_steps + 7 (it stops at the first round that brings its step
        # count to >= max_steps): the two agree bit for bit on every ray that needs fewer (tests/test_gpu_run_cuda.py checks both sides of that line).
        if not self.occupancy_rounds:
            with torch.no_grad():
                near, far = near_far_from_bound(ro, rd, bound, type='cube')
                near, far = near.reshape(-1), far.reshape(-1)
                o = nsr_ops.render_rays_occupancy(self._field(), ro, rd, self.density_grid, self.mean_density, bound, fd_eps, inv_s_t, cos_anneal_ratio,
                                                  max_steps=max_steps)
                self._last_cuda_rounds = 0
                image = o["image"] + (1 - o["weights_sum"]).unsqueeze(-1) * bg
                depth = torch.clamp(o["depth"] - near, min=0) / (far - near)
                return (depth.reshape(B, N), None, o["weights_sum"][:, None], image.reshape(B, N, 3), o["normal_map"],
                        torch.zeros((), dtype=torch.float32, device=device), 0.0, None, None, None)
        # ---- the loop: march / evaluate / composite in rounds, dead rays compacted away between rounds (one 4-byte D2H per round, like the reference's
        # `alive_counter.item()`: the next round's step count depends on it)
        with torch.no_grad():
            field = self._field()
            f32 = dict(dtype=torch.float32, device=device)
            weights_sum, depth = torch.zeros(n_rays, **f32), torch.zeros(n_rays, **f32)
            image, normal_map = torch.zeros(n_rays, 3, **f32), torch.zeros(n_rays, 3, **f32)
            near, far = near_far_from_bound(ro, rd, bound, type='cube')
            near, far = near.reshape(-1).contiguous(), far.reshape(-1).contiguous()
            n_alive = n_rays
            alive_counter = torch.zeros(1, dtype=torch.int32, device=device)
            rays_alive = torch.zeros(2, n_rays, dtype=torch.int32, device=device)
            rays_t = torch.zeros(2, n_rays, **f32)
            step = rnd = 0
            while step < max_steps:
                if step == 0:
                    rays_alive[0] = torch.arange(n_rays, dtype=torch.int32, device=device)
                    rays_t[0] = near
                else:
                    alive_counter.zero_()
                    raymarching.compact_rays(n_alive, rays_alive[rnd % 2], rays_alive[(rnd + 1) % 2], rays_t[rnd % 2], rays_t[(rnd + 1) % 2], alive_counter)
                    n_alive = int(alive_counter.item())
                if n_alive <= 0:
                    break
                n_step = max(min(n_rays // n_alive, 8), 1)
                xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, rays_alive[rnd % 2], rays_t[rnd % 2], ro, rd, bound, self.density_grid,
                                                            self.mean_density, near, far, 128, False)
                fs = nsr_ops.field_samples(field, xyzs, dirs, deltas, bound, fd_eps, inv_s_t, cos_anneal_ratio)
                raymarching.composite_rays(n_alive, n_step, rays_alive[rnd % 2], rays_t[rnd % 2], fs["alpha"], fs["rgb"], fs["normal"], deltas, weights_sum,
                                           depth, image, normal_map)
                step += n_step
                rnd += 1
            self._last_cuda_rounds = rnd
            image = image + (1 - weights_sum).unsqueeze(-1) * bg
            depth = torch.clamp(depth - near, min=0) / (far - near)
            return (depth.reshape(B, N), None, weights_sum[:, None], image.reshape(B, N, 3), normal_map, torch.zeros((), **f32), 0.0, None, None, None)

    # ------------------------------------------------------------------ occupancy grid of the ray marcher, reference :303-356
    def update_extra_state(self, bound, decay=0.95):
        """density grid for raymarching.march_rays_train / march_rays (only with cuda_ray=True, like the reference): the SDF on the 129^3
        grid -> a logistic density with inv_s = 512 (inv_s * sigmoid'(-|...|) written in two overflow-free branches), dilated by a 2^3 max
        pool, merged into the running grid with max(grid * decay, new); mean density and the step-counter bookkeeping.
        On the GPU the grid update is ONE launch (ac_density_grid_update, csrc/field_grid.hip; the grid is updated in place); the torch chain below
        is the formulation of the reference, kept for the CPU and as the cross-check of the tests (fused_density_grid = False)."""
        if not self.cuda_ray:
            return
        resolution = self.density_grid.shape[0]
        dev = self.density_grid.device
        inv_s = 512.0
        if self.fused_density_grid and self.density_grid.is_cuda and self._sdf_supported():
            with torch.no_grad():
                f = self._field_for()
                if not self.density_grid.is_contiguous():
                    self.density_grid = self.density_grid.contiguous()
                mean = nsr_ops.density_grid_update(f, self._grid_axis(bound, resolution), self.density_grid, bound, inv_s, decay)
        else:
            axes = torch.linspace(-bound, bound, resolution).split(128)
            tmp_grid = torch.zeros_like(self.density_grid)
            with torch.no_grad():
                for xi, xs in enumerate(axes):
                    for yi, ys in enumerate(axes):
                        for zi, zs in enumerate(axes):
                            lx, ly, lz = len(xs), len(ys), len(zs)
                            xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                            pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)
                            sdf = self.density(pts, bound).detach().float().reshape(-1)
                            mask = sdf > 0
                            density = torch.zeros_like(sdf)
                            density[mask] = inv_s * torch.exp(-inv_s * sdf[mask]) / (1 + torch.exp(-inv_s * sdf[mask]))
                            density[~mask] = inv_s * torch.exp(inv_s * sdf[~mask]) / (1 + torch.exp(inv_s * sdf[~mask]))
                            tmp_grid[xi * 128: xi * 128 + lx, yi * 128: yi * 128 + ly, zi * 128: zi * 128 + lz] = density.reshape(lx, ly, lz)
                tmp_grid = F.pad(tmp_grid, (0, 1, 0, 1, 0, 1))
                tmp_grid = F.max_pool3d(tmp_grid.unsqueeze(0).unsqueeze(0), kernel_size=2, stride=1).squeeze(0).squeeze(0)
                self.density_grid = torch.maximum(self.density_grid * decay, tmp_grid)
            mean = torch.mean(self.density_grid)
        # the two scalars the marcher takes as launch constants: ONE read-back for both
        total_step = min(64, self.local_step)
        if total_step > 0:
            both = torch.stack([mean.reshape(()).double(), self.step_counter[:total_step, 0].sum().double()]).tolist()
            self.mean_density = both[0]
            self.mean_count = int(both[1] / total_step)
        else:
            self.mean_density = mean.item()
        self.iter_density += 1
        self.local_step = 0
