// avatarcraft_amd/csrc/render_core_backward.hip -- the whole differentiable render core backward in one call (ac_render_core_backward): the driver that
// chains the operators' backward passes on one stream -- normals -> compositor (composite.hip) -> colour network (color_train.hip) -> normalisation +
// eikonal glue -> SDF query (sdf_stencil_train.hip) -> table-gradient scatter (hash_stencil.hip) -- and its two glue kernels.  The driver refuses a call
// before it queues anything: check_core_backward holds every rule.
#include "train_common.hpp"
#include "field_host.hpp"

namespace {

// normal =gradient / (1e-5 + |gradient|)  (instant_nsr.py:215), the renderer's own arithmetic: the colour / compositing backward
// kernels recompute their forward from exactly the normals the forward launch used
__global__ __launch_bounds__(256) void core_normals_kernel(const float *__restrict__ grad, uint32_t B, float *__restrict__ nrm)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float gx = grad[3 * (size_t)b], gy = grad[3 * (size_t)b + 1], gz = grad[3 * (size_t)b + 2];
    const float gn = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
    nrm[3 * (size_t)b] = gx / (1e-5f + gn); nrm[3 * (size_t)b + 1] = gy / (1e-5f + gn); nrm[3 * (size_t)b + 2] = gz / (1e-5f + gn);
}

// joins the gradients that reach the SDF query: d sdf_out = (colour backward) with column 0 += (compositing backward: d sdf);
// d gradient = backward of n = g / (1e-5 + |g|) applied to d normal (compositing + colour), plus the eikonal term
// d/dg [ sum relax (|g| - 1)^2 / (sum relax + 1e-5) ] = relax 2 (|g| - 1) / den * g / |g|   (instant_nsr.py:266-272; |g| = 0 -> 0 like
// torch.linalg.norm's backward)
__global__ __launch_bounds__(256) void core_mid_kernel(const float *__restrict__ grad, const float *__restrict__ pts, const float *__restrict__ g_sdf,
                                                       const float *__restrict__ g_nrm_a, const float *__restrict__ g_nrm_b, const float *__restrict__ g_eik,
                                                       const float *__restrict__ eik_den, uint32_t B, float *__restrict__ g_s16, float *__restrict__ g_grad,
                                                       uint32_t group_samples, uint32_t den_stride)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const size_t b3 = 3 * (size_t)b;
    const float gx = grad[b3], gy = grad[b3 + 1], gz = grad[b3 + 2];
    const float r = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz), c = 1e-5f + r;
    const float ux = g_nrm_a[b3] + g_nrm_b[b3], uy = g_nrm_a[b3 + 1] + g_nrm_b[b3 + 1], uz = g_nrm_a[b3 + 2] + g_nrm_b[b3 + 2];
    const float dot = (gx * ux + gy * uy) + gz * uz;
    float k = r > 0.0f ? -dot / (r * c * c) : 0.0f;                   // d(1 / (1e-5 + r)) / dg = -g / (r c^2)
    if (g_eik) {
        const float px = pts[b3], py = pts[b3 + 1], pz = pts[b3 + 2];
        const float relax = __builtin_sqrtf((px * px + py * py) + pz * pz) < 1.2f ? 1.0f : 0.0f;
        const uint32_t grp = group_samples ? b / group_samples : 0u;      // (several patches in one launch: ac_core_upstream.eik_group_rays)
        if (r > 0.0f) k += g_eik[grp] * relax * 2.0f * (r - 1.0f) / (eik_den[(size_t)grp * den_stride] * r);
    }
    g_grad[b3] = ux / c + k * gx; g_grad[b3 + 1] = uy / c + k * gy; g_grad[b3 + 2] = uz / c + k * gz;
    g_s16[(size_t)b * 16] += g_sdf[b];
}

struct CoreLayout { size_t nrm, g_sdf, g_nrm_a, g_col, g_nrm_b, g_s16, g_grad, gfeat, part_sdf, part_col, hash, total, hash_bytes; };
CoreLayout core_layout(const ac_field *field, uint32_t B)
{
    CoreLayout l{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    l.nrm = take((size_t)B * 12); l.g_sdf = take((size_t)B * 4); l.g_nrm_a = take((size_t)B * 12); l.g_col = take((size_t)B * 12);
    l.g_nrm_b = take((size_t)B * 12); l.g_s16 = take((size_t)B * 64); l.g_grad = take((size_t)B * 12);
    l.gfeat = take((size_t)B * 7 * 16 * 2 * 4);
    l.part_sdf = take(ac_sdf_stencil_backward_scratch(B)); l.part_col = take(ac_color_backward_scratch(B));
    l.hash_bytes = field ? ac_hash_stencil_backward_scratch(field->offsets, 16, field->S, field->H, 16, B) : 0;
    l.hash = take(l.hash_bytes);
    l.total = o;
    return l;
}

// Everything ac_render_core_backward refuses at n_rays > 0, before any device work: its own rules, then those of the operators it chains, each through the
// operator's own check and in its words (the operators check again when they are called: they serve their C entries too, and can no longer refuse here).
int check_core_backward(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d, const ac_core_saved *sv,
                        const ac_core_upstream *up, const ac_core_grads *gr, const void *scratch, size_t scratch_bytes, const CoreLayout &l)
{
    const int T0 = op->num_steps, T = T0 + op->upsample_steps;
    if (!rays_o || !rays_d || !sv->z_vals || !sv->pts || !sv->sdf || !sv->sdf_out16 || !sv->gradient || !sv->color || (up->g_eik && !sv->eik_den) ||
        !gr->g_table || !gr->g_sdf_params || !gr->g_color_params || !gr->g_inv_s_per_ray) {
        ac::set_error("render_core_backward: NULL buffer"); return AC_ERR_BAD_ARG;
    }
    if (!(op->fd_eps > 0.0f)) { ac::set_error("render_core_backward: fd_eps must be positive"); return AC_ERR_BAD_ARG; }
    // at a count that 16 does not divide (the long renderer's), a 16-sample tile of the flat samples straddles two rays
    if (T % 16 && sv->feat7) {
        ac::set_error("render_core_backward: feat7 needs T a multiple of 16 (T=%d): its tiles are one ray's 16 samples; the long renderer's outputs "
                      "take the re-gathering backward (feat7 = NULL)", T);
        return AC_ERR_BAD_ARG;
    }
    if (T % 16 && field->Wc1_sh) {
        ac::set_error("render_core_backward: a field with view directions needs T a multiple of 16 (T=%d): the colour backward takes a 16-sample tile "
                      "as one ray's", T);
        return AC_ERR_BAD_ARG;
    }
    if (!scratch || scratch_bytes < l.total) { ac::set_error("render_core_backward: scratch of %zu bytes needed, %zu given", l.total, scratch_bytes); return AC_ERR_BAD_ARG; }
    if (int rc = composite_check_counts("render_core_backward", T0, T)) return rc;
    if ((op->near_m != nullptr) != (op->far_m != nullptr)) { ac::set_error("render_core_backward: near_m and far_m go together"); return AC_ERR_BAD_ARG; }
    if ((field->Wc1_sh != nullptr) != (sv->sh_bias != nullptr) || (field->Wc1_sh != nullptr) != (gr->g_sh_tiles != nullptr)) {
        ac::set_error("render_core_backward: a field with view directions (ac_field.Wc1_sh) needs ac_core_saved.sh_bias and ac_core_grads.g_sh_tiles, one without takes neither");
        return AC_ERR_BAD_ARG;
    }
    if (up->eik_group_rays < 0 || (up->eik_group_rays > 0 && up->eik_den_stride < 1)) { ac::set_error("render_core_backward: eik_group_rays < 0 or eik_den_stride < 1"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};                                                 // the field's rules (both networks' parameters, the level layout): the SDF query's, a superset of the colour network's
    if (int rc = prep_args(a, field, op->bound, op->fd_eps)) return rc;
    return hash_stencil_backward_check(2, 16, field->offsets, op->fd_eps, op->bound);
}

}  // namespace

AC_API size_t ac_render_core_backward_scratch(const ac_field *field, int32_t n_rays, int32_t T)
{
    if (!field || n_rays <= 0 || T <= 0) return 0;
    return core_layout(field, (uint32_t)n_rays * (uint32_t)T).total;
}

// check everything -> lay out the scratch -> launch
AC_API int ac_render_core_backward(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d, const float *bg,
                                   const ac_core_saved *sv, const ac_core_upstream *up, const ac_core_grads *gr, void *scratch, size_t scratch_bytes,
                                   ac_stream_t stream)
{
    if (!field || !op || !sv || !up || !gr) { ac::set_error("render_core_backward: NULL argument struct"); return AC_ERR_BAD_ARG; }
    if (op->n_rays <= 0) return AC_OK;
    const int T = op->num_steps + op->upsample_steps;
    const uint32_t B = (uint32_t)op->n_rays * (uint32_t)T;
    const CoreLayout l = core_layout(field, B);
    if (int rc = check_core_backward(field, op, rays_o, rays_d, sv, up, gr, scratch, scratch_bytes, l)) return rc;
    char *sb = static_cast<char *>(scratch);
    float *nrm = reinterpret_cast<float *>(sb + l.nrm), *g_sdf = reinterpret_cast<float *>(sb + l.g_sdf), *g_nrm_a = reinterpret_cast<float *>(sb + l.g_nrm_a);
    float *g_col = reinterpret_cast<float *>(sb + l.g_col), *g_nrm_b = reinterpret_cast<float *>(sb + l.g_nrm_b), *g_s16 = reinterpret_cast<float *>(sb + l.g_s16);
    float *g_grad = reinterpret_cast<float *>(sb + l.g_grad), *gfeat = reinterpret_cast<float *>(sb + l.gfeat);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t eb = (B + 255) / 256;
    hipLaunchKernelGGL(core_normals_kernel, dim3(eb), dim3(256), 0, st, sv->gradient, B, nrm);
    // NeuS alpha + compositing (instant_nsr.py:219-263,290-299)
    if (int rc = composite_backward_core(op, rays_o, rays_d, bg, sv, nrm, up, g_sdf, g_nrm_a, g_col, gr->g_inv_s_per_ray, stream)) return rc;
    if (int rc = color_backward_impl(field, sv->pts, nrm, sv->sdf_out16, g_col, B, g_nrm_b, g_s16, gr->g_color_params, sb + l.part_col,
                                     ac_color_backward_scratch(B), stream, sv->sh_bias, (uint32_t)T, gr->g_sh_tiles)) return rc;
    hipLaunchKernelGGL(core_mid_kernel, dim3(eb), dim3(256), 0, st, sv->gradient, sv->pts, g_sdf, g_nrm_a, g_nrm_b, up->g_eik, sv->eik_den, B, g_s16, g_grad,
                       (uint32_t)up->eik_group_rays * (uint32_t)T, (uint32_t)(up->eik_group_rays > 0 ? up->eik_den_stride : 0));
    if (int rc = sdf_stencil_backward_impl(field, sv->pts, g_s16, g_grad, B, op->bound, op->fd_eps, gfeat, gr->g_sdf_params, sb + l.part_sdf,
                                           ac_sdf_stencil_backward_scratch(B), stream, sv->feat7)) return rc;
    if (int rc = hash_stencil_backward_split(gfeat, sv->pts, field->offsets, gr->g_table, B, 2, 16, field->S, field->H, op->fd_eps, op->bound,
                                             l.hash_bytes ? sb + l.hash : nullptr, l.hash_bytes, stream,
                                             gr->side_stream ? (uint32_t)(gr->split_level > 0 ? gr->split_level : 0) : 0u, gr->side_stream)) return rc;
    return ac::check_launch("render_core_backward");
}

