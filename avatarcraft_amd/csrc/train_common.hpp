// avatarcraft_amd/csrc/train_common.hpp -- what the training operators share: the workgroup shape of their backward kernels, and the functions through which
// the whole-core backward (render_core_backward.hip) chains the operators (sdf_stencil_train.hip, color_train.hip, composite.hip, hash_stencil.hip with its table_scatter.hpp).
// RenderArgs and every kernel live in anonymous namespaces (one copy per translation unit), so what crosses files takes the C ABI's own types only.
#pragma once
#include "ac_common.hpp"

namespace {

constexpr int TW = 4;                              // waves per workgroup of the backward kernels (296 / 284 VGPRs: one wave per SIMD)
constexpr int TBLOCK = TW * 64;
constexpr int TLD = 17;                            // padded leading dimension of the transpose slabs

uint32_t train_grid(uint32_t B)
{
    const uint32_t ntiles = (B + 15) / 16;
    uint32_t blocks = (ntiles + TW - 1) / TW;
    const uint32_t cap = ac::cu_count();               // persistent, ONE workgroup per CU: their ~145 KB of LDS admit no second one, and every workgroup
                                                       // first lays the weights out in LDS (512 workgroups: backward 3.32 ms per SDS step, 256: 3.20)
    if (blocks > cap) blocks = cap;
    return blocks ? blocks : 1;
}

}  // namespace

// sdf_stencil_train.hip: ac_sdf_stencil_backward with the forward's saved stencil features (feat7: no second gather) or the position gradient (g_x)
int sdf_stencil_backward_impl(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                              float eps, float *gfeat, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream, const float *feat7,
                              float *g_x = nullptr);
// out[i] = sum over w < nwaves of partials[w][i], i < n_out: the per-wave weight-gradient partials of both backward kernels, in a fixed order
void partials_reduce(const float *partials, uint32_t nwaves, uint32_t n_out, float *out, hipStream_t st);

// color_train.hip: ac_color_backward on a per-ray layer-1 bias (sh_bias [B / T, 64], its gradient per tile to g_sh_tiles; NULL, 16, NULL = none)
int color_backward_impl(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
                        float *g_normal, float *g_sdf16, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream,
                        const float *sh_bias, uint32_t T, float *g_sh_tiles);

// composite.hip: the sample counts the compositor takes (AC_ERR_BAD_ARG naming the rule for `who` otherwise), and ac_composite_backward as the whole-core
// backward runs it: inv_s from the device where opts has it there, the posed range and mask, upstream gradients that may be NULL (= 0).  It launches and
// leaves the launch check to its caller.
int composite_check_counts(const char *who, int32_t T0, int32_t T);
int composite_backward_core(const ac_render_opts *op, const float *rays_o, const float *rays_d, const float *bg, const ac_core_saved *sv, const float *nrm,
                            const ac_core_upstream *up, float *g_sdf, float *g_nrm, float *g_col, float *g_inv_s_per_ray, ac_stream_t stream);

// hash_stencil.hip: the argument rules of ac_hash_stencil_backward, and that entry with the accumulation split at a level and a side stream ordered behind
// the first part (queue_scatter, table_scatter.hpp)
int hash_stencil_backward_check(uint32_t C, uint32_t L, const int32_t *offsets_host, float eps, float bound);
int hash_stencil_backward_split(const float *grad, const float *x, const int32_t *offsets_host, float *grad_embeddings, uint32_t B,
                                uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, void *scratch, size_t scratch_bytes,
                                ac_stream_t stream, uint32_t split_level, ac_stream_t side_stream);
