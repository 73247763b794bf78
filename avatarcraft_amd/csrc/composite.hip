// avatarcraft_amd/csrc/composite.hip -- the ray compositor of the differentiable render core (training path), forward and backward.
//
// NeuS alpha + compositing of the render core (models/instant_nsr.py:219-263,290-299) for training: one wave per ray, the
// forward is the renderer's own arithmetic (16-sample tile scans with sequential carry), the backward recomputes it.
//   forward : (z, sdf, normal, colour, ray) -> image, weights_sum, depth, normal_map, weights, alpha
//   backward: (d image, d weights_sum, d depth, d normal_map) -> d sdf, d normal, d colour, per-ray partial of d inv_s
// Two instantiations each way, chosen by comp_launch:
//   CAP = 128, RAGGED = false: the short window (T a multiple of 16, at most 128), render_rays_kernel's tiles;
//   CAP = 512, RAGGED = true : the long renderer's envelope (any T up to 512), render_rays_long_kernel's tiles -- ceil(T / 16) of them, the last one
//     masked by that kernel's rules (render_long.hip): a masked lane evaluates the ray's last sample again, contributes the identity (1, not 1 + 1e-7)
//     to the transmittance scan and exact zeros (weight 0) to every sum, and writes nothing.  The weights and transmittances it recomputes are
//     therefore the long forward's bit for bit.
#include "train_common.hpp"
#include "wave_ops.hpp"
#include "ac_devmath.hpp"
#include "ac_sp_table.hpp"

using namespace acdev;

namespace {

struct CompArgs {
    const float *rays_o, *rays_d, *z, *sdf, *nrm, *col, *bg;
    int n_rays, T0, T;
    float bound, inv_s, car, one_m_car;
    const float *inv_s_dev;      // non-NULL: inv_s lives in device memory (the trainable variance), read once per kernel
    // posed space (the backward of run(render_can=False), instant_nsr.py:147-153,246-249): mesh-guided range where finite, alpha * mask; NULL = off
    const float *near_m, *far_m;
    const uint8_t *mask;
};

struct CompSample { float alpha, om, u, pc, nc, half, delta, tc, zn; };

__device__ __forceinline__ CompSample comp_sample(const float *__restrict__ spg, const CompArgs &a, const float *__restrict__ zr, int i, float sdf0,
                                                  float nx, float ny, float nz, float dx, float dy, float dz, float near, float span, float sample_dist)
{
    CompSample s;
    const float zi = zr[i];
    s.delta = (i < a.T - 1) ? zr[i + 1] - zi : sample_dist;
    s.tc = (dx * nx + dy * ny) + dz * nz;
    const float a1 = dv_softplus100(spg, -s.tc * 0.5f + 0.5f) * a.one_m_car;
    const float a2 = dv_softplus100(spg, -s.tc) * a.car;
    const float iter_cos = -(a1 + a2);
    s.half = iter_cos * s.delta * 0.5f;
    s.pc = dv_sigmoid((sdf0 - s.half) * a.inv_s); s.nc = dv_sigmoid((sdf0 + s.half) * a.inv_s);
    s.u = (s.pc - s.nc + 1e-5f) / (s.pc + 1e-5f);
    s.alpha = clampf(s.u, 0.0f, 1.0f);
    s.om = 1.0f - s.alpha + 1e-7f;
    s.zn = clampf((zi - near) / span, 0.0f, 1.0f);
    return s;
}

template <int CAP, bool RAGGED>
__global__ __launch_bounds__(256) void composite_fwd_kernel(const CompArgs a_in, float *__restrict__ image, float *__restrict__ wsum,
                                                            float *__restrict__ depth, float *__restrict__ nmap, float *__restrict__ weights,
                                                            float *__restrict__ alpha_out)
{
    CompArgs a = a_in;
    if (a.inv_s_dev) a.inv_s = *a.inv_s_dev;
    __shared__ float spg[SPQ_FLOATS];
    __shared__ float zsh[4][CAP];
    for (int e = threadIdx.x; e < SPQ_FLOATS; e += blockDim.x) spg[e] = AC_SP_G[e >> 2][e & 3];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15;
    float *zr = zsh[wave];
    for (int ray = blockIdx.x * 4 + wave; ray < a.n_rays; ray += gridDim.x * 4) {
        const float ox = a.rays_o[3 * ray], oy = a.rays_o[3 * ray + 1], oz = a.rays_o[3 * ray + 2];
        const float dx = a.rays_d[3 * ray], dy = a.rays_d[3 * ray + 1], dz = a.rays_d[3 * ray + 2];
        float near, far;
        cube_near_far(ox, oy, oz, dx, dy, dz, a.bound, near, far);
        if (a.near_m) {
            const float nm = a.near_m[ray], fm = a.far_m[ray];
            if (!is_inf(nm)) near = nm;
            if (!is_inf(fm)) far = fm;
        }
        const float span = far - near, sample_dist = span / (float)a.T0;
        for (int i = lane; i < a.T; i += 64) zr[i] = a.z[(size_t)ray * a.T + i];
        wave_sync();
        float cT = 1.0f, s_w = 0.0f, s_r = 0.0f, s_g = 0.0f, s_b = 0.0f, s_nx = 0.0f, s_ny = 0.0f, s_nz = 0.0f, s_d = 0.0f;
        for (int c = 0; c < (RAGGED ? (a.T + 15) / 16 : a.T / 16); ++c) {
            int i = 16 * c + n;
            const bool valid = !RAGGED || i < a.T;
            if (!valid) i = a.T - 1;                                                            // a masked lane: the ray's last sample again
            const size_t si = (size_t)ray * a.T + i;
            const float nx = a.nrm[3 * si], ny = a.nrm[3 * si + 1], nz = a.nrm[3 * si + 2];
            CompSample s = comp_sample(spg, a, zr, i, a.sdf[si], nx, ny, nz, dx, dy, dz, near, span, sample_dist);
            if (a.mask && !a.mask[si]) { s.alpha = 0.0f; s.om = 1.0f + 1e-7f; }                 // alpha * 0; the factor 1 - 0 + 1e-7 stays in the product
            if (!valid) { s.alpha = 0.0f; s.om = 1.0f; }                                        // the identity of the product scan, weight 0
            const float loc = row_scan<true>(s.om);
            const float sh = dpp_shr<1>(1.0f, loc);
            float Tex;
            if (n == 0) Tex = (c == 0) ? 1.0f : cT;
            else Tex = (c == 0) ? sh : cT * sh;
            const float tot = lane_bcast(loc, 15);
            cT = (c == 0) ? tot : cT * tot;
            const float wgt = s.alpha * Tex;
            const float r = a.col[3 * si], g = a.col[3 * si + 1], b = a.col[3 * si + 2];
#define AC_ACC(S, V) { const float t_ = lane_bcast(row_scan<false>(V), 15); S = (c == 0) ? t_ : S + t_; }
            AC_ACC(s_w, wgt)
            AC_ACC(s_r, r * wgt) AC_ACC(s_nx, nx * wgt)
            AC_ACC(s_g, g * wgt) AC_ACC(s_ny, ny * wgt)
            AC_ACC(s_b, b * wgt) AC_ACC(s_nz, nz * wgt)
            AC_ACC(s_d, wgt * s.zn)
#undef AC_ACC
            if (lane < 16 && valid) { weights[si] = wgt; alpha_out[si] = s.alpha; }
        }
        if (lane == 0) {
            const float b0 = a.bg ? a.bg[3 * ray] : 1.0f, b1 = a.bg ? a.bg[3 * ray + 1] : 1.0f, b2 = a.bg ? a.bg[3 * ray + 2] : 1.0f;
            image[3 * ray] = s_r + (1.0f - s_w) * b0; image[3 * ray + 1] = s_g + (1.0f - s_w) * b1; image[3 * ray + 2] = s_b + (1.0f - s_w) * b2;
            nmap[3 * ray] = s_nx; nmap[3 * ray + 1] = s_ny; nmap[3 * ray + 2] = s_nz;
            wsum[ray] = s_w; depth[ray] = s_d;
        }
        wave_sync();
    }
}

template <int CAP, bool RAGGED>
__global__ __launch_bounds__(256) void composite_bwd_kernel(const CompArgs a_in, const float *__restrict__ g_image, const float *__restrict__ g_wsum,
                                                            const float *__restrict__ g_depth, const float *__restrict__ g_nmap,
                                                            float *__restrict__ g_sdf, float *__restrict__ g_nrm, float *__restrict__ g_col,
                                                            float *__restrict__ g_invs_ray)
{
    CompArgs a = a_in;
    if (a.inv_s_dev) a.inv_s = *a.inv_s_dev;
    __shared__ float spg[SPQ_FLOATS];
    __shared__ float zsh[4][CAP], tex[4][CAP], wq[4][CAP], psum[4][CAP];
    for (int e = threadIdx.x; e < SPQ_FLOATS; e += blockDim.x) spg[e] = AC_SP_G[e >> 2][e & 3];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15;
    float *zr = zsh[wave];
    for (int ray = blockIdx.x * 4 + wave; ray < a.n_rays; ray += gridDim.x * 4) {
        const float ox = a.rays_o[3 * ray], oy = a.rays_o[3 * ray + 1], oz = a.rays_o[3 * ray + 2];
        const float dx = a.rays_d[3 * ray], dy = a.rays_d[3 * ray + 1], dz = a.rays_d[3 * ray + 2];
        float near, far;
        cube_near_far(ox, oy, oz, dx, dy, dz, a.bound, near, far);
        if (a.near_m) {
            const float nm = a.near_m[ray], fm = a.far_m[ray];
            if (!is_inf(nm)) near = nm;
            if (!is_inf(fm)) far = fm;
        }
        const float span = far - near, sample_dist = span / (float)a.T0;
        for (int i = lane; i < a.T; i += 64) zr[i] = a.z[(size_t)ray * a.T + i];
        wave_sync();
        const float gi0 = g_image ? g_image[3 * ray] : 0.0f, gi1 = g_image ? g_image[3 * ray + 1] : 0.0f, gi2 = g_image ? g_image[3 * ray + 2] : 0.0f;
        const float gws = g_wsum ? g_wsum[ray] : 0.0f, gdp = g_depth ? g_depth[ray] : 0.0f;          // NULL upstream = zero gradient
        const float gn0 = g_nmap ? g_nmap[3 * ray] : 0.0f, gn1 = g_nmap ? g_nmap[3 * ray + 1] : 0.0f, gn2 = g_nmap ? g_nmap[3 * ray + 2] : 0.0f;
        const float b0 = a.bg ? a.bg[3 * ray] : 1.0f, b1 = a.bg ? a.bg[3 * ray + 1] : 1.0f, b2 = a.bg ? a.bg[3 * ray + 2] : 1.0f;
        // pass A: transmittance, weights, d loss / d w_i, prefix sums of dw_i w_i
        float cT = 1.0f, run = 0.0f;
        for (int c = 0; c < (RAGGED ? (a.T + 15) / 16 : a.T / 16); ++c) {
            int i = 16 * c + n;
            const bool valid = !RAGGED || i < a.T;
            if (!valid) i = a.T - 1;                                                            // as in the forward
            const size_t si = (size_t)ray * a.T + i;
            const float nx = a.nrm[3 * si], ny = a.nrm[3 * si + 1], nz = a.nrm[3 * si + 2];
            CompSample s = comp_sample(spg, a, zr, i, a.sdf[si], nx, ny, nz, dx, dy, dz, near, span, sample_dist);
            if (a.mask && !a.mask[si]) { s.alpha = 0.0f; s.om = 1.0f + 1e-7f; }                 // alpha * 0; the factor 1 - 0 + 1e-7 stays in the product
            if (!valid) { s.alpha = 0.0f; s.om = 1.0f; }                                        // weight 0: dw * 0 adds an exact zero to the prefix sums
            const float loc = row_scan<true>(s.om);
            const float sh = dpp_shr<1>(1.0f, loc);
            float Tex;
            if (n == 0) Tex = (c == 0) ? 1.0f : cT;
            else Tex = (c == 0) ? sh : cT * sh;
            const float tot = lane_bcast(loc, 15);
            cT = (c == 0) ? tot : cT * tot;
            const float wgt = s.alpha * Tex;
            const float r = a.col[3 * si], g = a.col[3 * si + 1], b = a.col[3 * si + 2];
            const float dw = ((gi0 * (r - b0) + gi1 * (g - b1)) + gi2 * (b - b2)) + gws + gdp * s.zn + ((gn0 * nx + gn1 * ny) + gn2 * nz);
            const float incl = row_scan<false>(dw * wgt) + run;
            run = lane_bcast(incl, 15);
            if (lane < 16 && valid) { tex[wave][i] = Tex; wq[wave][i] = dw; psum[wave][i] = incl; }
        }
        const float total = run;
        wave_sync();
        // pass B: every lane one sample (two chunks of 64)
        float ds_acc = 0.0f;
        for (int i = lane; i < a.T; i += 64) {
            const size_t si = (size_t)ray * a.T + i;
            const float nx = a.nrm[3 * si], ny = a.nrm[3 * si + 1], nz = a.nrm[3 * si + 2];
            const float sdf0 = a.sdf[si];
            CompSample s = comp_sample(spg, a, zr, i, sdf0, nx, ny, nz, dx, dy, dz, near, span, sample_dist);
            const bool masked = a.mask && !a.mask[si];
            if (masked) { s.alpha = 0.0f; s.om = 1.0f + 1e-7f; }
            const float Tex = tex[wave][i], dw = wq[wave][i];
            const float wgt = s.alpha * Tex;
            const float suffix = total - psum[wave][i];                         // sum over j > i of dw_j w_j
            const float dalpha = masked ? 0.0f : dw * Tex - suffix / s.om;      // d (alpha * mask) / d alpha = mask
            const float du = (s.u >= 0.0f && s.u <= 1.0f) ? dalpha : 0.0f;      // torch.clip passes the gradient on the closed interval
            const float den = s.pc + 1e-5f;
            const float dpc = du * s.nc / (den * den), dnc = -du / den;
            const float dap = dpc * s.pc * (1.0f - s.pc), dan = dnc * s.nc * (1.0f - s.nc);
            const float dsdf = (dap + dan) * a.inv_s;
            const float dhalf = (dan - dap) * a.inv_s;
            ds_acc += dap * (sdf0 - s.half) + dan * (sdf0 + s.half);
            const float dic = dhalf * s.delta * 0.5f;
            float v1, d1, v2, d2;
            softplus100_vg(spg, -s.tc * 0.5f + 0.5f, v1, d1);
            softplus100_vg(spg, -s.tc, v2, d2);
            const float dtc = dic * (0.5f * d1 * a.one_m_car + d2 * a.car);
            g_sdf[si] = dsdf;
            g_nrm[3 * si] = dtc * dx + wgt * gn0; g_nrm[3 * si + 1] = dtc * dy + wgt * gn1; g_nrm[3 * si + 2] = dtc * dz + wgt * gn2;
            g_col[3 * si] = wgt * gi0; g_col[3 * si + 1] = wgt * gi1; g_col[3 * si + 2] = wgt * gi2;
        }
        // per-ray partial of d inv_s: wave reduction
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) ds_acc += __shfl_xor(ds_acc, d);
        if (lane == 0) g_invs_ray[ray] = ds_acc;
        wave_sync();
    }
}

constexpr int COMP_LONG_MAX_T = 512;

int comp_args(CompArgs &a, const char *who, const float *rays_o, const float *rays_d, const float *z, const float *sdf, const float *nrm,
              const float *col, const float *bg, int32_t n_rays, int32_t T0, int32_t T, float bound, float inv_s, float car)
{
    if (!rays_o || !rays_d || !z || !sdf || !nrm || !col) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    if (int rc = composite_check_counts(who, T0, T)) return rc;
    a.rays_o = rays_o; a.rays_d = rays_d; a.z = z; a.sdf = sdf; a.nrm = nrm; a.col = col; a.bg = bg;
    a.n_rays = n_rays; a.T0 = T0; a.T = T; a.bound = bound; a.inv_s = inv_s; a.car = car; a.one_m_car = (float)(1.0 - (double)car);
    a.inv_s_dev = nullptr;
    a.near_m = a.far_m = nullptr; a.mask = nullptr;
    return AC_OK;
}

// one launch of either direction: a workgroup of four waves per four rays, and the long instantiation (composite_*_kernel<512, true>) where the short one
// does not apply
template <class Short, class Long, class... Args>
void comp_launch(Short short_kernel, Long long_kernel, const CompArgs &a, ac_stream_t stream, Args... args)
{
    int blocks = (a.n_rays + 3) / 4; if (blocks > 4096) blocks = 4096;
    if (a.T > 128 || a.T % 16) hipLaunchKernelGGL(long_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, args...);
    else hipLaunchKernelGGL(short_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, args...);
}
void comp_launch_bwd(const CompArgs &a, const float *g_image, const float *g_weights_sum, const float *g_depth, const float *g_normal_map, float *g_sdf,
                     float *g_normal, float *g_color, float *g_inv_s_per_ray, ac_stream_t stream)
{
    comp_launch(composite_bwd_kernel<128, false>, composite_bwd_kernel<COMP_LONG_MAX_T, true>, a, stream, g_image, g_weights_sum, g_depth, g_normal_map, g_sdf,
                g_normal, g_color, g_inv_s_per_ray);
}

}  // namespace

int composite_check_counts(const char *who, int32_t T0, int32_t T)
{
    const bool short_ok = T0 > 0 && T % 16 == 0 && T >= T0 && T <= 128;
    const bool long_ok = T0 >= 2 && T >= T0 && (T - T0) % 16 == 0 && T <= COMP_LONG_MAX_T;          // ac_render_rays_long's counts
    if (short_ok || long_ok) return AC_OK;
    ac::set_error("%s: T0=%d T=%d unsupported (T a multiple of 16, <= 128; or T0 >= 2, T - T0 >= 0 a multiple of 16, T <= %d)", who, T0, T, COMP_LONG_MAX_T);
    return AC_ERR_BAD_ARG;
}

AC_API int ac_composite_forward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf, const float *normal, const float *color,
                                const float *bg, int32_t n_rays, int32_t num_steps, int32_t T, float bound, float inv_s, float cos_anneal_ratio,
                                float *image, float *weights_sum, float *depth, float *normal_map, float *weights, float *alpha, ac_stream_t stream)
{
    if (n_rays <= 0) return AC_OK;
    CompArgs a{};
    if (int rc = comp_args(a, "composite_forward", rays_o, rays_d, z_vals, sdf, normal, color, bg, n_rays, num_steps, T, bound, inv_s, cos_anneal_ratio)) return rc;
    if (!image || !weights_sum || !depth || !normal_map || !weights || !alpha) { ac::set_error("composite_forward: NULL output"); return AC_ERR_BAD_ARG; }
    comp_launch(composite_fwd_kernel<128, false>, composite_fwd_kernel<COMP_LONG_MAX_T, true>, a, stream, image, weights_sum, depth, normal_map, weights, alpha);
    return ac::check_launch("composite_forward");
}

AC_API int ac_composite_backward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf, const float *normal, const float *color,
                                 const float *bg, int32_t n_rays, int32_t num_steps, int32_t T, float bound, float inv_s, float cos_anneal_ratio,
                                 const float *g_image, const float *g_weights_sum, const float *g_depth, const float *g_normal_map,
                                 float *g_sdf, float *g_normal, float *g_color, float *g_inv_s_per_ray, ac_stream_t stream)
{
    if (n_rays <= 0) return AC_OK;
    CompArgs a{};
    if (int rc = comp_args(a, "composite_backward", rays_o, rays_d, z_vals, sdf, normal, color, bg, n_rays, num_steps, T, bound, inv_s, cos_anneal_ratio)) return rc;
    if (!g_image || !g_weights_sum || !g_depth || !g_normal_map || !g_sdf || !g_normal || !g_color || !g_inv_s_per_ray) {
        ac::set_error("composite_backward: NULL buffer"); return AC_ERR_BAD_ARG;
    }
    comp_launch_bwd(a, g_image, g_weights_sum, g_depth, g_normal_map, g_sdf, g_normal, g_color, g_inv_s_per_ray, stream);
    return ac::check_launch("composite_backward");
}

int composite_backward_core(const ac_render_opts *op, const float *rays_o, const float *rays_d, const float *bg, const ac_core_saved *sv, const float *nrm,
                            const ac_core_upstream *up, float *g_sdf, float *g_nrm, float *g_col, float *g_inv_s_per_ray, ac_stream_t stream)
{
    CompArgs a{};
    if (int rc = comp_args(a, "render_core_backward", rays_o, rays_d, sv->z_vals, sv->sdf, nrm, sv->color, bg, op->n_rays, op->num_steps,
                           op->num_steps + op->upsample_steps, op->bound, op->inv_s, op->cos_anneal_ratio)) return rc;
    a.inv_s_dev = op->inv_s_dev;
    a.near_m = op->near_m; a.far_m = op->far_m; a.mask = sv->mask;          // posed space: the range and the alpha mask of the forward
    comp_launch_bwd(a, up->g_image, up->g_weights_sum, up->g_depth, up->g_normal_map, g_sdf, g_nrm, g_col, g_inv_s_per_ray, stream);
    return AC_OK;
}

