// avatarcraft_amd/csrc/render_slab.hpp -- what only the two ray renderers use: the per-wave LDS slab behind the shared image and its budget at the
// renderer's AC_MAXT / AC_WPB, the state a ray's segment hands to the next, the phase counters of AC_PROFILE builds, and on the host the RenderArgs fill from
// ac_render_opts and the dispatch over the kernel instantiations.
// Included by render_fused.hip, render_long.hip and render_entry.hpp; render_rays_kernel.hpp, the kernel body render_fused.hip includes twice, relies on it.
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "field_lds.hpp"
#include "field_host.hpp"
#include <type_traits>

namespace {

constexpr int SEG_STATE = MAXT + 16 + 64;   // floats per ray handed from one segment of a ray to the next: z [128] | cT, 10 running sums | pad | (view directions) the ray's layer-1 bias [64]

constexpr int OFF_RWAVE = OFF_C3L + 2 * CF_FRAG;  // per-wave slabs of the renderer
constexpr int CF_OVERLAY = OFF_B1 - OFF_C1F;      // floats of the overlay: the prepared image keeps it behind the exact image
// per-wave slab of the renderer: the final z values (zs0) + ONE region that holds the up-sampling state (second z buffer, the two sdf
// buffers, cdf, new samples) until the sampling of the ray is finished and the finite-difference feature slab afterwards
constexpr int UPS_FLOATS = MAXT + 2 * MAXT + MAXT + 32;              // zs1[128], sd[2][128], cdf[128], znew[16] + pad
constexpr int SLAB_ACC = MAXT + (FE_SLAB > UPS_FLOATS ? FE_SLAB : UPS_FLOATS);     // the ray's ten running sums (compositing, eikonal): [16] floats, kept by lane 15
constexpr int SLAB_SHB = SLAB_ACC + 16;                                           // use_viewdirs: the ray's layer-1 bias of the colour network [64] + sh(d) [16]
constexpr int WAVE_SLAB = SLAB_SHB + 80;
constexpr int LDS_FLOATS = OFF_RWAVE + WAVES_PER_BLOCK * WAVE_SLAB;
static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget: one workgroup per CU");
static_assert(OFF_WAVE % 4 == 0 && OFF_RWAVE % 4 == 0 && WAVE_SLAB % 4 == 0, "16-byte aligned slabs");

#ifdef AC_PROFILE
#define AC_T0() unsigned long long t_prof_ = __builtin_amdgcn_s_memtime(); const unsigned long long ray_r0_ = __builtin_amdgcn_s_memrealtime()
#define AC_TICK(SLOT) { const unsigned long long t2_ = __builtin_amdgcn_s_memtime(); prof_acc[SLOT] += t2_ - t_prof_; t_prof_ = t2_; }
// item boundaries of the fused renderer: slot 0 = end of an item's last tile -> first instruction of the wave's next item (publish or pixel write, ticket,
// item decode), slot 1 = a continuing item's wait for its predecessor's flag + the load of the ray's state
#define AC_BND_MARK() prof_bm = __builtin_amdgcn_s_memtime()
#define AC_BND_TICK(SLOT) { const unsigned long long t3_ = __builtin_amdgcn_s_memtime(); prof_bnd[SLOT] += t3_ - prof_bm; prof_bm = t3_; }
#else
#define AC_T0()
#define AC_TICK(SLOT)
#define AC_BND_MARK()
#define AC_BND_TICK(SLOT)
#endif

// what both renderers (render_fused.hip, render_long.hip) take from ac_render_opts; each checks the options its own window accepts
int fill_render_common(RenderArgs &a, const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                       const float *bg, const float *noise, const float *lin_z, const float *lin_u)
{
    if (int rc = fill_args(a, field, op->bound)) return rc;
    a.rays_o = rays_o; a.rays_d = rays_d; a.bg = bg; a.noise = noise; a.lin_z = lin_z; a.lin_u = lin_u;
    a.n_rays = op->n_rays; a.T0 = op->num_steps; a.nup = op->upsample_steps / 16;
    a.inv_s = op->inv_s; a.inv_s_dev = op->inv_s_dev; a.car = op->cos_anneal_ratio; a.one_m_car = (float)(1.0 - (double)op->cos_anneal_ratio);
    a.perturb = op->perturb; a.fast = op->precision;
    a.near_m = op->near_m; a.far_m = op->far_m;
    set_fd_eps(a, op->fd_eps);
    return AC_OK;
}

// launch(FAST, EX, SH) with the three run-time switches as std::bool_constant: one kernel instantiation per combination
template <class L>
void dispatch_variants(bool fast, bool ex, bool sh, L &&launch)
{
    using T = std::true_type;
    using F = std::false_type;
    if (sh) { if (fast) { if (ex) launch(T{}, T{}, T{}); else launch(T{}, F{}, T{}); } else if (ex) launch(F{}, T{}, T{}); else launch(F{}, F{}, T{}); }
    else { if (fast) { if (ex) launch(T{}, T{}, F{}); else launch(T{}, F{}, F{}); } else if (ex) launch(F{}, T{}, F{}); else launch(F{}, F{}, F{}); }
}

}  // namespace
