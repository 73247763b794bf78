// avatarcraft_amd/csrc/field_args.hpp -- what a launch that evaluates the Instant-NSR field is given: the workgroup and window defaults (AC_WPB, AC_MAXT,
// AC_ENC_ROUND; render_long.hip sets its own before its first include, and no other header gives them a default), the per-level records, RenderArgs, the
// kernel modes and FieldCtx, the part of the arguments the field code itself reads.
// Included by field_lds.hpp and field_host.hpp, and through them by every file that evaluates the field.
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "ac_common.hpp"
#include "ac_devmath.hpp"

using namespace acdev;

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

#ifndef AC_WPB
#define AC_WPB 8
#endif
constexpr int WAVES_PER_BLOCK = AC_WPB;
constexpr int BLOCK = WAVES_PER_BLOCK * 64;
#ifndef AC_MAXT
#define AC_MAXT 128         // samples per ray a wave's LDS slab holds (render_long.hip: 512, at fewer waves per workgroup)
#endif
constexpr int MAXT = AC_MAXT;
#ifndef AC_ENC_ROUND
#define AC_ENC_ROUND 2      // hash levels gathered per round per lane (registers vs loads in flight)
#endif

// per-level launch constants: index = (hashed ? x ^ y*my ^ z*mz : x + y*my + z*mz) & mask [% wsize if wsize]
// (my,mz) = (P1,P2) for hashed levels, (res+1, (res+1)^2) for dense ones; mask = size-1 for power-of-two hashed
// levels, ~0 otherwise (a dense index is < size by construction); wsize = size only for a hashed level whose size
// is not a power of two (never the case for tables allocated by HashEncoder, handled for completeness).
struct LevelRec { float scale; uint32_t my, mz, offset, mask, hashed, wsize, pad; };

struct RenderArgs {
    const float *table;
    uint32_t table_bytes;
    const float *W1, *b1, *W2, *b2, *Wc1, *Wc2, *Wc3;
    const float *Wsh;           // ac_field.Wc1_sh: [64,16] colour layer-1 columns of the 16 spherical harmonics of the view direction, or NULL (no view directions)
    const float *prepared;      // ac_field.prepared: the renderer's LDS image [0, OFF_RWAVE) of these parameters, or NULL
    const float *rays_o, *rays_d, *bg, *noise, *lin_z, *lin_u;
    ac_render_out out;
    LevelRec lvl[16];
    int n_rays, T0, nup;
    int jmode[4];          // per gather round j (levels 4j..4j+3): 0 all dense, 1 all hashed, 2 mixed
    int jfine[4];          // per round: 1 if the FD offset eps can span >= 1 cell on any of its levels
    float bound, two_bound, inv_s, car, one_m_car, eps;
    float inv_tb;          // RN(1 / two_bound) if the divisor is one of the exhaustively verified ones (unit_div), else 0: IEEE division
    const float *inv_s_dev;     // non-NULL: inv_s is read from device memory (ac_render_opts.inv_s_dev)
    int fast;                   // ac_render_opts.precision
    int skip_masked;            // ac_render_opts.skip_masked (MODE_FINAL only)
    int opacity_only;           // ac_render_opts.opacity_only: no colour network (rgb = 0)
    int perturb;
    unsigned long long *prof;   // AC_PROFILE builds only: [n_waves][10]: 8 per-phase s_memtime counters, whole-wave s_memtime and s_memrealtime (100 MHz); [n_rays * 10 + ray] per-ray wall time; [n_rays * 11 + 2 wave + k] the boundary slots (AC_BND_TICK)
    // posed-space rendering (render_can=False) only: see ac_render_rays_warped
    const float *near_m, *far_m;   // [N] mesh-guided range (+-inf where the ray misses the body) or NULL
    const float *ext_pts;          // MODE_UPSAMPLE: warped coarse points [N,T0,3]; MODE_FINAL: warped mid points [N,T,3]
    const uint8_t *mask;           // MODE_FINAL: [N,T] alpha mask
    uint32_t *ray_counter;         // [8 XCDs] ticket counters, 8 words apart (zero before the launch): ticket t of an XCD takes item t of its work list
    uint32_t *seg_flags;           // [N] number of finished items of each ray, tagged with the launch generation, or NULL (one item per ray)
    float *seg_state;              // [N][SEG_STATE] what a ray's next item continues from: z values + running sums (library scratch)
    const uint32_t *work_list;     // MODE_FULL: the work lists of the launch (render_worklist.hpp: 16 header words, then two words per item); NULL: one item per ray, in closed form
    // pair launches (ac_render_rays_pair): the same pair_n rays twice, n_rays = 2 * pair_n work items handed out as a0 b0 a1 b1 ...; copy a = rows
    // [0, pair_n), copy b = rows [pair_n, 2 pair_n) of noise, bg and the per-ray outputs; rays_o / rays_d / near_m / far_m have pair_n rows.  0 = off.
    int pair_n;
    // launch hygiene (round 3): the last workgroup to finish (ticket from done_counter) reduces gradient_error into eik_red -- [1 or 2 (pair)][2] floats:
    // (sum relax * err / (sum relax + 1e-5), sum relax + 1e-5) in eikonal_reduce_kernel's fixed order, bit for bit -- and re-arms the work counters for the
    // slot's next launch; seg_flags carry the launch generation (gen << 4 | finished segments), so they need no clearing either: no memset and no reduction
    // launch around the render kernel.
    uint32_t *done_counter;
    uint32_t *handoff_timeouts;    // device word counting segment hand-offs that timed out (ac_render_handoff_timeouts), or NULL
    float *eik_red;
    uint32_t gen;
    int ex_from;                   // the per-sample outputs (EX kernels) are kept for rays >= ex_from only, at row ray - ex_from of arrays with ex_rows rows
    int ex_rows;
    const uint8_t *ray_dead;       // MODE_UPSAMPLE, skip_masked: [N] rays that cannot hold an unmasked sample (no field evaluation, coarse z only)
    float *zbuf;                   // [N,T] final z values: written by MODE_UPSAMPLE, read by MODE_FINAL
    float *mid_pts;                // MODE_UPSAMPLE: posed-space mid points [N,T,3]
};

// render_rays_kernel<MODE>: MODE_FULL is the fused canonical-space renderer.  With the SMPL inverse warp between the phases
// (a global closest-point search per sample: csrc/warp.hip) the same code is instantiated as its two halves:
// MODE_UPSAMPLE = coarse sdf at externally warped points + the NeuS up-sampling, writes z and the posed-space mid points;
// MODE_FINAL = render core at externally warped mid points, alpha multiplied by the mask.
enum { MODE_FULL = 0, MODE_UPSAMPLE = 2, MODE_FINAL = 3 };

// what the field code reads of the arguments: the table through a buffer descriptor (32-bit byte offsets, hardware bounds check), the gather modes, the bound
typedef __amdgpu_buffer_rsrc_t rsrc_t;
struct FieldCtx { rsrc_t table; int jmode[4]; int jfine[4]; float bound, two_bound, inv_tb; };
__device__ __forceinline__ rsrc_t table_of(const FieldCtx &fc) { return fc.table; }

__device__ __forceinline__ FieldCtx make_ctx(const RenderArgs &a)
{
    FieldCtx fc;
    fc.table = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.table), 0, a.table_bytes, 0x00020000);
    fc.jmode[0] = a.jmode[0]; fc.jmode[1] = a.jmode[1]; fc.jmode[2] = a.jmode[2]; fc.jmode[3] = a.jmode[3];
    fc.jfine[0] = a.jfine[0]; fc.jfine[1] = a.jfine[1]; fc.jfine[2] = a.jfine[2]; fc.jfine[3] = a.jfine[3];
    fc.bound = a.bound; fc.two_bound = a.two_bound; fc.inv_tb = a.inv_tb;
    return fc;
}

}  // namespace
