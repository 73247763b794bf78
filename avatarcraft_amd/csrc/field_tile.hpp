// avatarcraft_amd/csrc/field_tile.hpp -- the field on a tile of 16 packed samples: the workgroup shape and LDS image of the forward SDF query, the
// seven-evaluation stencil (fd_forward) and the whole per-sample body (field_tile: stencil, normal, colour, NeuS alpha).
// Included by sdf_stencil_train.hip, render_occupancy.hip and shade_tile.hpp (mesh_shade.hip, mesh_occlusion.hip, surface_rays.hip).
// Anonymous namespace, like the field headers it includes: each translation unit gets its own copy.
#pragma once
#include "sdf_mlp.hpp"
#include "field_stencil.hpp"
#include "field_color.hpp"

namespace {

constexpr int FW = 8;                              // waves per workgroup of the forward SDF query (224 VGPRs: two waves per SIMD, like the renderer)
constexpr int FBLOCK = FW * 64;
constexpr int FWD_LDS_FLOATS = OFF_WAVE + FW * FE_SLAB;
static_assert(FWD_LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");

// the 7 evaluations of one tile: centre outputs (o = 4g + r) and the finite-difference gradient (the same in all four lanes of a sample)
// (the renderers' exact stencil; they keep their own copy inline, because one helper shared with them changes the generated code)
__device__ __forceinline__ void fd_forward(const float *__restrict__ lds, const float *__restrict__ fsl, int lane, float px, float py, float pz,
                                           float eps, float bound, const float (&fe0)[4][2], f32x4 &oc, float (&gr)[3])
{
    const int g = lane >> 4;
    const float pc0 = sel4(g, px, py, pz, 0.0f);
    oc = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    gr[0] = gr[1] = gr[2] = 0.0f;
    float spos = 0.0f;
    const W2Row0 w2r0 = load_w2_row0(lds, lane);
    Acc4 acc = sdf_l1(lds, lane, pc0, fe0);
#pragma unroll 1
    for (int e = 0; e < 7; ++e) {
        Acc4 accn = acc;
        if (e < 6) {                                               // layer 1 of the next evaluation
            const int kn = e >> 1;
            float fe[4][2];
#pragma unroll
            for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fsl[(e * 8 + q_) * 64 + lane];
            const float pk = kn == 0 ? px : (kn == 1 ? py : pz);
            const float poff = clampf(pk + ((e & 1) ? -eps : eps), -bound, bound);
            accn = sdf_l1(lds, lane, g == kn ? poff : pc0, fe);
        }
        if (e == 0) oc = sdf_l2(lds, lane, acc);                   // the centre: all 16 outputs
        else {                                                     // the six offset points: the sdf alone (same arithmetic as the renderer)
            const float s_e = sdf_l2_sdf(lds, acc, w2r0);
            const int k = (e - 1) >> 1;
            if (e & 1) spos = s_e;
            else {
                const float gk = 0.5f * (spos - s_e) / eps;
                if (k == 0) gr[0] = gk; else if (k == 1) gr[1] = gk; else gr[2] = gk;
            }
        }
        acc = accn;
    }
}

// One tile of 16 packed samples of whatever rays through the final pass of render_rays_kernel (render_fused.hip): the stencil gather at the clamped point
// (new_pts.clamp(-bound, bound)), the seven SDF MLP passes, the normal, the colour tile (use_viewdirs: on the layer-1 bias of THIS sample's direction, a
// wave-uniform branch) and the cos-annealed NeuS alpha (instant_nsr.py:219-243) with the marcher's step `delta` as the section length -- a sample gets the
// bits here that it would get there for the same point, direction and section length.  Lane (n, g) handles sample n; rgb is valid in the lanes g == 0.
//   in : (sx, sy, sz) the marcher's point, unclamped | (dx, dy, dz) its ray's direction | delta | inv_s
//   out: alpha, rgb, normal | sdf0 = the centre's output 0 | gr = the raw finite-difference gradient, gn = its length (eikonal term)
// fsl, the wave's feature slab, is rewritten twice (features, then the direction biases); every lane must be past its reads of the previous tile on entry:
// the callers' wave_sync() at the end of a tile.
__device__ __forceinline__ void field_tile(const float *__restrict__ lds, float *__restrict__ fsl, const FieldCtx &fc, const RenderArgs &a, int lane,
                                           float sx, float sy, float sz, float dx, float dy, float dz, float delta, float inv_s,
                                           float &alpha, float (&rgb)[3], float (&nrm)[3], float &sdf0, float (&gr)[3], float &gn)
{
    const float bound = a.bound, eps = a.eps;
    const float px = clampf(sx, -bound, bound), py = clampf(sy, -bound, bound), pz = clampf(sz, -bound, bound);
    float fe0[4][2];
    encode_stencil(lds, fsl, fc, lane, px, py, pz, eps, fe0);
    f32x4 o16;
    fd_forward(lds, fsl, lane, px, py, pz, eps, bound, fe0, o16, gr);
    const FdNormal fn = fd_normal(gr[0], gr[1], gr[2]);
    gn = fn.gn; nrm[0] = fn.nx; nrm[1] = fn.ny; nrm[2] = fn.nz;
    if (a.Wsh) {
        wave_sync();                                                 // (every lane is done with the feature slab)
        sample_sh_bias(fsl, a.Wsh, dx, dy, dz, lane);
        color_tile(lds, lane, px, py, pz, fn.nx, fn.ny, fn.nz, o16, rgb, fsl + 4 * lane, 256);
    } else color_tile(lds, lane, px, py, pz, fn.nx, fn.ny, fn.nz, o16, rgb);
    sdf0 = o16[0];
    alpha = neus_alpha(lds, a, (dx * fn.nx + dy * fn.ny) + dz * fn.nz, sdf0, delta, inv_s);
}

}  // namespace
