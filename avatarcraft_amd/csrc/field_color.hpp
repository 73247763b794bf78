// avatarcraft_amd/csrc/field_color.hpp -- what follows the SDF at a sample: the normal from the finite-difference gradient, the NeuS alpha, the view-direction
// bias of the colour network's layer 1 (per ray and per packed sample) and the colour network 21-64-64-3 on a tile, exact and in split bf16.
// Included by field_tile.hpp, color_train.hip and the two ray renderers.
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "field_lds.hpp"
#include "sdf_mlp.hpp"
#include "wave_ops.hpp"
#include "ac_sh16.hpp"

namespace {

// the normal from the finite-difference gradient: |g| (eikonal term) and g / (1e-5 + |g|)
struct FdNormal { float gn, nx, ny, nz; };
__device__ __forceinline__ FdNormal fd_normal(float gx, float gy, float gz)
{
    const float gn = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
    return FdNormal{ gn, gx / (1e-5f + gn), gy / (1e-5f + gn), gz / (1e-5f + gn) };
}

// NeuS alpha (instant_nsr.py:219-248) of a section of length delta at sdf value sdf0: tc = dot(ray direction, normal), inv_s = forward_variance()
__device__ __forceinline__ float neus_alpha(const float *__restrict__ lds, const RenderArgs &a, float tc, float sdf0, float delta, float inv_s)
{
    const float a1 = dv_softplus100(lds + OFF_SPQ, -tc * 0.5f + 0.5f) * a.one_m_car;
    const float a2 = dv_softplus100(lds + OFF_SPQ, -tc) * a.car;
    const float iter_cos = -(a1 + a2);
    const float half = iter_cos * delta * 0.5f;
    const float pc = dv_sigmoid((sdf0 - half) * inv_s), nc = dv_sigmoid((sdf0 + half) * inv_s);
    return clampf((pc - nc + 1e-5f) / (pc + 1e-5f), 0.0f, 1.0f);
}

// ---- forward_color for a tile: rgb (post-sigmoid) valid in lanes g==0 ---------------------------------
// ---- use_viewdirs = True (models/instant_nsr.py:565-569, 644-653): h = cat[x, sh(d), n, geo_feat] ----------------------------------------
// The 16 spherical harmonics (degree 4, encoder/shencoder) of the RAW ray direction enter layer 1 of the colour network only.  The direction is constant
// along a ray, so Wsh sh(d) is a per-ray BIAS of that layer: bias[u] = fma chain over j = 0..15 of Wsh[u][j] * sh_j(d), and the accumulator of unit u
// starts from bias[u] instead of 0 -- zero cost per sample.  sh_j: the value table of the stand-alone encoder (shencoder.hip), same operations.
// one ray per wave: shb [80] floats of the wave's LDS slab -> shb[u] = bias of unit u (u = lane); KEEP_SH: shb[64 + j] = sh_j(d) as well (ac_sh_bias)
template <bool KEEP_SH = false>
__device__ __forceinline__ void ray_sh_bias(float *__restrict__ shb, const float *__restrict__ Wsh, float dx, float dy, float dz, int lane)
{
    float sh[16];
    ac_sh16(dx, dy, dz, sh);                                  // (ac_sh16.hpp: the stand-alone encoder's operations, written out)
    const f32x4 *w = reinterpret_cast<const f32x4 *>(Wsh + lane * 16);
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 wv = w[q];
        acc = fma_(wv[0], sh[4 * q], acc); acc = fma_(wv[1], sh[4 * q + 1], acc);
        acc = fma_(wv[2], sh[4 * q + 2], acc); acc = fma_(wv[3], sh[4 * q + 3], acc);
    }
    wave_sync();                                              // (the previous work item's readers of the slab are done)
    shb[lane] = acc;
    if constexpr (KEEP_SH) {
#pragma unroll
        for (int j = 0; j < 16; ++j) if (lane == j) shb[64 + j] = sh[j];
    }
    wave_sync();
}
// packed samples (a tile of 16 samples of whatever rays): lane (n, g) computes the 16 biases it needs -- units 16 t + 4 g + r of ITS sample's direction --
// into slab[(t * 64 + lane) * 4 + r] ([4][64][4] floats of the wave's LDS: the finite-difference feature slab, free once the normals are formed)
__device__ __forceinline__ void sample_sh_bias(float *__restrict__ slab, const float *__restrict__ Wsh, float dx, float dy, float dz, int lane)
{
    const int g = lane >> 4;
    float sh[16];
    ac_sh16(dx, dy, dz, sh);
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 *w = reinterpret_cast<const f32x4 *>(Wsh + (16 * t + 4 * g + r) * 16);
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 wv = w[q];
                acc = fma_(wv[0], sh[4 * q], acc); acc = fma_(wv[1], sh[4 * q + 1], acc); acc = fma_(wv[2], sh[4 * q + 2], acc); acc = fma_(wv[3], sh[4 * q + 3], acc);
            }
            o[r] = acc;
        }
        *reinterpret_cast<f32x4 *>(slab + (t * 64 + lane) * 4) = o;
    }
    wave_sync();
}

// The view-direction bias of layer 1 enters unit u's fma chain at ONE fixed position: after the three coordinates, in the k = 3 slot of the MFMA that
// carries (x, y, z, -) -- a slot that multiplies 0 by 0 without view directions.  acc = fma(bias[u], 1, acc) there, in both forms:
//   shb1 (the renderer: one ray per wave): the ray's bias row [64] in the wave's slab becomes that slot's A operand on the lanes of group 3 (B = 1 there):
//        no extra instruction but a select -- the renderer's tile loop has neither registers nor issue slots to spare;
//   shb  (packed samples, a direction per sample): this lane's bias quadruples -- (sample slab) + 4 lane, tstride 256 -- added to the accumulator right
//        after that MFMA (acc + bias, one rounding: the same bits as the slot's fma).
__device__ __forceinline__ void color_tile(const float *__restrict__ lds, int lane, float px, float py, float pz,
                                           float nx, float ny, float nz, f32x4 sdfout, float (&rgb)[3], const float *__restrict__ shb = nullptr,
                                           int tstride = 16, const float *__restrict__ shb1 = nullptr)
{
    const int g = lane >> 4;
    f32x4 h1[4], h2[4];
    const float bxyz = sel4(g, px, py, pz, shb1 ? 1.0f : 0.0f), bn = sel4(g, nx, ny, nz, 0.0f);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const float b = s < 4 ? sdfout[s] : (s == 4 ? bxyz : bn);
            float wv = lds[OFF_C1F + (t * 6 + s) * 64 + lane];
            // the ray's bias row for the lanes of group 3 as a second, plainly addressed LDS read and a select of the VALUE (round 6: the address select this
            // replaces kept a per-lane pointer alive across the tile, which the register allocator answered with a scratch reload inside this block)
            if (s == 4 && shb1) { const float wb = shb1[16 * t + (lane & 15)]; wv = g == 3 ? wb : wv; }
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, b, acc, 0, 0, 0);
            if (s == 4 && shb) {
                const f32x4 bq = *reinterpret_cast<const f32x4 *>(shb + t * tstride);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = acc[r] + bq[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] > 0.0f ? acc[r] : 0.0f;
        h1[t] = acc;
    }
#pragma unroll
    for (int to = 0; to < 4; ++to) {
        f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_C2F + (to * 16 + kk) * 64 + lane], h1[kk >> 2][kk & 3], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] > 0.0f ? acc[r] : 0.0f;
        h2[to] = acc;
    }
    f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_C3F + kk * 64 + lane], h2[kk >> 2][kk & 3], acc, 0, 0, 0);
    rgb[0] = dv_sigmoid(acc[0]); rgb[1] = dv_sigmoid(acc[1]); rgb[2] = dv_sigmoid(acc[2]);
}

// the same network in split bf16 (fast precision; fragments of fill_lds_color_fast): 42 MFMA of 16 clocks instead of 104 of 32
__device__ __forceinline__ f32x4 cf_mma(const float *__restrict__ lds, int f, int lane, const u32x4 &bh, const u32x4 &bl, f32x4 acc)
{
    const bf16x8 Ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + OFF_CFH + (f * 64 + lane) * 4));
    const bf16x8 Al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + (f < 12 ? OFF_CFL + f * CF_FRAG : OFF_C3L + (f - 12) * CF_FRAG) + lane * 4));
    const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh), Bl = __builtin_bit_cast(bf16x8, bl);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, acc, 0, 0, 0);
}
__device__ __forceinline__ void color_tile_fast(const float *__restrict__ lds, int lane, float px, float py, float pz,
                                                float nx, float ny, float nz, f32x4 sdfout, float (&rgb)[3], const float *__restrict__ shb = nullptr,
                                                int tstride = 16, const float *__restrict__ shb1 = nullptr)
{
    const int g = lane >> 4;
    u32x4 bh, bl;
    {
        const float in[8] = { sdfout[0], sdfout[1], sdfout[2], sdfout[3], g == 0 ? px : (g == 1 ? nx : 0.0f), g == 0 ? py : (g == 1 ? ny : 0.0f),
                              g == 0 ? pz : (g == 1 ? nz : 0.0f), 0.0f };
        split8_bf16(in, bh, bl);
    }
    f32x4 h1[4], h2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x4 acc0 = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (shb) acc0 = *reinterpret_cast<const f32x4 *>(shb + t * tstride);      // (the view-direction bias stays fp32 in either precision)
        if (shb1) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(shb1[16 * t + (lane & 15)], g == 0 ? 1.0f : 0.0f, acc0, 0, 0, 0);
        f32x4 acc = cf_mma(lds, t, lane, bh, bl, acc0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] > 0.0f ? acc[r] : 0.0f;
        h1[t] = acc;
    }
    u32x4 ch[2], cl[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float in[8] = { h1[2 * s][0], h1[2 * s][1], h1[2 * s][2], h1[2 * s][3], h1[2 * s + 1][0], h1[2 * s + 1][1], h1[2 * s + 1][2], h1[2 * s + 1][3] };
        split8_bf16(in, ch[s], cl[s]);
    }
#pragma unroll
    for (int to = 0; to < 4; ++to) {
        f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = cf_mma(lds, 4 + 2 * to + s, lane, ch[s], cl[s], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] > 0.0f ? acc[r] : 0.0f;
        h2[to] = acc;
    }
    f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float in[8] = { h2[2 * s][0], h2[2 * s][1], h2[2 * s][2], h2[2 * s][3], h2[2 * s + 1][0], h2[2 * s + 1][1], h2[2 * s + 1][2], h2[2 * s + 1][3] };
        u32x4 dh, dl;
        split8_bf16(in, dh, dl);
        acc = cf_mma(lds, 12 + s, lane, dh, dl, acc);
    }
    rgb[0] = dv_sigmoid(acc[0]); rgb[1] = dv_sigmoid(acc[1]); rgb[2] = dv_sigmoid(acc[2]);
}

}  // namespace
