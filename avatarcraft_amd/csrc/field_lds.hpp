// avatarcraft_amd/csrc/field_lds.hpp -- the LDS image every kernel that evaluates the field shares: where the MFMA-ordered weight fragments, biases, level
// records, sampling tables and the softplus table sit (OFF_W1F .. OFF_WAVE), the fragments of the fast precision behind them, the size of a wave's
// finite-difference feature slab, and the workgroup prologues that lay the weights out (fill_lds_*).
// Included by hash_gather.hpp, field_color.hpp and render_slab.hpp, and through them by every file that evaluates the field.
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "field_args.hpp"
#include "ac_sp_table.hpp"

namespace {

// ---- LDS layout (floats) -------------------------------------------------------------------------
constexpr int OFF_W1F = 0;                       // [4 tiles][9 ksteps][64]
constexpr int OFF_W2F = OFF_W1F + 4 * 9 * 64;    // [16 ksteps][64]
constexpr int OFF_C1F = OFF_W2F + 16 * 64;       // [4][6][64]
constexpr int OFF_C2F = OFF_C1F + 4 * 6 * 64;    // [4][16][64]
constexpr int OFF_C3F = OFF_C2F + 4 * 16 * 64;   // [16][64]
constexpr int OFF_B1 = OFF_C3F + 16 * 64;        // [64]
constexpr int OFF_B2 = OFF_B1 + 64;              // [16]
constexpr int OFF_LVL = OFF_B2 + 16;             // [16 levels][8 words]
constexpr int OFF_LIN = OFF_LVL + 16 * 8;        // lin_z[64] + lin_u[16]
constexpr int OFF_SPQ = OFF_LIN + 80;
constexpr int OFF_WAVE = OFF_SPQ + SPQ_FLOATS;        // end of the weights every kernel shares; per-wave slabs of the training kernels start here
constexpr int FE_SLAB = 6 * 8 * 64;                        // hash features of the 6 finite-difference points: [e-1][2j+c][lane]
// the renderer only: layer 1 of sdf_net for the "fast" precision (ac_render_opts.precision = 1) -- the 32 feature columns of W1 split into
// bf16 hi + lo in the A-fragment order of v_mfma_f32_16x16x32_bf16 (lane (unit m, group kk) holds k = 8 kk .. 8 kk + 7 = the eight
// features lane group kk gathers: 16 bytes per lane and tile), and the three coordinate columns as plain fp32
constexpr int OFF_W1H = OFF_WAVE;                // [4 tiles][64 lanes][4 dwords]
constexpr int OFF_W1L = OFF_W1H + 4 * 64 * 4;
constexpr int OFF_W1C = OFF_W1L + 4 * 64 * 4;    // [3 axes][64 units]
// ... and the colour network in split bf16 (fast precision): 14 A-fragments [64 lanes][4 dwords] (layer 1: 4 output tiles; layer 2: 4 tiles x 2 k-steps
// of 32; layer 3: 2 k-steps), hi and lo parts.  They OVERLAY the fp32 colour fragments [OFF_C1F, OFF_B1) -- 14 hi + the first 12 lo fill it exactly --
// and the last two lo fragments (layer 3) sit behind W1C.
constexpr int CF_FRAGS = 14, CF_FRAG = 64 * 4;
constexpr int OFF_CFH = OFF_C1F;                            // hi fragments 0..13
constexpr int OFF_CFL = OFF_C1F + CF_FRAGS * CF_FRAG;       // lo fragments 0..11
constexpr int OFF_C3L = OFF_W1C + 3 * 64;                   // lo fragments 12, 13
static_assert(OFF_CFL + 12 * CF_FRAG == OFF_B1, "the bf16 colour fragments fill the fp32 colour region exactly");

// ---- workgroup prologue: weights -> MFMA A-fragment order in LDS -------------------------------------
// the SDF side (sdf_net fragments, biases, level records, sampling tables, softplus table) and the colour side are laid out separately: the
// SDF-query training kernels never touch the colour fragments and use their 26 KB for their own
__device__ __forceinline__ void fill_lds_sdf(float *lds, const RenderArgs &a)
{
    for (int e = threadIdx.x; e < 4 * 9 * 64; e += blockDim.x) {          // sdf_net.0 [64,35]
        int l = e & 63, fs = e >> 6, t = fs / 9, s = fs % 9;
        int u = 16 * t + (l & 15), g = l >> 4;
        int col = (s == 0) ? (g < 3 ? g : -1) : 3 + 2 * (4 * ((s - 1) >> 1) + g) + ((s - 1) & 1);
        lds[OFF_W1F + e] = col < 0 ? 0.0f : a.W1[u * 35 + col];
    }
    for (int e = threadIdx.x; e < 16 * 64; e += blockDim.x) {             // sdf_net.1 [16,64]
        int l = e & 63, kk = e >> 6, t = kk >> 2, r = kk & 3;
        lds[OFF_W2F + e] = a.W2[(l & 15) * 64 + 16 * t + 4 * (l >> 4) + r];
    }
    for (int e = threadIdx.x; e < 64; e += blockDim.x) lds[OFF_B1 + e] = a.b1[e];
    for (int e = threadIdx.x; e < 16; e += blockDim.x) lds[OFF_B2 + e] = a.b2[e];
    {   // level records: static kernarg indexing only (a dynamic index would copy the struct to scratch)
        uint32_t *lw = reinterpret_cast<uint32_t *>(lds) + OFF_LVL;
#pragma unroll
        for (int l = 0; l < 16; ++l) {
            if (threadIdx.x == (unsigned)l) {
                lw[8 * l + 0] = __float_as_uint(a.lvl[l].scale); lw[8 * l + 1] = a.lvl[l].my;
                lw[8 * l + 2] = a.lvl[l].mz; lw[8 * l + 3] = a.lvl[l].offset;
                lw[8 * l + 4] = a.lvl[l].mask; lw[8 * l + 5] = a.lvl[l].hashed;
                lw[8 * l + 6] = a.lvl[l].wsize; lw[8 * l + 7] = 0u;
            }
        }
    }
    for (int e = threadIdx.x; e < 64; e += blockDim.x) lds[OFF_LIN + e] = e < a.T0 ? a.lin_z[e] : 0.0f;
    for (int e = threadIdx.x; e < 16; e += blockDim.x) lds[OFF_LIN + 64 + e] = a.lin_u ? a.lin_u[e] : 0.0f;
    for (int e = threadIdx.x; e < SPQ_FLOATS; e += blockDim.x) lds[OFF_SPQ + e] = AC_SP_G[e >> 2][e & 3];
}

__device__ __forceinline__ void fill_lds_color(float *lds, const RenderArgs &a)
{
    for (int e = threadIdx.x; e < 4 * 6 * 64; e += blockDim.x) {          // color_net.0 [64,21] = [x(3), n(3), feat(15)]
        int l = e & 63, fs = e >> 6, t = fs / 6, s = fs % 6;
        int u = 16 * t + (l & 15), g = l >> 4;
        float v;
        if (s < 4) { int o = 4 * g + s; v = (o == 0) ? 0.0f : a.Wc1[u * 21 + 6 + (o - 1)]; }
        else if (s == 4) v = g < 3 ? a.Wc1[u * 21 + g] : 0.0f;
        else v = g < 3 ? a.Wc1[u * 21 + 3 + g] : 0.0f;
        lds[OFF_C1F + e] = v;
    }
    for (int e = threadIdx.x; e < 4 * 16 * 64; e += blockDim.x) {         // color_net.1 [64,64]
        int l = e & 63, fs = e >> 6, to = fs >> 4, kk = fs & 15, t = kk >> 2, r = kk & 3;
        lds[OFF_C2F + e] = a.Wc2[(16 * to + (l & 15)) * 64 + 16 * t + 4 * (l >> 4) + r];
    }
    for (int e = threadIdx.x; e < 16 * 64; e += blockDim.x) {             // color_net.2 [3,64]
        int l = e & 63, kk = e >> 6, t = kk >> 2, r = kk & 3, o = l & 15;
        lds[OFF_C3F + e] = o < 3 ? a.Wc3[o * 64 + 16 * t + 4 * (l >> 4) + r] : 0.0f;
    }
}

__device__ __forceinline__ void fill_lds(float *lds, const RenderArgs &a)
{
    fill_lds_sdf(lds, a);
    fill_lds_color(lds, a);
}

// ---- "fast" precision: bf16 hi / lo fragments of W1's feature columns, fp32 coordinate columns ----------
__device__ __forceinline__ uint32_t bf16_rne_bits(float f)       // finite inputs (weights): round to nearest even
{
    const uint32_t u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
template <int W1H = OFF_W1H, int W1L = OFF_W1L, int W1C = OFF_W1C>
__device__ __forceinline__ void fill_lds_fast(float *lds, const RenderArgs &a)
{
    uint32_t *lw = reinterpret_cast<uint32_t *>(lds);
    for (int e = threadIdx.x; e < 4 * 64 * 4; e += blockDim.x) {          // dword q of lane l, tile t: slots i = 2q, 2q + 1 of lane group kk
        const int q = e & 3, l = (e >> 2) & 63, t = e >> 8;
        const int u = 16 * t + (l & 15), kk = l >> 4;
        uint32_t hi2 = 0, lo2 = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 2 * q + h;                                      // feature slot 2 j + c of lane group kk = level 4 j + kk, channel c
            const float w = a.W1[u * 35 + 3 + 2 * (4 * (i >> 1) + kk) + (i & 1)];
            const uint32_t hb = bf16_rne_bits(w);
            const uint32_t lb = bf16_rne_bits(w - __uint_as_float(hb << 16));
            hi2 |= hb << (16 * h); lo2 |= lb << (16 * h);
        }
        lw[W1H + e] = hi2; lw[W1L + e] = lo2;
    }
    for (int e = threadIdx.x; e < 3 * 64; e += blockDim.x) lds[W1C + e] = a.W1[(e & 63) * 35 + (e >> 6)];
}

// colour network, fast precision.  B operand of v_mfma_f32_16x16x32_bf16: lane (sample n, group g) supplies k = 8g .. 8g+7; the eight slots of a lane
// are values it already holds, so no data moves between lanes:
//   layer 1: slots 0..3 = sdf_out[4g + i] (the SDF network's output rows of this lane; row 0, the sdf itself, gets weight 0), slots 4..6 = x (g = 0) or
//            the normal (g = 1), everything else 0;
//   layer 2 / 3, k-step s: slots i = the lane's rows r = i & 3 of the previous layer's output tiles 2s + (i >> 2), i.e. units 16 (2s + (i >> 2)) + 4g + r.
// The weights (A operand, lane (row m, group g)) are permuted to match and split hi + lo by round-to-nearest; the activations are split by
// truncation (split8_bf16); three of the four partial products are formed.  Weight of fragment f, lane l, slot i:
__device__ __forceinline__ float color_fast_weight(const RenderArgs &a, int f, int l, int i)
{
    const int m = l & 15, g = l >> 4;
    if (f < 4) {                                                          // layer 1, output tile f
        const int u = 16 * f + m;
        if (i < 4) { const int o = 4 * g + i; return o == 0 ? 0.0f : a.Wc1[u * 21 + 5 + o]; }
        if (i < 7 && g < 2) return a.Wc1[u * 21 + 3 * g + (i - 4)];
        return 0.0f;
    }
    const int s = (f - 4) & 1, unit = 16 * (2 * s + (i >> 2)) + 4 * g + (i & 3);
    if (f < 12) return a.Wc2[(16 * ((f - 4) >> 1) + m) * 64 + unit];    // layer 2, output tile (f - 4) / 2, k-step s
    return m < 3 ? a.Wc3[m * 64 + unit] : 0.0f;                           // layer 3, k-step s
}
template <bool OVERLAY, bool TAIL>
__device__ __forceinline__ void fill_lds_color_fast(float *lds, const RenderArgs &a)
{
    uint32_t *lw = reinterpret_cast<uint32_t *>(lds);
    for (int e = threadIdx.x; e < CF_FRAGS * CF_FRAG; e += blockDim.x) {
        const int q = e & 3, l = (e >> 2) & 63, f = e >> 8;
        if (!(f < 12 ? OVERLAY : (OVERLAY || TAIL))) continue;
        uint32_t hi2 = 0, lo2 = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float w = color_fast_weight(a, f, l, 2 * q + h);
            const uint32_t hb = bf16_rne_bits(w);
            const uint32_t lb = bf16_rne_bits(w - __uint_as_float(hb << 16));
            hi2 |= hb << (16 * h); lo2 |= lb << (16 * h);
        }
        if (OVERLAY) lw[OFF_CFH + e] = hi2;
        if (f < 12) { if (OVERLAY) lw[OFF_CFL + e] = lo2; }
        else if (TAIL) lw[OFF_C3L + (e - 12 * CF_FRAG)] = lo2;
    }
}

}  // namespace
