// avatarcraft_amd/csrc/color_train.hip -- the colour network of the differentiable render core (training path), forward and backward, and the per-ray
// view-direction bias of its first layer (ac_sh_bias).
//
// colour MLP of the render core (forward_color, models/instant_nsr.py:644-663, use_viewdirs = False):
//   rgb = sigmoid(Wc3 relu(Wc2 relu(Wc1 [x(3), normal(3), feat(15)])))            (no biases, weight-normed matrices)
// forward = the renderer's colour tile; backward recomputes it and runs all six products on the matrix pipe:
//   dh2 = Wc3^T do3 (4 MFMA), dh1 = Wc2^T dh2 (64), dinp = Wc1^T dh1 (32; lane (n, g) receives d sdf_out[4g..4g+3] and d normal_g:
//   exactly the layouts sdf_stencil_bwd_kernel and the caller read), dWc3 += do3 h2^T (16), dWc2 += dh2 h1^T (64),
//   dWc1 += dh1 inp^T (32) with K = the 16 samples of the tile through LDS transposes.
// Since round 4, layer 3 of the forward recomputation and the two data-gradient products (dh1 = Wc2^T dh2, dinp = Wc1^T dh1) run as three-term bf16
// splits instead of fp32 MFMA.  Layers 1 and 2 of the recomputation stay fp32: they decide the ReLU masks, and a recomputation that is only 2^-16
// accurate flips enough of them to show (dWc1 3e-3 of max against the fp64 oracle, measured); the weight gradients (K = the tile's samples, through
// LDS) stay fp32 as well
#include "train_common.hpp"
#include "field_color.hpp"
#include "field_host.hpp"

namespace {

// layer 3 of the forward: its two bf16 hi and two lo fragments (k blocks 0, 1; order of color_fast_weight) take the place of the fp32 ones
constexpr int OFF_C3H = OFF_C3F, OFF_C3LO = OFF_C3F + 2 * 64 * 4;
constexpr int OFF_C3T = OFF_WAVE;                  // [4 tiles][64]                       fp32 A fragments of Wc3^T (4 MFMA: not worth splitting)
constexpr int OFF_C2T = OFF_C3T + 4 * 64;          // [4 tiles][2 k blocks][64][4] hi | lo   Wc2^T, v_mfma_f32_16x16x32_bf16 order
constexpr int OFF_C2TL = OFF_C2T + 8 * 64 * 4;
constexpr int OFF_C1T = OFF_C2TL + 8 * 64 * 4;     // [2 tiles][2 k blocks][64][4] hi | lo   Wc1^T (rows: sdf_out[16] | normal, coordinate)
constexpr int OFF_C1TL = OFF_C1T + 4 * 64 * 4;
constexpr int OFF_CW = OFF_C1TL + 4 * 64 * 4;      // per-wave slabs
constexpr int CS_H1 = 0, CS_H2 = 64 * TLD, CS_D1 = 128 * TLD, CS_D2 = 192 * TLD, CS_O3 = 256 * TLD, CS_IN = 272 * TLD;
constexpr int COLOR_SLAB = ((CS_IN + 32 * TLD + 3) / 4) * 4;
constexpr int CBWD_LDS_FLOATS = OFF_CW + TW * COLOR_SLAB;
static_assert(CBWD_LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
constexpr int NPART_C = 64 * 32 + 64 * 64 + 16 * 64;     // dWc1 [64][32] (columns 0..20 = x, n, feat) | dWc2 [64][64] | dWc3 [16][64] (rows 0..2)

__global__ __launch_bounds__(TBLOCK) void color_fwd_kernel(const RenderArgs a, const float *__restrict__ x, const float *__restrict__ nrm,
                                                           const float *__restrict__ sdf16, uint32_t B, float *__restrict__ rgb_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const uint32_t ntiles = (B + 15) / 16;
    for (uint32_t tile = blockIdx.x * TW + wave; tile < ntiles; tile += gridDim.x * TW) {
        const uint32_t b = tile * 16 + n, bb = b < B ? b : B - 1;
        const f32x4 so = *reinterpret_cast<const f32x4 *>(sdf16 + (size_t)bb * 16 + 4 * g);
        float rgb[3];
        color_tile(lds, lane, x[3 * (size_t)bb], x[3 * (size_t)bb + 1], x[3 * (size_t)bb + 2], nrm[3 * (size_t)bb], nrm[3 * (size_t)bb + 1],
                   nrm[3 * (size_t)bb + 2], so, rgb);
        if (b < B && g == 0) { rgb_out[3 * (size_t)b] = rgb[0]; rgb_out[3 * (size_t)b + 1] = rgb[1]; rgb_out[3 * (size_t)b + 2] = rgb[2]; }
    }
}

__device__ __forceinline__ void fill_lds_color_bwd(float *lds, const RenderArgs &a)
{
    for (int e = threadIdx.x; e < 4 * 64; e += blockDim.x) {        // fragment to: lane (m, kk) = Wc3[o = kk][unit = 16 to + m]
        const int l = e & 63, to = e >> 6, m = l & 15, kk = l >> 4;
        lds[OFF_C3T + e] = kk < 3 ? a.Wc3[kk * 64 + 16 * to + m] : 0.0f;
    }
    // K order of both products = the register layout the previous product leaves its result in (slot i of lane group kk in k block s = unit
    // 16 (2s + (i >> 2)) + 4 kk + (i & 3)): no data moves between lanes.  Weights split hi + lo by round-to-nearest like fill_lds_color_fast.
    uint32_t *lw = reinterpret_cast<uint32_t *>(lds);
    for (int e = threadIdx.x; e < (8 + 4) * 64 * 4; e += blockDim.x) {
        const int q = e & 3, l = (e >> 2) & 63, f = e >> 8, m = l & 15, kk = l >> 4;
        const bool c2 = f < 8;
        const int t = c2 ? f >> 1 : (f - 8) >> 1, sblk = f & 1;
        int col = -1;                                                 // Wc1^T rows: tile 0 row m = sdf_out[m] (feat m - 1; the sdf itself is no input), tile 1 row 4 g = normal component g
        if (!c2) { if (t == 0) col = m == 0 ? -1 : 6 + (m - 1); else if ((m & 3) == 0 && (m >> 2) < 3) col = 3 + (m >> 2); }
        uint32_t hi2 = 0, lo2 = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 2 * q + h, unit = 16 * (2 * sblk + (i >> 2)) + 4 * kk + (i & 3);
            const float w = c2 ? a.Wc2[unit * 64 + 16 * t + m] : (col < 0 ? 0.0f : a.Wc1[unit * 21 + col]);
            const uint32_t hb = bf16_rne_bits(w), lb = bf16_rne_bits(w - __uint_as_float(hb << 16));
            hi2 |= hb << (16 * h); lo2 |= lb << (16 * h);
        }
        if (c2) { lw[OFF_C2T + e] = hi2; lw[OFF_C2TL + e] = lo2; }
        else { lw[OFF_C1T + (e - 8 * 256)] = hi2; lw[OFF_C1TL + (e - 8 * 256)] = lo2; }
    }
    for (int e = threadIdx.x; e < 2 * 64 * 4; e += blockDim.x) {      // layer 3 of the forward, k blocks 0 and 1 (rows 3 .. 15 zero)
        const int q = e & 3, l = (e >> 2) & 63, sblk = e >> 8;
        uint32_t hi2 = 0, lo2 = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float w = color_fast_weight(a, 12 + sblk, l, 2 * q + h);
            const uint32_t hb = bf16_rne_bits(w), lb = bf16_rne_bits(w - __uint_as_float(hb << 16));
            hi2 |= hb << (16 * h); lo2 |= lb << (16 * h);
        }
        lw[OFF_C3H + e] = hi2; lw[OFF_C3LO + e] = lo2;
    }
}

// acc += A (bf16 hi + lo fragment pair at hi_off / lo_off, fragment f) x B (split activations): three of the four partial products
__device__ __forceinline__ f32x4 cb_mma(const float *__restrict__ lds, int hi_off, int lo_off, int f, int lane, const u32x4 &bh, const u32x4 &bl, f32x4 acc)
{
    const bf16x8 Ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + hi_off + (f * 64 + lane) * 4));
    const bf16x8 Al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + lo_off + (f * 64 + lane) * 4));
    const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh), Bl = __builtin_bit_cast(bf16x8, bl);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, acc, 0, 0, 0);
}
// 8 fp32 values -> bf16 hi and lo parts, both ROUNDED to nearest (v_cvt_pk_bf16_f32, two values per instruction): |x - hi - lo| <= 2^-17 |x| and the
// dropped lo x lo term has either sign.  The renderer's split8_bf16 truncates both parts (2^-14, biased towards zero): good enough for an image, but
// through the five chained products of this kernel the bias showed as 6.5e-4 of max in dWc1 against the fp64 oracle (contract 3e-4); rounded: where the
// fp32 products were.  Same packing (value 2q in the low half of dword q), same instruction count.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split8_bf16_rn(const float (&d)[8], u32x4 &bh, u32x4 &bl)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2_t v = { d[2 * q], d[2 * q + 1] };
        const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
        const f32x2_t r = { d[2 * q] - __uint_as_float(hb << 16), d[2 * q + 1] - __uint_as_float(hb & 0xffff0000u) };
        bh[q] = hb;
        bl[q] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2_t));
    }
}
__device__ __forceinline__ void split_tiles(const f32x4 (&v)[4], u32x4 (&bh)[2], u32x4 (&bl)[2])
{
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const float in[8] = { v[2 * sb][0], v[2 * sb][1], v[2 * sb][2], v[2 * sb][3], v[2 * sb + 1][0], v[2 * sb + 1][1], v[2 * sb + 1][2], v[2 * sb + 1][3] };
        split8_bf16_rn(in, bh[sb], bl[sb]);
    }
}

// use_viewdirs (sh_bias != NULL): sample b belongs to ray b / T (T a multiple of 16: a tile never straddles two rays); layer 1 of the recomputed forward
// starts from the ray's bias sh_bias[ray][64] (ac_sh_bias: the forward's own bits, so the ReLU masks are the forward's), and the gradient of that bias --
// the tile's sum over its 16 samples of d h1 -- goes to g_sh_tiles[tile][64]: d Wc1_sh = sum over rays of (sum of the ray's tiles) (x) sh(d_ray) is formed by
// the caller (a [N, 64]^T x [N, 16] product: the direction is constant along a ray, there is nothing per sample to multiply).
__global__ __launch_bounds__(TBLOCK) void color_bwd_kernel(const RenderArgs a, const float *__restrict__ x, const float *__restrict__ nrm,
                                                           const float *__restrict__ sdf16, const float *__restrict__ g_rgb, uint32_t B,
                                                           float *__restrict__ g_nrm, float *__restrict__ g_sdf16, float *__restrict__ partials,
                                                           const float *__restrict__ sh_bias, uint32_t T, float *__restrict__ g_sh_tiles)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    __syncthreads();                                  // (the bf16 fragments of layer 3 overwrite the fp32 ones fill_lds has just written)
    fill_lds_color_bwd(lds, a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *slab = lds + OFF_CW + wave * COLOR_SLAB;
    float *TH1 = slab + CS_H1, *TH2 = slab + CS_H2, *TD1 = slab + CS_D1, *TD2 = slab + CS_D2, *TO3 = slab + CS_O3, *TIN = slab + CS_IN;
    for (int e = lane; e < 16 * TLD; e += 64) TO3[e] = 0.0f;          // rows 3..15 stay zero
    for (int e = lane; e < 32 * TLD; e += 64) TIN[e] = 0.0f;          // rows 21..31 stay zero
    __syncthreads();
    f32x4 gW1[4][2], gW2[4][4], gW3[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        gW3[t] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int c = 0; c < 2; ++c) gW1[t][c] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int c = 0; c < 4; ++c) gW2[t][c] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    }
    const uint32_t ntiles = (B + 15) / 16;
    // like sdf_stencil_bwd_kernel: the next tile's inputs are requested while this one is computed (one wave per SIMD: nothing else covers the loads)
    struct TileIn { float p[3], nr[3], up[3]; f32x4 so; };
    auto request = [&](uint32_t tile, TileIn &in) {
        const uint32_t b = tile * 16 + n, bb = b < B ? b : B - 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            in.p[k] = x[3 * (size_t)bb + k]; in.nr[k] = nrm[3 * (size_t)bb + k];
            in.up[k] = (b < B && g == 0) ? g_rgb[3 * (size_t)bb + k] : 0.0f;
        }
        in.so = *reinterpret_cast<const f32x4 *>(sdf16 + (size_t)bb * 16 + 4 * g);
    };
    const uint32_t tile0 = blockIdx.x * TW + wave, tstride = gridDim.x * TW;
    TileIn nxt;
    if (tile0 < ntiles) request(tile0, nxt);
    for (uint32_t tile = tile0; tile < ntiles; tile += tstride) {
        const uint32_t b = tile * 16 + n;
        const bool live = b < B;
        const float px = nxt.p[0], py = nxt.p[1], pz = nxt.p[2];
        const float nx = nxt.nr[0], ny = nxt.nr[1], nz = nxt.nr[2];
        const float ups[3] = { nxt.up[0], nxt.up[1], nxt.up[2] };
        const f32x4 so = nxt.so;
        if (tile + tstride < ntiles) request(tile + tstride, nxt);
        const float bxyz = sel4(g, px, py, pz, 0.0f), bn = sel4(g, nx, ny, nz, 0.0f);
        // forward recompute, activations kept: layers 1 and 2 with the instruction sequence of color_tile (fp32: the ReLU masks are the forward's own)
        f32x4 h1[4], h2[4];
        const float *const shb = sh_bias ? sh_bias + (size_t)((tile * 16u) / T) * 64 + 4 * g : nullptr;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const float bv = s < 4 ? so[s] : (s == 4 ? bxyz : bn);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_C1F + (t * 6 + s) * 64 + lane], bv, acc, 0, 0, 0);
                if (s == 4 && shb) {                             // the view-direction bias: the forward's position in the chain (color_tile)
                    const f32x4 bq = *reinterpret_cast<const f32x4 *>(shb + 16 * t);
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
        f32x4 o3 = { 0.0f, 0.0f, 0.0f, 0.0f };
        {
            u32x4 ch[2], cl[2];
            split_tiles(h2, ch, cl);
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) o3 = cb_mma(lds, OFF_C3H, OFF_C3LO, sb, lane, ch[sb], cl[sb], o3);
        }
        // d o3 = d rgb * rgb (1 - rgb), held by the lanes g == 0 (o = r); broadcast to lane group kk = o as the B operand of Wc3^T
        float d3[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const float rgb = dv_sigmoid(o3[o]);
            const float up = ups[o];
            d3[o] = up * (rgb * (1.0f - rgb));
        }
        const float s0 = __shfl(d3[0], n), s1 = __shfl(d3[1], n), s2 = __shfl(d3[2], n);
        const float b3 = g == 0 ? s0 : (g == 1 ? s1 : (g == 2 ? s2 : 0.0f));
        // dh2 = Wc3^T d3 (.) [h2 > 0]; dh1 = Wc2^T dh2 (.) [h1 > 0]
        f32x4 dh2[4], dh1[4];
#pragma unroll
        for (int to = 0; to < 4; ++to) {
            f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_C3T + to * 64 + lane], b3, acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = h2[to][r] > 0.0f ? acc[r] : 0.0f;
            dh2[to] = acc;
        }
        u32x4 gbh[2], gbl[2];
        split_tiles(dh2, gbh, gbl);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) acc = cb_mma(lds, OFF_C2T, OFF_C2TL, 2 * t + sb, lane, gbh[sb], gbl[sb], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = h1[t][r] > 0.0f ? acc[r] : 0.0f;
            dh1[t] = acc;
        }
        if (g_sh_tiles) {                                            // d bias of this tile: row sums over the 16 samples (dead samples of a ragged last tile: d h1 = 0, their upstream is 0)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x4 sm;
#pragma unroll
                for (int r = 0; r < 4; ++r) sm[r] = row_scan<false>(dh1[t][r]);
                if (n == 15) *reinterpret_cast<f32x4 *>(g_sh_tiles + (size_t)tile * 64 + 16 * t + 4 * g) = sm;
            }
        }
        split_tiles(dh1, gbh, gbl);
        // dinp = Wc1^T dh1: tile 0 -> d sdf_out[4g + r], tile 1 reg 0 -> d normal_g
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
            f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) acc = cb_mma(lds, OFF_C1T, OFF_C1TL, 2 * tp + sb, lane, gbh[sb], gbl[sb], acc);
            if (live) {
                if (tp == 0) *reinterpret_cast<f32x4 *>(g_sdf16 + (size_t)b * 16 + 4 * g) = acc;
                else if (g < 3) g_nrm[3 * (size_t)b + g] = acc[0];
            }
        }
        // weight gradients (K = the tile's 16 samples)
        if (g == 0) { TO3[0 * TLD + n] = d3[0]; TO3[1 * TLD + n] = d3[1]; TO3[2 * TLD + n] = d3[2]; }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = (16 * t + 4 * g + r) * TLD + n;
                TH1[u] = h1[t][r]; TH2[u] = h2[t][r]; TD1[u] = dh1[t][r]; TD2[u] = dh2[t][r];
            }
        // inputs in the column order of Wc1: x (0..2), normal (3..5), feat (6..20) = sdf_out[1..15]
        if (g < 3) { TIN[g * TLD + n] = bxyz; TIN[(3 + g) * TLD + n] = bn; }
#pragma unroll
        for (int s = 0; s < 4; ++s) { const int o = 4 * g + s; if (o > 0) TIN[(6 + o - 1) * TLD + n] = so[s]; }
        wave_sync();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a3 = TO3[n * TLD + 4 * s + g];
            float bh2[4], bh1[4], bin[2];
#pragma unroll
            for (int c = 0; c < 4; ++c) { bh2[c] = TH2[(16 * c + n) * TLD + 4 * s + g]; bh1[c] = TH1[(16 * c + n) * TLD + 4 * s + g]; }
#pragma unroll
            for (int c = 0; c < 2; ++c) bin[c] = TIN[(16 * c + n) * TLD + 4 * s + g];
#pragma unroll
            for (int c = 0; c < 4; ++c) gW3[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, bh2[c], gW3[c], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float a2 = TD2[(16 * t + n) * TLD + 4 * s + g], a1 = TD1[(16 * t + n) * TLD + 4 * s + g];
#pragma unroll
                for (int c = 0; c < 4; ++c) gW2[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bh1[c], gW2[t][c], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < 2; ++c) gW1[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bin[c], gW1[t][c], 0, 0, 0);
            }
        }
        wave_sync();
    }
    float *part = partials + (size_t)(blockIdx.x * TW + wave) * NPART_C;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * g + r;
#pragma unroll
            for (int c = 0; c < 2; ++c) part[row * 32 + 16 * c + n] = gW1[t][c][r];
#pragma unroll
            for (int c = 0; c < 4; ++c) part[64 * 32 + row * 64 + 16 * c + n] = gW2[t][c][r];
        }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[64 * 32 + 64 * 64 + (4 * g + r) * 64 + 16 * c + n] = gW3[c][r];
}

// ---- use_viewdirs: per-ray layer-1 bias of the colour network, bias[r][u] = sum_j Wc1_sh[u][j] sh_j(rays_d[r]) -- the bits ac_render_rays forms in its prologue
__global__ __launch_bounds__(256) void sh_bias_kernel(const float *__restrict__ Wsh, const float *__restrict__ rays_d, uint32_t N, float *__restrict__ bias,
                                                      float *__restrict__ sh_out)
{
    __shared__ float slab[4][80];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t ray = blockIdx.x * 4 + wave; ray < N; ray += gridDim.x * 4) {
        ray_sh_bias<true>(slab[wave], Wsh, rays_d[3 * (size_t)ray], rays_d[3 * (size_t)ray + 1], rays_d[3 * (size_t)ray + 2], lane);
        bias[(size_t)ray * 64 + lane] = slab[wave][lane];
        if (sh_out && lane < 16) sh_out[(size_t)ray * 16 + lane] = slab[wave][64 + lane];
    }
}

// the colour kernels use the weight fragments only: no hash-level validation (the table of `field` is never touched)
int prep_color_args(RenderArgs &a, const ac_field *f)
{
    if (!f || !f->W1 || !f->b1 || !f->W2 || !f->b2 || !f->Wc1 || !f->Wc2 || !f->Wc3) { ac::set_error("ac_field: NULL parameter pointer"); return AC_ERR_BAD_ARG; }
    a.table = f->table; a.table_bytes = 0;
    a.W1 = f->W1; a.b1 = f->b1; a.W2 = f->W2; a.b2 = f->b2; a.Wc1 = f->Wc1; a.Wc2 = f->Wc2; a.Wc3 = f->Wc3;
    a.bound = 1.0f; a.two_bound = 2.0f;
    return AC_OK;
}

}  // namespace

AC_API int ac_color_forward(const ac_field *field, const float *x, const float *normal, const float *sdf16, uint32_t B, float *rgb, ac_stream_t stream)
{
    if (B == 0) return AC_OK;
    if (!x || !normal || !sdf16 || !rgb) { ac::set_error("color_forward: NULL buffer"); return AC_ERR_BAD_ARG; }
    if (field && field->Wc1_sh) { ac::set_error("color_forward: a field with view directions goes through ac_field_color_dirs / the fused renderer (the operator has no direction input)"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_color_args(a, field)) return rc;
    const size_t lds_bytes = OFF_WAVE * sizeof(float);
    uint32_t blocks = ((B + 15) / 16 + TW - 1) / TW;
    const uint32_t resident = 3 * ac::cu_count();                 // 41 KB of LDS per workgroup: three per CU, persistent
    if (blocks > resident) blocks = resident;
    hipLaunchKernelGGL(color_fwd_kernel, dim3(blocks), dim3(TBLOCK), lds_bytes, (hipStream_t)stream, a, x, normal, sdf16, B, rgb);
    return ac::check_launch("color_forward");
}

AC_API size_t ac_color_backward_scratch(uint32_t B)
{
    return (size_t)train_grid(B) * TW * NPART_C * sizeof(float);
}

AC_API int ac_sh_bias(const ac_field *field, const float *rays_d, uint32_t N, float *bias, float *sh, ac_stream_t stream)
{
    if (N == 0) return AC_OK;
    if (!field || !field->Wc1_sh) { ac::set_error("sh_bias: the field has no view-direction weights (ac_field.Wc1_sh)"); return AC_ERR_BAD_ARG; }
    if (!rays_d || !bias) { ac::set_error("sh_bias: NULL buffer"); return AC_ERR_BAD_ARG; }
    uint32_t blocks = (N + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sh_bias_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, field->Wc1_sh, rays_d, N, bias, sh);
    return ac::check_launch("sh_bias");
}

int color_backward_impl(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
                        float *g_normal, float *g_sdf16, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream,
                        const float *sh_bias, uint32_t T, float *g_sh_tiles)
{
    if (!gparams) { ac::set_error("color_backward: NULL gparams"); return AC_ERR_BAD_ARG; }
    if (B == 0) { hipMemsetAsync(gparams, 0, NPART_C * sizeof(float), (hipStream_t)stream); return AC_OK; }
    if (!x || !normal || !sdf16 || !g_rgb || !g_normal || !g_sdf16 || !scratch) { ac::set_error("color_backward: NULL buffer"); return AC_ERR_BAD_ARG; }
    const size_t need = ac_color_backward_scratch(B);
    if (scratch_bytes < need) { ac::set_error("color_backward: scratch of %zu bytes needed, %zu given", need, scratch_bytes); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_color_args(a, field)) return rc;
    const size_t lds_bytes = CBWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(color_bwd_kernel), lds_bytes);
    const uint32_t blocks = train_grid(B);
    hipLaunchKernelGGL(color_bwd_kernel, dim3(blocks), dim3(TBLOCK), lds_bytes, (hipStream_t)stream, a, x, normal, sdf16, g_rgb, B, g_normal, g_sdf16,
                       static_cast<float *>(scratch), sh_bias, T ? T : 16u, g_sh_tiles);
    partials_reduce(static_cast<const float *>(scratch), blocks * TW, (uint32_t)NPART_C, gparams, (hipStream_t)stream);
    return ac::check_launch("color_backward");
}

AC_API int ac_color_backward(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
                             float *g_normal, float *g_sdf16, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (field && field->Wc1_sh) { ac::set_error("color_backward: a field with view directions goes through ac_render_core_backward (the operator has no direction input)"); return AC_ERR_BAD_ARG; }
    return color_backward_impl(field, x, normal, sdf16, g_rgb, B, g_normal, g_sdf16, gparams, scratch, scratch_bytes, stream, nullptr, 16, nullptr);
}
