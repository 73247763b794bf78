// avatarcraft_amd/csrc/sdf_train.hip -- the differentiable render core (training path): fused SDF query, colour network and ray compositor, each forward
// and backward, and the whole-core backward ac_render_core_backward that chains them.  (The occupancy-grid renderers live in render_occupancy.hip.)
//
// One SDF query of the render core (reference models/instant_nsr.py:205-215) is forward_sdf at x (:627-642: hash encoder ->
// cat[x, h] -> WN-Linear 35->64 -> Softplus(100) -> WN-Linear 64->16) plus finite_difference_normals_approximator at
// clamp(x +- eps e_k) (:687-704): 7 encoder + MLP evaluations, ~40 PyTorch kernels forward and ~90 backward, every
// intermediate ([7B,35], [7B,64] x 2, [7B,16]) round-tripping HBM.  Here:
//   sdf_stencil_fwd_kernel : x -> sdf_out[B,16], gradient[B,3]     (the renderer's own stencil gather + MFMA MLP tiles,
//                                                                    bit-identical to the fused renderer and the oracle)
//   sdf_stencil_bwd_kernel : (x, d sdf_out, d gradient) -> d features [7,16,B,2] (consumed by hash_stencil_bwd_kernel, which
//                            owns the atomic-bound table scatter) and per-wave partial sums of dW1, db1, dW2, db2.
// The backward recomputes the forward per tile of 16 samples (gathers are L2/MALL hits, MFMA is cheap) instead of storing
// activations, and runs every product on the matrix pipe, tile layout lane = (sample n = lane & 15, group g = lane >> 4):
//   ga   = W2^T d2         16 MFMA   B operand = d2 in the register layout the forward produced it in (o = 4g + s)
//   d1   = ga * softplus'  (derivative of the SAME table polynomial the forward evaluates)
//   dinp = W1^T d1         32 MFMA   row order chosen so that every lane receives the gradient of ITS OWN 8 features
//   dW2 += d2 a^T          16 MFMA   } K = the 16 samples of the tile: operands transposed through a per-wave LDS slab,
//   dW1 += d1 inp^T        48 MFMA   } accumulators live in registers for the whole kernel (a column of ones gives db1)
// Weight-gradient partials are written per wave (no atomics) and summed by sdf_partials_reduce_kernel (deterministic).
#include "field_tile.hpp"

namespace {

constexpr int TW = 4;                              // waves per workgroup of the backward kernels (296 / 284 VGPRs: one wave per SIMD)
constexpr int TBLOCK = TW * 64;
#ifndef AC_TLD
#define AC_TLD 17
#endif
constexpr int TLD = AC_TLD;                         // padded leading dimension of the transpose slabs
// The SDF-query backward never evaluates the colour network: the 26 KB the shared layout reserves for its fragments hold this kernel's
// own ones instead (fill_lds_sdf leaves that region alone).
constexpr int OFF_W2T = OFF_C1F;                   // [4 tiles][4 ksteps][64]   fp32 A fragments of W2^T (the centre evaluation's ga = W2^T d2)
constexpr int OFF_W1TH = OFF_W2T + 16 * 64;        // [2 tiles][2 k blocks][64 lanes][4 dwords]  bf16 hi A fragments of W1^T (feature rows), 16x16x32 order
constexpr int OFF_W1TL = OFF_W1TH + 2 * 2 * 64 * 4;   // ... and the bf16 lo parts
constexpr int OFF_BW1H = OFF_W1TL + 2 * 2 * 64 * 4;   // layer-1 recomputation of the six offset evaluations (sdf_l1_delta): W1 hi / lo / coordinate columns
constexpr int OFF_BW1L = OFF_BW1H + 4 * 64 * 4;
constexpr int OFF_BW1C = OFF_BW1L + 4 * 64 * 4;
static_assert(OFF_BW1C + 3 * 64 <= OFF_B1, "the backward's fragments fit the colour region");
constexpr int OFF_TW = OFF_WAVE;                   // per-wave slabs
constexpr int TS_T2 = FE_SLAB;                     // d2  [16][TLD]
constexpr int TS_TA = TS_T2 + 16 * TLD;            // a   [64][TLD]
constexpr int TS_TD = TS_TA + 64 * TLD;            // d1  [64][TLD]
constexpr int TS_TI = TS_TD + 64 * TLD;            // inp [48][TLD]  rows 0..34 inputs, 35 = 1 (bias column), 36..47 = 0
constexpr int TRAIN_SLAB = ((TS_TI + 48 * TLD + 3) / 4) * 4;
constexpr int BWD_LDS_FLOATS = OFF_TW + TW * TRAIN_SLAB;
static_assert(BWD_LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
// Round 6: the SDF-query backward on SAVED stencil features (the render core's backward) at TWO waves per SIMD.  Round 4 / 5 ran it at one (296 registers: 66 of
// them the next tile's prefetched inputs, 56 of those the 14 x 16 bytes of saved features, which then also occupied a 12 KB slab per wave): every LDS round
// trip, every matrix-to-vector dependency of the serial chain was exposed (0.635 ms per 4096-ray patch, VALU + MFMA pipe time ~0.4 of that).  Now an evaluation's
// eight features are requested from the forward's buffer one evaluation ahead (2 x 16 bytes per lane): no feature slab.  What that buys:
//   * NOT a second wave per SIMD (AC_SDFBWD_WAVES=8: 256 registers, occupancy 2 -- and 148 spilled registers, 368 bytes of scratch per lane: the kernel's
//     natural live set is ~370 registers; backward of the SDS step 2.24 -> 3.10 ms);
//   * room for a second buffer of the d1 / input transposes, so that the weight-gradient products of evaluation e (48 fp32 MFMA of 32 clocks, a quarter of
//     the evaluation's time, with nothing beside them on the wave's only instruction stream) are issued INSIDE evaluation e + 1's recomputation
//     (softplus, splits: vector work) instead of behind a barrier at the end of their own evaluation.
#ifndef AC_SDFBWD_WAVES
#define AC_SDFBWD_WAVES 4
#endif
constexpr int TW_S = AC_SDFBWD_WAVES;                                  // waves per workgroup of sdf_stencil_bwd_kernel<SAVED = true>
// PIPE: the transposes of d1 [64 units][16 samples] and inp [48 columns][16 samples] as bf16 hi | lo parts, rows of 16 samples = 32 bytes padded to 48
// (conflict-free 16-byte reads, 16-byte aligned): one buffer = d1 hi 3072 | d1 lo 3072 | inp hi 2304 | inp lo 2304 bytes, two buffers per wave
constexpr int BF_ROW = 48, BF_D1H = 0, BF_D1L = 64 * BF_ROW, BF_INH = 2 * 64 * BF_ROW, BF_INL = BF_INH + 48 * BF_ROW, BF_BYTES = BF_INL + 48 * BF_ROW;
constexpr int TRAIN_SLAB_PIPE = ((TS_TD - FE_SLAB) + 2 * BF_BYTES / 4 + 3) / 4 * 4;       // T2 | TA | two bf16 buffers
constexpr int TRAIN_SLAB_NOPIPE = TRAIN_SLAB - FE_SLAB;
constexpr int TRAIN_SLAB_S = TRAIN_SLAB_PIPE > TRAIN_SLAB_NOPIPE ? TRAIN_SLAB_PIPE : TRAIN_SLAB_NOPIPE;    // the SAVED variant's per-wave slab: no feature region
constexpr int BWD_LDS_FLOATS_S = OFF_TW + TW_S * TRAIN_SLAB_S;
static_assert(BWD_LDS_FLOATS_S * 4 <= 160 * 1024, "LDS budget");
constexpr int NPART = 64 * 36 + 16 * 64 + 16;      // dW1 [64][36] (column 35 = db1), dW2 [16][64], db2 [16]

// four values at once: the table rows are requested together (one LDS round trip per batch, see dv_softplus100_n)
__device__ __forceinline__ void softplus100_vg4(const float *__restrict__ spg, const f32x4 &x, f32x4 &val, f32x4 &der)
{
    float v[4]; float4 c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a4 = __builtin_fminf(__builtin_fabsf(x[i] * 400.0f), 128.0f);
        const uint32_t idx = (uint32_t)a4;
        v[i] = __builtin_amdgcn_fractf(a4);
        c[i] = *reinterpret_cast<const float4 *>(spg + idx * 4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float q = c[i].w;
        q = fma_(q, v[i], c[i].z); q = fma_(q, v[i], c[i].y); q = fma_(q, v[i], c[i].x);
        float dq = 3.0f * c[i].w;
        dq = fma_(dq, v[i], 2.0f * c[i].z); dq = fma_(dq, v[i], c[i].y);
        const bool pos = x[i] > 0.0f;
        val[i] = fma_(0.5f, __builtin_fabsf(x[i]), fma_(0.5f, x[i], q));
        der[i] = (pos ? 1.0f : 0.0f) + (pos ? 400.0f : -400.0f) * dq;
    }
}

__global__ __launch_bounds__(FBLOCK) void sdf_stencil_fwd_kernel(const RenderArgs a, const float *__restrict__ x, uint32_t B, float eps,
                                                                 float *__restrict__ out16, float *__restrict__ grad)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const uint32_t ntiles = (B + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < B ? b : B - 1;
        const float px = x[3 * (size_t)bb], py = x[3 * (size_t)bb + 1], pz = x[3 * (size_t)bb + 2];
        float fe0[4][2];
        encode_stencil(lds, fsl, fc, lane, px, py, pz, eps, fe0);
        f32x4 oc; float gr[3];
        fd_forward(lds, fsl, lane, px, py, pz, eps, a.bound, fe0, oc, gr);
        if (b < B) {
            *reinterpret_cast<f32x4 *>(out16 + (size_t)b * 16 + 4 * g) = oc;
            if (g == 0) { grad[3 * (size_t)b] = gr[0]; grad[3 * (size_t)b + 1] = gr[1]; grad[3 * (size_t)b + 2] = gr[2]; }
        }
        wave_sync();
    }
}

// extra weight fragments of the backward: W2^T (ga = W2^T d2, fp32) and the feature rows of W1^T (dinp = W1^T d1) split into bf16 hi + lo
// for v_mfma_f32_16x16x32_bf16: K = the 64 hidden units in two blocks of 32; within block b lane group kk supplies slots i = 0..7 =
// units 16 (2b + (i >> 2)) + 4 kk + (i & 3) -- exactly the sixteen d1 values lane (n, kk) holds (accumulator tiles 2b, 2b+1), no data movement
__device__ __forceinline__ void fill_lds_bwd(float *lds, const RenderArgs &a)
{
    for (int e = threadIdx.x; e < 16 * 64; e += blockDim.x) {       // fragment (t, s): lane (m, kk) = W2[o = 4 kk + s][unit = 16 t + m]
        const int l = e & 63, fs = e >> 6, t = fs >> 2, s = fs & 3, m = l & 15, kk = l >> 4;
        lds[OFF_W2T + e] = a.W2[(4 * kk + s) * 64 + 16 * t + m];
    }
    uint32_t *lw = reinterpret_cast<uint32_t *>(lds);
    for (int e = threadIdx.x; e < 2 * 2 * 64 * 4; e += blockDim.x) { // dword q of lane l, k block b, output tile tp
        const int q = e & 3, l = (e >> 2) & 63, b = (e >> 8) & 1, tp = e >> 9, m = l & 15, kk = l >> 4;
        const int s1 = 4 * tp + (m & 3);                            // output row m = feature slot 2j + c of lane group m >> 2
        const int col = 3 + 2 * (4 * (s1 >> 1) + (m >> 2)) + (s1 & 1);
        uint32_t hi2 = 0, lo2 = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 2 * q + h, unit = 16 * (2 * b + (i >> 2)) + 4 * kk + (i & 3);
            const float w = a.W1[unit * 35 + col];
            const uint32_t hb = bf16_rne_bits(w), lb = bf16_rne_bits(w - __uint_as_float(hb << 16));
            hi2 |= hb << (16 * h); lo2 |= lb << (16 * h);
        }
        lw[OFF_W1TH + e] = hi2; lw[OFF_W1TL + e] = lo2;
    }
    fill_lds_fast<OFF_BW1H, OFF_BW1L, OFF_BW1C>(lds, a);
}

// SAVED: the features of the seven stencil points come from the forward launch (ac_render_out.feat7, [B / 16][14][64 lanes][4] in this kernel's lane order) as 14
// coalesced 16-byte loads per lane instead of being gathered from the table again (index arithmetic + ~100 scattered 8-byte loads per lane and tile)
// GX: the sample positions carry a gradient themselves (the curvature term's perturbed points, models/instant_nsr.py:276-288): g_x [B][3] receives the share
// that enters through the MLP's own xyz inputs (include_input, :632-633) -- W1[:, 0:3]^T d1 summed over the seven evaluations, the offset coordinate of an
// offset evaluation through its clamp (:690-702).  The share through the encodings is ac_hash_stencil_input_backward's.
template <bool SAVED, bool GX = false>
__global__ __launch_bounds__(SAVED ? TW_S * 64 : TBLOCK) void sdf_stencil_bwd_kernel(const RenderArgs a, const float *__restrict__ x, const float *__restrict__ g_out,
                                                                 const float *__restrict__ g_grad, uint32_t B, float eps,
                                                                 float *__restrict__ gfeat, float *__restrict__ partials,
                                                                 const float *__restrict__ feat7, float *__restrict__ g_x = nullptr)
{
    static_assert(!(SAVED && GX), "the position gradient is built for the stand-alone operator");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    fill_lds_bwd(lds, a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    constexpr int KW = SAVED ? TW_S : TW, SFE = SAVED ? FE_SLAB : 0;   // waves per workgroup | floats the slab does not hold (SAVED: no feature region)
    float *slab = lds + OFF_TW + wave * (SAVED ? TRAIN_SLAB_S : TRAIN_SLAB);
    float *fsl = slab, *T2 = slab + TS_T2 - SFE, *TA = slab + TS_TA - SFE, *TD0 = slab + TS_TD - SFE, *TI0 = slab + TS_TI - SFE;
    // PIPE: two buffers of (d1, inp) transposes -- evaluation `step` writes buffer step & 1 while the weight-gradient products of the evaluation before it read
    // the other one.  The very first step's "previous evaluation" is a buffer of zeros (products of 0: the accumulators keep their +0).
    constexpr bool PIPE = SAVED;                                // the weight-gradient products of evaluation e run inside evaluation e + 1 on the bf16 matrix pipe
    unsigned char *const BF = reinterpret_cast<unsigned char *>(TD0);      // PIPE: the two bf16 buffers take the place of the fp32 transposes
    if constexpr (PIPE) {
        uint32_t *bw = reinterpret_cast<uint32_t *>(BF);
        for (int e = lane; e < 2 * BF_BYTES / 4; e += 64) {                 // zeros; the bias column (input row 35) = bf16 1.0 in the hi part, for all 16 samples
            const int o = (4 * e) % BF_BYTES;
            bw[e] = (o >= BF_INH + 35 * BF_ROW && o < BF_INH + 35 * BF_ROW + 32) ? 0x3f803f80u : 0u;
        }
    } else {
        for (int e = lane; e < 48 * TLD; e += 64) TI0[e] = (e >= 35 * TLD && e < 36 * TLD) ? 1.0f : 0.0f;       // bias column, zero padding rows
    }
    __syncthreads();
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    f32x4 gW1[4][3], gW2[4];
    float gb2[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    float a6[4][4];                                   // running sum over samples and offset evaluations of s * a[unit 16t + 4g + r] (-> dW2 row 0)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) a6[t][r] = 0.0f;
    const W2Row0 w2r0 = load_w2_row0(lds, lane);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        gW2[t] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int c = 0; c < 3; ++c) gW1[t][c] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    }
    float wxyz[GX ? 4 : 1][4][3];                               // GX: W1[unit 16t + 4g + r][0..2], this lane's 16 units
    if constexpr (GX) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) wxyz[t][r][c] = a.W1[(16 * t + 4 * g + r) * 35 + c];
    }
    uint32_t step = 0;                                          // evaluations this wave has been through (PIPE: selects the buffer)
    // the weight-gradient products of ONE evaluation from its transposes: dW2 += d2 a^T (16 MFMA, centre evaluations only: the offset evaluations' share is
    // the rank-1 running sum a6) and dW1 += d1 inp^T (48 MFMA)
    auto w2_grads = [&]() {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a2 = T2[n * TLD + 4 * s + g];                         // A: d2[o = lane & 15][sample 4s + kk]
#pragma unroll
            for (int c = 0; c < 4; ++c)
                gW2[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, TA[(16 * c + n) * TLD + 4 * s + g], gW2[c], 0, 0, 0);
        }
    };
    auto w1_grads = [&](const float *__restrict__ TDr, const float *__restrict__ TIr) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float bi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) bi[c] = TIr[(16 * c + n) * TLD + 4 * s + g];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float a1 = TDr[(16 * t + n) * TLD + 4 * s + g];
#pragma unroll
                for (int c = 0; c < 3; ++c) gW1[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bi[c], gW1[t][c], 0, 0, 0);
            }
        }
    };
    const uint32_t ntiles = (B + 15) / 16;
    const float hs = 0.5f / eps;
    // The inputs of tile i + 1 are requested while tile i is computed (round 4): with one wave per SIMD nothing else covers their ~2 us, and a third of
    // the 512 registers a lone wave may use are free.  TileIn = what a lane reads per tile: its sample's position and upstream gradients and, with SAVED,
    // the 14 x 16 bytes of stencil features the forward kept ([tile][14][lane][4], see render_rays_kernel: each load 1 KB contiguous per wave).
    struct TileIn { float p[3], gg[3]; f32x4 go; };
    auto request = [&](uint32_t tile, TileIn &in) {
        const uint32_t b = tile * 16 + n, bb = b < B ? b : B - 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) { in.p[k] = x[3 * (size_t)bb + k]; in.gg[k] = g_grad[3 * (size_t)bb + k]; }
        in.go = *reinterpret_cast<const f32x4 *>(g_out + (size_t)bb * 16 + 4 * g);
    };
    // SAVED: the eight features of evaluation e of a tile = floats 8 e .. 8 e + 7 of this lane = two 16-byte loads ([tile][14][lane][4]), requested one
    // evaluation ahead
    struct Feat2 { f32x4 a, b; };
    auto request_feat = [&](uint32_t tile, int e, Feat2 &f) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(feat7) + ((size_t)tile * 14 + 2 * (size_t)e) * 64 + lane;
        f.a = src[0]; f.b = src[64];
    };
    const uint32_t tile0 = blockIdx.x * KW + wave, tstride = gridDim.x * KW;
    TileIn nxt;
    Feat2 fnx{};
    if (tile0 < ntiles) { request(tile0, nxt); if constexpr (SAVED) request_feat(tile0, 0, fnx); }
    for (uint32_t tile = tile0; tile < ntiles; tile += tstride) {
        const uint32_t b = tile * 16 + n;
        const bool live = b < B;
        const float px = nxt.p[0], py = nxt.p[1], pz = nxt.p[2];
        f32x4 go = nxt.go;
        float gg[3] = { nxt.gg[0], nxt.gg[1], nxt.gg[2] };
        if (!live) { go = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f }; gg[0] = gg[1] = gg[2] = 0.0f; }
        float fe0[4][2];
        if constexpr (SAVED) {
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_) { fe0[q_ >> 1][q_ & 1] = fnx.a[q_]; fe0[2 + (q_ >> 1)][q_ & 1] = fnx.b[q_]; }
        } else {
            encode_stencil(lds, fsl, fc, lane, px, py, pz, eps, fe0);
        }
        if (tile + tstride < ntiles) request(tile + tstride, nxt);
        const float pc0 = sel4(g, px, py, pz, 0.0f);
        Acc4 h10;                                               // layer 1 of the centre evaluation (set at e == 0)
#pragma unroll
        for (int t = 0; t < 4; ++t) h10.a[t] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
        float gxa[3] = { 0.0f, 0.0f, 0.0f };                    // GX: d loss / d (px, py, pz) through the xyz inputs, summed over the evaluations
#pragma unroll 1
        for (int e = 0; e < 7; ++e) {
            const int k = e > 0 ? (e - 1) >> 1 : 3;
            float *const TD = TD0, *const TI = TI0;                                                      // (!PIPE) this evaluation's fp32 transposes
            if constexpr (PIPE) { if (e == 1) w2_grads(); }                    // (the evaluation before this one was the tile's centre)
            float fe[4][2];
            if constexpr (SAVED) {
#pragma unroll
                for (int q_ = 0; q_ < 4; ++q_) { fe[q_ >> 1][q_ & 1] = fnx.a[q_]; fe[2 + (q_ >> 1)][q_ & 1] = fnx.b[q_]; }
                // the next evaluation's features (the next tile's centre after the last one) leave now: a whole evaluation of arithmetic covers them
                if (e < 6) request_feat(tile, e + 1, fnx);
                else if (tile + tstride < ntiles) request_feat(tile + tstride, 0, fnx);
            } else if (e == 0) {
#pragma unroll
                for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fe0[q_ >> 1][q_ & 1];
            } else {
#pragma unroll
                for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fsl[((e - 1) * 8 + q_) * 64 + lane];
            }
            const float pk = k == 0 ? px : (k == 1 ? py : pz);
            const float poff = clampf(pk + (((e - 1) & 1) ? -eps : eps), -bound, bound);
            const float bx = (e > 0 && g == k) ? poff : pc0;
            // upstream gradient of this evaluation's 16 outputs, in the forward's register layout (o = 4g + r)
            f32x4 d2;
            float s_all = 0.0f;                                                 // the offset evaluations' only upstream value, in every lane of the sample
            if (e == 0) d2 = go;
            else {
                const float gk = k == 0 ? gg[0] : (k == 1 ? gg[1] : gg[2]);
                s_all = ((e - 1) & 1) ? -(gk * hs) : gk * hs;                   // d gradient_k / d sdf(x +- eps e_k) = +-0.5 / eps
                d2 = f32x4{ g == 0 ? s_all : 0.0f, 0.0f, 0.0f, 0.0f };
            }
            // recompute layer 1, softplus and its derivative: the centre in fp32, the six offset evaluations as split-bf16 corrections of it
            // (sdf_l1_delta; the arithmetic of the renderer's "fast" precision: 12 short MFMA instead of 36 fp32 ones)
            Acc4 h1;
            if (e == 0) { h1 = sdf_l1(lds, lane, bx, fe); h10 = h1; }
            else h1 = sdf_l1_delta<OFF_BW1H, OFF_BW1L, OFF_BW1C>(lds, lane, h10, fe, fe0, k, poff - pk);
            Acc4 av, dv;
            if constexpr (PIPE) {
                // The PREVIOUS evaluation's weight-gradient products dW1 += d1 inp^T, issued inside this evaluation's 16 softplus values + derivatives (the
                // largest stretch of vector work of an evaluation: no LDS stores, no branches), the order pinned by scheduling fences.
                // On the bf16 matrix pipe, K = 32 = [hi parts of the tile's 16 samples | lo parts]: per 16 x 16 output tile
                //   gW1 += [d1 hi | d1 lo] x [inp hi | inp hi]   (hi hi + lo hi)      gW1 += [d1 hi | d1 lo] x [inp lo | 0]   (hi lo)
                // -- 24 instructions of 16 clocks that CO-EXECUTE with vector instructions, instead of 48 fp32 ones of 32 clocks that do not (the fp32 matrix
                // instructions run on the vector pipe's multipliers, SQ_VALU_MFMA_COEXEC_CYCLES = 0: interleaving THOSE with the softplus work was built
                // and measured first and bought nothing -- backward 2.244 -> 2.300 ms, profiles/r06_experiments.txt).  The dropped lo x lo term is 2^-16 of
                // a product; the sums stay fp32.  Lane (m, kk) reads 8 consecutive samples of row m: kk = 0, 1 from the hi part, kk = 2, 3 from the lo
                // part (d1) / the hi part again (inp, first product) / a row of zeros (inp, second product).
                const unsigned char *const Br = BF + ((step & 1u) ? 0 : BF_BYTES);
                const float *__restrict__ spg = lds + OFF_SPQ;
                const int kk_ = lane >> 4, m_ = lane & 15;
                const unsigned char *const pa = Br + (kk_ >= 2 ? BF_D1L : BF_D1H) + m_ * BF_ROW + (kk_ & 1) * 16;
                const unsigned char *const pb1 = Br + BF_INH + m_ * BF_ROW + (kk_ & 1) * 16;
                const unsigned char *const pb2 = kk_ >= 2 ? Br + BF_INL + 40 * BF_ROW : Br + BF_INL + m_ * BF_ROW + (kk_ & 1) * 16;    // (input rows 36 .. 47 are zero padding)
                const int pb2s = kk_ >= 2 ? 0 : 16 * BF_ROW;
                bf16x8 opA[4], opB1[3], opB2[3];
                auto rdA = [&](int t_) { opA[t_] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(pa + 16 * t_ * BF_ROW)); };
                auto rdB = [&](int c_) {
                    opB1[c_] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(pb1 + 16 * c_ * BF_ROW));
                    opB2[c_] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(pb2 + c_ * pb2s));
                };
                rdA(0); rdA(1); rdB(0); rdB(1); rdB(2);
                float xs[16], vv[16], qq[16], dq[16];
                float4 cc[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) xs[i] = h1.a[i >> 2][i & 3];
                auto P1 = [&](int i) {                                       // row request of value i
                    const float a4 = __builtin_fminf(__builtin_fabsf(xs[i] * 400.0f), 128.0f);
                    const uint32_t idx = (uint32_t)a4;
                    vv[i] = __builtin_amdgcn_fractf(a4);
                    cc[i] = *reinterpret_cast<const float4 *>(spg + idx * 4);
                };
                auto P2 = [&](int i) {                                       // the cubic and its derivative
                    float q = cc[i].w;
                    q = fma_(q, vv[i], cc[i].z); q = fma_(q, vv[i], cc[i].y); q = fma_(q, vv[i], cc[i].x);
                    float d = 3.0f * cc[i].w;
                    d = fma_(d, vv[i], 2.0f * cc[i].z); d = fma_(d, vv[i], cc[i].y);
                    qq[i] = q; dq[i] = d;
                };
                auto P3 = [&](int i) {                                       // value and derivative of softplus_100
                    const bool pos = xs[i] > 0.0f;
                    av.a[i >> 2][i & 3] = fma_(0.5f, __builtin_fabsf(xs[i]), fma_(0.5f, xs[i], qq[i]));
                    dv.a[i >> 2][i & 3] = (pos ? 1.0f : 0.0f) + (pos ? 400.0f : -400.0f) * dq[i];
                };
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kq = 0; kq < 24; ++kq) {
                    const int t_ = kq / 6, c_ = (kq % 6) >> 1, second = kq & 1;
                    gW1[t_][c_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(opA[t_], second ? opB2[c_] : opB1[c_], gW1[t_][c_], 0, 0, 0);
                    if (kq == 0) rdA(2);
                    if (kq == 2) rdA(3);
                    // two slices of the softplus work per group: P1(0) P1(1) P1(2) | P2(i) P3(i) P1(i + 3) for i = 0 .. 12 | P2(13) P3(13) .. P2(15) P3(15)
#pragma unroll
                    for (int h_ = 0; h_ < 2; ++h_) {
                        const int ks = 2 * kq + h_;
                        if (ks < 3) P1(ks);
                        else if (ks < 42) { const int i = (ks - 3) / 3, ph = (ks - 3) % 3; if (ph == 0) P2(i); else if (ph == 1) P3(i); else P1(i + 3); }
                        else { const int i = 13 + (ks - 42) / 2, ph = (ks - 42) % 2; if (ph == 0) P2(i); else P3(i); }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) softplus100_vg4(lds + OFF_SPQ, h1.a[t], av.a[t], dv.a[t]);
            }
            Acc4 d1;
            // The six offset evaluations feed the finite-difference gradient through their sdf alone: d2 = (s, 0, ..., 0).  Then
            // ga = W2^T d2 = s * W2[0, :] (16 multiplies instead of 16 MFMA), and their share of dW2 / db2 is row 0 only:
            // dW2[0, u] += sum over samples of s * a[u], kept as a per-lane running sum (reduced over the samples once, at the end).
            const bool rank1 = e > 0;
            if (rank1) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        d1.a[t][r] = (s_all * w2r0.w[t][r]) * dv.a[t][r];
                        a6[t][r] = fma_(s_all, av.a[t][r], a6[t][r]);
                    }
            } else
            {
                // ga = W2^T d2, d1 = ga * softplus'
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x4 ga = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
                    for (int s = 0; s < 4; ++s) ga = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_W2T + (t * 4 + s) * 64 + lane], d2[s], ga, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) d1.a[t][r] = ga[r] * dv.a[t][r];
                }
            }
            if constexpr (GX) {
                const float raw = pk + (((e - 1) & 1) ? -eps : eps);
                const float pass = (e == 0 || (raw >= -bound && raw <= bound)) ? 1.0f : 0.0f;       // d clamp / d x (inclusive, like torch.clamp's backward)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float sx = 0.0f;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sx = fma_(d1.a[t][r], wxyz[t][r][c], sx);
                    sx += __shfl_xor(sx, 16); sx += __shfl_xor(sx, 32);                                 // over the four lane groups of the sample
                    gxa[c] += (c == k) ? sx * pass : sx;
                }
            }
            // dinp = W1^T d1: this lane's own features (j = 2t' + (r >> 1), c = r & 1), on the bf16 matrix pipe with both factors split
            // hi + lo (3 products, fp32 accumulate: 2^-16 relative, far below the tolerance of a gradient): 12 short MFMA instead of 32 fp32 ones
            {
                u32x4 bh[2], bl[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float dd[8] = { d1.a[2 * b][0], d1.a[2 * b][1], d1.a[2 * b][2], d1.a[2 * b][3],
                                          d1.a[2 * b + 1][0], d1.a[2 * b + 1][1], d1.a[2 * b + 1][2], d1.a[2 * b + 1][3] };
                    split8_bf16(dd, bh[b], bl[b]);
                }
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {
                    f32x4 gi = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const bf16x8 Ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + OFF_W1TH + ((tp * 2 + b) * 64 + lane) * 4));
                        const bf16x8 Al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + OFF_W1TL + ((tp * 2 + b) * 64 + lane) * 4));
                        const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh[b]), Bl = __builtin_bit_cast(bf16x8, bl[b]);
                        gi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, gi, 0, 0, 0);
                        gi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, gi, 0, 0, 0);
                        gi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, gi, 0, 0, 0);
                    }
                    if (live) {
#pragma unroll
                        for (int m = 0; m < 2; ++m) {
                            const int j = 2 * tp + m;
                            *reinterpret_cast<float2 *>(gfeat + (((size_t)e * 16 + 4 * j + g) * B + b) * 2) = make_float2(gi[2 * m], gi[2 * m + 1]);
                        }
                    }
                }
            }
            // transposes for the weight gradients (K = the 16 samples of the tile)
            if (!rank1)
            {
#pragma unroll
                for (int r = 0; r < 4; ++r) T2[(4 * g + r) * TLD + n] = d2[r];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) TA[(16 * t + 4 * g + r) * TLD + n] = av.a[t][r];
            }
            if constexpr (PIPE) {
                // hi = the value ROUNDED TO NEAREST bf16 (v_cvt_pk_bf16_f32), lo = (value - hi) rounded likewise, 2-byte stores at [row][sample n].  Not
                // split8_bf16's truncation: a weight gradient is a sum of ~3.7 M such products per entry, and truncation errors all point towards zero -- they
                // add up coherently.  dW1 vs the fp64 oracle, of max (tests/test_oracle_backward.py; fp32 products before: 1.9e-4; bound 3e-4):
                //   hi and lo truncated 3.1e-4 | hi truncated (a free d16_hi store), lo rounded 2.2e-4 (the dropped lo x lo term keeps the product's sign, and the
                //   three separately back-propagated loss terms add up to the joint pass only to 2.1e-4) | both rounded 1.2e-4  <- shipped (+0.03 ms per patch)
                unsigned char *const Bw = BF + ((step & 1u) ? BF_BYTES : 0);
                auto put = [&](int part_hi, int part_lo, int row, float v) {
                    const __bf16 hb = (__bf16)v;
                    const __bf16 lb = (__bf16)(v - (float)hb);
                    *reinterpret_cast<__bf16 *>(Bw + part_hi + row * BF_ROW + 2 * n) = hb;
                    *reinterpret_cast<__bf16 *>(Bw + part_lo + row * BF_ROW + 2 * n) = lb;
                };
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) put(BF_D1H, BF_D1L, 16 * t + 4 * g + r, d1.a[t][r]);
                if (g < 3) put(BF_INH, BF_INL, g, bx);
#pragma unroll
                for (int s1 = 0; s1 < 8; ++s1) put(BF_INH, BF_INL, 3 + 2 * (4 * (s1 >> 1) + g) + (s1 & 1), fe[s1 >> 1][s1 & 1]);
            } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) TD[(16 * t + 4 * g + r) * TLD + n] = d1.a[t][r];
            if (g < 3) TI[g * TLD + n] = bx;
#pragma unroll
            for (int s1 = 0; s1 < 8; ++s1) TI[(3 + 2 * (4 * (s1 >> 1) + g) + (s1 & 1)) * TLD + n] = fe[s1 >> 1][s1 & 1];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) gb2[r] += d2[r];
            wave_sync();
            ++step;
            if constexpr (!PIPE) {
                if (!rank1)
                    w2_grads();
                w1_grads(TD, TI);
                wave_sync();
            }
        }
        if constexpr (GX) {
            if (live && g < 3) g_x[3 * (size_t)b + g] = g == 0 ? gxa[0] : (g == 1 ? gxa[1] : gxa[2]);
        }
    }
    if constexpr (PIPE) {                                       // the last evaluation's products (an offset evaluation; a wave without a tile: the zero buffer)
        const unsigned char *const Br = BF + ((step & 1u) ? 0 : BF_BYTES);
        const int kk_ = lane >> 4, m_ = lane & 15;
#pragma unroll
        for (int t_ = 0; t_ < 4; ++t_) {
            const bf16x8 A = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(Br + (kk_ >= 2 ? BF_D1L : BF_D1H) + (16 * t_ + m_) * BF_ROW + (kk_ & 1) * 16));
#pragma unroll
            for (int c_ = 0; c_ < 3; ++c_) {
                const bf16x8 B1 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(Br + BF_INH + (16 * c_ + m_) * BF_ROW + (kk_ & 1) * 16));
                const bf16x8 B2 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(Br + BF_INL + (kk_ >= 2 ? 40 : 16 * c_ + m_) * BF_ROW + (kk_ >= 2 ? 0 : (kk_ & 1) * 16)));
                gW1[t_][c_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B1, gW1[t_][c_], 0, 0, 0);
                gW1[t_][c_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B2, gW1[t_][c_], 0, 0, 0);
            }
        }
    }
    // per-wave partial sums: dW1 [64][36] | dW2 [16][64] | db2 [16]
    float *part = partials + (size_t)(blockIdx.x * KW + wave) * NPART;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int unit = 16 * t + 4 * g + r, kcol = 16 * c + n;
                if (kcol < 36) part[unit * 36 + kcol] = gW1[t][c][r];
            }
    // row 0 of dW2 also receives the offset evaluations' running sums: unit u = 16c + n of lane (n, g = 0) is held, after a row reduction over
    // the 16 samples, by lane 15 of lane group n >> 2 in register a6[c][n & 3]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float tot[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[r] = __shfl(row_scan<false>(a6[c][r]), 16 * (n >> 2) + 15);
        const float add = (n & 3) == 0 ? tot[0] : ((n & 3) == 1 ? tot[1] : ((n & 3) == 2 ? tot[2] : tot[3]));
        if (g == 0) gW2[c][0] += add;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[64 * 36 + (4 * g + r) * 64 + 16 * c + n] = gW2[c][r];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float tot = row_scan<false>(gb2[r]);                   // inclusive scan over the 16 samples of the row: lane n == 15 holds the total
        if (n == 15) part[64 * 36 + 16 * 64 + 4 * g + r] = tot;
    }
}

// out[i] = sum over waves of partials[w][i]: RED_OUT outputs x RED_SL wave slices per workgroup, fixed summation order (deterministic).  Round 4: 16 x 64
// instead of 64 x 16 -- four times the workgroups and a quarter of the dependent trip count per thread (21 -> ~8 us for 1024 partial sets)
constexpr uint32_t RED_OUT = 16, RED_SL = 64;
__global__ __launch_bounds__(1024) void sdf_partials_reduce_kernel(const float *__restrict__ partials, uint32_t nwaves, float *__restrict__ out)
{
    __shared__ double red[RED_SL][RED_OUT];  // (double: the order of the partials must not show up in the last bits of a sum of ~1000 of them)
    const uint32_t o = threadIdx.x % RED_OUT, sl = threadIdx.x / RED_OUT;
    const uint32_t i = blockIdx.x * RED_OUT + o;
    double s = 0.0;
    if (i < (uint32_t)NPART)
        for (uint32_t w = sl; w < nwaves; w += RED_SL) s += (double)partials[(size_t)w * NPART + i];
    red[sl][o] = s;
    __syncthreads();
    if (sl == 0 && i < (uint32_t)NPART) {
        double t = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < RED_SL; ++k) t += red[k][o];
        out[i] = (float)t;
    }
}

// ======================================================================================================================
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

// ======================================================================================================================
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

// generic: out[i] = sum over waves of partials[w][i], i < n_out
__global__ __launch_bounds__(1024) void partials_reduce_kernel(const float *__restrict__ partials, uint32_t nwaves, uint32_t n_out, float *__restrict__ out)
{
    __shared__ double red[RED_SL][RED_OUT]; // (double: the order of the partials must not show up in the last bits of a sum of ~1000 of them)
    const uint32_t o = threadIdx.x % RED_OUT, sl = threadIdx.x / RED_OUT;
    const uint32_t i = blockIdx.x * RED_OUT + o;
    double s = 0.0;
    if (i < n_out)
        for (uint32_t w = sl; w < nwaves; w += RED_SL) s += (double)partials[(size_t)w * n_out + i];
    red[sl][o] = s;
    __syncthreads();
    if (sl == 0 && i < n_out) {
        double t = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < RED_SL; ++k) t += red[k][o];
        out[i] = (float)t;
    }
}

// ---- glue of the whole-core backward (ac_render_core_backward) -------------------------------------------------------------------
// normal = gradient / (1e-5 + |gradient|)  (instant_nsr.py:215), the renderer's own arithmetic: the colour / compositing backward
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

uint32_t train_grid(uint32_t B)
{
    const uint32_t ntiles = (B + 15) / 16;
    uint32_t blocks = (ntiles + TW - 1) / TW;
    const uint32_t cap = ac::cu_count();               // persistent, ONE workgroup per CU: their ~145 KB of LDS admit no second one, and every workgroup
                                                       // first lays the weights out in LDS (512 workgroups: backward 3.32 ms per SDS step, 256: 3.20)
    if (blocks > cap) blocks = cap;
    return blocks ? blocks : 1;
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

AC_API int ac_sdf_stencil_forward(const ac_field *field, const float *x, uint32_t B, float bound, float eps, float *out16, float *grad,
                                  ac_stream_t stream)
{
    if (B == 0) return AC_OK;
    if (!x || !out16 || !grad || !(eps > 0.0f)) { ac::set_error("sdf_stencil_forward: NULL buffer or eps <= 0"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, bound, eps)) return rc;
    const size_t lds_bytes = FWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(sdf_stencil_fwd_kernel), lds_bytes);
    uint32_t blocks = ((B + 15) / 16 + FW - 1) / FW;              // persistent: the 140 KB of LDS allow one workgroup per CU, and every
    const uint32_t cus = ac::cu_count();                          // workgroup first lays the weights out in LDS
    if (blocks > cus) blocks = cus;
    hipLaunchKernelGGL(sdf_stencil_fwd_kernel, dim3(blocks), dim3(FBLOCK), lds_bytes, (hipStream_t)stream, a, x, B, eps, out16, grad);
    return ac::check_launch("sdf_stencil_forward");
}

AC_API size_t ac_sdf_stencil_backward_scratch(uint32_t B)
{
    return (size_t)train_grid(B) * (TW_S > TW ? TW_S : TW) * NPART * sizeof(float);
}

static int sdf_stencil_backward_impl(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                                     float eps, float *gfeat, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream, const float *feat7,
                                     float *g_x = nullptr)
{
    if (!gparams) { ac::set_error("sdf_stencil_backward: NULL gparams"); return AC_ERR_BAD_ARG; }
    if (g_x && feat7) { ac::set_error("sdf_stencil_backward: the position gradient is not built for the saved-feature form"); return AC_ERR_BAD_ARG; }
    if (B == 0) { hipMemsetAsync(gparams, 0, NPART * sizeof(float), (hipStream_t)stream); return AC_OK; }
    if (!x || !g_out16 || !g_grad || !gfeat || !scratch || !(eps > 0.0f)) { ac::set_error("sdf_stencil_backward: NULL buffer or eps <= 0"); return AC_ERR_BAD_ARG; }
    const size_t need = ac_sdf_stencil_backward_scratch(B);
    if (scratch_bytes < need) { ac::set_error("sdf_stencil_backward: scratch of %zu bytes needed, %zu given", need, scratch_bytes); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, bound, eps)) return rc;
    const size_t lds_bytes = BWD_LDS_FLOATS * sizeof(float), lds_bytes_s = BWD_LDS_FLOATS_S * sizeof(float);
    static uint64_t seen = 0, seen_s = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(sdf_stencil_bwd_kernel<false>), lds_bytes);
    ac::allow_dynamic_lds(seen_s, reinterpret_cast<const void *>(sdf_stencil_bwd_kernel<true>), lds_bytes_s);
    uint32_t blocks = train_grid(B);
    if (feat7) {
        const uint32_t need_blocks = ((B + 15) / 16 + TW_S - 1) / TW_S;           // (persistent: one workgroup of TW_S waves per compute unit)
        if (blocks > need_blocks) blocks = need_blocks ? need_blocks : 1;
        hipLaunchKernelGGL(sdf_stencil_bwd_kernel<true>, dim3(blocks), dim3(TW_S * 64), lds_bytes_s, (hipStream_t)stream, a, x, g_out16, g_grad, B, eps, gfeat,
                           static_cast<float *>(scratch), feat7, (float *)nullptr);
    } else if (g_x) {
        static uint64_t seen_x = 0;
        ac::allow_dynamic_lds(seen_x, reinterpret_cast<const void *>(sdf_stencil_bwd_kernel<false, true>), lds_bytes);
        hipLaunchKernelGGL((sdf_stencil_bwd_kernel<false, true>), dim3(blocks), dim3(TBLOCK), lds_bytes, (hipStream_t)stream, a, x, g_out16, g_grad, B, eps, gfeat,
                           static_cast<float *>(scratch), feat7, g_x);
    } else
        hipLaunchKernelGGL(sdf_stencil_bwd_kernel<false>, dim3(blocks), dim3(TBLOCK), lds_bytes, (hipStream_t)stream, a, x, g_out16, g_grad, B, eps, gfeat,
                           static_cast<float *>(scratch), feat7, (float *)nullptr);
    hipLaunchKernelGGL(sdf_partials_reduce_kernel, dim3((NPART + RED_OUT - 1) / RED_OUT), dim3(1024), 0, (hipStream_t)stream, static_cast<const float *>(scratch),
                       blocks * (feat7 ? TW_S : TW), gparams);
    return ac::check_launch("sdf_stencil_backward");
}

AC_API int ac_sdf_stencil_backward(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                                   float eps, float *gfeat, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    return sdf_stencil_backward_impl(field, x, g_out16, g_grad, B, bound, eps, gfeat, gparams, scratch, scratch_bytes, stream, nullptr);
}

AC_API int ac_sdf_stencil_backward_inputs(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                                          float eps, float *gfeat, float *gparams, float *g_x, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (!g_x && B) { ac::set_error("sdf_stencil_backward_inputs: NULL g_x"); return AC_ERR_BAD_ARG; }
    return sdf_stencil_backward_impl(field, x, g_out16, g_grad, B, bound, eps, gfeat, gparams, scratch, scratch_bytes, stream, nullptr, g_x);
}

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

static int color_backward_impl(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
                               float *g_normal, float *g_sdf16, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream,
                               const float *sh_bias, uint32_t T, float *g_sh_tiles);

AC_API int ac_color_backward(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
                             float *g_normal, float *g_sdf16, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (field && field->Wc1_sh) { ac::set_error("color_backward: a field with view directions goes through ac_render_core_backward (the operator has no direction input)"); return AC_ERR_BAD_ARG; }
    return color_backward_impl(field, x, normal, sdf16, g_rgb, B, g_normal, g_sdf16, gparams, scratch, scratch_bytes, stream, nullptr, 16, nullptr);
}

static int color_backward_impl(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
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
    hipLaunchKernelGGL(partials_reduce_kernel, dim3((NPART_C + RED_OUT - 1) / RED_OUT), dim3(1024), 0, (hipStream_t)stream, static_cast<const float *>(scratch),
                       blocks * TW, (uint32_t)NPART_C, gparams);
    return ac::check_launch("color_backward");
}

constexpr int COMP_LONG_MAX_T = 512;

// the long instantiation (composite_*_kernel<512, true>) where the short one does not apply
static bool comp_long(const CompArgs &a) { return a.T > 128 || a.T % 16; }

static int comp_args(CompArgs &a, const char *who, const float *rays_o, const float *rays_d, const float *z, const float *sdf, const float *nrm,
                     const float *col, const float *bg, int32_t n_rays, int32_t T0, int32_t T, float bound, float inv_s, float car)
{
    if (!rays_o || !rays_d || !z || !sdf || !nrm || !col) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    const bool short_ok = T0 > 0 && T % 16 == 0 && T >= T0 && T <= 128;
    const bool long_ok = T0 >= 2 && T >= T0 && (T - T0) % 16 == 0 && T <= COMP_LONG_MAX_T;          // ac_render_rays_long's counts
    if (!short_ok && !long_ok) {
        ac::set_error("%s: T0=%d T=%d unsupported (T a multiple of 16, <= 128; or T0 >= 2, T - T0 >= 0 a multiple of 16, T <= %d)", who, T0, T, COMP_LONG_MAX_T);
        return AC_ERR_BAD_ARG;
    }
    a.rays_o = rays_o; a.rays_d = rays_d; a.z = z; a.sdf = sdf; a.nrm = nrm; a.col = col; a.bg = bg;
    a.n_rays = n_rays; a.T0 = T0; a.T = T; a.bound = bound; a.inv_s = inv_s; a.car = car; a.one_m_car = (float)(1.0 - (double)car);
    a.inv_s_dev = nullptr;
    a.near_m = a.far_m = nullptr; a.mask = nullptr;
    return AC_OK;
}

AC_API int ac_composite_forward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf, const float *normal, const float *color,
                                const float *bg, int32_t n_rays, int32_t num_steps, int32_t T, float bound, float inv_s, float cos_anneal_ratio,
                                float *image, float *weights_sum, float *depth, float *normal_map, float *weights, float *alpha, ac_stream_t stream)
{
    if (n_rays <= 0) return AC_OK;
    CompArgs a{};
    if (int rc = comp_args(a, "composite_forward", rays_o, rays_d, z_vals, sdf, normal, color, bg, n_rays, num_steps, T, bound, inv_s, cos_anneal_ratio)) return rc;
    if (!image || !weights_sum || !depth || !normal_map || !weights || !alpha) { ac::set_error("composite_forward: NULL output"); return AC_ERR_BAD_ARG; }
    int blocks = (n_rays + 3) / 4; if (blocks > 4096) blocks = 4096;
    if (comp_long(a))
        hipLaunchKernelGGL((composite_fwd_kernel<COMP_LONG_MAX_T, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, image, weights_sum, depth, normal_map, weights, alpha);
    else
        hipLaunchKernelGGL((composite_fwd_kernel<128, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, image, weights_sum, depth, normal_map, weights, alpha);
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
    int blocks = (n_rays + 3) / 4; if (blocks > 4096) blocks = 4096;
    if (comp_long(a))
        hipLaunchKernelGGL((composite_bwd_kernel<COMP_LONG_MAX_T, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, g_image, g_weights_sum, g_depth,
                           g_normal_map, g_sdf, g_normal, g_color, g_inv_s_per_ray);
    else
        hipLaunchKernelGGL((composite_bwd_kernel<128, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, g_image, g_weights_sum, g_depth,
                           g_normal_map, g_sdf, g_normal, g_color, g_inv_s_per_ray);
    return ac::check_launch("composite_backward");
}

// ---- the whole render core backward -----------------------------------------------------------------------------------------------
namespace {
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
}  // namespace

// hash_stencil.hip: ac_hash_stencil_backward with the accumulation split at a level and a side stream ordered behind the first part
int hash_stencil_backward_split(const float *grad, const float *x, const int32_t *offsets_host, float *grad_embeddings, uint32_t B,
                                uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, void *scratch, size_t scratch_bytes,
                                ac_stream_t stream, uint32_t split_level, ac_stream_t side_stream);

AC_API size_t ac_render_core_backward_scratch(const ac_field *field, int32_t n_rays, int32_t T)
{
    if (!field || n_rays <= 0 || T <= 0) return 0;
    return core_layout(field, (uint32_t)n_rays * (uint32_t)T).total;
}

AC_API int ac_render_core_backward(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d, const float *bg,
                                   const ac_core_saved *sv, const ac_core_upstream *up, const ac_core_grads *gr, void *scratch, size_t scratch_bytes,
                                   ac_stream_t stream)
{
    if (!field || !op || !sv || !up || !gr) { ac::set_error("render_core_backward: NULL argument struct"); return AC_ERR_BAD_ARG; }
    if (op->n_rays <= 0) return AC_OK;
    const int N = op->n_rays, T0 = op->num_steps, T = T0 + op->upsample_steps;
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
    const uint32_t B = (uint32_t)N * (uint32_t)T;
    const CoreLayout l = core_layout(field, B);
    if (!scratch || scratch_bytes < l.total) { ac::set_error("render_core_backward: scratch of %zu bytes needed, %zu given", l.total, scratch_bytes); return AC_ERR_BAD_ARG; }
    char *sb = static_cast<char *>(scratch);
    float *nrm = reinterpret_cast<float *>(sb + l.nrm), *g_sdf = reinterpret_cast<float *>(sb + l.g_sdf), *g_nrm_a = reinterpret_cast<float *>(sb + l.g_nrm_a);
    float *g_col = reinterpret_cast<float *>(sb + l.g_col), *g_nrm_b = reinterpret_cast<float *>(sb + l.g_nrm_b), *g_s16 = reinterpret_cast<float *>(sb + l.g_s16);
    float *g_grad = reinterpret_cast<float *>(sb + l.g_grad), *gfeat = reinterpret_cast<float *>(sb + l.gfeat);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t eb = (B + 255) / 256;
    hipLaunchKernelGGL(core_normals_kernel, dim3(eb), dim3(256), 0, st, sv->gradient, B, nrm);
    {   // NeuS alpha + compositing (instant_nsr.py:219-263,290-299)
        CompArgs a{};
        if (int rc = comp_args(a, "render_core_backward", rays_o, rays_d, sv->z_vals, sv->sdf, nrm, sv->color, bg, N, T0, T, op->bound, op->inv_s, op->cos_anneal_ratio)) return rc;
        a.inv_s_dev = op->inv_s_dev;
        if ((op->near_m != nullptr) != (op->far_m != nullptr)) { ac::set_error("render_core_backward: near_m and far_m go together"); return AC_ERR_BAD_ARG; }
        a.near_m = op->near_m; a.far_m = op->far_m; a.mask = sv->mask;          // posed space: the range and the alpha mask of the forward
        int blocks = (N + 3) / 4; if (blocks > 4096) blocks = 4096;
        if (comp_long(a))
            hipLaunchKernelGGL((composite_bwd_kernel<COMP_LONG_MAX_T, true>), dim3(blocks), dim3(256), 0, st, a, up->g_image, up->g_weights_sum, up->g_depth,
                               up->g_normal_map, g_sdf, g_nrm_a, g_col, gr->g_inv_s_per_ray);
        else
            hipLaunchKernelGGL((composite_bwd_kernel<128, false>), dim3(blocks), dim3(256), 0, st, a, up->g_image, up->g_weights_sum, up->g_depth,
                               up->g_normal_map, g_sdf, g_nrm_a, g_col, gr->g_inv_s_per_ray);
    }
    if ((field->Wc1_sh != nullptr) != (sv->sh_bias != nullptr) || (field->Wc1_sh != nullptr) != (gr->g_sh_tiles != nullptr)) {
        ac::set_error("render_core_backward: a field with view directions (ac_field.Wc1_sh) needs ac_core_saved.sh_bias and ac_core_grads.g_sh_tiles, one without takes neither");
        return AC_ERR_BAD_ARG;
    }
    if (int rc = color_backward_impl(field, sv->pts, nrm, sv->sdf_out16, g_col, B, g_nrm_b, g_s16, gr->g_color_params, sb + l.part_col,
                                     ac_color_backward_scratch(B), stream, sv->sh_bias, (uint32_t)T, gr->g_sh_tiles)) return rc;
    if (up->eik_group_rays < 0 || (up->eik_group_rays > 0 && up->eik_den_stride < 1)) { ac::set_error("render_core_backward: eik_group_rays < 0 or eik_den_stride < 1"); return AC_ERR_BAD_ARG; }
    hipLaunchKernelGGL(core_mid_kernel, dim3(eb), dim3(256), 0, st, sv->gradient, sv->pts, g_sdf, g_nrm_a, g_nrm_b, up->g_eik, sv->eik_den, B, g_s16, g_grad,
                       (uint32_t)up->eik_group_rays * (uint32_t)T, (uint32_t)(up->eik_group_rays > 0 ? up->eik_den_stride : 0));
    if (int rc = sdf_stencil_backward_impl(field, sv->pts, g_s16, g_grad, B, op->bound, op->fd_eps, gfeat, gr->g_sdf_params, sb + l.part_sdf,
                                           ac_sdf_stencil_backward_scratch(B), stream, sv->feat7)) return rc;
    if (int rc = hash_stencil_backward_split(gfeat, sv->pts, field->offsets, gr->g_table, B, 2, 16, field->S, field->H, op->fd_eps, op->bound,
                                             l.hash_bytes ? sb + l.hash : nullptr, l.hash_bytes, stream,
                                             gr->side_stream ? (uint32_t)(gr->split_level > 0 ? gr->split_level : 0) : 0u, gr->side_stream)) return rc;
    return ac::check_launch("render_core_backward");
}
