// avatarcraft_amd/csrc/sdf_stencil_train.hip -- the fused SDF query of the differentiable render core (training path), forward and backward, and the
// reduction of the backward kernels' per-wave weight-gradient partials.  (The colour network: color_train.hip; the compositor: composite.hip; the whole-core
// backward that chains them: render_core_backward.hip.)
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
// Weight-gradient partials are written per wave (no atomics) and summed by partials_reduce_kernel (deterministic).
#include "train_common.hpp"
#include "field_tile.hpp"
#include "field_host.hpp"

namespace {

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
//   * NOT a second wave per SIMD (8 waves per workgroup: 256 registers, occupancy 2 -- and 148 spilled registers, 368 bytes of scratch per lane: the kernel's
//     natural live set is ~370 registers; backward of the SDS step 2.24 -> 3.10 ms: profiles/r06_experiments.txt section 3a, built there as AC_SDFBWD_WAVES=8; TW_S below is what is left of that switch);
//   * room for a second buffer of the d1 / input transposes, so that the weight-gradient products of evaluation e (48 fp32 MFMA of 32 clocks, a quarter of
//     the evaluation's time, with nothing beside them on the wave's only instruction stream) are issued INSIDE evaluation e + 1's recomputation
//     (softplus, splits: vector work) instead of behind a barrier at the end of their own evaluation.
constexpr int TW_S = TW;                                               // waves per workgroup of sdf_stencil_bwd_kernel<SAVED = true>
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
            // db2: the centre evaluation alone.  The two offset evaluations of an axis carry +s and -s on output 0 (exact negatives, s = g_k / (2 eps) ~ 100 x
            // the centre's upstream): their shares cancel exactly, and adding them to the running sum left only the rounding of (sum + s) - s behind --
            // db2[0] was 10 x further from float64 autograd than float32 autograd is (tests/test_gpu_field_ops.py)
            if (!rank1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gb2[r] += d2[r];
            }
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

// out[i] = sum over waves of partials[w][i], i < n_out (this file's NPART, the colour backward's NPART_C): RED_OUT outputs x RED_SL wave slices per workgroup, fixed summation order (deterministic).  Round 4: 16 x 64
// instead of 64 x 16 -- four times the workgroups and a quarter of the dependent trip count per thread (21 -> ~8 us for 1024 partial sets)
constexpr uint32_t RED_OUT = 16, RED_SL = 64;
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

}  // namespace

void partials_reduce(const float *partials, uint32_t nwaves, uint32_t n_out, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(partials_reduce_kernel, dim3((n_out + RED_OUT - 1) / RED_OUT), dim3(1024), 0, st, partials, nwaves, n_out, out);
}

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
    return (size_t)train_grid(B) * TW * NPART * sizeof(float);
}

int sdf_stencil_backward_impl(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                              float eps, float *gfeat, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream, const float *feat7,
                              float *g_x)
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
    const uint32_t blocks = train_grid(B);
    if (feat7) {
        hipLaunchKernelGGL(sdf_stencil_bwd_kernel<true>, dim3(blocks), dim3(TBLOCK), lds_bytes_s, (hipStream_t)stream, a, x, g_out16, g_grad, B, eps, gfeat,
                           static_cast<float *>(scratch), feat7, (float *)nullptr);
    } else if (g_x) {
        static uint64_t seen_x = 0;
        ac::allow_dynamic_lds(seen_x, reinterpret_cast<const void *>(sdf_stencil_bwd_kernel<false, true>), lds_bytes);
        hipLaunchKernelGGL((sdf_stencil_bwd_kernel<false, true>), dim3(blocks), dim3(TBLOCK), lds_bytes, (hipStream_t)stream, a, x, g_out16, g_grad, B, eps, gfeat,
                           static_cast<float *>(scratch), feat7, g_x);
    } else
        hipLaunchKernelGGL(sdf_stencil_bwd_kernel<false>, dim3(blocks), dim3(TBLOCK), lds_bytes, (hipStream_t)stream, a, x, g_out16, g_grad, B, eps, gfeat,
                           static_cast<float *>(scratch), feat7, (float *)nullptr);
    partials_reduce(static_cast<const float *>(scratch), blocks * TW, (uint32_t)NPART, gparams, (hipStream_t)stream);
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
