// avatarcraft_amd/csrc/sdf_mlp.hpp -- the SDF network 35-64-16 on a tile of 16 points, on the matrix pipe: layer 1 (exact, and as a bf16-split update of the
// centre's layer 1 for the finite-difference points), softplus + layer 2 (all 16 outputs, or output 0 alone as a dot product), and forward_sdf of a tile
// (sdf_tile = hash gather + network).
// Included by field_grid.hip, field_color.hpp (the bf16 split and its vector types) and field_tile.hpp, and by the two ray renderers.
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "hash_gather.hpp"
#include "wave_ops.hpp"

namespace {

// ---- forward_sdf for a tile of 16 points: returns the 16 outputs as D2^T fragment (o = 4g+r) ----------

// SDF MLP 35-64-16 on the tile's features (f[j][c] = level 4j+g, channel c; bxyz = this lane group's coordinate),
// split into layer 1 (36 MFMA) and softplus + layer 2 (16 x ~40 VALU + 16 MFMA) so that the caller can overlap
// layer 1 of the NEXT evaluation (matrix pipe) with the softplus of the current one (vector pipe).
struct Acc4 { f32x4 a[4]; };

__device__ __forceinline__ Acc4 sdf_l1(const float *__restrict__ lds, int lane, float bxyz, const float (&f)[4][2])
{
    const int g = lane >> 4;
    Acc4 acc;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc.a[t] = *reinterpret_cast<const f32x4 *>(lds + OFF_B1 + 16 * t + 4 * g);
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        const float b = (s == 0) ? bxyz : f[(s - 1) >> 1][(s - 1) & 1];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            acc.a[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_W1F + (t * 9 + s) * 64 + lane], b, acc.a[t], 0, 0, 0);
    }
    return acc;
}

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// layer 1 of one finite-difference evaluation from the centre's layer 1 (acc0, exact fp32):
//   l1(x +- eps e_k) = acc0 + W1[:, features] (fe - fe0) + W1[:, k] (p_off - p)
// the middle product on the bf16 matrix pipe with both factors split hi + lo (3 of the 4 partial products; the dropped lo x lo is
// 2^-16 of a term that is itself ~1e-2 of l1).  The differences are split by truncation: d = hi + (d - hi) exactly, lo = the top 16
// bits of (d - hi).  B operand: this lane's eight differences = k 8g .. 8g+7, the order fill_lds_fast gives the A rows.
// 8 fp32 values -> their bf16 hi parts and the bf16 hi parts of the remainders, packed in B-operand order (value 2q in the low half of dword q)
__device__ __forceinline__ void split8_bf16(const float (&d)[8], u32x4 &bh, u32x4 &bl)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t u0 = __float_as_uint(d[2 * q]), u1 = __float_as_uint(d[2 * q + 1]);
        const float r0 = d[2 * q] - __uint_as_float(u0 & 0xffff0000u), r1 = d[2 * q + 1] - __uint_as_float(u1 & 0xffff0000u);
        bh[q] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);               // (top half of d[2q+1]) << 16 | top half of d[2q]
        bl[q] = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
    }
}

template <int W1H = OFF_W1H, int W1L = OFF_W1L, int W1C = OFF_W1C>
__device__ __forceinline__ Acc4 sdf_l1_delta(const float *__restrict__ lds, int lane, const Acc4 &acc0, const float (&fe)[4][2],
                                             const float (&fe0)[4][2], int kn, float dcoord)
{
    const int g = lane >> 4;
    u32x4 bh, bl;
    float dlt[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) { dlt[2 * q] = fe[q][0] - fe0[q][0]; dlt[2 * q + 1] = fe[q][1] - fe0[q][1]; }
    split8_bf16(dlt, bh, bl);
    const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh), Bl = __builtin_bit_cast(bf16x8, bl);
    Acc4 r;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const bf16x8 Ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + W1H + (t * 64 + lane) * 4));
        const bf16x8 Al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(lds + W1L + (t * 64 + lane) * 4));
        f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, acc0.a[t], 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, c, 0, 0, 0);
        const f32x4 wc = *reinterpret_cast<const f32x4 *>(lds + W1C + kn * 64 + 16 * t + 4 * g);     // W1[16t + 4g + r][kn]
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) c[rr] = fma_(dcoord, wc[rr], c[rr]);
        r.a[t] = c;
    }
    return r;
}

#ifndef AC_SP_BATCH
#define AC_SP_BATCH 4        // softplus values per LDS round trip (table rows in flight: 4 x 4 registers)
#endif
__device__ __forceinline__ f32x4 sdf_l2(const float *__restrict__ lds, int lane, const Acc4 &acc)
{
    const int g = lane >> 4;
    f32x4 o2 = *reinterpret_cast<const f32x4 *>(lds + OFF_B2 + 4 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float h[4];
        const float xin[4] = { acc.a[t][0], acc.a[t][1], acc.a[t][2], acc.a[t][3] };
        dv_softplus100_n<4>(lds + OFF_SPQ, xin, h);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            o2 = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[OFF_W2F + (4 * t + r) * 64 + lane], h[r], o2, 0, 0, 0);
    }
    return o2;
}

// Layer 2 for an evaluation whose only consumer is the sdf value (the six finite-difference points of a sample): output row 0 as
// a dot product on the vector pipe instead of 16 MFMA that would also produce the 15 unused feature rows (fp32 MFMA and fp32
// VALU share the datapath: 16 x 32 clocks against ~20 x 4).  Every lane sums its own 16 hidden units (16t + 4g + r: t outer, r inner),
// the four lane groups are joined as ((p0 + p1) + (p2 + p3)) + b2[0]; all lanes of a sample receive the same bits.
// oracle/ac_oracle.c: orc_sdf_mlp_sdf.
struct W2Row0 { float w[4][4]; };
__device__ __forceinline__ W2Row0 load_w2_row0(const float *__restrict__ lds, int lane)
{
    W2Row0 r;                                         // fragment (4t + r) holds W2[l & 15][16t + 4(l >> 4) + r]: row 0 sits in lane 16 g
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) r.w[t][q] = lds[OFF_W2F + (4 * t + q) * 64 + (lane & 48)];
    return r;
}
__device__ __forceinline__ float sdf_l2_sdf(const float *__restrict__ lds, const Acc4 &acc, const W2Row0 &w0)
{
    float p = 0.0f;
#pragma unroll
    for (int t0 = 0; t0 < 4; t0 += AC_SP_BATCH / 4) {
        constexpr int NB_ = AC_SP_BATCH;
        float xin[NB_], h[NB_];
#pragma unroll
        for (int i = 0; i < NB_; ++i) xin[i] = acc.a[t0 + (i >> 2)][i & 3];
        dv_softplus100_n<NB_>(lds + OFF_SPQ, xin, h);
#pragma unroll
        for (int i = 0; i < NB_; ++i) p = fma_(w0.w[t0 + (i >> 2)][i & 3], h[i], p);
    }
    const float other = __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, p), (0x10 << 10) | 0x1f));   // lane ^ 16
    // v_permlane32_swap exchanges lanes 32..63 of its first register with lanes 0..31 of its second: with s1 in both, the first ends up
    // holding the lower-half sums in both halves and the second the upper-half sums.  (Inline assembly: the builtin of this compiler
    // returns the first register for both results.  The s_nop covers the VALU write -> permlane read wait states.)
    int lo = __builtin_bit_cast(int, p + other), hi = lo;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo), "+v"(hi));
    return (__builtin_bit_cast(float, lo) + __builtin_bit_cast(float, hi)) + lds[OFF_B2];
}

__device__ __forceinline__ f32x4 sdf_mlp(const float *__restrict__ lds, int lane, float bxyz, const float (&f)[4][2])
{
    const Acc4 acc = sdf_l1(lds, lane, bxyz, f);
    __builtin_amdgcn_sched_barrier(0);
    return sdf_l2(lds, lane, acc);
}

template <bool H16 = false>
__device__ __forceinline__ f32x4 sdf_tile(const float *__restrict__ lds, const FieldCtx &fc, int lane, float px, float py, float pz)
{
    const int g = lane >> 4;
    float f[4][2];
    encode4<AC_ENC_ROUND, H16>(lds, fc.table, g, fc.jmode, px, py, pz, fc.bound, fc.two_bound, f, fc.inv_tb);
    __builtin_amdgcn_sched_barrier(0);
    return sdf_mlp(lds, lane, sel4(g, px, py, pz, 0.0f), f);
}

}  // namespace
