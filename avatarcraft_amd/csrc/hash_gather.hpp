// avatarcraft_amd/csrc/hash_gather.hpp -- the hash-grid gather of one point: a table entry through the buffer descriptor (fp32 or half table), the trilinear
// interpolation of a cell's eight corners, and the features of a lane's four levels (encode4).
// Included by sdf_mlp.hpp (sdf_tile) and field_stencil.hpp (the seven-point stencil uses the same entry load and interpolation).
// Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "field_lds.hpp"

namespace {

// ---- hash-grid features of this lane's 4 levels (HashEncoder.forward + kernel_grid) -------------------
// p: world position (clamped to +-bound); returns f[j][c] for level 4j+g.  The gathers go through a
// buffer descriptor (32-bit byte offsets, hardware bounds check) and are issued ROUND levels at a time.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32q __attribute__((ext_vector_type(4)));
// dense levels' corner pairs through one 16-byte gather: bit-identical, no gain -- profiles/r04_experiments.txt section 7b
// packed-fp32 interpolation (v_pk_mul_f32 / v_pk_fma_f32): bit-identical, slower -- profiles/r06_experiments.txt section 4d
__device__ __forceinline__ void interp8(const u32x2 (&v)[8], float qx, float qy, float qz, bool oob, float &f0, float &f1)
{
    const float wx0 = 1.0f - qx, wy0 = 1.0f - qy, wz0 = 1.0f - qz;
    const float w00 = wx0 * wy0, w10 = qx * wy0, w01 = wx0 * qy, w11 = qx * qy;
    float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float wxy = (c & 2) ? ((c & 1) ? w11 : w01) : ((c & 1) ? w10 : w00);
        const float w = wxy * ((c & 4) ? qz : wz0);
        a0 = fma_(w, __uint_as_float(v[c].x), a0);
        a1 = fma_(w, __uint_as_float(v[c].y), a1);
    }
    f0 = oob ? 0.0f : a0;
    f1 = oob ? 0.0f : a1;
}
// one table entry = the bit patterns of its two fp32 features.  H16 = false: the fp32 table, one 8-byte gather.  H16 = true: the half table of
// ac_table_to_half (one dword per entry, channel 0 in the low half; descriptor of n_entries x 4 bytes): one 4-byte gather, widened by two f16 -> f32
// conversions (exact, subnormals included) into the registers the fp32 path fills -- everything behind the load is the same code in both forms
template <bool H16>
__device__ __forceinline__ u32x2 table_entry(rsrc_t table, uint32_t idx)
{
    if constexpr (H16) {
        const uint32_t d = __builtin_amdgcn_raw_buffer_load_b32(table, idx * 4u, 0, 0);
        const float c0 = (float)__builtin_bit_cast(_Float16, (unsigned short)(d & 0xffffu)), c1 = (float)__builtin_bit_cast(_Float16, (unsigned short)(d >> 16));
        return u32x2{ __float_as_uint(c0), __float_as_uint(c1) };
    } else return __builtin_amdgcn_raw_buffer_load_b64(table, idx * 8u, 0, 0);
}
template <int ROUND, bool H16 = false>
__device__ __forceinline__ void encode4(const float *__restrict__ lds, rsrc_t table, int g, const int (&jmode)[4],
                                        float px, float py, float pz, float bound, float two_bound, float (&f)[4][2], float inv_tb = 0.0f)
{
    float ux, uy, uz;
    if (inv_tb != 0.0f) { ux = unit_div(px + bound, two_bound, inv_tb); uy = unit_div(py + bound, two_bound, inv_tb); uz = unit_div(pz + bound, two_bound, inv_tb); }
    else { ux = (px + bound) / two_bound; uy = (py + bound) / two_bound; uz = (pz + bound) / two_bound; }
    const bool oob = (ux < 0.0f) | (ux > 1.0f) | (uy < 0.0f) | (uy > 1.0f) | (uz < 0.0f) | (uz > 1.0f);
#pragma unroll
    for (int j0 = 0; j0 < 4; j0 += ROUND) {
        float q[ROUND][3];
        u32x2 v[ROUND][8];
#pragma unroll
        for (int jj = 0; jj < ROUND; ++jj) {
            const int j = j0 + jj;
            const uint4 r0 = *reinterpret_cast<const uint4 *>(lds + OFF_LVL + (4 * j + g) * 8);
            const uint4 r1 = *reinterpret_cast<const uint4 *>(lds + OFF_LVL + (4 * j + g) * 8 + 4);
            const float scale = __uint_as_float(r0.x);
            const uint32_t my = r0.y, mz = r0.z, offset = r0.w, mask = r1.x, hashed = r1.y;
            float qx = fma_(ux, scale, 0.5f), qy = fma_(uy, scale, 0.5f), qz = fma_(uz, scale, 0.5f);
            const uint32_t gx = (uint32_t)__builtin_floorf(qx), gy = (uint32_t)__builtin_floorf(qy), gz = (uint32_t)__builtin_floorf(qz);
            q[jj][0] = qx - (float)gx; q[jj][1] = qy - (float)gy; q[jj][2] = qz - (float)gz;
            const uint32_t ax0 = gx, ax1 = gx + 1u, ay0 = gy * my, ay1 = ay0 + my, az0 = gz * mz, az1 = az0 + mz;
            const int mode = jmode[j];                      // wave-uniform: one code path per gather round
            uint32_t idx[8];
            if (mode == 0) {                                // all four levels of this round are dense
#pragma unroll
                for (int c = 0; c < 8; ++c) idx[c] = ((c & 1) ? ax1 : ax0) + ((c & 2) ? ay1 : ay0) + ((c & 4) ? az1 : az0);
            } else if (mode == 1) {                         // all hashed
#pragma unroll
                for (int c = 0; c < 8; ++c) idx[c] = (((c & 1) ? ax1 : ax0) ^ ((c & 2) ? ay1 : ay0) ^ ((c & 4) ? az1 : az0)) & mask;
            } else {                                        // mixed round (levels 4..7 of the default model)
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const uint32_t tx = (c & 1) ? ax1 : ax0, ty = (c & 2) ? ay1 : ay0, tz = (c & 4) ? az1 : az0;
                    idx[c] = (hashed ? (tx ^ ty ^ tz) : (tx + ty + tz)) & mask;
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) v[jj][c] = table_entry<H16>(table, offset + idx[c]);
        }
#pragma unroll
        for (int jj = 0; jj < ROUND; ++jj)
            interp8(v[jj], q[jj][0], q[jj][1], q[jj][2], oob, f[j0 + jj][0], f[j0 + jj][1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace
