// avatarcraft_amd/csrc/wave_ops.hpp -- operations inside one wave of 64 lanes: the LDS hand-over between its lanes (wave_sync), DPP row shifts and scans,
// lane broadcast, the lane-group select and the 64-bin chunk scan of up_sample.  No field, no LDS layout.
// Included by composite.hip, table_scatter.hpp (hash_stencil.hip), warp.hip, sdf_mlp.hpp and field_color.hpp, and through those two by everything that
// evaluates the field.  Anonymous namespace: each translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ---- wave-level helpers -----------------------------------------------------------------------------
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int OFF> __device__ __forceinline__ float dpp_shr(float ident, float v)
{
    // lanes n >= OFF of every 16-lane row receive v[n-OFF]; the others keep `ident`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ident), __builtin_bit_cast(int, v),
                                                                  0x110 + OFF, 0xf, 0xf, false));
}
// Kogge-Stone inclusive scan inside every 16-lane row
template <bool MUL> __device__ __forceinline__ float row_scan(float v)
{
    const float id = MUL ? 1.0f : 0.0f;
    float s;
    s = dpp_shr<1>(id, v); v = MUL ? s * v : s + v;
    s = dpp_shr<2>(id, v); v = MUL ? s * v : s + v;
    s = dpp_shr<4>(id, v); v = MUL ? s * v : s + v;
    s = dpp_shr<8>(id, v); v = MUL ? s * v : s + v;
    return v;
}
__device__ __forceinline__ float lane_bcast(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ float sel4(int g, float a, float b, float c, float d)
{
    return g == 0 ? a : (g == 1 ? b : (g == 2 ? c : d));
}

// ---- one 64-bin chunk of the per-bin scans of up_sample: row-local inclusive scan + cross-row carry ----
// v: this lane's element (identity-padded); carry/first: state entering the chunk; returns the inclusive
// tile-scan value and the value entering this lane's row (rc), updates carry/first.
template <bool MUL>
__device__ __forceinline__ float chunk_scan(float v, int lane, float &carry, bool &first, float &loc, float &row_in, bool &row_first)
{
    loc = row_scan<MUL>(v);
    const float t0 = lane_bcast(loc, 15), t1 = lane_bcast(loc, 31), t2 = lane_bcast(loc, 47), t3 = lane_bcast(loc, 63);
    const float c0 = carry; const bool f0 = first;
    const float c1 = f0 ? t0 : (MUL ? c0 * t0 : c0 + t0);
    const float c2 = MUL ? c1 * t1 : c1 + t1;
    const float c3 = MUL ? c2 * t2 : c2 + t2;
    const float c4 = MUL ? c3 * t3 : c3 + t3;
    const int g = lane >> 4;
    row_in = sel4(g, c0, c1, c2, c3);
    row_first = f0 && g == 0;
    carry = c4; first = false;
    return row_first ? loc : (MUL ? row_in * loc : row_in + loc);
}

}  // namespace
