// avatarcraft_amd/csrc/occlusion_tile.hpp -- ambient occlusion of one tile of 16 points from cone taps into the SDF: the kit (directions, weights, distances) as a
// kernel argument and in LDS, and the tile body.  The quantity, operation by operation: include/avatarcraft_hip.h, ac_field_occlusion.
// Included by mesh_occlusion.hip.  Anonymous namespace, like shade_tile.hpp: each translation unit gets its own copy.
#pragma once
#include "shade_tile.hpp"

namespace {

constexpr int OCC_MAX_DIRS = 32, OCC_MAX_STEPS = 16;
constexpr int OCC_DIRS = 0, OCC_WEIGHTS = 3 * OCC_MAX_DIRS, OCC_DISTS = OCC_WEIGHTS + OCC_MAX_DIRS, OCC_FLOATS = OCC_DISTS + OCC_MAX_STEPS;

// the kit by value in the kernel's arguments: the tables are 576 bytes; K == 0: no occlusion in this launch
struct OccKit {
    int K, J;                   // directions, taps per direction
    float gain, level;
    float tab[OCC_FLOATS];      // dirs [32][3] | weights [32] | dists [16]; zero past K and J
};

// the tables -> LDS at kit[0 .. OCC_FLOATS), before the workgroup's barrier.  The body indexes them by k and j: a dynamic index into the by-value argument would
// copy it to scratch, so the argument is read with static indices only (like the level records of fill_lds_sdf).
__device__ __forceinline__ void fill_lds_kit(float *kit, const OccKit &k)
{
#pragma unroll
    for (int i = 0; i < OCC_FLOATS; ++i)
        if (threadIdx.x == (unsigned)i) kit[i] = k.tab[i];
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    const float inf = __builtin_inff();
    return __builtin_fabsf(x) < inf && __builtin_fabsf(y) < inf && __builtin_fabsf(z) < inf;
}

// "occlusion of one tile of 16 points".  In: lane (n, g)'s point p (clamped) and unit normal (the four lanes of a point agree) and whether the point is active.
// Out: the occlusion of an active point, 0 for an inactive one.  Inactive lanes ride along at the first active lane's point and normal; a tile without an active
// point issues no evaluation.  K J sdf_tile calls, all of them by every lane of the wave; the one early exit (the rest of a direction once its v is 0 in every
// active lane: fminf(0, r) stays 0 for every r in [0, 1]) is wave-uniform and changes no bit.  All fp32, every operation rounded once.
__device__ __forceinline__ float occlusion_tile(const float *__restrict__ lds, const float *__restrict__ kit, const FieldCtx &fc, int lane, int K, int J,
                                                float gain, float level, float bound, bool active, float px, float py, float pz, float nx, float ny, float nz)
{
    const int n = lane & 15;
    if (!ride_along(active, px, py, pz)) return 0.0f;                            // (wave-uniform)
    ride_along(active, nx, ny, nz);
    // the frame whose z axis is the normal; |sg + nz| >= 1
    const float sg = __builtin_copysignf(1.0f, nz);
    const float a = -1.0f / (sg + nz);
    const float b = (nx * ny) * a;
    const float tx = 1.0f + sg * ((nx * nx) * a), ty = sg * b, tz = -(sg * nx);
    const float ux = b, uy = sg + (ny * ny) * a, uz = -ny;
    float acc = 0.0f;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const float lx = kit[OCC_DIRS + 3 * k], ly = kit[OCC_DIRS + 3 * k + 1], lz = kit[OCC_DIRS + 3 * k + 2];
        const float wx = (lx * tx + ly * ux) + lz * nx, wy = (lx * ty + ly * uy) + lz * ny, wz = (lx * tz + ly * uz) + lz * nz;
        float v = 1.0f;
#pragma unroll 1
        for (int j = 0; j < J; ++j) {
            const float t = kit[OCC_DISTS + j];
            // (NaN-proof: fmaxf drops a NaN operand, so a NaN coordinate becomes -bound)
            const float qx = __builtin_fminf(__builtin_fmaxf(px + t * wx, -bound), bound);
            const float qy = __builtin_fminf(__builtin_fmaxf(py + t * wy, -bound), bound);
            const float qz = __builtin_fminf(__builtin_fmaxf(pz + t * wz, -bound), bound);
            const f32x4 o = sdf_tile(lds, fc, lane, qx, qy, qz);
            const float s = __shfl(o[0], n) - level;                             // output 0 lives in the lanes g == 0
            const float h = t * lz;
            v = __builtin_fminf(v, __builtin_fminf(__builtin_fmaxf((gain * s) / h, 0.0f), 1.0f));      // (a NaN value: fully occluded)
            if (__ballot(active && v != 0.0f) == 0ull) break;                   // (wave-uniform)
        }
        acc = acc + kit[OCC_WEIGHTS + k] * v;
    }
    return active ? __builtin_fminf(acc, 1.0f) : 0.0f;
}

}  // namespace
