// avatarcraft_amd/csrc/mesh_blend.hpp -- the blended SMPL transform at a point of a guide face and what is formed from it, shared by the mesh posing
// (mesh_pose.hip) and the posed first-hit render (surface_rays.hip).  All fp64, every operation rounded once (-ffp-contract=off), in the order
// include/avatarcraft_hip.h states (ac_mesh_pose: Blended transform, Forward application, Normal).  Anonymous namespace: each translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace {

#define AC_DOT3(u, v) ((u)[0] * (v)[0] + (u)[1] * (v)[1] + (u)[2] * (v)[2])

// barycentrics of q on the face (f0v, f1v, f2v); the inverse warp (warp.hip's finish_sample) and the forward one share this formula
__device__ __forceinline__ void face_bary(const double (&q)[3], const float *__restrict__ verts, int32_t f0v, int32_t f1v, int32_t f2v, double (&bc)[3])
{
    double a[3], b[3], c[3], v0[3], v1[3], v2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[k] = (double)verts[3 * (size_t)f0v + k]; b[k] = (double)verts[3 * (size_t)f1v + k]; c[k] = (double)verts[3 * (size_t)f2v + k];
        v0[k] = b[k] - a[k]; v1[k] = c[k] - a[k]; v2[k] = q[k] - a[k];
    }
    const double d00 = AC_DOT3(v0, v0), d01 = AC_DOT3(v0, v1), d11 = AC_DOT3(v1, v1), d20 = AC_DOT3(v2, v0), d21 = AC_DOT3(v2, v1);
    const double den = d00 * d11 - d01 * d01;
    const double bv = (d11 * d20 - d01 * d21) / den, bw = (d00 * d21 - d01 * d20) / den;
    bc[0] = 1.0 - bv - bw; bc[1] = bv; bc[2] = bw;
}

// the rows of M that fwd and the normal need: A (3x3), t (3), kappa
struct Blend { double A[9], t[3], kappa; };
__device__ __forceinline__ Blend blend3(const double *__restrict__ T, int32_t f0v, int32_t f1v, int32_t f2v, const double (&bc)[3])
{
    const double *T0 = T + 16 * (size_t)f0v, *T1 = T + 16 * (size_t)f1v, *T2 = T + 16 * (size_t)f2v;
    Blend m;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int j = 0; j < 3; j++) m.A[3 * r + j] = T0[4 * r + j] * bc[0] + T1[4 * r + j] * bc[1] + T2[4 * r + j] * bc[2];
        m.t[r] = T0[4 * r + 3] * bc[0] + T1[4 * r + 3] * bc[1] + T2[4 * r + 3] * bc[2];
    }
    m.kappa = T0[15] * bc[0] + T1[15] * bc[1] + T2[15] * bc[2];
    return m;
}

__device__ __forceinline__ void fwd_store(const Blend &m, const float (&c)[3], float *__restrict__ p)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        p[r] = (float)((m.A[3 * r] * (double)c[0] + m.A[3 * r + 1] * (double)c[1]) + m.A[3 * r + 2] * (double)c[2] + m.t[r] / m.kappa);
}

__device__ __forceinline__ void normal_store(const Blend &m, const float *__restrict__ n, float *__restrict__ out)
{
    const double *A = m.A;
    const double C[9] = { A[4] * A[8] - A[5] * A[7], A[5] * A[6] - A[3] * A[8], A[3] * A[7] - A[4] * A[6],
                          A[7] * A[2] - A[8] * A[1], A[8] * A[0] - A[6] * A[2], A[6] * A[1] - A[7] * A[0],
                          A[1] * A[5] - A[2] * A[4], A[2] * A[3] - A[0] * A[5], A[0] * A[4] - A[1] * A[3] };
    const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
    double w[3];
#pragma unroll
    for (int r = 0; r < 3; r++) w[r] = (C[3 * r] * n0 + C[3 * r + 1] * n1) + C[3 * r + 2] * n2;
    const double len = 1e-30 + __builtin_sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = (float)(w[r] / len);
}

}  // namespace
