// avatarcraft_amd/csrc/mesh_pose.hip -- forward SMPL warp of an exported mesh's vertices for gfx950 (ac_mesh_bind, ac_mesh_pose).
//
// The posed renderer draws the surface { p : sdf(W^-1(p)) = 0 }, W^-1 = the SMPL-guided inverse warp of ac_warp_samples (warp.hip).  The posed position of a
// canonical vertex c is therefore the p with W^-1(p) = c: a fixed point of p <- fwd(M(p), c), M(p) = the blended transform at the closest face of the
// posed guide.  The closest-face searches are warp.hip's (over the structure that warp_accel_build.hip builds), launched through their public entries
// exactly as they are; this file adds the per-vertex
// arithmetic around them.  All of it in fp64 unless stated, every operation rounded once (-ffp-contract=off), so that it can be restated in numpy:
//
// Blended transform.  A face (i0, i1, i2) and a point q on it.  Barycentrics (bu, bv, bw) by mesh_blend.hpp's face_bary, the one formula warp.hip's finish_sample uses too: with a, b, c the
//   face's corners widened to fp64, v0 = b - a, v1 = c - a, v2 = q - a, d00 = v0.v0, d01 = v0.v1, d11 = v1.v1, d20 = v2.v0, d21 = v2.v1 (each dot product
//   x x + y y + z z, left to right), den = d00 d11 - d01 d01, bv = (d11 d20 - d01 d21) / den, bw = (d00 d21 - d01 d20) / den, bu = 1 - bv - bw.
//   M = T[i0] bu + T[i1] bv + T[i2] bw, element by element, in that order.  Write M = [[A, t], [., kappa]], so kappa = M[3][3].
// Forward application.  fwd(M, c) = A c + t / kappa: each coordinate is (A[r][0] c0 + A[r][1] c1) + A[r][2] c2 + t[r] / kappa, evaluated left to right,
//   then rounded to fp32.  This is the p that solves (M^-1 (p, 1))[:3] = c; it includes the reference's quirk that the Ts carry eye(4) / SMPL_SCALE.
// Normal.  n' = C n, C the cofactor matrix of A (the transposed adjugate: C[0][0] = A11 A22 - A12 A21, C[0][1] = A12 A20 - A10 A22, ... cyclically), each
//   coordinate (C[r][0] n0 + C[r][1] n1) + C[r][2] n2; then n' / (1e-30 + |n'|), |n'| = sqrt((x x + y y) + z z), rounded to fp32.
//
// ac_mesh_bind (once per exported mesh): closest face of the CANONICAL guide per vertex, then the barycentrics of the closest point (mesh_bary_kernel).
// ac_mesh_pose (once per frame): p_0 = fwd(M_bind, c) (mesh_pose_start_kernel); for k = 0 .. iters: search at p_k -> can_k = W^-1(p_k), closest point, face,
//   mask; mesh_pose_step_kernel: r_k = max_j |can_k[j] - c[j]|; a difference that is not finite: status 2, stop, keep p_k; r_k <= tol: status 0, stop;
//   k == iters: status 1, stop; otherwise p_{k+1} = fwd(M(p_k), c).  A vertex that stops gets residual = r_k, mask = the search's at p_k and its normal from
//   the A of M(p_k), the blend at the returned position; from then on it keeps its outputs and rides along.  Every launch covers all V vertices, lane =
//   vertex; no atomics, no waits, iters + 1 searches.
#include "ac_common.hpp"
#include "mesh_blend.hpp"

namespace {

constexpr uint8_t RUNNING = 255;     // scratch state of a vertex that still iterates (status values are 0, 1, 2)

// face_bary, Blend / blend3, fwd_store, normal_store: mesh_blend.hpp (shared with the posed first-hit render)

__global__ __launch_bounds__(256) void mesh_identity_kernel(double *__restrict__ T, uint32_t n16)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n16) T[e] = ((e & 15u) % 5u == 0u) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void mesh_bary_kernel(const double *__restrict__ closest, const int32_t *__restrict__ face_id,
                                                        const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V,
                                                        double *__restrict__ bary)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const size_t f = (size_t)face_id[v];                       // the search's own answer: always a face of the mesh
    const double q[3] = { closest[3 * (size_t)v], closest[3 * (size_t)v + 1], closest[3 * (size_t)v + 2] };
    double bc[3];
    face_bary(q, verts, faces[3 * f], faces[3 * f + 1], faces[3 * f + 2], bc);
    bary[3 * (size_t)v] = bc[0]; bary[3 * (size_t)v + 1] = bc[1]; bary[3 * (size_t)v + 2] = bc[2];
}

// p_0 = fwd(M_bind, c).  A binding face outside [0, F) (the host front end refuses it before anything is launched) stops the vertex at c with status 2
// instead of reading through it.
__global__ __launch_bounds__(256) void mesh_pose_start_kernel(const float *__restrict__ points, const int32_t *__restrict__ bind_face,
                                                              const double *__restrict__ bind_bary, const int32_t *__restrict__ faces,
                                                              const double *__restrict__ T, uint32_t V, uint32_t F, float *__restrict__ positions,
                                                              float *__restrict__ normals_out, float *__restrict__ residual, uint8_t *__restrict__ status,
                                                              uint8_t *__restrict__ mask, uint8_t *__restrict__ state)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float c[3] = { points[3 * (size_t)v], points[3 * (size_t)v + 1], points[3 * (size_t)v + 2] };
    const int32_t bf = bind_face[v];
    if (bf < 0 || (uint32_t)bf >= F) {
        positions[3 * (size_t)v] = c[0]; positions[3 * (size_t)v + 1] = c[1]; positions[3 * (size_t)v + 2] = c[2];
        if (normals_out) { normals_out[3 * (size_t)v] = 0.0f; normals_out[3 * (size_t)v + 1] = 0.0f; normals_out[3 * (size_t)v + 2] = 0.0f; }
        if (residual) residual[v] = __builtin_inff();
        if (status) status[v] = 2;
        if (mask) mask[v] = 0;
        state[v] = 2;
        return;
    }
    const double bc[3] = { bind_bary[3 * (size_t)v], bind_bary[3 * (size_t)v + 1], bind_bary[3 * (size_t)v + 2] };
    const Blend m = blend3(T, faces[3 * (size_t)bf], faces[3 * (size_t)bf + 1], faces[3 * (size_t)bf + 2], bc);
    fwd_store(m, c, positions + 3 * (size_t)v);
    state[v] = RUNNING;
}

__global__ __launch_bounds__(256) void mesh_pose_step_kernel(const float *__restrict__ points, const float *__restrict__ normals,
                                                             const double *__restrict__ can_pts, const double *__restrict__ closest,
                                                             const int32_t *__restrict__ face_id, const uint8_t *__restrict__ smask,
                                                             const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                             const double *__restrict__ T, uint32_t V, double tol, int last,
                                                             float *__restrict__ positions, float *__restrict__ normals_out, float *__restrict__ residual,
                                                             uint8_t *__restrict__ status, uint8_t *__restrict__ mask, uint8_t *__restrict__ state)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    if (state[v] != RUNNING) return;                           // stopped earlier: rides along
    const float c[3] = { points[3 * (size_t)v], points[3 * (size_t)v + 1], points[3 * (size_t)v + 2] };
    double r = 0.0;
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double d = __builtin_fabs(can_pts[3 * (size_t)v + j] - (double)c[j]);
        finite = finite && (d - d == 0.0);
        r = d > r ? d : r;
    }
    const uint8_t st = !finite ? 2 : (r <= tol ? 0 : (last ? 1 : RUNNING));
    const size_t f = (size_t)face_id[v];
    const int32_t f0v = faces[3 * f], f1v = faces[3 * f + 1], f2v = faces[3 * f + 2];
    const double q[3] = { closest[3 * (size_t)v], closest[3 * (size_t)v + 1], closest[3 * (size_t)v + 2] };
    double bc[3];
    face_bary(q, verts, f0v, f1v, f2v, bc);
    const Blend m = blend3(T, f0v, f1v, f2v, bc);
    if (st == RUNNING) { fwd_store(m, c, positions + 3 * (size_t)v); return; }
    state[v] = st;
    if (status) status[v] = st;
    if (residual) residual[v] = finite ? (float)r : __builtin_inff();
    if (mask) mask[v] = smask[v];
    if (normals_out) {
        if (finite) normal_store(m, normals + 3 * (size_t)v, normals_out + 3 * (size_t)v);
        else { normals_out[3 * (size_t)v] = 0.0f; normals_out[3 * (size_t)v + 1] = 0.0f; normals_out[3 * (size_t)v + 2] = 0.0f; }
    }
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// one closest-face search over P points with the outputs the steps read: the culled search where the structure covers the mesh, else the exhaustive one
int search(const float *pts, const float *verts, const int32_t *faces, const double *T, uint32_t P, uint32_t V, uint32_t F, double threshold,
           const void *accel, double *can, float *can_f32, double *closest, double *dist2, int32_t *face_id, uint8_t *mask, ac_stream_t stream)
{
    if (accel && ac_warp_accel_bytes(F) != 0)
        return ac_warp_samples_accel(pts, verts, faces, T, P, V, F, threshold, accel, can, can_f32, closest, dist2, face_id, mask, stream);
    return ac_warp_samples(pts, verts, faces, T, P, V, F, threshold, can, can_f32, closest, dist2, face_id, mask, stream);
}

}  // namespace

AC_API size_t ac_mesh_bind_scratch(uint32_t V, uint32_t Vg)
{
    // identity transforms [Vg,4,4] f64 | canonical points of the search [V,3] f32 (not used further) | closest [V,3] f64 | mask [V] u8
    return up256((size_t)Vg * 128) + up256((size_t)V * 12) + up256((size_t)V * 24) + up256((size_t)V);
}

AC_API int ac_mesh_bind(const float *points, uint32_t V, const float *guide_verts, uint32_t Vg, const int32_t *faces, uint32_t F, const void *accel,
                        int32_t *face_id, double *bary, double *dist2, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (V == 0) return AC_OK;
    if (!points || !guide_verts || !faces || !face_id || !bary || Vg == 0 || F == 0) { ac::set_error("mesh_bind: NULL buffer or empty guide"); return AC_ERR_BAD_ARG; }
    const size_t need = ac_mesh_bind_scratch(V, Vg);
    if (!scratch || scratch_bytes < need) { ac::set_error("mesh_bind: scratch smaller than %zu bytes", need); return AC_ERR_BAD_ARG; }
    char *b = static_cast<char *>(scratch);
    double *Tid = reinterpret_cast<double *>(b); b += up256((size_t)Vg * 128);
    float *can = reinterpret_cast<float *>(b); b += up256((size_t)V * 12);
    double *clo = reinterpret_cast<double *>(b); b += up256((size_t)V * 24);
    uint8_t *msk = reinterpret_cast<uint8_t *>(b);
    const hipStream_t st = (hipStream_t)stream;
    if (Vg > 0x0fffffffu) { ac::set_error("mesh_bind: %u guide vertices not supported", Vg); return AC_ERR_BAD_ARG; }
    const uint32_t n16 = Vg * 16u;
    hipLaunchKernelGGL(mesh_identity_kernel, dim3((n16 + 255) / 256), dim3(256), 0, st, Tid, n16);
    if (int rc = ac::check_launch("mesh_bind")) return rc;
    if (int rc = search(points, guide_verts, faces, Tid, V, Vg, F, 0.0, accel, nullptr, can, clo, dist2, face_id, msk, stream)) return rc;
    hipLaunchKernelGGL(mesh_bary_kernel, dim3((V + 255) / 256), dim3(256), 0, st, clo, face_id, guide_verts, faces, V, bary);
    return ac::check_launch("mesh_bind");
}

AC_API size_t ac_mesh_pose_scratch(uint32_t V)
{
    // W^-1(p) [V,3] f64 | closest [V,3] f64 | face [V] i32 | the search's mask [V] u8 | state [V] u8
    return 2 * up256((size_t)V * 24) + up256((size_t)V * 4) + 2 * up256((size_t)V);
}

AC_API int ac_mesh_pose(const float *points, const float *normals, uint32_t V, const int32_t *face_id, const double *bary, const ac_warp_mesh *mesh,
                        const ac_mesh_pose_opts *opts, void *scratch, size_t scratch_bytes, float *positions, float *normals_out, float *residual,
                        uint8_t *status, uint8_t *mask, ac_stream_t stream)
{
    if (!opts || opts->iters < 0 || opts->iters > 16 || !(opts->tol >= 0.0f)) { ac::set_error("mesh_pose: iters outside 0 .. 16 or tol not >= 0"); return AC_ERR_BAD_ARG; }
    if (V == 0) return AC_OK;
    if (!points || !face_id || !bary || !positions || !mesh || !mesh->verts || !mesh->faces || !mesh->T || mesh->F == 0) {
        ac::set_error("mesh_pose: NULL buffer or empty guide"); return AC_ERR_BAD_ARG;
    }
    if (normals_out && !normals) { ac::set_error("mesh_pose: posed normals need the canonical normals"); return AC_ERR_BAD_ARG; }
    const size_t need = ac_mesh_pose_scratch(V);
    if (!scratch || scratch_bytes < need) { ac::set_error("mesh_pose: scratch smaller than %zu bytes", need); return AC_ERR_BAD_ARG; }
    char *b = static_cast<char *>(scratch);
    double *can = reinterpret_cast<double *>(b); b += up256((size_t)V * 24);
    double *clo = reinterpret_cast<double *>(b); b += up256((size_t)V * 24);
    int32_t *fid = reinterpret_cast<int32_t *>(b); b += up256((size_t)V * 4);
    uint8_t *smask = reinterpret_cast<uint8_t *>(b); b += up256((size_t)V);
    uint8_t *state = reinterpret_cast<uint8_t *>(b);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((V + 255) / 256), block(256);
    hipLaunchKernelGGL(mesh_pose_start_kernel, grid, block, 0, st, points, face_id, bary, mesh->faces, mesh->T, V, mesh->F, positions, normals_out, residual,
                       status, mask, state);
    if (int rc = ac::check_launch("mesh_pose")) return rc;
    for (int k = 0; k <= opts->iters; ++k) {
        if (int rc = search(positions, mesh->verts, mesh->faces, mesh->T, V, mesh->V, mesh->F, mesh->threshold, mesh->accel, can, nullptr, clo, nullptr, fid,
                            smask, stream)) return rc;
        hipLaunchKernelGGL(mesh_pose_step_kernel, grid, block, 0, st, points, normals, can, clo, fid, smask, mesh->verts, mesh->faces, mesh->T, V,
                           (double)opts->tol, k == opts->iters ? 1 : 0, positions, normals_out, residual, status, mask, state);
        if (int rc = ac::check_launch("mesh_pose")) return rc;
    }
    return AC_OK;
}
