// avatarcraft_amd/csrc/warp.hip -- SMPL-guided sample warp and mesh-guided near/far for gfx950.
//
// Replaces two CPU stages of the reference's animation path (render_warp.py -> NeRFRenderer.run with render_can=False):
//   geometry_guided_near_far_torch (utils/ray_utils.py:277-294): O(N*V) with three [N,V,3] temporaries (0.68 GB each at
//     N=8192) -> mesh_near_far_kernel: lane = ray, 16 waves share 64 rays and split the vertices (LDS tiles), no temporaries;
//   warp_samples_to_canonical (utils/ray_utils.py:62-90): libigl closest-point query + numpy fp64 4x4 inverse on the CPU
//     with two PCIe round trips per ray batch (models/instant_nsr.py:166-172,198-203) -> warp_samples_kernel: one lane
//     per sample, the triangle soup streamed through LDS tiles, exact closest point / barycentric blend / 4x4 inverse in
//     fp64 on the device (fp64 vector rate of MI355X: 78 TFLOP/s).
// Arithmetic order follows oracle/ac_oracle_ops.c (orc_mesh_near_far, orc_warp_samples) operation for operation
// (-ffp-contract=off), so results are bit-identical to the CPU oracle.  warp_samples_kernel is the exhaustive search;
// warp_samples_accel_kernel (further down) returns the same bits from an exact culled search, a wave owning 64 samples, through
// the per-frame structure of warp_accel.hpp (built by warp_accel_build.hip); ray_cull_kernel reads the same structure.
#include "ac_common.hpp"
#include "mesh_blend.hpp"
#include "warp_accel.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int VT = 1024;   // vertices per LDS tile (12 KB)
constexpr int FT = 512;    // faces per LDS tile (9 floats each, 18 KB)

// one workgroup = 64 rays x 16 waves: every wave scans a 1/16 slice of each vertex tile for the same 64 rays (lane = ray), the
// per-wave min / max meet in LDS.  min / max are exact and order independent: the result does not depend on the split.
constexpr int NF_WAVES = 16;
__global__ __launch_bounds__(NF_WAVES * 64) void mesh_near_far_kernel(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                                      const float *__restrict__ verts, uint32_t N, uint32_t V, float r2,
                                                                      float *__restrict__ near, float *__restrict__ far)
{
    __shared__ float sv[VT * 3];
    __shared__ float sg[VT / 32][4];                      // bounding sphere of every run of 32 consecutive vertices of the tile (centre, padded radius)
    __shared__ float snr[NF_WAVES][64], sfr[NF_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = blockIdx.x * 64 + lane;
    const bool live = n < N;
    const uint32_t nn = live ? n : 0;
    const float ox = rays_o[3 * nn], oy = rays_o[3 * nn + 1], oz = rays_o[3 * nn + 2];
    const float dx = rays_d[3 * nn], dy = rays_d[3 * nn + 1], dz_ = rays_d[3 * nn + 2];
    float nr = __builtin_inff(), fr = -__builtin_inff();
    const float rad = __builtin_sqrtf(r2) * (1.0f + 1e-6f);
    // gridDim.y > 1: this workgroup scans ONE vertex tile and the tiles' results meet in near / far through atomic min / max (both exact and order
    // independent; the host presets +inf / -inf).  A 8192-ray batch is only 128 workgroups otherwise -- half the device idle, and seven dependent
    // load -> barrier -> scan rounds each.
    const uint32_t v_begin = gridDim.y > 1 ? blockIdx.y * (uint32_t)VT : 0u;
    const uint32_t v_end = gridDim.y > 1 ? (v_begin + (uint32_t)VT < V ? v_begin + (uint32_t)VT : V) : V;
    // the run test below bounds a DISTANCE; the per-vertex formula (the reference's) is one only for unit directions: with |d|^2 = 1 +- 2e-6 the two
    // differ by < 2e-6 z0^2, inside the 1e-5 s2 slack of the test.  Other rays (never produced by the drivers): every run is scanned.
    const bool cull_ok = __all(!live || __builtin_fabsf(((dx * dx + dy * dy) + dz_ * dz_) - 1.0f) <= 2e-6f) != 0;
    for (uint32_t v0 = v_begin; v0 < v_end; v0 += VT) {
        const uint32_t cnt = (v_end - v0 < (uint32_t)VT) ? v_end - v0 : (uint32_t)VT;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt * 3; i += blockDim.x) sv[i] = verts[(size_t)v0 * 3 + i];
        __syncthreads();
        // mesh vertex order is spatially coherent (body parts): a run of 32 vertices sits in a small sphere, and the 64 rays of a wave are a thin fan
        // (neighbouring pixels) -- most runs are missed by the whole fan and cost one test instead of 32
        const uint32_t ngr = (cnt + 31u) >> 5;
        if (threadIdx.x < ngr) {
            const uint32_t b0 = threadIdx.x * 32u, b1 = (b0 + 32u < cnt) ? b0 + 32u : cnt;
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
            for (uint32_t v = b0; v < b1; ++v) { cx += sv[3 * v]; cy += sv[3 * v + 1]; cz += sv[3 * v + 2]; }
            const float inv = 1.0f / (float)(b1 - b0);
            cx *= inv; cy *= inv; cz *= inv;
            float m2 = 0.0f;
            for (uint32_t v = b0; v < b1; ++v) {
                const float ex = sv[3 * v] - cx, ey = sv[3 * v + 1] - cy, ez = sv[3 * v + 2] - cz, e2 = (ex * ex + ey * ey) + ez * ez;
                m2 = e2 > m2 ? e2 : m2;                    // NaN vertices compare false: they are handled (ignored) by the per-vertex code below
            }
            sg[threadIdx.x][0] = cx; sg[threadIdx.x][1] = cy; sg[threadIdx.x][2] = cz;
            sg[threadIdx.x][3] = __builtin_sqrtf(m2) * (1.0f + 1e-5f) + 1e-6f;
        }
        __syncthreads();
        for (uint32_t gi = wave; gi < ngr; gi += NF_WAVES) {
            {   // the whole run: a ray farther than R + r from the centre (as a line, like the per-vertex formula) touches none of its spheres
                const float x = sg[gi][0] - ox, y = sg[gi][1] - oy, z = sg[gi][2] - oz;
                const float z0 = (x * dx + y * dy) + z * dz_, s2 = (x * x + y * y) + z * z;
                const float rr = sg[gi][3] + rad;
                // (a NaN centre -- a NaN vertex in the run -- compares false everywhere: `!(... > ...)` keeps the run)
                if (cull_ok && !__any(!((s2 - z0 * z0) > rr * rr * (1.0f + 1e-5f) + 1e-5f * s2 + 1e-10f))) continue;
            }
            const uint32_t e1 = (gi * 32u + 32u < cnt) ? gi * 32u + 32u : cnt;
        for (uint32_t v = gi * 32u; v < e1; ++v) {
            const float x = sv[3 * v] - ox, y = sv[3 * v + 1] - oy, z = sv[3 * v + 2] - oz;
            const float z0 = (x * dx + y * dy) + z * dz_;
            const float s2 = (x * x + y * y) + z * z;
            // the sphere of this vertex is missed for sure (negative radicand -> NaN -> ignored below) when the squared distance of the
            // vertex from the ray exceeds r^2 by more than the rounding of nrm * nrm; most vertices are far from all 64 rays of the
            // wave, and then both square roots are skipped (wave-uniform branch; the arithmetic of the kept path is unchanged)
            if (!__any((s2 - z0 * z0) - r2 <= 1e-6f * s2 + 1e-12f)) continue;
            const float nrm = __builtin_sqrtf(s2);
            const float dz = __builtin_sqrtf(r2 - (nrm * nrm - z0 * z0));
            const float a = z0 - dz, b = z0 + dz;
            if (a == a && a < nr) nr = a;
            if (b == b && b > fr) fr = b;
        }
        }
    }
    snr[wave][lane] = nr; sfr[wave][lane] = fr;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 1; w < NF_WAVES; ++w) { const float a = snr[w][lane], b = sfr[w][lane]; nr = a < nr ? a : nr; fr = b > fr ? b : fr; }
        if (gridDim.y == 1) { near[n] = nr; far[n] = fr; }
        else {
            uint32_t *pn = reinterpret_cast<uint32_t *>(near + n), *pf = reinterpret_cast<uint32_t *>(far + n);
            for (uint32_t old = *pn; nr < __uint_as_float(old);) { const uint32_t was = atomicCAS(pn, old, __float_as_uint(nr)); if (was == old) break; old = was; }
            for (uint32_t old = *pf; fr > __uint_as_float(old);) { const uint32_t was = atomicCAS(pf, old, __float_as_uint(fr)); if (was == old) break; old = was; }
        }
    }
}

// 4x4 inverse: Gauss-Jordan with partial pivoting on an augmented [4][8] system (oracle: inv4)
__device__ __forceinline__ bool inv4(const double (&m)[16], double (&out)[16])
{
    double a[4][8];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { a[i][j] = m[4 * i + j]; a[i][4 + j] = (i == j) ? 1.0 : 0.0; }
#pragma unroll
    for (int col = 0; col < 4; col++) {
        int piv = col; double best = __builtin_fabs(a[col][col]);
#pragma unroll
        for (int r = col + 1; r < 4; r++) { const double t = __builtin_fabs(a[r][col]); if (t > best) { best = t; piv = r; } }
        if (best == 0.0) return false;
#pragma unroll
        for (int r = col + 1; r < 4; r++)            // swap row `piv` into place without dynamic register indexing
            if (piv == r) {
#pragma unroll
                for (int j = 0; j < 8; j++) { const double t = a[col][j]; a[col][j] = a[r][j]; a[r][j] = t; }
            }
        const double ip = 1.0 / a[col][col];
#pragma unroll
        for (int j = 0; j < 8; j++) a[col][j] *= ip;
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r != col) {
                const double f = a[r][col];
                if (f != 0.0) {
#pragma unroll
                    for (int j = 0; j < 8; j++) a[r][j] -= f * a[col][j];
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) out[4 * i + j] = a[i][4 + j];
    return true;
}

// barycentric coordinates of the closest point, blend of the three per-vertex 4x4, inverse, application  (ray_utils.py:77-88)
__device__ __forceinline__ void finish_sample(uint32_t i, const double (&p)[3], const double (&bc)[3], double best, int bf,
                                              const float *__restrict__ verts, const int32_t *__restrict__ faces, const double *__restrict__ T,
                                              double threshold, double *__restrict__ can_pts, float *__restrict__ can_pts_f32,
                                              double *__restrict__ closest, double *__restrict__ dist2, int32_t *__restrict__ face_id,
                                              uint8_t *__restrict__ mask)
{
    const int32_t f0v = faces[3 * (size_t)bf], f1v = faces[3 * (size_t)bf + 1], f2v = faces[3 * (size_t)bf + 2];
    double w[3], M[16], Mi[16];
    face_bary(bc, verts, f0v, f1v, f2v, w);
#pragma unroll
    for (int e = 0; e < 16; e++) M[e] = T[16 * (size_t)f0v + e] * w[0] + T[16 * (size_t)f1v + e] * w[1] + T[16 * (size_t)f2v + e] * w[2];
    inv4(M, Mi);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double v = Mi[4 * r] * p[0] + Mi[4 * r + 1] * p[1] + Mi[4 * r + 2] * p[2] + Mi[4 * r + 3];
        if (can_pts) can_pts[3 * (size_t)i + r] = v;
        if (can_pts_f32) can_pts_f32[3 * (size_t)i + r] = (float)v;
    }
    if (closest) { closest[3 * (size_t)i] = bc[0]; closest[3 * (size_t)i + 1] = bc[1]; closest[3 * (size_t)i + 2] = bc[2]; }
    if (dist2) dist2[i] = best;
    if (face_id) face_id[i] = bf;
    mask[i] = best < threshold ? 1 : 0;
}

__global__ __launch_bounds__(256) void warp_samples_kernel(const float *__restrict__ pts, const float *__restrict__ verts,
                                                           const int32_t *__restrict__ faces, const double *__restrict__ T, uint32_t P,
                                                           uint32_t F, double threshold, double *__restrict__ can_pts,
                                                           float *__restrict__ can_pts_f32, double *__restrict__ closest,
                                                           double *__restrict__ dist2, int32_t *__restrict__ face_id,
                                                           uint8_t *__restrict__ mask)
{
    __shared__ float st[FT * 9];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < P;
    const uint32_t ii = live ? i : 0;
    const double p[3] = { (double)pts[3 * ii], (double)pts[3 * ii + 1], (double)pts[3 * ii + 2] };
    double best = __builtin_inf(), bc[3] = { 0.0, 0.0, 0.0 };
    int bf = 0;
    for (uint32_t f0 = 0; f0 < F; f0 += FT) {
        const uint32_t cnt = (F - f0 < (uint32_t)FT) ? F - f0 : (uint32_t)FT;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < cnt * 3; e += blockDim.x) {       // one (face, corner) per step
            const int32_t vi = faces[(size_t)f0 * 3 + e];
            st[3 * e] = verts[3 * (size_t)vi]; st[3 * e + 1] = verts[3 * (size_t)vi + 1]; st[3 * e + 2] = verts[3 * (size_t)vi + 2];
        }
        __syncthreads();
        for (uint32_t f = 0; f < cnt; ++f) {
            // (written out, not tri_closest(t, p, q): through the helper this loop is scheduled differently and the kernel measured 3 % slower,
            // 23.6 against 23.0 ms for 524 288 points x 13 778 faces -- profiles/warp_search_cleanup.txt)
            const float *t = st + 9 * f;
            const double a[3] = { (double)t[0], (double)t[1], (double)t[2] }, b[3] = { (double)t[3], (double)t[4], (double)t[5] },
                         c[3] = { (double)t[6], (double)t[7], (double)t[8] };
            double q[3];
            closest_pt_tri(p, a, b, c, q);
            const double ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2], d2 = ex * ex + ey * ey + ez * ez;
            if (d2 < best) { best = d2; bf = (int)(f0 + f); bc[0] = q[0]; bc[1] = q[1]; bc[2] = q[2]; }
        }
    }
    if (!live) return;
    finish_sample(i, p, bc, best, bf, verts, faces, T, threshold, can_pts, can_pts_f32, closest, dist2, face_id, mask);
}

// skip_masked rendering: a ray none of whose samples can come within the mask threshold of the mesh renders to the background whatever the field
// says.  pts = the coarse samples [N, T0, 3] (posed space); every later sample of the ray (up-sampled z, mid points) lies within half a coarse step
// of one of them, so the ray is DEAD if  sqrt(far_bound(p_i)) - step_i / 2 >= sqrt(threshold)  for every coarse sample.  One lane per ray.
__global__ __launch_bounds__(256) void ray_cull_kernel(const float *__restrict__ pts, uint32_t N, uint32_t T0, AccelView av, float thr,
                                                       uint8_t *__restrict__ ray_dead)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float rt = __builtin_sqrtf(thr) * (1.0f + 1e-6f);
    bool dead = true;
    float dprev = 0.0f;
    for (uint32_t i = 0; i < T0 && dead; ++i) {
        const float *pp = pts + ((size_t)r * T0 + i) * 3;
        const float p[3] = { pp[0], pp[1], pp[2] };
        float dnext = 0.0f;
        if (i + 1 < T0) { const float ex = pp[3] - p[0], ey = pp[4] - p[1], ez = pp[5] - p[2]; dnext = __builtin_sqrtf((ex * ex + ey * ey) + ez * ez); }
        const float step = (dprev > dnext ? dprev : dnext) * (1.0f + 1e-5f);
        const float lo = __builtin_sqrtf(grid_far_bound(av, p)) * (1.0f - 1e-6f) - 0.5f * step;
        dead = lo >= rt;                                               // NaN points / steps compare false: the ray is searched
        dprev = dnext;
    }
    ray_dead[r] = dead ? 1 : 0;
}

// ---- the search: one wave owns 64 consecutive samples -------------------------------------------------------------------------------------------
// A sample's candidate tiles come from its cell's list -- every lane walks the list of ITS sample's cell, four entries per trip, box-testing them
// against the sample's current bound -- or, without a cell, from a pass over all tile boxes, one sample at a time.  The rest is a pipeline of packed LDS
// queues shared by the wave's samples:
//   (sample, tile) -> sub-box test -> (sample, tile, group) -> disc test -> (sample, face) -> fp64 Ericson routine -> running minimum of the sample
// with lanes = 16 pairs x 4 groups, 8 triples x 8 faces and 64 pairs respectively, so the lanes never diverge and every step is full.
// Every test before the last is a conservative lower bound; the exact routine is the brute-force kernel's; ties -> lowest face id.
// The barycentric blend / 4x4 inverse epilogue runs lane-parallel for the 64 samples.  Bit-identical to warp_samples_kernel.
// The work of the wave's samples is PACKED: (sample, tile) pairs whose box can hold the answer go to a queue; a disc trip takes 8 pairs of whatever
// samples and tests their 8 x 32 faces against the bounding discs; the surviving (sample, face) pairs go to a second queue and through the fp64
// Ericson routine 64 at a time.  Every trip and every exact batch is full (up to the wave's last one) whatever the number of candidates of a single
// sample is -- with one sample at a time a batch held 17 faces on average.  Running minima live in LDS: best[s] as the bit pattern of the (non-negative)
// fp64 distance^2 under an unsigned 64-bit minimum, the lowest face id among equal distances under a second minimum; the result does not depend on the
// order of the pairs, and equals the exhaustive kernel's bit for bit.
constexpr uint32_t TQ = 1024, GQ = 256, FQ = 256;     // pair queues (rings): a sample adds <= NIT x 64 = 512 (sample, tile) pairs to < 32 left over; a group trip
                                                       // <= 128 (sample, tile, group) triples to < 16; a disc trip <= 128 (sample, face) pairs to < 64
constexpr int GSTEPS = 2, DSTEPS = 3;           // steps per group trip (16 tile pairs each) and per disc trip (8 triples each)
static_assert(TQ >= NIT * 64 + 16 * GSTEPS && GQ >= 64 * GSTEPS + 8 * DSTEPS && FQ >= 64 * DSTEPS + 64 && MAX_TILES <= 512 && TILE_F == 32 && SUBS == 4 && SUB_F == 8,
              "queue capacities / pair encoding");
constexpr int PK_WAVES = 8;                     // waves per workgroup (they share the 32 KB of boxes)
constexpr int WARP_WAVES = 4;                   // waves per SIMD the search kernel is compiled for (<= 128 VGPRs)
constexpr uint32_t PK_WAVE_BYTES = 64 * 8 + 64 * 4 + 3 * 64 * 4 + FQ * 4 + GQ * 4 + TQ * 2;

// the closest point to p on face f of the mesh as the caller gave it (corners from verts / faces)
__device__ __forceinline__ void face_closest(const float *__restrict__ verts, const int32_t *__restrict__ faces, size_t f, const double (&p)[3], double (&cq)[3])
{
    const int32_t f0v = faces[3 * f], f1v = faces[3 * f + 1], f2v = faces[3 * f + 2];
    double a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { a[k] = (double)verts[3 * (size_t)f0v + k]; b[k] = (double)verts[3 * (size_t)f1v + k]; c[k] = (double)verts[3 * (size_t)f2v + k]; }
    closest_pt_tri(p, a, b, c, cq);
}
// a running fp64 bound as an fp32 number >= it (+inf stays +inf): what the fp32 lower bounds are compared with
__device__ __forceinline__ float bound_f32(double best) { return (float)(best * (1.0 + 1e-9)) * 1.000001f; }

#ifdef AC_PROFILE_WARP         // s_memtime per phase, summed over waves: tools/warp_profile.py
__device__ unsigned long long g_warp_prof[8];
#define WP_T0() unsigned long long wp_t_ = __builtin_amdgcn_s_memtime(), wp_acc_[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }
#define WP_TICK(S) { const unsigned long long t2_ = __builtin_amdgcn_s_memtime(); wp_acc_[S] += t2_ - wp_t_; wp_t_ = t2_; }
#define WP_END() if (lane == 0) { for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_warp_prof[i_], wp_acc_[i_]); }
#else
#define WP_T0()
#define WP_TICK(S)
#define WP_END()
#endif

__global__ __launch_bounds__(PK_WAVES * 64, WARP_WAVES) void warp_samples_accel_kernel(const float *__restrict__ pts, const float *__restrict__ verts,
                                                                 const int32_t *__restrict__ faces, const double *__restrict__ T, uint32_t P,
                                                                 double threshold, AccelView av, double *__restrict__ can_pts,
                                                                 float *__restrict__ can_pts_f32, double *__restrict__ closest,
                                                                 double *__restrict__ dist2, int32_t *__restrict__ face_id,
                                                                 uint8_t *__restrict__ mask, float skip_thr,
                                                                 const uint8_t *__restrict__ ray_dead, uint32_t spr, uint32_t perm_mul,
                                                                 int32_t *__restrict__ tseeds, uint32_t tseed_stride, uint32_t tseed_off, uint32_t n_faces)
{
    const int lane = threadIdx.x & 63;
    // which 64 samples this wave owns: consecutive waves take chunks perm_mul apart (a bijection: gcd(perm_mul, chunks) = 1, chosen by the host), so
    // that the eight waves of a workgroup -- and the two workgroups of a compute unit -- hold a mix of cheap chunks (rays far from the body, samples the
    // caller lets the search skip) and expensive ones instead of 16 neighbouring rays of the same kind
    const uint32_t wave = (uint32_t)(((unsigned long long)((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * perm_mul) % ((P + 63u) >> 6));
    const uint32_t nt = av.hdr[0];
    const uint32_t nit = (nt + 63) >> 6;
    extern __shared__ __attribute__((aligned(16))) float sbox_raw[];
    const uint32_t ntp = nit * 64;                                     // tiles rounded up to whole bounding-pass iterations: the LDS row length
    char *wl = reinterpret_cast<char *>(sbox_raw + NBT * ntp) + (threadIdx.x >> 6) * PK_WAVE_BYTES;
    unsigned long long *sbest = reinterpret_cast<unsigned long long *>(wl);      // [64] bits of the running minimum distance^2 of sample s
    uint32_t *sbid = reinterpret_cast<uint32_t *>(wl + 512);                     // [64] lowest face id at that distance
    float *sq = reinterpret_cast<float *>(wl + 768);                             // [3][64] the samples
    uint32_t *fq = reinterpret_cast<uint32_t *>(wl + 1536);                      // [FQ] (sample << 14) | slot
    uint32_t *gq = reinterpret_cast<uint32_t *>(wl + 1536 + FQ * 4);             // [GQ] (sample << 11) | (tile << 2) | group
    uint16_t *tq = reinterpret_cast<uint16_t *>(wl + 1536 + FQ * 4 + GQ * 4);    // [TQ] (sample << 9) | tile
    load_boxes<BoxLayout::TileMajor>(sbox_raw, av, ntp);
    __syncthreads();
    if (((blockIdx.x * blockDim.x + threadIdx.x) >> 6) >= ((P + 63u) >> 6)) return;       // (after the barrier) a wave without samples
    const uint32_t i = wave * 64 + lane;
    const bool live = i < P;
    const uint32_t ii = live ? i : P - 1;
    const float pf[3] = { pts[3 * (size_t)ii], pts[3 * (size_t)ii + 1], pts[3 * (size_t)ii + 2] };
    const double p[3] = { (double)pf[0], (double)pf[1], (double)pf[2] };
    const uint32_t npts = (P - wave * 64 < 64u) ? P - wave * 64 : 64u;            // wave-uniform
    WP_T0();
    // 0. lane = sample: the sample's cell (finest level that has a list), and the exact distance^2 to the cell's seed face: an upper bound of the
    // result and a real face's distance, so the running minimum may start from it
    uint32_t mybase = 0, mycnt = CELL_OVERFLOW;
    double myseed = __builtin_inf();
    // skip_thr >= 0 (the caller only wants mask and the canonical points of UNMASKED samples): a sample whose cell proves dist^2 >= threshold is
    // masked out whatever its closest face is -- it is not searched at all (dead).  Outside both grids the mesh is >= the coarse margin away.
    // (grid_far_bound's values, but not `grid_far_bound(av, pf) >= skip_thr`: where nothing is known -- outside both grids of a structure without a
    // coarse grid -- that answers 0, which a threshold of 0 would take for a proof; here such a sample is always searched.)
    bool dead = ray_dead ? ray_dead[ii / spr] != 0 : false;              // skip_masked: the sample's whole ray is provably masked out (ray_cull_kernel)
    if (dead) mycnt = 0;
    else if (skip_thr >= 0.0f) {
        bool in_any = false;
#pragma unroll
        for (int l = 0; l < GRID_LEVELS; ++l) {
            const uint32_t cell = grid_cell(grid_params(av, l), pf);
            if (cell != ~0u && !in_any) { in_any = true; dead = av.cfar[LVL_CELL0[l] + cell] >= skip_thr; }
        }
        if (!in_any && av.hdr[HDR_LVL + HDR_LVL_STRIDE * (GRID_LEVELS - 1) + 8] != 0u)
            dead = GRID_MARGIN1 * GRID_MARGIN1 * (1.0f - 1e-5f) >= skip_thr;
        if (dead) mycnt = 0;                                           // no list, no full pass
    }
#pragma unroll
    for (int l = 0; l < GRID_LEVELS; ++l) {
        if (mycnt != CELL_OVERFLOW) continue;
        const GridParams g = grid_params(av, l);
        const uint32_t cell = grid_cell(g, pf);
        if (cell != ~0u) {
            const uint32_t info = av.cell[LVL_CELL0[l] + cell];
            if ((info >> 16) != CELL_OVERFLOW) {
                const uint32_t slot = info & 0xffffu;
                double cq[3];
                const double d2 = tri_closest(av.tri + (size_t)slot * 9, p, cq);
                if (d2 < 1e30) {                                       // NaN from a degenerate seed face in this sample's region: next level / full pass
                    myseed = d2; mycnt = info >> 16; mybase = LVL_CTL0[l] + cell * LVL_K[l];
                }
            }
        }
    }
    // TEMPORAL SEED: the caller keeps, per (ray, sample slot), the face the PREVIOUS frame's search found (tseeds; -1 = none) -- an animation's
    // body moves little between frames, so that face is usually the closest one again or next to it.  Its exact distance in THIS frame's pose is a real
    // face's distance, i.e. a valid first bound like the cell's seed face, and usually a much tighter one: the walk prunes against it from the first
    // tile on.  Results: the same face, the same bits (the bound only removes candidates that are provably farther).
    double tseed = __builtin_inf();
    const size_t tsi = tseeds ? (size_t)(ii / spr) * tseed_stride + tseed_off + (ii % spr) : 0;
    if (tseeds && live && !dead) {
        const int32_t tf = tseeds[tsi];
        if (tf >= 0 && (uint32_t)tf < n_faces) {
            double cq[3];
            face_closest(verts, faces, (size_t)tf, p, cq);
            const double d2 = dist2_pts(p, cq);
            if (d2 < 1e30) tseed = d2;
        }
    }
    if (tseed < myseed && mycnt != CELL_OVERFLOW) myseed = tseed;
    // skip_thr >= 0: the caller reads mask and the canonical points of UNMASKED samples only, i.e. a closest face matters only if it is closer than
    // the mask's threshold -- so the running bound never needs to start above it.  A sample whose seed face is farther away (the outer part of the
    // shell the cell grids cannot prove masked: the samples with the LONGEST candidate lists) walks its list against threshold (1 + 1e-6) instead; if no
    // face comes in under that, the sample is masked out and leaves like a dead one.  Unmasked samples: the same face, the same bits.
    if (skip_thr >= 0.0f && myseed > (double)skip_thr) myseed = (double)skip_thr;
    sbest[lane] = __builtin_bit_cast(unsigned long long, myseed);
    sbid[lane] = 0x7fffffffu;
#pragma unroll
    for (int k = 0; k < 3; ++k) sq[k * 64 + lane] = pf[k];
    wave_sync();
    WP_TICK(7)
    uint32_t th = 0, tt = 0, gh = 0, gt = 0, fh = 0, ft = 0;             // wave-uniform ring positions: tile pairs, group triples, face pairs
    // work counters of this wave (wave-uniform; one atomic each at the end -> AccelView::work: what bench.py prices the search with)
    uint32_t n_exact = 0, n_disc = 0, n_sub = 0, n_box = 0;

    // exact distances of n queued (sample, face) pairs, folded into the samples' running minima
    auto exact_batch = [&](uint32_t n) {
        wave_sync();
        bool act = (uint32_t)lane < n;
        const uint32_t e = fq[(fh + (act ? (uint32_t)lane : 0u)) & (FQ - 1)];
        const uint32_t s = e >> 14, slot = e & 16383u;
        unsigned long long d2b = ~0ull;
        int id = 0x7fffffff;
        if (act) {
            const double q[3] = { (double)sq[s], (double)sq[64 + s], (double)sq[128 + s] };
            double cq[3];
            const double d2 = tri_closest(av.tri + (size_t)slot * 9, q, cq);
            id = av.oid[slot];
            act = d2 == d2;                                              // a degenerate face (0 / 0 in an edge region) is never accepted
            d2b = __builtin_bit_cast(unsigned long long, d2);             // d2 >= +0: the bit patterns order like the values
        }
        n_exact += n;
        const unsigned long long prev = sbest[s];
        wave_sync();
        if (act) atomicMin(&sbest[s], d2b);
        wave_sync();
        const unsigned long long cur = sbest[s];
        if (act && d2b == cur && cur < prev) sbid[s] = 0x7fffffffu;      // a strictly better distance: ids recorded for the old one are void
        wave_sync();
        if (act && d2b == cur) atomicMin(&sbid[s], (uint32_t)id);
        fh += n;
        wave_sync();
    };
    // up to GSTEPS x 16 queued (sample, tile) pairs: the four sub-boxes of the tile (groups of 8 consecutive faces, boxes in the tile's frame) against
    // the sample's current bound, lane = (pair, group); the survivors are queued as (sample, tile, group)
    auto group_trip = [&]() {
        wave_sync();
        const uint32_t np = (tt - th) < (uint32_t)(16 * GSTEPS) ? (tt - th) : (uint32_t)(16 * GSTEPS);
#pragma unroll
        for (int u = 0; u < GSTEPS; ++u) {
            if ((uint32_t)(16 * u) >= np) break;                         // wave-uniform
            const uint32_t pi = (uint32_t)(16 * u + (lane >> 2));
            const bool have = pi < np;
            const uint32_t e = tq[(th + (have ? pi : 0u)) & (TQ - 1)];
            const uint32_t smp = e >> 9, tile = e & 511u, tg = tile * SUBS + (uint32_t)(lane & 3);
            const float2 *sb2 = reinterpret_cast<const float2 *>(av.sub + (size_t)tg * 6);
            const float2 b0 = sb2[0], b1 = sb2[1], b2 = sb2[2];          // lo.x lo.y | lo.z hi.x | hi.y hi.z
            const float qf[3] = { sq[smp], sq[64 + smp], sq[128 + smp] };
            const float limf = bound_f32(__builtin_bit_cast(double, sbest[smp]));
            const float blo[3] = { b0.x, b0.y, b1.x }, bhi[3] = { b1.y, b2.x, b2.y };
            const f32x4w *rec = reinterpret_cast<const f32x4w *>(sbox_raw + tile * NBT);     // the tile's axes: three 16-byte reads (tile-major bounds)
            const f32x4w a0 = rec[0], a1 = rec[1], a2 = rec[2];
            const float ax[9] = { a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3], a2[0] };
            const bool pass = have && slab_lower_bound(ax, blo, bhi, qf, query_pad(qf)) <= limf;
            const unsigned long long pm = __ballot(pass);
            if (pass) gq[(gt + (uint32_t)__builtin_popcountll(pm & ((1ull << lane) - 1ull))) & (GQ - 1)] = (smp << 11) | tg;
            gt += (uint32_t)__builtin_popcountll(pm);
        }
        th += np;
        n_sub += 4u * np;
        WP_TICK(3)
    };
    // up to DSTEPS x 8 queued (sample, tile, group) triples: the group's 8 faces against their bounding discs (a lower bound of a face's distance)
    // under the sample's current bound, lane = (triple, face); survivors are queued for the exact routine
    auto disc_trip = [&]() {
        wave_sync();
        const uint32_t ne = (gt - gh) < (uint32_t)(8 * DSTEPS) ? (gt - gh) : (uint32_t)(8 * DSTEPS);
        uint32_t slot[DSTEPS], smp[DSTEPS]; bool have[DSTEPS];
        float4 sp[DSTEPS], sn[DSTEPS];
#pragma unroll
        for (int u = 0; u < DSTEPS; ++u) {
            const uint32_t ei = (uint32_t)(8 * u + (lane >> 3));
            have[u] = ei < ne;
            const uint32_t e = gq[(gh + (have[u] ? ei : 0u)) & (GQ - 1)];
            smp[u] = e >> 11;
            slot[u] = (e & 2047u) * SUB_F + (uint32_t)(lane & 7);        // (tile * 4 + group) * 8 + face = tile * 32 + ...
            sp[u] = av.sph[2 * (size_t)slot[u]]; sn[u] = av.sph[2 * (size_t)slot[u] + 1];
        }
        gh += ne;
        n_disc += 8u * ne;
#pragma unroll
        for (int u = 0; u < DSTEPS; ++u) {
            if ((uint32_t)(8 * u) >= ne) break;                          // wave-uniform
            // lower bound of the face's distance from its bounding disc (accel_tiles_kernel), in fp32: q, the disc and the normal are
            // fp32 data, and every rounding below is padded towards "pass" (a face that passes wrongly only costs an exact test)
            const float q0 = sq[smp[u]], q1 = sq[64 + smp[u]], q2 = sq[128 + smp[u]];
            const float limf = bound_f32(__builtin_bit_cast(double, sbest[smp[u]]));
            const float ex = q0 - sp[u].x, ey = q1 - sp[u].y, ez = q2 - sp[u].z;
            const float e1 = (__builtin_fabsf(ex) + __builtin_fabsf(ey)) + __builtin_fabsf(ez);
            const float e2 = (ex * ex + ey * ey) + ez * ez;
            const float apd = __builtin_fabsf((ex * sn[u].x + ey * sn[u].y) + ez * sn[u].z);
            const float err = 1e-6f * e1 + 1e-6f;                              // rounding of the dot product, of the stored normal and centre
            const float pdl = apd > err ? apd - err : 0.0f, pdh = apd + err;   // plane distance of q: lower / upper bound
            const float rem = (limf - pdl * pdl) + 1e-6f * (limf + pdl * pdl); // >= what the bound leaves for the in-plane distance^2
            const float rho2 = (e2 - pdh * pdh) - 2e-6f * (e2 + pdh * pdh);    // <= (in-plane distance of q from the disc centre)^2
            const float rr = (sp[u].w + __builtin_sqrtf(rem > 0.0f ? rem : 0.0f) * 1.000001f) + 1e-12f;
            const bool pass = have[u] && rem >= 0.0f && rho2 <= rr * rr * 1.000001f;
            const unsigned long long pm = __ballot(pass);
            if (pass) fq[(ft + (uint32_t)__builtin_popcountll(pm & ((1ull << lane) - 1ull))) & (FQ - 1)] = (smp[u] << 14) | slot[u];
            ft += (uint32_t)__builtin_popcountll(pm);
        }
        WP_TICK(4)
    };
    // queue the tiles in `cand` (lane = position, tile id `tl`) for sample j
    auto push_tiles = [&](uint32_t j, unsigned long long cand, uint32_t tl) {
        if ((cand >> lane) & 1ull) tq[(tt + (uint32_t)__builtin_popcountll(cand & ((1ull << lane) - 1ull))) & (TQ - 1)] = (uint16_t)((j << 9) | tl);
        tt += (uint32_t)__builtin_popcountll(cand);
    };

    // ONE inlined copy of each downstream stage; downstream first (that bounds the queues): full trips / batches while candidates are still coming, the
    // leftovers at the end (last)
    auto drain = [&](bool last) {
        for (;;) {
            const uint32_t ntq = tt - th, ngq = gt - gh, nfq = ft - fh;
            const bool do_e = nfq >= 64u || (last && !ntq && !ngq && nfq);
            const bool do_d = !do_e && (ngq >= (uint32_t)(8 * DSTEPS) || (last && !ntq && ngq));
            const bool do_g = !do_e && !do_d && (ntq >= (uint32_t)(16 * GSTEPS) || (last && ntq));
            if (do_e) { exact_batch(nfq < 64u ? nfq : 64u); WP_TICK(5) }
            else if (do_d) disc_trip();
            else if (do_g) group_trip();
            else break;
        }
    };
    // 1. the front end, lane = sample: every lane walks the tile list of ITS cell, four entries per trip -- the box test of an entry against the lane's
    // CURRENT bound (the running minimum the exact batches keep lowering, not only the seed), survivors compacted into the pair queue.  A trip costs
    // 15 LDS reads + ~40 vector instructions and serves up to 64 samples (35 listed tiles per sample on average).  Trips = the longest list in the wave.
    {
        const bool has_list = (uint32_t)lane < npts && mycnt != CELL_OVERFLOW && mycnt != 0u;
        const uint32_t kmax = (uint32_t)(-wave_min_i32(has_list ? -(int)mycnt : 0));
        const float padq_l = query_pad(pf);
        // four list entries per trip (one 8-byte load: lists start on multiples of four entries), requested one trip ahead; the bound is read once per trip
        constexpr int BU = 4;
        static_assert(LVL_K[0] % BU == 0 && LVL_K[1] % BU == 0 && LVL_CTL0[1] % BU == 0, "8-byte aligned list chunks");
        auto chunk = [&](uint32_t k) -> uint2 {
            return (has_list && k < mycnt) ? *reinterpret_cast<const uint2 *>(av.ctl + (size_t)mybase + k) : make_uint2(0u, 0u);
        };
        uint2 nxt = chunk(0u);
        for (uint32_t k = 0; k < kmax; k += BU) {
            const uint2 cur = nxt;
            nxt = chunk(k + (uint32_t)BU);
            const uint32_t tl[BU] = { cur.x & 0xffffu, cur.x >> 16, cur.y & 0xffffu, cur.y >> 16 };
            const float limf = bound_f32(__builtin_bit_cast(double, sbest[lane]));
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const bool mine = has_list && k + (uint32_t)u < mycnt;
                const float l = box_lower_bound<BoxLayout::TileMajor>(sbox_raw, ntp, (int)(mine ? tl[u] : 0u), pf, padq_l);
                n_box += (uint32_t)__builtin_popcountll(__ballot(mine));
                const unsigned long long cand = __ballot(mine && l <= limf);
                if (cand) push_tiles((uint32_t)lane, cand, tl[u]);
            }
            WP_TICK(0)
            drain(false);
        }
    }
    // 2. samples without a list (outside both grids, an overflowing cell) take the full bounding pass, one at a time
    for (uint32_t j = 0; j <= npts; ++j) {                                 // j == npts: drain the queues
        const bool last = j == npts;
        if (!last) {
            if ((uint32_t)__builtin_amdgcn_readlane((int)mycnt, (int)j) != CELL_OVERFLOW) continue;
            // the lower bound of every tile, exact test of the two most promising tiles; the best of their faces is the sample's first bound (a
            // real face's distance)
            const float qf[3] = { lane_f32(pf[0], (int)j), lane_f32(pf[1], (int)j), lane_f32(pf[2], (int)j) };
            float lb[NIT];
            int tA, tB;
            bounding_pass<BoxLayout::TileMajor>(sbox_raw, ntp, nit, lane, qf, lb, tA, tB);
            WP_TICK(1)
            const double q[3] = { (double)qf[0], (double)qf[1], (double)qf[2] };
            double best = __builtin_inf(), bc[3] = { 0.0, 0.0, 0.0 };
            int bid = 0x7fffffff;
            uint32_t myslot;
            seed_test(av, q, tA, tB, lane, best, bid, bc, myslot);
            double seed = wave_min_f64(best);                            // +inf if every seed face is degenerate
            { const double ts = lane_f64(tseed, (int)j); if (ts < seed) seed = ts; }        // (the previous frame's face, see stage 0)
            if (skip_thr >= 0.0f && seed > (double)skip_thr) seed = (double)skip_thr;       // (as above: only faces under the mask's threshold matter)
            n_box += nt; n_exact += 2u * TILE_F;
            if (lane == 0) sbest[j] = __builtin_bit_cast(unsigned long long, seed);
            WP_TICK(2)
            const float lim0f = bound_f32(seed);
            // the candidate tiles (box distance^2 <= bound): the seed tiles among them -- their faces go through the queues like all others
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if ((uint32_t)it >= nit) break;                            // wave-uniform
                unsigned long long cand = __ballot(lb[it] <= lim0f);       // fp32 compare against the bound rounded up: a superset
                push_tiles(j, cand, (uint32_t)(it * 64 + lane));
            }
            WP_TICK(3)
        }
        drain(last);
    }
    WP_TICK(5)
    if (live && !dead && skip_thr >= 0.0f && sbid[lane] == 0x7fffffffu) dead = true;      // no face under the mask's threshold: masked out
    if (live && dead) {                                           // certainly masked out: no closest face was looked for
        mask[i] = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (can_pts) can_pts[3 * (size_t)i + r] = p[r];
            if (can_pts_f32) can_pts_f32[3 * (size_t)i + r] = pf[r];
            if (closest) closest[3 * (size_t)i + r] = p[r];
        }
        if (dist2) dist2[i] = __builtin_inf();
        if (face_id) face_id[i] = 0;
    } else if (live) {
        // lane = sample again: the closest point on the winning face (the same routine on the same operands as in the batch that found it)
        const double rbest = __builtin_bit_cast(double, sbest[lane]);
        uint32_t rb = sbid[lane];
        double rbc[3] = { 0.0, 0.0, 0.0 };
        if (rb == 0x7fffffffu) rb = 0;                                   // no face with a distance (all degenerate): what the exhaustive kernel reports
        else face_closest(verts, faces, (size_t)rb, p, rbc);
        finish_sample(i, p, rbc, rbest, (int)rb, verts, faces, T, threshold, can_pts, can_pts_f32, closest, dist2, face_id, mask);
        if (tseeds && sbid[lane] != 0x7fffffffu) tseeds[tsi] = (int32_t)rb;                  // the next frame's seed of this (ray, slot)
    }
    const uint32_t seeds = (uint32_t)__builtin_popcountll(__ballot(myseed < 1e30)) + (uint32_t)__builtin_popcountll(__ballot(tseed < 1e30));   // exact tests of the seed faces (stage 0)
    if (lane == 0) {
        unsigned long long *wk = av.work + 4 * (((blockIdx.x * blockDim.x + threadIdx.x) >> 6) % (uint32_t)WORK_SLOTS);
        atomicAdd(wk, (unsigned long long)(n_exact + seeds)); atomicAdd(wk + 1, (unsigned long long)n_disc);
        atomicAdd(wk + 2, (unsigned long long)n_sub); atomicAdd(wk + 3, (unsigned long long)n_box);
    }
    WP_TICK(6)
    WP_END()
}

}  // namespace

#ifdef AC_PROFILE_WARP
AC_API void ac_debug_warp_prof(unsigned long long *out, int reset)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_warp_prof), sizeof(unsigned long long) * 8);
    if (reset) { static unsigned long long z[8] = { 0 }; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_warp_prof), z, sizeof(z)); }
}
#endif

AC_API int ac_mesh_near_far(const float *rays_o, const float *rays_d, const float *verts, uint32_t N, uint32_t V, float geo_threshold,
                            float *near, float *far, ac_stream_t stream)
{
    if (N == 0) return AC_OK;
    if (!rays_o || !rays_d || !verts || !near || !far || V == 0) { ac::set_error("mesh_near_far: NULL buffer or empty mesh"); return AC_ERR_BAD_ARG; }
    const float r2 = (float)((double)geo_threshold * (double)geo_threshold);
    uint32_t tiles = (V + VT - 1) / VT;
    if ((N + 63) / 64 >= ac::cu_count()) tiles = 1;                  // enough ray blocks to fill the device: one workgroup walks all vertex tiles
    if (tiles > 1) {                                                 // one workgroup per (64 rays, vertex tile): results meet through atomic min / max
        (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(near), 0x7f800000, N, (hipStream_t)stream);      // +inf
        (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(far), (int)0xff800000u, N, (hipStream_t)stream); // -inf
    }
    hipLaunchKernelGGL(mesh_near_far_kernel, dim3((N + 63) / 64, tiles), dim3(NF_WAVES * 64), 0, (hipStream_t)stream, rays_o, rays_d, verts, N, V, r2, near, far);
    return ac::check_launch("mesh_near_far");
}

AC_API int ac_warp_samples(const float *pts, const float *verts, const int32_t *faces, const double *T, uint32_t P, uint32_t V, uint32_t F,
                           double threshold, double *can_pts, float *can_pts_f32, double *closest, double *dist2, int32_t *face_id,
                           uint8_t *mask, ac_stream_t stream)
{
    (void)V;
    if (P == 0) return AC_OK;
    if (!pts || !verts || !faces || !T || !mask || F == 0 || (!can_pts && !can_pts_f32)) { ac::set_error("warp_samples: NULL buffer or empty mesh"); return AC_ERR_BAD_ARG; }
    hipLaunchKernelGGL(warp_samples_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, verts, faces, T, P, F, threshold,
                       can_pts, can_pts_f32, closest, dist2, face_id, mask);
    return ac::check_launch("warp_samples");
}

// skip_far: samples that the cell grids prove to be masked out (dist^2 >= threshold) are not searched; their canonical point is reported as the
// sample itself (ac_render_rays_warped with skip_masked: the final pass never evaluates them)
int ac::warp_samples_accel_impl(const float *pts, const float *verts, const int32_t *faces, const double *T, uint32_t P, uint32_t V,
                                uint32_t F, double threshold, const void *accel, double *can_pts, float *can_pts_f32, double *closest,
                                double *dist2, int32_t *face_id, uint8_t *mask, ac_stream_t stream, int skip_far, const uint8_t *ray_dead,
                                uint32_t samples_per_ray, int32_t *tseeds, uint32_t tseed_stride, uint32_t tseed_off)
{
    (void)V;
    if (P == 0) return AC_OK;
    if (!pts || !verts || !faces || !T || !mask || !accel || F == 0 || F > MAX_ACCEL_FACES || (!can_pts && !can_pts_f32)) {
        ac::set_error("warp_samples_accel: NULL buffer, empty mesh or more than %u faces", MAX_ACCEL_FACES); return AC_ERR_BAD_ARG;
    }
    const AccelView av = accel_view(const_cast<void *>(accel));
    const uint32_t waves = (P + 63) / 64;
    const size_t ntp = (((size_t)F + TILE_F - 1) / TILE_F + 63) / 64 * 64;        // as in the kernel: tiles rounded up to 64
    const size_t lds = (size_t)NBT * ntp * sizeof(float) + (size_t)PK_WAVES * PK_WAVE_BYTES;
    static uint64_t seen = 0;        // the limit for the largest mesh the search supports; a launch asks for what its mesh needs
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(warp_samples_accel_kernel), (size_t)NBT * MAX_TILES * sizeof(float) + (size_t)PK_WAVES * PK_WAVE_BYTES);
    uint32_t perm_mul = 1;
    for (uint32_t m : { 37u, 41u, 43u, 47u, 53u }) {
        uint32_t a = waves, b = m;
        while (b) { const uint32_t t = a % b; a = b; b = t; }
        if (a == 1u) { perm_mul = m; break; }
    }
    const float skip_thr = skip_far ? (float)threshold * (1.0f + 1e-6f) : -1.0f;
    const uint32_t spr = samples_per_ray ? samples_per_ray : 1u;
    hipLaunchKernelGGL(warp_samples_accel_kernel, dim3((waves + PK_WAVES - 1) / PK_WAVES), dim3(PK_WAVES * 64), lds, (hipStream_t)stream, pts, verts, faces, T, P,
                       threshold, av, can_pts, can_pts_f32, closest, dist2, face_id, mask, skip_thr, ray_dead, spr, perm_mul,
                       tseeds, tseed_stride, tseed_off, F);
    return ac::check_launch("warp_samples_accel");
}

int ac::warp_ray_cull(const float *coarse_pts, uint32_t N, uint32_t T0, double threshold, const void *accel, uint8_t *ray_dead, ac_stream_t stream)
{
    if (N == 0) return AC_OK;
    const AccelView av = accel_view(const_cast<void *>(accel));
    hipLaunchKernelGGL(ray_cull_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, coarse_pts, N, T0, av, (float)threshold * (1.0f + 1e-6f), ray_dead);
    return ac::check_launch("warp_ray_cull");
}

AC_API int ac_warp_samples_accel(const float *pts, const float *verts, const int32_t *faces, const double *T, uint32_t P, uint32_t V,
                                 uint32_t F, double threshold, const void *accel, double *can_pts, float *can_pts_f32, double *closest,
                                 double *dist2, int32_t *face_id, uint8_t *mask, ac_stream_t stream)
{
    return ac::warp_samples_accel_impl(pts, verts, faces, T, P, V, F, threshold, accel, can_pts, can_pts_f32, closest, dist2, face_id, mask, stream, 0, nullptr, 1,
                                       nullptr, 0, 0);
}
