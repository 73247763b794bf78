// avatarcraft_amd/csrc/render_long.hip -- the fused Instant-NSR renderer for any sample count the reference accepts (ac_render_rays_long,
// ac_render_rays_long_pair, ac_sample_rays_long): num_steps >= 2 (not necessarily a multiple of 16), upsample_steps a multiple of 16, at most 512 samples per ray.
//
// The per-ray algorithm is render_rays_kernel's (render_fused.hip, MODE_FULL / MODE_UPSAMPLE): the same device blocks of the field headers (sdf_mlp.hpp, field_stencil.hpp, field_color.hpp)
// (fd_normal among them), the same scans in the same order; the blocks still written out in both kernels are marked where they stand.
// Where both renderers accept a sample count they agree bit for bit (tests/test_gpu_long_rays.py).
// What differs:
//   * a wave's LDS slab holds 512 samples (AC_MAXT), so a workgroup has 7 waves instead of 8: 13 540 + 7 x 3 680 floats = 153.5 KiB of the 160 KiB
//     (8 waves would need 168 KiB);
//   * num_steps need not be a multiple of 16: the last coarse tile and the last render tile are masked.  A masked lane still takes part in the
//     field evaluation (the MFMA tiles need all 64 lanes; it evaluates the ray's last sample again) but contributes the identity to every scan
//     and nothing to the cdf, the merges, the sums or the outputs;
//   * lin_z is read from device memory (any length) instead of the 64-float LDS slot;
//   * whole rays are the work items, dealt statically (no segment hand-off, no scratch): every ray costs the same number of tiles.
// Posed space (ac_render_rays_long_warped) is the sequence of ac_render_rays_warped on this kernel: MODE_UPSAMPLE takes the warped coarse points
// and writes z and the posed mid points, MODE_FINAL runs the render core at the warped mid points with alpha * mask.
#define AC_MAXT 512
#ifndef AC_WPB
#define AC_WPB 7
#endif
#include "sdf_mlp.hpp"
#include "field_stencil.hpp"
#include "field_color.hpp"
#include "render_slab.hpp"
#include "render_entry.hpp"

namespace {

static_assert(LONG_MAX_T == MAXT, "the long window is this kernel's slab");
constexpr int NCH = MAXT / 64;          // 64-lane chunks of the up-sampling scans

template <int MODE, bool FAST, bool EX, bool SH>
__global__ __launch_bounds__(BLOCK) void render_rays_long_kernel(const RenderArgs a)
{
    constexpr bool FC = FAST;
    // the training options of the canonical entry (pair launch, opacity_only, the stencil features feat7) live in the <MODE_FULL, *, EX = true, *> instantiations
    // only, behind run-time tests: a launch that asks for one of them takes such an instantiation, every other instantiation compiles as if they did not exist
    constexpr bool TR = EX && MODE == MODE_FULL;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (a.prepared) {
        const float4 *src = reinterpret_cast<const float4 *>(a.prepared);
        float4 *dst = reinterpret_cast<float4 *>(lds);
        for (int e = threadIdx.x; e < OFF_RWAVE / 4; e += blockDim.x)
            dst[e] = src[(FC && 4 * e >= OFF_C1F && 4 * e < OFF_B1) ? e + (OFF_RWAVE - OFF_C1F) / 4 : e];
        __syncthreads();
        for (int e = threadIdx.x; e < 16; e += blockDim.x) lds[OFF_LIN + 64 + e] = a.lin_u ? a.lin_u[e] : 0.0f;
    } else {
        fill_lds_sdf(lds, a);
        if constexpr (FAST) fill_lds_fast(lds, a);
        if constexpr (FC) fill_lds_color_fast<true, true>(lds, a);
        else fill_lds_color(lds, a);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    float *zs0 = lds + OFF_RWAVE + wave * WAVE_SLAB;    // final z values [512]
    float *zs1 = zs0 + MAXT;                            // up-sampling state: zs1 [512], sd [2][512], cdf [512], znew [16] ...
    float *sd = zs1 + MAXT;
    float *cdf = sd + 2 * MAXT;
    float *znl = cdf + MAXT;
    float *fsl = zs1;                                   // ... then the finite-difference features [6][8][64]
    const FieldCtx fc = make_ctx(a);
    const W2Row0 w2r0 = load_w2_row0(lds, lane);
    const float bound = a.bound;
    const float inv_s_core = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
    const int T0 = a.T0, nup = a.nup, T = T0 + 16 * nup;
    const int ntile0 = (T0 + 15) / 16, ntile = (T + 15) / 16;

    // static hand-out, XCD-aware like render_rays_kernel's counters: chunks of 512 consecutive rays, chunk c to XCD c % 8 (workgroup b runs on XCD
    // b % 8; the grid is a multiple of 8); the waves of an XCD take its rays in turn
    const int xper = ((a.n_rays + 7) / 8 + 7) & ~7, xchunk = xper < 512 ? xper : 512, xcd = blockIdx.x & 7;
    const int kstride = (int)(gridDim.x >> 3) * WAVES_PER_BLOCK;
    for (int k = (int)(blockIdx.x >> 3) * WAVES_PER_BLOCK + wave;; k += kstride) {
        const int kc = k / xchunk, base = (kc * 8 + xcd) * xchunk;
        if (base >= a.n_rays) break;
        int ray = base + (k - kc * xchunk);
        if (ray >= a.n_rays) continue;
        int rin = ray;                                              // row of this ray in rays_o / rays_d / near_m / far_m
        int exr = ray;                                              // row in the per-sample outputs
        bool ex_on = true;
        if constexpr (TR) {
            // pair launch (ac_render_rays_long_pair): the 2 pair_n work items are a0 b0 a1 b1 ...; a chunk holds an even number of them, so the two copies
            // of a ray are consecutive items of one chunk = of one XCD, taken by neighbouring waves at the same time: they meet in that XCD's L2.
            // Copy b = rows [pair_n, 2 pair_n) of noise, bg and the per-ray outputs; the per-sample outputs are kept for copy b only (ex_from = pair_n)
            if (a.pair_n) { rin = ray >> 1; ray = rin + ((ray & 1) ? a.pair_n : 0); }
            exr = ray - a.ex_from;
            ex_on = exr >= 0;
        }
        const float ox = a.rays_o[3 * rin], oy = a.rays_o[3 * rin + 1], oz = a.rays_o[3 * rin + 2];
        const float dx = a.rays_d[3 * rin], dy = a.rays_d[3 * rin + 1], dz = a.rays_d[3 * rin + 2];
        float near, far;
        cube_near_far(ox, oy, oz, dx, dy, dz, bound, near, far);
        if (a.near_m) {
            const float nm = a.near_m[rin], fm = a.far_m[rin];
            if (!is_inf(nm)) near = nm;
            if (!is_inf(fm)) far = fm;
        }
        const float span = far - near;
        const float sample_dist = span / (float)T0;
        int cur = (MODE == MODE_FINAL) ? 0 : (nup & 1), cnt = T0;
        float *const zs_first = cur ? zs1 : zs0;

        if constexpr (MODE == MODE_UPSAMPLE) {
            // skip_masked: a ray that cannot hold an unmasked sample (ray_cull) is not evaluated; its z array is the coarse one padded with its last value
            if (a.ray_dead && a.ray_dead[ray]) {
                for (int i = lane; i < T; i += 64) {
                    const int ic = i < T0 ? i : T0 - 1;
                    float zi = near + span * a.lin_z[ic];
                    if (a.perturb) zi = zi + (a.noise[(size_t)ray * T0 + ic] - 0.5f) * sample_dist;
                    const size_t si = (size_t)ray * T + i;
                    a.zbuf[si] = zi;
                    if (a.mid_pts) { a.mid_pts[3 * si] = ox + dx * zi; a.mid_pts[3 * si + 1] = oy + dy * zi; a.mid_pts[3 * si + 2] = oz + dz * zi; }
                }
                wave_sync();
                continue;
            }
        }
        // ---- coarse samples (last tile masked when 16 does not divide num_steps) --------------------------------------------------
        if constexpr (MODE == MODE_FINAL) {
            for (int i = lane; i < T; i += 64) zs0[i] = a.zbuf[(size_t)ray * T + i];
        }
        for (int c = 0; c < (MODE == MODE_FINAL ? 0 : ntile0); ++c) {
            const int i = 16 * c + n;
            const bool valid = i < T0;
            const int ic = valid ? i : T0 - 1;
            float zi = near + span * a.lin_z[ic];
            if (a.perturb) zi = zi + (a.noise[(size_t)ray * T0 + ic] - 0.5f) * sample_dist;
            if (nup > 0) {
                float px = clampf(ox + dx * zi, -bound, bound), py = clampf(oy + dy * zi, -bound, bound), pz = clampf(oz + dz * zi, -bound, bound);
                if constexpr (MODE == MODE_UPSAMPLE) {
                    if (a.ext_pts) {                                // posed space: the warped coarse points
                        const float *e = a.ext_pts + ((size_t)ray * T0 + ic) * 3;
                        px = clampf(e[0], -bound, bound); py = clampf(e[1], -bound, bound); pz = clampf(e[2], -bound, bound);
                    }
                }
                const f32x4 o2 = sdf_tile(lds, fc, lane, px, py, pz);
                if (g == 0 && valid) sd[cur * MAXT + i] = o2[0];
            }
            if (g == 0 && valid) zs_first[i] = zi;
        }
        wave_sync();

        // ---- NeuS up-sampling: chunks of 64 bins; chunks past the last bin are not visited (they would only scan identities) -----------
        for (int it = 0; it < (MODE == MODE_FINAL ? 0 : nup); ++it) {
            const float *zc = cur ? zs1 : zs0, *sc = sd + cur * MAXT;
            float *zn_ = cur ? zs0 : zs1, *sn_ = sd + (cur ^ 1) * MAXT;
            const int m = cnt - 1;
            const int nch_m = (m + 63) / 64, nch_c = (cnt + 63) / 64;
            const float inv_s = __builtin_ldexpf(64.0f, it);        // 64 * 2^it (instant_nsr.py:183), exact; an int shift would overflow from it = 25 (up to 31 here)
            float w[NCH];
            float carry = 1.0f; bool first = true;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                w[ch] = 0.0f;
                if (ch >= nch_m) continue;
                const int i = 64 * ch + lane;
                float alpha = 0.0f, om = 1.0f;
                if (i < m) {
                    const float z0 = zc[i], z1 = zc[i + 1], s0 = sc[i], s1 = sc[i + 1];
                    const float p0x = ox + dx * z0, p0y = oy + dy * z0, p0z = oz + dz * z0;
                    const float p1x = ox + dx * z1, p1y = oy + dy * z1, p1z = oz + dz * z1;
                    const float r0 = __builtin_sqrtf((p0x * p0x + p0y * p0y) + p0z * p0z);
                    const float r1 = __builtin_sqrtf((p1x * p1x + p1y * p1y) + p1z * p1z);
                    const bool inside = (r0 < 1.0f) | (r1 < 1.0f);
                    const float mid = (s0 + s1) * 0.5f;
                    const float dist = z1 - z0;
                    const float cosv = (s1 - s0) / (dist + 1e-5f);
                    float prev_cos = 0.0f;
                    if (i > 0) { const float zm = zc[i - 1], sm = sc[i - 1]; prev_cos = (s0 - sm) / ((z0 - zm) + 1e-5f); }
                    float cmin = prev_cos < cosv ? prev_cos : cosv;
                    cmin = clampf(cmin, -1e3f, 0.0f) * (inside ? 1.0f : 0.0f);
                    const float half = cmin * dist * 0.5f;
                    const float pc = dv_sigmoid((mid - half) * inv_s), nc = dv_sigmoid((mid + half) * inv_s);
                    alpha = (pc - nc + 1e-5f) / (pc + 1e-5f);
                    om = 1.0f - alpha + 1e-7f;
                }
                float loc, row_in; bool row_first;
                (void)chunk_scan<true>(om, lane, carry, first, loc, row_in, row_first);
                const float sh = dpp_shr<1>(1.0f, loc);
                float Tex;
                if (n == 0) Tex = row_first ? 1.0f : row_in;
                else Tex = row_first ? sh : row_in * sh;
                w[ch] = (i < m) ? alpha * Tex + 1e-5f : 0.0f;
            }
            float total;
            {
                float c2 = 0.0f; bool f2 = true; float lc, ri; bool rf;
                float last = 0.0f;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (ch >= nch_m) continue;
                    const float incl = chunk_scan<false>(w[ch], lane, c2, f2, lc, ri, rf);
                    const int il = m - 1 - 64 * ch;
                    const float cand = __shfl(incl, il & 63);
                    if (il >= 0 && il < 64) last = cand;
                }
                total = last;
            }
            {
                float c3 = 0.0f; bool f3 = true; float lc, ri; bool rf;
                if (lane == 0) cdf[0] = 0.0f;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (ch >= nch_m) continue;
                    const int i = 64 * ch + lane;
                    const float pdf = (i < m) ? w[ch] / total : 0.0f;
                    const float incl = chunk_scan<false>(pdf, lane, c3, f3, lc, ri, rf);
                    if (i < m) cdf[i + 1] = incl;
                }
            }
            wave_sync();
            float znew;
            int ind;
            {
                const float u = lds[OFF_LIN + 64 + n];
                int lo = 0, hi = cnt;
                while (lo < hi) { const int md = (lo + hi) >> 1; if (cdf[md] <= u) lo = md + 1; else hi = md; }
                ind = lo;
                const int below = lo - 1 > 0 ? lo - 1 : 0;
                const int above = lo < cnt - 1 ? lo : cnt - 1;
                const float cb = cdf[below], ca = cdf[above];
                float den = ca - cb;
                if (den < 1e-5f) den = 1.0f;
                const float t = (u - cb) / den;
                const float zb = zc[below], za = zc[above];
                znew = zb + t * (za - zb);
            }
            if (g == 0) {
                znl[n] = znew;
                if (EX && ex_on && a.out.ss_inds) a.out.ss_inds[((size_t)exr * nup + it) * 16 + n] = ind;
            }
            const bool last_it = (it + 1 == nup);
            float sdf_new = 0.0f;
            if (!last_it) {
                const float px = clampf(ox + dx * znew, -bound, bound), py = clampf(oy + dy * znew, -bound, bound),
                            pz = clampf(oz + dz * znew, -bound, bound);
                const f32x4 o2 = sdf_tile(lds, fc, lane, px, py, pz);
                sdf_new = o2[0];
            }
            wave_sync();
            // stable merge == torch.sort(cat([z, znew])); see render_rays_kernel for the unsorted first iteration of a ray that misses the cube
            const bool old_sorted = !(it == 0 && span < 0.0f);
            int32_t *sidx = (EX && ex_on && a.out.sort_index) ? a.out.sort_index + ((size_t)exr * nup + it) * T : nullptr;     // [N, nup, T]
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                if (ch >= nch_c) continue;
                const int i = 64 * ch + lane;
                if (i < cnt) {
                    const float zi = zc[i];
                    int c = 0;
#pragma unroll
                    for (int j = 0; j < 16; ++j) c += (znl[j] < zi) ? 1 : 0;
                    int before = i;
                    if (!old_sorted) {
                        before = 0;
                        for (int q = 0; q < cnt; ++q) { const float zk = zc[q]; before += ((zk < zi) || (zk == zi && q < i)) ? 1 : 0; }
                    }
                    zn_[before + c] = zi; sn_[before + c] = sc[i];
                    if (sidx) sidx[before + c] = i;
                }
            }
            if (sidx)
                for (int i = cnt + 16 + lane; i < T; i += 64) sidx[i] = -1;
            if (g == 0) {
                int lo = 0, hi = cnt;
                if (old_sorted) {
                    while (lo < hi) { const int md = (lo + hi) >> 1; if (zc[md] <= znew) lo = md + 1; else hi = md; }
                } else {
                    for (int q = 0; q < cnt; ++q) lo += (zc[q] <= znew) ? 1 : 0;
                }
                int c = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) { const float zj = znl[j]; c += ((zj < znew) || (zj == znew && j < n)) ? 1 : 0; }
                zn_[lo + c] = znew; sn_[lo + c] = sdf_new;
                if (sidx) sidx[lo + c] = cnt + n;
            }
            cnt += 16; cur ^= 1;
            wave_sync();
        }

        const float *zf = zs0;
        if constexpr (MODE == MODE_UPSAMPLE) {
            for (int i = lane; i < T; i += 64) {
                const size_t si = (size_t)ray * T + i;
                const float zi = zf[i];
                a.zbuf[si] = zi;
                if (a.mid_pts) {                                    // posed space: the mid points o + d * zmid (before the clamp) go to the second search
                    const float delta = (i < T - 1) ? zf[i + 1] - zi : sample_dist;
                    const float zmid = (i < T - 1) ? zi + 0.5f * delta : zi;
                    a.mid_pts[3 * si] = ox + dx * zmid; a.mid_pts[3 * si + 1] = oy + dy * zmid; a.mid_pts[3 * si + 2] = oz + dz * zmid;
                }
            }
            wave_sync();
            continue;
        }

        // ---- render core (last tile masked when 16 does not divide T) ------------------------------------------------------------------
        float cT = 1.0f;
        float *const accs = zs0 + SLAB_ACC;
        if constexpr (SH) { if (!(TR && a.opacity_only)) ray_sh_bias(zs0 + SLAB_SHB, a.Wsh, dx, dy, dz, lane); }
        const float bxe = a.eps;
        for (int c = 0; c < ntile; ++c) {
            const int i = 16 * c + n;
            const bool valid = i < T;
            const int ii = valid ? i : T - 1;
            const float zi = zf[ii];
            const float delta = (ii < T - 1) ? zf[ii + 1] - zi : sample_dist;
            const float zmid = (ii < T - 1) ? zi + 0.5f * delta : zi;
            float px, py, pz;
            // posed space: the warp's mask of this sample, and (skip_masked) a tile whose 16 samples are all masked out is not evaluated: it contributes
            // alpha * 0 whatever the field says there (wave-uniform; lanes past T count as masked)
            float mk = 1.0f;
            bool skip = false;
            if constexpr (MODE == MODE_FINAL) {
                const float *e = a.ext_pts + ((size_t)ray * T + ii) * 3;
                px = clampf(e[0], -bound, bound); py = clampf(e[1], -bound, bound); pz = clampf(e[2], -bound, bound);
                const bool live = a.mask[(size_t)ray * T + ii] != 0;
                mk = live ? 1.0f : 0.0f;
                if (a.skip_masked) skip = __ballot(valid && live) == 0ull;
            } else {
                px = clampf(ox + dx * zmid, -bound, bound); py = clampf(oy + dy * zmid, -bound, bound); pz = clampf(oz + dz * zmid, -bound, bound);
            }
            f32x4 oc = { 0.0f, 0.0f, 0.0f, 0.0f };
            float gr[3] = { 0.0f, 0.0f, 0.0f };
            if (MODE != MODE_FINAL || !skip) {
            float fe0[4][2];
            encode_stencil(lds, fsl, fc, lane, px, py, pz, bxe, fe0);
            if constexpr (TR) {
                if (ex_on && a.out.feat7) {
                    // training render: keep the 7 x 8 features of this lane, in render_rays_kernel's layout [tile of 16 samples][14][lane][4] (the host admits
                    // feat7 only when 16 divides T: every tile is whole); the lane term enters through an opaque copy, as there
                    int lane_x = lane;
                    asm volatile("" : "+v"(lane_x));
                    f32x4 *dst = reinterpret_cast<f32x4 *>(a.out.feat7) + (((size_t)exr * (T / 16) + c) * 14) * 64 + lane_x;
                    dst[0] = f32x4{ fe0[0][0], fe0[0][1], fe0[1][0], fe0[1][1] };
                    dst[64] = f32x4{ fe0[2][0], fe0[2][1], fe0[3][0], fe0[3][1] };
#pragma unroll 1
                    for (int e = 0; e < 6; ++e) {
                        const float *sp = fsl + (e * 8) * 64 + lane;
                        dst[(2 * e + 2) * 64] = f32x4{ sp[0], sp[64], sp[128], sp[192] };
                        dst[(2 * e + 3) * 64] = f32x4{ sp[256], sp[320], sp[384], sp[448] };
                    }
                }
            }
            // (render_rays_kernel's stencil, kept inline: as a shared helper it changes both renderers' code)
            const float pc0 = sel4(g, px, py, pz, 0.0f);
            float spos = 0.0f;
            if constexpr (FAST) {
                const Acc4 acc0 = sdf_l1(lds, lane, pc0, fe0);
                oc = sdf_l2(lds, lane, acc0);
#pragma unroll 1
                for (int e = 0; e < 6; ++e) {
                    const int kn = e >> 1;
                    float fe[4][2];
#pragma unroll
                    for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fsl[(e * 8 + q_) * 64 + lane];
                    const float pk = kn == 0 ? px : (kn == 1 ? py : pz);
                    const float poff = clampf(pk + ((e & 1) ? -bxe : bxe), -bound, bound);
                    const Acc4 acc = sdf_l1_delta(lds, lane, acc0, fe, fe0, kn, poff - pk);
                    const float s_e = sdf_l2_sdf(lds, acc, w2r0);
                    if (!(e & 1)) spos = s_e;
                    else {
                        const float gk = 0.5f * (spos - s_e) / bxe;
                        if (kn == 0) gr[0] = gk; else if (kn == 1) gr[1] = gk; else gr[2] = gk;
                    }
                }
            } else {
            Acc4 acc = sdf_l1(lds, lane, pc0, fe0);
#pragma unroll 1
            for (int e = 0; e < 7; ++e) {
                Acc4 accn = acc;
                if (e < 6) {
                    const int kn = e >> 1;
                    float fe[4][2];
#pragma unroll
                    for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fsl[(e * 8 + q_) * 64 + lane];
                    const float pk = kn == 0 ? px : (kn == 1 ? py : pz);
                    const float poff = clampf(pk + ((e & 1) ? -bxe : bxe), -bound, bound);
                    accn = sdf_l1(lds, lane, g == kn ? poff : pc0, fe);
                }
                if (e == 0) oc = sdf_l2(lds, lane, acc);
                else {
                    const float s_e = sdf_l2_sdf(lds, acc, w2r0);
                    const int kk = (e - 1) >> 1;
                    if (e & 1) spos = s_e;
                    else {
                        const float gk = 0.5f * (spos - s_e) / bxe;
                        if (kk == 0) gr[0] = gk; else if (kk == 1) gr[1] = gk; else gr[2] = gk;
                    }
                }
                acc = accn;
            }
            }
            }
            const float gx = gr[0], gy = gr[1], gz = gr[2];
            const FdNormal nrm = fd_normal(gx, gy, gz);
            const float gn = nrm.gn, nx = nrm.nx, ny = nrm.ny, nz = nrm.nz;
            float rgb[3] = { 0.0f, 0.0f, 0.0f };
            if ((MODE != MODE_FINAL || !skip) && !(TR && a.opacity_only)) {       // (wave-uniform; opacity_only: a black body)
            if constexpr (FC) color_tile_fast(lds, lane, px, py, pz, nx, ny, nz, oc, rgb, nullptr, 16, SH ? zs0 + SLAB_SHB : nullptr);
            else color_tile(lds, lane, px, py, pz, nx, ny, nz, oc, rgb, nullptr, 16, SH ? zs0 + SLAB_SHB : nullptr);
            }
            const float sdf0 = oc[0];
            // (neus_alpha's arithmetic, inline: through the helper this kernel's code changes)
            const float tc = (dx * nx + dy * ny) + dz * nz;
            const float a1 = dv_softplus100(lds + OFF_SPQ, -tc * 0.5f + 0.5f) * a.one_m_car;
            const float a2 = dv_softplus100(lds + OFF_SPQ, -tc) * a.car;
            const float iter_cos = -(a1 + a2);
            const float half = iter_cos * delta * 0.5f;
            const float pc = dv_sigmoid((sdf0 - half) * inv_s_core), nc = dv_sigmoid((sdf0 + half) * inv_s_core);
            float alpha = valid ? clampf((pc - nc + 1e-5f) / (pc + 1e-5f), 0.0f, 1.0f) : 0.0f;
            if constexpr (MODE == MODE_FINAL) alpha = alpha * mk;
            const float om = valid ? 1.0f - alpha + 1e-7f : 1.0f;              // masked lanes: the identity of the product scan
            const float loc = row_scan<true>(om);
            const float sh = dpp_shr<1>(1.0f, loc);
            float Tex;
            if (n == 0) Tex = (c == 0) ? 1.0f : cT;
            else Tex = (c == 0) ? sh : cT * sh;
            const float tot = lane_bcast(loc, 15);
            cT = (c == 0) ? tot : cT * tot;
            const float wgt = alpha * Tex;
            const float zn01 = clampf((zi - near) / span, 0.0f, 1.0f);
            const float pn = __builtin_sqrtf((px * px + py * py) + pz * pz);
            const float relax = (pn < 1.2f && valid && !(MODE == MODE_FINAL && skip)) ? 1.0f : 0.0f;
            const float eerr = relax * ((gn - 1.0f) * (gn - 1.0f));
            {
                // masked lanes add exact zeros (x + 0 = x): wgt = 0 there, and every factor it meets is finite whenever the ray's own last
                // sample is (a masked lane evaluates that very point again)
                const float t1 = row_scan<false>(wgt), t2 = row_scan<false>(rgb[0] * wgt), t3 = row_scan<false>(rgb[1] * wgt), t4 = row_scan<false>(rgb[2] * wgt),
                            t5 = row_scan<false>(nx * wgt), t6 = row_scan<false>(ny * wgt), t7 = row_scan<false>(nz * wgt), t8 = row_scan<false>(wgt * zn01),
                            t9 = row_scan<false>(eerr), t10 = row_scan<false>(relax);
                if (lane == 15) {
#define AC_ACC(K, T_) accs[K] = (c == 0) ? T_ : accs[K] + T_;
                    AC_ACC(1, t1) AC_ACC(2, t2) AC_ACC(3, t3) AC_ACC(4, t4) AC_ACC(5, t5) AC_ACC(6, t6) AC_ACC(7, t7) AC_ACC(8, t8) AC_ACC(9, t9) AC_ACC(10, t10)
#undef AC_ACC
                }
            }
            if (g == 0 && valid && ex_on) {
                const size_t si = (size_t)exr * T + i;
                if (EX && a.out.z_vals) a.out.z_vals[si] = zi;
                if (EX && a.out.weights) a.out.weights[si] = wgt;
                if (EX && a.out.alpha) a.out.alpha[si] = alpha;
                if (EX && a.out.sdf) a.out.sdf[si] = sdf0;
                if (EX && a.out.color) { a.out.color[3 * si] = rgb[0]; a.out.color[3 * si + 1] = rgb[1]; a.out.color[3 * si + 2] = rgb[2]; }
                if (EX && a.out.gradient) { a.out.gradient[3 * si] = gx; a.out.gradient[3 * si + 1] = gy; a.out.gradient[3 * si + 2] = gz; }
                if (EX && a.out.pts) { a.out.pts[3 * si] = px; a.out.pts[3 * si + 1] = py; a.out.pts[3 * si + 2] = pz; }
            }
            if (EX && valid && ex_on && a.out.sdf_out16)
                *reinterpret_cast<f32x4 *>(a.out.sdf_out16 + ((size_t)exr * T + i) * 16 + 4 * g) = oc;
        }
        wave_sync();
        if (lane == 0) {
            const float s_w = accs[1], s_r = accs[2], s_g = accs[3], s_b = accs[4], s_nx = accs[5], s_ny = accs[6], s_nz = accs[7], s_d = accs[8], s_en = accs[9], s_ed = accs[10];
            const float b0 = a.bg ? a.bg[3 * ray] : 1.0f, b1 = a.bg ? a.bg[3 * ray + 1] : 1.0f, b2 = a.bg ? a.bg[3 * ray + 2] : 1.0f;
            a.out.image[3 * ray] = s_r + (1.0f - s_w) * b0;
            a.out.image[3 * ray + 1] = s_g + (1.0f - s_w) * b1;
            a.out.image[3 * ray + 2] = s_b + (1.0f - s_w) * b2;
            a.out.normal_map[3 * ray] = s_nx; a.out.normal_map[3 * ray + 1] = s_ny; a.out.normal_map[3 * ray + 2] = s_nz;
            a.out.weights_sum[ray] = s_w;
            a.out.depth[ray] = s_d;
            a.out.eik[2 * ray] = s_en; a.out.eik[2 * ray + 1] = s_ed;
        }
        wave_sync();
    }
}

template <int MODE, bool FAST, bool EX, bool SH>
static void launch_long_p(const RenderArgs &a, hipStream_t stream)
{
    static uint64_t seen = 0;
    const size_t lds_bytes = LDS_FLOATS * sizeof(float);
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(render_rays_long_kernel<MODE, FAST, EX, SH>), lds_bytes);
    int blocks = (a.n_rays + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const int cus = (int)ac::cu_count();
    if (blocks > cus) blocks = cus;
    blocks = (blocks + 7) & ~7;                                      // the hand-out assumes every XCD has the same number of workgroups
    hipLaunchKernelGGL((render_rays_long_kernel<MODE, FAST, EX, SH>), dim3(blocks), dim3(BLOCK), lds_bytes, stream, a);
}

// the training options of the canonical launch (pair launch, opacity_only, feat7) are compiled into its EX instantiations only
template <int MODE>
static void launch_long(const RenderArgs &a, hipStream_t st)
{
    if constexpr (MODE == MODE_UPSAMPLE) {                                      // (the sampling launch can export the sample indices)
        if (!a.out.ss_inds && !a.out.sort_index) launch_long_p<MODE, false, false, false>(a, st);
        else launch_long_p<MODE, false, true, false>(a, st);
    } else {
        const bool ex = wants_samples(a.out) || (MODE == MODE_FULL && (a.pair_n || a.opacity_only));
        dispatch_variants(a.fast, ex, a.Wsh != nullptr, [&](auto fast, auto ex_, auto sh) {
            launch_long_p<MODE, decltype(fast)::value, decltype(ex_)::value, decltype(sh)::value>(a, st);
        });
    }
}

}  // namespace

AC_API int ac_render_rays_long(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                               const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                               const ac_render_out *out, ac_stream_t stream)
{
    static const RenderEntry d("render_rays_long", K_LONG);
    const RayInputs in = { rays_o, rays_d, bg, noise, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, nullptr, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, out)) return rc;
    launch_long<MODE_FULL>(a, (hipStream_t)stream);
    if (int rc = ac::check_launch(d.name)) return rc;
    // gradient_error in the fixed order the other renderer's last workgroup uses (eikonal_reduce_kernel's): bit-identical
    if (out->eik_reduced) return ac_eikonal_reduce2(out->eik, op->n_rays, out->eik_reduced, stream);
    return AC_OK;
}

// ac_render_rays_pair at the long counts: the same N rays twice in one launch (two noise draws, two backgrounds).  The 2N work items go through the static
// hand-out unchanged (chunks of 512 items, chunk c to XCD c % 8), the two copies of a ray as consecutive items of one chunk; no scratch, no counters, no
// hand-off.  The rays are independent: every value equals two ac_render_rays_long calls bit for bit.  gradient_error of each copy: ac_eikonal_reduce2.
AC_API int ac_render_rays_long_pair(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                                    const float *bg2, const float *noise2, const float *lin_z, const float *lin_u,
                                    const ac_render_out *out, ac_stream_t stream)
{
    static const RenderEntry d("render_rays_long_pair", K_LONG | K_PAIR);
    const RayInputs in = { rays_o, rays_d, bg2, noise2, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, nullptr, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, out)) return rc;
    make_pair_args(a);
    launch_long<MODE_FULL>(a, (hipStream_t)stream);
    if (int rc = ac::check_launch(d.name)) return rc;
    if (out->eik_reduced) {
        if (int rc = ac_eikonal_reduce2(out->eik, op->n_rays, out->eik_reduced, stream)) return rc;
        return ac_eikonal_reduce2(out->eik + 2 * (size_t)op->n_rays, op->n_rays, out->eik_reduced + 2, stream);
    }
    return AC_OK;
}

AC_API int ac_sample_rays_long(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d, const float *noise,
                               const float *lin_z, const float *lin_u, float *z_vals, ac_stream_t stream)
{
    static const RenderEntry d("sample_rays_long", K_LONG | K_SAMPLING);
    const RayInputs in = { rays_o, rays_d, nullptr, noise, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, nullptr, nullptr, z_vals)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, nullptr)) return rc;
    a.zbuf = z_vals;
    launch_long<MODE_UPSAMPLE>(a, (hipStream_t)stream);
    return ac::check_launch(d.name);
}

// Posed space at the long counts: the posed sequence (render_entry.hpp: render_posed) on this kernel's MODE_UPSAMPLE and MODE_FINAL.
// Scratch: ac_render_rays_warped_scratch(n_rays, T, offs).
AC_API int ac_render_rays_long_warped(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                                      const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                                      const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out,
                                      ac_stream_t stream)
{
    static const RenderEntry d("render_rays_long_warped", K_LONG | K_POSED);
    const RayInputs in = { rays_o, rays_d, bg, noise, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, mesh, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, out)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = render_posed(d, a, mesh, scratch, scratch_bytes, stream, [&](const RenderArgs &b) { launch_long<MODE_UPSAMPLE>(b, st); },
                              [&](const RenderArgs &b) { launch_long<MODE_FINAL>(b, st); })) return rc;
    if (out->eik_reduced) return ac_eikonal_reduce2(out->eik, op->n_rays, out->eik_reduced, stream);
    return AC_OK;
}
