// avatarcraft_amd/csrc/hash_stencil.hip -- the hash-grid encoder on the 7-point finite-difference stencil (training path).
//
// One SDF query of the render core is 7 encoder calls in the reference: the sample x (forward_sdf, models/instant_nsr.py:627-642)
// and x +- eps e_k clamped to the bound (finite_difference_normals_approximator, :687-704), each through
// HashEncoder.forward / _hash_encode.backward (encoder/hashencoder/hashgrid.py:11-73,126-142).  This operator evaluates the seven
// points of every sample in one launch.  Its backward to the table collapses, on the levels where eps spans less than one cell (all seven points
// lie in the same or a neighbouring cell), the 7 x 8 corners onto at most 32 distinct table entries (normally 8) in registers (stencil_scatter)
// and hands them to the table-gradient scatter (table_scatter.hpp: run scan, queues per bucket, sums in LDS).  The same scatter serves the
// reference's one-point operator (hash_bwd_binned_kernel); grid addressing is grid_cell.hpp's.
// This file: the stencil operator (forward, input backward, the collapse and its two table-backward kernels), the one-point fill kernel, the C entry points.
//
// Point order p = 0..6: x, +x, -x, +y, -y, +z, -z.  Layouts: x [B,3] fp32 world space (already clamped to the bound, as the
// render core passes it); features / their gradient [7, L, B, 2] (level-major like the reference's [L,B,C] kernel output).
#include "table_scatter.hpp"

namespace {

__device__ __forceinline__ float offset_coord(float xc, int sign, float eps, float bound)
{
    return clampf(xc + (sign ? -eps : eps), -bound, bound);
}

// ---- forward: out[p][level][b][0..1] ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hash_stencil_fwd_kernel(const float *__restrict__ x, const float *__restrict__ grid,
                                                               float *__restrict__ out, uint32_t B, ac::LevelTable lt, float eps,
                                                               float bound, float two_bound)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y, Lc = lt.L;
    const LevelC L = level_of(lt, level);
    const float2 *g = reinterpret_cast<const float2 *>(grid) + lt.offset[level];
    const float xc[3] = { x[3 * (size_t)b], x[3 * (size_t)b + 1], x[3 * (size_t)b + 2] };
    Loc c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = locate(xc[d], bound, two_bound, L.scale);
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        Loc q[3] = { c[0], c[1], c[2] };
        if (p > 0) { const int k = (p - 1) >> 1; q[k] = locate(offset_coord(xc[k], (p - 1) & 1, eps, bound), bound, two_bound, L.scale); }
        float a0 = 0.0f, a1 = 0.0f;
        if (!(q[0].oob | q[1].oob | q[2].oob)) {
#pragma unroll
            for (uint32_t idx = 0; idx < 8; ++idx) {
                float w = 1.0f; uint32_t pl[3];
#pragma unroll
                for (uint32_t d = 0; d < 3; ++d) {
                    if ((idx & (1u << d)) == 0) { w *= 1.0f - q[d].fr; pl[d] = q[d].pg; }
                    else { w *= q[d].fr; pl[d] = q[d].pg + 1u; }
                }
                const float2 f = g[gindex(L, pl[0], pl[1], pl[2])];
                a0 = fma_(w, f.x, a0); a1 = fma_(w, f.y, a1);
            }
        }
        reinterpret_cast<float2 *>(out)[((size_t)p * Lc + level) * B + b] = make_float2(a0, a1);
    }
}

// ---- backward to the INPUT: d loss / d x through the seven encodings ------------------------------------------------------------------
// What the reference does with dy_dx (kernel_grid's derivative branch, hashencoder.cu:177-220, and kernel_input_backward, :311-337) for a sample whose
// position itself carries a gradient -- the curvature term's perturbed points (models/instant_nsr.py:276-288: they are a function of the normal).  Nothing
// is stored: the eight corners of every stencil point are gathered again and the derivative of the trilinear weights is formed in registers.
//   gx_part[grp][b][d] = sum over the levels of group grp (4 levels each), points p, channels c of
//        gfeat[p][level][b][c] * scale * sum_{corners of the two other axes} w_other * (T[corner + e_d] - T[corner])[c] / (2 bound) * pass_p,d
// pass = the derivative of the offset point's clamp (1 inside [-bound, bound], torch.clamp's inclusive rule; finite_difference_normals_approximator :690-702).
__global__ __launch_bounds__(256) void hash_stencil_input_bwd_kernel(const float *__restrict__ gfeat, const float *__restrict__ x, const float *__restrict__ grid,
                                                                     float *__restrict__ gx_part, uint32_t B, ac::LevelTable lt, float eps, float bound,
                                                                     float two_bound)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t Lc = lt.L;
    const float xc[3] = { x[3 * (size_t)b], x[3 * (size_t)b + 1], x[3 * (size_t)b + 2] };
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    for (uint32_t level = blockIdx.y * 4; level < blockIdx.y * 4 + 4 && level < Lc; ++level) {
        const LevelC L = level_of(lt, level);
        const float2 *g = reinterpret_cast<const float2 *>(grid) + lt.offset[level];
        Loc c[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) c[d] = locate(xc[d], bound, two_bound, L.scale);
#pragma unroll 1
        for (int p = 0; p < 7; ++p) {
            const float2 gf = reinterpret_cast<const float2 *>(gfeat)[((size_t)p * Lc + level) * B + b];
            if (gf.x == 0.0f && gf.y == 0.0f) continue;                  // (the centre of a gradient-only use, masked samples)
            Loc q[3] = { c[0], c[1], c[2] };
            const int k = p > 0 ? (p - 1) >> 1 : 3;
            float pass = 1.0f;
            if (p > 0) {
                const float raw = xc[k] + (((p - 1) & 1) ? -eps : eps);
                pass = (raw >= -bound && raw <= bound) ? 1.0f : 0.0f;
                q[k] = locate(clampf(raw, -bound, bound), bound, two_bound, L.scale);
            }
            if (q[0].oob | q[1].oob | q[2].oob) continue;                // (hashencoder.cu:95-119: an out-of-range input has zero output and zero dy_dx)
            float2 f[8];
#pragma unroll
            for (uint32_t idx = 0; idx < 8; ++idx)
                f[idx] = g[gindex(L, q[0].pg + (idx & 1u), q[1].pg + ((idx >> 1) & 1u), q[2].pg + ((idx >> 2) & 1u))];
#pragma unroll
            for (uint32_t d = 0; d < 3; ++d) {
                const uint32_t da = (d == 0) ? 1u : 0u, db = (d == 2) ? 1u : 2u;
                float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
                for (uint32_t jm = 0; jm < 4; ++jm) {
                    const float w = ((jm & 1u) ? q[da].fr : 1.0f - q[da].fr) * ((jm >> 1) ? q[db].fr : 1.0f - q[db].fr);
                    const uint32_t left = ((jm & 1u) << da) | ((jm >> 1) << db), right = left | (1u << d);
                    s0 = fma_(w, f[right].x - f[left].x, s0); s1 = fma_(w, f[right].y - f[left].y, s1);
                }
                const float dd = L.scale * fma_(s0, gf.x, s1 * gf.y) / two_bound;
                acc[d] += ((int)d == k) ? dd * pass : dd;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) gx_part[((size_t)blockIdx.y * B + b) * 3 + d] = acc[d];
}

// ---- backward to the table -------------------------------------------------------------------------------------------------------
// the seven stencil points of one sample per lane (64 consecutive samples per wave) on one level.
// fine: eps can reach a non-neighbouring cell on this level -> the seven points scatter independently
template <class Sink>
__device__ __forceinline__ void stencil_scatter(Sink &sink, const LevelC &L, bool fine, const float (&xc)[3], const float2 (&gp)[7], float eps,
                                                float bound, float two_bound, int lane, float inv_tb = 0.0f)
{
    Loc c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = locate(xc[d], bound, two_bound, L.scale, inv_tb);
    const bool cen_ok = !(c[0].oob | c[1].oob | c[2].oob);
    bool bad = false;
#pragma unroll
    for (int p = 0; p < 7; ++p) bad |= nonfinite(gp[p].x) | nonfinite(gp[p].y);
    const bool norun = __any(bad);                       // wave-uniform: Inf / NaN somewhere in this group of 64 samples (see run_reduce)

    if (fine || norun || !__all(cen_ok)) {               // wave-uniform: every lane takes the same path (shuffles inside)
#pragma unroll
        for (int p = 0; p < 7; ++p) {
            Loc q[3] = { c[0], c[1], c[2] };
            if (p > 0) { const int k = (p - 1) >> 1; q[k] = locate(offset_coord(xc[k], (p - 1) & 1, eps, bound), bound, two_bound, L.scale, inv_tb); }
            scatter8_runs(sink, L, q, gp[p].x, gp[p].y, lane, norun);
        }
        return;
    }
    // combine the seven points: v[2*idx+c] = the 8 corners of the centre cell; v[16 + ((k*2+side)*4+jm)*2 + c] = the 4 corners one
    // plane below (side 0) / above (side 1) the centre cell along axis k (jm = corner bits of the two other axes, in axis order)
    float v[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = 0.0f;
    const float wd[3][2] = { { 1.0f - c[0].fr, c[0].fr }, { 1.0f - c[1].fr, c[1].fr }, { 1.0f - c[2].fr, c[2].fr } };
#pragma unroll
    for (uint32_t idx = 0; idx < 8; ++idx) {
        float w = 1.0f;
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) w *= wd[d][(idx >> d) & 1u];
        v[2 * idx] = w * gp[0].x; v[2 * idx + 1] = w * gp[0].y;
    }
    // products of the two off-axis weights of a face corner, shared by the two offset points of an axis: pw[k][jm], jm = corner bits of the other two axes
    float pw[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int da = (k == 0) ? 1 : 0, db = (k == 2) ? 1 : 2;
#pragma unroll
        for (uint32_t jm = 0; jm < 4; ++jm) pw[k][jm] = wd[da][jm & 1u] * wd[db][jm >> 1];
    }
    // Corner bit b (along axis k) of an offset point lies on plane delta + b of the centre cell, delta = its cell minus the centre's: 0, or +1 for
    // x + eps / -1 for x - eps on a coarse level.  Planes 0 and 1 are the centre cell's own corners, -1 and 2 the neighbour planes.  The two cases
    // are weighted with {0, 1} masks folded into the corner weight -- 4 fma per corner instead of 8 selects + 8 adds (round 3: the combine was 36 %
    // of the fill's time, tools/fill_profile.py).
#pragma unroll
    for (int p = 1; p < 7; ++p) {
        const int k = (p - 1) >> 1, sign = (p - 1) & 1;                 // sign 0: + eps, 1: - eps (offset_coord)
        const Loc q = locate(offset_coord(xc[k], sign, eps, bound), bound, two_bound, L.scale, inv_tb);
        const float live = q.oob ? 0.0f : 1.0f;
        const int delta = (int)q.pg - (int)c[k].pg;
        const float m0 = (delta == 0) ? live : 0.0f, m1 = (delta == (sign ? -1 : 1)) ? live : 0.0f;
        const float wk[2] = { 1.0f - q.fr, q.fr };
#pragma unroll
        for (uint32_t jm = 0; jm < 4; ++jm) {
            const uint32_t lo = jm & 1u, hi = jm >> 1;
            const uint32_t c0 = (k == 0) ? ((lo << 1) | (hi << 2)) : (k == 1) ? (lo | (hi << 2)) : (lo | (hi << 1));      // centre corner with bit k = 0
            const uint32_t c1 = c0 | (1u << k);
            const uint32_t e0 = 16 + ((k * 2 + 0) * 4 + jm) * 2, e1 = 16 + ((k * 2 + 1) * 4 + jm) * 2;
#pragma unroll
            for (uint32_t b = 0; b < 2; ++b) {
                const float w = pw[k][jm] * wk[b], wa = w * m0, wb = w * m1;
                const uint32_t ta = 2 * (b ? c1 : c0);                                      // same cell as the centre: plane b
                const uint32_t tb = sign ? (b ? 2 * c0 : e0) : (b ? e1 : 2 * c1);           // neighbouring cell: plane b - 1 / b + 1
                v[ta] = __builtin_fmaf(wa, gp[p].x, v[ta]); v[ta + 1] = __builtin_fmaf(wa, gp[p].y, v[ta + 1]);
                v[tb] = __builtin_fmaf(wb, gp[p].x, v[tb]); v[tb + 1] = __builtin_fmaf(wb, gp[p].y, v[tb + 1]);
            }
        }
    }
    const bool tail = run_reduce<64>(v, run_head(c, true, lane), lane);
    sink.tick(0);
    // the centre cell's pre-multiplied terms: every one of the 32 entries below is these plus / minus multiples of (1, cmy, cmz) (gindex_t)
    const uint32_t cmy = level_my(L), cmz = level_mz(L), cty = c[1].pg * cmy, ctz = c[2].pg * cmz;
    if constexpr (Sink::packs) {
        // After the run combining only the TAIL lanes carry anything -- a handful per wave on the coarse levels -- and the four add8 calls below walk 32 entries with
        // a tenth of the lanes live (half of the fill's time: tools/fill_profile.py, round 6).  With few tails the work is transposed through LDS instead: a chunk of
        // 8 tails stages, per group of 8 entries, its 16 values (+ once: the cell's axis terms), and lane j of the wave forms the record of (tail j / 8, entry j % 8)
        // -- one dense pass per group instead of eight sparse ones.  The same (entry, v0, v1) contributions reach the queues (their order does not enter the sums).
        const unsigned long long T = __ballot(tail);
        const int nt = __builtin_popcountll(T);
        if (nt <= AC_FILL_PACK_MAX) {
            const int myrank = __builtin_popcountll(T & ((1ull << lane) - 1ull));
            const int t = lane >> 3, k = lane & 7;
            float *const st = sink.stage;
            for (int base = 0; base < nt; base += PACK_TAILS) {
                const bool mine = tail && myrank >= base && myrank < base + PACK_TAILS;
                float *const row = st + (myrank - base) * PACK_STRIDE;
                const bool valid = base + t < nt;
                uint32_t q0 = 0u, qy = 0u, qz = 0u;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (mine) {
#pragma unroll
                        for (int w = 0; w < 4; ++w)
                            *reinterpret_cast<float4 *>(row + 4 * w) = make_float4(v[16 * g + 4 * w], v[16 * g + 4 * w + 1], v[16 * g + 4 * w + 2], v[16 * g + 4 * w + 3]);
                        if (g == 0) { row[16] = __uint_as_float(c[0].pg); row[17] = __uint_as_float(cty); row[18] = __uint_as_float(ctz); }
                    }
                    wave_sync();
                    const float2 val = *reinterpret_cast<const float2 *>(st + t * PACK_STRIDE + 2 * k);
                    if (g == 0) { q0 = __float_as_uint(st[t * PACK_STRIDE + 16]); qy = __float_as_uint(st[t * PACK_STRIDE + 17]); qz = __float_as_uint(st[t * PACK_STRIDE + 18]); }
                    uint32_t tx, ty, tz;
                    if (g == 0) {                                   // the centre cell's corner k
                        tx = q0 + ((uint32_t)k & 1u); ty = qy + ((k & 2) ? cmy : 0u); tz = qz + ((k & 4) ? cmz : 0u);
                    } else {                                        // slot k = side * 4 + jm of the two planes next to the cell along axis g - 1
                        const bool lo = (k & 1) != 0, hi = (k & 2) != 0, side = (k & 4) != 0;
                        if (g == 1) { tx = side ? q0 + 2u : q0 - 1u; ty = qy + (lo ? cmy : 0u); tz = qz + (hi ? cmz : 0u); }
                        else if (g == 2) { tx = q0 + (lo ? 1u : 0u); ty = side ? qy + 2u * cmy : qy - cmy; tz = qz + (hi ? cmz : 0u); }
                        else { tx = q0 + (lo ? 1u : 0u); ty = qy + (hi ? cmy : 0u); tz = side ? qz + 2u * cmz : qz - cmz; }
                    }
                    sink.add1(valid && (val.x != 0.0f || val.y != 0.0f), gindex_t(L, tx, ty, tz), val.x, val.y);
                    wave_sync();                                // (the next group's values overwrite the rows)
                }
            }
            sink.tick(1);
            return;
        }
    }
    {
        bool pred[8]; float vv[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) { vv[2 * k] = v[2 * k]; vv[2 * k + 1] = v[2 * k + 1]; pred[k] = tail && (v[2 * k] != 0.0f || v[2 * k + 1] != 0.0f); }
        sink.add8(pred, [&](int k) { return cell_corner(L, c[0].pg, cty, ctz, cmy, cmz, (uint32_t)k); }, vv);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                            // the two planes next to the centre cell along axis k: slot n = side * 4 + jm
        bool pred[8]; float vv[16];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const uint32_t e = 16 + (k * 8 + n) * 2;
            vv[2 * n] = v[e]; vv[2 * n + 1] = v[e + 1]; pred[n] = tail && (v[e] != 0.0f || v[e + 1] != 0.0f);
        }
        sink.add8(pred, [&](int n) {
            const uint32_t jm = (uint32_t)n & 3u, lo = jm & 1u, hi = jm >> 1;
            const uint32_t m3[3] = { 1u, cmy, cmz };
            uint32_t t[3];
            t[0] = c[0].pg + (k == 0 ? 0u : lo);
            t[1] = cty + ((k == 1 ? 0u : (k == 0 ? lo : hi)) ? cmy : 0u);
            t[2] = ctz + ((k == 2 ? 0u : hi) ? cmz : 0u);
            const uint32_t base = k == 0 ? c[0].pg : (k == 1 ? cty : ctz);
            t[k] = (n >> 2) ? base + 2u * m3[k] : base - m3[k];                  // plane + 2 / - 1 along axis k (32-bit wrap-around like the product's)
            return gindex_t(L, t[0], t[1], t[2]);
        }, vv);
    }
    sink.tick(1);
}

// direct atomics: one sample per thread, level = blockIdx.y in [0, n_levels)
__global__ __launch_bounds__(256) void hash_stencil_bwd_kernel(const float *__restrict__ grad, const float *__restrict__ x,
                                                               float *__restrict__ grad_grid, uint32_t B, ac::LevelTable lt, float eps,
                                                               float bound, float two_bound, uint32_t fine_mask, float *__restrict__ priv,
                                                               uint32_t n_priv, uint32_t priv_entries, uint32_t n_copies, uint32_t direct_mask)
{
    const uint32_t level = blockIdx.y, Lc = lt.L;
    if (!((direct_mask >> level) & 1u)) return;          // this level goes through the binned path
    const uint32_t b0 = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = b0 < B;
    const uint32_t b = valid ? b0 : B - 1;
    const int lane = threadIdx.x & 63;
    const LevelC L = level_of(lt, level);
    // the small dense levels take bursts of same-address atomics from neighbouring rays: spread them over n_copies private
    // copies (one per workgroup, round robin), summed into the table by priv_reduce_kernel
    DirectSink sink;
    sink.gg = (level < n_priv) ? reinterpret_cast<float2 *>(priv) + (size_t)(blockIdx.x % n_copies) * priv_entries + lt.offset[level]
                               : reinterpret_cast<float2 *>(grad_grid) + lt.offset[level];
    const float xc[3] = { x[3 * (size_t)b], x[3 * (size_t)b + 1], x[3 * (size_t)b + 2] };
    float2 gp[7];
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        gp[p] = reinterpret_cast<const float2 *>(grad)[((size_t)p * Lc + level) * B + b];
        if (!valid) gp[p] = make_float2(0.0f, 0.0f);
    }
    stencil_scatter(sink, L, ((fine_mask >> level) & 1u) != 0, xc, gp, eps, bound, two_bound, lane);
}

// binned path: blockIdx.y indexes the binned levels; every wave walks over groups of 64 samples and flushes its record buffer
// when the next batch might not fit
__global__ __launch_bounds__(256) void hash_stencil_bwd_binned_kernel(const float *__restrict__ grad, const float *__restrict__ x,
                                                                      float *__restrict__ grad_grid, uint32_t B, ac::LevelTable lt, float eps,
                                                                      float bound, float two_bound, uint32_t fine_mask, uint32_t binned_mask,
                                                                      uint32_t *__restrict__ qcount, Rec *__restrict__ queues, uint32_t cap, float inv_tb)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    // the finest levels cost 2.5x the coarse ones (every stencil point scatters on its own): dispatch them FIRST, so that the cheap
    // levels fill the tail of the launch.  ylev = which binned level this workgroup serves (queue / counter index), highest first.
    const uint32_t ylev = gridDim.y - 1u - blockIdx.y;
    const uint32_t level = level_of_rank(binned_mask, lt, ylev);
    const uint32_t Lc = lt.L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LevelC L = level_of(lt, level);
    BinSink sink;
    sink.init(smem + wave * WAVE_WORDS, lane, lt, level, ylev, gridDim.y, qcount, queues, cap, grad_grid);
    const bool fine = ((fine_mask >> level) & 1u) != 0;
    const uint32_t ngroups = (B + 63) / 64;
    // the next group's position and seven feature gradients are requested before this group is scattered (round 4)
    struct GroupIn { float xc[3]; float2 gp[7]; };
    auto request = [&](uint32_t grp, GroupIn &in) {
        const uint32_t b0 = grp * 64 + lane;
        const bool valid = b0 < B;
        const uint32_t b = valid ? b0 : B - 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) in.xc[k] = x[3 * (size_t)b + k];
#pragma unroll
        for (int p = 0; p < 7; ++p) {
            in.gp[p] = reinterpret_cast<const float2 *>(grad)[((size_t)p * Lc + level) * B + b];
            if (!valid) in.gp[p] = make_float2(0.0f, 0.0f);
        }
    };
    const uint32_t grp0 = blockIdx.x * 4 + wave, gstride = gridDim.x * 4;
    GroupIn nxt;
    if (grp0 < ngroups) request(grp0, nxt);
    for (uint32_t grp = grp0; grp < ngroups; grp += gstride) {
        const float xc[3] = { nxt.xc[0], nxt.xc[1], nxt.xc[2] };
        float2 gp[7];
#pragma unroll
        for (int p = 0; p < 7; ++p) gp[p] = nxt.gp[p];
        if (grp + gstride < ngroups) request(grp + gstride, nxt);
        stencil_scatter(sink, L, fine, xc, gp, eps, bound, two_bound, lane, inv_tb);
    }
    sink.finish();
    sink.report(level);                                  // (AC_PROFILE_FILL builds: tools/fill_profile.py)
}

// the reference's one-point backward (kernel_grid_backward, hashencoder.cu:223-308; D = 3, C = 2) through the binned scatter:
// inputs [B,3] in [0,1], grad [L,B,2]; one sample per lane, runs of lanes in the same cell are combined like in the stencil path
__global__ __launch_bounds__(256) void hash_bwd_binned_kernel(const float *__restrict__ grad, const float *__restrict__ inputs,
                                                              float *__restrict__ grad_grid, uint32_t B, ac::LevelTable lt, uint32_t binned_mask,
                                                              uint32_t *__restrict__ qcount, Rec *__restrict__ queues, uint32_t cap)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t ylev = gridDim.y - 1u - blockIdx.y;            // finest level first (see hash_stencil_bwd_binned_kernel)
    const uint32_t level = level_of_rank(binned_mask, lt, ylev);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LevelC L = level_of(lt, level);
    BinSink sink;
    sink.init(smem + wave * WAVE_WORDS, lane, lt, level, ylev, gridDim.y, qcount, queues, cap, grad_grid);
    const uint32_t ngroups = (B + 63) / 64;
    for (uint32_t grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
        const uint32_t b0 = grp * 64 + lane;
        const bool valid = b0 < B;
        const uint32_t b = valid ? b0 : B - 1;
        Loc q[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) q[d] = locate_unit(inputs[(size_t)b * 3 + d], L.scale);
        float2 g = reinterpret_cast<const float2 *>(grad)[(size_t)level * B + b];
        if (!valid) g = make_float2(0.0f, 0.0f);
        scatter8_runs(sink, L, q, g.x, g.y, lane, __any(nonfinite(g.x) | nonfinite(g.y)) != 0);
    }
    sink.finish();
}

int check(const char *who, uint32_t C, uint32_t L, const int32_t *offsets_host, float eps, float bound)
{
    if (C != 2) { ac::set_error("%s: level_dim must be 2, got %u", who, C); return AC_ERR_BAD_ARG; }
    if (L == 0 || L > AC_MAX_LEVELS) { ac::set_error("%s: L=%u out of range (1..%d)", who, L, AC_MAX_LEVELS); return AC_ERR_BAD_ARG; }
    if (!offsets_host) { ac::set_error("%s: offsets_host is NULL", who); return AC_ERR_BAD_ARG; }
    if (!(eps > 0.0f) || !(bound > 0.0f)) { ac::set_error("%s: eps and bound must be positive", who); return AC_ERR_BAD_ARG; }
    return AC_OK;
}

}  // namespace

AC_API int ac_hash_stencil_forward(const float *x, const float *embeddings, const int32_t *offsets_host, float *outputs, uint32_t B,
                                   uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, ac_stream_t stream)
{
    if (int rc = check("hash_stencil_forward", C, L, offsets_host, eps, bound)) return rc;
    if (B == 0) return AC_OK;
    if (!x || !embeddings || !outputs) { ac::set_error("hash_stencil_forward: NULL buffer"); return AC_ERR_BAD_ARG; }
    ac::LevelTable lt; ac::make_level_table(lt, L, 3, S, H, offsets_host);
    hipLaunchKernelGGL(hash_stencil_fwd_kernel, dim3((B + 255) / 256, L), dim3(256), 0, (hipStream_t)stream, x, embeddings, outputs, B, lt, eps,
                       bound, (float)(2.0 * (double)bound));
    return ac::check_launch("hash_stencil_forward");
}

AC_API int ac_hash_stencil_input_backward(const float *gfeat, const float *x, const float *embeddings, const int32_t *offsets_host, float *gx_part,
                                          uint32_t B, uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, ac_stream_t stream)
{
    if (int rc = check("hash_stencil_input_backward", C, L, offsets_host, eps, bound)) return rc;
    if (B == 0) return AC_OK;
    if (!gfeat || !x || !embeddings || !gx_part) { ac::set_error("hash_stencil_input_backward: NULL buffer"); return AC_ERR_BAD_ARG; }
    ac::LevelTable lt; ac::make_level_table(lt, L, 3, S, H, offsets_host);
    hipLaunchKernelGGL(hash_stencil_input_bwd_kernel, dim3((B + 255) / 256, (L + 3) / 4), dim3(256), 0, (hipStream_t)stream, gfeat, x, embeddings, gx_part, B,
                       lt, eps, bound, (float)(2.0 * (double)bound));
    return ac::check_launch("hash_stencil_input_backward");
}

AC_API size_t ac_hash_stencil_backward_scratch(const int32_t *offsets_host, uint32_t L, float S, uint32_t H, uint32_t n_copies, uint32_t B)
{
    if (!offsets_host || L == 0 || L > AC_MAX_LEVELS) return 0;
    ac::LevelTable lt; ac::make_level_table(lt, L, 3, S, H, offsets_host);
    return stencil_layout(lt, L, n_copies, B).total;
}

// the argument rules of the two functions below, for a caller that must refuse before its own first launch (ac_render_core_backward; train_common.hpp)
int hash_stencil_backward_check(uint32_t C, uint32_t L, const int32_t *offsets_host, float eps, float bound)
{
    return check("hash_stencil_backward", C, L, offsets_host, eps, bound);
}

// split_level / side_stream (ac_core_grads, data-parallel training): the accumulation runs in two launches, levels >= split_level first, and side_stream is
// ordered behind that launch (queue_scatter).  side_stream == NULL: one launch, no event.
int hash_stencil_backward_split(const float *grad, const float *x, const int32_t *offsets_host, float *grad_embeddings, uint32_t B,
                                uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, void *scratch, size_t scratch_bytes,
                                ac_stream_t stream, uint32_t split_level, ac_stream_t side_stream)
{
    // whatever happens below, a caller that passed a side stream will enqueue work on it that reads the table gradient: on every early return the side
    // stream is ordered behind what `stream` holds so far (the accumulations of earlier patches), like the normal path orders it behind the split launch
    auto leave = [&](int rc) { if (side_stream) (void)order_side_stream((hipStream_t)stream, (hipStream_t)side_stream); return rc; };
    if (int rc = hash_stencil_backward_check(C, L, offsets_host, eps, bound)) return leave(rc);
    if (B == 0) return leave(AC_OK);
    if (!grad || !x || !grad_embeddings) { ac::set_error("hash_stencil_backward: NULL buffer"); return leave(AC_ERR_BAD_ARG); }
    ac::LevelTable lt; ac::make_level_table(lt, L, 3, S, H, offsets_host);
    const float two_bound = (float)(2.0 * (double)bound);
    hipStream_t st = (hipStream_t)stream;
    uint32_t fine_mask = 0;
    for (uint32_t l = 0; l < L; ++l) {           // same rule as the fused renderer's jfine (render_fused.hip)
        const double cells = (double)eps / (double)two_bound * (double)lt.scale[l];
        if (!(cells * 1.001 + 1e-3 < 1.0)) fine_mask |= 1u << l;
    }
    // scratch: the layout for the largest copy count (<= 64) that fits; without scratch everything goes through direct atomics
    StencilScratch sc{};
    uint32_t n_copies = 1;
    if (scratch) {
        for (uint32_t k = 64; k >= 1; k >>= 1) {
            sc = stencil_layout(lt, L, k, B);
            if (sc.total <= scratch_bytes) { n_copies = k; break; }
            if (k == 1) { sc = StencilScratch{}; }
        }
    }
    float *priv = sc.n_priv ? reinterpret_cast<float *>(static_cast<char *>(scratch) + sc.priv_off) : nullptr;
    if (sc.n_priv) hipMemsetAsync(priv, 0, (size_t)sc.entries * 8 * n_copies, st);
    const uint32_t all = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
    const uint32_t direct_mask = all & ~sc.binned_mask;
    if (direct_mask)
        hipLaunchKernelGGL(hash_stencil_bwd_kernel, dim3((B + 255) / 256, L), dim3(256), 0, st, grad, x, grad_embeddings, B, lt, eps, bound, two_bound,
                           fine_mask, priv, sc.n_priv, sc.entries, n_copies, direct_mask);
    if (sc.n_binned) {
        // binned levels >= split_level have ranks n_lo .. n_binned - 1
        const uint32_t n_lo = (uint32_t)__builtin_popcount(sc.binned_mask & (split_level >= 32 ? 0xffffffffu : ((1u << split_level) - 1u)));
        const bool every_hi_binned = ((all & ~sc.binned_mask) >> (split_level >= 32 ? 31 : split_level)) == 0 && split_level < 32;
        const bool split = side_stream && every_hi_binned && n_lo > 0 && n_lo < sc.n_binned && !sc.n_priv;
        const auto fill = [&](uint32_t gx, size_t lds, uint32_t *qcount, Rec *queues) {
            hipLaunchKernelGGL(hash_stencil_bwd_binned_kernel, dim3(gx, sc.n_binned), dim3(256), lds, st, grad, x, grad_embeddings, B, lt, eps, bound,
                               two_bound, fine_mask, sc.binned_mask, qcount, queues, sc.cap, ac::verified_reciprocal(two_bound));
        };
        if (!queue_scatter(sc, scratch, lt, grad_embeddings, B, st, reinterpret_cast<const void *>(hash_stencil_bwd_binned_kernel), fill, split ? n_lo : 0u,
                           (hipStream_t)side_stream)) {
            ac::set_error("hash_stencil_backward: cannot order the side stream behind the first level group"); return AC_ERR_BAD_ARG;
        }
        if (split) side_stream = nullptr;                                // (done: the fallback below is for the cases that could not split)
    }
    if (sc.n_priv)
        hipLaunchKernelGGL(priv_reduce_kernel, dim3((sc.entries * 2 + 255) / 256), dim3(256), 0, st, priv, sc.entries * 2, n_copies, grad_embeddings);
    if (side_stream) {                          // no split happened (direct levels, no scratch): the side stream waits for everything
        if (!order_side_stream(st, (hipStream_t)side_stream)) { ac::set_error("hash_stencil_backward: cannot order the side stream"); return AC_ERR_BAD_ARG; }
    }
    return ac::check_launch("hash_stencil_backward");
}

AC_API int ac_hash_stencil_backward(const float *grad, const float *x, const int32_t *offsets_host, float *grad_embeddings, uint32_t B,
                                    uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, void *scratch, size_t scratch_bytes,
                                    ac_stream_t stream)
{
    return hash_stencil_backward_split(grad, x, offsets_host, grad_embeddings, B, C, L, S, H, eps, bound, scratch, scratch_bytes, stream, 0, nullptr);
}

#ifdef AC_PROFILE_FILL
AC_API void ac_debug_fill_prof(unsigned long long *out, int reset)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fill_prof), sizeof(unsigned long long) * AC_MAX_LEVELS * 6);
    if (reset) { static unsigned long long z[AC_MAX_LEVELS * 6] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_fill_prof), z, sizeof(z)); }
}
#endif

// ---- the reference's operator (ac_hash_encode_backward) with caller scratch: binned scatter when D = 3, C = 2 and every level fits
AC_API size_t ac_hash_encode_backward_scratch(const int32_t *offsets_host, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t B)
{
    if (!offsets_host || D != 3 || C != 2 || L == 0 || L > AC_MAX_LEVELS || B == 0) return 0;
    ac::LevelTable lt; ac::make_level_table(lt, L, 3, S, H, offsets_host);
    const uint32_t all = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
    if (binned_levels(lt, L) != all) return 0;
    return stencil_layout(lt, L, 0, B, 8u).total;
}

AC_API int ac_hash_encode_backward_ws(const float *grad, const float *inputs, const float *embeddings, const int32_t *offsets,
                                      const int32_t *offsets_host, float *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                      uint32_t H, int calc_grad_inputs, const float *dy_dx, float *grad_inputs, void *scratch, size_t scratch_bytes,
                                      ac_stream_t stream)
{
    const size_t need = ac_hash_encode_backward_scratch(offsets_host, D, C, L, S, H, B);
    if (!scratch || need == 0 || scratch_bytes < need || calc_grad_inputs)         // not coverable: the direct-atomic operator
        return ac_hash_encode_backward(grad, inputs, embeddings, offsets, offsets_host, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs, dy_dx,
                                       grad_inputs, stream);
    if (!grad || !inputs || !grad_embeddings) { ac::set_error("hash_encode_backward: NULL buffer"); return AC_ERR_BAD_ARG; }
    ac::LevelTable lt; ac::make_level_table(lt, L, 3, S, H, offsets_host);
    const StencilScratch sc = stencil_layout(lt, L, 0, B, 8u);
    hipStream_t st = (hipStream_t)stream;
    queue_scatter(sc, scratch, lt, grad_embeddings, B, st, reinterpret_cast<const void *>(hash_bwd_binned_kernel),
                  [&](uint32_t gx, size_t lds, uint32_t *qcount, Rec *queues) {
                      hipLaunchKernelGGL(hash_bwd_binned_kernel, dim3(gx, sc.n_binned), dim3(256), lds, st, grad, inputs, grad_embeddings, B, lt, sc.binned_mask,
                                         qcount, queues, sc.cap);
                  });
    return ac::check_launch("hash_encode_backward");
}
