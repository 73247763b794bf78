// avatarcraft_amd/csrc/warp_accel_build.hip -- builds the culling structure of the closest-face search (format and shared pieces: warp_accel.hpp) for gfx950.
// Per frame, five kernels on the caller's stream (ac_warp_accel_build): the vertex bounding box and the grid parameters, the Morton keys of the faces,
// their ranks (the face order), the tiles with their bounds, and the candidate lists of the cells of both grids.
#include "warp_accel.hpp"

namespace {

// grid parameters of both levels from the vertex bounding box (one workgroup)
__global__ __launch_bounds__(1024) void accel_grid_setup_kernel(const float *__restrict__ verts, uint32_t V, AccelView av)
{
    __shared__ float red[6][1024];
    const uint32_t t = threadIdx.x;
    float lo[3] = { __builtin_inff(), __builtin_inff(), __builtin_inff() }, hi[3] = { -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
    for (uint32_t v = t; v < V; v += 1024)
#pragma unroll
        for (int k = 0; k < 3; ++k) { const float c = verts[3 * (size_t)v + k]; lo[k] = c < lo[k] ? c : lo[k]; hi[k] = c > hi[k] ? c : hi[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { red[k][t] = lo[k]; red[3 + k][t] = hi[k]; }
    __syncthreads();
    for (uint32_t s = 512; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                red[k][t] = red[k][t + s] < red[k][t] ? red[k][t + s] : red[k][t];
                red[3 + k][t] = red[3 + k][t + s] > red[3 + k][t] ? red[3 + k][t + s] : red[3 + k][t];
            }
        }
        __syncthreads();
    }
    if (t < 6) av.hdr[HDR_BBOX + t] = __builtin_bit_cast(uint32_t, red[t][0]);
    for (uint32_t e = t; e < (uint32_t)WORK_SLOTS * 4u; e += 1024) av.work[e] = 0ull;      // work counters of the searches on this structure
    if (t < (uint32_t)GRID_LEVELS) {
        const int l = (int)t;
        const float margin = l == 0 ? GRID_MARGIN0 : GRID_MARGIN1;
        const uint32_t cap = LVL_CELLS[l];
        float org[3], ext[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            org[k] = red[k][0] - margin; ext[k] = (red[3 + k][0] - red[k][0]) + 2.0f * margin;
            ok = ok && ext[k] > 0.0f && ext[k] < 1e6f;           // NaN / inf vertices: no grid, every sample takes the full bounding pass
        }
        uint32_t n[3] = { 0, 0, 0 };
        float cs = 1.0f;
        if (ok) {
            cs = cbrtf(ext[0] * ext[1] * ext[2] / (float)cap);
            cs = cs > 0.005f ? cs : 0.005f;                        // cells below 5 mm buy nothing (faces are ~1 cm)
            for (int trial = 0; trial < 64; ++trial) {
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = (uint32_t)(ext[k] / cs) + 1u;
                if ((unsigned long long)n[0] * n[1] * n[2] <= cap) break;
                cs *= 1.02f;
            }
            if ((unsigned long long)n[0] * n[1] * n[2] > cap) { n[0] = n[1] = n[2] = 0; }
        }
        uint32_t *h = av.hdr + HDR_LVL + HDR_LVL_STRIDE * l;
#pragma unroll
        for (int k = 0; k < 3; ++k) { h[k] = __builtin_bit_cast(uint32_t, org[k]); h[5 + k] = n[k]; }
        h[3] = __builtin_bit_cast(uint32_t, 1.0f / cs);
        // |q - centre| <= h for every q that the search maps to the cell: half diagonal, plus the rounding of the index computation
        // ((q - org) * inv: relative 2^-23 of a value < 2^10 cells) and of the centre itself
        const float hd = 0.8660254f * cs * (1.0f + 1e-3f) + 1e-6f;
        h[4] = __builtin_bit_cast(uint32_t, 2.0f * hd);
        h[8] = n[0] * n[1] * n[2];
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v)      // 10 bits -> every third bit
{
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu; v = (v | (v << 8)) & 0x0300f00fu; v = (v | (v << 4)) & 0x030c30c3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// Face order along a Morton curve.  Keys ((30-bit code of the centroid, quantised in the vertex bounding box that accel_grid_setup_kernel left in
// the header) << 32 | face id) are unique, so the position of a face is the number of smaller keys: accel_keys_kernel writes the keys, the
// (face block, key slice) grid of accel_rank_kernel counts, and the last slice of a face block to finish writes its part of the order.
constexpr uint32_t SORT_SLICE = 1024;          // keys per slice (staged in LDS)

__global__ __launch_bounds__(256) void accel_keys_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t F, AccelView av)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    const SortScratch ss = sort_scratch(av);
    if (threadIdx.x == 0) ss.done[blockIdx.x] = 0;
    if (f >= MAX_ACCEL_FACES) return;
    ss.rank[f] = 0;
    if (f >= F) return;
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = __builtin_bit_cast(float, av.hdr[HDR_BBOX + k]), ext = __builtin_bit_cast(float, av.hdr[HDR_BBOX + 3 + k]) - lo;
        const float inv = ext > 0.0f ? 1023.0f / (3.0f * ext) : 0.0f;
        const float c = (verts[3 * (size_t)faces[3 * f] + k] + verts[3 * (size_t)faces[3 * f + 1] + k]) + verts[3 * (size_t)faces[3 * f + 2] + k];
        float g = (c - 3.0f * lo) * inv;
        g = g < 0.0f ? 0.0f : (g > 1023.0f ? 1023.0f : g);
        q[k] = (uint32_t)g;
    }
    const uint32_t m = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
    ss.keys[f] = ((unsigned long long)m << 32) | f;
}

__global__ __launch_bounds__(256) void accel_rank_kernel(uint32_t F, AccelView av)
{
    __shared__ __attribute__((aligned(16))) unsigned long long sk[SORT_SLICE];
    __shared__ uint32_t last;
    const SortScratch ss = sort_scratch(av);
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    const uint32_t k0 = blockIdx.y * SORT_SLICE;
    for (uint32_t i = threadIdx.x; i < SORT_SLICE; i += 256) sk[i] = k0 + i < F ? ss.keys[k0 + i] : ~0ull;      // (no key is below a padding key)
    __syncthreads();
    if (f < F) {
        const unsigned long long mine = ss.keys[f];
        const ulonglong2 *sk2 = reinterpret_cast<const ulonglong2 *>(sk);
        uint32_t cnt = 0;
#pragma unroll 16
        for (uint32_t i = 0; i < SORT_SLICE / 2; ++i) { const ulonglong2 v = sk2[i]; cnt += (v.x < mine ? 1u : 0u) + (v.y < mine ? 1u : 0u); }
        if (cnt) atomicAdd(&ss.rank[f], cnt);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(&ss.done[blockIdx.x], 1u) == gridDim.y - 1 ? 1u : 0u;
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (f < F) av.sorted[__hip_atomic_load(&ss.rank[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = f;
    // the slots behind the last face (the tile builder repeats the last face there and never reads them)
    for (uint32_t p = F + f; p < MAX_ACCEL_FACES; p += gridDim.x * 256) av.sorted[p] = 0xffffffffu;
}

// the tiles: TILE_F consecutive faces of the sorted order each -- the faces' corners and bounding discs per slot, the oriented box, the sub-boxes and the
// representative vertex per tile.  One lane per slot; the first TPB lanes of a block then bound the block's tiles.
constexpr int TPB = 256 / TILE_F;   // tiles per block
__global__ __launch_bounds__(256) void accel_tiles_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t F,
                                                          AccelView av)
{
    __shared__ float sb[256][9];
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    const uint32_t nt = (F + TILE_F - 1) / TILE_F;
    const uint32_t src = slot < F ? slot : F - 1;                     // the tail of the last tile repeats the last face
    const uint32_t f = av.sorted[src];
    float v[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[3 * c + k] = verts[3 * (size_t)faces[3 * f + c] + k];
    if (slot < nt * TILE_F) {
#pragma unroll
        for (int e = 0; e < 9; ++e) av.tri[(size_t)slot * 9 + e] = v[e];
        av.oid[slot] = (int32_t)f;
        // bounding disc: the face lies in the disc (centre c = centroid, radius r = largest vertex distance from the STORED c) of its
        // own plane, so dist(q, face)^2 >= pd^2 + max(0, rho - r)^2 with pd = n.(q - c) and rho^2 = |q - c|^2 - pd^2.  Built in fp64
        // from the fp32 vertices and rounded to fp32; the search pads for that rounding.  A (nearly) degenerate face gets n = 0:
        // the bound then falls back to the bounding sphere.
        const double A[3] = { (double)v[0], (double)v[1], (double)v[2] }, Bv[3] = { (double)v[3], (double)v[4], (double)v[5] },
                     Cv[3] = { (double)v[6], (double)v[7], (double)v[8] };
        float cf[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cf[k] = (float)((A[k] + Bv[k] + Cv[k]) / 3.0);
        double r2 = 0.0;
#pragma unroll
        for (int cnr = 0; cnr < 3; ++cnr) {
            const double ex = (double)v[3 * cnr] - (double)cf[0], ey = (double)v[3 * cnr + 1] - (double)cf[1], ez = (double)v[3 * cnr + 2] - (double)cf[2];
            const double d = ex * ex + ey * ey + ez * ez;
            r2 = d > r2 ? d : r2;
        }
        const double e0[3] = { Bv[0] - A[0], Bv[1] - A[1], Bv[2] - A[2] }, e1[3] = { Cv[0] - A[0], Cv[1] - A[1], Cv[2] - A[2] };
        const double nx = e0[1] * e1[2] - e0[2] * e1[1], ny = e0[2] * e1[0] - e0[0] * e1[2], nz = e0[0] * e1[1] - e0[1] * e1[0];
        const double nl = __builtin_sqrt(nx * nx + ny * ny + nz * nz);
        const double l0 = __builtin_sqrt(AC_DOT3(e0, e0)), l1 = __builtin_sqrt(AC_DOT3(e1, e1));
        const bool flat = nl > 1e-6 * l0 * l1 && nl > 0.0;           // sin(angle at A) > 1e-6: the normal of a sliver is not trustworthy
        av.sph[2 * (size_t)slot] = make_float4(cf[0], cf[1], cf[2], (float)(__builtin_sqrt(r2) * (1.0 + 1e-6) + 1e-7));
        av.sph[2 * (size_t)slot + 1] = flat ? make_float4((float)(nx / nl), (float)(ny / nl), (float)(nz / nl), 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) sb[threadIdx.x][e] = v[e];
    __syncthreads();
    if (threadIdx.x < TPB) {
        const uint32_t tile = blockIdx.x * TPB + threadIdx.x;
        if (tile < MAX_TILES) {
            // oriented box of the tile: axis 0 = area-weighted mean normal of its faces, axes 1, 2 = a tangent basis; a surface patch
            // is thin along its normal, so this box is tight where an axis-aligned one is loose (by the patch size) -- and the
            // looseness of the lower bound is what decides how many tiles a sample has to test
            float ax[3][3] = { { 1.0f, 0.0f, 0.0f }, { 0.0f, 1.0f, 0.0f }, { 0.0f, 0.0f, 1.0f } };
            float lo[3] = { __builtin_inff(), __builtin_inff(), __builtin_inff() }, hi[3] = { -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
            float rep[3] = { __builtin_inff(), __builtin_inff(), __builtin_inff() };
            if (tile < nt) {
                float nrm[3] = { 0.0f, 0.0f, 0.0f };
                for (int j = 0; j < TILE_F; ++j) {
                    const float *t = sb[threadIdx.x * TILE_F + j];
                    const float e0[3] = { t[3] - t[0], t[4] - t[1], t[5] - t[2] }, e1[3] = { t[6] - t[0], t[7] - t[1], t[8] - t[2] };
                    nrm[0] += e0[1] * e1[2] - e0[2] * e1[1]; nrm[1] += e0[2] * e1[0] - e0[0] * e1[2]; nrm[2] += e0[0] * e1[1] - e0[1] * e1[0];
                }
                const float len = __builtin_sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
                if (len > 0.0f) {
                    const float n0 = nrm[0] / len, n1 = nrm[1] / len, n2 = nrm[2] / len;
                    // tangent: the coordinate axis least aligned with n, made orthogonal to it
                    const float a0 = __builtin_fabsf(n0), a1 = __builtin_fabsf(n1), a2 = __builtin_fabsf(n2);
                    float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
                    if (a0 <= a1 && a0 <= a2) h0 = 1.0f; else if (a1 <= a2) h1 = 1.0f; else h2 = 1.0f;
                    const float dp = h0 * n0 + h1 * n1 + h2 * n2;
                    float t0 = h0 - dp * n0, t1 = h1 - dp * n1, t2 = h2 - dp * n2;
                    const float tl = __builtin_sqrtf(t0 * t0 + t1 * t1 + t2 * t2);
                    t0 /= tl; t1 /= tl; t2 /= tl;
                    ax[0][0] = n0; ax[0][1] = n1; ax[0][2] = n2;
                    ax[1][0] = t0; ax[1][1] = t1; ax[1][2] = t2;
                    ax[2][0] = n1 * t2 - n2 * t1; ax[2][1] = n2 * t0 - n0 * t2; ax[2][2] = n0 * t1 - n1 * t0;
                }
                for (int gI = 0; gI < SUBS; ++gI) {                   // per group of SUB_F consecutive faces (compact along the curve): its own box in the tile's frame
                    float slo[3] = { __builtin_inff(), __builtin_inff(), __builtin_inff() }, shi[3] = { -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
                    for (int j = gI * SUB_F; j < (gI + 1) * SUB_F; ++j)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float *t = sb[threadIdx.x * TILE_F + j] + 3 * c;
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                const float d = ax[k][0] * t[0] + ax[k][1] * t[1] + ax[k][2] * t[2];
                                slo[k] = d < slo[k] ? d : slo[k]; shi[k] = d > shi[k] ? d : shi[k];
                            }
                        }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        lo[k] = slo[k] < lo[k] ? slo[k] : lo[k]; hi[k] = shi[k] > hi[k] ? shi[k] : hi[k];
                        const float pad = 1e-5f * (1.0f + __builtin_fabsf(slo[k]) + __builtin_fabsf(shi[k]));      // as for the tile's box below
                        av.sub[((size_t)tile * SUBS + gI) * 6 + k] = slo[k] - pad; av.sub[((size_t)tile * SUBS + gI) * 6 + 3 + k] = shi[k] + pad;
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {                        // fp32 dot products and axes: stay conservative
                    const float pad = 1e-5f * (1.0f + __builtin_fabsf(lo[k]) + __builtin_fabsf(hi[k]));
                    lo[k] -= pad; hi[k] += pad;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) rep[k] = sb[threadIdx.x * TILE_F][k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) av.box[(3 * k + c) * MAX_TILES + tile] = ax[k][c];
                av.box[(9 + k) * MAX_TILES + tile] = lo[k]; av.box[(12 + k) * MAX_TILES + tile] = hi[k]; av.box[(15 + k) * MAX_TILES + tile] = rep[k];
            }
        }
    }
    if (slot == 0) { av.hdr[0] = nt; av.hdr[1] = F; }
}

constexpr int LIST_CLASSES = 3;     // a cell's tile list is written in this many distance classes, nearest first

// one wave per cell (strided): the full bounding pass + seed test at the cell centre c, then the list of tiles t with
//   sqrt(lb_t(c)) <= sqrt(d2(c, seed face)) + 2 h:   for q in the cell, boxdist(q, t) >= boxdist(c, t) - h and dist(q, mesh) <= dist(c, seed face) + h,
// so a tile outside the list cannot hold the closest face (nor one at equal distance) of any q of the cell.
__global__ __launch_bounds__(256) void accel_cells_kernel(AccelView av)
{
    const int lane = threadIdx.x & 63;
    const uint32_t nt = av.hdr[0];
    const uint32_t nit = (nt + 63) >> 6;
    extern __shared__ __attribute__((aligned(16))) float sbox_raw[];
    const uint32_t ntp = nit * 64;
    load_boxes<BoxLayout::RowMajor>(sbox_raw, av, ntp);
    __syncthreads();
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
#pragma unroll 1
    for (int l = 0; l < GRID_LEVELS; ++l) {
        const GridParams g = grid_params(av, l);
        const float cs = 1.0f / g.inv;
        const uint32_t K = LVL_K[l];
        for (uint32_t cell = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); cell < g.cells; cell += nwaves) {
            const uint32_t ix = cell % g.n[0], iy = (cell / g.n[0]) % g.n[1], iz = cell / (g.n[0] * g.n[1]);
            const float qf[3] = { g.org[0] + ((float)ix + 0.5f) * cs, g.org[1] + ((float)iy + 0.5f) * cs, g.org[2] + ((float)iz + 0.5f) * cs };
            const double q[3] = { (double)qf[0], (double)qf[1], (double)qf[2] };
            float lb[NIT];
            int tA, tB;
            bounding_pass<BoxLayout::RowMajor>(sbox_raw, ntp, nit, lane, qf, lb, tA, tB);
            {   // every face lies in its tile's box: dist(q, mesh) >= min_t boxdist(c, t) - h for all q of the cell
                float mn = lb[0];
#pragma unroll
                for (int it = 1; it < NIT; ++it) mn = lb[it] < mn ? lb[it] : mn;
                mn = wave_min_f32(mn);
                const float dl = __builtin_sqrtf(mn) * (1.0f - 1e-6f) - 0.5f * g.h2;
                const float cfar_cell = dl > 0.0f ? dl * dl * (1.0f - 1e-6f) : 0.0f;
                if (lane == 0) av.cfar[LVL_CELL0[l] + cell] = cfar_cell;
            }
            double best = __builtin_inf(), bc[3] = { 0.0, 0.0, 0.0 };
            int bid = 0x7fffffff;
            uint32_t myslot;
            seed_test(av, q, tA, tB, lane, best, bid, bc, myslot);
            const double seed = wave_min_f64(best);
            uint32_t info = CELL_OVERFLOW << 16;
            if (seed < 1e30) {                                           // false for inf / NaN: a cell next to nothing but degenerate faces
                const uint32_t sslot = (uint32_t)__builtin_amdgcn_readlane((int)myslot, __builtin_ctzll(__ballot(best == seed)));
                const float su = __builtin_sqrtf((float)seed * (1.0f + 1e-6f)) * (1.0f + 1e-6f) + g.h2 * (1.0f + 1e-6f);      // >= sqrt(seed) + 2 h
                uint32_t cnt = 0;
                unsigned long long cand[NIT];
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    cand[it] = 0;
                    if ((uint32_t)it >= nit) continue;
                    cand[it] = __ballot(__builtin_sqrtf(lb[it]) * (1.0f - 1e-6f) <= su);      // <= sqrt(lb): a superset
                    cnt += (uint32_t)__builtin_popcountll(cand[it]);
                }
                if (cnt <= K) {
                    uint16_t *dst = av.ctl + LVL_CTL0[l] + (size_t)cell * K;
                    uint32_t at = 0;
                    // Listed NEAR TILES FIRST: the search walks a list front to back against a bound that falls with every exact test, so the
                    // tiles most likely to hold the closest face should come before the ones that are only in the list because of the 2 h band.
                    // Three classes by the box distance from the cell centre: <= half, <= the whole, > the distance of the seed face.
                    const float seedf = (float)seed;
#pragma unroll 1
                    for (int cls = 0; cls < LIST_CLASSES; ++cls) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            if ((uint32_t)it >= nit) continue;
                            const int mycls = lb[it] <= 0.25f * seedf ? 0 : (lb[it] <= seedf ? 1 : 2);
                            const unsigned long long m = cand[it] & __ballot(mycls == cls);
                            if ((m >> lane) & 1ull) {
                                const uint32_t at_l = at + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                                dst[at_l] = (uint16_t)(it * 64 + lane);
                            }
                            at += (uint32_t)__builtin_popcountll(m);
                        }
                    }
                    info = (cnt << 16) | sslot;
                }
            }
            if (lane == 0) av.cell[LVL_CELL0[l] + cell] = info;
        }
    }
}

}  // namespace

AC_API int ac_warp_accel_work(const void *accel, unsigned long long out[4], ac_stream_t stream)
{
    if (!accel || !out) { ac::set_error("warp_accel_work: NULL argument"); return AC_ERR_BAD_ARG; }
    const AccelView av = accel_view(const_cast<void *>(accel));
    static unsigned long long host[WORK_SLOTS * 4];
    if (hipMemcpyAsync(host, av.work, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { ac::set_error("warp_accel_work: copy failed"); return AC_ERR_LAUNCH; }
    for (int k = 0; k < 4; ++k) { out[k] = 0; for (int sl = 0; sl < WORK_SLOTS; ++sl) out[k] += host[4 * sl + k]; }
    return AC_OK;
}

AC_API size_t ac_warp_accel_bytes(uint32_t F)
{
    if (F == 0 || F > MAX_ACCEL_FACES) return 0;
    size_t o[ACCEL_SEGS];
    return accel_offsets(o);
}

AC_API int ac_warp_accel_build(const float *verts, const int32_t *faces, uint32_t V, uint32_t F, void *accel, size_t accel_bytes,
                               ac_stream_t stream)
{
    const size_t need = ac_warp_accel_bytes(F);
    if (need == 0) { ac::set_error("warp_accel_build: %u faces not supported (1..%u); use ac_warp_samples", F, MAX_ACCEL_FACES); return AC_ERR_BAD_ARG; }
    if (!verts || !faces || !accel || accel_bytes < need) { ac::set_error("warp_accel_build: NULL buffer or accel buffer smaller than %zu bytes", need); return AC_ERR_BAD_ARG; }
    const AccelView av = accel_view(accel);
    // grid parameters and the vertex bounding box (one workgroup), the Morton order of the faces (keys, then ranks), the tiles, then one wave per
    // cell (strided over a grid that fills the device)
    hipLaunchKernelGGL(accel_grid_setup_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, verts, V, av);
    hipLaunchKernelGGL(accel_keys_kernel, dim3(MAX_ACCEL_FACES / 256), dim3(256), 0, (hipStream_t)stream, verts, faces, F, av);
    hipLaunchKernelGGL(accel_rank_kernel, dim3((F + 255) / 256, (F + SORT_SLICE - 1) / SORT_SLICE), dim3(256), 0, (hipStream_t)stream, F, av);
    hipLaunchKernelGGL(accel_tiles_kernel, dim3(MAX_TILES / TPB), dim3(256), 0, (hipStream_t)stream, verts, faces, F, av);
    const size_t ntp = (((size_t)F + TILE_F - 1) / TILE_F + 63) / 64 * 64;
    const size_t lds_c = (size_t)NB * ntp * sizeof(float);
    static uint64_t seen_c = 0;
    ac::allow_dynamic_lds(seen_c, reinterpret_cast<const void *>(accel_cells_kernel), (size_t)NB * MAX_TILES * sizeof(float));
    hipLaunchKernelGGL(accel_cells_kernel, dim3(4 * (unsigned)ac::cu_count()), dim3(256), lds_c, (hipStream_t)stream, av);
    return ac::check_launch("warp_accel_build");
}
