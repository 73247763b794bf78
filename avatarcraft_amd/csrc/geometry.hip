// avatarcraft_amd/csrc/geometry.hip -- the two consumers of the learned SDF outside the ray path:
//
//   mesh export   NeRFNetwork.extract_geometry (models/instant_nsr.py:706-764; the reference's one call: stylize.py:267, resolution 512):
//                 forward_sdf on a resolution^3 grid over [-bound, bound]^3 (extract_fields :728-745, 256^3-point blocks through query_func, assembled
//                 on the HOST) -> u = -sdf -> PyMCubes marching_cubes(u, threshold) -> vertices scaled to world units.
//                 Here: ac_field_sdf_grid (grid coordinates formed in the kernel from the three axis tables, the volume stays on the device) and
//                 ac_marching_cubes_count / _emit (classify -> scan -> emit, shared-edge vertex indexing, no atomics: a deterministic mesh).
//   mesh attributes  nothing in the reference: utils.save_mesh(vert, face, ...) (stylize.py:263-269) writes geometry only.  Here: ac_mesh_vertex_attrs -- every
//                 vertex of the marching-cubes buffer through a few Newton steps along the finite-difference gradient onto the level set, then the normal and
//                 the colour network at the final position (mesh_attrs_kernel: the seven-point stencil of field_tile.hpp on tiles of 16 vertices).
//   density grid  NeRFRenderer.update_extra_state (:303-356): forward_sdf on the 129^3 grid -> logistic density -> zero pad + 2^3 max pool ->
//                 maximum(grid * decay, new) -> mean.  Here two launches (ac_density_grid_update): the density of every grid point on the x-tiles of
//                 ac_field_sdf_grid into a scratch volume, then one streaming pass that pools, merges into the running grid in place and forms the mean.
//
// The SDF itself is the renderer's own tile code (nsr_device.hpp: sdf_tile = hash gather + MFMA SDF network), so every value is bit-identical to
// ac_field_sdf / density() and therefore to the CPU oracle's orc_field_sdf.
//
// Marching cubes: the 256-case table is GENERATED from the algorithm's definition (tools/gen_mc_table.py -> ac_mc_table.hpp): corner flagged <=> u <= iso
// (PyMCubes' convention), one vertex per sign-changing grid edge at the linear zero crossing (formed in double like PyMCubes: it evaluates its float32
// input in double), ambiguous faces always cut off the flagged corners (a rule of the face's own 4 flags: watertight by construction), triangles oriented
// with the normal towards u <= iso = out of the body for u = -sdf.  PyMCubes is not in this image: "unpinned vs PyMCubes, pinned vs the definition".
// Order of the output (what makes the mesh reproducible bit for bit, and equal to the CPU oracle's serial loop): vertices by owning grid point (linear
// index, z fastest) then by axis x, y, z; triangles by cell (linear index) then by table position.
#include "field_tile.hpp"
#include "mesh_blend.hpp"

#define AC_MC_CONST static __constant__ const
#include "ac_mc_table.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------- SDF on a regular grid
// update_extra_state's density (:331-337): inv_s e^(-inv_s sdf) / (1 + e^(-inv_s sdf)) for sdf > 0, the mirrored form for sdf <= 0 -- the two
// overflow-free branches, every operation in the reference's order (mul, exp, mul | add, div) in fp32
__device__ __forceinline__ float dg_density(float sdf, float inv_s)
{
    const float e = expf(sdf > 0.0f ? -inv_s * sdf : inv_s * sdf);
    return (inv_s * e) / (1.0f + e);
}

constexpr uint32_t GB_X = 16, GB_Y = 4, GB_Z = 16;           // a brick of grid points: 64 tiles of 16 points along X

// The volume is cut into bricks of 16 x 4 x 16 points; a workgroup evaluates one brick at a time, its 8 waves take 8 tiles each, and a
//   tile is 16 consecutive points ALONG X.  Why x: the spatial hash of the fine levels is x ^ y P1 ^ z P2 (hashencoder.cu:54-70) -- linear in x, so the eight cells
//   x in [8k, 8k + 8) of one (y, z) row are the eight entries of ONE 64-byte sector of the table (and consecutive entries on the dense levels).  A gather
//   instruction serves one corner of the 16 points of a tile: along x those 16 entries sit in 2 .. 9 sectors, along y or z in 16 (the primes scatter them
//   over the level's 4 MB).  The per-CU gather path and the fabric behind L2 -- what this kernel is short of -- see a fraction of the requests.
//   The results are staged in LDS and written with z fastest (64-byte runs) -- the volume keeps the reference's [x][y][z] layout.
//   Every XCD (workgroup index mod 8) walks through its own contiguous eighth of the bricks: coarse and middle levels are re-used from its L2.
__global__ __launch_bounds__(BLOCK) void field_sdf_grid_kernel(const RenderArgs a, const float *__restrict__ ax, const float *__restrict__ ay,
                                                               const float *__restrict__ az, uint32_t nx, uint32_t ny, uint32_t nz, int mode, float inv_s,
                                                               float *__restrict__ vol)
{
    // mode: what is stored per grid point -- 0 the sdf, 1 its negative (the mesh export's u), 2 update_extra_state's logistic density of it (dg_density)
    auto value = [&](float sdf) { return mode == 2 ? dg_density(sdf, inv_s) : (mode == 1 ? -sdf : sdf); };
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const FieldCtx fc = make_ctx(a);
    float *stage = lds + OFF_WAVE;                                                               // [GB_X][GB_Y][GB_Z]
    const uint32_t nbz = (nz + GB_Z - 1) / GB_Z, nby = (ny + GB_Y - 1) / GB_Y, nbx = (nx + GB_X - 1) / GB_X;
    const uint32_t nbricks = nbx * nby * nbz, per_xcd = (nbricks + 7u) / 8u;
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;        // (the grid is a multiple of 8 workgroups)
    for (uint32_t bi = slot; bi < per_xcd; bi += slots) {
        const uint32_t brick = xcd * per_xcd + bi;
        if (brick >= nbricks) break;                                                             // (workgroup-uniform)
        const uint32_t bz = brick % nbz, bt = brick / nbz, by = bt % nby, bx = bt / nby;
#pragma unroll 1
        for (uint32_t t = (uint32_t)wave; t < GB_Y * GB_Z; t += WAVES_PER_BLOCK) {
            const uint32_t ly = t >> 4, lz = t & 15u;
            const uint32_t ix = bx * GB_X + (uint32_t)n, iy = by * GB_Y + ly, iz = bz * GB_Z + lz;
            if (iy >= ny || iz >= nz) continue;                                                  // (wave-uniform)
            const uint32_t cx = ix < nx ? ix : nx - 1u;
            const f32x4 o = sdf_tile(lds, fc, lane, ax[cx], ay[iy], az[iz]);
            if (g == 0) stage[((uint32_t)n * GB_Y + ly) * GB_Z + lz] = value(o[0]);
        }
        __syncthreads();
        for (uint32_t o = threadIdx.x; o < GB_X * GB_Y * GB_Z; o += BLOCK) {
            const uint32_t lz = o & 15u, ly = (o >> 4) & 3u, lx = o >> 6;
            const uint32_t ix = bx * GB_X + lx, iy = by * GB_Y + ly, iz = bz * GB_Z + lz;
            if (ix < nx && iy < ny && iz < nz) vol[((size_t)ix * ny + iy) * nz + iz] = stage[o];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- marching cubes
constexpr int MC_PTS = 1024;                     // grid points per workgroup (256 threads x 4 consecutive points: their four count bytes are one dword)
struct McDims { uint32_t nx, ny, nz, npts; };

__device__ __forceinline__ bool mc_flag(float u, float iso) { return u <= iso; }

// The corner flags of the whole volume as a bit array (1 bit per grid point: 16.8 MB at 512^3, L2-resident), written by ONE coalesced pass over the
// volume: a wave takes 64 consecutive points per step, the ballot of `u <= iso` is their 64 flags.  The classification then reads bits: its eight
// look-ups per point (four rows of the volume) were 2.1 GB of L2 traffic on floats (0.95 ms at 512^3), on bits they are nothing.
__global__ __launch_bounds__(256) void mc_flags_kernel(const float *__restrict__ vol, uint32_t npts, float iso, unsigned long long *__restrict__ bits64)
{
    const uint32_t lane = threadIdx.x & 63u, nchunks = (npts + 1023u) >> 10;            // a wave's unit of work: 1024 points = 16 steps
    for (uint32_t chunk = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; chunk < nchunks; chunk += (gridDim.x * blockDim.x) >> 6) {
        const uint32_t base = chunk << 10;
        unsigned long long mine = 0ull;
#pragma unroll
        for (uint32_t it = 0; it < 16; ++it) {
            const uint32_t p = base + it * 64u + lane;
            const unsigned long long m = __ballot(p < npts && mc_flag(vol[p < npts ? p : npts - 1u], iso));
            if (lane == it) mine = m;
        }
        if (lane < 16u && base + lane * 64u < npts) bits64[(base >> 6) + lane] = mine;     // 16 consecutive 8-byte words
    }
}
__device__ __forceinline__ bool mc_bit(const uint32_t *__restrict__ bits, uint32_t q) { return (bits[q >> 5] >> (q & 31u)) & 1u; }

// count byte of a grid point: bits 0-2 = which of its three OWNED edges (towards +x, +y, +z) change sign; bits 3-5 = triangles of the cell it is the origin of
__device__ __forceinline__ uint32_t mc_classify(const uint32_t *__restrict__ bits, const McDims d, uint32_t p, uint32_t *case_out = nullptr)
{
    const uint32_t k = p % d.nz, t = p / d.nz, j = t % d.ny, i = t / d.ny;
    const bool hx = i + 1u < d.nx, hy = j + 1u < d.ny, hz = k + 1u < d.nz;
    const uint32_t sx = d.ny * d.nz, sy = d.nz;
    const bool f0 = mc_bit(bits, p);
    uint32_t vmask = 0, cs = f0 ? 1u : 0u;
    bool f1 = false, f2 = false, f4 = false;
    if (hx) { f1 = mc_bit(bits, p + sx); vmask |= (f1 != f0) ? 1u : 0u; }
    if (hy) { f2 = mc_bit(bits, p + sy); vmask |= (f2 != f0) ? 2u : 0u; }
    if (hz) { f4 = mc_bit(bits, p + 1u); vmask |= (f4 != f0) ? 4u : 0u; }
    uint32_t nt = 0;
    if (hx && hy && hz) {
        cs |= (f1 ? 2u : 0u) | (f2 ? 4u : 0u) | (f4 ? 16u : 0u);
        cs |= mc_bit(bits, p + sx + sy) ? 8u : 0u;
        cs |= mc_bit(bits, p + sx + 1u) ? 32u : 0u;
        cs |= mc_bit(bits, p + sy + 1u) ? 64u : 0u;
        cs |= mc_bit(bits, p + sx + sy + 1u) ? 128u : 0u;
        nt = AC_MC_NTRI[cs];
    } else cs = 0u;
    if (case_out) *case_out = cs;
    return vmask | (nt << 3);
}

// workgroup-wide exclusive scan of one value per thread (256 threads), in thread order; total -> every thread
__device__ __forceinline__ uint32_t block_exscan_256(uint32_t v, uint32_t *sh /* [8] */, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += o; }
    __syncthreads();                              // (sh may still be read by a previous call)
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (w < wave) base += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + inc - v;
}

__global__ __launch_bounds__(256) void mc_classify_kernel(const uint32_t *__restrict__ bits, const McDims d, uint32_t *__restrict__ cnt4,
                                                          uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sh[8];
    const uint32_t p0 = blockIdx.x * MC_PTS + threadIdx.x * 4u;
    uint32_t packed = 0, nv = 0, nt = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t p = p0 + r;
        uint32_t c = 0;
        if (p < d.npts) c = mc_classify(bits, d, p);
        packed |= c << (8 * r);
        nv += (uint32_t)__builtin_popcount(c & 7u); nt += c >> 3;
    }
    if (p0 < d.npts) cnt4[p0 >> 2] = packed;      // (the count array is padded to a multiple of 4 points)
    uint32_t tot;
    (void)block_exscan_256(nv | (nt << 16), sh, tot);      // 1024 points: at most 3072 vertices / 5120 triangles per workgroup -- 16 bits each
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// exclusive scan of the per-workgroup totals (vertices in the low, triangles in the high 16 bits) -> boff[2 * b], boff[2 * b + 1]; totals -> counts[0..1].
// One workgroup of 16 waves; a wave owns a contiguous range of the totals and walks it 64 at a time (coalesced loads, shuffle scan, running carry);
// the waves' totals are combined through LDS and added in a second coalesced pass (131 072 totals at 512^3: 128 steps per wave and pass).
__device__ __forceinline__ uint32_t wave_incscan(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)v, d); if (lane >= d) v += o; }
    return v;
}
__global__ __launch_bounds__(1024) void mc_scan_kernel(const uint32_t *__restrict__ bsum, uint32_t nblk, uint32_t *__restrict__ boff, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wv[16], wt[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t per = (((nblk + 15u) / 16u) + 63u) & ~63u, lo = (uint32_t)wave * per, hi = lo + per < nblk ? lo + per : nblk;
    uint32_t cv = 0, ct = 0;
    for (uint32_t b0 = lo; b0 < hi; b0 += 64u) {
        const uint32_t b = b0 + (uint32_t)lane;
        const uint32_t sv = b < hi ? bsum[b] : 0u;
        const uint32_t v = sv & 0xffffu, t = sv >> 16;
        const uint32_t iv = wave_incscan(v, lane), it = wave_incscan(t, lane);
        if (b < hi) { boff[2 * b] = cv + iv - v; boff[2 * b + 1] = ct + it - t; }
        cv += (uint32_t)__shfl((int)iv, 63); ct += (uint32_t)__shfl((int)it, 63);
    }
    if (lane == 0) { wv[wave] = cv; wt[wave] = ct; }
    __syncthreads();
    uint32_t bv = 0, bt = 0;
    for (int w = 0; w < wave; ++w) { bv += wv[w]; bt += wt[w]; }
    if (bv | bt)
        for (uint32_t b = lo + (uint32_t)lane; b < hi; b += 64u) { boff[2 * b] += bv; boff[2 * b + 1] += bt; }
    if (threadIdx.x == 1023) { counts[0] = bv + cv; counts[1] = bt + ct; }
}

struct McXform { double den, span[3], lo[3]; };   // world = index / den * span + lo, the reference's three operations in its order (instant_nsr.py:760-762)

__global__ __launch_bounds__(256) void mc_vertices_kernel(const float *__restrict__ vol, const McDims d, float iso, const uint32_t *__restrict__ cnt4,
                                                          const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, uint32_t *__restrict__ voff,
                                                          const McXform xf, double *__restrict__ verts, uint32_t n_verts)
{
    __shared__ uint32_t sh[8];
    if ((bsum[blockIdx.x] & 0xffffu) == 0u) return;
    const uint32_t p0 = blockIdx.x * MC_PTS + threadIdx.x * 4u;
    const uint32_t packed = p0 < d.npts ? cnt4[p0 >> 2] : 0u;
    uint32_t nv = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) nv += (uint32_t)__builtin_popcount((packed >> (8 * r)) & 7u);
    uint32_t tot;
    uint32_t vid = boff[2 * blockIdx.x] + block_exscan_256(nv, sh, tot);
    const uint32_t stride[3] = { d.ny * d.nz, d.nz, 1u };
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t m = (packed >> (8 * r)) & 7u;
        if (!m) continue;
        const uint32_t p = p0 + r;
        voff[p] = vid;
        const uint32_t k = p % d.nz, t = p / d.nz, j = t % d.ny, i = t / d.ny;
        const double va = (double)vol[p];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((m >> a) & 1u)) continue;
            const double vb = (double)vol[p + stride[a]];
            const double tt = ((double)iso - va) / (vb - va);            // the linear zero crossing between the two grid points, 0 <= tt <= 1
            double c[3] = { (double)i, (double)j, (double)k };
            c[a] += tt;
            if (vid < n_verts) {
                verts[3 * (size_t)vid] = c[0] / xf.den * xf.span[0] + xf.lo[0];
                verts[3 * (size_t)vid + 1] = c[1] / xf.den * xf.span[1] + xf.lo[1];
                verts[3 * (size_t)vid + 2] = c[2] / xf.den * xf.span[2] + xf.lo[2];
            }
            ++vid;
        }
    }
}

__global__ __launch_bounds__(256) void mc_triangles_kernel(const uint32_t *__restrict__ bits, const McDims d, const uint32_t *__restrict__ cnt4,
                                                           const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ voff,
                                                           int32_t *__restrict__ tris, uint32_t n_tris)
{
    __shared__ uint32_t sh[8];
    if ((bsum[blockIdx.x] >> 16) == 0u) return;
    const uint32_t p0 = blockIdx.x * MC_PTS + threadIdx.x * 4u;
    const uint32_t packed = p0 < d.npts ? cnt4[p0 >> 2] : 0u;
    uint32_t nt = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) nt += (packed >> (8 * r + 3)) & 7u;
    uint32_t tot;
    uint32_t tid = boff[2 * blockIdx.x + 1] + block_exscan_256(nt, sh, tot);
    const uint8_t *cnt8 = reinterpret_cast<const uint8_t *>(cnt4);
    const uint32_t sx = d.ny * d.nz, sy = d.nz;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t n = (packed >> (8 * r + 3)) & 7u;
        if (!n) continue;
        const uint32_t p = p0 + r;
        uint32_t cs;
        (void)mc_classify(bits, d, p, &cs);
        for (uint32_t t = 0; t < n; ++t) {
            int32_t id[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int e = AC_MC_TRI[cs][3 * t + q];
                const uint32_t c0 = AC_MC_EDGE[e][0], a = (uint32_t)e >> 2;
                const uint32_t pq = p + (c0 & 1u) * sx + ((c0 >> 1) & 1u) * sy + ((c0 >> 2) & 1u);     // the grid point that owns edge e of this cell
                const uint32_t m = cnt8[pq] & 7u;
                id[q] = (int32_t)(voff[pq] + (uint32_t)__builtin_popcount(m & ((1u << a) - 1u)));
            }
            if (tid < n_tris) { tris[3 * (size_t)tid] = id[0]; tris[3 * (size_t)tid + 1] = id[1]; tris[3 * (size_t)tid + 2] = id[2]; }
            ++tid;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- attributes of a mesh's vertices
// What a coloured export needs per vertex and marching cubes does not give: a position ON the level set (the linear zero crossing of a grid edge is off it by
// up to 8.6e-3 on the golden field at 24^3), the field's normal and the colour network there.  Shaped like field_samples_kernel (render_occupancy.hip): a wave owns
// tiles of 16 vertices, lane (n, g) works on vertex n of the tile, the four lanes of a vertex hold the same position.  Per vertex, all in fp32:
//   p = clamp((float)vertex); at most `steps` times: stencil at p -> s, g; r = s - target; |r| <= tol: stop; gg = (gx gx + gy gy) + gz gz; not gg > 1e-12:
//   stop (status 2); q = clamp(p - (r / gg) g); max_k |q_k - p0_k| > max_move: stop (status 3); p = q.  Then normal and colour at the final p.
// The status is the reason the steps ended: 0 the tolerance test of a step was met, 1 all `steps` steps were taken (the value at the final p is in `sdf`).
// One copy of the stencil code serves the steps AND the final evaluation: iteration `it` evaluates at p, then the lanes still moving step; when no lane of the
// wave moved (or it == steps: no step is allowed) that evaluation was at every lane's final position and the loop ends -- at most steps + 1 trips, the count
// wave-uniform, stopped lanes ride along at their p.  No atomics, no waits on other waves.
struct MeshAttrArgs {
    const double *verts;        // [V,3] as mc_vertices_kernel writes them
    const float *dirs;          // [V,3] or NULL: -normal
    uint32_t V;
    int steps;
    float target, tol, max_move;
    float *pos, *nrm, *rgb, *sdf;      // [V,3] [V,3] [V,3] | NULL, [V] | NULL
    uint8_t *status;                   // [V] | NULL
};

// "refine and shade one tile of 16 points": the loop above and the evaluation at the final p, shared by the vertex kernel and the texel kernel below.  In: lane
// (n, g)'s point p (clamped; the four lanes of a point agree) and whether it may move.  Out: the final p, sdf, status, normal and colour there (rgb in the lanes
// g == 0).  dirs / di: the launch's view directions and this lane's row in them, or NULL: -normal.  Every lane of the wave calls it.
struct RefineOpts { int steps; float target, tol, max_move; bool want_rgb; };
struct TileShade { float s; uint32_t st; FdNormal fn; float rgb[3]; };

__device__ __forceinline__ TileShade refine_shade_tile(float *lds, float *fsl, const FieldCtx &fc, const RenderArgs &a, const RefineOpts &m, int lane,
                                                       const float *dirs, size_t di, bool moving, float &px, float &py, float &pz)
{
    const int n = lane & 15;
    const float bound = a.bound, eps = a.eps;
    const float p0x = px, p0y = py, p0z = pz;
    uint32_t st = 1u;
    f32x4 o16;
    float gr[3], s;
#pragma unroll 1
    for (int it = 0;; ++it) {
        float fe0[4][2];
        encode_stencil(lds, fsl, fc, lane, px, py, pz, eps, fe0);
        fd_forward(lds, fsl, lane, px, py, pz, eps, bound, fe0, o16, gr);
        s = __shfl(o16[0], n);                                               // output 0 lives in the lanes g == 0
        wave_sync();                                                         // (every lane is done with the feature slab)
        bool moved = false;
        if (moving && it < m.steps) {
            const float r = s - m.target;
            const float gg = (gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2];
            if (__builtin_fabsf(r) <= m.tol) { moving = false; st = 0u; }
            else if (!(gg > 1e-12f)) { moving = false; st = 2u; }
            else {
                const float t = r / gg;
                const float qx = clampf(px - t * gr[0], -bound, bound), qy = clampf(py - t * gr[1], -bound, bound), qz = clampf(pz - t * gr[2], -bound, bound);
                const float dm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(qx - p0x), __builtin_fabsf(qy - p0y)), __builtin_fabsf(qz - p0z));
                if (dm > m.max_move) { moving = false; st = 3u; }
                else { px = qx; py = qy; pz = qz; moved = true; }
            }
        }
        if (it >= m.steps || __ballot(moved) == 0ull) break;               // (wave-uniform)
    }
    TileShade r{ s, st, fd_normal(gr[0], gr[1], gr[2]), { 0.0f, 0.0f, 0.0f } };
    if (m.want_rgb) {                                                        // (uniform over the launch)
        if (a.Wsh) {
            float dx = -r.fn.nx, dy = -r.fn.ny, dz = -r.fn.nz;
            if (dirs) { const float *d = dirs + 3 * di; dx = d[0]; dy = d[1]; dz = d[2]; }
            sample_sh_bias(fsl, a.Wsh, dx, dy, dz, lane);
            color_tile(lds, lane, px, py, pz, r.fn.nx, r.fn.ny, r.fn.nz, o16, r.rgb, fsl + 4 * lane, 256);
        } else color_tile(lds, lane, px, py, pz, r.fn.nx, r.fn.ny, r.fn.nz, o16, r.rgb);
    }
    return r;
}

__global__ __launch_bounds__(FBLOCK) void mesh_attrs_kernel(const RenderArgs a, const MeshAttrArgs m)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (m.rgb) fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const RefineOpts ro{ m.steps, m.target, m.tol, m.max_move, m.rgb != nullptr };
    const uint32_t ntiles = (m.V + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.V ? b : m.V - 1;
        const double *vx = m.verts + 3 * (size_t)bb;
        float px = clampf((float)vx[0], -bound, bound), py = clampf((float)vx[1], -bound, bound), pz = clampf((float)vx[2], -bound, bound);
        const TileShade r = refine_shade_tile(lds, fsl, fc, a, ro, lane, m.dirs, (size_t)bb, true, px, py, pz);
        if (b < m.V && g == 0) {
            m.pos[3 * (size_t)b] = px; m.pos[3 * (size_t)b + 1] = py; m.pos[3 * (size_t)b + 2] = pz;
            m.nrm[3 * (size_t)b] = r.fn.nx; m.nrm[3 * (size_t)b + 1] = r.fn.ny; m.nrm[3 * (size_t)b + 2] = r.fn.nz;
            if (m.rgb) { m.rgb[3 * (size_t)b] = r.rgb[0]; m.rgb[3 * (size_t)b + 1] = r.rgb[1]; m.rgb[3 * (size_t)b + 2] = r.rgb[2]; }
            if (m.sdf) m.sdf[b] = r.s;
            if (m.status) m.status[b] = (uint8_t)r.st;
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------- texture bake: the same body over texels
// The atlas is closed form (avatarcraft_amd/geometry.py: atlas_layout): the S x S image is cut into R x R cells of c x c texels, R = S / c; triangle t
// lives in cell t >> 1 (column k % R, row k / R), half t & 1.  Texel (i, j) of a cell belongs to half 0 iff i + j <= c - 2.  Its barycentric weights, in fp32, every
// operation rounded once, L = c - 5:  half 0: w1 = (i - 1) / L, w2 = (j - 1) / L;  half 1: w1 = (c - 2 - i) / L, w2 = (c - 2 - j) / L;  w1 = max(w1, 0),
// w2 = max(w2, 0), s = w1 + w2;  s > 1: w1 /= s, w2 /= s, w0 = 0;  else w0 = 1 - s -- a texel outside the UV triangle takes a point ON the triangle (the gutter).
// Its point, per coordinate: p = (w0 P0 + w1 P1) + w2 P2, clamped to +-bound; then refine_shade_tile, view direction -normal.
// A wave takes tiles of 16 consecutive texels of an image row (ceil(S / 16) tiles per row).  A tile without an owned texel issues no field evaluation (the test is
// wave-uniform); in a tile with some, the lanes of the others ride along at the first owned texel's point without moving, and store owner = -1 and zeros.
struct BakeArgs {
    const float *pos;           // [V,3]
    const int32_t *tris;        // [T,3], every index in [0, V)
    uint32_t T, S, c, R;
    RefineOpts ro;
    float *rgb, *nrm, *sdf;     // [S,S,3], [S,S,3] | NULL, [S,S] | NULL
    int32_t *owner;             // [S,S]
    uint8_t *status;            // [S,S] | NULL
};

__global__ __launch_bounds__(FBLOCK) void texture_bake_kernel(const RenderArgs a, const BakeArgs m)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const uint32_t S = m.S, c = m.c, per_row = (S + 15) / 16, ntiles = per_row * S;
    const float L = (float)(c - 5u);
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t y = tile / per_row, x = (tile - y * per_row) * 16 + n;
        const uint32_t cx = x / c, cy = y / c, i = x - cx * c, j = y - cy * c;
        const uint32_t h = i + j + 2 <= c ? 0u : 1u, t = 2 * (cy * m.R + cx) + h;
        const bool owned = x < S && cx < m.R && cy < m.R && t < m.T;
        const unsigned long long own_mask = __ballot(owned);
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        TileShade r{ 0.0f, 0u, FdNormal{ 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
        if (own_mask) {                                                          // (wave-uniform)
            if (owned) {
                const int di = h ? (int)(c - 2u - i) : (int)i - 1, dj = h ? (int)(c - 2u - j) : (int)j - 1;
                float w1 = __builtin_fmaxf((float)di / L, 0.0f), w2 = __builtin_fmaxf((float)dj / L, 0.0f), w0 = 0.0f;
                const float s = w1 + w2;
                if (s > 1.0f) { w1 = w1 / s; w2 = w2 / s; } else w0 = 1.0f - s;
                const int32_t *tv = m.tris + 3 * (size_t)t;
                const float *P0 = m.pos + 3 * (size_t)tv[0], *P1 = m.pos + 3 * (size_t)tv[1], *P2 = m.pos + 3 * (size_t)tv[2];
                px = clampf((w0 * P0[0] + w1 * P1[0]) + w2 * P2[0], -bound, bound);
                py = clampf((w0 * P0[1] + w1 * P1[1]) + w2 * P2[1], -bound, bound);
                pz = clampf((w0 * P0[2] + w1 * P1[2]) + w2 * P2[2], -bound, bound);
            }
            const int first = __builtin_ctzll(own_mask) & 15;                   // (the four lanes of a texel agree, so its lane g == 0 is the lowest set bit)
            const float fx = __shfl(px, first), fy = __shfl(py, first), fz = __shfl(pz, first);
            if (!owned) { px = fx; py = fy; pz = fz; }
            r = refine_shade_tile(lds, fsl, fc, a, m.ro, lane, nullptr, 0, owned, px, py, pz);
        }
        if (x < S && g == 0) {
            const size_t b = (size_t)y * S + x;
            m.owner[b] = owned ? (int32_t)t : -1;
            m.rgb[3 * b] = owned ? r.rgb[0] : 0.0f; m.rgb[3 * b + 1] = owned ? r.rgb[1] : 0.0f; m.rgb[3 * b + 2] = owned ? r.rgb[2] : 0.0f;
            if (m.nrm) { m.nrm[3 * b] = owned ? r.fn.nx : 0.0f; m.nrm[3 * b + 1] = owned ? r.fn.ny : 0.0f; m.nrm[3 * b + 2] = owned ? r.fn.nz : 0.0f; }
            if (m.sdf) m.sdf[b] = owned ? r.s : 0.0f;
            if (m.status) m.status[b] = owned ? (uint8_t)r.st : (uint8_t)0;
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------- first-hit render of the level set
// The image of the surface the export writes: per ray the first point with sdf = level, found by sphere-tracing steps until the sign changes and guarded false
// position inside the bracket (the procedure, operation by operation: include/avatarcraft_hip.h, ac_render_rays_surface), then refine_shade_tile with steps = 0
// at that point -- normal, sdf and colour as ac_field_samples gives them.  A wave owns tiles of 16 consecutive rays, lane (n, g) serves ray n of the tile (the
// four lanes of a ray hold the same state).  Every trip of the root-finder loop is ONE sdf_tile call at every lane's current point, then the scalar update in the
// lanes still active; stopped lanes ride along at their point.  The loop ends when no lane of the wave is active or after max_iters trips: wave-uniform, bounded.
// A tile without a shaded ray (status 0, 1 or 3) skips the stencil and the colour network; in a tile with some, the other lanes ride along at the first shaded
// lane's point.  No atomics, no waits on other waves, plain vector stores.
struct SurfaceArgs {
    const float *rays_o, *rays_d, *bg;     // [N,3] [N,3] [N,3] | NULL: white
    uint32_t N;
    int max_iters;
    float level, tol, step_scale, min_step, guard;
    float *image, *weights_sum, *depth, *position, *normal_map, *sdf;      // each [N] / [N,3] | NULL
    uint8_t *status, *iters;               // [N], [N] | NULL
};

__global__ __launch_bounds__(FBLOCK) void surface_rays_kernel(const RenderArgs a, const SurfaceArgs m)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (m.image) fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const RefineOpts ro{ 0, 0.0f, 0.0f, 0.0f, m.image != nullptr };
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const float *po = m.rays_o + 3 * (size_t)bb, *pd = m.rays_d + 3 * (size_t)bb;
        const float ox = po[0], oy = po[1], oz = po[2], dx = pd[0], dy = pd[1], dz = pd[2];
        float near, far;
        cube_near_far(ox, oy, oz, dx, dy, dz, bound, near, far);
        float t = near, t_lo = 0.0f, s_lo = 0.0f, t_hi = 0.0f, s_hi = 0.0f;
        uint32_t st = 2u, iters = 0u;
        bool active = far > near, have_lo = false, bracketed = false;
        float px = clampf(ox + t * dx, -bound, bound), py = clampf(oy + t * dy, -bound, bound), pz = clampf(oz + t * dz, -bound, bound);
#pragma unroll 1
        for (int it = 1; it <= m.max_iters; ++it) {
            if (__ballot(active) == 0ull) break;                                 // (wave-uniform)
            const f32x4 o = sdf_tile(lds, fc, lane, px, py, pz);
            const float s = __shfl(o[0], n) - m.level;                           // output 0 lives in the lanes g == 0
            if (active) {
                iters = (uint32_t)it;
                float t_next = t;
                bool in_bracket = false;
                if (!(__builtin_fabsf(s) < __builtin_inff())) { st = 5u; active = false; }
                else if (__builtin_fabsf(s) <= m.tol) { st = 0u; active = false; }
                else if (bracketed) {
                    if (s > 0.0f) { t_lo = t; s_lo = s; } else { t_hi = t; s_hi = s; }
                    in_bracket = true;
                } else if (s > 0.0f) {                                           // still outside: a sphere-tracing step, never past far
                    if (t >= far) { st = 2u; active = false; }
                    else {
                        t_lo = t; s_lo = s; have_lo = true;
                        t_next = __builtin_fminf(t + __builtin_fmaxf(m.step_scale * s, m.min_step), far);
                    }
                } else if (!have_lo) { st = 3u; active = false; }                // the first evaluation is already inside
                else { bracketed = true; t_hi = t; s_hi = s; in_bracket = true; }
                if (in_bracket) {                                                // guarded false position
                    const float w = t_hi - t_lo, q = s_lo / (s_lo - s_hi), f = t_lo + w * q, gd = m.guard * w;
                    t_next = __builtin_fminf(__builtin_fmaxf(f, t_lo + gd), t_hi - gd);
                }
                if (active) {
                    if (it == m.max_iters) { st = bracketed ? 1u : 4u; active = false; }       // (t stays the last evaluated t)
                    else {
                        t = t_next;
                        px = clampf(ox + t * dx, -bound, bound); py = clampf(oy + t * dy, -bound, bound); pz = clampf(oz + t * dz, -bound, bound);
                    }
                }
            }
        }
        const bool shaded = st == 0u || st == 1u || st == 3u;
        const unsigned long long sh_mask = __ballot(shaded);
        TileShade r{ 0.0f, 0u, FdNormal{ 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
        const float hx = px, hy = py, hz = pz;                                   // this ray's own point
        if (sh_mask) {                                                           // (wave-uniform)
            const int first = __builtin_ctzll(sh_mask) & 15;                     // (the four lanes of a ray agree, so its lane g == 0 is the lowest set bit)
            const float fx = __shfl(px, first), fy = __shfl(py, first), fz = __shfl(pz, first);
            if (!shaded) { px = fx; py = fy; pz = fz; }
            r = refine_shade_tile(lds, fsl, fc, a, ro, lane, m.rays_d, (size_t)bb, false, px, py, pz);
        }
        if (b < m.N && g == 0) {
            const size_t b3 = 3 * (size_t)b;
            if (m.image) {
                float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
                if (shaded) { c0 = r.rgb[0]; c1 = r.rgb[1]; c2 = r.rgb[2]; }
                else if (m.bg) { c0 = m.bg[b3]; c1 = m.bg[b3 + 1]; c2 = m.bg[b3 + 2]; }
                m.image[b3] = c0; m.image[b3 + 1] = c1; m.image[b3 + 2] = c2;
            }
            if (m.weights_sum) m.weights_sum[b] = shaded ? 1.0f : 0.0f;
            if (m.depth) m.depth[b] = shaded ? t : 0.0f;
            if (m.position) { m.position[b3] = shaded ? hx : 0.0f; m.position[b3 + 1] = shaded ? hy : 0.0f; m.position[b3 + 2] = shaded ? hz : 0.0f; }
            if (m.normal_map) { m.normal_map[b3] = shaded ? r.fn.nx : 0.0f; m.normal_map[b3 + 1] = shaded ? r.fn.ny : 0.0f; m.normal_map[b3 + 2] = shaded ? r.fn.nz : 0.0f; }
            if (m.sdf) m.sdf[b] = shaded ? r.s : 0.0f;
            m.status[b] = (uint8_t)st;
            if (m.iters) m.iters[b] = (uint8_t)iters;
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------- first-hit render of the POSED level set
// The image of { p : sdf(W^-1(p)) = level, p inside the mask }: the set the posed renderer draws and net.pose_mesh moves the exported mesh onto (the procedure,
// operation by operation: include/avatarcraft_hip.h, ac_render_rays_surface_warped).  Every evaluation of the traced function needs the closest-face search of
// warp.hip (over the mesh's culling structure: warp_accel.hpp, built by warp_accel_build.hip) at the ray's posed point first.  That search is wave-cooperative and compiled for <= 128 VGPRs, the sdf_tile code needs about 226: they stay separate
// kernels and the root finder's loop is unrolled on the HOST -- a sequence on one stream, the per-ray state kept in the scratch between the launches:
//   posed_start_kernel: near / far, the ray state, the first posed point;
//   max_iters times: the search (unchanged, through its internal launcher; the per-ray `stopped` byte is its ray_dead with one sample per ray), then
//     posed_trip_kernel: ONE sdf_tile call per tile of 16 rays at the clamped canonical points -- only for a tile with an active unmasked ray (ballot) -- and the
//     scalar update; it writes the state, the next posed point (the shaded point of a ray that stops) and the stopped byte;
//   one search at the shaded points (ray_dead = the `noshade` byte), then posed_shade_kernel: refine_shade_tile with steps = 0 at the clamped canonical point behind
//     surface_rays_kernel's ride-along rule, then the blended transform and the cofactor normal of mesh_blend.hpp in fp64, lane = ray.
// The host cannot know when every ray has stopped: all max_iters trips are enqueued, a trip without an active ray reads 16 bytes per tile and evaluates nothing.
// No atomics, no grid barrier, no waits on other waves, plain vector stores; a short last tile reads ray N - 1 and stores nothing for its padding lanes.
enum : uint8_t { PF_HAVE_LO = 1, PF_BRACKETED = 2, PF_LO_MASKED = 4 };
struct PosedState {                        // the scratch of ac_render_rays_surface_warped, one row per ray
    float *pts, *can;                      // [N,3] the posed point the next search reads | its canonical point (the search's can_pts_f32)
    double *closest, *dist2;               // [N,3], [N] of the search
    int32_t *face;                         // [N]
    uint8_t *smask;                        // [N] the search's mask
    uint8_t *stopped, *noshade;            // [N] ray_dead of the trips' searches | of the shading search
    uint8_t *st, *iters, *flags;           // [N] status, evaluations, PF_*
    float *t, *t_lo, *s_lo, *t_hi, *s_hi, *far;      // [N] each; t = the shaded parameter once the ray has stopped
};
struct PosedArgs {
    const float *rays_o, *rays_d, *bg;
    uint32_t N;
    int max_iters;
    float level, tol, step_scale, min_step, guard, w_tol, rt;
    PosedState s;
};

__global__ __launch_bounds__(256) void posed_start_kernel(const PosedArgs m, float bound)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= m.N) return;
    const float *po = m.rays_o + 3 * (size_t)b, *pd = m.rays_d + 3 * (size_t)b;
    float near, far;
    cube_near_far(po[0], po[1], po[2], pd[0], pd[1], pd[2], bound, near, far);
    const PosedState &s = m.s;
    s.t[b] = near; s.far[b] = far;
    s.t_lo[b] = 0.0f; s.s_lo[b] = 0.0f; s.t_hi[b] = 0.0f; s.s_hi[b] = 0.0f;
    s.flags[b] = 0; s.st[b] = 2; s.iters[b] = 0;
    s.stopped[b] = far > near ? 0 : 1;
    s.noshade[b] = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.pts[3 * (size_t)b + k] = clampf(po[k] + near * pd[k], -bound, bound);
}

__global__ __launch_bounds__(FBLOCK) void posed_trip_kernel(const RenderArgs a, const PosedArgs m, int it)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const PosedState &s = m.s;
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const bool active = s.stopped[bb] == 0;                                  // a stopped ray was not searched: nothing of the search is read for it
        const bool unmasked = active && s.smask[bb] != 0;
        const unsigned long long um = __ballot(unmasked);
        float sv = 0.0f;
        if (um) {                                                                // (wave-uniform) one evaluation at the clamped canonical points
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
            if (unmasked) {
                const float *c = s.can + 3 * (size_t)bb;
                cx = clampf(c[0], -bound, bound); cy = clampf(c[1], -bound, bound); cz = clampf(c[2], -bound, bound);
            }
            const int first = __builtin_ctzll(um) & 15;                          // (the four lanes of a ray agree) the other lanes ride along at its point
            const float fx = __shfl(cx, first), fy = __shfl(cy, first), fz = __shfl(cz, first);
            if (!unmasked) { cx = fx; cy = fy; cz = fz; }
            const f32x4 o = sdf_tile(lds, fc, lane, cx, cy, cz);
            sv = __shfl(o[0], n) - m.level;                                      // output 0 lives in the lanes g == 0
        }
        if (active && b < m.N && g == 0) {
            float t = s.t[b], t_lo = s.t_lo[b], s_lo = s.s_lo[b], t_hi = s.t_hi[b], s_hi = s.s_hi[b];
            const float far = s.far[b];
            uint32_t fl = s.flags[b], st = 2u;
            bool stop = false, in_bracket = false;
            float sc = sv, k = m.step_scale, t_next = t;
            if (!unmasked) {                                                     // outside the mask: the gap to the drawable region, an exact safe step
                const float e = __builtin_sqrtf((float)s.dist2[b]) - m.rt;
                if (!(__builtin_fabsf(e) < __builtin_inff())) { st = 5u; stop = true; }
                sc = __builtin_fmaxf(e, m.min_step); k = 1.0f;
            }
            if (stop) {}
            else if (!(__builtin_fabsf(sc) < __builtin_inff())) { st = 5u; stop = true; }
            else if (unmasked && __builtin_fabsf(sc) <= m.tol) { st = 0u; stop = true; }
            else if (fl & PF_BRACKETED) {
                if (sc > 0.0f) { t_lo = t; s_lo = sc; fl = unmasked ? (fl & ~(uint32_t)PF_LO_MASKED) : (fl | PF_LO_MASKED); } else { t_hi = t; s_hi = sc; }
                in_bracket = true;
            } else if (sc > 0.0f) {                                              // still outside: a sphere-tracing step, never past far
                if (t >= far) { st = 2u; stop = true; }
                else {
                    t_lo = t; s_lo = sc; fl |= PF_HAVE_LO; fl = unmasked ? (fl & ~(uint32_t)PF_LO_MASKED) : (fl | PF_LO_MASKED);
                    t_next = __builtin_fminf(t + __builtin_fmaxf(k * sc, m.min_step), far);
                }
            } else if (!(fl & PF_HAVE_LO)) { st = 3u; stop = true; }             // the first evaluation is already inside
            else { fl |= PF_BRACKETED; t_hi = t; s_hi = sc; in_bracket = true; }
            if (in_bracket) {
                const float w = t_hi - t_lo;
                if (w <= m.w_tol) { st = 6u; stop = true; }                      // the bracket closed on a jump: the mask boundary cuts the body here
                else {                                                           // guarded false position; bisection while the positive end is a masked point
                    const float q = (fl & PF_LO_MASKED) ? 0.5f : s_lo / (s_lo - s_hi), f = t_lo + w * q, gd = m.guard * w;
                    t_next = __builtin_fminf(__builtin_fmaxf(f, t_lo + gd), t_hi - gd);
                }
            }
            if (!stop && it == m.max_iters) { st = (fl & PF_BRACKETED) ? 1u : 4u; stop = true; }
            bool shaded = false;
            if (stop) {
                shaded = st == 0u || st == 1u || st == 3u || st == 6u;
                if (st == 1u || st == 6u) t = t_hi;                              // the shaded parameter: the bracket's inner end
                s.stopped[b] = 1; s.noshade[b] = shaded ? 0 : 1; s.st[b] = (uint8_t)st;
            } else t = t_next;
            s.iters[b] = (uint8_t)it;
            s.t[b] = t; s.t_lo[b] = t_lo; s.s_lo[b] = s_lo; s.t_hi[b] = t_hi; s.s_hi[b] = s_hi; s.flags[b] = (uint8_t)fl;
            if (!stop || shaded) {                                               // the next search's point | the shading search's point
                const float *po = m.rays_o + 3 * (size_t)b, *pd = m.rays_d + 3 * (size_t)b;
#pragma unroll
                for (int c = 0; c < 3; ++c) s.pts[3 * (size_t)b + c] = clampf(po[c] + t * pd[c], -bound, bound);
            }
        }
    }
}

struct PosedOut {
    float *image, *weights_sum, *depth, *position, *normal_map, *sdf, *canonical, *normal_can;      // each [N] / [N,3] | NULL
    int32_t *face_id;                      // [N] | NULL
    uint8_t *status, *iters;               // [N], [N] | NULL
    const float *verts; const int32_t *faces; const double *T;                                      // the frame's guide
};

__global__ __launch_bounds__(FBLOCK) void posed_shade_kernel(const RenderArgs a, const PosedArgs m, const PosedOut out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (out.image) fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const PosedState &s = m.s;
    const RefineOpts ro{ 0, 0.0f, 0.0f, 0.0f, out.image != nullptr };
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const bool shaded = s.noshade[bb] == 0;
        const unsigned long long sh_mask = __ballot(shaded);
        TileShade r{ 0.0f, 0u, FdNormal{ 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;
        if (sh_mask) {                                                           // (wave-uniform)
            if (shaded) {
                const float *c = s.can + 3 * (size_t)bb;
                cx = clampf(c[0], -bound, bound); cy = clampf(c[1], -bound, bound); cz = clampf(c[2], -bound, bound);
            }
            const float hx = cx, hy = cy, hz = cz;                               // this ray's own point
            const int first = __builtin_ctzll(sh_mask) & 15;
            const float fx = __shfl(cx, first), fy = __shfl(cy, first), fz = __shfl(cz, first);
            if (!shaded) { cx = fx; cy = fy; cz = fz; }
            r = refine_shade_tile(lds, fsl, fc, a, ro, lane, m.rays_d, (size_t)bb, false, cx, cy, cz);
            cx = hx; cy = hy; cz = hz;
        }
        if (b < m.N && g == 0) {
            const size_t b3 = 3 * (size_t)b;
            if (out.image) {
                float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
                if (shaded) { c0 = r.rgb[0]; c1 = r.rgb[1]; c2 = r.rgb[2]; }
                else if (m.bg) { c0 = m.bg[b3]; c1 = m.bg[b3 + 1]; c2 = m.bg[b3 + 2]; }
                out.image[b3] = c0; out.image[b3 + 1] = c1; out.image[b3 + 2] = c2;
            }
            if (out.weights_sum) out.weights_sum[b] = shaded ? 1.0f : 0.0f;
            if (out.depth) out.depth[b] = shaded ? s.t[b] : 0.0f;
            if (out.position) { out.position[b3] = shaded ? s.pts[b3] : 0.0f; out.position[b3 + 1] = shaded ? s.pts[b3 + 1] : 0.0f; out.position[b3 + 2] = shaded ? s.pts[b3 + 2] : 0.0f; }
            if (out.canonical) { out.canonical[b3] = shaded ? cx : 0.0f; out.canonical[b3 + 1] = shaded ? cy : 0.0f; out.canonical[b3 + 2] = shaded ? cz : 0.0f; }
            if (out.normal_can) { out.normal_can[b3] = shaded ? r.fn.nx : 0.0f; out.normal_can[b3 + 1] = shaded ? r.fn.ny : 0.0f; out.normal_can[b3 + 2] = shaded ? r.fn.nz : 0.0f; }
            if (out.sdf) out.sdf[b] = shaded ? r.s : 0.0f;
            if (out.face_id) out.face_id[b] = shaded ? s.face[b] : -1;
            if (out.normal_map) {
                float nm[3] = { 0.0f, 0.0f, 0.0f };
                if (shaded) {                                                    // ac_mesh_pose's rules: M blended at the search's closest point and face
                    const size_t f = (size_t)s.face[b];                          // the search's own answer: always a face of the mesh
                    const int32_t f0v = out.faces[3 * f], f1v = out.faces[3 * f + 1], f2v = out.faces[3 * f + 2];
                    const double q[3] = { s.closest[b3], s.closest[b3 + 1], s.closest[b3 + 2] };
                    double bc[3];
                    face_bary(q, out.verts, f0v, f1v, f2v, bc);
                    const Blend M = blend3(out.T, f0v, f1v, f2v, bc);
                    const float nc[3] = { r.fn.nx, r.fn.ny, r.fn.nz };
                    normal_store(M, nc, nm);
                }
                out.normal_map[b3] = nm[0]; out.normal_map[b3 + 1] = nm[1]; out.normal_map[b3 + 2] = nm[2];
            }
            out.status[b] = s.st[b];
            if (out.iters) out.iters[b] = s.iters[b];
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------- density grid of the ray marcher
// Round 6: two launches instead of one.  Round 5 gave every workgroup a brick of 16 x 8 x 8 outputs PLUS the one-point halo the 2^3 max pool reads
// (17 x 9 x 9 = 1377 evaluations for 1024 outputs, 3.58 M for the 2.15 M points of the 129^3 grid) and cut them into tiles of 16 consecutive evaluations of
// a 17-wide row -- tiles that straddle two rows, i.e. none of what makes field_sdf_grid_kernel fast (16 points along x = 2 .. 9 sectors per gather).
//   1. field_sdf_grid_kernel<.., true> in mode 2: the density of every grid point ONCE, on x-tiles, into a scratch volume (8.6 MB at 129^3: L2-resident);
//   2. density_pool_kernel: zero pad + 2^3 max pool of that volume, maximum(grid * decay, new) in place, the mean -- one short streaming pass.
// 0.94 -> 0.3x ms per update (bench.py: density_grid_update); the same values (sdf bits, expf / divide, max).
struct DgArgs {
    const float *dens;        // [H,H,H] the densities of pass 1
    uint32_t H;
    float decay;
    float *grid;              // [H,H,H] in / out
    double *partials;         // [number of workgroups]
    uint32_t *ticket;         // [1], zero between launches (the last workgroup re-arms it)
    double *mean_out;         // [1]
};
constexpr int DP_BLOCK = 256;

__global__ __launch_bounds__(DP_BLOCK) void density_pool_kernel(const DgArgs g_)
{
    __shared__ double red[DP_BLOCK / 64];
    __shared__ uint32_t last;
    const uint32_t H = g_.H, N = H * H * H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double part = 0.0;
#pragma unroll 4
    for (uint32_t p = blockIdx.x * DP_BLOCK + threadIdx.x; p < N; p += gridDim.x * DP_BLOCK) {       // z fastest: the grid's own order
        const uint32_t gz = p % H, t = p / H, gy = t % H, gx = t / H;
        float m = 0.0f;                                                      // (F.max_pool3d over the zero-padded tmp_grid (:341); densities are >= 0)
#pragma unroll
        for (uint32_t dx = 0; dx < 2; ++dx)
#pragma unroll
            for (uint32_t dy = 0; dy < 2; ++dy)
#pragma unroll
                for (uint32_t dz = 0; dz < 2; ++dz)
                    if (gx + dx < H && gy + dy < H && gz + dz < H) m = fmaxf(m, g_.dens[((size_t)(gx + dx) * H + (gy + dy)) * H + (gz + dz)]);
        const float v = fmaxf(g_.grid[p] * g_.decay, m);                     // torch.maximum(density_grid * decay, tmp_grid)  (:345)
        g_.grid[p] = v;
        part += (double)v;
    }
    // mean: per-wave shuffle tree -> per-workgroup sum (fixed order) -> the last workgroup adds the workgroups' partials (fixed order); in double, where the
    // reference's torch.mean reduces in fp32 -- the two agree to ~1e-7 relative (tests: <= 1e-6), not bit for bit: mean_density is a threshold of the marcher
    // (density > min(mean, 0.01 ...)), compared against values that differ from it by orders of magnitude
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < DP_BLOCK / 64; ++w) s += red[w];
        g_.partials[blockIdx.x] = s;
        __threadfence();
        last = atomicAdd(g_.ticket, 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += DP_BLOCK)             // (agent-scope loads: served by L2, never by a stale vector-L1 line)
        s += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(g_.partials) + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < DP_BLOCK / 64; ++w) tot += red[w];
        g_.mean_out[0] = tot / ((double)H * (double)H * (double)H);
        *g_.ticket = 0u;
    }
}

int geo_args(RenderArgs &a, const ac_field *field, float bound)
{
    if (int rc = fill_args(a, field, bound)) return rc;
    a.T0 = 0; a.lin_z = nullptr; a.lin_u = nullptr;
    return AC_OK;
}

struct McLayout { size_t cnt, voff, bsum, boff, bits, total; uint32_t nblk; };
McLayout mc_layout(uint32_t nx, uint32_t ny, uint32_t nz)
{
    McLayout l{};
    const uint64_t npts = (uint64_t)nx * ny * nz;
    l.nblk = (uint32_t)((npts + MC_PTS - 1) / MC_PTS);
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    l.cnt = o; o += al((size_t)l.nblk * MC_PTS);
    l.voff = o; o += al((size_t)npts * 4);
    l.bsum = o; o += al((size_t)l.nblk * 4);
    l.boff = o; o += al((size_t)l.nblk * 8);
    l.bits = o; o += al(((size_t)l.nblk * MC_PTS / 64 + 2) * 8);
    l.total = o;
    return l;
}

int mc_check(const char *who, const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, const void *scratch, size_t scratch_bytes, McLayout &l)
{
    if (!vol || !scratch) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    if (nx < 2 || ny < 2 || nz < 2 || (uint64_t)nx * ny * nz >= (1ull << 31)) { ac::set_error("%s: grid %u x %u x %u unsupported (2 <= n, fewer than 2^31 points)", who, nx, ny, nz); return AC_ERR_BAD_ARG; }
    l = mc_layout(nx, ny, nz);
    if (scratch_bytes < l.total) { ac::set_error("%s: scratch of %zu bytes needed, %zu given", who, l.total, scratch_bytes); return AC_ERR_BAD_ARG; }
    return AC_OK;
}

// the regular-grid launch shared by ac_field_sdf_grid and ac_density_grid_update (mode: see field_sdf_grid_kernel)
int launch_grid(const RenderArgs &a, const float *axis_x, const float *axis_y, const float *axis_z, uint32_t nx, uint32_t ny, uint32_t nz, int mode, float inv_s,
                float *volume, hipStream_t stream, const char *what)
{
    const size_t lds_bytes = (OFF_WAVE + GB_X * GB_Y * GB_Z) * sizeof(float);
    uint32_t blocks = ((nx + GB_X - 1) / GB_X) * ((ny + GB_Y - 1) / GB_Y) * ((nz + GB_Z - 1) / GB_Z);
    // persistent workgroups, exactly as many as the device keeps resident at once (43 KB of LDS each; the registers decide): a workgroup that had to
    // wait for a slot would start its share of the tiles when the others are done
    static int per_cu = 0;
    if (!per_cu) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, field_sdf_grid_kernel, BLOCK, lds_bytes) != hipSuccess || n < 1) n = 1;
        per_cu = n;
    }
    const uint32_t cap = (uint32_t)per_cu * ac::cu_count();
    if (blocks > cap) blocks = cap;
    blocks = (blocks + 7u) & ~7u;                                     // every XCD the same number of workgroups
    hipLaunchKernelGGL(field_sdf_grid_kernel, dim3(blocks), dim3(BLOCK), lds_bytes, stream, a, axis_x, axis_y, axis_z, nx, ny, nz, mode, inv_s, volume);
    return ac::check_launch(what);
}

}  // namespace

AC_API int ac_field_sdf_grid(const ac_field *field, const float *axis_x, const float *axis_y, const float *axis_z, uint32_t nx, uint32_t ny, uint32_t nz,
                             float bound, int negate, float *volume, ac_stream_t stream)
{
    if (nx == 0 || ny == 0 || nz == 0) return AC_OK;
    if (!axis_x || !axis_y || !axis_z || !volume) { ac::set_error("field_sdf_grid: NULL buffer"); return AC_ERR_BAD_ARG; }
    if ((uint64_t)nx * ny * nz >= (1ull << 32) - 16) { ac::set_error("field_sdf_grid: more than 2^32 grid points"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = geo_args(a, field, bound)) return rc;
    return launch_grid(a, axis_x, axis_y, axis_z, nx, ny, nz, negate ? 1 : 0, 0.0f, volume, (hipStream_t)stream, "field_sdf_grid");
}

AC_API size_t ac_marching_cubes_scratch(uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (nx < 2 || ny < 2 || nz < 2 || (uint64_t)nx * ny * nz >= (1ull << 31)) return 0;
    return mc_layout(nx, ny, nz).total;
}

AC_API int ac_marching_cubes_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *scratch, size_t scratch_bytes,
                                   uint32_t *counts, ac_stream_t stream)
{
    McLayout l;
    if (int rc = mc_check("marching_cubes_count", volume, nx, ny, nz, scratch, scratch_bytes, l)) return rc;
    if (!counts) { ac::set_error("marching_cubes_count: NULL counts"); return AC_ERR_BAD_ARG; }
    char *sc = static_cast<char *>(scratch);
    const McDims d{ nx, ny, nz, nx * ny * nz };
    {
        const uint32_t nchunks = (d.npts + 1023u) >> 10;
        uint32_t blocks = (nchunks + 3u) / 4u;
        const uint32_t cap = 32u * ac::cu_count();
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(mc_flags_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, volume, d.npts, iso, reinterpret_cast<unsigned long long *>(sc + l.bits));
    }
    hipLaunchKernelGGL(mc_classify_kernel, dim3(l.nblk), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(sc + l.bits), d,
                       reinterpret_cast<uint32_t *>(sc + l.cnt), reinterpret_cast<uint32_t *>(sc + l.bsum));
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(sc + l.bsum), l.nblk,
                       reinterpret_cast<uint32_t *>(sc + l.boff), counts);
    return ac::check_launch("marching_cubes_count");
}

AC_API int ac_marching_cubes_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *scratch, size_t scratch_bytes,
                                  double den, const double span[3], const double lo[3], double *vertices, uint32_t n_vertices, int32_t *triangles,
                                  uint32_t n_triangles, ac_stream_t stream)
{
    McLayout l;
    if (int rc = mc_check("marching_cubes_emit", volume, nx, ny, nz, scratch, scratch_bytes, l)) return rc;
    if ((n_vertices && !vertices) || (n_triangles && !triangles) || !span || !lo || !(den != 0.0)) { ac::set_error("marching_cubes_emit: NULL buffer or den == 0"); return AC_ERR_BAD_ARG; }
    char *sc = static_cast<char *>(scratch);
    const McDims d{ nx, ny, nz, nx * ny * nz };
    McXform xf{ den, { span[0], span[1], span[2] }, { lo[0], lo[1], lo[2] } };
    const uint32_t *cnt4 = reinterpret_cast<const uint32_t *>(sc + l.cnt), *bsum = reinterpret_cast<const uint32_t *>(sc + l.bsum);
    const uint32_t *boff = reinterpret_cast<const uint32_t *>(sc + l.boff);
    uint32_t *voff = reinterpret_cast<uint32_t *>(sc + l.voff);
    if (n_vertices)
        hipLaunchKernelGGL(mc_vertices_kernel, dim3(l.nblk), dim3(256), 0, (hipStream_t)stream, volume, d, iso, cnt4, bsum, boff, voff, xf, vertices, n_vertices);
    if (n_triangles)
        hipLaunchKernelGGL(mc_triangles_kernel, dim3(l.nblk), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(sc + l.bits), d, cnt4, bsum, boff, voff,
                           triangles, n_triangles);
    return ac::check_launch("marching_cubes_emit");
}

AC_API int ac_mesh_vertex_attrs(const ac_field *field, const double *vertices, uint32_t V, const float *dirs, const ac_mesh_attr_opts *opts,
                                float *positions, float *normals, float *rgb, float *sdf, uint8_t *status, ac_stream_t stream)
{
    if (!opts) { ac::set_error("mesh_vertex_attrs: NULL opts"); return AC_ERR_BAD_ARG; }
    if (opts->refine_steps < 0 || opts->refine_steps > 16 || !(opts->max_move > 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("mesh_vertex_attrs: refine_steps outside 0..16, or max_move, fd_eps or bound not > 0"); return AC_ERR_BAD_ARG;
    }
    if (V == 0) return AC_OK;
    if (!vertices || !positions || !normals) { ac::set_error("mesh_vertex_attrs: NULL buffer"); return AC_ERR_BAD_ARG; }
    if (V > 0xffffffe0u) { ac::set_error("mesh_vertex_attrs: more than 2^32 - 32 vertices"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    MeshAttrArgs m{ vertices, dirs, V, opts->refine_steps, opts->target_sdf, opts->tol, opts->max_move, positions, normals, rgb, sdf, status };
    const size_t lds_bytes = FWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(mesh_attrs_kernel), lds_bytes);
    uint32_t blocks = ((V + 15) / 16 + FW - 1) / FW;              // persistent, one workgroup per CU (140 KB of LDS), like ac_field_samples
    const uint32_t cus = ac::cu_count();
    if (blocks > cus) blocks = cus;
    hipLaunchKernelGGL(mesh_attrs_kernel, dim3(blocks), dim3(FBLOCK), lds_bytes, (hipStream_t)stream, a, m);
    return ac::check_launch("mesh_vertex_attrs");
}

AC_API int ac_mesh_bake_texture(const ac_field *field, const float *positions, uint32_t V, const int32_t *triangles, uint32_t T, const ac_atlas_opts *atlas,
                                const ac_mesh_attr_opts *opts, float *rgb, int32_t *owner, float *normals, float *sdf, uint8_t *status, ac_stream_t stream)
{
    if (!atlas || !opts) { ac::set_error("mesh_bake_texture: NULL atlas or opts"); return AC_ERR_BAD_ARG; }
    if (opts->refine_steps < 0 || opts->refine_steps > 16 || !(opts->max_move > 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("mesh_bake_texture: refine_steps outside 0..16, or max_move, fd_eps or bound not > 0"); return AC_ERR_BAD_ARG;
    }
    const uint32_t S = atlas->size, c = atlas->cell;
    if (c < 8) { ac::set_error("mesh_bake_texture: cell %u < 8", c); return AC_ERR_BAD_ARG; }
    if (S < c || S > 32768u) { ac::set_error("mesh_bake_texture: size %u outside cell .. 32768", S); return AC_ERR_BAD_ARG; }
    const uint32_t R = S / c;
    if ((uint64_t)T > 2ull * R * R) { ac::set_error("mesh_bake_texture: %u triangles, but a %u x %u atlas of %u-texel cells holds 2 (size / cell)^2 = %llu", T, S, S, c, 2ull * R * R); return AC_ERR_BAD_ARG; }
    if (!rgb || !owner || (T && (!positions || !triangles || !V))) { ac::set_error("mesh_bake_texture: NULL buffer"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    BakeArgs m{ positions, triangles, T, S, c, R, { opts->refine_steps, opts->target_sdf, opts->tol, opts->max_move, true }, rgb, normals, sdf, owner, status };
    const size_t lds_bytes = FWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(texture_bake_kernel), lds_bytes);
    uint32_t blocks = (((S + 15) / 16) * S + FW - 1) / FW;         // persistent, one workgroup per CU, like ac_mesh_vertex_attrs
    const uint32_t cus = ac::cu_count();
    if (blocks > cus) blocks = cus;
    hipLaunchKernelGGL(texture_bake_kernel, dim3(blocks), dim3(FBLOCK), lds_bytes, (hipStream_t)stream, a, m);
    return ac::check_launch("mesh_bake_texture");
}

AC_API int ac_render_rays_surface(const ac_field *field, const ac_surface_opts *opts, const float *rays_o, const float *rays_d, uint32_t N, const float *bg,
                                  const ac_surface_out *out, ac_stream_t stream)
{
    if (!field || !opts || !out) { ac::set_error("render_rays_surface: NULL field, opts or out"); return AC_ERR_BAD_ARG; }
    if (opts->max_iters < 1 || opts->max_iters > 255) { ac::set_error("render_rays_surface: max_iters %d outside 1..255", opts->max_iters); return AC_ERR_BAD_ARG; }
    if (!(opts->tol >= 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->step_scale > 0.0f) || !(opts->min_step > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("render_rays_surface: tol not >= 0, or fd_eps, step_scale, min_step or bound not > 0"); return AC_ERR_BAD_ARG;
    }
    if (!(opts->guard >= 0.0f && opts->guard < 0.5f)) { ac::set_error("render_rays_surface: guard outside [0, 0.5)"); return AC_ERR_BAD_ARG; }
    if (N == 0) return AC_OK;
    if (!rays_o || !rays_d || !out->status) { ac::set_error("render_rays_surface: NULL rays or status"); return AC_ERR_BAD_ARG; }
    if (N > 0xffffffe0u) { ac::set_error("render_rays_surface: more than 2^32 - 32 rays"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    SurfaceArgs m{ rays_o, rays_d, bg, N, opts->max_iters, opts->level, opts->tol, opts->step_scale, opts->min_step, opts->guard,
                   out->image, out->weights_sum, out->depth, out->position, out->normal_map, out->sdf, out->status, out->iters };
    const size_t lds_bytes = FWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(surface_rays_kernel), lds_bytes);
    uint32_t blocks = ((N + 15) / 16 + FW - 1) / FW;              // persistent, one workgroup per CU, like ac_mesh_vertex_attrs
    const uint32_t cus = ac::cu_count();
    if (blocks > cus) blocks = cus;
    hipLaunchKernelGGL(surface_rays_kernel, dim3(blocks), dim3(FBLOCK), lds_bytes, (hipStream_t)stream, a, m);
    return ac::check_launch("render_rays_surface");
}

static size_t posed_state(PosedState *s, void *scratch, uint32_t N)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    char *b = static_cast<char *>(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = b ? b + o : nullptr; o += up(bytes); return p; };
    const size_t n = N;
    double *closest = reinterpret_cast<double *>(take(n * 24)), *dist2 = reinterpret_cast<double *>(take(n * 8));
    float *pts = reinterpret_cast<float *>(take(n * 12)), *can = reinterpret_cast<float *>(take(n * 12));
    int32_t *face = reinterpret_cast<int32_t *>(take(n * 4));
    float *f[6];
    for (auto &p : f) p = reinterpret_cast<float *>(take(n * 4));
    uint8_t *u[6];
    for (auto &p : u) p = reinterpret_cast<uint8_t *>(take(n));
    if (s) *s = PosedState{ pts, can, closest, dist2, face, u[0], u[1], u[2], u[3], u[4], u[5], f[0], f[1], f[2], f[3], f[4], f[5] };
    return o;
}

AC_API size_t ac_render_rays_surface_warped_scratch(uint32_t N) { return posed_state(nullptr, nullptr, N); }

AC_API int ac_render_rays_surface_warped(const ac_field *field, const ac_surface_opts *opts, float w_tol, const float *rays_o, const float *rays_d, uint32_t N,
                                         const float *bg, const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_surface_out *out,
                                         const ac_surface_warped_out *out_w, ac_stream_t stream)
{
    const char *who = "render_rays_surface_warped";
    if (!field || !opts || !out) { ac::set_error("%s: NULL field, opts or out", who); return AC_ERR_BAD_ARG; }
    if (opts->max_iters < 1 || opts->max_iters > 255) { ac::set_error("%s: max_iters %d outside 1..255", who, opts->max_iters); return AC_ERR_BAD_ARG; }
    if (!(opts->tol >= 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->step_scale > 0.0f) || !(opts->min_step > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("%s: tol not >= 0, or fd_eps, step_scale, min_step or bound not > 0", who); return AC_ERR_BAD_ARG;
    }
    if (!(opts->guard >= 0.0f && opts->guard < 0.5f)) { ac::set_error("%s: guard outside [0, 0.5)", who); return AC_ERR_BAD_ARG; }
    if (!(w_tol >= 0.0f)) { ac::set_error("%s: w_tol not >= 0", who); return AC_ERR_BAD_ARG; }
    if (!mesh || !mesh->verts || !mesh->faces || !mesh->T || mesh->F == 0) { ac::set_error("%s: NULL mesh, verts, faces or T, or a mesh without faces", who); return AC_ERR_BAD_ARG; }
    if (N == 0) return AC_OK;
    if (!rays_o || !rays_d || !out->status) { ac::set_error("%s: NULL rays or status", who); return AC_ERR_BAD_ARG; }
    if (N > 0xffffffe0u) { ac::set_error("%s: more than 2^32 - 32 rays", who); return AC_ERR_BAD_ARG; }
    const size_t need = ac_render_rays_surface_warped_scratch(N);
    if (!scratch || scratch_bytes < need) { ac::set_error("%s: scratch smaller than %zu bytes", who, need); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    PosedArgs m{ rays_o, rays_d, bg, N, opts->max_iters, opts->level, opts->tol, opts->step_scale, opts->min_step, opts->guard, w_tol,
                 sqrtf((float)mesh->threshold), {} };
    posed_state(&m.s, scratch, N);
    const PosedState &s = m.s;
    const hipStream_t st = (hipStream_t)stream;
    // the culled search where the structure covers the mesh (it skips the rays flagged in `dead`), else the exhaustive one: the same bits
    const bool culled = mesh->accel && ac_warp_accel_bytes(mesh->F) != 0;
    auto search = [&](const uint8_t *dead, double *closest, int32_t *face) {
        if (culled)
            return ac::warp_samples_accel_impl(s.pts, mesh->verts, mesh->faces, mesh->T, N, mesh->V, mesh->F, mesh->threshold, mesh->accel, nullptr, s.can, closest,
                                               s.dist2, face, s.smask, stream, 0, dead, 1);
        return ac_warp_samples(s.pts, mesh->verts, mesh->faces, mesh->T, N, mesh->V, mesh->F, mesh->threshold, nullptr, s.can, closest, s.dist2, face, s.smask, stream);
    };
    hipLaunchKernelGGL(posed_start_kernel, dim3((N + 255) / 256), dim3(256), 0, st, m, opts->bound);
    if (int rc = ac::check_launch(who)) return rc;
    uint32_t blocks = ((N + 15) / 16 + FW - 1) / FW;              // persistent, one workgroup per CU, like ac_render_rays_surface
    const uint32_t cus = ac::cu_count();
    if (blocks > cus) blocks = cus;
    const size_t trip_lds = OFF_WAVE * sizeof(float), shade_lds = FWD_LDS_FLOATS * sizeof(float);
    for (int it = 1; it <= opts->max_iters; ++it) {
        if (int rc = search(s.stopped, nullptr, nullptr)) return rc;
        hipLaunchKernelGGL(posed_trip_kernel, dim3(blocks), dim3(FBLOCK), trip_lds, st, a, m, it);
        if (int rc = ac::check_launch(who)) return rc;
    }
    if (int rc = search(s.noshade, s.closest, s.face)) return rc;
    const PosedOut po{ out->image, out->weights_sum, out->depth, out->position, out->normal_map, out->sdf, out_w ? out_w->canonical : nullptr,
                       out_w ? out_w->normal_can : nullptr, out_w ? out_w->face_id : nullptr, out->status, out->iters, mesh->verts, mesh->faces, mesh->T };
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(posed_shade_kernel), shade_lds);
    hipLaunchKernelGGL(posed_shade_kernel, dim3(blocks), dim3(FBLOCK), shade_lds, st, a, m, po);
    return ac::check_launch(who);
}

static uint32_t dp_blocks(uint32_t H)
{
    // few workgroups, several points per thread: every workgroup ends with a device-scope fence + a ticket (the mean's fixed-order reduction), and with one
    // point per thread (8403 workgroups at 129^3) those epilogues were the pass: 223 us against 65 us with 2048 workgroups
    const uint64_t n = ((uint64_t)H * H * H + DP_BLOCK - 1) / DP_BLOCK;
    const uint32_t cap = 4u * ac::cu_count();
    return (uint32_t)(n < cap ? n : cap);
}
static size_t dg_dens_offset(uint32_t H) { return (256 + (size_t)dp_blocks(H) * sizeof(double) + 255) & ~(size_t)255; }

AC_API size_t ac_density_grid_update_scratch(uint32_t H)
{
    if (H < 2 || H > 1024) return 0;
    return dg_dens_offset(H) + (size_t)H * H * H * sizeof(float);           // ticket | per-workgroup partial sums | the densities of pass 1
}

AC_API int ac_density_grid_update(const ac_field *field, const float *axis, uint32_t H, float bound, float inv_s, float decay, float *grid,
                                  double *mean_out, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (!axis || !grid || !mean_out || !scratch) { ac::set_error("density_grid_update: NULL buffer"); return AC_ERR_BAD_ARG; }
    const size_t need = ac_density_grid_update_scratch(H);
    if (!need || scratch_bytes < need) { ac::set_error("density_grid_update: H = %u unsupported or scratch of %zu bytes needed, %zu given", H, need, scratch_bytes); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = geo_args(a, field, bound)) return rc;
    float *dens = reinterpret_cast<float *>(static_cast<char *>(scratch) + dg_dens_offset(H));
    if (int rc = launch_grid(a, axis, axis, axis, H, H, H, 2, inv_s, dens, (hipStream_t)stream, "density_grid_update")) return rc;
    DgArgs g{};
    g.dens = dens; g.H = H; g.decay = decay; g.grid = grid;
    g.ticket = static_cast<uint32_t *>(scratch);
    g.partials = reinterpret_cast<double *>(static_cast<char *>(scratch) + 256);
    g.mean_out = mean_out;
    hipLaunchKernelGGL(density_pool_kernel, dim3(dp_blocks(H)), dim3(DP_BLOCK), 0, (hipStream_t)stream, g);
    return ac::check_launch("density_grid_update");
}
