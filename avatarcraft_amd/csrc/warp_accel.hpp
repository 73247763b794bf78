// avatarcraft_amd/csrc/warp_accel.hpp -- the culling structure of the closest-face search: its format in the caller's accel buffer, and the device
// pieces that its builder (warp_accel_build.hip) and the search (warp.hip) share.  Anonymous namespace: each translation unit gets its own copy.
//
// The structure, rebuilt per frame by ac_warp_accel_build: the faces ordered along a Morton curve of their centroids (a rank sort: every face counts the
// smaller keys, over a (face block, key slice) grid), cut into tiles of TILE_F consecutive faces.  A tile has an oriented box (axis 0 = mean normal), four
// sub-boxes (groups of SUB_F consecutive faces, in the tile's frame) and one representative vertex; a face has a bounding disc.  Two axis-aligned cell grids
// lie around the body -- a fine one hugging the mesh and a coarse one for the rest of the scene.  Every cell knows, for ALL points inside it, a superset of the
// tiles that can hold their closest face (<= K of them, else the cell is marked CELL_OVERFLOW), one face near its centre (the "seed": its exact distance is
// an upper bound for any sample of the cell) and a lower bound of the distance to the mesh.  Samples without a usable cell (outside both grids, overflow)
// take the full bounding pass over all tile boxes.
// Every bound is conservative (each fp32 rounding padded to the safe side); the exact routine is Ericson's in fp64, operation for operation the oracle's
// (-ffp-contract=off, every operation rounded once).
#pragma once
#include "ac_common.hpp"
#include "mesh_blend.hpp"            // AC_DOT3

namespace {

// ---- format ----------------------------------------------------------------------------------------------------------------------------------
constexpr int TILE_F = 32;           // faces per tile (the pair encodings of the search's queues assume 32; tiles of 16 cost twice the boxes to bound)
constexpr int MAX_TILES = 16384 / TILE_F;
constexpr int NIT = MAX_TILES / 64;  // bounding-pass iterations of 64 lanes
constexpr uint32_t MAX_ACCEL_FACES = MAX_TILES * TILE_F;     // 16384
constexpr int NB = 18;               // floats of bounds per tile
constexpr int SUBS = 4, SUB_F = TILE_F / SUBS;   // sub-boxes per tile, faces per sub-box

constexpr int GRID_LEVELS = 2;
// capacity in cells: 2^15 fine cells of ~4 cm (2^17 of 2.5 cm cost 0.13 ms more per frame in the build than they saved the search), 2^16 coarse ones
constexpr uint32_t LVL_CELLS[GRID_LEVELS] = { 1u << 15, 1u << 16 };
constexpr uint32_t LVL_K[GRID_LEVELS] = { 128, 192 };                   // listed tiles per cell
constexpr uint32_t LVL_CELL0[GRID_LEVELS] = { 0, LVL_CELLS[0] };        // first cell of the level in AccelView::cell
constexpr uint32_t LVL_CTL0[GRID_LEVELS] = { 0, LVL_CELLS[0] * LVL_K[0] };   // first entry of the level in AccelView::ctl
constexpr uint32_t CTL_ENTRIES = LVL_CELLS[0] * LVL_K[0] + LVL_CELLS[1] * LVL_K[1];
constexpr uint32_t CELL_OVERFLOW = 0xffffu;      // count field of a cell without a list
// metres of grid around the mesh's bounding box.  Fine: wider than sqrt(0.05) = 0.224, the reach of the warp mask, so that every sample that can be
// unmasked lies in a fine cell
constexpr float GRID_MARGIN0 = 0.25f, GRID_MARGIN1 = 1.25f;
constexpr int HDR_WORDS = 64;
constexpr int HDR_LVL = 8, HDR_LVL_STRIDE = 12;
constexpr int HDR_BBOX = 32;                     // hdr[32..37]: vertex bounding box lo (3), hi (3)
constexpr int WORK_SLOTS = 256;                  // AccelView::work: [WORK_SLOTS][4] 64-bit work counters of the searches since the build (exact point-triangle
                                                 // tests, bounding-disc tests, sub-box tests, tile-box tests), a wave adds to slot (its index % WORK_SLOTS): spread
                                                 // over slots because ~10^5 waves adding to ONE address cost the frame 1.4 ms (measured); zeroed by the build
// hdr words: [0] tiles, [1] F, [4..7] debug counters (64-bit x 2), level l at [8 + 12 l]: grid origin (3 floats), 1 / cell size, 2 x padded half
// diagonal of a cell (float), nx, ny, nz, cells
struct AccelView {                   // pointers into the caller's accel buffer
    uint32_t *hdr;                   // [HDR_WORDS]
    uint32_t *sorted;                // [16384] face ids along the curve
    float *tri;                      // [MAX_ACCEL_FACES][9]
    int32_t *oid;                    // [MAX_ACCEL_FACES] original face id of each slot
    float *box;                      // [NB][MAX_TILES]: oriented box: axes u0 (mean normal), u1, u2 (9), lo (3), hi (3); representative vertex (3)
    float4 *sph;                     // [MAX_ACCEL_FACES][2] bounding disc of each slot's face: (centre, padded radius), (unit normal or 0, -)
    uint32_t *cell;                  // [cells of all levels] (count << 16) | seed slot; count = CELL_OVERFLOW: no list
    uint16_t *ctl;                   // [CTL_ENTRIES] the cells' candidate tiles
    float *sub;                      // [MAX_TILES * SUBS][6] lo (3), hi (3) of each group of TILE_F / SUBS consecutive faces of a tile, in the tile's frame
    float *cfar;                     // [cells of all levels] a conservative LOWER bound of dist(q, mesh)^2 over the points q of the cell
    unsigned long long *work;        // [WORK_SLOTS][4] work counters (see WORK_SLOTS)
};
constexpr int ACCEL_SEGS = 11;
__host__ __device__ inline size_t accel_offsets(size_t (&o)[ACCEL_SEGS])
{
    size_t off = 0;
    const size_t sz[ACCEL_SEGS] = { HDR_WORDS * 4, MAX_ACCEL_FACES * 4, (size_t)MAX_ACCEL_FACES * 36, (size_t)MAX_ACCEL_FACES * 4, (size_t)NB * MAX_TILES * 4,
                                    (size_t)MAX_ACCEL_FACES * 32, ((size_t)LVL_CELLS[0] + LVL_CELLS[1]) * 4, (size_t)CTL_ENTRIES * 2,
                                    (size_t)MAX_TILES * SUBS * 6 * 4, ((size_t)LVL_CELLS[0] + LVL_CELLS[1]) * 4, (size_t)WORK_SLOTS * 4 * 8 };
    for (int i = 0; i < ACCEL_SEGS; ++i) { o[i] = off; off += (sz[i] + 255) & ~(size_t)255; }
    return off;
}
__host__ __device__ inline AccelView accel_view(void *base)
{
    size_t o[ACCEL_SEGS]; accel_offsets(o);
    char *b = static_cast<char *>(base);
    AccelView v;
    v.hdr = reinterpret_cast<uint32_t *>(b + o[0]); v.sorted = reinterpret_cast<uint32_t *>(b + o[1]);
    v.tri = reinterpret_cast<float *>(b + o[2]); v.oid = reinterpret_cast<int32_t *>(b + o[3]); v.box = reinterpret_cast<float *>(b + o[4]);
    v.sph = reinterpret_cast<float4 *>(b + o[5]);
    v.cell = reinterpret_cast<uint32_t *>(b + o[6]); v.ctl = reinterpret_cast<uint16_t *>(b + o[7]); v.sub = reinterpret_cast<float *>(b + o[8]); v.cfar = reinterpret_cast<float *>(b + o[9]);
    v.work = reinterpret_cast<unsigned long long *>(b + o[10]);
    return v;
}

struct SortScratch { unsigned long long *keys; uint32_t *rank, *done; };     // the builder's sort: lives in the cfar segment until accel_cells_kernel overwrites it
__host__ __device__ inline SortScratch sort_scratch(const AccelView &av)
{
    SortScratch s;
    s.keys = reinterpret_cast<unsigned long long *>(av.cfar);
    s.rank = reinterpret_cast<uint32_t *>(s.keys + MAX_ACCEL_FACES);
    s.done = s.rank + MAX_ACCEL_FACES;
    return s;
}
static_assert(((size_t)LVL_CELLS[0] + LVL_CELLS[1]) * 4 >= (size_t)MAX_ACCEL_FACES * 12 + 4 * (MAX_ACCEL_FACES / 256), "sort scratch must fit the cfar segment");

struct GridParams { float org[3], inv, h2; uint32_t n[3], cells; };
__device__ __forceinline__ GridParams grid_params(const AccelView &av, int l)
{
    GridParams g;
    const uint32_t *h = av.hdr + HDR_LVL + HDR_LVL_STRIDE * l;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.org[k] = __builtin_bit_cast(float, h[k]); g.n[k] = h[5 + k]; }
    g.inv = __builtin_bit_cast(float, h[3]); g.h2 = __builtin_bit_cast(float, h[4]); g.cells = h[8];
    return g;
}
// cell of a point in level g, or ~0u (outside; NaN coordinates fail every comparison)
__device__ __forceinline__ uint32_t grid_cell(const GridParams &g, const float (&pf)[3])
{
    const float gx = (pf[0] - g.org[0]) * g.inv, gy = (pf[1] - g.org[1]) * g.inv, gz = (pf[2] - g.org[2]) * g.inv;
    const bool inside = g.cells != 0 && gx >= 0.0f && gy >= 0.0f && gz >= 0.0f && gx < (float)g.n[0] && gy < (float)g.n[1] && gz < (float)g.n[2];
    return inside ? ((uint32_t)gz * g.n[1] + (uint32_t)gy) * g.n[0] + (uint32_t)gx : ~0u;
}
// conservative lower bound of dist(q, mesh)^2 from the cell grids (0 when nothing is known; the coarse margin outside both grids)
__device__ __forceinline__ float grid_far_bound(const AccelView &av, const float (&pf)[3])
{
#pragma unroll
    for (int l = 0; l < GRID_LEVELS; ++l) {
        const uint32_t cell = grid_cell(grid_params(av, l), pf);
        if (cell != ~0u) return av.cfar[LVL_CELL0[l] + cell];
    }
    return av.hdr[HDR_LVL + HDR_LVL_STRIDE * (GRID_LEVELS - 1) + 8] != 0u ? GRID_MARGIN1 * GRID_MARGIN1 * (1.0f - 1e-5f) : 0.0f;
}

// ---- exact distances -------------------------------------------------------------------------------------------------------------------------
// Ericson, Real-Time Collision Detection 5.1.5 (same branch order as the oracle)
__device__ __forceinline__ void closest_pt_tri(const double (&p)[3], const double (&a)[3], const double (&b)[3], const double (&c)[3],
                                               double (&out)[3])
{
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { ab[i] = b[i] - a[i]; ac[i] = c[i] - a[i]; ap[i] = p[i] - a[i]; }
    const double d1 = AC_DOT3(ab, ap), d2 = AC_DOT3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
#pragma unroll
    for (int i = 0; i < 3; i++) bp[i] = p[i] - b[i];
    const double d3 = AC_DOT3(ab, bp), d4 = AC_DOT3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int i = 0; i < 3; i++) out[i] = a[i] + v * ab[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) cp[i] = p[i] - c[i];
    const double d5 = AC_DOT3(ab, cp), d6 = AC_DOT3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int i = 0; i < 3; i++) out[i] = a[i] + w * ac[i];
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int i = 0; i < 3; i++) out[i] = b[i] + w * (c[i] - b[i]);
        return;
    }
    const double denom = 1.0 / (va + vb + vc), v = vb * denom, w = vc * denom;
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = a[i] + ab[i] * v + ac[i] * w;
}

__device__ __forceinline__ double dist2_pts(const double (&p)[3], const double (&q)[3])
{
    const double ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
    return ex * ex + ey * ey + ez * ez;
}

// a face stored as nine fp32 (corner a, b, c): its closest point to p, and the squared distance (NaN for a degenerate face: 0 / 0 in an edge region)
__device__ __forceinline__ double tri_closest(const float *t, const double (&p)[3], double (&cq)[3])
{
    const double a[3] = { (double)t[0], (double)t[1], (double)t[2] }, b[3] = { (double)t[3], (double)t[4], (double)t[5] },
                 c[3] = { (double)t[6], (double)t[7], (double)t[8] };
    closest_pt_tri(p, a, b, c, cq);
    return dist2_pts(p, cq);
}

// ---- wave-wide minima ------------------------------------------------------------------------------------------------------------------------
// without LDS traffic: inclusive min scan inside every 16-lane row (DPP row_shr 1, 2, 4, 8), the rows are joined with
// row_bcast15 / row_bcast31, the total sits in lane 63 and is broadcast through an SGPR.  Lanes without a DPP source keep their own value.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_keep(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false); }
#define AC_WAVE_MIN_STEPS(STEP) STEP(0x111, 0xf) STEP(0x112, 0xf) STEP(0x114, 0xf) STEP(0x118, 0xf) STEP(0x142, 0xa) STEP(0x143, 0xc)
__device__ __forceinline__ float wave_min_f32(float v)
{
#define STEP(C, M) { const float o = __builtin_bit_cast(float, dpp_keep<C, M>(__builtin_bit_cast(int, v))); v = o < v ? o : v; }
    AC_WAVE_MIN_STEPS(STEP)
#undef STEP
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ int wave_min_i32(int v)
{
#define STEP(C, M) { const int o = dpp_keep<C, M>(v); v = o < v ? o : v; }
    AC_WAVE_MIN_STEPS(STEP)
#undef STEP
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ double lane_f64(double v, int l)        // l wave-uniform
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_min_f64(double v)
{
#define STEP(C, M) { const unsigned long long b = __builtin_bit_cast(unsigned long long, v); \
                     const unsigned lo = (unsigned)dpp_keep<C, M>((int)(unsigned)b), hi = (unsigned)dpp_keep<C, M>((int)(unsigned)(b >> 32)); \
                     const double o = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo); v = o < v ? o : v; }
    AC_WAVE_MIN_STEPS(STEP)
#undef STEP
    return lane_f64(v, 63);
}
#undef AC_WAVE_MIN_STEPS
__device__ __forceinline__ float lane_f32(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// ---- the tiles' bounds in LDS ----------------------------------------------------------------------------------------------------------------
// Two layouts.  RowMajor [NB][ntp]: lane = tile reads are conflict-free -- the structure build (accel_cells_kernel: every cell runs the full bounding
// pass).  TileMajor [ntp][NBT]: one tile's 15 numbers are four 16-byte reads for a lane that looks at ITS OWN tile -- the search, whose front end is
// lane = sample (15 scattered dword reads with 4 - 8-way bank conflicts were a third of its time: tools/warp_profile.py).
enum class BoxLayout { RowMajor, TileMajor };
typedef float f32x4w __attribute__((ext_vector_type(4)));
constexpr int NBT = 20;            // floats per tile in the tile-major layout: axes (9) | lo (3) | hi (3) | representative vertex (3) | pad (2)
template <BoxLayout L> __device__ __forceinline__ float sbox_at(const float *sbox_raw, uint32_t ntp, int row, int tl)
{
    return L == BoxLayout::TileMajor ? sbox_raw[tl * NBT + row] : sbox_raw[(uint32_t)row * ntp + (uint32_t)tl];
}
template <BoxLayout L> __device__ __forceinline__ void load_boxes(float *sbox_raw, const AccelView &av, uint32_t ntp)
{
    if (L == BoxLayout::TileMajor) {
        for (uint32_t e = threadIdx.x; e < (uint32_t)NBT * ntp; e += blockDim.x) {
            const uint32_t tl = e / NBT, r = e % NBT;
            sbox_raw[e] = r < (uint32_t)NB ? av.box[r * MAX_TILES + tl] : 0.0f;
        }
    } else {
        for (uint32_t e = threadIdx.x; e < NB * ntp; e += blockDim.x) sbox_raw[e] = av.box[(e / ntp) * MAX_TILES + e % ntp];
    }
}

// >= the fp32 rounding error of q . axis for a unit axis
__device__ __forceinline__ float query_pad(const float (&qf)[3])
{
    return 4e-7f * ((__builtin_fabsf(qf[0]) + __builtin_fabsf(qf[1])) + __builtin_fabsf(qf[2]));
}
// conservative fp32 lower bound of dist(q, box)^2 for a box [blo, bhi] in the frame `ax` (three unit axes, orthonormal up to fp32 rounding); the box
// itself is padded by its builder, every rounding here is padded to the safe side
__device__ __forceinline__ float slab_lower_bound(const float (&ax)[9], const float (&blo)[3], const float (&bhi)[3], const float (&qf)[3], float padq)
{
    float l = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sk = qf[0] * ax[3 * k] + qf[1] * ax[3 * k + 1] + qf[2] * ax[3 * k + 2];
        const float lo = blo[k] - sk, hi = sk - bhi[k];
        float d = (lo > hi ? lo : hi) - padq;
        d = d > 0.0f ? d : 0.0f;
        l += d * d;
    }
    return l * (1.0f - 1e-5f);
}
// ... of the box of tile tl (+inf for padding tiles)
template <BoxLayout L>
__device__ __forceinline__ float box_lower_bound(const float *sbox_raw, uint32_t ntp, int tl, const float (&qf)[3], float padq)
{
    float ax[9], blo[3], bhi[3];
    if (L == BoxLayout::TileMajor) {
        const f32x4w *rec = reinterpret_cast<const f32x4w *>(sbox_raw + tl * NBT);
        const f32x4w a0 = rec[0], a1 = rec[1], a2 = rec[2], a3 = rec[3];
        ax[0] = a0[0]; ax[1] = a0[1]; ax[2] = a0[2]; ax[3] = a0[3]; ax[4] = a1[0]; ax[5] = a1[1]; ax[6] = a1[2]; ax[7] = a1[3]; ax[8] = a2[0];
        blo[0] = a2[1]; blo[1] = a2[2]; blo[2] = a2[3]; bhi[0] = a3[0]; bhi[1] = a3[1]; bhi[2] = a3[2];
    } else {
#pragma unroll
        for (int r = 0; r < 9; ++r) ax[r] = sbox_at<L>(sbox_raw, ntp, r, tl);
#pragma unroll
        for (int k = 0; k < 3; ++k) { blo[k] = sbox_at<L>(sbox_raw, ntp, 9 + k, tl); bhi[k] = sbox_at<L>(sbox_raw, ntp, 12 + k, tl); }
    }
    return slab_lower_bound(ax, blo, bhi, qf, padq);
}

// The full bounding pass for a point q, lane = tile: the lower bound of every tile (lb[]), and the two most promising tiles: tA = nearest
// representative vertex, tB = smallest lower bound
template <BoxLayout L>
__device__ __forceinline__ void bounding_pass(const float *sbox_raw, uint32_t ntp, uint32_t nit, int lane, const float (&qf)[3], float (&lb)[NIT],
                                              int &tA, int &tB)
{
    const float padq = query_pad(qf);
    float ubl = __builtin_inff();
    int tbest = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        lb[it] = __builtin_inff();
        if ((uint32_t)it >= nit) continue;                         // wave-uniform
        const int tl = it * 64 + lane;
        const float ex = qf[0] - sbox_at<L>(sbox_raw, ntp, 15, tl), ey = qf[1] - sbox_at<L>(sbox_raw, ntp, 16, tl), ez = qf[2] - sbox_at<L>(sbox_raw, ntp, 17, tl);
        const float u = (ex * ex + ey * ey + ez * ez) * (1.0f + 1e-6f);      // >= |q - representative vertex|^2
        if (u < ubl) { ubl = u; tbest = tl; }                      // padding tiles hold +inf
        lb[it] = box_lower_bound<L>(sbox_raw, ntp, tl, qf, padq);
    }
    const float ub = wave_min_f32(ubl);
    float lmin = lb[0];
    int tlow = lane;
#pragma unroll
    for (int it = 1; it < NIT; ++it) if (lb[it] < lmin) { lmin = lb[it]; tlow = it * 64 + lane; }
    const float lminw = wave_min_f32(lmin);
    tA = __builtin_amdgcn_readlane(tbest, __builtin_ctzll(__ballot(ubl == ub)));
    tB = __builtin_amdgcn_readlane(tlow, __builtin_ctzll(__ballot(lmin == lminw)));
}

// seed: the faces of tile tA (lanes 0..31) and of tile tB (lanes 32..63) through the exact routine; each lane keeps (best, bid, bc, its slot)
__device__ __forceinline__ void seed_test(const AccelView &av, const double (&q)[3], int tA, int tB, int lane, double &best, int &bid, double (&bc)[3],
                                          uint32_t &myslot)
{
    myslot = 0;
    if (lane < 2 * TILE_F) {
        const int tmine = lane < TILE_F ? tA : tB;
        const uint32_t slot = (uint32_t)tmine * TILE_F + (uint32_t)(lane & (TILE_F - 1));
        myslot = slot;
        double cq[3];
        const double d2 = tri_closest(av.tri + (size_t)slot * 9, q, cq);
        // same acceptance rule as everywhere else: a degenerate face yields NaN and is never accepted -- an unconditional assignment would poison
        // this lane's running minimum for the rest of the sample
        if (d2 < best) { best = d2; bid = av.oid[slot]; bc[0] = cq[0]; bc[1] = cq[1]; bc[2] = cq[2]; }
    }
}

}  // namespace
