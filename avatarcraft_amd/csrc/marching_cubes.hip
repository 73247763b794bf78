// avatarcraft_amd/csrc/marching_cubes.hip -- marching cubes on the device: ac_marching_cubes_count / _emit turn a volume u (the mesh export's -sdf of
// ac_field_sdf_grid, or any other [nx][ny][nz] floats) into the mesh PyMCubes' marching_cubes(u, threshold) would give extract_geometry
// (models/instant_nsr.py:747-764): classify -> scan -> emit, shared-edge vertex indexing, no atomics: a deterministic mesh.  No field code is involved.
//
// Marching cubes: the 256-case table is GENERATED from the algorithm's definition (tools/gen_mc_table.py -> ac_mc_table.hpp): corner flagged <=> u <= iso
// (PyMCubes' convention), one vertex per sign-changing grid edge at the linear zero crossing (formed in double like PyMCubes: it evaluates its float32
// input in double), ambiguous faces always cut off the flagged corners (a rule of the face's own 4 flags: watertight by construction), triangles oriented
// with the normal towards u <= iso = out of the body for u = -sdf.  PyMCubes is not in this image: "unpinned vs PyMCubes, pinned vs the definition".
// Order of the output (what makes the mesh reproducible bit for bit, and equal to the CPU oracle's serial loop): vertices by owning grid point (linear
// index, z fastest) then by axis x, y, z; triangles by cell (linear index) then by table position.
#include "mesh_index.hpp"   // the ordered passes (a workgroup's pair of totals = its vertices and its triangles), the scratch walk, the shared refusals

#define AC_MC_CONST static __constant__ const
#include "ac_mc_table.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------- marching cubes
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

__global__ __launch_bounds__(256) void mc_classify_kernel(const uint32_t *__restrict__ bits, const McDims d, uint32_t *__restrict__ cnt4,
                                                          uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sh[8];
    const uint32_t p0 = mi::first_item();             // (a thread's four consecutive points: their four count bytes are one dword)
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
    mi::block_totals(nv, nt, sh, bsum);            // 1024 points: at most 3072 vertices / 5120 triangles per workgroup
}

struct McXform { double den, span[3], lo[3]; };   // world = index / den * span + lo, the reference's three operations in its order (instant_nsr.py:760-762)

// A window of a larger grid (ac_marching_cubes_slab_*): layers [x0, x0 + d.nx) along x.  The scan of the count pass runs over the whole window, so a vertex
// has a window-local index; the count pass leaves in info[MC_INFO_SHIFT] the local index of the first vertex the window emits.  Global index = local -
// shift + vertex_base (the carried layer 0 gets the indices just below vertex_base: the ones the previous window wrote them under); position in this
// window's piece = local - shift.  Emitted: vertices of layers [vlo, vhi), triangles of cell layers [0, tlayers).
struct McSlab { uint32_t x0, vertex_base, vlo, vhi, tlayers; const uint32_t *info; };
enum { MC_INFO_TOTALS = 0 /* [2]: pair_scan_kernel's totals over the window */, MC_INFO_SHIFT = 2, MC_INFO_WORDS = 64 };

template <bool SLAB>
__device__ __forceinline__ void mc_vertices_body(const float *__restrict__ vol, const McDims d, float iso, const uint32_t *__restrict__ cnt4,
                                                 const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, uint32_t *__restrict__ voff,
                                                 const McXform &xf, double *__restrict__ verts, uint32_t n_verts, const McSlab &s)
{
    __shared__ uint32_t sh[8];
    if (mi::block_total<0>(bsum) == 0u) return;
    const uint32_t shift = SLAB ? s.info[MC_INFO_SHIFT] : 0u;
    const uint32_t p0 = mi::first_item();
    const uint32_t packed = p0 < d.npts ? cnt4[p0 >> 2] : 0u;
    uint32_t nv = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) nv += (uint32_t)__builtin_popcount((packed >> (8 * r)) & 7u);
    uint32_t vid = mi::ordered_base<0>(nv, boff, sh);
    const uint32_t stride[3] = { d.ny * d.nz, d.nz, 1u };
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t m = (packed >> (8 * r)) & 7u;
        if (!m) continue;
        const uint32_t p = p0 + r;
        voff[p] = SLAB ? vid - shift + s.vertex_base : vid;
        const uint32_t k = p % d.nz, t = p / d.nz, j = t % d.ny, i = t / d.ny;
        if (SLAB && (i < s.vlo || i >= s.vhi)) { vid += (uint32_t)__builtin_popcount(m); continue; }      // a carried or an incomplete layer: indexed, not written
        const double va = (double)vol[p];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((m >> a) & 1u)) continue;
            const double vb = (double)vol[p + stride[a]];
            const double tt = ((double)iso - va) / (vb - va);            // the linear zero crossing between the two grid points, 0 <= tt <= 1
            double c[3] = { (double)(SLAB ? s.x0 + i : i), (double)j, (double)k };
            c[a] += tt;
            const uint32_t o = vid - shift;
            if (o < n_verts) {
                verts[3 * (size_t)o] = c[0] / xf.den * xf.span[0] + xf.lo[0];
                verts[3 * (size_t)o + 1] = c[1] / xf.den * xf.span[1] + xf.lo[1];
                verts[3 * (size_t)o + 2] = c[2] / xf.den * xf.span[2] + xf.lo[2];
            }
            ++vid;
        }
    }
}
__global__ __launch_bounds__(256) void mc_vertices_kernel(const float *__restrict__ vol, const McDims d, float iso, const uint32_t *__restrict__ cnt4,
                                                          const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, uint32_t *__restrict__ voff,
                                                          const McXform xf, double *__restrict__ verts, uint32_t n_verts)
{
    mc_vertices_body<false>(vol, d, iso, cnt4, bsum, boff, voff, xf, verts, n_verts, McSlab{});
}
__global__ __launch_bounds__(256) void mc_slab_vertices_kernel(const float *__restrict__ vol, const McDims d, float iso, const uint32_t *__restrict__ cnt4,
                                                               const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, uint32_t *__restrict__ voff,
                                                               const McXform xf, double *__restrict__ verts, uint32_t n_verts, const McSlab s)
{
    mc_vertices_body<true>(vol, d, iso, cnt4, bsum, boff, voff, xf, verts, n_verts, s);
}

// (tlayers: triangles of cell layers [0, tlayers) only.  They come first in the scan's order, so their indices are the piece's; voff holds global indices.)
template <bool SLAB>
__device__ __forceinline__ void mc_triangles_body(const uint32_t *__restrict__ bits, const McDims d, const uint32_t *__restrict__ cnt4,
                                                  const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ voff,
                                                  int32_t *__restrict__ tris, uint32_t n_tris, uint32_t tlayers)
{
    __shared__ uint32_t sh[8];
    if (mi::block_total<1>(bsum) == 0u) return;
    if (SLAB && (uint64_t)blockIdx.x * mi::ITEMS >= (uint64_t)tlayers * d.ny * d.nz) return;
    const uint32_t p0 = mi::first_item();
    const uint32_t packed = p0 < d.npts ? cnt4[p0 >> 2] : 0u;
    uint32_t nt = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) nt += (packed >> (8 * r + 3)) & 7u;
    uint32_t tid = mi::ordered_base<1>(nt, boff, sh);
    const uint8_t *cnt8 = reinterpret_cast<const uint8_t *>(cnt4);
    const uint32_t sx = d.ny * d.nz, sy = d.nz;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t n = (packed >> (8 * r + 3)) & 7u;
        if (!n) continue;
        const uint32_t p = p0 + r;
        if (SLAB && p / sx >= tlayers) continue;     // (the last ones of the order: nothing after them needs tid)
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
__global__ __launch_bounds__(256) void mc_triangles_kernel(const uint32_t *__restrict__ bits, const McDims d, const uint32_t *__restrict__ cnt4,
                                                           const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ voff,
                                                           int32_t *__restrict__ tris, uint32_t n_tris)
{
    mc_triangles_body<false>(bits, d, cnt4, bsum, boff, voff, tris, n_tris, d.nx);
}
__global__ __launch_bounds__(256) void mc_slab_triangles_kernel(const uint32_t *__restrict__ bits, const McDims d, const uint32_t *__restrict__ cnt4,
                                                                const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ voff,
                                                                int32_t *__restrict__ tris, uint32_t n_tris, uint32_t tlayers)
{
    mc_triangles_body<true>(bits, d, cnt4, bsum, boff, voff, tris, n_tris, tlayers);
}

// What a window emits, from the count bytes and the scan of the whole window: the scan's exclusive prefix (vertices low, triangles high word of a pair) at the
// first point of four layers.  One workgroup; a prefix = the offset of the point's workgroup + the count bytes before the point in it.
__device__ __forceinline__ void mc_prefix_at(const uint32_t *__restrict__ cnt4, const uint32_t *__restrict__ boff, const McDims d, uint32_t layer,
                                             const uint32_t *__restrict__ totals, uint32_t *sh, uint32_t &pv, uint32_t &pt)
{
    if (layer >= d.nx) { pv = totals[0]; pt = totals[1]; return; }                     // (uniform over the workgroup)
    const uint32_t p = layer * d.ny * d.nz, blk = p / mi::ITEMS, q0 = blk * mi::ITEMS + threadIdx.x * 4u;
    const uint32_t packed = q0 < p ? cnt4[q0 >> 2] : 0u;                                // (q0 < p < npts: a dword mc_classify_kernel wrote)
    uint32_t nv = 0, nt = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t c = q0 + r < p ? (packed >> (8 * r)) & 0xffu : 0u;
        nv += (uint32_t)__builtin_popcount(c & 7u); nt += c >> 3;
    }
    const mi::Pair before = mi::block_totals(nv, nt, sh);
    pv = mi::block_offset<0>(boff, blk) + before.lo; pt = mi::block_offset<1>(boff, blk) + before.hi;
}
__global__ __launch_bounds__(256) void mc_slab_counts_kernel(const uint32_t *__restrict__ cnt4, const uint32_t *__restrict__ boff, const McDims d, uint32_t vlo,
                                                             uint32_t vhi, uint32_t tlayers, uint32_t *__restrict__ info, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t sh[8];
    uint32_t v_lo, v_one, v_top, v_hi, t_hi, unused;
    mc_prefix_at(cnt4, boff, d, vlo, info + MC_INFO_TOTALS, sh, v_lo, unused);
    mc_prefix_at(cnt4, boff, d, 1u, info + MC_INFO_TOTALS, sh, v_one, unused);
    mc_prefix_at(cnt4, boff, d, vhi - 1u, info + MC_INFO_TOTALS, sh, v_top, unused);
    mc_prefix_at(cnt4, boff, d, vhi, info + MC_INFO_TOTALS, sh, v_hi, unused);
    mc_prefix_at(cnt4, boff, d, tlayers, info + MC_INFO_TOTALS, sh, unused, t_hi);
    if (threadIdx.x == 0) {
        info[MC_INFO_SHIFT] = v_lo;
        counts[0] = v_hi - v_lo; counts[1] = t_hi; counts[2] = v_one; counts[3] = v_hi - v_top;
    }
}

// The scratch of an nx x ny x nz grid or window: count bytes (padded to whole workgroups), a vertex offset per point, the scans' words, the flag bits; a
// window's info words come last, so a window runs in the dense scratch of its size plus those.
struct McScratch { uint32_t *cnt4, *voff; mi::ScanWords scan; unsigned long long *bits64; uint32_t *info; size_t bytes; };
McScratch mc_scratch(void *base, uint32_t nx, uint32_t ny, uint32_t nz, bool slab)
{
    mi::Carver c(base);
    McScratch s{};
    const uint64_t npts = (uint64_t)nx * ny * nz;
    const size_t nblk = mi::blocks(npts);
    s.cnt4 = c.take<uint32_t>(nblk * (mi::ITEMS / 4));
    s.voff = c.take<uint32_t>((size_t)npts);
    s.scan = mi::take_scan_words(c, npts);
    s.bits64 = c.take<unsigned long long>(nblk * (mi::ITEMS / 64) + 2);
    if (slab) s.info = c.take<uint32_t>(MC_INFO_WORDS);
    s.bytes = c.bytes;
    return s;
}
const uint32_t *mc_bits(const McScratch &s) { return reinterpret_cast<const uint32_t *>(s.bits64); }      // (the classification reads the flag words by halves)

bool mc_grid_ok(uint32_t nx, uint32_t ny, uint32_t nz) { return nx >= 2 && ny >= 2 && nz >= 2 && (uint64_t)nx * ny * nz < (1ull << 31); }

int mc_check(const char *who, const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, void *scratch, size_t scratch_bytes, McDims &d, McScratch &s)
{
    if (!vol || !scratch) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    if (!mc_grid_ok(nx, ny, nz)) { ac::set_error("%s: grid %u x %u x %u unsupported (2 <= n, fewer than 2^31 points)", who, nx, ny, nz); return AC_ERR_BAD_ARG; }
    d = McDims{ nx, ny, nz, nx * ny * nz };
    s = mc_scratch(scratch, nx, ny, nz, false);
    return mi::check_scratch_bytes(who, s.bytes, scratch_bytes);
}

struct McSlabPlan { McScratch s; McDims d; uint32_t vlo, vhi, tlayers; };
int mc_slab_check(const char *who, const float *window, uint32_t n, uint32_t ny, uint32_t nz, uint32_t first, uint32_t last, void *scratch, size_t scratch_bytes,
                  McSlabPlan &p)
{
    if (!window || !scratch) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    if (!mc_grid_ok(n, ny, nz) || (n == 2 && !(first && last))) {
        ac::set_error("%s: window %u x %u x %u unsupported (3 <= n, or n = 2 for a window both first and last; 2 <= ny, nz; fewer than 2^31 points)", who, n, ny, nz);
        return AC_ERR_BAD_ARG;
    }
    p.d = McDims{ n, ny, nz, n * ny * nz };
    p.s = mc_scratch(scratch, n, ny, nz, true);
    p.vlo = first ? 0u : 1u; p.vhi = last ? n : n - 1u; p.tlayers = last ? n : n - 2u;
    return mi::check_scratch_bytes(who, p.s.bytes, scratch_bytes);
}

// flags -> count bytes and the workgroups' totals -> their scan; totals[0..1] = the vertices and triangles of the whole grid or window
void mc_count_launches(const float *vol, const McDims &d, float iso, const McScratch &s, uint32_t *totals, hipStream_t st)
{
    const uint32_t nchunks = (d.npts + 1023u) >> 10;
    uint32_t blocks = (nchunks + 3u) / 4u;
    const uint32_t cap = 32u * ac::cu_count();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(mc_flags_kernel, dim3(blocks), dim3(256), 0, st, vol, d.npts, iso, s.bits64);
    hipLaunchKernelGGL(mc_classify_kernel, dim3(s.scan.nblk), dim3(256), 0, st, mc_bits(s), d, s.cnt4, s.scan.bsum);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, st, s.scan.bsum, s.scan.nblk, s.scan.boff, totals);
}

// what both emit entries refuse about their outputs and the transform, then the transform
int mc_xform(const char *who, double den, const double span[3], const double lo[3], const double *vertices, uint32_t n_vertices, const int32_t *triangles,
             uint32_t n_triangles, McXform &xf)
{
    if ((n_vertices && !vertices) || (n_triangles && !triangles) || !span || !lo || !(den != 0.0)) { ac::set_error("%s: NULL buffer or den == 0", who); return AC_ERR_BAD_ARG; }
    xf = McXform{ den, { span[0], span[1], span[2] }, { lo[0], lo[1], lo[2] } };
    return AC_OK;
}

}  // namespace

AC_API size_t ac_marching_cubes_slab_scratch(uint32_t n, uint32_t ny, uint32_t nz)
{
    if (n < 3 || !mc_grid_ok(n, ny, nz)) return 0;     // (n = 2, the whole of a two-layer grid, runs in the scratch of any larger window)
    return mc_scratch(nullptr, n, ny, nz, true).bytes;
}

AC_API int ac_marching_cubes_slab_count(const float *window, uint32_t n, uint32_t ny, uint32_t nz, float iso, uint32_t first, uint32_t last, void *scratch,
                                        size_t scratch_bytes, uint32_t *counts, ac_stream_t stream)
{
    McSlabPlan p;
    if (int rc = mc_slab_check("marching_cubes_slab_count", window, n, ny, nz, first, last, scratch, scratch_bytes, p)) return rc;
    if (int rc = mi::check_counts("marching_cubes_slab_count", counts)) return rc;
    mc_count_launches(window, p.d, iso, p.s, p.s.info + MC_INFO_TOTALS, (hipStream_t)stream);
    hipLaunchKernelGGL(mc_slab_counts_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p.s.cnt4, p.s.scan.boff, p.d, p.vlo, p.vhi, p.tlayers, p.s.info, counts);
    return ac::check_launch("marching_cubes_slab_count");
}

AC_API int ac_marching_cubes_slab_emit(const float *window, uint32_t n, uint32_t ny, uint32_t nz, float iso, uint32_t first, uint32_t last, void *scratch,
                                       size_t scratch_bytes, uint32_t x0, uint32_t vertex_base, double den, const double span[3], const double lo[3],
                                       double *vertices, uint32_t n_vertices, int32_t *triangles, uint32_t n_triangles, ac_stream_t stream)
{
    McSlabPlan p; McXform xf;
    if (int rc = mc_slab_check("marching_cubes_slab_emit", window, n, ny, nz, first, last, scratch, scratch_bytes, p)) return rc;
    if (int rc = mc_xform("marching_cubes_slab_emit", den, span, lo, vertices, n_vertices, triangles, n_triangles, xf)) return rc;
    if ((uint64_t)x0 + n > 0xffffffffull || (first && x0 != 0u)) { ac::set_error("marching_cubes_slab_emit: x0 %u + n %u overflows 32 bits, or a first window with x0 != 0", x0, n); return AC_ERR_BAD_ARG; }
    const McScratch &s = p.s;
    const McSlab sl{ x0, vertex_base, p.vlo, p.vhi, p.tlayers, s.info };
    if (n_vertices || n_triangles)                // (triangles of cell layer 0 may use carried vertices only: their indices are formed by this pass all the same)
        hipLaunchKernelGGL(mc_slab_vertices_kernel, dim3(s.scan.nblk), dim3(256), 0, (hipStream_t)stream, window, p.d, iso, s.cnt4, s.scan.bsum, s.scan.boff, s.voff, xf,
                           vertices, n_vertices, sl);
    if (n_triangles)
        hipLaunchKernelGGL(mc_slab_triangles_kernel, dim3(s.scan.nblk), dim3(256), 0, (hipStream_t)stream, mc_bits(s), p.d, s.cnt4, s.scan.bsum, s.scan.boff, s.voff,
                           triangles, n_triangles, p.tlayers);
    return ac::check_launch("marching_cubes_slab_emit");
}

AC_API size_t ac_marching_cubes_scratch(uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (!mc_grid_ok(nx, ny, nz)) return 0;
    return mc_scratch(nullptr, nx, ny, nz, false).bytes;
}

AC_API int ac_marching_cubes_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *scratch, size_t scratch_bytes,
                                   uint32_t *counts, ac_stream_t stream)
{
    McDims d; McScratch s;
    if (int rc = mc_check("marching_cubes_count", volume, nx, ny, nz, scratch, scratch_bytes, d, s)) return rc;
    if (int rc = mi::check_counts("marching_cubes_count", counts)) return rc;
    mc_count_launches(volume, d, iso, s, counts, (hipStream_t)stream);
    return ac::check_launch("marching_cubes_count");
}

AC_API int ac_marching_cubes_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *scratch, size_t scratch_bytes,
                                  double den, const double span[3], const double lo[3], double *vertices, uint32_t n_vertices, int32_t *triangles,
                                  uint32_t n_triangles, ac_stream_t stream)
{
    McDims d; McScratch s; McXform xf;
    if (int rc = mc_check("marching_cubes_emit", volume, nx, ny, nz, scratch, scratch_bytes, d, s)) return rc;
    if (int rc = mc_xform("marching_cubes_emit", den, span, lo, vertices, n_vertices, triangles, n_triangles, xf)) return rc;
    if (n_vertices)
        hipLaunchKernelGGL(mc_vertices_kernel, dim3(s.scan.nblk), dim3(256), 0, (hipStream_t)stream, volume, d, iso, s.cnt4, s.scan.bsum, s.scan.boff, s.voff, xf,
                           vertices, n_vertices);
    if (n_triangles)
        hipLaunchKernelGGL(mc_triangles_kernel, dim3(s.scan.nblk), dim3(256), 0, (hipStream_t)stream, mc_bits(s), d, s.cnt4, s.scan.bsum, s.scan.boff, s.voff,
                           triangles, n_triangles);
    return ac::check_launch("marching_cubes_emit");
}
