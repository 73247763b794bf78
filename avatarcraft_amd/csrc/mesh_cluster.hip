// avatarcraft_amd/csrc/mesh_cluster.hip -- decimating the exported mesh on the device by vertex clustering on a grid (ac_mesh_cluster_count / _emit).  The contract
// is worded in include/avatarcraft_hip.h.  It stands in for nothing in the reference (its export writes every marching-cubes triangle).
//
// The vertices of one grid cell merge.  A cell is found through an open-addressing table in scratch: slots keyed by the 64-bit cell key, claimed with a 64-bit
// compare-exchange under linear probing; a slot holds the smallest member index (integer atomic min), the member count and three int64 sums of the members'
// fixed-point offsets inside the cell (integer atomic adds); every vertex remembers its slot.  A cell's leader is its smallest member, clusters are numbered by
// ascending leader (flags -> the ordered passes of mesh_index.hpp), and the position is a function of the exact integer sums: nothing depends on scheduling or on
// the hash, although the table is filled with atomics.  No wave ever waits for another one: see mi::key_slot (mesh_index.hpp).  No floating-point atomics.
#include "mesh_index.hpp"

namespace {

constexpr uint32_t MCL_MAX_N = 1u << 21;          // cells per axis: three of them fit a 63-bit key
enum { MCL_INFO_BAD_V = 0, MCL_INFO_BAD_T = 1, MCL_INFO_WORDS = 64 };

struct MclGrid { double lo[3], h; uint32_t n[3]; };

// a vertex in the grid, per axis (the header's definitions, in their order): t = (v - lo) / h; valid iff 0 <= t < n + 1 (a NaN or an infinity fails the
// comparisons); c = min(floor(t), n - 1); q = floor((t - c) 2^30), 0 <= q < 2^31
__device__ __forceinline__ bool mcl_cell(const double *__restrict__ p, const MclGrid &g, uint64_t &key, uint32_t q[3])
{
    uint64_t c3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double t = (p[a] - g.lo[a]) / g.h;
        if (!(t >= 0.0 && t < (double)(g.n[a] + 1u))) return false;
        const double fl = floor(t), top = (double)(g.n[a] - 1u);
        const double c = fl < top ? fl : top;
        const double f = t - c;
        c3[a] = (uint64_t)c;
        q[a] = (uint32_t)(int64_t)floor(f * 1073741824.0);
    }
    key = (c3[0] * g.n[1] + c3[1]) * g.n[2] + c3[2];
    return true;
}

struct MclTable { uint64_t *keys; int32_t *lead; uint32_t *cnt; uint64_t *sums; int32_t *rank; };

__global__ __launch_bounds__(256) void mcl_init_kernel(MclTable tb, uint64_t capacity, uint32_t *__restrict__ info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s < capacity) {
        tb.keys[s] = mi::KEY_EMPTY; tb.lead[s] = 0x7fffffff; tb.cnt[s] = 0u;
        tb.sums[3 * s] = 0ull; tb.sums[3 * s + 1] = 0ull; tb.sums[3 * s + 2] = 0ull;
    }
    if (s < MCL_INFO_WORDS) info[s] = 0u;
}

// one vertex per lane: its cell's slot, then four integer adds and one integer min on it (sums of non-negative q below 2^31: 2^31 members stay below 2^62)
__global__ __launch_bounds__(256) void mcl_fill_kernel(const double *__restrict__ verts, uint32_t V, MclGrid g, MclTable tb, uint64_t mask, int64_t *__restrict__ slot,
                                                       uint32_t *info)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    uint64_t key; uint32_t q[3];
    if (!mcl_cell(verts + 3 * (size_t)v, g, key, q)) { slot[v] = -1; atomicAdd(info + MCL_INFO_BAD_V, 1u); return; }
    const uint64_t s = mi::key_slot(tb.keys, mask, key);
    slot[v] = (int64_t)s;
    (void)__hip_atomic_fetch_min((mi::gi32 *)(tb.lead + s), (int32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add((mi::gu32 *)(tb.cnt + s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int a = 0; a < 3; ++a) (void)__hip_atomic_fetch_add((mi::gu64 *)(tb.sums + 3 * s + a), (uint64_t)q[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (the table is the filling launch's: read-only from here on)
__device__ __forceinline__ bool mcl_is_leader(const int64_t *__restrict__ slot, const int32_t *__restrict__ lead, uint32_t v)
{
    const int64_t s = slot[v];
    return s >= 0 && lead[s] == (int32_t)v;
}

// a triangle's three slots, -1 if it is invalid (an index outside [0, V) or an invalid vertex).  Two vertices share a cluster iff they share a slot.
__device__ __forceinline__ bool mcl_tri_slots(const int32_t *__restrict__ tris, uint32_t t, uint32_t V, const int64_t *__restrict__ slot, int64_t s[3])
{
    const int32_t i[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
    if (!mi::tri_in_range(i[0], i[1], i[2], V)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = slot[i[k]];
    return s[0] >= 0 && s[1] >= 0 && s[2] >= 0;
}
__device__ __forceinline__ bool mcl_survives(const int64_t s[3]) { return s[0] != s[1] && s[1] != s[2] && s[0] != s[2]; }

// leaders among a thread's four vertices (bits 0-3), surviving triangles among its four triangles (bits 4-7), invalid triangles (bits 8-11)
template <bool WANT_V, bool WANT_T>
__device__ __forceinline__ uint32_t mcl_flags(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int64_t *__restrict__ slot,
                                              const int32_t *__restrict__ lead, uint32_t i0)
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t i = i0 + r;
        if (WANT_V && i < V && mcl_is_leader(slot, lead, i)) m |= 1u << r;
        if (WANT_T && i < T) {
            int64_t s[3];
            if (!mcl_tri_slots(tris, i, V, slot, s)) m |= 256u << r;
            else if (mcl_survives(s)) m |= 16u << r;
        }
    }
    return m;
}

__global__ __launch_bounds__(256) void mcl_count_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int64_t *__restrict__ slot,
                                                        const int32_t *__restrict__ lead, uint32_t *__restrict__ bsum, uint32_t *info)
{
    __shared__ uint32_t sh[8];
    const uint32_t m = mcl_flags<true, true>(tris, T, V, slot, lead, mi::first_item());
    mi::block_totals((uint32_t)__builtin_popcount(m & 15u), (uint32_t)__builtin_popcount((m >> 4) & 15u), sh, bsum);
    const uint32_t bad = (uint32_t)__builtin_popcount(m >> 8);
    if (bad) atomicAdd(info + MCL_INFO_BAD_T, bad);
}

// rank of every leader among the leaders in ascending order -> rank[its slot]; the two counts the scan does not write
__global__ __launch_bounds__(256) void mcl_rank_kernel(uint32_t V, const int64_t *__restrict__ slot, const int32_t *__restrict__ lead, const uint32_t *__restrict__ boff,
                                                       int32_t *__restrict__ rank, const uint32_t *__restrict__ info, uint32_t *__restrict__ counts)
{
    const uint32_t m = mcl_flags<true, false>(nullptr, 0u, V, slot, lead, mi::first_item());
    mi::ordered_pass<0>(m, boff, [&](uint32_t v, uint32_t c) { rank[slot[v]] = (int32_t)c; });
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts[2] = info[MCL_INFO_BAD_V]; counts[3] = info[MCL_INFO_BAD_T]; }
}

__global__ __launch_bounds__(256) void mcl_cluster_kernel(uint32_t V, const int64_t *__restrict__ slot, const int32_t *__restrict__ rank, int32_t *__restrict__ cluster)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    const int64_t s = slot[v];
    cluster[v] = s >= 0 ? rank[s] : -1;
}

// one lane per vertex; a leader writes its cluster's row.  positions = lo + (c + S / (members 2^30)) h per axis, in that order, in fp64 (no contraction: the
// build's -ffp-contract=off); the cell index c comes back out of the key
__global__ __launch_bounds__(256) void mcl_emit_clusters_kernel(uint32_t V, MclGrid g, MclTable tb, const int64_t *__restrict__ slot, int32_t *__restrict__ leader,
                                                                uint32_t *__restrict__ members, double *__restrict__ positions, uint32_t n_clusters)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V || !mcl_is_leader(slot, tb.lead, v)) return;
    const int64_t s = slot[v];
    const uint32_t c = (uint32_t)tb.rank[s];
    if (c >= n_clusters) return;
    const uint32_t n = tb.cnt[s];
    const uint64_t key = tb.keys[s];
    const uint64_t cz = key % g.n[2], cxy = key / g.n[2];
    const uint64_t cell[3] = { cxy / g.n[1], cxy % g.n[1], cz };
    leader[c] = (int32_t)v;
    members[c] = n;
    const double den = (double)n * 1073741824.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mean = (double)(int64_t)tb.sums[3 * s + a] / den;
        const double u = (double)cell[a] + mean;
        const double w = u * g.h;
        positions[3 * (size_t)c + a] = g.lo[a] + w;
    }
}

__global__ __launch_bounds__(256) void mcl_emit_triangles_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int64_t *__restrict__ slot,
                                                                 const int32_t *__restrict__ rank, const uint32_t *__restrict__ boff, int32_t *__restrict__ tris_out,
                                                                 int32_t *__restrict__ kept_triangles, uint32_t n_kept)
{
    const uint32_t m = mcl_flags<false, true>(tris, T, V, slot, nullptr, mi::first_item()) >> 4;
    mi::emit_kept_triangles(m, tris, boff, [&](int32_t v) { return rank[slot[v]]; }, tris_out, kept_triangles, n_kept);
}

// the scratch: the info words, the table (`capacity` slots, a power of two >= 2 V: never more than half full), a slot per vertex, the scan's words over
// vertices and triangles alike
struct MclScratch { uint32_t *info; MclTable tb; int64_t *slot; mi::ScanWords scan; uint64_t capacity; size_t bytes; };
MclScratch mcl_scratch(void *base, uint32_t V, uint32_t T)
{
    mi::Carver c(base);
    MclScratch s{};
    s.capacity = 2;
    while (s.capacity < 2 * (uint64_t)V) s.capacity <<= 1;
    s.info = c.take<uint32_t>(MCL_INFO_WORDS);
    s.tb.keys = c.take<uint64_t>((size_t)s.capacity);
    s.tb.sums = c.take<uint64_t>(3 * (size_t)s.capacity);
    s.tb.lead = c.take<int32_t>((size_t)s.capacity);
    s.tb.cnt = c.take<uint32_t>((size_t)s.capacity);
    s.tb.rank = c.take<int32_t>((size_t)s.capacity);
    s.slot = c.take<int64_t>(V);
    s.scan = mi::take_scan_words(c, V > T ? V : T);
    s.bytes = c.bytes;
    return s;
}

// what both entries refuse, before any launch
int mcl_check(const char *who, const double *verts, uint32_t V, const int32_t *tris, uint32_t T, const ac_cluster_grid *grid, void *scratch, size_t scratch_bytes,
              MclScratch &s, MclGrid &g)
{
    if (int rc = mi::check_index_limit(who, V, T)) return rc;
    if (!grid) { ac::set_error("%s: NULL grid", who); return AC_ERR_BAD_ARG; }
    if (!(grid->h > 0.0) || !isfinite(grid->h)) { ac::set_error("%s: cell edge h %g must be finite and > 0", who, grid->h); return AC_ERR_BAD_ARG; }
    for (int a = 0; a < 3; ++a) {
        if (grid->n[a] < 1u || grid->n[a] > MCL_MAX_N) { ac::set_error("%s: n[%d] %u outside [1, 2^21] cells", who, a, grid->n[a]); return AC_ERR_BAD_ARG; }
        g.lo[a] = grid->lo[a]; g.n[a] = grid->n[a];
    }
    g.h = grid->h;
    if ((V && !verts) || (T && !tris) || ((V || T) && !scratch)) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    s = mcl_scratch(scratch, V, T);
    return V || T ? mi::check_scratch_bytes(who, s.bytes, scratch_bytes) : AC_OK;
}

}  // namespace

AC_API size_t ac_mesh_cluster_scratch(uint32_t V, uint32_t T)
{
    if (!mi::index_limit_ok(V, T)) return 0;
    return mcl_scratch(nullptr, V, T).bytes;
}

AC_API int ac_mesh_cluster_count(const double *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const ac_cluster_grid *grid, void *scratch,
                                 size_t scratch_bytes, int32_t *cluster, uint32_t *counts, ac_stream_t stream)
{
    MclScratch s; MclGrid g;
    if (int rc = mcl_check("mesh_cluster_count", vertices, V, triangles, T, grid, scratch, scratch_bytes, s, g)) return rc;
    if (int rc = mi::check_counts("mesh_cluster_count", counts)) return rc;
    if (V && !cluster) { ac::set_error("mesh_cluster_count: NULL cluster"); return AC_ERR_BAD_ARG; }
    hipStream_t st = (hipStream_t)stream;
    if (V == 0 && T == 0) {                       // nothing to cluster: no launch
        if (hipMemsetAsync(counts, 0, 16, st) != hipSuccess) return ac::check_launch("mesh_cluster_count");
        return AC_OK;
    }
    hipLaunchKernelGGL(mcl_init_kernel, dim3((uint32_t)((s.capacity + 255u) / 256u)), dim3(256), 0, st, s.tb, s.capacity, s.info);
    if (V) hipLaunchKernelGGL(mcl_fill_kernel, dim3((V + 255u) / 256u), dim3(256), 0, st, vertices, V, g, s.tb, s.capacity - 1u, s.slot, s.info);
    hipLaunchKernelGGL(mcl_count_kernel, dim3(s.scan.nblk), dim3(256), 0, st, triangles, T, V, s.slot, s.tb.lead, s.scan.bsum, s.info);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, st, s.scan.bsum, s.scan.nblk, s.scan.boff, counts);
    hipLaunchKernelGGL(mcl_rank_kernel, dim3(s.scan.nblk), dim3(256), 0, st, V, s.slot, s.tb.lead, s.scan.boff, s.tb.rank, s.info, counts);
    if (V) hipLaunchKernelGGL(mcl_cluster_kernel, dim3((V + 255u) / 256u), dim3(256), 0, st, V, s.slot, s.tb.rank, cluster);
    return ac::check_launch("mesh_cluster_count");
}

AC_API int ac_mesh_cluster_emit(const double *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const ac_cluster_grid *grid, void *scratch,
                                size_t scratch_bytes, int32_t *leader, uint32_t *members, double *positions, uint32_t n_clusters, int32_t *triangles_out,
                                int32_t *kept_triangles, uint32_t n_kept_triangles, ac_stream_t stream)
{
    MclScratch s; MclGrid g;
    if (int rc = mcl_check("mesh_cluster_emit", vertices, V, triangles, T, grid, scratch, scratch_bytes, s, g)) return rc;
    if (n_clusters > V || n_kept_triangles > T) {
        ac::set_error("mesh_cluster_emit: n_clusters %u > V %u or n_kept_triangles %u > T %u", n_clusters, V, n_kept_triangles, T);
        return AC_ERR_BAD_ARG;
    }
    if ((n_clusters && (!leader || !members || !positions)) || (n_kept_triangles && (!triangles_out || !kept_triangles))) {
        ac::set_error("mesh_cluster_emit: NULL output buffer");
        return AC_ERR_BAD_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_clusters)
        hipLaunchKernelGGL(mcl_emit_clusters_kernel, dim3((V + 255u) / 256u), dim3(256), 0, st, V, g, s.tb, s.slot, leader, members, positions, n_clusters);
    if (n_kept_triangles)
        hipLaunchKernelGGL(mcl_emit_triangles_kernel, dim3(mi::blocks(T)), dim3(256), 0, st, triangles, T, V, s.slot, s.tb.rank, s.scan.boff, triangles_out,
                           kept_triangles, n_kept_triangles);
    return ac::check_launch("mesh_cluster_emit");
}
