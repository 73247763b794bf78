// avatarcraft_amd/csrc/mesh_components.hip -- cleaning the exported mesh on the device: connected components of a triangle mesh (ac_mesh_components),
// their sizes, and an order-preserving compaction to the components the caller keeps (ac_mesh_compact_count / _emit).  The contract is worded in
// include/avatarcraft_hip.h.  It stands in for nothing in the reference (its export writes every floater the field has).
//
// Labelling: a union-find over parent[V] in scratch -- initialise, ONE hooking launch over the triangles, flatten.  A hook always links the LARGER root under
// the SMALLER, so every value ever stored in parent[v] is <= the one before it and <= v, a root is a vertex with parent[v] == v, a vertex that stopped being
// a root never becomes one again, and the last root left in a component is its smallest vertex: the labelling is canonical (no dependence on triangle order
// or scheduling) although the hooks are atomics.  Ranks, sizes and the compaction are ordered passes (mesh_index.hpp) and integer adds: deterministic as well.
// No wave ever waits for another one: see mi::cc_find / mi::cc_unite (mesh_index.hpp, shared with mesh_repair.hip).  No floating-point atomics.
#include "mesh_index.hpp"

namespace {

enum { CC_INFO_TOTALS = 0 /* [2]: pair_scan_kernel's totals = { C, 0 } */, CC_INFO_BAD = 2 /* invalid triangles */, CC_INFO_WORDS = 64 };

__global__ __launch_bounds__(256) void cc_init_kernel(int32_t *__restrict__ parent, uint32_t V, uint32_t *__restrict__ info)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < V) parent[v] = (int32_t)v;
    if (v < CC_INFO_WORDS) info[v] = 0u;
}

// one triangle per lane: two edges join its three vertices; the third joins nothing new -- its two finds halve the paths of b and c once more, which is what
// keeps the flatten pass short when a whole wave hooked a chain in one step (a strip with descending indices)
__global__ __launch_bounds__(256) void cc_hook_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, int32_t *parent, uint32_t *info)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    const int32_t a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    if (!mi::tri_in_range(a, b, c, V)) { atomicAdd(info + CC_INFO_BAD, 1u); return; }      // (joins nothing; the compiler forms one add per wave)
    mi::cc_unite(parent, a, b);
    mi::cc_unite(parent, a, c);
    mi::cc_unite(parent, b, c);
}

// parent[] is read-only in this launch (plain loads of what the hooking launch left), root[] is another array; the walk ends because parent[x] < x off a root
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int32_t *__restrict__ parent, uint32_t V, int32_t *__restrict__ root, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sh[8];
    uint32_t n = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t v = mi::first_item() + r;
        if (v >= V) continue;
        int32_t x = (int32_t)v;
        for (;;) { const int32_t p = parent[x]; if (p == x) break; x = p; }
        root[v] = x;
        n += x == (int32_t)v ? 1u : 0u;
    }
    mi::block_totals(n, 0u, sh, bsum);                             // the roots are the low count of the pair, the high one stays 0
}

// rank of every root among the roots in ascending order -> rank[root] (the parent array, which nothing reads any more: root[] has its content), the rows of
// the size table zeroed, the two counts written
__global__ __launch_bounds__(256) void cc_rank_kernel(const int32_t *__restrict__ root, uint32_t V, const uint32_t *__restrict__ boff, int32_t *__restrict__ rank,
                                                      uint32_t *__restrict__ sizes, uint32_t max_components, const uint32_t *__restrict__ info,
                                                      uint32_t *__restrict__ counts)
{
    const uint32_t v0 = mi::first_item();
    uint32_t is_root = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
        if (v0 + r < V && root[v0 + r] == (int32_t)(v0 + r)) is_root |= 1u << r;
    mi::ordered_pass<0>(is_root, boff, [&](uint32_t v, uint32_t c) {
        rank[v] = (int32_t)c;
        if (c < max_components) { sizes[2 * (size_t)c] = 0u; sizes[2 * (size_t)c + 1] = 0u; }
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts[0] = info[CC_INFO_TOTALS]; counts[1] = info[CC_INFO_BAD]; }
}

// sizes[c][k] += 1 for every lane that has a component, aggregated in the wave first: neighbouring vertices and triangles nearly always share a component,
// and the body's counter would otherwise take every add of the mesh.  The wave peels its components off one at a time -- the first lane still waiting names a
// component, the lanes that agree are counted by a ballot and that lane adds their number once -- so a wave that agrees does ONE add, and a wave on the border
// between the body and a floater two (all-or-nothing cost 27.8 ms on a 2.2 M-triangle mesh with 25 611 components: every mixed wave sent the body's lanes to one
// word one by one).  After CC_PEEL components the lanes left add for themselves (a wave of 64 different components: debris, no word is shared anyway).
// Integer adds: the sums do not depend on the order.  Every lane of the wave calls this (ballot, shuffle); the loop is wave-uniform and waits for nobody.
constexpr int CC_PEEL = 4;
__device__ __forceinline__ void cc_wave_add(uint32_t *__restrict__ sizes, uint32_t k, int32_t c, uint32_t max_components)
{
    bool todo = c >= 0 && (uint32_t)c < max_components;
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll 1
    for (int round = 0; round < CC_PEEL; ++round) {
        const unsigned long long act = __ballot(todo);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const int32_t c0 = __shfl(c, leader);
        const bool mine = todo && c == c0;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(sizes + 2 * (size_t)c0 + k, (uint32_t)__popcll(same));
        if (mine) todo = false;
    }
    if (todo) atomicAdd(sizes + 2 * (size_t)c + k, 1u);
}

__global__ __launch_bounds__(256) void cc_sizes_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int32_t *__restrict__ root,
                                                       const int32_t *__restrict__ rank, int32_t *__restrict__ component, uint32_t *__restrict__ sizes,
                                                       uint32_t max_components)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int32_t c = -1;
    if (i < V) { c = rank[root[i]]; component[i] = c; }
    cc_wave_add(sizes, 0u, c, max_components);
    c = -1;
    if (i < T) {
        const int32_t a = tris[3 * (size_t)i], b = tris[3 * (size_t)i + 1], d = tris[3 * (size_t)i + 2];
        if (mi::tri_in_range(a, b, d, V)) c = rank[root[a]];
    }
    cc_wave_add(sizes, 1u, c, max_components);
}

// ---------------------------------------------------------------------------------------------------------------- compaction
// keep flags of a thread's four vertices (bits 0-3) and four triangles (bits 4-7): flags -> the same scans -> ordered writes, no atomics
template <bool WANT_V, bool WANT_T>
__device__ __forceinline__ uint32_t cp_flags(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int32_t *__restrict__ component,
                                             const uint8_t *__restrict__ keep, uint32_t C, uint32_t i0)
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t i = i0 + r;
        if (WANT_V && i < V) {
            const uint32_t c = (uint32_t)component[i];
            if (c < C && keep[c]) m |= 1u << r;
        }
        if (WANT_T && i < T) {
            const int32_t a = tris[3 * (size_t)i], b = tris[3 * (size_t)i + 1], d = tris[3 * (size_t)i + 2];
            if (mi::tri_in_range(a, b, d, V)) {
                const uint32_t c = (uint32_t)component[a];
                if (c < C && keep[c]) m |= 16u << r;
            }
        }
    }
    return m;
}

__global__ __launch_bounds__(256) void cp_count_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int32_t *__restrict__ component,
                                                       const uint8_t *__restrict__ keep, uint32_t C, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sh[8];
    const uint32_t m = cp_flags<true, true>(tris, T, V, component, keep, C, mi::first_item());
    mi::block_totals((uint32_t)__builtin_popcount(m & 15u), (uint32_t)__builtin_popcount(m >> 4), sh, bsum);
}

__global__ __launch_bounds__(256) void cp_vertices_kernel(uint32_t V, const int32_t *__restrict__ component, const uint8_t *__restrict__ keep, uint32_t C,
                                                          const uint32_t *__restrict__ boff, int32_t *__restrict__ vertex_map,
                                                          int32_t *__restrict__ kept_vertices, uint32_t n_kept)
{
    const uint32_t i0 = mi::first_item();
    const uint32_t m = cp_flags<true, false>(nullptr, 0u, V, component, keep, C, i0);
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
        if (i0 + r < V && !((m >> r) & 1u)) vertex_map[i0 + r] = -1;
    mi::ordered_pass<0>(m, boff, [&](uint32_t v, uint32_t o) {
        vertex_map[v] = (int32_t)o;
        if (o < n_kept) kept_vertices[o] = (int32_t)v;
    });
}

// (vertex_map is the previous launch's: read-only here)
__global__ __launch_bounds__(256) void cp_triangles_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int32_t *__restrict__ component,
                                                           const uint8_t *__restrict__ keep, uint32_t C, const uint32_t *__restrict__ boff,
                                                           const int32_t *__restrict__ vertex_map, int32_t *__restrict__ tris_out,
                                                           int32_t *__restrict__ kept_triangles, uint32_t n_kept)
{
    const uint32_t m = cp_flags<false, true>(tris, T, V, component, keep, C, mi::first_item()) >> 4;
    mi::emit_kept_triangles(m, tris, boff, [&](int32_t v) { return vertex_map[v]; }, tris_out, kept_triangles, n_kept);
}

// the labelling's scratch: the info words, parent[V], the scan's words over the vertices
struct CcScratch { uint32_t *info; int32_t *parent; mi::ScanWords scan; size_t bytes; };
CcScratch cc_scratch(void *base, uint32_t V)
{
    mi::Carver c(base);
    CcScratch s{};
    s.info = c.take<uint32_t>(CC_INFO_WORDS);
    s.parent = c.take<int32_t>(V);
    s.scan = mi::take_scan_words(c, V);
    s.bytes = c.bytes;
    return s;
}
// the compaction's: one scan's words over vertices and triangles alike
struct CpScratch { mi::ScanWords scan; size_t bytes; };
CpScratch cp_scratch(void *base, uint32_t V, uint32_t T)
{
    mi::Carver c(base);
    CpScratch s{};
    s.scan = mi::take_scan_words(c, V > T ? V : T);
    s.bytes = c.bytes;
    return s;
}

// what both compaction entries refuse, before any launch
int cp_check(const char *who, const int32_t *tris, uint32_t T, uint32_t V, const int32_t *component, const uint8_t *keep, uint32_t C, void *scratch,
             size_t scratch_bytes, CpScratch &s)
{
    if (int rc = mi::check_index_limit(who, V, T)) return rc;
    if (int rc = mi::check_some_vertex(who, V, T)) return rc;
    if (C > V) { ac::set_error("%s: C %u > V %u (a component has at least one vertex)", who, C, V); return AC_ERR_BAD_ARG; }
    if (V && (!component || !scratch || (T && !tris) || (C && !keep))) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    s = cp_scratch(scratch, V, T);
    return V ? mi::check_scratch_bytes(who, s.bytes, scratch_bytes) : AC_OK;
}

}  // namespace

AC_API size_t ac_mesh_components_scratch(uint32_t V, uint32_t T)
{
    if (!mi::index_limit_ok(V, T)) return 0;
    return cc_scratch(nullptr, V).bytes;
}

AC_API int ac_mesh_components(const int32_t *triangles, uint32_t T, uint32_t V, int32_t *root, int32_t *component, uint32_t *sizes, uint32_t max_components,
                              uint32_t *counts, void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (int rc = mi::check_index_limit("mesh_components", V, T)) return rc;
    if (int rc = mi::check_some_vertex("mesh_components", V, T)) return rc;
    if (int rc = mi::check_counts("mesh_components", counts)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {                                 // C = 0, n_bad = 0: no launch
        if (hipMemsetAsync(counts, 0, 8, st) != hipSuccess) return ac::check_launch("mesh_components");
        return AC_OK;
    }
    if (!root || !component || !scratch || (T && !triangles) || (max_components && !sizes)) { ac::set_error("mesh_components: NULL buffer"); return AC_ERR_BAD_ARG; }
    const CcScratch s = cc_scratch(scratch, V);
    if (int rc = mi::check_scratch_bytes("mesh_components", s.bytes, scratch_bytes)) return rc;
    const uint32_t items = V > T ? V : T;
    hipLaunchKernelGGL(cc_init_kernel, dim3((V + 255u) / 256u), dim3(256), 0, st, s.parent, V, s.info);
    if (T) hipLaunchKernelGGL(cc_hook_kernel, dim3((T + 255u) / 256u), dim3(256), 0, st, triangles, T, V, s.parent, s.info);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(s.scan.nblk), dim3(256), 0, st, s.parent, V, root, s.scan.bsum);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, st, s.scan.bsum, s.scan.nblk, s.scan.boff, s.info + CC_INFO_TOTALS);
    hipLaunchKernelGGL(cc_rank_kernel, dim3(s.scan.nblk), dim3(256), 0, st, root, V, s.scan.boff, s.parent, sizes, max_components, s.info, counts);
    hipLaunchKernelGGL(cc_sizes_kernel, dim3((items + 255u) / 256u), dim3(256), 0, st, triangles, T, V, root, s.parent, component, sizes, max_components);
    if (int rc = ac::check_launch("mesh_components")) return rc;
    if (max_components < V) {                     // a table that may be too short: the one case in which the call has to look at C itself
        uint32_t h[2] = { 0u, 0u };
        if (hipMemcpyAsync(h, counts, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return ac::check_launch("mesh_components");
        if (h[0] > max_components) {
            ac::set_error("mesh_components: %u components, sizes holds %u rows (max_components = V always suffices); counts, root and component are written", h[0], max_components);
            return AC_ERR_BAD_ARG;
        }
    }
    return AC_OK;
}

AC_API size_t ac_mesh_compact_scratch(uint32_t V, uint32_t T)
{
    if (!mi::index_limit_ok(V, T)) return 0;
    return cp_scratch(nullptr, V, T).bytes;
}

AC_API int ac_mesh_compact_count(const int32_t *triangles, uint32_t T, uint32_t V, const int32_t *component, const uint8_t *keep, uint32_t C, void *scratch,
                                 size_t scratch_bytes, uint32_t *counts, ac_stream_t stream)
{
    CpScratch s;
    if (int rc = cp_check("mesh_compact_count", triangles, T, V, component, keep, C, scratch, scratch_bytes, s)) return rc;
    if (int rc = mi::check_counts("mesh_compact_count", counts)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {
        if (hipMemsetAsync(counts, 0, 8, st) != hipSuccess) return ac::check_launch("mesh_compact_count");
        return AC_OK;
    }
    hipLaunchKernelGGL(cp_count_kernel, dim3(s.scan.nblk), dim3(256), 0, st, triangles, T, V, component, keep, C, s.scan.bsum);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, st, s.scan.bsum, s.scan.nblk, s.scan.boff, counts);
    return ac::check_launch("mesh_compact_count");
}

AC_API int ac_mesh_compact_emit(const int32_t *triangles, uint32_t T, uint32_t V, const int32_t *component, const uint8_t *keep, uint32_t C, void *scratch,
                                size_t scratch_bytes, int32_t *vertex_map, int32_t *kept_vertices, uint32_t n_kept_vertices, int32_t *triangles_out,
                                int32_t *kept_triangles, uint32_t n_kept_triangles, ac_stream_t stream)
{
    CpScratch s;
    if (int rc = cp_check("mesh_compact_emit", triangles, T, V, component, keep, C, scratch, scratch_bytes, s)) return rc;
    if (n_kept_vertices > V || n_kept_triangles > T) {
        ac::set_error("mesh_compact_emit: n_kept_vertices %u > V %u or n_kept_triangles %u > T %u", n_kept_vertices, V, n_kept_triangles, T);
        return AC_ERR_BAD_ARG;
    }
    if ((V && !vertex_map) || (n_kept_vertices && !kept_vertices) || (n_kept_triangles && (!triangles_out || !kept_triangles))) {
        ac::set_error("mesh_compact_emit: NULL output buffer");
        return AC_ERR_BAD_ARG;
    }
    if (V == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cp_vertices_kernel, dim3(mi::blocks(V)), dim3(256), 0, st, V, component, keep, C, s.scan.boff, vertex_map, kept_vertices, n_kept_vertices);
    if (n_kept_triangles)
        hipLaunchKernelGGL(cp_triangles_kernel, dim3(mi::blocks(T)), dim3(256), 0, st, triangles, T, V, component, keep, C, s.scan.boff, vertex_map, triangles_out,
                           kept_triangles, n_kept_triangles);
    return ac::check_launch("mesh_compact_emit");
}
