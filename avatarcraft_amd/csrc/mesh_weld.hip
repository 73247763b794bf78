// avatarcraft_amd/csrc/mesh_weld.hip -- welding the decimated mesh on the device (ac_mesh_weld_count / _emit): duplicate triangles are merged, back-to-back pairs
// cancel, the vertices nobody names any more are dropped -- and the topology report of a triangle list (ac_mesh_topology): distinct, boundary, non-manifold and
// misoriented edges.  The contract is worded in include/avatarcraft_hip.h.  It stands in for nothing in the reference (its export writes every marching-cubes
// triangle).  Index buffers only: no vertex positions are read.
//
// Weld: the triangles with the same SET of corners form a group, found through an open-addressing table in scratch.  The set needs 93 bits, so a slot holds a
// triangle INDEX, claimed with a 32-bit compare-exchange from "empty" under linear probing, and two triangles are compared by reading the occupant's corners from
// the immutable input: see mw_slot.  A slot holds the smallest member index of either sign (integer atomic mins) and the two member counts (integer atomic adds).
// Which member of a group claimed the slot depends on scheduling; nothing that is written out does: the kept member is named by the mins and the counts alone.
// Topology: the 64-bit key table of mesh_cluster.hip (mi::key_slot), keyed by the edge (min << 31) | max, two use counters per slot.
// After its filling launch a table is read-only; flags -> the ordered passes of mesh_index.hpp -> ordered writes.  No wave ever waits for another one, no
// floating-point atomics, counters are aggregated in the wave and added as integers: every output is a function of the input alone.
#include "mesh_index.hpp"

namespace {

constexpr int32_t MW_EMPTY = -1;                  // no occupant: a triangle index is >= 0
enum { MW_INVALID = 0, MW_DEGENERATE = 1, MW_CANCELLED = 2, MW_REPEATED = 3, MW_EXCESS = 4,          // the weld's info words
       MT_EDGES = 0, MT_BOUNDARY = 1, MT_NONMANIFOLD = 2, MT_MISORIENTED = 3, MT_REFERENCED = 4, MT_FACES = 5, MT_INVALID = 6, MT_DEGENERATE = 7,      // the report's
       MW_INFO_WORDS = 64 };
enum { MW_TRI_INVALID = 0, MW_TRI_DEGENERATE = 1, MW_TRI_MEMBER = 2 };

// a triangle as the definitions see it: its corners as they stand, its sorted triple (the group's name) and its sign -- rotated so that the smallest corner
// comes first, (a, b, c), it is + iff b < c
struct MwTri { int32_t v[3]; int32_t lo, mid, hi; bool plus; };

__device__ __forceinline__ int mw_read(const int32_t *__restrict__ tris, uint32_t t, uint32_t V, MwTri &k)
{
    const int32_t a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    k.v[0] = a; k.v[1] = b; k.v[2] = c;
    if (!mi::tri_in_range(a, b, c, V)) return MW_TRI_INVALID;
    if (a == b || b == c || a == c) return MW_TRI_DEGENERATE;
    int32_t s, p, q;                              // the rotation with the smallest corner first
    if (a < b && a < c) { s = a; p = b; q = c; }
    else if (b < c) { s = b; p = c; q = a; }
    else { s = c; p = a; q = b; }
    k.lo = s; k.plus = p < q; k.mid = p < q ? p : q; k.hi = p < q ? q : p;
    return MW_TRI_MEMBER;
}

// ---------------------------------------------------------------------------------------------------------------- weld
struct MwTable { int32_t *occ, *min_plus, *min_minus; uint32_t *n_plus, *n_minus; };

// The slot of triangle t's group, claiming one if the group has none.  A lock-free probe, no wait: a slot's occupant changes once, from MW_EMPTY to a triangle
// index, and never again.  A trip reads the occupant or wins the compare-exchange; if the exchange FAILED it returns what the slot holds now -- a triangle, for
// good.  That triangle's corners are read from the input, which nobody writes: it names this group (the walk ends) or another (the walk moves on).  Every slot
// is looked at once: the table has capacity >= 2 T slots and at most T groups, so an empty slot or the group's own comes up within `capacity` trips whatever
// other waves do and whether or not they run at all.  (occupants are members: valid and not degenerate, so mw_read fills the triple.)
__device__ __forceinline__ uint64_t mw_slot(int32_t *occ, uint64_t mask, const int32_t *__restrict__ tris, uint32_t V, uint32_t t, const MwTri &k)
{
    uint64_t s = mi::key_mix(((uint64_t)(uint32_t)k.lo << 31 | (uint64_t)(uint32_t)k.mid) ^ mi::key_mix((uint64_t)(uint32_t)k.hi)) & mask;
    for (;;) {
        int32_t seen = __hip_atomic_load((mi::gi32 *)(occ + s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == MW_EMPTY &&
            __hip_atomic_compare_exchange_strong((mi::gi32 *)(occ + s), &seen, (int32_t)t, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return s;
        MwTri o;
        (void)mw_read(tris, (uint32_t)seen, V, o);
        if (o.lo == k.lo && o.mid == k.mid && o.hi == k.hi) return s;
        s = (s + 1u) & mask;
    }
}

__global__ __launch_bounds__(256) void mw_init_kernel(MwTable tb, uint64_t capacity, uint8_t *__restrict__ vmark, uint32_t V, uint32_t *__restrict__ info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s < capacity) { tb.occ[s] = MW_EMPTY; tb.min_plus[s] = 0x7fffffff; tb.min_minus[s] = 0x7fffffff; tb.n_plus[s] = 0u; tb.n_minus[s] = 0u; }
    if (s < V) vmark[s] = 0;
    if (s < MW_INFO_WORDS) info[s] = 0u;
}

// one triangle per lane: its group's slot, then one integer min and one integer add on the side of its sign
__global__ __launch_bounds__(256) void mw_fill_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, MwTable tb, uint64_t mask, uint32_t *__restrict__ tslot)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    MwTri k;
    if (mw_read(tris, t, V, k) != MW_TRI_MEMBER) return;
    const uint64_t s = mw_slot(tb.occ, mask, tris, V, t, k);
    tslot[t] = (uint32_t)s;
    (void)__hip_atomic_fetch_min((mi::gi32 *)((k.plus ? tb.min_plus : tb.min_minus) + s), (int32_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add((mi::gu32 *)((k.plus ? tb.n_plus : tb.n_minus) + s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (the table is the filling launch's: read-only from here on)  One triangle per lane: kept iff its group does not cancel and it is the smallest member of the
// majority sign; a kept triangle marks its corners (plain stores of the same value).  The five counts, aggregated in the wave.
__global__ __launch_bounds__(256) void mw_mark_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, MwTable tb, const uint32_t *__restrict__ tslot,
                                                      uint8_t *__restrict__ tkeep, uint8_t *__restrict__ vmark, uint32_t *info)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t n[5] = { 0u, 0u, 0u, 0u, 0u };
    if (t < T) {
        MwTri k;
        const int cls = mw_read(tris, t, V, k);
        bool kept = false;
        if (cls == MW_TRI_MEMBER) {
            const uint32_t s = tslot[t];
            const uint32_t np = tb.n_plus[s], nm = tb.n_minus[s];
            if (np == nm) n[MW_CANCELLED] = 1u;
            else {
                kept = (np > nm ? tb.min_plus[s] : tb.min_minus[s]) == (int32_t)t;
                if (kept) n[MW_EXCESS] = (np > nm ? np - nm : nm - np) - 1u;
                else n[MW_REPEATED] = 1u;
            }
        } else n[cls == MW_TRI_INVALID ? MW_INVALID : MW_DEGENERATE] = 1u;
        tkeep[t] = kept ? 1 : 0;
        if (kept) { vmark[k.v[0]] = 1; vmark[k.v[1]] = 1; vmark[k.v[2]] = 1; }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) mi::wave_add(info + i, n[i]);
}

// kept vertices among a thread's four vertices (bits 0-3), kept triangles among its four triangles (bits 4-7)
template <bool WANT_V, bool WANT_T>
__device__ __forceinline__ uint32_t mw_flags(const uint8_t *__restrict__ vmark, uint32_t V, const uint8_t *__restrict__ tkeep, uint32_t T, uint32_t i0)
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t i = i0 + r;
        if (WANT_V && i < V && vmark[i]) m |= 1u << r;
        if (WANT_T && i < T && tkeep[i]) m |= 16u << r;
    }
    return m;
}

__global__ __launch_bounds__(256) void mw_count_kernel(const uint8_t *__restrict__ vmark, uint32_t V, const uint8_t *__restrict__ tkeep, uint32_t T,
                                                       uint32_t *__restrict__ bsum, const uint32_t *__restrict__ info, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t sh[8];
    const uint32_t m = mw_flags<true, true>(vmark, V, tkeep, T, mi::first_item());
    mi::block_totals((uint32_t)__builtin_popcount(m & 15u), (uint32_t)__builtin_popcount(m >> 4), sh, bsum);
    if (blockIdx.x == 0 && threadIdx.x < 6u) counts[2u + threadIdx.x] = threadIdx.x < 5u ? info[threadIdx.x] : 0u;      // (the scan writes counts[0..1])
}

__global__ __launch_bounds__(256) void mw_vertices_kernel(const uint8_t *__restrict__ vmark, uint32_t V, const uint32_t *__restrict__ boff,
                                                          int32_t *__restrict__ vertex_map, int32_t *__restrict__ kept_vertices, uint32_t n_kept)
{
    const uint32_t i0 = mi::first_item();
    const uint32_t m = mw_flags<true, false>(vmark, V, nullptr, 0u, i0);
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
        if (i0 + r < V && !((m >> r) & 1u)) vertex_map[i0 + r] = -1;
    mi::ordered_pass<0>(m, boff, [&](uint32_t v, uint32_t o) {
        vertex_map[v] = (int32_t)o;
        if (o < n_kept) kept_vertices[o] = (int32_t)v;
    });
}

// (vertex_map is the previous launch's: read-only here)
__global__ __launch_bounds__(256) void mw_triangles_kernel(const int32_t *__restrict__ tris, uint32_t T, const uint8_t *__restrict__ tkeep,
                                                           const uint32_t *__restrict__ boff, const int32_t *__restrict__ vertex_map,
                                                           int32_t *__restrict__ tris_out, int32_t *__restrict__ kept_triangles, uint32_t n_kept)
{
    const uint32_t m = mw_flags<false, true>(nullptr, 0u, tkeep, T, mi::first_item()) >> 4;
    mi::emit_kept_triangles(m, tris, boff, [&](int32_t v) { return vertex_map[v]; }, tris_out, kept_triangles, n_kept);
}

// the scratch: the info words, the table (`capacity` slots, a power of two >= 2 T: never more than half full), a slot and a flag per triangle, a mark per
// vertex, the scan's words over vertices and triangles alike
struct MwScratch { uint32_t *info; MwTable tb; uint32_t *tslot; uint8_t *tkeep, *vmark; mi::ScanWords scan; uint64_t capacity; size_t bytes; };
MwScratch mw_scratch(void *base, uint32_t V, uint32_t T)
{
    mi::Carver c(base);
    MwScratch s{};
    s.capacity = 2;
    while (s.capacity < 2 * (uint64_t)T) s.capacity <<= 1;
    s.info = c.take<uint32_t>(MW_INFO_WORDS);
    s.tb.occ = c.take<int32_t>((size_t)s.capacity);
    s.tb.min_plus = c.take<int32_t>((size_t)s.capacity);
    s.tb.min_minus = c.take<int32_t>((size_t)s.capacity);
    s.tb.n_plus = c.take<uint32_t>((size_t)s.capacity);
    s.tb.n_minus = c.take<uint32_t>((size_t)s.capacity);
    s.tslot = c.take<uint32_t>(T);
    s.tkeep = c.take<uint8_t>(T);
    s.vmark = c.take<uint8_t>(V);
    s.scan = mi::take_scan_words(c, V > T ? V : T);
    s.bytes = c.bytes;
    return s;
}

// what the weld entries and the report refuse alike, before any launch
int mw_check_head(const char *who, const int32_t *tris, uint32_t T, uint32_t V, void *scratch)
{
    if (int rc = mi::check_index_limit(who, V, T)) return rc;
    if (int rc = mi::check_some_vertex(who, V, T)) return rc;
    if ((T && !tris) || (V && !scratch)) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    return AC_OK;
}
int mw_check(const char *who, const int32_t *tris, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, MwScratch &s)
{
    if (int rc = mw_check_head(who, tris, T, V, scratch)) return rc;
    s = mw_scratch(scratch, V, T);
    return V ? mi::check_scratch_bytes(who, s.bytes, scratch_bytes) : AC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- topology
struct MtTable { uint64_t *keys; uint32_t *fwd, *bwd; };

__global__ __launch_bounds__(256) void mt_init_kernel(MtTable tb, uint64_t capacity, uint8_t *__restrict__ vmark, uint32_t V, uint32_t *__restrict__ info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s < capacity) { tb.keys[s] = mi::KEY_EMPTY; tb.fwd[s] = 0u; tb.bwd[s] = 0u; }
    if (s < V) vmark[s] = 0;
    if (s < MW_INFO_WORDS) info[s] = 0u;
}

// one triangle per lane: its three edges u -> v, each one use of the slot of (min << 31) | max in its direction; its corners are referenced
__global__ __launch_bounds__(256) void mt_fill_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, MtTable tb, uint64_t mask, uint8_t *__restrict__ vmark,
                                                      uint32_t *info)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    int cls = -1;
    if (t < T) {
        MwTri k;
        cls = mw_read(tris, t, V, k);
        if (cls == MW_TRI_MEMBER) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int32_t u = k.v[e], v = k.v[(e + 1) % 3];
                const uint64_t key = u < v ? ((uint64_t)(uint32_t)u << 31) | (uint32_t)v : ((uint64_t)(uint32_t)v << 31) | (uint32_t)u;
                const uint64_t s = mi::key_slot(tb.keys, mask, key);
                (void)__hip_atomic_fetch_add((mi::gu32 *)((u < v ? tb.fwd : tb.bwd) + s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                vmark[u] = 1;
            }
        }
    }
    mi::wave_add(info + MT_FACES, cls == MW_TRI_MEMBER ? 1u : 0u);
    mi::wave_add(info + MT_INVALID, cls == MW_TRI_INVALID ? 1u : 0u);
    mi::wave_add(info + MT_DEGENERATE, cls == MW_TRI_DEGENERATE ? 1u : 0u);
}

// (the table and the marks are the filling launch's: read-only here)  One slot and one vertex per lane -> the five sums, aggregated in the wave
__global__ __launch_bounds__(256) void mt_reduce_kernel(MtTable tb, uint64_t capacity, const uint8_t *__restrict__ vmark, uint32_t V, uint32_t *info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t edge = 0, boundary = 0, nonmanifold = 0, misoriented = 0;
    if (s < capacity && tb.keys[s] != mi::KEY_EMPTY) {
        const uint32_t f = tb.fwd[s], b = tb.bwd[s], n = f + b;
        edge = 1u; boundary = n == 1u; nonmanifold = n > 2u; misoriented = n == 2u && f != b;
    }
    mi::wave_add(info + MT_EDGES, edge);
    mi::wave_add(info + MT_BOUNDARY, boundary);
    mi::wave_add(info + MT_NONMANIFOLD, nonmanifold);
    mi::wave_add(info + MT_MISORIENTED, misoriented);
    mi::wave_add(info + MT_REFERENCED, s < V && vmark[s] ? 1u : 0u);
}

__global__ __launch_bounds__(64) void mt_counts_kernel(const uint32_t *__restrict__ info, uint32_t *__restrict__ counts)
{
    if (threadIdx.x < 8u) counts[threadIdx.x] = info[threadIdx.x];
}

// the scratch: the info words, the edge table (`capacity` slots, a power of two >= 6 T -- a triangle has three edges: never more than half full), a mark per vertex
struct MtScratch { uint32_t *info; MtTable tb; uint8_t *vmark; uint64_t capacity; size_t bytes; };
MtScratch mt_scratch(void *base, uint32_t V, uint32_t T)
{
    mi::Carver c(base);
    MtScratch s{};
    s.capacity = 2;
    while (s.capacity < 6 * (uint64_t)T) s.capacity <<= 1;
    s.info = c.take<uint32_t>(MW_INFO_WORDS);
    s.tb.keys = c.take<uint64_t>((size_t)s.capacity);
    s.tb.fwd = c.take<uint32_t>((size_t)s.capacity);
    s.tb.bwd = c.take<uint32_t>((size_t)s.capacity);
    s.vmark = c.take<uint8_t>(V);
    s.bytes = c.bytes;
    return s;
}

}  // namespace

AC_API size_t ac_mesh_weld_scratch(uint32_t V, uint32_t T)
{
    if (!mi::index_limit_ok(V, T)) return 0;
    return mw_scratch(nullptr, V, T).bytes;
}

AC_API int ac_mesh_weld_count(const int32_t *triangles, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, uint32_t *counts, ac_stream_t stream)
{
    MwScratch s;
    if (int rc = mw_check("mesh_weld_count", triangles, T, V, scratch, scratch_bytes, s)) return rc;
    if (int rc = mi::check_counts("mesh_weld_count", counts)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {                                 // (then T == 0) nothing to weld: no launch
        if (hipMemsetAsync(counts, 0, 32, st) != hipSuccess) return ac::check_launch("mesh_weld_count");
        return AC_OK;
    }
    const uint64_t cells = s.capacity > V ? s.capacity : V;
    hipLaunchKernelGGL(mw_init_kernel, dim3((uint32_t)((cells + 255u) / 256u)), dim3(256), 0, st, s.tb, s.capacity, s.vmark, V, s.info);
    if (T) {
        hipLaunchKernelGGL(mw_fill_kernel, dim3((T + 255u) / 256u), dim3(256), 0, st, triangles, T, V, s.tb, s.capacity - 1u, s.tslot);
        hipLaunchKernelGGL(mw_mark_kernel, dim3((T + 255u) / 256u), dim3(256), 0, st, triangles, T, V, s.tb, s.tslot, s.tkeep, s.vmark, s.info);
    }
    hipLaunchKernelGGL(mw_count_kernel, dim3(s.scan.nblk), dim3(256), 0, st, s.vmark, V, s.tkeep, T, s.scan.bsum, s.info, counts);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, st, s.scan.bsum, s.scan.nblk, s.scan.boff, counts);
    return ac::check_launch("mesh_weld_count");
}

AC_API int ac_mesh_weld_emit(const int32_t *triangles, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, int32_t *vertex_map, int32_t *kept_vertices,
                             uint32_t n_kept_vertices, int32_t *triangles_out, int32_t *kept_triangles, uint32_t n_kept_triangles, ac_stream_t stream)
{
    MwScratch s;
    if (int rc = mw_check("mesh_weld_emit", triangles, T, V, scratch, scratch_bytes, s)) return rc;
    if (n_kept_vertices > V || n_kept_triangles > T) {
        ac::set_error("mesh_weld_emit: n_kept_vertices %u > V %u or n_kept_triangles %u > T %u", n_kept_vertices, V, n_kept_triangles, T);
        return AC_ERR_BAD_ARG;
    }
    if ((V && !vertex_map) || (n_kept_vertices && !kept_vertices) || (n_kept_triangles && (!triangles_out || !kept_triangles))) {
        ac::set_error("mesh_weld_emit: NULL output buffer");
        return AC_ERR_BAD_ARG;
    }
    if (V == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mw_vertices_kernel, dim3(mi::blocks(V)), dim3(256), 0, st, s.vmark, V, s.scan.boff, vertex_map, kept_vertices, n_kept_vertices);
    if (n_kept_triangles)
        hipLaunchKernelGGL(mw_triangles_kernel, dim3(mi::blocks(T)), dim3(256), 0, st, triangles, T, s.tkeep, s.scan.boff, vertex_map, triangles_out, kept_triangles,
                           n_kept_triangles);
    return ac::check_launch("mesh_weld_emit");
}

AC_API size_t ac_mesh_topology_scratch(uint32_t V, uint32_t T)
{
    if (!mi::index_limit_ok(V, T)) return 0;
    return mt_scratch(nullptr, V, T).bytes;
}

AC_API int ac_mesh_topology(const int32_t *triangles, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, uint32_t *counts, ac_stream_t stream)
{
    if (int rc = mw_check_head("mesh_topology", triangles, T, V, scratch)) return rc;
    const MtScratch s = mt_scratch(scratch, V, T);
    if (V) if (int rc = mi::check_scratch_bytes("mesh_topology", s.bytes, scratch_bytes)) return rc;
    if (int rc = mi::check_counts("mesh_topology", counts)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {                                 // (then T == 0) nothing to report: no launch
        if (hipMemsetAsync(counts, 0, 32, st) != hipSuccess) return ac::check_launch("mesh_topology");
        return AC_OK;
    }
    const uint64_t cells = s.capacity > V ? s.capacity : V;
    const uint32_t nblk = (uint32_t)((cells + 255u) / 256u);
    hipLaunchKernelGGL(mt_init_kernel, dim3(nblk), dim3(256), 0, st, s.tb, s.capacity, s.vmark, V, s.info);
    if (T) hipLaunchKernelGGL(mt_fill_kernel, dim3((T + 255u) / 256u), dim3(256), 0, st, triangles, T, V, s.tb, s.capacity - 1u, s.vmark, s.info);
    hipLaunchKernelGGL(mt_reduce_kernel, dim3(nblk), dim3(256), 0, st, s.tb, s.capacity, s.vmark, V, s.info);
    hipLaunchKernelGGL(mt_counts_kernel, dim3(1), dim3(64), 0, st, s.info, counts);
    return ac::check_launch("mesh_topology");
}
