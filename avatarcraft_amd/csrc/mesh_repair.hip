// avatarcraft_amd/csrc/mesh_repair.hip -- making the exported mesh manifold on the device (ac_mesh_repair_count / _emit): the sheets that vertex clustering pushed
// onto one edge or one vertex are told apart again and every vertex is split into one copy per fan.  The contract -- the uses of an edge, their order around it,
// the pairing, the fans -- is worded in include/avatarcraft_hip.h.  It stands in for nothing in the reference (its export writes marching-cubes triangles as
// they are).
//
// Edge table: the 64-bit key table of mesh_index.hpp, keyed (min << 31) | max; a slot counts its uses and holds the smallest and the largest use id (integer
// atomic min / max): all an edge with two uses needs.  The slots with 3 to 8 uses -- a fraction of a percent on real meshes -- get a list of their use ids in a
// side buffer: a pass over the slots hands out the lists, a second pass over the triangles fills them through a ticket per slot.  Where a list lies and in which
// order it is filled depends on scheduling; nothing that is written out does: the lane that owns the edge orders its uses by (key, use id), a total order, in
// registers, and matches the brackets on bit masks.  Fans: the union-find of mesh_index.hpp over the 3 T corner ids, then a flatten pass, an integer atomic min of
// the root per vertex, the flags of the extra roots -> the ordered passes -> ordered writes.  No wave ever waits for another one; inside the filling, the
// ticketing and the hooking launch the shared words are touched only by agent-scope atomics on global pointers; no floating-point atomics; all fp64 arithmetic is
// plain IEEE (-ffp-contract=off, no fast-math: the division is correctly rounded), so that the keys are those of the numpy restatement bit for bit.
#include "mesh_index.hpp"

namespace {

enum { MR_TOTALS = 0 /* [2]: pair_scan_kernel's totals = { extra roots, 0 } */, MR_SPLIT = 2, MR_NONMANIFOLD = 3, MR_PAIRED = 4, MR_CUT = 5, MR_CROWDED = 6, MR_INVALID = 7,
       MR_DEGENERATE = 8, MR_LIST_TOP = 9 /* use-list words handed out */, MR_INFO_WORDS = 64 };
enum { MR_TRI_INVALID = 0, MR_TRI_DEGENERATE = 1, MR_TRI_MEMBER = 2 };
constexpr uint32_t MR_MAX_USES = 8;               // an edge with more uses is crowded: all its uses are cut
constexpr int32_t MR_NONE = 0x7fffffff;           // no use / no root yet: corner ids stay below it
constexpr uint32_t MR_PAD = 0xffffffffu;          // no use in this place of the sorting network

struct MrTable { uint64_t *keys; uint32_t *cnt; int32_t *umin, *umax; uint32_t *base; };

__device__ __forceinline__ int mr_read(const int32_t *__restrict__ tris, uint32_t t, uint32_t V, int32_t v[3])
{
    v[0] = tris[3 * (size_t)t]; v[1] = tris[3 * (size_t)t + 1]; v[2] = tris[3 * (size_t)t + 2];
    if (!mi::tri_in_range(v[0], v[1], v[2], V)) return MR_TRI_INVALID;
    if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) return MR_TRI_DEGENERATE;
    return MR_TRI_MEMBER;
}
__device__ __forceinline__ uint64_t mr_key(int32_t p, int32_t q)
{
    return p < q ? ((uint64_t)(uint32_t)p << 31) | (uint32_t)q : ((uint64_t)(uint32_t)q << 31) | (uint32_t)p;
}
__device__ __forceinline__ bool mr_listed(uint32_t n) { return n >= 3u && n <= MR_MAX_USES; }

__global__ __launch_bounds__(256) void mr_init_kernel(MrTable tb, uint64_t capacity, int32_t *__restrict__ parent, uint32_t corners, int32_t *__restrict__ first,
                                                      uint32_t *__restrict__ vsplit, uint32_t V, uint32_t *__restrict__ info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s < capacity) { tb.keys[s] = mi::KEY_EMPTY; tb.cnt[s] = 0u; tb.umin[s] = MR_NONE; tb.umax[s] = -1; tb.base[s] = 0u; }
    if (s < corners) parent[s] = (int32_t)s;
    if (s < V) { first[s] = MR_NONE; vsplit[s] = 0u; }
    if (s < MR_INFO_WORDS) info[s] = 0u;
}

// one triangle per lane: its three sides, each one use of the slot of its edge -- one integer add, one min and one max of the use id 3 t + k
__global__ __launch_bounds__(256) void mr_fill_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, MrTable tb, uint64_t mask, uint32_t *info)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    int cls = -1;
    if (t < T) {
        int32_t v[3];
        cls = mr_read(tris, t, V, v);
        if (cls == MR_TRI_MEMBER) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint64_t s = mi::key_slot(tb.keys, mask, mr_key(v[k], v[(k + 1) % 3]));
                const int32_t use = (int32_t)(3u * t + (uint32_t)k);
                (void)__hip_atomic_fetch_add((mi::gu32 *)(tb.cnt + s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_min((mi::gi32 *)(tb.umin + s), use, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_max((mi::gi32 *)(tb.umax + s), use, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    mi::wave_add(info + MR_INVALID, cls == MR_TRI_INVALID ? 1u : 0u);
    mi::wave_add(info + MR_DEGENERATE, cls == MR_TRI_DEGENERATE ? 1u : 0u);
}

// (the table is the filling launch's: read-only here but for the slot's own words)  One slot per lane: a slot with 3 to 8 uses takes its list from the side
// buffer -- the lists hold at most 3 T words together -- and its largest use id, which only an edge with two uses needs, becomes its ticket counter
__global__ __launch_bounds__(256) void mr_lists_kernel(MrTable tb, uint64_t capacity, uint32_t *info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s >= capacity || tb.keys[s] == mi::KEY_EMPTY) return;
    const uint32_t n = tb.cnt[s];
    if (!mr_listed(n)) return;
    tb.base[s] = atomicAdd(info + MR_LIST_TOP, n);
    tb.umax[s] = 0;
}

// one triangle per lane: a side whose edge has a list writes its use id to the place its ticket names (the key is in the table: the probe claims nothing)
__global__ __launch_bounds__(256) void mr_tickets_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, MrTable tb, uint64_t mask, uint32_t *__restrict__ list)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    int32_t v[3];
    if (mr_read(tris, t, V, v) != MR_TRI_MEMBER) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t s = mi::key_slot(tb.keys, mask, mr_key(v[k], v[(k + 1) % 3]));
        const uint32_t n = tb.cnt[s];
        if (!mr_listed(n)) continue;
        const uint32_t ticket = (uint32_t)__hip_atomic_fetch_add((mi::gi32 *)(tb.umax + s), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket < n) list[(size_t)tb.base[s] + ticket] = 3u * t + (uint32_t)k;
    }
}

struct MrVec { double x, y, z; };
__device__ __forceinline__ MrVec mr_point(const float *__restrict__ P, int32_t v)
{
    return MrVec{ (double)P[3 * (size_t)v], (double)P[3 * (size_t)v + 1], (double)P[3 * (size_t)v + 2] };
}
__device__ __forceinline__ MrVec mr_sub(const MrVec &a, const MrVec &b) { return MrVec{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ MrVec mr_cross(const MrVec &a, const MrVec &b) { return MrVec{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double mr_dot(const MrVec &a, const MrVec &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// what a use is made of: its vertex at the start of the side, and the one opposite
__device__ __forceinline__ void mr_use(const int32_t *__restrict__ tris, uint32_t use, int32_t &from, int32_t &opposite)
{
    const uint32_t t = use / 3u, k = use - 3u * t;
    from = tris[3 * (size_t)t + k];
    opposite = tris[3 * (size_t)t + (k + 2u) % 3u];
}

// Join two uses of the edge (a, b): the two triangles' corners at a become one fan, and so do their corners at b.  code = 2 * use id + (1 if forward).
__device__ __forceinline__ void mr_join(int32_t *parent, uint32_t cx, uint32_t cy)
{
    int32_t at_a[2], at_b[2];
    const uint32_t code[2] = { cx, cy };
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t use = code[i] >> 1, t = use / 3u, k = use - 3u * t;
        const int32_t here = (int32_t)use, there = (int32_t)(3u * t + (k + 1u) % 3u);
        at_a[i] = (code[i] & 1u) ? here : there;
        at_b[i] = (code[i] & 1u) ? there : here;
    }
    mi::cc_unite(parent, at_a[0], at_a[1]);
    mi::cc_unite(parent, at_b[0], at_b[1]);
}

// a[i] by masks at constant places: the array stays in registers (the compiler turns a chain of selects back into an indexed load of a copy in LDS)
__device__ __forceinline__ uint32_t mr_pick(const uint32_t (&a)[8], int i)
{
    uint32_t r = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) r |= a[q] & (0u - (uint32_t)(q == i));
    return r;
}

// Batcher's odd-even merge sort of eight: 19 compare-exchanges at constant places, so the arrays stay in registers
__device__ __forceinline__ void mr_sort8(double (&key)[8], uint32_t (&code)[8])
{
    constexpr int net[19][2] = { { 0, 1 }, { 2, 3 }, { 4, 5 }, { 6, 7 }, { 0, 2 }, { 1, 3 }, { 4, 6 }, { 5, 7 }, { 1, 2 }, { 5, 6 },
                                 { 0, 4 }, { 1, 5 }, { 2, 6 }, { 3, 7 }, { 2, 4 }, { 3, 5 }, { 1, 2 }, { 3, 4 }, { 5, 6 } };
#pragma unroll
    for (int c = 0; c < 19; ++c) {
        const int i = net[c][0], j = net[c][1];
        const bool swap = key[i] > key[j] || (key[i] == key[j] && code[i] > code[j]);
        const double ki = key[i], kj = key[j];
        const uint32_t ci = code[i], cj = code[j];
        key[i] = swap ? kj : ki; key[j] = swap ? ki : kj;
        code[i] = swap ? cj : ci; code[j] = swap ? ci : cj;
    }
}

// (the table and the lists are earlier launches': read-only here; parent[] is touched through mi::cc_* alone)  The hooking launch, one slot per lane.  An edge
// with two uses joins them.  An edge with 3 to 8 uses orders them around itself and joins the pairs of the bracket matching; with more, or with a key that is
// not finite, it is crowded and joins nothing.  The four counts, aggregated in the wave.
__global__ __launch_bounds__(256) void mr_hook_kernel(const float *__restrict__ P, const int32_t *__restrict__ tris, MrTable tb, uint64_t capacity,
                                                      const uint32_t *__restrict__ list, int32_t *parent, uint32_t *info)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t nonmanifold = 0, paired = 0, cut = 0, crowded = 0;
    const uint64_t edge = s < capacity ? tb.keys[s] : mi::KEY_EMPTY;
    const uint32_t n = edge != mi::KEY_EMPTY ? tb.cnt[s] : 0u;
    if (n == 2u) {
        const uint32_t x = (uint32_t)tb.umin[s], y = (uint32_t)tb.umax[s];
        const int32_t a = (int32_t)(edge >> 31);
        int32_t fx, fy, o;
        mr_use(tris, x, fx, o);
        mr_use(tris, y, fy, o);
        mr_join(parent, 2u * x + (fx == a ? 1u : 0u), 2u * y + (fy == a ? 1u : 0u));
    } else if (n > 2u) {
        nonmanifold = 1u;
        bool ok = n <= MR_MAX_USES;
        double key[8];
        uint32_t code[8];
        if (ok) {
            const int32_t a = (int32_t)(edge >> 31), b = (int32_t)(edge & 0x7fffffffu);
            const MrVec pa = mr_point(P, a);
            const MrVec e = mr_sub(mr_point(P, b), pa);
            int32_t from, opposite;
            mr_use(tris, (uint32_t)tb.umin[s], from, opposite);                          // the reference use: the one of smallest id
            const MrVec w = mr_cross(e, mr_sub(mr_point(P, opposite), pa));
            const MrVec u = mr_cross(w, e);
            const size_t l0 = tb.base[s];
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                key[i] = 8.0; code[i] = MR_PAD;                                            // (behind every key: a key stays below 4)
                if (i < n) {
                    const uint32_t use = list[l0 + i];
                    mr_use(tris, use, from, opposite);
                    const MrVec d = mr_sub(mr_point(P, opposite), pa);
                    const double X = mr_dot(d, u), Y = mr_dot(d, w), sum = fabs(X) + fabs(Y);
                    double k = 0.0;
                    if (!(sum == 0.0)) {
                        const double q = Y / sum;
                        k = (X >= 0.0 && Y >= 0.0) ? q : (X < 0.0 ? 2.0 - q : 4.0 + q);
                    }
                    ok = ok && isfinite(k);
                    key[i] = k; code[i] = 2u * use + (from == a ? 1u : 0u);
                }
            }
        }
        if (!ok) { crowded = 1u; cut = n; }
        else {
            mr_sort8(key, code);
            uint32_t alive = (1u << n) - 1u, forward = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) forward |= (code[i] & 1u) << i;                  // (the pads sit behind the n uses: never alive)
#pragma unroll 1
            for (int round = 0; round < 4; ++round) {
                int bi = -1, bj = -1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t rest = alive & ~(1u << i);
                    if (bi >= 0 || !((alive >> i) & 1u) || ((forward >> i) & 1u) || !rest) continue;
                    const uint32_t above = rest & ~((2u << i) - 1u);
                    const int j = __ffs((int)(above ? above : rest)) - 1;                // the cyclic successor among the uses still in the list
                    if ((forward >> j) & 1u) { bi = i; bj = j; }
                }
                if (bi < 0) break;
                mr_join(parent, mr_pick(code, bi), mr_pick(code, bj));
                alive &= ~((1u << bi) | (1u << bj));
                paired += 2u;
            }
            cut = n - paired;
        }
    }
    mi::wave_add(info + MR_NONMANIFOLD, nonmanifold);
    mi::wave_add(info + MR_PAIRED, paired);
    mi::wave_add(info + MR_CUT, cut);
    mi::wave_add(info + MR_CROWDED, crowded);
}

// parent[] is read-only in this launch (plain loads of what the hooking launch left), root[] is another array; the walk ends because parent[x] < x off a root.
// One triangle per lane: the roots of its three corners (-1: not a member's corner), and the smallest root of every vertex by an integer atomic min
__global__ __launch_bounds__(256) void mr_flatten_kernel(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const int32_t *__restrict__ parent,
                                                         int32_t *__restrict__ root, int32_t *first)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    int32_t v[3];
    const bool member = mr_read(tris, t, V, v) == MR_TRI_MEMBER;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        int32_t x = (int32_t)(3u * t + k);
        if (member) {
            for (;;) { const int32_t p = parent[x]; if (p == x) break; x = p; }
            (void)__hip_atomic_fetch_min((mi::gi32 *)(first + v[k]), x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else x = -1;
        root[3 * (size_t)t + k] = x;
    }
}

// (root[] and first[] are the previous launch's: read-only here)  the extra roots among a thread's four corners: a root that is not its vertex's smallest one
__device__ __forceinline__ uint32_t mr_flags(const int32_t *__restrict__ tris, uint32_t corners, const int32_t *__restrict__ root, const int32_t *__restrict__ first,
                                             uint32_t c0)
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t c = c0 + r;
        if (c < corners && root[c] == (int32_t)c && first[tris[c]] != (int32_t)c) m |= 1u << r;
    }
    return m;
}

// the number of extra roots per workgroup; a vertex with an extra root is split: the first extra root to flag it counts it (an integer exchange: who comes
// first depends on scheduling, how many vertices are flagged does not)
__global__ __launch_bounds__(256) void mr_count_kernel(const int32_t *__restrict__ tris, uint32_t corners, const int32_t *__restrict__ root,
                                                       const int32_t *__restrict__ first, uint32_t *vsplit, uint32_t *__restrict__ bsum, uint32_t *info)
{
    __shared__ uint32_t sh[8];
    const uint32_t c0 = mi::first_item();
    const uint32_t m = mr_flags(tris, corners, root, first, c0);
    uint32_t split = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
        if ((m >> r) & 1u)
            split += __hip_atomic_exchange((mi::gu32 *)(vsplit + tris[c0 + r]), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u ? 1u : 0u;
    mi::block_totals((uint32_t)__builtin_popcount(m), 0u, sh, bsum);
    mi::wave_add(info + MR_SPLIT, split);
}

__global__ __launch_bounds__(64) void mr_counts_kernel(const uint32_t *__restrict__ info, uint32_t V, uint32_t *__restrict__ counts)
{
    if (threadIdx.x == 0) counts[0] = V + info[MR_TOTALS];
    else if (threadIdx.x < 8u) counts[threadIdx.x] = info[MR_SPLIT + threadIdx.x - 1u];
}

// rank of every extra root among the extra roots in ascending order -> rank[root] (the parent array, which nothing reads any more: root[] has its content),
// source[V + rank] = the vertex it is a copy of; source[v] = v for the vertices that were there
__global__ __launch_bounds__(256) void mr_rank_kernel(const int32_t *__restrict__ tris, uint32_t corners, const int32_t *__restrict__ root, const int32_t *__restrict__ first,
                                                      const uint32_t *__restrict__ boff, uint32_t V, int32_t *__restrict__ rank, int32_t *__restrict__ source,
                                                      uint32_t n_vertices)
{
    const uint32_t c0 = mi::first_item();
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
        if (c0 + r < V && c0 + r < n_vertices) source[c0 + r] = (int32_t)(c0 + r);
    mi::ordered_pass<0>(mr_flags(tris, corners, root, first, c0), boff, [&](uint32_t c, uint32_t o) {
        rank[c] = (int32_t)o;
        if (o < n_vertices - V) source[(size_t)V + o] = tris[c];
    });
}

// (rank[] is the previous launch's: read-only here)  One corner per lane: a member's corner is rewritten to its fan's index, any other is copied
__global__ __launch_bounds__(256) void mr_triangles_kernel(const int32_t *__restrict__ tris, uint32_t corners, const int32_t *__restrict__ root,
                                                           const int32_t *__restrict__ first, const int32_t *__restrict__ rank, uint32_t V, int32_t *__restrict__ tris_out)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= corners) return;
    const int32_t v = tris[c], r = root[c];
    tris_out[c] = (r < 0 || first[v] == r) ? v : (int32_t)(V + (uint32_t)rank[r]);
}

// the scratch: the info words, the edge table (`capacity` slots, a power of two >= 6 T -- a triangle has three edges: never more than half full), the use lists
// (at most 3 T words), parent and root per corner, the smallest root and the split flag per vertex, the scan's words over corners and vertices alike
struct MrScratch { uint32_t *info; MrTable tb; uint32_t *list; int32_t *parent, *root, *first; uint32_t *vsplit; mi::ScanWords scan; uint64_t capacity; size_t bytes; };
MrScratch mr_scratch(void *base, uint32_t V, uint32_t T)
{
    mi::Carver c(base);
    MrScratch s{};
    const size_t corners = 3 * (size_t)T;
    s.capacity = 2;
    while (s.capacity < 6 * (uint64_t)T) s.capacity <<= 1;
    s.info = c.take<uint32_t>(MR_INFO_WORDS);
    s.tb.keys = c.take<uint64_t>((size_t)s.capacity);
    s.tb.cnt = c.take<uint32_t>((size_t)s.capacity);
    s.tb.umin = c.take<int32_t>((size_t)s.capacity);
    s.tb.umax = c.take<int32_t>((size_t)s.capacity);
    s.tb.base = c.take<uint32_t>((size_t)s.capacity);
    s.list = c.take<uint32_t>(corners);
    s.parent = c.take<int32_t>(corners);
    s.root = c.take<int32_t>(corners);
    s.first = c.take<int32_t>(V);
    s.vsplit = c.take<uint32_t>(V);
    s.scan = mi::take_scan_words(c, corners > V ? corners : V);
    s.bytes = c.bytes;
    return s;
}

// corner and use ids are int32 like every index: 3 T stays below 2^31
bool mr_corner_limit_ok(uint32_t T) { return 3 * (uint64_t)T <= mi::INDEX_MAX; }

// what both entries refuse, before any launch
int mr_check(const char *who, const float *vertices, const int32_t *tris, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, MrScratch &s)
{
    if (int rc = mi::check_index_limit(who, V, T)) return rc;
    if (!mr_corner_limit_ok(T)) { ac::set_error("%s: 3 T = 3 x %u above 2^31 - 1 (corner ids are int32)", who, T); return AC_ERR_BAD_ARG; }
    if (int rc = mi::check_some_vertex(who, V, T)) return rc;
    if ((T && !tris) || (V && (!vertices || !scratch))) { ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG; }
    s = mr_scratch(scratch, V, T);
    return V ? mi::check_scratch_bytes(who, s.bytes, scratch_bytes) : AC_OK;
}

}  // namespace

AC_API size_t ac_mesh_repair_scratch(uint32_t V, uint32_t T)
{
    if (!mi::index_limit_ok(V, T) || !mr_corner_limit_ok(T)) return 0;
    return mr_scratch(nullptr, V, T).bytes;
}

AC_API int ac_mesh_repair_count(const float *vertices, const int32_t *triangles, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, uint32_t *counts,
                                ac_stream_t stream)
{
    MrScratch s;
    if (int rc = mr_check("mesh_repair_count", vertices, triangles, T, V, scratch, scratch_bytes, s)) return rc;
    if (int rc = mi::check_counts("mesh_repair_count", counts)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {                                 // (then T == 0) nothing to repair: no launch
        if (hipMemsetAsync(counts, 0, 32, st) != hipSuccess) return ac::check_launch("mesh_repair_count");
        return AC_OK;
    }
    const uint32_t corners = 3u * T, tblk = (T + 255u) / 256u;
    uint64_t cells = s.capacity > V ? s.capacity : V;
    if (cells < corners) cells = corners;
    if (cells < MR_INFO_WORDS) cells = MR_INFO_WORDS;
    const uint32_t sblk = (uint32_t)((s.capacity + 255u) / 256u);
    hipLaunchKernelGGL(mr_init_kernel, dim3((uint32_t)((cells + 255u) / 256u)), dim3(256), 0, st, s.tb, s.capacity, s.parent, corners, s.first, s.vsplit, V, s.info);
    if (T) {
        hipLaunchKernelGGL(mr_fill_kernel, dim3(tblk), dim3(256), 0, st, triangles, T, V, s.tb, s.capacity - 1u, s.info);
        hipLaunchKernelGGL(mr_lists_kernel, dim3(sblk), dim3(256), 0, st, s.tb, s.capacity, s.info);
        hipLaunchKernelGGL(mr_tickets_kernel, dim3(tblk), dim3(256), 0, st, triangles, T, V, s.tb, s.capacity - 1u, s.list);
        hipLaunchKernelGGL(mr_hook_kernel, dim3(sblk), dim3(256), 0, st, vertices, triangles, s.tb, s.capacity, s.list, s.parent, s.info);
        hipLaunchKernelGGL(mr_flatten_kernel, dim3(tblk), dim3(256), 0, st, triangles, T, V, s.parent, s.root, s.first);
    }
    hipLaunchKernelGGL(mr_count_kernel, dim3(s.scan.nblk), dim3(256), 0, st, triangles, corners, s.root, s.first, s.vsplit, s.scan.bsum, s.info);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, st, s.scan.bsum, s.scan.nblk, s.scan.boff, s.info + MR_TOTALS);
    hipLaunchKernelGGL(mr_counts_kernel, dim3(1), dim3(64), 0, st, s.info, V, counts);
    return ac::check_launch("mesh_repair_count");
}

AC_API int ac_mesh_repair_emit(const float *vertices, const int32_t *triangles, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, int32_t *triangles_out,
                               int32_t *source, uint32_t n_vertices, ac_stream_t stream)
{
    MrScratch s;
    if (int rc = mr_check("mesh_repair_emit", vertices, triangles, T, V, scratch, scratch_bytes, s)) return rc;
    if (n_vertices < V || n_vertices - V > 3u * T || n_vertices > mi::INDEX_MAX) {
        ac::set_error("mesh_repair_emit: n_vertices %u outside [V, V + 3 T] = [%u, %llu] or above 2^31 - 1", n_vertices, V, (unsigned long long)V + 3ull * T);
        return AC_ERR_BAD_ARG;
    }
    if ((T && !triangles_out) || (n_vertices && !source)) { ac::set_error("mesh_repair_emit: NULL output buffer"); return AC_ERR_BAD_ARG; }
    if (V == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t corners = 3u * T;
    hipLaunchKernelGGL(mr_rank_kernel, dim3(s.scan.nblk), dim3(256), 0, st, triangles, corners, s.root, s.first, s.scan.boff, V, s.parent, source, n_vertices);
    if (T) hipLaunchKernelGGL(mr_triangles_kernel, dim3((corners + 255u) / 256u), dim3(256), 0, st, triangles, corners, s.root, s.first, s.parent, V, triangles_out);
    return ac::check_launch("mesh_repair_emit");
}
