// avatarcraft_amd/csrc/mesh_index.hpp -- what the mesh index kernels share (marching_cubes.hip, mesh_components.hip, mesh_cluster.hip, mesh_weld.hip, mesh_repair.hip).  Each of them turns
// per-item flags or counts into output indices the same way: a count pass stores a PAIR of totals per workgroup, pair_scan_kernel (ac_scan.hpp) scans them, and
// an emit pass gives every item the index its place in the input order earns it -- no atomics, so the output is a function of the input alone.
// Device half: the pair of totals and the ordered passes; a caller never sees how the pair is packed or laid out; and the 64-bit key claim of the
// open-addressing tables (mesh_cluster.hip's cells, mesh_weld.hip's and mesh_repair.hip's edges), the wave-aggregated counters and the lock-free union-find.  Host half: the scratch walk and the refusals that more than one of the files states.
#pragma once
#include "ac_common.hpp"
#include "ac_scan.hpp"

namespace mi {

constexpr uint32_t ITEMS = 1024;                  // items per workgroup of a scanned pass: 256 threads x 4 consecutive items
constexpr uint32_t INDEX_MAX = 0x7fffffffu;       // vertex and triangle indices are int32
inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + ITEMS - 1) / ITEMS); }

// ---------------------------------------------------------------------------------------------------------------- device
namespace {       // (like the scans of ac_scan.hpp these build on: every file that includes the header has its own)

struct Pair { uint32_t lo, hi; };

__device__ __forceinline__ uint32_t first_item() { return blockIdx.x * ITEMS + threadIdx.x * 4u; }        // the first of this thread's four items

// The workgroup's totals of two per-thread counts.  A workgroup's total of either stays below 65536 (at most 5 per item), so the two are scanned as one word:
// the word pair_scan_kernel unpacks.  With bsum the word goes to bsum[this workgroup]; without, the totals come back.  Every thread of the workgroup calls this.
__device__ __forceinline__ uint32_t packed_totals(uint32_t lo, uint32_t hi, uint32_t *sh /* [8] */)
{
    uint32_t tot;
    (void)block_exscan_256(lo | (hi << 16), sh, tot);
    return tot;
}
__device__ __forceinline__ void block_totals(uint32_t lo, uint32_t hi, uint32_t *sh, uint32_t *__restrict__ bsum)
{
    const uint32_t tot = packed_totals(lo, hi, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__device__ __forceinline__ Pair block_totals(uint32_t lo, uint32_t hi, uint32_t *sh)
{
    const uint32_t tot = packed_totals(lo, hi, sh);
    return Pair{ tot & 0xffffu, tot >> 16 };
}
template <int HALF>
__device__ __forceinline__ uint32_t block_total(const uint32_t *__restrict__ bsum) { return HALF ? bsum[blockIdx.x] >> 16 : bsum[blockIdx.x] & 0xffffu; }

// count HALF (0 = low, 1 = high) of everything before workgroup `block`, from pair_scan_kernel's output
template <int HALF>
__device__ __forceinline__ uint32_t block_offset(const uint32_t *__restrict__ boff, uint32_t block) { return boff[2 * block + HALF]; }

// the output index of this thread's first item: everything before its workgroup + everything before it in the workgroup.  Every thread calls this.
template <int HALF>
__device__ __forceinline__ uint32_t ordered_base(uint32_t count, const uint32_t *__restrict__ boff, uint32_t *sh /* [8] */)
{
    uint32_t tot;
    return block_offset<HALF>(boff, blockIdx.x) + block_exscan_256(count, sh, tot);
}

// sink(item, index) for every set bit of `mask` (bit r = item first_item() + r), in item order; index = the number of set bits before it in the whole input.
// The index counts on whether or not the caller's output has room for it: where an output holds a count the caller chose, the sink writes only below it.
template <int HALF, class Sink>
__device__ __forceinline__ void ordered_pass(uint32_t mask, const uint32_t *__restrict__ boff, Sink sink)
{
    __shared__ uint32_t sh[8];
    uint32_t o = ordered_base<HALF>((uint32_t)__builtin_popcount(mask & 15u), boff, sh);
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
        if ((mask >> r) & 1u) sink(first_item() + r, o++);
}

// The kept triangles of `mask`, re-indexed, in their input order: tris_out[o] = reindex(corners of triangle t), kept_triangles[o] = t, for o < n_kept.
// (mesh_components.hip re-indexes through vertex_map, mesh_cluster.hip through the rank of the corner's slot.)
template <class Reindex>
__device__ __forceinline__ void emit_kept_triangles(uint32_t mask, const int32_t *__restrict__ tris, const uint32_t *__restrict__ boff, Reindex reindex,
                                                    int32_t *__restrict__ tris_out, int32_t *__restrict__ kept_triangles, uint32_t n_kept)
{
    ordered_pass<1>(mask, boff, [&](uint32_t t, uint32_t o) {
        if (o >= n_kept) return;
#pragma unroll
        for (int q = 0; q < 3; ++q) tris_out[3 * (size_t)o + q] = reindex(tris[3 * (size_t)t + q]);
        kept_triangles[o] = (int32_t)t;
    });
}

__device__ __forceinline__ bool tri_in_range(int32_t a, int32_t b, int32_t c, uint32_t V) { return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V; }

// ---- the 64-bit key claim of an open-addressing table (a power-of-two capacity, never more than half full, linear probing)
constexpr uint64_t KEY_EMPTY = ~0ull;             // no key: a key stays below 2^63
// gfx950 has eight XCDs with private L2s: inside a filling launch a table is touched by agent-scope atomics on GLOBAL pointers only
typedef __attribute__((address_space(1))) uint64_t gu64;
typedef __attribute__((address_space(1))) int32_t gi32;
typedef __attribute__((address_space(1))) uint32_t gu32;

__device__ __forceinline__ uint64_t key_mix(uint64_t x)           // (the finaliser of splitmix64: where a key's probe starts; no output depends on it)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// The slot of `key`, claiming one if the key has none.  A lock-free probe, no wait: a slot's key changes once, from KEY_EMPTY to a key, and never again.
// A trip ends the walk if it reads the key or wins the compare-exchange; if the exchange FAILED it returns what the slot holds now -- a key, for good -- and the
// walk ends there or moves on.  Every slot is looked at once: the table has at least twice as many slots as there are keys, so an empty slot or the key's own
// comes up within `capacity` trips whatever other waves do and whether or not they run at all.
__device__ __forceinline__ uint64_t key_slot(uint64_t *keys, uint64_t mask, uint64_t key)
{
    uint64_t s = key_mix(key) & mask;
    for (;;) {
        uint64_t seen = __hip_atomic_load((gu64 *)(keys + s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == key) return s;
        if (seen == KEY_EMPTY) {
            if (__hip_atomic_compare_exchange_strong((gu64 *)(keys + s), &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return s;
            if (seen == key) return s;
        }
        s = (s + 1u) & mask;
    }
}

// ---- counters: the sum of v over the wave, on every lane.  Every lane of the wave calls this.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
// word += the wave's sum of v: one integer add per wave, none for a wave of zeros.  Every lane of the wave calls this.
__device__ __forceinline__ void wave_add(uint32_t *word, uint32_t v)
{
    const uint32_t s = wave_sum(v);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(word, s);
}

// ---- the lock-free union-find over parent[] (mesh_components.hip's vertices, mesh_repair.hip's corners).  parent[x] == x at the start.  A hook always links
// the LARGER root under the SMALLER, so every value ever stored in parent[x] is <= the one before it and <= x, a root is an x with parent[x] == x, an x that
// stopped being a root never becomes one again, and the last root left in a set is its smallest member: the labelling is canonical although the hooks are
// atomics.  Inside the hooking launch parent[] is touched by agent-scope atomics on a GLOBAL pointer only (a plain load may return another XCD's stale line;
// the compare-exchange would still arbitrate, but progress must not rest on a stale word).
__device__ __forceinline__ int32_t cc_load(int32_t *parent, int32_t x)
{
    return __hip_atomic_load((gi32 *)(parent + x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, halving the path on the way.  Termination without anyone else running: parent[y] <= y always and a trip goes on only after it has READ
// p = parent[x] < x (and g = parent[p] < p), then continues from g < x: the index in hand strictly decreases and is bounded by 0.  The atomic min only ever
// lowers parent[x] to an ancestor of x (g is one, and x is no root: a non-root never becomes a root again), so it keeps every invariant whoever else writes.
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = cc_load(parent, x);
        if (p == x) return x;
        const int32_t g = cc_load(parent, p);
        if (g == p) return p;
        (void)__hip_atomic_fetch_min((gi32 *)(parent + x), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// Join the sets of u and v.  A lock-free retry, no wait: the loop goes round again only when the compare-exchange on parent[hi] FAILED, and a failed
// exchange returns the word's current value `seen` != hi; values stored in parent[hi] are <= hi, so seen < hi.  The next trip works on (seen, lo), both
// below hi: max(u, v) strictly decreases from trip to trip, whatever other waves do and whether or not they run at all, and it is bounded by 0 -- at most
// max(u, v) + 1 trips.  (seen and lo are in the set of hi and lo respectively, so joining them joins what was asked for.)
__device__ __forceinline__ void cc_unite(int32_t *parent, int32_t u, int32_t v)
{
    for (;;) {
        u = cc_find(parent, u);
        v = cc_find(parent, v);
        if (u == v) return;
        const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong((gi32 *)(parent + hi), &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        u = seen; v = lo;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- host
// An operation's scratch is ONE walk over its buffers, each rounded up to 256 bytes.  With a null base the walk only measures (the *_scratch entries and the
// size check: `bytes` is what it needs); with the caller's scratch the same walk hands out the typed pointers.
struct Carver {
    char *base;
    size_t bytes = 0;
    explicit Carver(void *scratch) : base(static_cast<char *>(scratch)) {}
    template <class T> T *take(size_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};
struct ScanWords { uint32_t *bsum, *boff; uint32_t nblk; };      // a workgroup's pair of totals, and pair_scan_kernel's two offsets per workgroup
inline ScanWords take_scan_words(Carver &c, uint64_t items)
{
    ScanWords s;
    s.nblk = blocks(items);
    s.bsum = c.take<uint32_t>(s.nblk);
    s.boff = c.take<uint32_t>(2 * (size_t)s.nblk);
    return s;
}

// the refusals the entries share; each returns AC_OK or sets the message and returns AC_ERR_BAD_ARG
inline bool index_limit_ok(uint32_t V, uint32_t T) { return V <= INDEX_MAX && T <= INDEX_MAX; }
inline int check_index_limit(const char *who, uint32_t V, uint32_t T)
{
    if (index_limit_ok(V, T)) return AC_OK;
    ac::set_error("%s: V %u or T %u above 2^31 - 1 (indices are int32)", who, V, T);
    return AC_ERR_BAD_ARG;
}
inline int check_some_vertex(const char *who, uint32_t V, uint32_t T)
{
    if (V != 0 || T == 0) return AC_OK;
    ac::set_error("%s: %u triangles over no vertex", who, T);
    return AC_ERR_BAD_ARG;
}
inline int check_scratch_bytes(const char *who, size_t needed, size_t given)
{
    if (given >= needed) return AC_OK;
    ac::set_error("%s: scratch of %zu bytes needed, %zu given", who, needed, given);
    return AC_ERR_BAD_ARG;
}
inline int check_counts(const char *who, const uint32_t *counts)
{
    if (counts) return AC_OK;
    ac::set_error("%s: NULL counts", who);
    return AC_ERR_BAD_ARG;
}

}  // namespace mi
