// avatarcraft_amd/csrc/table_scatter.hpp -- the table-gradient scatter of the hash-grid encoder (profiles/r01_sds.txt): where the (entry, v0, v1) contributions of
// a backward go.  Its two users are the kernels of hash_stencil.hip: the 7-point stencil's backward and the reference's one-point backward.  Three steps: runs of
// lanes in the same cell (a wave holds 64 depth-sorted samples of a ray) are summed with a segmented DPP scan (run_reduce); the surviving records do not touch the
// table with atomics: they are queued per destination bucket (BinSink) and summed per bucket in LDS (bucket_accumulate_kernel); the small dense levels and every
// case without scratch go through float atomics (DirectSink).  Then the scratch layout and the host launch of the queue path.
// ONLY hash_stencil.hip includes this file: everything that sees Rec must be compiled with the same AC_REC8 (build.py's rec12 variant defines it for that one
// source), and a second translation unit with another value would corrupt the queues silently.  Anonymous namespace, like field_tile.hpp.
#pragma once
#include <mutex>
#include "grid_cell.hpp"
#include "wave_ops.hpp"

// ---- tuning constants (each may be overridden with -D: tools/build_variants.py) -----------------------------------------------------------------------------------
#ifndef AC_ACC_W
#define AC_ACC_W 8             // bucket_accumulate_kernel: table elements per thread whose read-modify-write is issued together
#endif
#ifndef AC_ACC_U
#define AC_ACC_U 4             // bucket_accumulate_kernel: queue records in flight per thread
#endif
#ifndef AC_RCAP
#define AC_RCAP 1536           // records per wave buffer of the queue fill; add8 reserves room for 8 x 64 records
#endif
#ifndef AC_FILL_PACK_MAX
#define AC_FILL_PACK_MAX 32    // most run tails per wave for which the packed path is taken (8 per chunk; above ~40 the sparse walk is cheaper)
#endif
#ifndef AC_FILL_GX
#define AC_FILL_GX 96      // workgroups per level.  Round 2: 256 -> 128 was 3.66 -> 3.39 ms of backward per step (96: 3.51, 64: 3.53, 32: 3.77; profiles/r02_experiments.txt);
                           // round 6, after the fill's index arithmetic shrank: 96 = 2.14 ms against 128: 2.18, 112: 2.15, 80: 2.20, 64: 2.21, 160: 2.29 (16 levels x 96 x 4 waves =
                           // three full rounds of the device's 2048 wave slots; the sums are order-independent, the bits do not depend on this)
#endif

namespace {

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// the level of rank `rank` among the binned ones = the rank-th set bit of binned_mask (ranks index the queues and their counters)
__device__ __forceinline__ uint32_t level_of_rank(uint32_t binned_mask, const ac::LevelTable &lt, uint32_t rank)
{
    uint32_t level = 0, seen = 0;
    for (uint32_t l = 0; l < lt.L; ++l) if ((binned_mask >> l) & 1u) { if (seen == rank) level = l; ++seen; }
    return level;
}

// ---- the run scan ------------------------------------------------------------------------------------------------------------
// A wave holds 64 consecutive samples of one ray (B index = ray * T + sample, sorted by depth), and the importance sampling packs
// most of them into a few cells: neighbouring lanes that sit in the same cell address the same table entries.  Their
// contributions are summed inside the wave first (segmented inclusive scan over runs of equal cell, 6 shuffle steps) and only
// the last lane of each run issues the atomics.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_f(float v)
{
    // lanes without a valid source (first lanes of a row for row_shr, rows outside ROW_MASK for row_bcast) receive 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf));
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf); }

// one step of the segmented scan: every lane that has not met the head of its run yet (f == 0) adds the value CTRL points at.
// v += dpp(v) * m with m in {0, 1} is ONE v_fmac_f32_dpp per value (the compiler's DPP combiner does not fold a DPP move into
// v_fmac, hence the inline assembly).  The s_nop covers the "VALU write -> DPP read" (2) and "VALU writes EXEC -> DPP" (5) wait states for the first value of a step
// (the hazard recogniser does not look into inline assembly); within a step and between steps N - 1 >= 15 instructions lie
// between the write of a register and its DPP read.
#define AC_FMAC_DPP(MODS) asm volatile("v_fmac_f32_dpp %0, %0, %1 " MODS : "+v"(v[i]) : "v"(m))
template <int N, int CTRL, int ROW_MASK>
__device__ __forceinline__ void run_step(float (&v)[N], int &f)
{
    const float m = f ? 0.0f : 1.0f;
    asm volatile("s_nop 4");
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if constexpr (CTRL == 0x111) AC_FMAC_DPP("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0");
        else if constexpr (CTRL == 0x112) AC_FMAC_DPP("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0");
        else if constexpr (CTRL == 0x114) AC_FMAC_DPP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0");
        else if constexpr (CTRL == 0x118) AC_FMAC_DPP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:0");
        else if constexpr (CTRL == 0x142) AC_FMAC_DPP("row_bcast:15 row_mask:0xa bank_mask:0xf");
        else AC_FMAC_DPP("row_bcast:31 row_mask:0xc bank_mask:0xf");
    }
    f |= dpp_i<CTRL, ROW_MASK>(f);
}
#undef AC_FMAC_DPP

// segmented inclusive sums over runs of lanes (head = first lane of a run): DPP only, no LDS traffic -- Kogge-Stone inside every
// 16-lane row (row_shr 1, 2, 4, 8), then the open tail of the previous row(s) is carried over with row_bcast15 / row_bcast31.
// Returns true in the last lane of every run (the one that holds the run's total).
template <int N>
__device__ __forceinline__ bool run_reduce(float (&v)[N], bool head, int lane, bool norun = false)
{
    // norun (wave-uniform): a lane of this wave carries an Inf / NaN upstream gradient.  The scan below adds `neighbour * {0, 1}`, and
    // Inf * 0 = NaN would leak into every lane of the row: such a group scatters lane by lane, so that a non-finite gradient reaches
    // exactly the entries the reference's atomicAdd would give it (hashencoder.cu:302-305)
    if (norun) return true;
    int f = head ? 1 : 0;
    // every value has to be final BEFORE the first DPP read (the scheduler may otherwise sink the instruction that produces v[i + 1]
    // between two of the inline-assembly statements, inside the hazard window): empty volatile statements pin them
    static_assert(N % 8 == 0, "run_reduce works on multiples of 8 values");
#pragma unroll
    for (int c = 0; c < N; c += 8)
        asm volatile("" : "+v"(v[c]), "+v"(v[c + 1]), "+v"(v[c + 2]), "+v"(v[c + 3]), "+v"(v[c + 4]), "+v"(v[c + 5]), "+v"(v[c + 6]), "+v"(v[c + 7]));
    // A step only moves values into lanes that have not met the head of their run yet (f == 0): once no such lane is left in the wave, the
    // remaining steps would add `neighbour * 0` everywhere and are skipped (wave-uniform branch; round 4: the scan is more than half of the
    // fill's vector instructions, and outside the densely sampled shell of the surface runs are a few lanes long on all but the coarsest levels).
    // The skipped additions of +-0 can only turn a -0 into +0: a value that the != 0 predicate drops or the fixed-point sum reads as 0 either way.
#define AC_RUN_DONE() (__builtin_amdgcn_ballot_w64(f == 0) == 0ull)
    do {
        if (AC_RUN_DONE()) break;
        run_step<N, 0x111, 0xf>(v, f);
        if (AC_RUN_DONE()) break;
        run_step<N, 0x112, 0xf>(v, f);
        if (AC_RUN_DONE()) break;
        run_step<N, 0x114, 0xf>(v, f);
        if (AC_RUN_DONE()) break;
        run_step<N, 0x118, 0xf>(v, f);
        if (AC_RUN_DONE()) break;
        run_step<N, 0x142, 0xa>(v, f);          // row_bcast15: rows 1 and 3 take lane 15 of rows 0 and 2
        if (AC_RUN_DONE()) break;
        run_step<N, 0x143, 0xc>(v, f);          // row_bcast31: rows 2 and 3 take lane 31
    } while (false);
#undef AC_RUN_DONE
    const int next_head = __shfl_down(head ? 1 : 0, 1);
    return lane == 63 || next_head != 0;
}

__device__ __forceinline__ bool run_head(const Loc (&q)[3], bool ok, int lane)
{
    const uint32_t p0 = __shfl_up(q[0].pg, 1), p1 = __shfl_up(q[1].pg, 1), p2 = __shfl_up(q[2].pg, 1);
    const int pok = __shfl_up(ok ? 1 : 0, 1);
    return lane == 0 || p0 != q[0].pg || p1 != q[1].pg || p2 != q[2].pg || pok != (ok ? 1 : 0);    // runs are homogeneous in `ok`
}

// ---- where the combined gradients go -------------------------------------------------------------------------------------------
// DirectSink: two hardware float atomics per table entry (the device does ~20.9 G of those per second, whatever the scope, table
// size or address spread: tools/atomics_bench.hip) -- used for the small dense levels (with private copies).
// BinSink: the hashed levels.  A record (entry, v0, v1) is appended to a per-wave LDS buffer; a flush bins the buffer by
// destination bucket (64 buckets of 8192 entries per level), reserves the slots of every bucket with ONE global atomic per
// (flush, bucket) and streams the records into per-bucket queues in HBM; bucket_accumulate_kernel then gives every bucket to
// one workgroup that sums its queue in LDS (ds_add_f32, ~1000x the global atomic rate) and adds the 64 KB slice to the table
// without atomics.  Global atomics per record: 2 -> ~1/30.
struct DirectSink {
    static constexpr bool packs = false;
    float2 *gg;
    __device__ __forceinline__ void tick(int) const {}
    // eight table entries at once: pred[k] says whether this lane contributes (v[2k], v[2k+1]) to entry index_of(k)
    template <class F> __device__ __forceinline__ void add8(const bool (&pred)[8], F index_of, const float (&v)[16]) const
    {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (pred[k]) { float *t = reinterpret_cast<float *>(gg + index_of(k)); unsafeAtomicAdd(t, v[2 * k]); unsafeAtomicAdd(t + 1, v[2 * k + 1]); }
    }
};

constexpr int NBUCKET = 64;
constexpr int RCAP = AC_RCAP;
constexpr int PACK_TAILS = 8;                          // run tails staged per chunk: 8 tails x 8 entries = the wave's 64 lanes
constexpr int PACK_STRIDE = 20;                        // staged words per tail: 16 values (8 entries x 2 channels) + the cell's three axis terms (+ 1 pad: 16-byte rows)
constexpr int STAGE_WORDS = PACK_TAILS * PACK_STRIDE;
constexpr int WAVE_WORDS = 3 * RCAP + 2 * NBUCKET + STAGE_WORDS;     // LDS words per wave: ridx, rv0, rv1 [RCAP], hist, base [64], the packing stage
static_assert(RCAP % 2 == 0 && RCAP >= 1024, "wave buffer: room for two batches of 8 x 64 records");

// ---- the record codec: the ONE place that knows a queue record's layout --------------------------------------------------------------------------------------
// rec_quantise(v0, v1) rounds a contribution to what a record holds, rec_make(idx, v0, v1) forms the record of quantised values for the entry idx of its bucket,
// rec_read(r, idx, v0, v1) takes it apart again.
#ifndef AC_REC8
#define AC_REC8 1           // 1 (round 4): 8-byte queue records -- 13 bits of entry index inside its bucket | v0 rounded to 16 explicit mantissa bits (25 bits) | v1
#endif                      //    rounded to 17 (26 bits).  PRECISION CONTRACT of the table gradient: every (entry, v0, v1) contribution is rounded
                            //    to nearest at 2^-17 / 2^-18 of its own magnitude before the order-independent fixed-point sum -- below the fp32 round-off of a sum
                            //    of a few records, checked against the fp64 oracle backward at 3e-4 of max (observed 1.2e-4, unchanged).  The queue traffic is what
                            //    the two scatter passes are short of: 16-byte records cost the step +0.21 ms, 8-byte ones gain (profiles/r04_experiments.txt 8b).
#if AC_REC8
struct __attribute__((aligned(8))) Rec { uint32_t lo, hi; };
__device__ __forceinline__ float rec_round(float v, int drop)        // round to nearest at bit `drop` (quiet NaN and Inf survive; FLT_MAX may round to Inf)
{
    return __uint_as_float((__float_as_uint(v) + (1u << (drop - 1))) & ~((1u << drop) - 1u));
}
// values are rounded BEFORE the level's max |v| -- the fixed-point scale -- is taken (BinSink::flush), so that it is taken over what is actually summed
__device__ __forceinline__ void rec_quantise(float &v0, float &v1) { v0 = rec_round(v0, 7); v1 = rec_round(v1, 6); }
__device__ __forceinline__ Rec rec_make(uint32_t idx13, float v0, float v1)
{
    const uint32_t a = __float_as_uint(v0) >> 7, b = __float_as_uint(v1) >> 6;      // 25 and 26 bits (the dropped bits are zero: rec_quantise)
    Rec r; r.lo = idx13 | (a << 13); r.hi = (a >> 19) | (b << 6);
    return r;
}
__device__ __forceinline__ void rec_read(const Rec &r, uint32_t &idx13, float &v0, float &v1)
{
    idx13 = r.lo & 0x1fffu;
    v0 = __uint_as_float(((r.lo >> 13) | ((r.hi & 0x3fu) << 19)) << 7);
    v1 = __uint_as_float((r.hi >> 6) << 6);
}
#else
struct Rec { uint32_t idx; float v0, v1; };
__device__ __forceinline__ void rec_quantise(float &, float &) {}
__device__ __forceinline__ Rec rec_make(uint32_t idx, float v0, float v1) { Rec r; r.idx = idx; r.v0 = v0; r.v1 = v1; return r; }
__device__ __forceinline__ void rec_read(const Rec &r, uint32_t &idx, float &v0, float &v1) { idx = r.idx; v0 = r.v0; v1 = r.v1; }
#endif

// entries per bucket = 2^bucket_shift: the smallest power of two that covers the level with NBUCKET buckets
__host__ __device__ __forceinline__ uint32_t bucket_shift(uint32_t size)
{
    uint32_t sh = 0;
    while (((size + (1u << sh) - 1u) >> sh) > (uint32_t)NBUCKET) ++sh;
    return sh;
}
// Largest level the binned scatter takes (binned_levels): an entry's index inside its bucket must fit the 13 bits rec_make gives it (8-byte records) and the
// 19 bits ridx gives the entry in the wave buffer (BinSink::add8, every record layout); a bucket's slice must fit bucket_accumulate_kernel's LDS image.
constexpr uint32_t BIN_IDX_BITS = 13, BIN_MAX_LEVEL = 1u << 19;
static_assert((uint32_t)NBUCKET << BIN_IDX_BITS >= BIN_MAX_LEVEL, "rec_make: the in-bucket index of the largest binned level needs more than 13 bits");

// the counter block of a launch over n_binned levels: [n_binned][NBUCKET] queue lengths, then [n_binned] bits of the level's max |v|
__host__ __device__ __forceinline__ size_t vmax_slot(uint32_t n_binned, uint32_t rank) { return (size_t)n_binned * NBUCKET + rank; }
inline size_t counter_bytes(uint32_t n_binned) { return vmax_slot(n_binned, n_binned) * 4; }

#ifdef AC_PROFILE_FILL
__device__ unsigned long long g_fill_prof[AC_MAX_LEVELS * 6];      // [level][combine, records, reservation, write-out, whole wave, flushes] s_memtime ticks summed over waves
#endif

struct BinSink {
    static constexpr bool packs = true;
    uint32_t *ridx; float *rv0, *rv1;      // this wave's LDS record buffer [RCAP]; ridx = entry | rank inside its bucket << 19
    uint32_t *hist, *base;                 // this wave's LDS [NBUCKET] each (hist zero between flushes)
    uint32_t cnt;                          // wave-uniform
    uint32_t sh;                           // bucket = index >> sh (2^sh entries per bucket, <= NBUCKET buckets per level)
    uint32_t mx;                           // per lane: bits of the largest |v| this lane has recorded (published once, by finish())
    uint32_t *qcount;                      // global [NBUCKET] of this level
    uint32_t *vmax;                        // global: bits of max |v| over this level's records (positive floats order like uints)
    Rec *queue;                            // global [NBUCKET][cap] of this level
    uint32_t cap;
    float2 *gg;                            // overflow path: direct atomics
    int lane;
    float *stage;                          // this wave's LDS [PACK_TAILS][PACK_STRIDE] (the packed path of stencil_scatter)
#ifdef AC_PROFILE_FILL                     // s_memtime per phase: 0 stencil combine + run scan, 1 records -> LDS, 2 flush: slot reservation, 3 flush: write-out
    unsigned long long ft, t0, facc[4], nflush;
    __device__ __forceinline__ void tick(int slot) { const unsigned long long t2 = __builtin_amdgcn_s_memtime(); facc[slot] += t2 - ft; ft = t2; }
    __device__ __forceinline__ void report(uint32_t level) const
    {
        if (lane != 0) return;
        unsigned long long *o = g_fill_prof + (size_t)level * 6;
        atomicAdd(o, facc[0]); atomicAdd(o + 1, facc[1]); atomicAdd(o + 2, facc[2]); atomicAdd(o + 3, facc[3]);
        atomicAdd(o + 4, __builtin_amdgcn_s_memtime() - t0); atomicAdd(o + 5, nflush);
    }
#else
    __device__ __forceinline__ void tick(int) {}
    __device__ __forceinline__ void report(uint32_t) const {}
#endif
    // the sink of one wave for the binned level `level` of rank ylev among the launch's n_binned (= the fill's gridDim.y); wbase: the wave's WAVE_WORDS of LDS
    __device__ __forceinline__ void init(uint32_t *wbase, int lane_, const ac::LevelTable &lt, uint32_t level, uint32_t ylev, uint32_t n_binned,
                                         uint32_t *qcount_, Rec *queues, uint32_t cap_, float *grad_grid)
    {
        ridx = wbase; rv0 = reinterpret_cast<float *>(wbase + RCAP); rv1 = reinterpret_cast<float *>(wbase + 2 * RCAP);
        hist = wbase + 3 * RCAP; base = hist + NBUCKET;
        stage = reinterpret_cast<float *>(base + NBUCKET);
        cnt = 0; lane = lane_;
        sh = bucket_shift(lt.size[level]); mx = 0u;
        qcount = qcount_ + (size_t)ylev * NBUCKET;
        vmax = qcount_ + vmax_slot(n_binned, ylev);
        queue = queues + (size_t)ylev * NBUCKET * cap_;
        cap = cap_;
        gg = reinterpret_cast<float2 *>(grad_grid) + lt.offset[level];
        hist[lane] = 0u;
#ifdef AC_PROFILE_FILL
        facc[0] = facc[1] = facc[2] = facc[3] = 0ull; nflush = 0ull; ft = t0 = __builtin_amdgcn_s_memtime();
#endif
    }
    // the bucket histogram is taken while the record is still in registers: the flush is then ONE pass over the buffer (three passes over LDS cost 1.2 of
    // the kernel's 1.85 ms, profiles/r01_sds.txt); that pass also rounds the values to the record's precision and tracks the running max |v| (round 6)
    // eight table entries at once (after reserving room for 8 x 64 records): the bucket ranks of all eight are requested first
    // (LDS atomics with return), then the records are written -- one LDS round trip per eight slots instead of eight
    template <class F> __device__ __forceinline__ void add8(const bool (&pred)[8], F index_of, const float (&v)[16])
    {
        if (cnt + 512u > (uint32_t)RCAP) flush();
        unsigned long long m[8];
        uint32_t index[8], rank[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            m[k] = __ballot(pred[k]);
            index[k] = 0u; rank[k] = 0u;
            if (m[k] != 0ull && pred[k]) {                                         // wave-uniform skip: most neighbour slots of a coarse level are empty
                index[k] = index_of(k);
                rank[k] = atomicAdd(&hist[index[k] >> sh], 1u);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (m[k] == 0ull) continue;
            if (pred[k]) {
                const uint32_t pos = cnt + (uint32_t)__builtin_popcountll(m[k] & ((1ull << lane) - 1ull));
                // (the contribution is stored as it is: its rounding to the record's precision and the running max |v| happen in flush(), on the DENSE record
                // stream -- here, after the run combining, a tenth to a half of the lanes are live and every instruction costs a full issue slot all the same)
                ridx[pos] = index[k] | (rank[k] << 19); rv0[pos] = v[2 * k]; rv1[pos] = v[2 * k + 1];
            }
            cnt += (uint32_t)__builtin_popcountll(m[k]);
        }
    }
    // one table entry per lane (the packed path: every lane may carry one)
    __device__ __forceinline__ void add1(bool pred, uint32_t index, float v0, float v1)
    {
        if (cnt + 64u > (uint32_t)RCAP) flush();
        const unsigned long long m = __ballot(pred);
        if (m == 0ull) return;
        if (pred) {
            const uint32_t rank = atomicAdd(&hist[index >> sh], 1u);
            const uint32_t pos = cnt + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            ridx[pos] = index | (rank << 19); rv0[pos] = v0; rv1[pos] = v1;
        }
        cnt += (uint32_t)__builtin_popcountll(m);
    }
    // the level's largest |v| (the fixed-point scale of bucket_accumulate_kernel): one wave reduction and one global atomic per WAVE,
    // after its last flush (it used to be per flush: 0.26 of the fill's 1.8 ms, profiles/r01_sds.txt "without the max pass")
    __device__ __forceinline__ void finish()
    {
        flush();
        uint32_t wmx = mx;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)wmx, d); wmx = wmx > o ? wmx : o; }
        if (lane == 0 && wmx) atomicMax(vmax, wmx);
    }
    __device__ __forceinline__ void flush()
    {
        tick(1);
        wave_sync();
        {
            const uint32_t c = hist[lane];
            base[lane] = c ? atomicAdd(&qcount[lane], c) : 0u;
            hist[lane] = 0u;
        }
        wave_sync();
        tick(2);
        // write-out, WU records per lane and trip: the LDS reads of a trip are issued together (one LDS latency per trip, not per record)
        constexpr uint32_t WU = 4;
        for (uint32_t i0 = lane; i0 < cnt; i0 += 64 * WU) {
            uint32_t packed[WU]; float v0[WU], v1[WU]; uint32_t bs[WU];
#pragma unroll
            for (uint32_t u = 0; u < WU; ++u) {
                const uint32_t i = i0 + 64 * u, ic = i < cnt ? i : i0;
                packed[u] = ridx[ic]; v0[u] = rv0[ic]; v1[u] = rv1[ic];
                rec_quantise(v0[u], v1[u]);                                            // the record's precision (rec_make drops nothing after this)
                if (i < cnt) {
                    const uint32_t a0 = __float_as_uint(v0[u]) & 0x7fffffffu, a1 = __float_as_uint(v1[u]) & 0x7fffffffu;
                    mx = mx > a0 ? mx : a0; mx = mx > a1 ? mx : a1;
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < WU; ++u) bs[u] = base[(packed[u] & 0x7ffffu) >> sh];
#pragma unroll
            for (uint32_t u = 0; u < WU; ++u) {
                if (i0 + 64 * u >= cnt) continue;
                const uint32_t idx = packed[u] & 0x7ffffu, bucket = idx >> sh;
                const uint32_t slot = bs[u] + (packed[u] >> 19);
                if (slot < cap) {
                    queue[(size_t)bucket * cap + slot] = rec_make(idx - (bucket << sh), v0[u], v1[u]);
                } else {                    // queue full (never with the default sizing): fall back to atomics
                    float *t = reinterpret_cast<float *>(gg + idx); unsafeAtomicAdd(t, v0[u]); unsafeAtomicAdd(t + 1, v1[u]);
                }
            }
        }
        wave_sync();
        cnt = 0;
        tick(3);
#ifdef AC_PROFILE_FILL
        ++nflush;
#endif
    }
};

// one point's 8 corners, combined over the run of lanes in the same cell
template <class Sink>
__device__ __forceinline__ void scatter8_runs(Sink &sink, const LevelC &L, const Loc (&q)[3], float g0, float g1, int lane, bool norun = false)
{
    const bool ok = !(q[0].oob | q[1].oob | q[2].oob);
    float v[16];
#pragma unroll
    for (uint32_t idx = 0; idx < 8; ++idx) {
        float w = 1.0f;
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) w *= ((idx >> d) & 1u) ? q[d].fr : 1.0f - q[d].fr;
        v[2 * idx] = ok ? w * g0 : 0.0f; v[2 * idx + 1] = ok ? w * g1 : 0.0f;
    }
    const bool tail = run_reduce<16>(v, run_head(q, ok, lane), lane, norun) && ok;
    sink.tick(0);
    bool pred[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) pred[k] = tail && (v[2 * k] != 0.0f || v[2 * k + 1] != 0.0f);
    const uint32_t my = level_my(L), mz = level_mz(L), ty0 = q[1].pg * my, tz0 = q[2].pg * mz;
    sink.add8(pred, [&](int k) { return cell_corner(L, q[0].pg, ty0, tz0, my, mz, (uint32_t)k); }, v);
    sink.tick(1);
}

// one workgroup per (bucket, binned level): sum the bucket's queue in LDS, then add the slice to the table (no atomics: the
// workgroup owns these entries, and every producer of records has finished -- kernel boundary).
// LDS float atomics (ds_add_f32) run at 0.33 lane-operations per clock and CU on gfx950, integer ones (ds_add_u32 / ds_add_u64) at
// > 3 (tools/lds_atomics_bench.hip), so the sums are taken in 64-bit fixed point: v * 2^k with 2^k chosen from the level's largest
// |v| (collected by the queue fill) and the length n of this queue, |v| 2^k < 2^(62 - ceil(log2(n + 1))), so that no entry can
// overflow.  Contributions keep >= 24 significant bits down to 2^-18 of the level's maximum and vanish below 2^-42 of it; in
// exchange the result does not depend on the order of the records (deterministic), which float atomics never gave.
// One launch covers the binned levels of rank y0 .. y0 + gridDim.y - 1 (rank = position among the set bits of binned_mask, n_binned of them).
__global__ __launch_bounds__(1024) void bucket_accumulate_kernel(float *__restrict__ grad_grid, ac::LevelTable lt, uint32_t binned_mask,
                                                                 const uint32_t *__restrict__ qcount, const Rec *__restrict__ queues, uint32_t cap,
                                                                 uint32_t y0, uint32_t n_binned)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];        // [entries per bucket][2]
    const uint32_t ylev = y0 + gridDim.y - 1u - blockIdx.y;       // longest queues (finest levels) first
    const uint32_t level = level_of_rank(binned_mask, lt, ylev);
    const uint32_t per = 1u << bucket_shift(lt.size[level]), bucket = blockIdx.x;
    const uint32_t first = bucket * per;
    const uint32_t mine = first >= lt.size[level] ? 0u : (lt.size[level] - first < per ? lt.size[level] - first : per);     // the last bucket may be short
    uint32_t n = qcount[(size_t)ylev * NBUCKET + bucket];
    n = n < cap ? n : cap;
    const uint32_t mbits = qcount[vmax_slot(n_binned, ylev)];
    if (n == 0 || mbits == 0 || mine == 0) return;                                   // wave-uniform: nothing queued for this bucket
    const Rec *q = queues + ((size_t)ylev * NBUCKET + bucket) * cap;
    float *dst = grad_grid + ((size_t)lt.offset[level] + (size_t)first) * 2;
    if ((mbits >> 23) == 255u) {
        // an Inf or NaN record on this level (the largest |v| carries exponent 255): no fixed-point scale exists.  Sum this bucket in float
        // instead (slow LDS float atomics, but only ever on a diverged step), so that Inf / NaN reach the table exactly as the
        // reference's atomicAdd would deliver them (hashencoder.cu:302-305) instead of being quantised away.
        float *accf = reinterpret_cast<float *>(acc);
        for (uint32_t e = threadIdx.x; e < per * 2; e += blockDim.x) accf[e] = 0.0f;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            uint32_t ri; float rv0, rv1; rec_read(q[i], ri, rv0, rv1);
            atomicAdd(&accf[2 * ri], rv0); atomicAdd(&accf[2 * ri + 1], rv1);
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < mine * 2; e += blockDim.x)
            if (accf[e] != 0.0f) dst[e] += accf[e];                                  // NaN != 0 is true: NaN is written
        return;
    }
    for (uint32_t e = threadIdx.x; e < per * 2; e += blockDim.x) acc[e] = 0ull;
    __syncthreads();
    // fixed-point sums of the bucket's entries: channel c of entry i at AC_ACC_AT(i, c).  (Round 4 measured the two channels in separate halves of the slice,
    // so that the 64 lanes of one LDS atomic spread over 32 bank pairs instead of 16 bank quads: nothing.)
#define AC_ACC_AT(I, CH) (2u * (I) + (CH))
    const int emax = (int)(mbits >> 23) - 126;                                       // |v| < 2^emax for every record of the level
    const int head = 32 - __builtin_clz(n);                                          // ceil(log2(n + 1))
    const int k = 62 - head - emax;
    constexpr int U = AC_ACC_U;
    for (uint32_t i0 = threadIdx.x; i0 < n; i0 += blockDim.x * U) {
        Rec raw[U];
        struct { uint32_t idx; float v0, v1; } r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const uint32_t i = i0 + u * blockDim.x; raw[u] = q[i < n ? i : i0]; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * blockDim.x;
            rec_read(raw[u], r[u].idx, r[u].v0, r[u].v1);
            if (i >= n) { r[u].v0 = 0.0f; r[u].v1 = 0.0f; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r[u].v0 != 0.0f) atomicAdd(&acc[AC_ACC_AT(r[u].idx, 0u)], (unsigned long long)__double2ll_rn(ldexp((double)r[u].v0, k)));
            if (r[u].v1 != 0.0f) atomicAdd(&acc[AC_ACC_AT(r[u].idx, 1u)], (unsigned long long)__double2ll_rn(ldexp((double)r[u].v1, k)));
        }
    }
    __syncthreads();
    // slice += sums, AC_ACC_W elements per thread at a time with their table loads issued together: one element per trip made every workgroup pay 16
    // dependent global round trips here (~1 / 4 of the kernel: r04_experiments.txt 8d)
    constexpr uint32_t W = AC_ACC_W;
    for (uint32_t e0 = threadIdx.x; e0 < mine * 2; e0 += blockDim.x * W) {
        long long v[W]; float old[W];
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) { const uint32_t e = e0 + u * blockDim.x; v[u] = e < mine * 2 ? (long long)acc[AC_ACC_AT(e >> 1, e & 1u)] : 0ll; }
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) old[u] = v[u] != 0 ? dst[e0 + u * blockDim.x] : 0.0f;
#pragma unroll
        for (uint32_t u = 0; u < W; ++u)
            if (v[u] != 0) dst[e0 + u * blockDim.x] = old[u] + (float)ldexp((double)v[u], -k);
    }
#undef AC_ACC_AT
}

__global__ __launch_bounds__(256) void priv_reduce_kernel(const float *__restrict__ priv, uint32_t n_floats, uint32_t n_copies,
                                                          float *__restrict__ grad_grid)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    float s = 0.0f;
    for (uint32_t c = 0; c < n_copies; ++c) s += priv[(size_t)c * n_floats + i];
    if (s != 0.0f) grad_grid[i] += s;
}

// ---- the scratch layout ---------------------------------------------------------------------------------------------------------------------------------------
// entries of the leading dense levels that are worth privatising (none if the caller gives no scratch)
uint32_t priv_levels(const ac::LevelTable &lt, uint32_t L, uint32_t &entries)
{
    uint32_t n = 0; entries = 0;
    while (n < L && !lt.hashed[n] && lt.size[n] <= (1u << 18) && lt.offset[n] == entries) { entries += lt.size[n]; ++n; }
    return n;
}

// levels that go through the binned path: 64 buckets of <= 8192 entries (64 KB of LDS), i.e. every level of up to 2^19 entries
uint32_t binned_levels(const ac::LevelTable &lt, uint32_t L)
{
    uint32_t m = 0;
    for (uint32_t l = 0; l < L; ++l)
        if (lt.size[l] >= (uint32_t)NBUCKET && lt.size[l] <= BIN_MAX_LEVEL && bucket_shift(lt.size[l]) <= BIN_IDX_BITS) m |= 1u << l;
    return m;
}
uint32_t queue_cap(uint32_t B, uint32_t per_sample = 56u) { return (uint32_t)(((uint64_t)B * per_sample * 3u / 2u) / NBUCKET) + 4096u; }   // 1.5 x the average

struct StencilScratch { size_t priv_off, qcount_off, queue_off, total; uint32_t entries, n_priv, binned_mask, n_binned, cap; };
StencilScratch stencil_layout(const ac::LevelTable &lt, uint32_t L, uint32_t n_copies, uint32_t B, uint32_t per_sample = 56u)
{
    StencilScratch sc{};
    sc.n_priv = (n_copies >= 2 && B == 0) ? priv_levels(lt, L, sc.entries) : 0;       // with queues (B > 0) every level is binned
    size_t off = 0;
    sc.priv_off = off; off += ((size_t)sc.entries * 8 * (sc.n_priv ? n_copies : 0) + 255) & ~(size_t)255;
    sc.binned_mask = B ? binned_levels(lt, L) : 0;
    sc.n_binned = (uint32_t)__builtin_popcount(sc.binned_mask);
    sc.cap = queue_cap(B, per_sample);
    sc.qcount_off = off; off += (counter_bytes(sc.n_binned) + 255) & ~(size_t)255;       // slot counters + the level's max |v|
    sc.queue_off = off; off += (size_t)sc.n_binned * NBUCKET * sc.cap * sizeof(Rec);
    sc.total = off;
    return sc;
}

// ---- the host side of the queue path ------------------------------------------------------------------------------------------------------------------------------
// side waits for everything enqueued on st so far (one event per device, recorded and waited for under one lock: host threads cannot interleave)
bool order_side_stream(hipStream_t st, hipStream_t side)
{
    static std::mutex mu;
    static hipEvent_t ev[64];
    static bool have[64];
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    dev &= 63;
    if (!have[dev]) { if (hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming) != hipSuccess) return false; have[dev] = true; }
    return hipEventRecord(ev[dev], st) == hipSuccess && hipStreamWaitEvent(side, ev[dev], 0) == hipSuccess;
}

// The queue path of one backward over B samples on st: clear the counters, fill the queues of the sc.n_binned levels with the caller's kernel -- fill(gx, lds_bytes,
// qcount, queues) launches fill_kernel on a grid of (gx, sc.n_binned) x 256 threads -- and accumulate them into the table.  y_split > 0: the accumulation runs in two
// launches, ranks >= y_split first, and `side` is ordered behind that launch, so that work the caller enqueues there (the all-reduce of that part of the table
// gradient) starts while the second launch -- and whatever follows on st -- still runs; false if that ordering failed (the rest is then not launched).
// (Fill is a type of its own per caller: so are the statics, one per fill kernel.)
template <class Fill>
bool queue_scatter(const StencilScratch &sc, void *scratch, const ac::LevelTable &lt, float *grad_grid, uint32_t B, hipStream_t st, const void *fill_kernel,
                   Fill fill, uint32_t y_split = 0, hipStream_t side = nullptr)
{
    uint32_t *qcount = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + sc.qcount_off);
    Rec *queues = reinterpret_cast<Rec *>(static_cast<char *>(scratch) + sc.queue_off);
    hipMemsetAsync(qcount, 0, counter_bytes(sc.n_binned), st);
    static uint64_t seen1 = 0, seen2 = 0;
    const size_t lds1 = (size_t)4 * WAVE_WORDS * 4, lds2 = (size_t)BIN_MAX_LEVEL / NBUCKET * 16;
    ac::allow_dynamic_lds(seen1, fill_kernel, lds1);
    ac::allow_dynamic_lds(seen2, reinterpret_cast<const void *>(bucket_accumulate_kernel), lds2);
    uint32_t gx = ((B + 63) / 64 + 3) / 4;
    if (gx > AC_FILL_GX) gx = AC_FILL_GX;            // persistent waves: full record buffers per flush, few partial last ones
    fill(gx, lds1, qcount, queues);
    auto accumulate = [&](uint32_t y0, uint32_t y1) {                // the binned levels of rank y0 .. y1 - 1
        hipLaunchKernelGGL(bucket_accumulate_kernel, dim3(NBUCKET, y1 - y0), dim3(1024), lds2, st, grad_grid, lt, sc.binned_mask, qcount, queues, sc.cap, y0,
                           sc.n_binned);
    };
    if (y_split) {
        accumulate(y_split, sc.n_binned);
        if (!order_side_stream(st, side)) return false;
        accumulate(0u, y_split);
    } else accumulate(0u, sc.n_binned);
    return true;
}

}  // namespace
