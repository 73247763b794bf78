// avatarcraft_amd/csrc/render_worklist.hpp -- the ordered work lists of the fused renderer (render_rays_kernel.hpp), as plain C++: nothing from HIP is included,
// so the builder compiles and is tested on the host alone (tests/test_worklist_host.py).
//
// A launch deals its rays to the eight XCDs (workgroup b runs on XCD b % 8) in chunks of consecutive rays; every XCD has ONE ticket counter, and ticket t
// takes item t of the XCD's list.  An item is a run of tiles [c_begin, c_end) of one ray; the sampling stage (coarse samples + NeuS up-sampling) rides on
// the ray's first item, the pixel is written by its last.  Whatever the list, a ray's sums are carried tile by tile in order, so every output is
// bit-identical for every list: the list decides only WHO works WHEN.
//
// The one property every list must have: it is a linear extension of "item k of a ray before item k + 1".  The taker of item k + 1 then only ever waits for
// a smaller ticket, which a resident wave already holds (every wave of a launch is resident: one workgroup per compute unit), and the wave that holds the
// smallest unfinished ticket waits for nobody -- so no order of arrival deadlocks.  build() keeps it by emitting the lists stage-major: all items with
// sequence number 0, then all with 1, ...
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AC_WL_HD __host__ __device__ inline
#else
#define AC_WL_HD inline
#endif

#ifndef AC_XCD_CHUNK
#define AC_XCD_CHUNK 512    // consecutive rays dealt to one XCD at a time (two image rows of a 256-wide view: neighbouring rays share grid cells in the XCD's L2)
#endif
#ifndef AC_WORKLIST_POLICY
#define AC_WORKLIST_POLICY 1    // how a ray's tiles are cut into items: see policy_split
#endif

namespace ac_worklist {

constexpr int XCDS = 8;
constexpr int MAX_ITEMS = 8;            // items per ray at most (the per-ray flag counts them in four bits)
constexpr int HEADER_WORDS = 16;        // device copy: [8] first item of each XCD's list | [8] items in it | the items, two words each

// item word 1 (word 0 is the ray: its row in the per-ray outputs)
constexpr uint32_t META_SAMPLING = 1u << 12, META_LAST = 1u << 13;
struct Item { uint32_t ray, meta; };
AC_WL_HD uint32_t make_meta(int c_begin, int c_end, int seq, bool sampling, bool last)
{
    return (uint32_t)c_begin | ((uint32_t)c_end << 4) | ((uint32_t)seq << 8) | (sampling ? META_SAMPLING : 0u) | (last ? META_LAST : 0u);
}
AC_WL_HD int meta_begin(uint32_t m) { return (int)(m & 15u); }
AC_WL_HD int meta_end(uint32_t m) { return (int)((m >> 4) & 15u); }
AC_WL_HD int meta_seq(uint32_t m) { return (int)((m >> 8) & 15u); }

// ---- the XCD chunking, in closed form (also what the one-item launches -- the two posed-space halves -- decode their tickets with) --------------------
// chunk c of xcd_chunk(n) consecutive work indices goes to XCD c % 8; a batch of up to 8 chunks is cut into eight contiguous parts
AC_WL_HD int xcd_chunk(int n_rays)
{
    const int xper = ((n_rays + 7) / 8 + 7) & ~7;
    return xper < AC_XCD_CHUNK ? xper : AC_XCD_CHUNK;
}
enum { TICKET_END = -2, TICKET_GAP = -1 };
// ticket t of XCD `xcd` -> work index in [0, n_rays), TICKET_GAP (the tail of the last chunk: take the next ticket) or TICKET_END (nothing left)
AC_WL_HD int ticket_to_work(int n_rays, int xchunk, int xcd, int t)
{
    const int k = t / xchunk, base = (k * XCDS + xcd) * xchunk;
    if (base >= n_rays) return TICKET_END;
    const int w = base + (t - k * xchunk);
    return w < n_rays ? w : TICKET_GAP;
}
// pair launches hand the 2 pair_n work indices out as a0 b0 a1 b1 ...: copy a = rows [0, pair_n), copy b = rows [pair_n, 2 pair_n)
AC_WL_HD int work_to_ray(int w, int pair_n) { return pair_n ? (w >> 1) + ((w & 1) ? pair_n : 0) : w; }

// ---- policies ----------------------------------------------------------------------------------------------------------------------------------------
// A split is given as item lengths on an 8-tile ray; a ray of `tiles` tiles gets the boundaries floor(tiles * cum / 8), empty items dropped
// (2/2/2/2 at 4 tiles is 1/1/1/1, at 5 tiles 1/1/1/2).
//   0  2/2/2/2 for every ray
//   1  3/2/2/1
//   2  2/2/2/1/1
//   3  tapered: the rays of the first round (the first waves_per_xcd rays of an XCD: every wave's first ray) keep 2/2/2/2, the later ones end 2/2/2/1/1
//   4  as 3, and the later rays alternate 1/3/2/1/1 and 3/1/2/1/1: their waves re-enter the sampling stage spread out instead of together
//   5  3/3/2      6  4/2/1/1      7  3/3/1/1      8  4/3/1        (fewer, longer items: a hand-off less per ray against a coarser end)
// The renderer is built with ONE of them (-DAC_WORKLIST_POLICY=n, default below; profiles/worklist_experiments.txt has the A/B).
constexpr int N_POLICIES = 9;
inline const int *policy_split(int policy, bool first_round, int local)
{
    static const int s2222[] = { 2, 2, 2, 2, 0 }, s3221[] = { 3, 2, 2, 1, 0 }, s22211[] = { 2, 2, 2, 1, 1, 0 }, s13211[] = { 1, 3, 2, 1, 1, 0 }, s31211[] = { 3, 1, 2, 1, 1, 0 },
                     s332[] = { 3, 3, 2, 0 }, s4211[] = { 4, 2, 1, 1, 0 }, s3311[] = { 3, 3, 1, 1, 0 }, s431[] = { 4, 3, 1, 0 };
    switch (policy) {
    case 1: return s3221;
    case 2: return s22211;
    case 3: return first_round ? s2222 : s22211;
    case 4: return first_round ? s2222 : ((local & 1) ? s31211 : s13211);
    case 5: return s332;
    case 6: return s4211;
    case 7: return s3311;
    case 8: return s431;
    default: return s2222;
    }
}
// tile boundaries of one ray: b[0] = 0 < b[1] < ... < b[n] = tiles; -> n
inline int split_bounds(const int *split8, int tiles, int b[MAX_ITEMS + 1])
{
    int n = 0, cum = 0;
    b[0] = 0;
    for (int q = 0; split8[q]; ++q) {
        cum += split8[q];
        const int e = (tiles * cum) / 8;
        if (e > b[n]) b[++n] = e;
    }
    return n;
}

// The lists of a launch of n_rays work indices (a pair launch: n_rays = 2 pair_n) of `tiles` tiles each, for waves_per_xcd waves on every XCD.
// out: HEADER_WORDS header words, then the items of XCD 0, XCD 1, ... (the layout of the device copy).
inline void build(int n_rays, int tiles, int pair_n, int waves_per_xcd, int policy, std::vector<uint32_t> &out)
{
    out.assign(HEADER_WORDS, 0u);
    if (n_rays <= 0 || tiles < 1) return;
    if (tiles > 15) tiles = 15;                                       // (four bits per boundary; the fused renderer has at most 8)
    const int xchunk = xcd_chunk(n_rays);
    std::vector<int> rays;
    uint32_t n_items = 0;
    for (int xcd = 0; xcd < XCDS; ++xcd) {
        rays.clear();
        for (int t = 0;; ++t) {
            const int w = ticket_to_work(n_rays, xchunk, xcd, t);
            if (w == TICKET_END) break;
            if (w != TICKET_GAP) rays.push_back(w);
        }
        out[xcd] = n_items;
        for (int seq = 0; seq < MAX_ITEMS; ++seq)
            for (int local = 0; local < (int)rays.size(); ++local) {
                int b[MAX_ITEMS + 1];
                const int n = split_bounds(policy_split(policy, local < waves_per_xcd, local), tiles, b);
                if (seq >= n) continue;
                out.push_back((uint32_t)work_to_ray(rays[local], pair_n));
                out.push_back(make_meta(b[seq], b[seq + 1], seq, seq == 0, seq + 1 == n));
                ++n_items;
            }
        out[XCDS + xcd] = n_items - out[xcd];
    }
}

}  // namespace ac_worklist
