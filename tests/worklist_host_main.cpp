// tests/worklist_host_main.cpp -- stand-alone check of csrc/render_worklist.hpp (plain host code: tests/test_worklist_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it).  For every policy and shape it checks what the render kernel relies on:
//   * every (ray, tile) is covered exactly once;
//   * a ray's items appear in order (sequence numbers 0, 1, ... at increasing positions of ONE list), contiguous in tiles, at most MAX_ITEMS of them;
//   * each ray is on the list of the XCD the chunking gives it (written out independently below);
//   * the sampling stage rides on a ray's first item only, and only the last item is marked last;
//   * the closed-form ticket decode of the one-item launches walks the XCD's rays in the order the builder lists them.
// Prints one line per policy; exit status 0 = all properties hold.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "render_worklist.hpp"

namespace wl = ac_worklist;

static int g_fail = 0;
#define CHECK(COND, ...) do { if (!(COND)) { if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++g_fail; } } while (0)

// the XCD of work index w, as the kernel has always dealt them: chunks of min(512, ceil(n / 8) rounded up to 8) consecutive indices, chunk c to XCD c % 8
static int xcd_of(int n, int w)
{
    int per = (n + 7) / 8;
    per = (per + 7) / 8 * 8;
    const int chunk = per < 512 ? per : 512;
    return (w / chunk) % 8;
}

static long check_shape(int policy, int n, int tiles, int pair_n, int waves)
{
    std::vector<uint32_t> words;
    wl::build(n, tiles, pair_n, waves, policy, words);
    CHECK(words.size() >= (size_t)wl::HEADER_WORDS, "no header");
    std::vector<int> cover((size_t)n * tiles, 0), next_tile((size_t)n, 0), next_seq((size_t)n, 0), done((size_t)n, 0), home((size_t)n, -1);
    uint32_t expect_off = 0;
    long items = 0;
    for (int xcd = 0; xcd < wl::XCDS; ++xcd) {
        const uint32_t off = words[xcd], cnt = words[wl::XCDS + xcd];
        CHECK(off == expect_off, "policy %d n %d: list of XCD %d starts at %u, expected %u", policy, n, xcd, off, expect_off);
        expect_off += cnt;
        CHECK((size_t)wl::HEADER_WORDS + 2 * ((size_t)off + cnt) <= words.size(), "list of XCD %d runs past the end", xcd);
        std::vector<int> first_order;                                          // rays in the order of their first items
        for (uint32_t t = 0; t < cnt; ++t) {
            const uint32_t ray = words[wl::HEADER_WORDS + 2 * ((size_t)off + t)], meta = words[wl::HEADER_WORDS + 2 * ((size_t)off + t) + 1];
            const int cb = wl::meta_begin(meta), ce = wl::meta_end(meta), seq = wl::meta_seq(meta);
            ++items;
            CHECK(ray < (uint32_t)n, "ray %u out of range", ray);
            if (ray >= (uint32_t)n) continue;
            // the work index this row was dealt as (pair launches: a0 b0 a1 b1 ...)
            const int w = pair_n ? 2 * (int)(ray % (uint32_t)pair_n) + (ray >= (uint32_t)pair_n ? 1 : 0) : (int)ray;
            CHECK(xcd_of(n, w) == xcd, "policy %d n %d: ray %u (work %d) on XCD %d, chunking says %d", policy, n, ray, w, xcd, xcd_of(n, w));
            CHECK(home[ray] == -1 || home[ray] == xcd, "ray %u on two lists", ray);
            home[ray] = xcd;
            CHECK(seq == next_seq[ray], "policy %d n %d tiles %d: ray %u item %d at ticket %u, expected item %d", policy, n, tiles, ray, seq, t, next_seq[ray]);
            CHECK(seq < wl::MAX_ITEMS, "too many items");
            CHECK(cb == next_tile[ray] && ce > cb && ce <= tiles, "policy %d n %d tiles %d: ray %u item %d covers [%d, %d), expected to start at %d", policy, n, tiles, ray, seq, cb, ce, next_tile[ray]);
            CHECK(((meta & wl::META_SAMPLING) != 0u) == (seq == 0), "sampling flag on item %d of ray %u", seq, ray);
            CHECK(!done[ray], "item behind the last one of ray %u", ray);
            CHECK(((meta & wl::META_LAST) != 0u) == (ce == tiles), "last flag of ray %u item %d", ray, seq);
            if (meta & wl::META_LAST) done[ray] = 1;
            for (int c = cb; c < ce && c < tiles; ++c) ++cover[(size_t)ray * tiles + c];
            next_tile[ray] = ce; next_seq[ray] = seq + 1;
            if (seq == 0) first_order.push_back((int)ray);
        }
        // closed form == builder: the tickets of a one-item launch, gaps skipped, name the same rays in the same order
        size_t k = 0;
        const int xchunk = wl::xcd_chunk(n);
        for (int t = 0;; ++t) {
            const int w = wl::ticket_to_work(n, xchunk, xcd, t);
            if (w == wl::TICKET_END) break;
            if (w == wl::TICKET_GAP) continue;
            CHECK(k < first_order.size() && first_order[k] == wl::work_to_ray(w, pair_n), "policy %d n %d: closed form and builder differ at ray %zu of XCD %d", policy, n, k, xcd);
            ++k;
            CHECK(t < n + 8 * 512, "closed form does not end");
            if (t >= n + 8 * 512) break;
        }
        CHECK(k == first_order.size(), "policy %d n %d: closed form names %zu rays on XCD %d, the builder %zu", policy, n, k, xcd, first_order.size());
    }
    CHECK((size_t)wl::HEADER_WORDS + 2 * (size_t)expect_off == words.size(), "words behind the last list");
    for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1, "policy %d n %d tiles %d pair %d: (ray %zu, tile %zu) covered %d times", policy, n, tiles, pair_n, i / tiles, i % tiles, cover[i]);
    for (int r = 0; r < n; ++r) CHECK(done[r] == 1, "ray %d has no last item", r);
    return items;
}

int main()
{
    const int counts[] = { 1, 8, 9, 511, 513, 2056, 4096 }, tile_counts[] = { 1, 4, 8 }, wave_counts[] = { 8, 256 };
    for (int policy = 0; policy < wl::N_POLICIES; ++policy) {
        long items = 0;
        int shapes = 0;
        for (int n : counts) for (int tiles : tile_counts) for (int waves : wave_counts) for (int pair = 0; pair < 2; ++pair) {
            if (pair && (n & 1)) continue;                                     // (a pair launch has an even number of work items)
            items += check_shape(policy, n, tiles, pair ? n / 2 : 0, waves);
            ++shapes;
        }
        std::printf("policy %d: %d shapes, %ld items, %d failures so far\n", policy, shapes, items, g_fail);
    }
    // policy 0 is the order the renderer shipped with before the lists: stage-major, boundaries floor(tiles * q / min(tiles, 4))
    for (int tiles = 1; tiles <= 8; ++tiles) {
        int b[wl::MAX_ITEMS + 1];
        const int nseg = tiles < 4 ? tiles : 4, got = wl::split_bounds(wl::policy_split(0, true, 0), tiles, b);
        CHECK(got == nseg, "policy 0, %d tiles: %d items, expected %d", tiles, got, nseg);
        for (int q = 0; q <= nseg && q <= got; ++q) CHECK(b[q] == (tiles * q) / nseg, "policy 0, %d tiles: boundary %d is %d", tiles, q, b[q]);
    }
    std::printf("%s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
