// avatarcraft_amd/csrc/render_fused.hip -- the fused Instant-NSR ray renderer for MI355X (gfx950).
//
// One launch = NeRFRenderer.run (reference models/instant_nsr.py:133-299, render_can=True) for a
// batch of rays; the reference runs the same work as ~11 forward_sdf calls x ~6 PyTorch kernels
// plus ~200 small sampling kernels, every intermediate through HBM.
//
// Mapping (wave64 / CDNA4 first):
//   * one wavefront owns one ray at a time; the ray's z / sdf arrays (<=128 entries) live in a
//     wave-private LDS slab, everything else in registers.
//   * a wave evaluates the field on TILES OF 16 SAMPLES: lane = (sample n = lane&15, group g = lane>>4).
//     Group g gathers hash levels {g, 4+g, 8+g, 12+g} (8 of the 32 features), so the features
//     of one sample are spread over 4 lanes exactly as the B operand of
//     v_mfma_f32_16x16x4_f32 wants them (B[k=lane>>4][j=lane&15]): NO LDS transpose between the
//     gather and the MLP.  Layers are computed transposed (D^T = W * X^T), so the D layout of
//     layer i (row = 4*(lane>>4)+reg) is directly the B operand of layer i+1 with the k-order
//     (t, r, g) -> unit 16t+4g+r: the whole 35-64-16 SDF MLP and 21-64-64-3 colour MLP chain
//     through registers.  f32-input MFMA is bit-for-bit an fp32 fma chain in k order, which is
//     what the CPU oracle evaluates (oracle/ac_oracle.c: orc_sdf_mlp / orc_color_mlp).
//   * weights are converted once per workgroup from row-major global memory into MFMA A-fragment
//     order in LDS (40 KB, shared by the 8 waves of the workgroup) and read with conflict-free
//     lane-linear ds_read_b32.
//   * per-ray cumprod / cumsum / reductions are 16-lane DPP Kogge-Stone scans (row_shr 1,2,4,8)
//     with a scalar carry between tiles = "wavefront segmented scan".
//   * NeuS up-sampling (up_sample + sample_pdf + cat_z_vals) runs inside the wave: 64-lane chunks
//     for the per-bin math, binary searches in LDS, rank-based stable merge instead of a sort.
//
// Numerics contract: see ac_devmath.hpp and DESIGN.md; every value produced here is bit-identical
// to oracle/ac_oracle.c:orc_render_rays on the same inputs.
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>
#include "sdf_mlp.hpp"
#include "field_stencil.hpp"
#include "field_color.hpp"
#include "render_slab.hpp"
#include "render_entry.hpp"
#include "render_worklist.hpp"      // (AC_XCD_CHUNK, AC_WORKLIST_POLICY and the XCD chunking live there, with the builder of the work lists)

namespace {

// a workgroup's waves on blocks of 8 consecutive rays (dynamic or static): 16 - 21 % slower than one ticket per wave -- profiles/r06_experiments.txt section 4c
// EX = false: a launch that wants the per-ray results only (image, weights_sum, depth, normal_map, eik): none of the optional per-sample outputs is
// compiled in, which takes their sixteen pointers (and the address arithmetic on them) out of the register budget of the tile loop
// SH = true: a field with view directions (ac_field.Wc1_sh).  A template parameter, not a run-time branch: the tile loop runs at 256 VGPRs with a few
// spilled registers, and the live pointer / flag of a run-time switch cost the DEFAULT model six more spills (+0.7 % on the headline launch, measured).
// the kernel's text lives in render_rays_kernel.hpp: one inclusion per table format (fp32 entries; the half table of ac_table_to_half)
#define AC_RENDER_KERNEL render_rays_kernel
#define AC_RENDER_H16 false
#include "render_rays_kernel.hpp"
#undef AC_RENDER_KERNEL
#undef AC_RENDER_H16
#define AC_RENDER_KERNEL render_rays_h16_kernel
#define AC_RENDER_H16 true
#include "render_rays_kernel.hpp"
#undef AC_RENDER_KERNEL
#undef AC_RENDER_H16

// ---- stand-alone field queries (density(), extract_geometry(), unit tests) -------------------------------
__global__ __launch_bounds__(BLOCK) void field_sdf_kernel(const RenderArgs a, const float *__restrict__ x, uint32_t B,
                                                          float *__restrict__ out16)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const FieldCtx fc = make_ctx(a);
    const uint32_t ntiles = (B + 15) / 16;
    for (uint32_t tile = blockIdx.x * WAVES_PER_BLOCK + wave; tile < ntiles; tile += gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t b = tile * 16 + n, bb = b < B ? b : B - 1;
        const float px = x[3 * bb], py = x[3 * bb + 1], pz = x[3 * bb + 2];
        const f32x4 o = sdf_tile(lds, fc, lane, px, py, pz);
        if (b < B) *reinterpret_cast<f32x4 *>(out16 + (size_t)b * 16 + 4 * g) = o;
    }
}

// dirs (use_viewdirs, with a.Wsh): the view direction of every point; the per-sample bias goes through a [4][64][4] slab per wave behind the weights
__global__ __launch_bounds__(BLOCK) void field_color_kernel(const RenderArgs a, const float *__restrict__ x, const float *__restrict__ dirs,
                                                            const float *__restrict__ nrm, const float *__restrict__ sdfout,
                                                            uint32_t B, float *__restrict__ rgb_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const uint32_t ntiles = (B + 15) / 16;
    float *slab = lds + OFF_WAVE + wave * 1024;
    for (uint32_t tile = blockIdx.x * WAVES_PER_BLOCK + wave; tile < ntiles; tile += gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t b = tile * 16 + n, bb = b < B ? b : B - 1;
        const f32x4 so = *reinterpret_cast<const f32x4 *>(sdfout + (size_t)bb * 16 + 4 * g);
        float rgb[3];
        if (dirs) {
            wave_sync();
            sample_sh_bias(slab, a.Wsh, dirs[3 * bb], dirs[3 * bb + 1], dirs[3 * bb + 2], lane);
            color_tile(lds, lane, x[3 * bb], x[3 * bb + 1], x[3 * bb + 2], nrm[3 * bb], nrm[3 * bb + 1], nrm[3 * bb + 2], so, rgb, slab + 4 * lane, 256);
        } else
        color_tile(lds, lane, x[3 * bb], x[3 * bb + 1], x[3 * bb + 2], nrm[3 * bb], nrm[3 * bb + 1], nrm[3 * bb + 2], so, rgb);
        if (b < B && g == 0) { rgb_out[3 * b] = rgb[0]; rgb_out[3 * b + 1] = rgb[1]; rgb_out[3 * b + 2] = rgb[2]; }
    }
}

// ac_field_prepare: one workgroup lays the weights out in LDS exactly like a render workgroup would and dumps the image
__global__ __launch_bounds__(BLOCK) void field_prepare_kernel(const RenderArgs a, float *__restrict__ image)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    fill_lds_fast(lds, a);
    fill_lds_color_fast<false, true>(lds, a);                 // the two fragments outside the overlay
    __syncthreads();
    for (int e = threadIdx.x; e < OFF_RWAVE; e += blockDim.x) image[e] = lds[e];
    __syncthreads();
    fill_lds_color_fast<true, false>(lds, a);                 // the overlay of the colour region (fast precision), kept behind the exact image
    __syncthreads();
    for (int e = threadIdx.x; e < CF_OVERLAY; e += blockDim.x) image[OFF_RWAVE + e] = lds[OFF_C1F + e];
}

// gradient_error: fixed-order reduction of per-ray partials (oracle: orc_eikonal_reduce)
__global__ __launch_bounds__(1024) void eikonal_reduce_kernel(const float *__restrict__ eik, int n_rays, float *__restrict__ result, int with_den)
{
    __shared__ float pn[1024], pd[1024];
    const int t = threadIdx.x;
    float a = 0.0f, b = 0.0f;
    for (int r = t; r < n_rays; r += 1024) { a += eik[2 * r]; b += eik[2 * r + 1]; }
    pn[t] = a; pd[t] = b;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) { pn[t] += pn[t + s]; pd[t] += pd[t + s]; }
        __syncthreads();
    }
    if (t == 0) { result[0] = pn[0] / (pd[0] + 1e-5f); if (with_den) result[1] = pd[0] + 1e-5f; }
}

}  // namespace

#ifdef AC_PROFILE
static unsigned long long *g_prof = nullptr;
AC_API void ac_debug_set_prof(unsigned long long *p) { g_prof = p; }
#endif

// posed-space coarse samples: pts[n, i] = o + d * z_i (unclamped, fp32), the input of the first warp  (:155-165)
__global__ __launch_bounds__(256) void coarse_pts_kernel(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                         const float *__restrict__ near_m, const float *__restrict__ far_m,
                                                         const float *__restrict__ lin_z, const float *__restrict__ noise, int n_rays, int T0,
                                                         float bound, int perturb, float *__restrict__ pts)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rays * T0) return;
    const int ray = idx / T0, i = idx - ray * T0;
    const float ox = rays_o[3 * ray], oy = rays_o[3 * ray + 1], oz = rays_o[3 * ray + 2];
    const float dx = rays_d[3 * ray], dy = rays_d[3 * ray + 1], dz = rays_d[3 * ray + 2];
    float near, far;
    cube_near_far(ox, oy, oz, dx, dy, dz, bound, near, far);
    if (near_m) {
        const float nm = near_m[ray], fm = far_m[ray];
        if (!is_inf(nm)) near = nm;
        if (!is_inf(fm)) far = fm;
    }
    const float span = far - near;
    const float sample_dist = span / (float)T0;
    float zi = near + span * lin_z[i];
    if (perturb) zi = zi + (noise[idx] - 0.5f) * sample_dist;
    pts[3 * (size_t)idx] = ox + dx * zi; pts[3 * (size_t)idx + 1] = oy + dy * zi; pts[3 * (size_t)idx + 2] = oz + dz * zi;
}

// Per-launch scratch of the dynamic hand-out: [8 XCDs] ticket counters, 32 bytes apart (256 B) | finished-workgroup counter | timed-out hand-offs |
// flags [N] u32 | state [N][SEG_STATE] f32.
// One slot per (device, stream), grown to the largest batch it has served and kept for the life of the process: launches of one stream run in order, so a
// slot is never in use by two launches at once, however many streams render concurrently.
// The slot also keeps the device copies of the work lists (render_worklist.hpp) of the last few launch shapes it has served -- a view rendered in batches
// alternates between two (the last batch differs) --: a list is built and uploaded once, on the launch's stream, from a pinned buffer that belongs to the
// entry and is never written again; both buffers are freed only after the upload's event has completed.
struct WorkList { int n_rays, tiles, pair_n, waves; uint32_t *dev, *host; hipEvent_t uploaded; uint64_t last_use; };
constexpr size_t WORKLISTS_PER_SLOT = 4;
struct SegSlot { char *p; size_t bytes; uint32_t gen; uint64_t last_use; std::vector<WorkList> lists; };
constexpr size_t SEG_POOL_MAX = 32;        // (device, stream) slots kept; beyond that the least recently used one is freed (stream churn must not grow device memory without bound)
static std::mutex g_seg_mu;
static std::map<std::pair<int, hipStream_t>, SegSlot> g_seg_pool;
static uint64_t g_seg_clock = 0;
static void free_worklist(WorkList &w)
{
    if (w.uploaded) { (void)hipEventSynchronize(w.uploaded); (void)hipEventDestroy(w.uploaded); }       // no copy can still be reading the host buffer
    if (w.dev) (void)hipFree(w.dev);
    if (w.host) (void)hipHostFree(w.host);
    w.dev = w.host = nullptr; w.uploaded = nullptr;
}
// the device copy of the work lists of this launch shape on the slot of (current device, stream); NULL: out of memory.  Call after seg_scratch (which makes the slot).
static const uint32_t *seg_worklist(int n_rays, int tiles, int pair_n, int waves, hipStream_t stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    std::lock_guard<std::mutex> lock(g_seg_mu);
    auto it = g_seg_pool.find(std::make_pair(dev, stream));
    if (it == g_seg_pool.end()) return nullptr;
    std::vector<WorkList> &ls = it->second.lists;
    for (WorkList &w : ls)
        if (w.n_rays == n_rays && w.tiles == tiles && w.pair_n == pair_n && w.waves == waves) { w.last_use = ++g_seg_clock; return w.dev; }
    if (ls.size() >= WORKLISTS_PER_SLOT) {
        size_t v = 0;
        for (size_t i = 1; i < ls.size(); ++i) if (ls[i].last_use < ls[v].last_use) v = i;
        free_worklist(ls[v]);                                            // (hipFree waits for the device: no launch can still be reading the list)
        ls.erase(ls.begin() + (long)v);
    }
    std::vector<uint32_t> words;
    ac_worklist::build(n_rays, tiles, pair_n, waves, AC_WORKLIST_POLICY, words);
    WorkList w{ n_rays, tiles, pair_n, waves, nullptr, nullptr, nullptr, ++g_seg_clock };
    const size_t bytes = words.size() * sizeof(uint32_t);
    if (hipMalloc(reinterpret_cast<void **>(&w.dev), bytes) != hipSuccess) { w.dev = nullptr; (void)hipGetLastError(); return nullptr; }
    if (hipHostMalloc(reinterpret_cast<void **>(&w.host), bytes, hipHostMallocDefault) != hipSuccess) { w.host = nullptr; (void)hipGetLastError(); free_worklist(w); return nullptr; }
    std::copy(words.begin(), words.end(), w.host);
    if (hipEventCreateWithFlags(&w.uploaded, hipEventDisableTiming) != hipSuccess) { w.uploaded = nullptr; free_worklist(w); return nullptr; }
    if (hipMemcpyAsync(w.dev, w.host, bytes, hipMemcpyHostToDevice, stream) != hipSuccess || hipEventRecord(w.uploaded, stream) != hipSuccess) {
        (void)hipStreamSynchronize(stream); free_worklist(w); return nullptr;
    }
    ls.push_back(w);
    return w.dev;
}
// -> the slot's memory and the generation of this launch (1 .. 2^28 - 1): a slot is zeroed when it is allocated; after that every launch leaves its
// counters at zero (the kernel's last workgroup re-arms them) and tags its per-ray flags with its generation, so nothing is cleared between launches
static char *seg_scratch(size_t need, uint32_t &gen, hipStream_t stream)
{
    std::mutex &mu = g_seg_mu;
    auto &pool = g_seg_pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, stream);
    if (pool.find(key) == pool.end() && pool.size() >= SEG_POOL_MAX) {   // evict the least recently used slot (hipFree waits for the device: nothing can still use it)
        auto victim = pool.begin();
        for (auto it = pool.begin(); it != pool.end(); ++it) if (it->second.last_use < victim->second.last_use) victim = it;
        if (victim->second.p) (void)hipFree(victim->second.p);
        for (WorkList &w : victim->second.lists) free_worklist(w);
        pool.erase(victim);
    }
    SegSlot &sl = pool[key];
    sl.last_use = ++g_seg_clock;
    if (sl.bytes < need) {
        if (sl.p) (void)hipFree(sl.p);                                   // (synchronises the device: no launch can still be using the slot)
        sl.p = nullptr; sl.bytes = 0; sl.gen = 0;
        const size_t want = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
        if (hipMalloc(reinterpret_cast<void **>(&sl.p), want) != hipSuccess) { sl.p = nullptr; return nullptr; }
        // (on the launch's own stream: ordered before the kernel that is about to use the slot -- a null-stream memset is not, for non-blocking streams)
        if (hipMemsetAsync(sl.p, 0, want, stream) != hipSuccess) { (void)hipFree(sl.p); sl.p = nullptr; return nullptr; }
        sl.bytes = want;
    }
    sl.gen = (sl.gen + 1u) & 0x0fffffffu;
    if (sl.gen == 0u) {                                                  // wrapped: flags of 2^28 launches ago could match again -- start over from zeroed memory
        if (hipMemsetAsync(sl.p, 0, sl.bytes, stream) != hipSuccess) return nullptr;
        sl.gen = 1u;
    }
    gen = sl.gen;
    return sl.p;
}

// hand-offs that timed out (a taker waited ~1 s for a segment that was never published: its pixel is NaN) on the slot of (current device, stream), over
// the life of that slot; waits for the stream.  0 on a healthy run -- the GPU tier asserts it after its soak and co-residency tests.
AC_API int ac_render_handoff_timeouts(ac_stream_t stream, uint32_t *count)
{
    if (!count) { ac::set_error("render_handoff_timeouts: NULL count"); return AC_ERR_BAD_ARG; }
    *count = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    char *p = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_seg_mu);
        auto it = g_seg_pool.find(std::make_pair(dev, (hipStream_t)stream));
        if (it != g_seg_pool.end()) p = it->second.p;
    }
    if (!p) return AC_OK;                                                // no render has run on this stream
    if (hipMemcpyAsync(count, p + 260, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { ac::set_error("render_handoff_timeouts: copy failed"); return AC_ERR_LAUNCH; }
    return AC_OK;
}

template <int MODE, bool FAST, bool EX, bool SH = false, bool H16 = false>
static void launch_render_p(const RenderArgs &a, hipStream_t stream)
{
    const auto kernel = H16 ? render_rays_h16_kernel<MODE, FAST, EX, SH> : render_rays_kernel<MODE, FAST, EX, SH>;
    int blocks = (a.n_rays + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    static uint64_t seen = 0;                       // one flag per instantiation
    const size_t lds_bytes = LDS_FLOATS * sizeof(float);
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(kernel), lds_bytes);
    RenderArgs b = a;
    {
        // MODE_FULL: a ray's tiles are cut into items by the work lists of render_worklist.hpp (policy AC_WORKLIST_POLICY), whatever the tile count
        // (posed space: the two halves stay with whole rays and decode their tickets in closed form, no list -- their ray count changes from frame to
        //  frame; with skip_masked most tiles of the final pass are skipped anyway, and segments measured 8 % slower there)
        const int nt = (a.T0 + 16 * a.nup) / 16;
        const bool listed = MODE == MODE_FULL;
        const size_t N = (size_t)a.n_rays, head = 512, flags = (N * 4 + 255) & ~(size_t)255;      // head: [0, 256) ticket counters | [256] finished workgroups | [260] timeouts
        const size_t need = head + (listed ? flags + N * SEG_STATE * sizeof(float) : 0);
        uint32_t gen = 0;
        char *sc = seg_scratch(need, gen, stream);
        const int cus = (int)ac::cu_count();
        if (blocks > cus) blocks = cus;
        blocks = (blocks + 7) & ~7;                                      // every XCD gets the same number of workgroups
        b.work_list = (listed && sc) ? seg_worklist(a.n_rays, nt, a.pair_n, (blocks / 8) * WAVES_PER_BLOCK, stream) : nullptr;
        if (listed && !b.work_list) sc = nullptr;
        b.ray_counter = reinterpret_cast<uint32_t *>(sc);
        b.done_counter = sc ? reinterpret_cast<uint32_t *>(sc + 256) : nullptr;
        b.handoff_timeouts = sc ? reinterpret_cast<uint32_t *>(sc + 260) : nullptr;      // (never re-armed: counts over the life of the slot)
        b.gen = gen;
        b.eik_red = (MODE == MODE_UPSAMPLE) ? nullptr : a.out.eik_reduced;
        b.seg_flags = (listed && sc) ? reinterpret_cast<uint32_t *>(sc + head) : nullptr;
        b.seg_state = (listed && sc) ? reinterpret_cast<float *>(sc + head + flags) : nullptr;
        if (!sc) blocks = 0;                                             // (the scratch could not be allocated: an empty grid is a launch error the caller reports)
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), lds_bytes, stream, b);
}
// h16: a.table is the half table (the ac_*_h16 entries): the same instantiations of the kernel's second inclusion
template <int MODE>
static void launch_render(const RenderArgs &a, hipStream_t stream, bool h16 = false)
{
    const bool ex = wants_samples(a.out);
    if constexpr (MODE != MODE_UPSAMPLE) {          // (the sampling-only launch has no finite-difference stage)
        // a field with view directions has its own instantiations (see the kernel's SH parameter)
        dispatch_variants(a.fast, ex, a.Wsh != nullptr, [&](auto fast, auto ex_, auto sh) {
            if (h16) launch_render_p<MODE, decltype(fast)::value, decltype(ex_)::value, decltype(sh)::value, true>(a, stream);
            else launch_render_p<MODE, decltype(fast)::value, decltype(ex_)::value, decltype(sh)::value>(a, stream);
        });
        return;
    }
    const bool inds = a.out.ss_inds || a.out.sort_index;                                       // (the sampling-only launch can export the sample indices)
    if (h16) { if (inds) launch_render_p<MODE, false, true, false, true>(a, stream); else launch_render_p<MODE, false, false, false, true>(a, stream); }
    else if (inds) launch_render_p<MODE, false, true>(a, stream);
    else launch_render_p<MODE, false, false>(a, stream);
}

// ---- the half table (include/avatarcraft_hip.h: ac_table_to_half) ---------------------------------------------------------------------------------
// one dword per entry: channel 0 in the low half, channel 1 in the high half; fp32 -> fp16 by v_cvt_f16_f32 (round to nearest even, subnormals kept,
// NaN stays NaN); n_bad += entries in which a finite value became +-inf
__global__ __launch_bounds__(256) void table_to_half_kernel(const float2 *__restrict__ table, uint32_t n_entries, uint32_t *__restrict__ out, uint32_t *__restrict__ n_bad)
{
    uint32_t bad = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_entries; i += gridDim.x * blockDim.x) {
        const float2 v = table[i];
        const _Float16 h0 = (_Float16)v.x, h1 = (_Float16)v.y;
        const uint32_t b0 = __builtin_bit_cast(unsigned short, h0), b1 = __builtin_bit_cast(unsigned short, h1);
        out[i] = b0 | (b1 << 16);
        const bool o0 = (b0 & 0x7fffu) == 0x7c00u && !is_inf(v.x), o1 = (b1 & 0x7fffu) == 0x7c00u && !is_inf(v.y);      // (a NaN keeps a non-zero mantissa)
        bad += (o0 || o1) ? 1u : 0u;
    }
    if (bad) atomicAdd(n_bad, bad);
}

AC_API int ac_table_to_half(const float *table, uint32_t n_entries, void *table_h16, uint32_t *n_bad, ac_stream_t stream)
{
    if (n_entries == 0) return AC_OK;
    if (!table || !table_h16 || !n_bad) { ac::set_error("table_to_half: NULL buffer"); return AC_ERR_BAD_ARG; }
    uint32_t blocks = (n_entries + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    hipLaunchKernelGGL(table_to_half_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2 *>(table), n_entries,
                       static_cast<uint32_t *>(table_h16), n_bad);
    return ac::check_launch("table_to_half");
}

static_assert(SHORT_MAX_T == MAXT, "the short window is this kernel's slab");

AC_API int ac_render_rays(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                          const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                          const ac_render_out *out, ac_stream_t stream)
{
    static const RenderEntry d("render_rays", 0);
    const RayInputs in = { rays_o, rays_d, bg, noise, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, nullptr, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, out)) return rc;
#ifdef AC_PROFILE
    a.prof = g_prof;
#endif
    launch_render<MODE_FULL>(a, (hipStream_t)stream);
    return ac::check_launch(d.name);
}

// ac_render_rays from the half table: the same launch on the kernel's half-table inclusion
AC_API int ac_render_rays_h16(const ac_field *field, const void *table_h16, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                              const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                              const ac_render_out *out, ac_stream_t stream)
{
    static const RenderEntry d("render_rays_h16", K_H16);
    const RayInputs in = { rays_o, rays_d, bg, noise, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, table_h16, op, in, nullptr, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, table_h16, op, in, out)) return rc;
    launch_render<MODE_FULL>(a, (hipStream_t)stream, true);
    return ac::check_launch(d.name);
}

// The same N rays rendered twice in one launch, with two draws of the jitter noise and two backgrounds: what one stylisation step does with net_style
// (stylize.py:98-116 render_val under no_grad, then :143-152 the differentiable render of the same rays) -- two calls of run() in the reference, two launches
// of ac_render_rays before round 3.  The 2N work items are handed out as a0 b0 a1 b1 ...: the two copies of a ray walk through (nearly) the same grid
// cells at (nearly) the same time on the same XCD, so the second finds most table sectors in L2 (-11 % on the stride-4 training view, where neighbouring
// rays share little: profiles/r03_experiments.txt).  Every result is bit-identical to two separate launches (the rays are independent).
// noise [2][N][num_steps], bg [2][N][3] (or NULL); out: the per-ray arrays hold 2N rows ([0, N) copy a, [N, 2N) copy b); the optional per-sample
// arrays are written for copy b only and hold N rows.
AC_API int ac_render_rays_pair(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                               const float *bg2, const float *noise2, const float *lin_z, const float *lin_u,
                               const ac_render_out *out, ac_stream_t stream)
{
    static const RenderEntry d("render_rays_pair", K_PAIR);
    const RayInputs in = { rays_o, rays_d, bg2, noise2, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, nullptr, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, out)) return rc;
    make_pair_args(a);
    launch_render<MODE_FULL>(a, (hipStream_t)stream);
    return ac::check_launch(d.name);
}

// the sampling stage alone (coarse z, coarse sdf, NeuS up-sampling): what the reference computes under no_grad before the
// differentiable render core (instant_nsr.py:155-184)
AC_API int ac_sample_rays(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d, const float *noise,
                          const float *lin_z, const float *lin_u, float *z_vals, ac_stream_t stream)
{
    static const RenderEntry d("sample_rays", K_SAMPLING);
    const RayInputs in = { rays_o, rays_d, nullptr, noise, lin_z, lin_u };
    if (int rc = check_render_entry(d, field, nullptr, op, in, nullptr, nullptr, z_vals)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, nullptr, op, in, nullptr)) return rc;
    a.zbuf = z_vals;
    launch_render<MODE_UPSAMPLE>(a, (hipStream_t)stream);
    return ac::check_launch(d.name);
}

// scratch layout of ac_render_rays_warped (byte offsets, 256-byte aligned): near_m, far_m [N] f32; pts, can [N,T,3] f32;
// mask [N,T] u8; zbuf [N,T] f32; behind the six documented segments: ray_dead [N] u8 (skip_masked)
AC_API size_t ac_render_rays_warped_scratch(int32_t n_rays, int32_t T, size_t offs[6])
{
    size_t o[7];
    const size_t need = warped_scratch_offsets(n_rays, T, o);
    if (offs) std::copy(o, o + 6, offs);
    return need;
}

// the helpers of the posed sequence (render_entry.hpp: render_posed); ac:: linkage (ac_common.hpp) because ac_render_rays_long_warped (render_long.hip) runs it too
int ac::warped_coarse_pts(const char *who, const float *rays_o, const float *rays_d, const float *near_m, const float *far_m, const float *lin_z, const float *noise,
                          int n_rays, int T0, float bound, int perturb, float *pts, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_pts_kernel, dim3((n_rays * T0 + 255) / 256), dim3(256), 0, st, rays_o, rays_d, near_m, far_m, lin_z, noise, n_rays, T0, bound, perturb, pts);
    return ac::check_launch(who);
}

int ac::warp_any(const ac_warp_mesh *m, const float *pts, uint32_t P, float *can, uint8_t *mask, ac_stream_t stream, int skip_far,
                 const uint8_t *ray_dead, uint32_t spr, uint32_t seed_off)
{
    if (m->accel) {
        // temporal seeds (ac_warp_mesh.seed_faces): this search's columns [seed_off, seed_off + spr) of the caller's per-ray rows
        int32_t *ts = (m->seed_faces && m->seed_stride >= seed_off + spr && spr > 0) ? m->seed_faces : nullptr;
        return ac::warp_samples_accel_impl(pts, m->verts, m->faces, m->T, P, m->V, m->F, m->threshold, m->accel, nullptr, can, nullptr, nullptr, nullptr,
                                           mask, stream, skip_far, ray_dead, spr, ts, m->seed_stride, seed_off);
    }
    return ac_warp_samples(pts, m->verts, m->faces, m->T, P, m->V, m->F, m->threshold, nullptr, can, nullptr, nullptr, nullptr, mask, stream);
}

// Measurement hook (bench.py's posed-frame roofline): with ac_debug_warped_phases(1) every posed render (render_posed) records HIP events on its stream
// at the phase boundaries -- [0] start, [1] near / far + coarse points + ray cull, [2] first warp search, [3] up-sampling pass, [4] second warp search,
// [5] final pass -- and ac_debug_warped_phase_ms() returns the five intervals of the LAST call in ms (it waits for that call).  Off by default.
namespace {
hipEvent_t g_phase_ev[6];
int g_phase_on = 0, g_phase_have = 0;
}
void ac::warped_phase_mark(int k, hipStream_t st) { if (g_phase_on) { (void)hipEventRecord(g_phase_ev[k], st); if (k == 5) g_phase_have = 1; } }
AC_API void ac_debug_warped_phases(int enable)
{
    if (enable && !g_phase_on) for (auto &e : g_phase_ev) (void)hipEventCreate(&e);
    if (!enable && g_phase_on) { for (auto &e : g_phase_ev) (void)hipEventDestroy(e); g_phase_have = 0; }
    g_phase_on = enable ? 1 : 0;
}
AC_API int ac_debug_warped_phase_ms(float out[5])
{
    if (!g_phase_on || !g_phase_have) { ac::set_error("ac_debug_warped_phase_ms: no instrumented ac_render_rays_warped call yet"); return AC_ERR_BAD_ARG; }
    if (hipEventSynchronize(g_phase_ev[5]) != hipSuccess) { ac::set_error("ac_debug_warped_phase_ms: event wait failed"); return AC_ERR_LAUNCH; }
    for (int k = 0; k < 5; ++k) { out[k] = 0.0f; (void)hipEventElapsedTime(out + k, g_phase_ev[k], g_phase_ev[k + 1]); }
    return AC_OK;
}

// the posed entries of the short window: render_posed on this kernel's two halves; h16: both passes gather from the half table
static int render_rays_warped_any(const RenderEntry &d, const ac_field *field, const void *table_h16, const ac_render_opts *op, const RayInputs &in,
                                  const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out, ac_stream_t stream)
{
    if (int rc = check_render_entry(d, field, table_h16, op, in, mesh, out)) return rc;
    if (op->n_rays <= 0) return AC_OK;
    RenderArgs a{};
    if (int rc = fill_entry_args(a, field, table_h16, op, in, out)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    return render_posed(d, a, mesh, scratch, scratch_bytes, stream, [&](const RenderArgs &b) { launch_render<MODE_UPSAMPLE>(b, st, d.h16); },
                        [&](const RenderArgs &b) { launch_render<MODE_FINAL>(b, st, d.h16); });
}

AC_API int ac_render_rays_warped(const ac_field *field, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                                 const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                                 const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out,
                                 ac_stream_t stream)
{
    static const RenderEntry d("render_rays_warped", K_POSED);
    return render_rays_warped_any(d, field, nullptr, op, { rays_o, rays_d, bg, noise, lin_z, lin_u }, mesh, scratch, scratch_bytes, out, stream);
}

// ac_render_rays_warped from the half table (same scratch: ac_render_rays_warped_scratch)
AC_API int ac_render_rays_warped_h16(const ac_field *field, const void *table_h16, const ac_render_opts *op, const float *rays_o, const float *rays_d,
                                     const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                                     const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out,
                                     ac_stream_t stream)
{
    static const RenderEntry d("render_rays_warped_h16", K_POSED | K_H16);
    return render_rays_warped_any(d, field, table_h16, op, { rays_o, rays_d, bg, noise, lin_z, lin_u }, mesh, scratch, scratch_bytes, out, stream);
}

static_assert((OFF_RWAVE + CF_OVERLAY) * sizeof(float) <= AC_FIELD_PREPARED_BYTES && OFF_C1F % 4 == 0 && OFF_B1 % 4 == 0 && OFF_RWAVE % 4 == 0, "the prepared image fits its buffer");
AC_API int ac_field_prepare(const ac_field *field, void *prepared, ac_stream_t stream)
{
    if (!prepared) { ac::set_error("field_prepare: NULL buffer"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = fill_args(a, field, 1.0f)) return rc;
    a.T0 = 0; a.lin_z = nullptr; a.lin_u = nullptr;            // the sampling tables are per launch, not part of the image
    const size_t lds_bytes = OFF_RWAVE * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(field_prepare_kernel), lds_bytes);
    hipLaunchKernelGGL(field_prepare_kernel, dim3(1), dim3(BLOCK), lds_bytes, (hipStream_t)stream, a, static_cast<float *>(prepared));
    return ac::check_launch("field_prepare");
}

AC_API int ac_eikonal_reduce(const float *eik, int32_t n_rays, float *result, ac_stream_t stream)
{
    if (!result || n_rays < 0 || (!eik && n_rays > 0)) { ac::set_error("eikonal_reduce: bad argument"); return AC_ERR_BAD_ARG; }
    hipLaunchKernelGGL(eikonal_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, eik, n_rays, result, 0);
    return ac::check_launch("eikonal_reduce");
}

AC_API int ac_eikonal_reduce2(const float *eik, int32_t n_rays, float *result2, ac_stream_t stream)
{
    if (!result2 || n_rays < 0 || (!eik && n_rays > 0)) { ac::set_error("eikonal_reduce2: bad argument"); return AC_ERR_BAD_ARG; }
    hipLaunchKernelGGL(eikonal_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, eik, n_rays, result2, 1);
    return ac::check_launch("eikonal_reduce2");
}

AC_API int ac_field_sdf(const ac_field *field, const float *x, uint32_t B, float bound, float *out16, ac_stream_t stream)
{
    if (B == 0) return AC_OK;
    if (!x || !out16) { ac::set_error("field_sdf: NULL buffer"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = fill_args(a, field, bound)) return rc;
    a.T0 = 0;
    const size_t lds_bytes = OFF_WAVE * sizeof(float);
    const uint32_t ntiles = (B + 15) / 16;
    uint32_t blocks = (ntiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(field_sdf_kernel, dim3(blocks), dim3(BLOCK), lds_bytes, (hipStream_t)stream, a, x, B, out16);
    return ac::check_launch("field_sdf");
}

AC_API int ac_field_color_dirs(const ac_field *field, const float *x, const float *dirs, const float *n, const float *sdfout, uint32_t B, float *rgb,
                               ac_stream_t stream)
{
    if (B == 0) return AC_OK;
    if (!x || !n || !sdfout || !rgb) { ac::set_error("field_color: NULL buffer"); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = fill_args(a, field, 1.0f)) return rc;
    if (a.Wsh && !dirs) { ac::set_error("field_color: the field has view-direction weights (ac_field.Wc1_sh): pass the directions (ac_field_color_dirs)"); return AC_ERR_BAD_ARG; }
    if (!a.Wsh) dirs = nullptr;
    a.T0 = 0;
    const size_t lds_bytes = (OFF_WAVE + (dirs ? WAVES_PER_BLOCK * 1024 : 0)) * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(field_color_kernel), (OFF_WAVE + WAVES_PER_BLOCK * 1024) * sizeof(float));
    const uint32_t ntiles = (B + 15) / 16;
    uint32_t blocks = (ntiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(field_color_kernel, dim3(blocks), dim3(BLOCK), lds_bytes, (hipStream_t)stream, a, x, dirs, n, sdfout, B, rgb);
    return ac::check_launch("field_color");
}

AC_API int ac_field_color(const ac_field *field, const float *x, const float *n, const float *sdfout, uint32_t B, float *rgb,
                          ac_stream_t stream)
{
    return ac_field_color_dirs(field, x, nullptr, n, sdfout, B, rgb, stream);
}
