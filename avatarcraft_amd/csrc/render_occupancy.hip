// avatarcraft_amd/csrc/render_occupancy.hip -- the occupancy-grid renderers: what stands in for NeRFRenderer.run_cuda of the reference (whose run_cuda is
// undefined for this network), built from the marcher (rm_device.hpp), the field on packed samples (field_tile.hpp) and the packed compositors.
//   field_samples_kernel      : packed samples -> alpha, rgb, normal (ac_field_samples: between march_rays and composite_rays of raymarching.hip)
//   occupancy_render_kernel   : the inference render as one launch, a wave per group of rays (ac_render_rays_occupancy)
//   occupancy_phased_kernel   : the same render in rounds of march | field | composite with grid barriers, tiles dealt to all waves (..._phased)
//   occupancy_train_kernel    : the training render without autograd as one launch of four phases (..._train)
//   packed_shading_fwd / bwd  : the shading glue of the training form under autograd (ac_packed_shading_forward / _backward)
// Every form gives a sample, and a ray, the bits of the chain of stand-alone operators (tests/test_gpu_run_cuda.py, tests/test_gpu_marcher_edges.py).
#include <atomic>
#include "field_tile.hpp"
#include "field_host.hpp"
#include "rm_device.hpp"

namespace {

// ---- field evaluation on PACKED samples: what stands between the occupancy-grid marcher and the packed compositor (run_cuda) -------------------
// One tile = 16 samples of whatever rays (the marcher lays a ray's samples out consecutively) through field_tile.
struct SampleArgs {
    const float *xyzs, *dirs, *deltas;          // [M,3] [M,3] [M * dstride] (march_rays_train: dstride 1; march_rays: dstride 2, column 0 = the step)
    uint32_t dstride, M;
    float *alpha, *rgb, *normal;                // [M] [M,3] [M,3]
    float *sdf, *gradient;                      // optional [M] [M,3] (the raw finite-difference gradient: eikonal term)
};

__global__ __launch_bounds__(FBLOCK) void field_samples_kernel(const RenderArgs a, const SampleArgs s)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float inv_s = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
    const uint32_t ntiles = (s.M + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < s.M ? b : s.M - 1;
        const float *x = s.xyzs + 3 * (size_t)bb, *d = s.dirs + 3 * (size_t)bb;
        float alpha, rgb[3], nrm[3], sdf0, gr[3], gn;
        field_tile(lds, fsl, fc, a, lane, x[0], x[1], x[2], d[0], d[1], d[2], s.deltas[(size_t)bb * s.dstride], inv_s, alpha, rgb, nrm, sdf0, gr, gn);
        if (b < s.M && g == 0) {
            s.alpha[b] = alpha;
            s.rgb[3 * (size_t)b] = rgb[0]; s.rgb[3 * (size_t)b + 1] = rgb[1]; s.rgb[3 * (size_t)b + 2] = rgb[2];
            s.normal[3 * (size_t)b] = nrm[0]; s.normal[3 * (size_t)b + 1] = nrm[1]; s.normal[3 * (size_t)b + 2] = nrm[2];
            if (s.sdf) s.sdf[b] = sdf0;
            if (s.gradient) { s.gradient[3 * (size_t)b] = gr[0]; s.gradient[3 * (size_t)b + 1] = gr[1]; s.gradient[3 * (size_t)b + 2] = gr[2]; }
        }
        wave_sync();
    }
}

// ---- the march of the two inference launches ----------------------------------------------------------------------------------------------------
// One ray's next samples, at most `room` of them and never beyond its cap of max_steps (0: none) in all: march_rays_kernel's loop body.  put(x, y, z, dt, dl1)
// receives each sample with the marcher's second delta dl1 = t_after - last_t.  Returns their number; ended: the walk is over (t >= far: composite_rays would
// meet dl[0] == 0 here) or the cap is reached -- the samples of this call are still composited.
template <class Put>
__device__ __forceinline__ uint32_t occ_march(const RayCtx &c, float &t, float &last_t, float &skip_tt, float far, uint32_t room, uint32_t max_steps,
                                              uint32_t &taken, const float *etab, bool &ended, Put &&put)
{
    if (max_steps && max_steps - taken < room) room = max_steps - taken;        // (taken < max_steps while the ray is alive)
    const uint32_t room0 = room;
    auto emit = [&](float x, float y, float z, float dt, float t_after, uint32_t) {
        put(x, y, z, dt, t_after - last_t);
        last_t = t_after;
    };
    bool more = true;                                                           // grid look-ups RM_BATCH at a time (rm_march_batch): the reference's walk, fewer round trips
    uint32_t kpos = 0;
    while (room > 0 && more) more = rm_march_batch<RM_BATCH>(c, t, skip_tt, far, room, kpos, emit, etab);
    taken += room0 - room;
    ended = !more || (max_steps && taken >= max_steps);
    return room0 - room;
}

// ---- the occupancy-grid INFERENCE render as one launch (round 4): march + field + composite per ray, no host round trips -----------------------------
// What NeRFRenderer.run_cuda's eval() loop computes in rounds of compact_rays / march_rays / ac_field_samples / composite_rays (one 4-byte D2H per round),
// computed as if it were ONE round with n_step = 1024: lane = ray.  Per iteration every alive lane marches to its NEXT occupied sample (the body of
// march_rays_kernel, raymarching.hip), the samples of the wave's alive rays are packed into tiles of 16 (ballot ranks through an LDS stage), the tiles go through
// the renderer's stencil gather / MLP / colour / alpha code (the body of field_samples_kernel), and every lane composites its own sample in order (the body of
// composite_rays_kernel: T = 1 - weights_sum, early stop at T < 1e-2).  Bit-identical to the three stand-alone operators run with n_step = 1024.
constexpr int OC_STAGE = 10 * 64;                  // per-wave stage: 64 sample slots x 8 floats (in: x y z dt . . . dl1 | out: alpha r g b nx ny nz, dl1 kept) + slot map [64] + lane map [64]
constexpr int OCC_LDS_FLOATS = FWD_LDS_FLOATS + FW * OC_STAGE;
static_assert(OCC_LDS_FLOATS * 4 + 256 <= 160 * 1024, "LDS budget (+ the training form's static words)");
struct OccArgs {
    const float *rays_o, *rays_d, *grid;
    uint32_t N, H;
    float mean_density;
    float *weights_sum, *depth, *image, *normal_map;     // [N] [N] [N,3] [N,3]: accumulators as composite_rays leaves them (background / depth normalisation: the caller)
    uint32_t *n_samples;                                   // optional [1]: total samples evaluated (atomic, one add per wave)
    uint32_t glog;                                         // a wave marches 2^glog rays at a time (lanes 0 .. 2^glog - 1); the 64 sample slots of an iteration (4 tiles) are
                                                           // shared out among the rays still alive: 64 / alive each -- the last, long rays of a group get whole tiles
    uint32_t max_steps;                                    // a ray stops after this many samples (run_cuda's max_steps; the loop of rounds stops at the first round that
                                                           // brings its step count to >= max_steps, i.e. after max_steps .. max_steps + 7 samples); 0 = no cap
    uint32_t edge_tab;                                     // 1: H + 1 floats of LDS behind the stages hold the voxel faces (rm_skip_target_tab)
    const uint32_t *run_if;                                // NULL, or a device word: the launch does nothing unless it is non-zero (the barrier-free answer to a phased
                                                           // launch whose grid barrier timed out: queued behind it unconditionally, a few microseconds when not needed)
};

__global__ __launch_bounds__(FBLOCK) void occupancy_render_kernel(const RenderArgs a, const OccArgs oc)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (oc.run_if && __hip_atomic_load(oc.run_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;      // (uniform over the grid: written before this launch started)
    fill_lds(lds, a);
    const float *etab = nullptr;
    if (oc.edge_tab) { rm_edge_table(lds + OCC_LDS_FLOATS, oc.H, a.bound); etab = lds + OCC_LDS_FLOATS; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    float *stage = lds + FWD_LDS_FLOATS + wave * OC_STAGE;
    uint32_t *slotmap = reinterpret_cast<uint32_t *>(stage + 8 * 64), *lanemap = slotmap + 64;
    const FieldCtx fc = make_ctx(a);
    const float inv_s = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
    const float bound = a.bound;
    const uint32_t gsz = 1u << oc.glog;
    const uint32_t ngroups = (oc.N + gsz - 1) >> oc.glog;
    uint32_t evaluated = 0;
    // groups are dealt to the workgroups first, to the waves of a workgroup second: a small batch spreads over the compute units instead of filling few of them
    for (uint32_t grp = (uint32_t)wave * gridDim.x + blockIdx.x; grp < ngroups; grp += gridDim.x * FW) {
        const uint32_t ray = (grp << oc.glog) + (uint32_t)lane;
        const bool mine = (uint32_t)lane < gsz && ray < oc.N;
        bool alive = mine;
        const uint32_t rr = mine ? ray : oc.N - 1;
        RayCtx c; rm_setup(c, oc.rays_o + 3 * (size_t)rr, oc.rays_d + 3 * (size_t)rr, oc.grid, oc.mean_density, bound, oc.H);
        float near, far;
        cube_near_far(c.ox, c.oy, c.oz, c.dx, c.dy, c.dz, bound, near, far);      // near_far_from_bound(type='cube'), instant_nsr.py:58-77 (what run_cuda passes to march_rays)
        float t = near, last_t = near;                                             // marcher's t | its last_t (the compositor's t, rays_t: acc.t)
        float skip_tt = RM_NO_SKIP;                                                 // the walk's pending skip target (rm_march_batch)
        RayAcc acc{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, near };
        uint32_t taken = 0;                                                         // samples this ray has marched so far
        while (__ballot(alive) != 0ull) {
            // ---- march: this lane's next (up to K) occupied samples into its own slots (march_rays_kernel's loop body).  K = 64 / (rays of the group still
            // alive): a group starts with few samples per ray and iteration and ends with whole tiles for its last, longest rays ----
            const unsigned long long am = __ballot(alive);
            const uint32_t na = (uint32_t)__builtin_popcountll(am), K = 64u / na;
            const uint32_t arank = (uint32_t)__builtin_popcountll(am & ((1ull << lane) - 1ull)), mybase = arank * K;
            if (alive) lanemap[arank] = (uint32_t)lane;
            uint32_t mycnt = 0;
            if (alive) {
                float *sp = stage + 8 * mybase;
                bool ended;
                mycnt = occ_march(c, t, last_t, skip_tt, far, K, oc.max_steps, taken, etab, ended, [&](float x, float y, float z, float dt, float dl1) {
                    sp[0] = x; sp[1] = y; sp[2] = z; sp[3] = dt; sp[7] = dl1;
                    sp += 8;
                });
                if (ended) alive = false;
            }
            wave_sync();
            // slot s = lane: it belongs to the (s / K)-th alive ray and is valid if that ray produced more than s % K samples this iteration
            const uint32_t orank = (uint32_t)lane / K, owner = orank < na ? lanemap[orank] : 0u;
            const uint32_t owner_cnt = (uint32_t)__shfl((int)mycnt, (int)owner);
            const bool valid = orank < na && ((uint32_t)lane - orank * K) < owner_cnt;
            const unsigned long long vm = __ballot(valid);
            if (vm == 0ull) break;
            const uint32_t cnt = (uint32_t)__builtin_popcountll(vm);
            if (valid) slotmap[__builtin_popcountll(vm & ((1ull << lane) - 1ull))] = (uint32_t)lane;
            wave_sync();
            evaluated += cnt;
            // ---- field on the packed samples, tiles of 16 (field_samples_kernel's body) ----
            for (uint32_t q0 = 0; q0 < cnt; q0 += 16) {
                const uint32_t ci = q0 + (uint32_t)n;
                const uint32_t slot = slotmap[ci < cnt ? ci : cnt - 1];
                const float *sp = stage + 8 * slot;
                const int src = (int)lanemap[slot / K];
                float alpha, rgb[3], nrm[3], sdf0, gr[3], gn;
                field_tile(lds, fsl, fc, a, lane, sp[0], sp[1], sp[2], __shfl(c.dx, src), __shfl(c.dy, src), __shfl(c.dz, src), sp[3], inv_s,
                           alpha, rgb, nrm, sdf0, gr, gn);
                wave_sync();                                                         // every lane has read its inputs: the slots become outputs
                if (g == 0 && ci < cnt) {
                    float *so = stage + 8 * slot;
                    so[0] = alpha; so[1] = rgb[0]; so[2] = rgb[1]; so[3] = rgb[2]; so[4] = nrm[0]; so[5] = nrm[1]; so[6] = nrm[2];
                }
                wave_sync();
            }
            // ---- composite: every lane its own samples, in order (composite_rays_kernel's loop body) ----
            for (uint32_t k = 0; k < mycnt; ++k) {
                const float *so = stage + 8 * (mybase + k);
                if (rm_composite_step(acc, so[0], so[7], so[1], so[2], so[3], so[4], so[5], so[6])) { alive = false; break; }
            }
            wave_sync();
        }
        if (mine) {
            oc.weights_sum[ray] = acc.ws; oc.depth[ray] = acc.dep;
            oc.image[3 * (size_t)ray] = acc.r; oc.image[3 * (size_t)ray + 1] = acc.g; oc.image[3 * (size_t)ray + 2] = acc.b;
            oc.normal_map[3 * (size_t)ray] = acc.nx; oc.normal_map[3 * (size_t)ray + 1] = acc.ny; oc.normal_map[3 * (size_t)ray + 2] = acc.nz;
        }
    }
    if (oc.n_samples && lane == 0 && evaluated) atomicAdd(oc.n_samples, evaluated);
}

// ---- the occupancy-grid TRAINING render without autograd as one launch (round 5) -------------------------------------------------------------------
// What NeRFRenderer.run_cuda's train() branch computes under torch.no_grad() -- stylize.py's render_val of a cuda_ray network, which never leaves train mode --
// as march_rays_train (count, scan, write) / ac_field_samples / two composite_rays_train / a dozen torch kernels for the eikonal term and the background.
// One persistent workgroup per compute unit at most (so that every workgroup is resident), four phases separated by grid barriers:
//   A  lane = ray: the walk (march_count_kernel's), counting the occupied steps and recording their positions in the ray's recurrence (RayRecorder); per
//      256 rays a total (integer atomics: order-free);
//   B  lane = ray: the ray's offset in the packed layout = counter[0] + totals of the chunks before + counts before it in its chunk, the reference's budget
//      rule (a ray whose samples would end at or beyond M is left out: raymarching.cu:133), and the samples written by REPLAYING the recurrence at the
//      recorded positions (no second walk);
//   C  tile = 16 consecutive packed samples, dealt to ALL waves (a tile through the field code is ~45 us of latency: a wave that kept its own rays' tiles to
//      itself -- the first form of this kernel, r05_experiments.txt section 8c -- ran three or four in a row while most of the device idled): the body of
//      field_samples_kernel, plus the eikonal term's partial sums;
//   D  lane = ray: composite_train_fwd_kernel's loop for image and normal map on the same weights, background.
// weights_sum / image / normal_map: the bits of the chain of operators (tests/test_gpu_run_cuda.py).  gradient_error: the same terms summed in double
// in a fixed order (per lane, per wave, per workgroup; the last workgroup to leave adds the partials) instead of torch's fp32 tree: equal to ~1e-6 relative.
constexpr uint32_t OT_CHUNK_LOG = 8;                     // 2^8 rays per chunk total (a multiple of the wave's 64)
// bound of a grid barrier's spin, in ticks of the 100 MHz wall clock: two seconds unless AC_OCC_BARRIER_MS or ac_set_occupancy_barrier_ms says otherwise
static std::atomic<uint32_t> g_barrier_ms{0};            // 0 = the default
static uint32_t ot_default_ms()
{
    static const uint32_t d = []() { const char *e = getenv("AC_OCC_BARRIER_MS"); const long ms = e ? atol(e) : 0; return (uint32_t)(ms > 0 ? ms : 2000); }();
    return d;
}
static unsigned long long ot_spin_ticks()
{
    const uint32_t ms = g_barrier_ms.load(std::memory_order_relaxed);
    return (unsigned long long)(ms ? ms : ot_default_ms()) * 100000ull;
}
struct OccTrainArgs {
    const float *rays_o, *rays_d, *grid;
    uint32_t N, H, M_write, M_comp, perturb;             // M_write: capacity of the packed layout (march_write's budget, > 0); M_comp: the compositor's
    float mean_density;
    int32_t *counter;                                    // optional [2]: += samples of all rays, += N (march_rays_train's step counter)
    float *weights_sum, *image, *normal_map, *gradient_error;
    const float *bg; uint32_t bg_mode; float bg_value;   // image += (1 - weights_sum) * bg:  0 none, 1 bg_value, 2 bg[3], 3 bg[N][3]
    uint32_t *sync;                                      // [16]; 0 - 3 zero on entry and on exit: arrivals, departures, barrier failure, samples written; 8: failed launches (sticky)
    int32_t *chunk_tot, *counts, *offs, *ovf;            // [chunks] zero on entry and on exit | [N] | [N] offset of a written ray, else -1 | [N]
    uint32_t *wmask, *rec;                               // [N] | [N][RM_REC_WORDS]: the samples' positions (RayRecorder)
    double *partials;                                    // [gridDim.x][2]
    int32_t *p_ray; float *p_in, *p_out;                 // packed samples: ray [M] | x y z dt [M][4] | alpha r g b nx ny nz - [M][8]
    unsigned long long spin_ticks;                       // bound of a grid barrier's spin (ot_spin_ticks)
};

__device__ __forceinline__ int32_t ot_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// every workgroup has arrived `phase` + 1 times (false: timed out after `ticks` of the 100 MHz wall clock -- a foreign kernel held compute units for that long:
// the launch itself cannot be too large, ac::launch_resident sized it -- the caller gives up instead of hanging; the host re-renders, see the launch sites)
__device__ __forceinline__ bool ot_barrier(uint32_t *sync, uint32_t phase, uint32_t *flag, unsigned long long ticks)
{
    // every wave first waits until ITS OWN stores have been written to its XCD's L2 (s_waitcnt vmcnt(0): ADVICE round 5 -- outside tgsplit mode the
    // workgroup-scope release inside __syncthreads() need not wait for them), then ONE thread writes that L2's dirty lines back to where the other XCDs see them
    // (agent-scope release) -- once per workgroup.  Measured: that fence by lane 0 of every wave instead costs the 65 536-ray inference launch 1.08 -> 1.39 ms
    // and the training form 0.335 -> 0.449 (eight L2 write-backs + invalidations per workgroup and barrier); by every thread 0.537 (round 5).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __threadfence();
    if (threadIdx.x == 0) {
        atomicAdd(&sync[0], 1u);
        const uint32_t want = (phase + 1u) * gridDim.x;
        const unsigned long long t0 = wall_clock64();
        bool all = false;
        while (!(all = __hip_atomic_load(&sync[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) && wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(10);
        *flag = all ? 1u : 0u;
        if (!*flag) atomicExch(&sync[2], 1u);
        __threadfence();                                 // acquire: the compute unit's L1 (shared by the workgroup's waves) and the L2's copies of other XCDs' lines are dropped
    }
    __syncthreads();
    return *flag != 0u;
}

__global__ __launch_bounds__(FBLOCK) void occupancy_train_kernel(const RenderArgs a, const OccTrainArgs oc)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ uint32_t bar_flag, last;
    __shared__ double red[2 * FW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const float bound = a.bound;
    const int32_t base = oc.counter ? oc.counter[0] : 0;                  // (read before the first barrier: the last workgroup to leave updates it)
    const uint32_t nchunks = (oc.N + (1u << OT_CHUNK_LOG) - 1) >> OT_CHUNK_LOG;
    const uint32_t wid = (uint32_t)wave * gridDim.x + blockIdx.x, nwaves = gridDim.x * FW;   // work is dealt to the workgroups first, to a workgroup's waves second:
                                                                                             // a 4096-ray batch is one walking wave on each of 64 compute units, not eight on eight
    bool ok = true;
    // ---- A: counts and records ----
    const float *etab = nullptr;                                            // the voxel faces (rm_skip_target_tab) where the weights will be: H + 1 floats
    if (oc.H < (uint32_t)RM_EDGE_MAX) { rm_edge_table(lds, oc.H, bound); etab = lds; }
    __syncthreads();
    for (uint32_t r0 = wid * 64u; r0 < oc.N; r0 += nwaves * 64u) {         // (a wave's 64 consecutive rays lie in one chunk)
        const uint32_t ray = r0 + (uint32_t)lane;
        int32_t cnt = 0;
        if (ray < oc.N) {
            RayCtx c; rm_setup(c, oc.rays_o + 3 * (size_t)ray, oc.rays_d + 3 * (size_t)ray, oc.grid, oc.mean_density, bound, oc.H);
            float near, far; rm_near_far(c, near, far);
            float t = ray_t0(c, near, ray, oc.perturb), skip_tt = RM_NO_SKIP;
            uint32_t room = RM_MAX_STEPS, kpos = 0;
            RayRecorder rr; rr.begin(oc.rec + (size_t)ray * RM_REC_WORDS);
            while (room > 0 && rm_march_batch<RM_BATCH, true>(c, t, skip_tt, far, room, kpos, [&](float, float, float, float, float, uint32_t k) { rr.add(k); }, etab)) {}
            rr.end();
            cnt = (int32_t)(RM_MAX_STEPS - room);
            oc.counts[ray] = cnt; oc.ovf[ray] = rr.ovf ? 1 : 0; oc.wmask[ray] = rr.wmask;
        }
        int32_t tot = cnt;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d);
        if (lane == 0 && tot) atomicAdd(&oc.chunk_tot[r0 >> OT_CHUNK_LOG], tot);
    }
    __syncthreads();                                                        // (the face table is done with: the weights take its place)
    fill_lds(lds, a);
    ok = ot_barrier(oc.sync, 0, &bar_flag, oc.spin_ticks);
    // ---- B: offsets, the budget rule, the packed samples ----
    for (uint32_t r0 = wid * 64u; r0 < oc.N && ok; r0 += nwaves * 64u) {
        const uint32_t ray = r0 + (uint32_t)lane;
        const bool mine = ray < oc.N;
        int32_t pre = 0;
        {
            const uint32_t c0 = r0 >> OT_CHUNK_LOG, s0 = c0 << OT_CHUNK_LOG;
            for (uint32_t cix = (uint32_t)lane; cix < c0; cix += 64) pre += oc.chunk_tot[cix];
            for (uint32_t i = s0 + (uint32_t)lane; i < r0; i += 64) pre += oc.counts[i];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) pre += __shfl_xor(pre, d);
        }
        const int32_t cnt = mine ? oc.counts[ray] : 0;
        int32_t inc = cnt;                                                  // inclusive scan over the wave's rays
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int32_t v = __shfl_up(inc, d); if (lane >= d) inc += v; }
        const uint32_t offset = (uint32_t)(base + pre + (inc - cnt)), end = offset + (uint32_t)cnt;
        const bool written = mine && cnt > 0 && end < oc.M_write;           // march_write_kernel: `point_index + num_steps >= M -> return`
        if (mine) oc.offs[ray] = written ? (int32_t)offset : -1;
        uint32_t wend = written ? end : 0u;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const uint32_t v = (uint32_t)__shfl_xor((int)wend, d); wend = v > wend ? v : wend; }
        if (lane == 0 && wend) atomicMax(&oc.sync[3], wend);
        if (written) {
            RayCtx c; rm_setup(c, oc.rays_o + 3 * (size_t)ray, oc.rays_d + 3 * (size_t)ray, oc.grid, oc.mean_density, bound, oc.H);
            float near, far; rm_near_far(c, near, far);
            const float t0 = ray_t0(c, near, ray, oc.perturb);
            float *pi = oc.p_in + 4 * (size_t)offset; int32_t *pr = oc.p_ray + offset;
            auto put = [&](float x, float y, float z, float dt) { pi[0] = x; pi[1] = y; pi[2] = z; pi[3] = dt; pi += 4; *pr++ = (int32_t)ray; };
            if (!oc.ovf[ray]) rm_replay(c, t0, oc.rec + (size_t)ray * RM_REC_WORDS, oc.wmask[ray], (uint32_t)cnt, put);
            else {
                float t = t0, skip_tt = RM_NO_SKIP; uint32_t room = (uint32_t)cnt, kpos = 0;
                while (room > 0 && rm_march_batch<RM_BATCH>(c, t, skip_tt, far, room, kpos, [&](float x, float y, float z, float dt, float, uint32_t) { put(x, y, z, dt); })) {}
            }
        }
    }
    ok = ok && ot_barrier(oc.sync, 1, &bar_flag, oc.spin_ticks);
    // ---- C: the field on the packed samples, tiles dealt to all waves ----
    double e_num = 0.0, e_den = 0.0;                                       // this lane's share of sum(relax * gerr), sum(relax)
    {
        float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
        const FieldCtx fc = make_ctx(a);
        const float inv_s = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
        const uint32_t W = ok ? __hip_atomic_load(&oc.sync[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const uint32_t ntiles = (W + 15u) / 16u;
        for (uint32_t tile = wid; tile < ntiles; tile += nwaves) {
            const uint32_t b = tile * 16 + (uint32_t)n, bb = b < W ? b : W - 1;
            const float4 in = *reinterpret_cast<const float4 *>(oc.p_in + 4 * (size_t)bb);
            const int32_t ray = oc.p_ray[bb];
            const float sx = in.x, sy = in.y, sz = in.z;
            const float *d = oc.rays_d + 3 * (size_t)ray;
            float alpha, rgb[3], nrm[3], sdf0, gr[3], gn;
            field_tile(lds, fsl, fc, a, lane, sx, sy, sz, d[0], d[1], d[2], in.w, inv_s, alpha, rgb, nrm, sdf0, gr, gn);
            if (g == 0 && b < W) {
                // eikonal term over the packed samples (instant_nsr.py:266-272): relax = |x| < 1.2 on the marcher's point, (|gradient| - 1)^2
                if (__builtin_sqrtf((sx * sx + sy * sy) + sz * sz) < 1.2f) { const float d1 = gn - 1.0f; e_num += (double)(d1 * d1); e_den += 1.0; }
                float *po = oc.p_out + 8 * (size_t)b;
                *reinterpret_cast<float4 *>(po) = make_float4(alpha, rgb[0], rgb[1], rgb[2]);
                *reinterpret_cast<float4 *>(po + 4) = make_float4(nrm[0], nrm[1], nrm[2], 0.0f);
            }
            wave_sync();
        }
    }
    ok = ok && ot_barrier(oc.sync, 2, &bar_flag, oc.spin_ticks);
    // ---- D: the packed compositor per ray (composite_train_fwd_kernel's loop), image and normal map on the same weights; background ----
    for (uint32_t r0 = wid * 64u; r0 < oc.N && ok; r0 += nwaves * 64u) {
        const uint32_t ray = r0 + (uint32_t)lane;
        if (ray >= oc.N) continue;
        const int32_t off = oc.offs[ray], cnt = oc.counts[ray];
        const bool composited = off >= 0 && (uint32_t)off + (uint32_t)cnt < oc.M_comp;      // `offset + num_steps >= M -> zeros`
        float T = 1.0f, cn[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };        // colour | normal
        if (composited) {
            const float *po = oc.p_out + 8 * (size_t)off;
            T = rm_composite_train((uint32_t)cnt, cn, [&](uint32_t k, float (&v)[6]) {
                const float4 u = *reinterpret_cast<const float4 *>(po + 8 * (size_t)k), w = *reinterpret_cast<const float4 *>(po + 8 * (size_t)k + 4);
                v[0] = u.y; v[1] = u.z; v[2] = u.w; v[3] = w.x; v[4] = w.y; v[5] = w.z;
                return u.x;
            });
        }
        const float ws = composited ? 1.0f - T : 0.0f;
        float cr = cn[0], cg = cn[1], cb = cn[2];
        if (oc.bg_mode) {                                                   // image + (1 - weights_sum) * bg, torch's three operations in torch's order
            const float om = 1.0f - ws;
            const size_t bo = oc.bg_mode == 3 ? 3 * (size_t)ray : 0;
            const float b0 = oc.bg_mode == 1 ? oc.bg_value : oc.bg[bo], b1 = oc.bg_mode == 1 ? oc.bg_value : oc.bg[bo + 1], b2 = oc.bg_mode == 1 ? oc.bg_value : oc.bg[bo + 2];
            cr = cr + om * b0; cg = cg + om * b1; cb = cb + om * b2;
        }
        oc.weights_sum[ray] = ws;
        oc.image[3 * (size_t)ray] = cr; oc.image[3 * (size_t)ray + 1] = cg; oc.image[3 * (size_t)ray + 2] = cb;
        oc.normal_map[3 * (size_t)ray] = cn[3]; oc.normal_map[3 * (size_t)ray + 1] = cn[4]; oc.normal_map[3 * (size_t)ray + 2] = cn[5];
    }
    // ---- eikonal partials: lane -> wave -> workgroup (fixed order); the last workgroup to leave adds the workgroups' and re-arms the scratch ----
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { e_num += __shfl_xor(e_num, d); e_den += __shfl_xor(e_den, d); }
    if (lane == 0) { red[2 * wave] = e_num; red[2 * wave + 1] = e_den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sn = 0.0, sd = 0.0;
        for (int w = 0; w < FW; ++w) { sn += red[2 * w]; sd += red[2 * w + 1]; }
        oc.partials[2 * blockIdx.x] = sn; oc.partials[2 * blockIdx.x + 1] = sd;
        __threadfence();
        last = atomicAdd(&oc.sync[1], 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (wave == 0) {
        double sn = 0.0, sd = 0.0;
        for (uint32_t b = (uint32_t)lane; b < gridDim.x; b += 64) {
            sn += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(oc.partials) + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            sd += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(oc.partials) + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { sn += __shfl_xor(sn, d); sd += __shfl_xor(sd, d); }
        int32_t tot = 0;
        for (uint32_t cix = (uint32_t)lane; cix < nchunks; cix += 64) { tot += ot_load(oc.chunk_tot + cix); oc.chunk_tot[cix] = 0; }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d);
        if (lane == 0) {
            const bool failed = __hip_atomic_load(&oc.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            oc.gradient_error[0] = failed ? __builtin_nanf("") : (float)sn / ((float)sd + 1e-5f);
            if (oc.counter) { oc.counter[0] = base + tot; oc.counter[1] += (int32_t)oc.N; }
            if (failed) oc.sync[8] += 1u;                                   // (sticky: launches of this scratch whose barrier timed out -- never reset)
            oc.sync[0] = 0u; oc.sync[1] = 0u; oc.sync[2] = 0u; oc.sync[3] = 0u;
        }
    }
}

// ---- the occupancy-grid INFERENCE render in phases (round 5): rounds of march | field | composite inside ONE launch, grid barriers between them --------------
// occupancy_render_kernel above gives every wave 8 - 16 rays and lets it march (a quarter of its lanes), evaluate (its own tiles, one after the other: ~45 us of
// latency each) and composite them.  What the training kernel taught -- walk with every lane, deal the tiles to ALL waves -- applies here too, except that a ray's
// march depends on its composite (it stops at T < 1e-2): so the reference's loop of rounds comes back, inside the launch, without its host read-backs:
//   M  lane = alive ray (64 per wave, waves dealt over the device): up to n_step samples into the ray's slots, the slot ids appended to the round's tile list
//      (one integer atomic per wave: the order of the list does not reach any result);
//   F  the field on tiles of 16 listed samples, dealt to all waves (field_samples_kernel's body);
//   C  lane = alive ray: composite_rays_kernel's loop over the ray's samples of this round; rays that go on are appended to the next round's list.
// A ray's samples, their order and every operation on them are those of occupancy_render_kernel (and of the three stand-alone operators run as one round):
// the same bits for any n_step (tests/test_gpu_run_cuda.py); n_step only decides how many samples past a ray's last one are evaluated in vain.
struct OccPhArgs {
    const float *rays_o, *rays_d, *grid;
    uint32_t N, H, max_steps, nlog;                        // n_step = 1 << nlog samples per ray and round
    float mean_density;
    float *weights_sum, *depth, *image, *normal_map;       // accumulators, as composite_rays leaves them
    uint32_t *n_samples;                                   // optional [1]
    uint32_t *sync;                                        // [16]; 0 - 7 zero on entry and on exit: 0 arrivals, 1 departures, 2 failure, 4 - 5 rays alive, 6 - 7 samples listed; 8: failed launches (sticky)
    int32_t *alive;                                        // [2][N]
    float *st;                                             // [N][4] per ray: marcher's t, its last_t, the compositor's t, samples taken (bits)
    uint32_t *cnt;                                         // [N] per alive entry: samples of this round | bit 31: the walk ended
    uint32_t *list;                                        // [N << nlog] slot ids
    float *s_in, *s_out;                                   // [N << nlog][8]: x y z dt dl1 - - - | alpha r g b nx ny nz -
    unsigned long long spin_ticks;                         // bound of a grid barrier's spin (ot_spin_ticks)
};

__global__ __launch_bounds__(FBLOCK) void occupancy_phased_kernel(const RenderArgs a, const OccPhArgs oc)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ uint32_t bar_flag, last;
    fill_lds(lds, a);
    const float *etab = nullptr;
    if ((FWD_LDS_FLOATS + (size_t)oc.H + 1) * sizeof(float) + 64 <= 160 * 1024) { rm_edge_table(lds + FWD_LDS_FLOATS, oc.H, a.bound); etab = lds + FWD_LDS_FLOATS; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float inv_s = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
    const float bound = a.bound;
    const uint32_t wid = (uint32_t)wave * gridDim.x + blockIdx.x, nwaves = gridDim.x * FW;
    uint32_t n_al = oc.N, round = 0, phase = 0, evaluated = 0;
    bool ok = true;
    for (;;) {
        const uint32_t cur = round & 1u, nxt = cur ^ 1u;
        // samples per ray in this round: 2^oc.nlog while most rays are alive, up to 64 once the slots allow it (like the reference's n_step = N / n_alive: the
        // stragglers -- rays along a limb -- finish in a round or two instead of one round per 16 samples, and a round costs three barriers whatever its size)
        uint32_t nlog = oc.nlog;
        while (nlog < 6u && ((uint64_t)n_al << (nlog + 1u)) <= ((uint64_t)oc.N << oc.nlog)) ++nlog;
        const uint32_t nstep = 1u << nlog;
        const int32_t *L = oc.alive + (size_t)cur * oc.N;
        // ---- M: march ----
        if (blockIdx.x == 0 && threadIdx.x == 0) oc.sync[4 + nxt] = 0u;                 // (the next round's ray counter: idle until this round's phase C)
        for (uint32_t a0 = wid * 64u; a0 < n_al; a0 += nwaves * 64u) {
            const uint32_t e = a0 + (uint32_t)lane;
            const bool mine = e < n_al;
            const uint32_t ray = mine ? (round ? (uint32_t)L[e] : e) : 0u;
            RayCtx c; rm_setup(c, oc.rays_o + 3 * (size_t)ray, oc.rays_d + 3 * (size_t)ray, oc.grid, oc.mean_density, bound, oc.H);
            float near, far;
            cube_near_far(c.ox, c.oy, c.oz, c.dx, c.dy, c.dz, bound, near, far);
            float t = near, last_t = near, skip_tt = RM_NO_SKIP;
            uint32_t taken = 0;
            float4 *stp = reinterpret_cast<float4 *>(oc.st) + ray;
            if (mine) {
                if (round) { const float4 v = *stp; t = v.x; last_t = v.y; taken = __float_as_uint(v.w); }
                else {
                    oc.weights_sum[ray] = 0.0f; oc.depth[ray] = 0.0f;
                    for (int k = 0; k < 3; ++k) { oc.image[3 * (size_t)ray + k] = 0.0f; oc.normal_map[3 * (size_t)ray + k] = 0.0f; }
                }
            }
            uint32_t mycnt = 0;
            if (mine) {
                float *sp = oc.s_in + 8 * ((size_t)e << nlog);
                bool ended;
                mycnt = occ_march(c, t, last_t, skip_tt, far, nstep, oc.max_steps, taken, etab, ended, [&](float x, float y, float z, float dt, float dl1) {
                    *reinterpret_cast<float4 *>(sp) = make_float4(x, y, z, dt); sp[4] = dl1;
                    sp += 8;
                });
                const float tc0 = round ? (*stp).z : near;
                *stp = make_float4(t, last_t, tc0, __uint_as_float(taken));
                oc.cnt[e] = mycnt | (ended ? 0x80000000u : 0u);
            }
            // the round's tile list: a wave reserves room for its samples with one atomic
            uint32_t inc = mycnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += v; }
            const uint32_t tot = (uint32_t)__shfl((int)inc, 63);
            uint32_t base = 0;
            if (lane == 0 && tot) base = atomicAdd(&oc.sync[6 + cur], tot);
            base = (uint32_t)__shfl((int)base, 0) + (inc - mycnt);
            for (uint32_t k = 0; k < mycnt; ++k) oc.list[base + k] = (e << nlog) + k;
        }
        ok = ok && ot_barrier(oc.sync, phase++, &bar_flag, oc.spin_ticks);
        // ---- F: field on the listed samples ----
        if (blockIdx.x == 0 && threadIdx.x == 0) oc.sync[6 + nxt] = 0u;                 // (the next round's list counter)
        const uint32_t nl = ok ? __hip_atomic_load(&oc.sync[6 + cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        for (uint32_t tile = wid; tile * 16u < nl; tile += nwaves) {
            const uint32_t q = tile * 16u + (uint32_t)n, slot = oc.list[q < nl ? q : nl - 1];
            const uint32_t e = slot >> nlog, ray = round ? (uint32_t)L[e] : e;
            const float4 in = *reinterpret_cast<const float4 *>(oc.s_in + 8 * (size_t)slot);
            const float *d = oc.rays_d + 3 * (size_t)ray;
            float alpha, rgb[3], nrm[3], sdf0, gr[3], gn;
            field_tile(lds, fsl, fc, a, lane, in.x, in.y, in.z, d[0], d[1], d[2], in.w, inv_s, alpha, rgb, nrm, sdf0, gr, gn);
            if (g == 0 && q < nl) {
                float *po = oc.s_out + 8 * (size_t)slot;
                *reinterpret_cast<float4 *>(po) = make_float4(alpha, rgb[0], rgb[1], rgb[2]);
                *reinterpret_cast<float4 *>(po + 4) = make_float4(nrm[0], nrm[1], nrm[2], 0.0f);
            }
            wave_sync();
        }
        if (wid == 0 && lane == 0) evaluated += nl;
        ok = ok && ot_barrier(oc.sync, phase++, &bar_flag, oc.spin_ticks);
        // ---- C: composite, and who goes on ----
        for (uint32_t a0 = wid * 64u; a0 < n_al && ok; a0 += nwaves * 64u) {
            const uint32_t e = a0 + (uint32_t)lane;
            const bool mine = e < n_al;
            bool goes = false;
            uint32_t ray = 0;
            if (mine) {
                ray = round ? (uint32_t)L[e] : e;
                const uint32_t cw = oc.cnt[e], mycnt = cw & 0x7fffffffu;
                bool alive = !(cw >> 31);
                float4 *stp = reinterpret_cast<float4 *>(oc.st) + ray;
                RayAcc acc{ oc.weights_sum[ray], oc.depth[ray], oc.image[3 * (size_t)ray], oc.image[3 * (size_t)ray + 1], oc.image[3 * (size_t)ray + 2],
                            oc.normal_map[3 * (size_t)ray], oc.normal_map[3 * (size_t)ray + 1], oc.normal_map[3 * (size_t)ray + 2], (*stp).z };
                const float *pi = oc.s_in + 8 * ((size_t)e << nlog), *po = oc.s_out + 8 * ((size_t)e << nlog);
                for (uint32_t k = 0; k < mycnt; ++k, pi += 8, po += 8) {            // composite_rays_kernel's loop body
                    const float4 u = *reinterpret_cast<const float4 *>(po), v = *reinterpret_cast<const float4 *>(po + 4);
                    if (rm_composite_step(acc, u.x, pi[4], u.y, u.z, u.w, v.x, v.y, v.z)) { alive = false; break; }
                }
                (*stp).z = acc.t;
                oc.weights_sum[ray] = acc.ws; oc.depth[ray] = acc.dep;
                oc.image[3 * (size_t)ray] = acc.r; oc.image[3 * (size_t)ray + 1] = acc.g; oc.image[3 * (size_t)ray + 2] = acc.b;
                oc.normal_map[3 * (size_t)ray] = acc.nx; oc.normal_map[3 * (size_t)ray + 1] = acc.ny; oc.normal_map[3 * (size_t)ray + 2] = acc.nz;
                goes = alive;
            }
            const unsigned long long gm = __ballot(goes);
            if (gm) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&oc.sync[4 + nxt], (uint32_t)__builtin_popcountll(gm));
                base = (uint32_t)__shfl((int)base, 0);
                if (goes) oc.alive[(size_t)nxt * oc.N + base + (uint32_t)__builtin_popcountll(gm & ((1ull << lane) - 1ull))] = (int32_t)ray;
            }
        }
        ok = ok && ot_barrier(oc.sync, phase++, &bar_flag, oc.spin_ticks);
        n_al = ok ? __hip_atomic_load(&oc.sync[4 + nxt], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        if (n_al == 0u) break;
        ++round;
    }
    if (oc.n_samples && wid == 0 && lane == 0 && evaluated) atomicAdd(oc.n_samples, evaluated);
    // the last workgroup to leave re-arms the scratch
    __syncthreads();
    if (threadIdx.x == 0) { __threadfence(); last = atomicAdd(&oc.sync[1], 1u) == gridDim.x - 1u ? 1u : 0u; }
    __syncthreads();
    if (last && threadIdx.x < 8) {
        // a barrier timed out: a NaN pixel, the sticky count (word 8) and THIS launch's verdict (word 9, rewritten by every launch): the barrier-free launch the
        // host has queued behind this one (ac_render_rays_occupancy_phased) runs if and only if it is set, and overwrites every output
        if (threadIdx.x == 2) {
            const bool failed = oc.sync[2] != 0u;
            if (failed) { oc.weights_sum[0] = __builtin_nanf(""); oc.sync[8] += 1u; if (oc.n_samples) *oc.n_samples = 0u; }
            __hip_atomic_store(&oc.sync[9], failed ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
        oc.sync[threadIdx.x] = 0u;
    }
}

}  // namespace

// the RenderArgs of a launch that shades: the field's (prep_args) and the NeuS alpha's constants
static int shade_args(RenderArgs &a, const ac_field *field, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio)
{
    if (int rc = prep_args(a, field, bound, eps)) return rc;
    a.inv_s = inv_s; a.inv_s_dev = inv_s_dev; a.car = cos_anneal_ratio; a.one_m_car = (float)(1.0 - (double)cos_anneal_ratio);
    return AC_OK;
}

// what every render entry asks of its arguments; buffers: all of the entry's required pointers are non-NULL
static int check_render(const char *who, bool buffers, uint32_t H, float eps)
{
    if (buffers && H >= 2 && eps > 0.0f) return AC_OK;
    ac::set_error("%s: NULL buffer, H < 2 or eps <= 0", who);
    return AC_ERR_BAD_ARG;
}

AC_API int ac_field_samples(const ac_field *field, const float *xyzs, const float *dirs, const float *deltas, uint32_t delta_stride, uint32_t M,
                            float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio, float *alpha, float *rgb, float *normal,
                            float *sdf, float *gradient, ac_stream_t stream)
{
    if (M == 0) return AC_OK;
    if (!xyzs || !dirs || !deltas || !alpha || !rgb || !normal || delta_stride == 0 || !(eps > 0.0f)) {
        ac::set_error("field_samples: NULL buffer, delta_stride == 0 or eps <= 0"); return AC_ERR_BAD_ARG;
    }
    RenderArgs a{};
    if (int rc = shade_args(a, field, bound, eps, inv_s, inv_s_dev, cos_anneal_ratio)) return rc;
    SampleArgs sa{ xyzs, dirs, deltas, delta_stride, M, alpha, rgb, normal, sdf, gradient };
    const size_t lds_bytes = FWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(field_samples_kernel), lds_bytes);
    uint32_t blocks = ((M + 15) / 16 + FW - 1) / FW;              // persistent, one workgroup per CU (140 KB of LDS), like the SDF query
    const uint32_t cus = ac::cu_count();
    if (blocks > cus) blocks = cus;
    hipLaunchKernelGGL(field_samples_kernel, dim3(blocks), dim3(FBLOCK), lds_bytes, (hipStream_t)stream, a, sa);
    return ac::check_launch("field_samples");
}

static int render_rays_occupancy_impl(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                                      float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                                      float *weights_sum, float *depth, float *image, float *normal_map, uint32_t *n_samples, uint32_t max_steps,
                                      ac_stream_t stream, const uint32_t *run_if)
{
    if (N == 0) return AC_OK;
    if (int rc = check_render("render_rays_occupancy", rays_o && rays_d && grid && weights_sum && depth && image && normal_map, H, eps)) return rc;
    RenderArgs a{};
    if (int rc = shade_args(a, field, bound, eps, inv_s, inv_s_dev, cos_anneal_ratio)) return rc;
    const uint32_t cus = ac::cu_count();
    // rays per wave (2^glog): 16 for whole views, 8 for small batches (more waves in flight: the march is a chain of ~200 dependent grid look-ups per ray,
    // 0.26 ms end to end, and only concurrency hides it).  Measured on the 256 x 256 bench view (profiles/r04_experiments.txt section 11): 65 536 rays in one
    // launch 2.67 / 2.37 / 2.92 / 3.26 ms for 8 / 16 / 32 / 64 rays per wave; in 4096-ray launches 12.1 / 15.6 / 20.0 / 23.4 ms.
    const uint32_t glog = N >= 32768u ? 4u : 3u;
    const uint32_t gsz = 1u << glog;
    // the voxel faces as a table behind the stages when H + 1 floats still fit the compute unit's LDS (H = 128: 516 of the 1.9 KB left)
    const bool tab = (OCC_LDS_FLOATS + (size_t)H + 1) * sizeof(float) + 64 <= 160 * 1024;
    OccArgs oc{ rays_o, rays_d, grid, N, H, mean_density, weights_sum, depth, image, normal_map, n_samples, glog, max_steps, tab ? 1u : 0u, run_if };
    const size_t lds_bytes = (OCC_LDS_FLOATS + (tab ? (size_t)H + 1 : 0)) * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(occupancy_render_kernel), 160 * 1024 - 64);      // (a ceiling, set once: lds_bytes depends on H)
    uint32_t blocks = (N + gsz - 1) / gsz;                         // one group per workgroup first (see the kernel's loop), one persistent workgroup per CU at most
    if (blocks > cus) blocks = cus;
    hipLaunchKernelGGL(occupancy_render_kernel, dim3(blocks), dim3(FBLOCK), lds_bytes, (hipStream_t)stream, a, oc);
    return ac::check_launch("render_rays_occupancy");
}

AC_API int ac_render_rays_occupancy(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                                    float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                                    float *weights_sum, float *depth, float *image, float *normal_map, uint32_t *n_samples, uint32_t max_steps,
                                    ac_stream_t stream)
{
    return render_rays_occupancy_impl(field, rays_o, rays_d, N, grid, H, mean_density, bound, eps, inv_s, inv_s_dev, cos_anneal_ratio, weights_sum, depth, image,
                                      normal_map, n_samples, max_steps, stream, nullptr);
}

// scratch of ac_render_rays_occupancy_train: [16] sync words (word 8: launches whose grid barrier timed out, sticky) | [chunks] totals | counts, offsets, overflow flags, word masks [N] each | records [N][32] | [CUs][2] doubles |
// packed samples: ray [M], x y z dt [M][4], alpha r g b nx ny nz - [M][8].  ZERO-FILLED by the caller once (the sync words and the totals; every call leaves
// them zero again), reusable for calls with the SAME N and capacity on the same stream (the layout depends on both).
struct OccTrainLayout { size_t tot, cnt, offs, ovf, wmask, rec, part, p_ray, p_in, p_out, total; };
static OccTrainLayout occ_train_layout(uint32_t N, uint32_t M)
{
    OccTrainLayout l{};
    const size_t chunks = ((size_t)N + (1u << OT_CHUNK_LOG) - 1) >> OT_CHUNK_LOG;
    size_t o = 16 * sizeof(uint32_t);
    l.tot = o; o += chunks * sizeof(int32_t);
    l.cnt = o; o += (size_t)N * sizeof(int32_t);
    l.offs = o; o += (size_t)N * sizeof(int32_t);
    l.ovf = o; o += (size_t)N * sizeof(int32_t);
    l.wmask = o; o += (size_t)N * sizeof(uint32_t);
    l.rec = o; o += (size_t)N * RM_REC_WORDS * sizeof(uint32_t);
    o = (o + 15) & ~(size_t)15;
    l.part = o; o += (size_t)ac::cu_count() * 2 * sizeof(double);
    l.p_ray = o; o += (size_t)M * sizeof(int32_t);
    o = (o + 15) & ~(size_t)15;
    l.p_in = o; o += (size_t)M * 4 * sizeof(float);
    l.p_out = o; o += (size_t)M * 8 * sizeof(float);
    l.total = o;
    return l;
}
AC_API size_t ac_render_rays_occupancy_train_scratch(uint32_t N, uint32_t capacity) { return occ_train_layout(N, capacity).total; }

AC_API int ac_render_rays_occupancy_train(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                                          float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                                          uint32_t perturb, uint32_t capacity, uint32_t composite_capacity, int32_t *counter, const float *bg,
                                          uint32_t bg_mode, float bg_value, float *weights_sum, float *image, float *normal_map, float *gradient_error,
                                          void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (!gradient_error) { ac::set_error("render_rays_occupancy_train: NULL gradient_error"); return AC_ERR_BAD_ARG; }
    if (N == 0) { hipMemsetAsync(gradient_error, 0, sizeof(float), (hipStream_t)stream); return AC_OK; }
    if (int rc = check_render("render_rays_occupancy_train", rays_o && rays_d && grid && weights_sum && image && normal_map && scratch, H, eps)) return rc;
    if (bg_mode > 3u || (bg_mode >= 2u && !bg)) { ac::set_error("render_rays_occupancy_train: bad background mode"); return AC_ERR_BAD_ARG; }
    if (capacity == 0u || composite_capacity == 0u) {
        ac::set_error("render_rays_occupancy_train: capacity / composite_capacity must be > 0 (the packed layout lives in the scratch: a budgeted call)"); return AC_ERR_BAD_ARG;
    }
    const OccTrainLayout l = occ_train_layout(N, capacity);
    if (scratch_bytes < l.total) { ac::set_error("render_rays_occupancy_train: scratch of %zu bytes needed, %zu given", l.total, scratch_bytes); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = shade_args(a, field, bound, eps, inv_s, inv_s_dev, cos_anneal_ratio)) return rc;
    char *sc = static_cast<char *>(scratch);
    OccTrainArgs oc{ rays_o, rays_d, grid, N, H, capacity, composite_capacity, perturb, mean_density, counter, weights_sum, image, normal_map, gradient_error,
                     bg, bg_mode, bg_value, reinterpret_cast<uint32_t *>(sc), reinterpret_cast<int32_t *>(sc + l.tot), reinterpret_cast<int32_t *>(sc + l.cnt),
                     reinterpret_cast<int32_t *>(sc + l.offs), reinterpret_cast<int32_t *>(sc + l.ovf), reinterpret_cast<uint32_t *>(sc + l.wmask),
                     reinterpret_cast<uint32_t *>(sc + l.rec),
                     reinterpret_cast<double *>(sc + l.part), reinterpret_cast<int32_t *>(sc + l.p_ray), reinterpret_cast<float *>(sc + l.p_in),
                     reinterpret_cast<float *>(sc + l.p_out), ot_spin_ticks() };
    const size_t lds_bytes = FWD_LDS_FLOATS * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(occupancy_train_kernel), lds_bytes);
    // one persistent workgroup per compute unit AT MOST: the kernel's grid barriers need every workgroup resident (FBLOCK threads at two waves per SIMD and
    // the LDS image make it one per CU); fewer when the batch has less than one 64-ray wave of walking per workgroup
    const uint32_t cus = ac::cu_count();
    uint32_t blocks = (N + 63u) / 64u;
    if (blocks > cus) blocks = cus;
    if (blocks < cus && capacity / 16u > blocks * FW) blocks = cus;         // (the tiles of phase C want every wave)
    void *params[2] = { &a, &oc };
    return ac::launch_resident("render_rays_occupancy_train", reinterpret_cast<const void *>(occupancy_train_kernel), blocks, FBLOCK, lds_bytes, (hipStream_t)stream, params);
}

AC_API uint32_t ac_set_occupancy_barrier_ms(uint32_t ms)
{
    const uint32_t prev = g_barrier_ms.exchange(ms, std::memory_order_relaxed);
    return prev ? prev : ot_default_ms();
}

// scratch of ac_render_rays_occupancy_phased: [16] sync words | alive lists [2][N] | per-ray state [N][4] | per-entry counts [N] | tile list [N << nlog] |
// sample slots in / out [N << nlog][8] each.  ZERO-FILLED by the caller once (the sync words; every call leaves them zero again); any call with the same or a
// smaller N may reuse it on the same stream.
struct OccPhLayout { size_t alive, st, cnt, list, s_in, s_out, total; };
constexpr uint32_t OCC_PHASED_NLOG = 4;          // log2 of n_step, the samples per ray and round
static OccPhLayout occ_phased_layout(uint32_t N)
{
    constexpr uint32_t nlog = OCC_PHASED_NLOG;
    OccPhLayout l{};
    size_t o = 16 * sizeof(uint32_t);
    l.alive = o; o += 2 * (size_t)N * sizeof(int32_t);
    o = (o + 15) & ~(size_t)15;
    l.st = o; o += (size_t)N * 4 * sizeof(float);
    l.cnt = o; o += (size_t)N * sizeof(uint32_t);
    l.list = o; o += ((size_t)N << nlog) * sizeof(uint32_t);
    o = (o + 15) & ~(size_t)15;
    l.s_in = o; o += ((size_t)N << nlog) * 8 * sizeof(float);
    l.s_out = o; o += ((size_t)N << nlog) * 8 * sizeof(float);
    l.total = o;
    return l;
}
AC_API size_t ac_render_rays_occupancy_phased_scratch(uint32_t N) { return occ_phased_layout(N).total; }

AC_API int ac_render_rays_occupancy_phased(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                                           float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                                           float *weights_sum, float *depth, float *image, float *normal_map, uint32_t *n_samples, uint32_t max_steps,
                                           void *scratch, size_t scratch_bytes, ac_stream_t stream)
{
    if (N == 0) return AC_OK;
    if (int rc = check_render("render_rays_occupancy_phased", rays_o && rays_d && grid && weights_sum && depth && image && normal_map && scratch, H, eps)) return rc;
    const uint32_t nlog = OCC_PHASED_NLOG;
    if (((uint64_t)N << nlog) >= (1ull << 31)) { ac::set_error("render_rays_occupancy_phased: too many rays for 32-bit slot ids"); return AC_ERR_BAD_ARG; }
    const OccPhLayout l = occ_phased_layout(N);
    if (scratch_bytes < l.total) { ac::set_error("render_rays_occupancy_phased: scratch of %zu bytes needed, %zu given", l.total, scratch_bytes); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = shade_args(a, field, bound, eps, inv_s, inv_s_dev, cos_anneal_ratio)) return rc;
    char *sc = static_cast<char *>(scratch);
    OccPhArgs oc{ rays_o, rays_d, grid, N, H, max_steps, nlog, mean_density, weights_sum, depth, image, normal_map, n_samples,
                  reinterpret_cast<uint32_t *>(sc), reinterpret_cast<int32_t *>(sc + l.alive), reinterpret_cast<float *>(sc + l.st),
                  reinterpret_cast<uint32_t *>(sc + l.cnt), reinterpret_cast<uint32_t *>(sc + l.list), reinterpret_cast<float *>(sc + l.s_in),
                  reinterpret_cast<float *>(sc + l.s_out), ot_spin_ticks() };
    const bool tab = (FWD_LDS_FLOATS + (size_t)H + 1) * sizeof(float) + 64 <= 160 * 1024;
    const size_t lds_bytes = (FWD_LDS_FLOATS + (tab ? (size_t)H + 1 : 0)) * sizeof(float);
    static uint64_t seen = 0;
    ac::allow_dynamic_lds(seen, reinterpret_cast<const void *>(occupancy_phased_kernel), 160 * 1024 - 64);
    // one persistent workgroup per compute unit AT MOST (grid barriers: every workgroup must be resident)
    const uint32_t cus = ac::cu_count();
    uint32_t blocks = (N + 63u) / 64u;
    if (blocks > cus) blocks = cus;
    if (blocks < cus && N / 4u > blocks * FW) blocks = cus;              // (the tiles of phase F want every wave)
    void *params[2] = { &a, &oc };
    if (int rc = ac::launch_resident("render_rays_occupancy_phased", reinterpret_cast<const void *>(occupancy_phased_kernel), blocks, FBLOCK, lds_bytes, (hipStream_t)stream, params)) return rc;
    // never a partial result (the reference's loop, raymarching/raymarching.py:136-188, cannot produce one): the barrier-free kernel is queued behind the
    // phased one and does nothing unless that launch's verdict word says a grid barrier timed out -- then it renders every ray again (the same bits: tests)
    return render_rays_occupancy_impl(field, rays_o, rays_d, N, grid, H, mean_density, bound, eps, inv_s, inv_s_dev, cos_anneal_ratio, weights_sum, depth, image,
                                      normal_map, n_samples, max_steps, stream, reinterpret_cast<const uint32_t *>(sc) + 9);
}

// ---- the shading glue of run_cuda's TRAINING form under autograd (round 6) ---------------------------------------------------------------
// Between the fused SDF query (ac_sdf_stencil_*) and the packed compositor (composite_rays_train) the chain ran ~40 torch kernels forward and backward per batch
// (normalisation of the finite-difference gradient, the cos-annealed NeuS alpha, the eikonal term): 2.5 ms per 4096-ray batch against 0.5 ms for the no-grad launch.
// One elementwise kernel each way, the arithmetic of ac_field_samples (forward) and of composite_bwd_kernel / core_mid_kernel (backward):
//   normal = g / (1e-5 + |g|);  alpha = clip((pc - nc + 1e-5) / (pc + 1e-5), 0, 1), pc / nc = sigmoid((sdf -+ half) inv_s), half = iter_cos dt / 2,
//   iter_cos = -(softplus(-tc / 2 + 1 / 2) (1 - car) + softplus(-tc) car), tc = d . normal;  eik = (relax (|g| - 1)^2, relax), relax = [|x| < 1.2][row < n_valid]
struct PackedShade {
    const float *sdf16, *gradient, *xyzs, *dirs, *deltas;
    uint32_t delta_stride, M;
    const int32_t *n_valid;             // device scalar: rows >= *n_valid are alignment padding (no eikonal share)
    float inv_s; const float *inv_s_dev; float car, one_m_car;
};
__global__ __launch_bounds__(256) void packed_shading_fwd_kernel(const PackedShade a, float *__restrict__ alpha, float *__restrict__ normal, float *__restrict__ eik)
{
    __shared__ float spg[SPQ_FLOATS];
    for (int e = threadIdx.x; e < SPQ_FLOATS; e += blockDim.x) spg[e] = AC_SP_G[e >> 2][e & 3];
    __syncthreads();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.M) return;
    const float inv_s = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
    const size_t b3 = 3 * (size_t)b;
    const float gx = a.gradient[b3], gy = a.gradient[b3 + 1], gz = a.gradient[b3 + 2];
    const float r = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz), c = 1e-5f + r;
    const float nx = gx / c, ny = gy / c, nz = gz / c;
    const float tc = (a.dirs[b3] * nx + a.dirs[b3 + 1] * ny) + a.dirs[b3 + 2] * nz;
    RenderArgs ra{}; ra.car = a.car; ra.one_m_car = a.one_m_car;                 // (what neus_alpha reads: these two and the table at its place in the LDS image)
    alpha[b] = neus_alpha(spg - OFF_SPQ, ra, tc, a.sdf16[(size_t)b * 16], a.deltas[(size_t)b * a.delta_stride], inv_s);
    normal[b3] = nx; normal[b3 + 1] = ny; normal[b3 + 2] = nz;
    const float px = a.xyzs[b3], py = a.xyzs[b3 + 1], pz = a.xyzs[b3 + 2];
    const float relax = (__builtin_sqrtf((px * px + py * py) + pz * pz) < 1.2f && (int32_t)b < *a.n_valid) ? 1.0f : 0.0f;
    eik[2 * (size_t)b] = relax * ((r - 1.0f) * (r - 1.0f)); eik[2 * (size_t)b + 1] = relax;
}
__global__ __launch_bounds__(256) void packed_shading_bwd_kernel(const PackedShade a, const float *__restrict__ g_alpha, const float *__restrict__ g_normal,
                                                                 const float *__restrict__ g_eik, float *__restrict__ g_sdf16, float *__restrict__ g_gradient,
                                                                 float *__restrict__ g_inv_s_rows)
{
    __shared__ float spg[SPQ_FLOATS];
    for (int e = threadIdx.x; e < SPQ_FLOATS; e += blockDim.x) spg[e] = AC_SP_G[e >> 2][e & 3];
    __syncthreads();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.M) return;
    const float inv_s = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;
    const size_t b3 = 3 * (size_t)b;
    const float gx = a.gradient[b3], gy = a.gradient[b3 + 1], gz = a.gradient[b3 + 2];
    const float r = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz), c = 1e-5f + r;
    const float nx = gx / c, ny = gy / c, nz = gz / c;
    const float dx = a.dirs[b3], dy = a.dirs[b3 + 1], dz = a.dirs[b3 + 2];
    const float tc = (dx * nx + dy * ny) + dz * nz;
    float v1, d1, v2, d2;
    softplus100_vg(spg, -tc * 0.5f + 0.5f, v1, d1);
    softplus100_vg(spg, -tc, v2, d2);
    const float delta = a.deltas[(size_t)b * a.delta_stride];
    const float half = -(v1 * a.one_m_car + v2 * a.car) * delta * 0.5f;
    const float sdf = a.sdf16[(size_t)b * 16];
    const float pc = dv_sigmoid((sdf - half) * inv_s), nc = dv_sigmoid((sdf + half) * inv_s);
    const float den = pc + 1e-5f, u = (pc - nc + 1e-5f) / den;
    const float du = (u >= 0.0f && u <= 1.0f) ? (g_alpha ? g_alpha[b] : 0.0f) : 0.0f;      // torch.clip passes the gradient on the closed interval
    const float dpc = du * nc / (den * den), dnc = -du / den;
    const float dap = dpc * pc * (1.0f - pc), dan = dnc * nc * (1.0f - nc);
    g_sdf16[(size_t)b * 16] = (dap + dan) * inv_s;
    g_inv_s_rows[b] = dap * (sdf - half) + dan * (sdf + half);
    const float dic = (dan - dap) * inv_s * delta * 0.5f;
    const float dtc = dic * (0.5f * d1 * a.one_m_car + d2 * a.car);
    const float ux = (g_normal ? g_normal[b3] : 0.0f) + dtc * dx, uy = (g_normal ? g_normal[b3 + 1] : 0.0f) + dtc * dy, uz = (g_normal ? g_normal[b3 + 2] : 0.0f) + dtc * dz;
    float k = 0.0f;
    if (r > 0.0f) {
        k = -((gx * ux + gy * uy) + gz * uz) / (r * c * c);                 // d (1 / (1e-5 + r)) / dg = -g / (r c^2)
        const float px = a.xyzs[b3], py = a.xyzs[b3 + 1], pz = a.xyzs[b3 + 2];
        const float relax = (__builtin_sqrtf((px * px + py * py) + pz * pz) < 1.2f && (int32_t)b < *a.n_valid) ? 1.0f : 0.0f;
        if (g_eik) k += g_eik[2 * (size_t)b] * relax * 2.0f * (r - 1.0f) / r;
    }
    g_gradient[b3] = ux / c + k * gx; g_gradient[b3 + 1] = uy / c + k * gy; g_gradient[b3 + 2] = uz / c + k * gz;
}
static int packed_shade_args(PackedShade &a, const char *who, const float *sdf16, const float *gradient, const float *xyzs, const float *dirs, const float *deltas,
                             uint32_t delta_stride, uint32_t M, const int32_t *n_valid, float inv_s, const float *inv_s_dev, float car)
{
    if (!sdf16 || !gradient || !xyzs || !dirs || !deltas || !n_valid || delta_stride < 1 || delta_stride > 2) { ac::set_error("%s: NULL buffer or delta_stride not 1 / 2", who); return AC_ERR_BAD_ARG; }
    a = PackedShade{ sdf16, gradient, xyzs, dirs, deltas, delta_stride, M, n_valid, inv_s, inv_s_dev, car, (float)(1.0 - (double)car) };
    return AC_OK;
}
AC_API int ac_packed_shading_forward(const float *sdf16, const float *gradient, const float *xyzs, const float *dirs, const float *deltas, uint32_t delta_stride,
                                     uint32_t M, const int32_t *n_valid, float inv_s, const float *inv_s_dev, float cos_anneal_ratio, float *alpha, float *normal,
                                     float *eik, ac_stream_t stream)
{
    if (M == 0) return AC_OK;
    PackedShade a;
    if (int rc = packed_shade_args(a, "packed_shading_forward", sdf16, gradient, xyzs, dirs, deltas, delta_stride, M, n_valid, inv_s, inv_s_dev, cos_anneal_ratio)) return rc;
    if (!alpha || !normal || !eik) { ac::set_error("packed_shading_forward: NULL output"); return AC_ERR_BAD_ARG; }
    hipLaunchKernelGGL(packed_shading_fwd_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, alpha, normal, eik);
    return ac::check_launch("packed_shading_forward");
}
AC_API int ac_packed_shading_backward(const float *sdf16, const float *gradient, const float *xyzs, const float *dirs, const float *deltas, uint32_t delta_stride,
                                      uint32_t M, const int32_t *n_valid, float inv_s, const float *inv_s_dev, float cos_anneal_ratio, const float *g_alpha,
                                      const float *g_normal, const float *g_eik, float *g_sdf16, float *g_gradient, float *g_inv_s_rows, ac_stream_t stream)
{
    if (M == 0) return AC_OK;
    PackedShade a;
    if (int rc = packed_shade_args(a, "packed_shading_backward", sdf16, gradient, xyzs, dirs, deltas, delta_stride, M, n_valid, inv_s, inv_s_dev, cos_anneal_ratio)) return rc;
    if (!g_sdf16 || !g_gradient || !g_inv_s_rows) { ac::set_error("packed_shading_backward: NULL output"); return AC_ERR_BAD_ARG; }
    hipLaunchKernelGGL(packed_shading_bwd_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, g_alpha, g_normal, g_eik, g_sdf16, g_gradient, g_inv_s_rows);
    return ac::check_launch("packed_shading_backward");
}
