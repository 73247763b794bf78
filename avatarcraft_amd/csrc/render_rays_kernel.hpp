// avatarcraft_amd/csrc/render_rays_kernel.hpp -- the text of the fused renderer's kernel.  Included by render_fused.hip (inside its anonymous namespace) once per
// table format, with
//   AC_RENDER_KERNEL  the kernel's name
//   AC_RENDER_H16     false: the fp32 hash table (two floats per entry);  true: the half table of ac_table_to_half (one dword per entry: a.table /
//                     a.table_bytes describe n_entries dwords) -- every gather is one dword, widened exactly (hash_gather.hpp: table_entry); nothing else
//                     differs, so a render equals the fp32 kernel's render of the widened table bit for bit.
// A second inclusion instead of a template parameter or a shared body function: the fp32 kernels keep their names and their instruction stream
// (DESIGN.md section 5.9); no include guard on purpose.
template <int MODE, bool FAST, bool EX, bool SH = false>
__global__ __launch_bounds__(BLOCK) void AC_RENDER_KERNEL(const RenderArgs a)
{
    constexpr bool FC = FAST;                                // fast precision: the colour network in split bf16 too
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (a.prepared) {
        // the weights arrive in LDS order (ac_field_prepare): a linear copy, 16 bytes per lane and trip, instead of ~27 dependent
        // gather-and-place trips per thread in each of the 512 workgroups of a launch; only the per-launch sampling tables are added
        const float4 *src = reinterpret_cast<const float4 *>(a.prepared);
        float4 *dst = reinterpret_cast<float4 *>(lds);
        // (fast precision: the colour region holds the split-bf16 fragments, which the image keeps behind the exact one)
        for (int e = threadIdx.x; e < OFF_RWAVE / 4; e += blockDim.x)
            dst[e] = src[(FC && 4 * e >= OFF_C1F && 4 * e < OFF_B1) ? e + (OFF_RWAVE - OFF_C1F) / 4 : e];
        __syncthreads();
        for (int e = threadIdx.x; e < 64; e += blockDim.x) lds[OFF_LIN + e] = e < a.T0 ? a.lin_z[e] : 0.0f;
        for (int e = threadIdx.x; e < 16; e += blockDim.x) lds[OFF_LIN + 64 + e] = a.lin_u ? a.lin_u[e] : 0.0f;
    } else {
        fill_lds_sdf(lds, a);
        if constexpr (FAST) fill_lds_fast(lds, a);
        if constexpr (FC) fill_lds_color_fast<true, true>(lds, a);
        else fill_lds_color(lds, a);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    float *zs0 = lds + OFF_RWAVE + wave * WAVE_SLAB;    // z buffer 0 [128]: where the final samples of the ray end up
    float *zs1 = zs0 + MAXT;                            // --- from here on: up-sampling state while the ray is being sampled ...
    float *sd = zs1 + MAXT;                             // sd[2][128]
    float *cdf = sd + 2 * MAXT;                         // cdf[128]
    float *znl = cdf + MAXT;                            // znew[16]
    float *fsl = zs1;                                   // ... and the features of the finite-difference points [6][8][64] afterwards
    const FieldCtx fc = make_ctx(a);
    const W2Row0 w2r0 = load_w2_row0(lds, lane);
    const float bound = a.bound;
    const float inv_s_core = a.inv_s_dev ? *a.inv_s_dev : a.inv_s;     // forward_variance(): a launch constant, or one float on the device
    const int T0 = a.T0, nup = a.nup, T = T0 + 16 * nup;

#ifdef AC_PROFILE
    unsigned long long prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long prof_t0 = __builtin_amdgcn_s_memtime(), prof_r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long prof_bnd[2] = {0, 0}, prof_bm = prof_t0;
#endif
    // XCD-aware order: workgroup b runs on XCD b % 8 (observed dispatch rule; speed only): give every XCD a contiguous
    // slab of rays so that neighbouring pixels share one L2 instead of eight
    int bid = blockIdx.x;
    {   // XCD k runs the workgroups b with b % 8 == k: give it the k-th contiguous range (ranges differ by one when 8 does not divide the grid)
        const int k = blockIdx.x & 7, q = gridDim.x >> 3, r = gridDim.x & 7;
        bid = k * q + (k < r ? k : r) + (blockIdx.x >> 3);
    }
    // Staggered start: wave w of a workgroup begins AC_START_STAGGER x 4096 clocks (~2 us each) x w late.  All 2048 waves of a launch would otherwise walk
    // through the same phases of their first ray together (every wave gathering, then every wave in the MLPs): rays of the first round took 350 .. 420 us
    // against 280 .. 330 us for the ones fetched later, when the waves have drifted apart (tools/phase_profile.py).  Round 2 used 3 (6 us per wave index, 41 us
    // for the last wave); with quarter-ray work items (round 3) 1 = 2 us per index, 14 us for the last wave, does the same (0.762 vs 0.760 ms; none: 0.776,
    // profiles/r03_experiments.txt section 14).
#ifndef AC_START_STAGGER
#define AC_START_STAGGER 1
#endif
    // (only launches that fill the device: a small batch -- a posed frame's tail, a unit test -- has no lock-step to break and would only pay the delay)
    if (a.n_rays >= 2048)
        for (int k_ = 0; k_ < AC_START_STAGGER * wave; ++k_) __builtin_amdgcn_s_sleep(64);
    // Work items are runs of tiles of one ray, fetched one at a time: every XCD has ONE ticket counter, and ticket t takes item t of the XCD's work list
    // (render_worklist.hpp: built on the host, read here from its device copy; which ray, tiles [c_begin, c_end), the item's number within its ray,
    // whether the sampling stage rides on it, whether it writes the pixel).  A wave that finishes an item which is not the ray's last leaves the ray's z
    // values and running sums in seg_state and raises the ray's flag; whichever wave of the XCD takes the ray's next item continues the SAME sequential
    // arithmetic from there (bit-identical results for every list).  A 4096-ray launch is only two rays per wave slot, and with whole rays as work items
    // it ended with the slowest pair (per-wave busy time: mean 664 us, max 802 us); how the rays are cut decides how the launch ends.
    // A wave never waits for an item nobody holds: a list is a linear extension of "item k of a ray before item k + 1", so the predecessor of an item has a
    // smaller ticket, and tickets are only ever taken by resident waves (one workgroup per compute unit: the whole grid is resident).
    // The batch is dealt to the XCDs in chunks of AC_XCD_CHUNK consecutive rays (two image rows of a 256-wide view: neighbouring rays share grid
    // cells in the XCD's L2), chunk c to XCD c % 8; a batch of up to 8 chunks is cut into eight contiguous parts.  Large batches stay balanced
    // that way when the body covers only some rows of the image (posed frames, skip_masked).  (The lists are built with the same chunking.)
    // The two posed-space halves (MODE_UPSAMPLE, MODE_FINAL) keep one item per ray and no list: their tickets are decoded in closed form.
    constexpr bool LISTED = MODE == MODE_FULL;
    const int xchunk = ac_worklist::xcd_chunk(a.n_rays), xcd = blockIdx.x & 7;
    uint32_t *const tk_counter = a.ray_counter + xcd * 8;
    // (the list is read-only for the whole launch and its words are fetched at wave-uniform indices: scalar loads through the constant address space)
    const __attribute__((address_space(4))) uint32_t *const wl = (const __attribute__((address_space(4))) uint32_t *)a.work_list;
    uint32_t wl_cnt = 0;
    const __attribute__((address_space(4))) uint32_t *wl_items = wl;
    if constexpr (LISTED) { wl_cnt = wl[ac_worklist::XCDS + xcd]; wl_items = wl + ac_worklist::HEADER_WORDS + 2 * (size_t)wl[xcd]; }
#define AC_TAKE_TICKET(TK) { uint32_t v_ = 0; if (lane == 0) v_ = atomicAdd(tk_counter, 1u); TK = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_); }
#define AC_FETCH_ITEM(TK, W0, W1) { W0 = 0u; W1 = 0u; if (TK < wl_cnt) { W0 = wl_items[2 * (size_t)TK]; W1 = wl_items[2 * (size_t)TK + 1]; } }
    uint32_t tk = 0, it_ray = 0, it_meta = 0;              // the wave's next ticket and (LISTED) its item, all wave-uniform
    if constexpr (LISTED) { AC_TAKE_TICKET(tk) AC_FETCH_ITEM(tk, it_ray, it_meta) }
    for (;;) {
        int ray = 0, c_begin = 0, c_end = MAXT / 16, seq = 0;
        bool seg_first = true, seg_last = true;
        bool tk_ahead = false;                                       // LISTED: this item has already taken the wave's next ticket (see the tile loop)
        if constexpr (LISTED) {
            if (tk >= wl_cnt) break;
            ray = (int)it_ray;
            c_begin = ac_worklist::meta_begin(it_meta); c_end = ac_worklist::meta_end(it_meta); seq = ac_worklist::meta_seq(it_meta);
            seg_first = (it_meta & ac_worklist::META_SAMPLING) != 0u; seg_last = (it_meta & ac_worklist::META_LAST) != 0u;
        } else {
            AC_TAKE_TICKET(tk)
            ray = ac_worklist::ticket_to_work(a.n_rays, xchunk, xcd, (int)tk);
            if (ray == ac_worklist::TICKET_END) break;
            if (ray == ac_worklist::TICKET_GAP) continue;
        }
        int rin = ray;                                               // row of this ray in rays_o / rays_d / near_m / far_m
        if (LISTED && a.pair_n && ray >= a.pair_n) rin = ray - a.pair_n;      // (pair launches: the list hands the copies out as a0 b0 a1 b1 ...: the two copies of a ray meet in their XCD's L2)
        (void)bid;                                                   // (used by the static hand-out, removed; dropping the remap changes the kernel's register setup)
        const int exr = ray - a.ex_from;                             // row in the per-sample outputs (pair launches keep them for copy b only)
        const bool ex_on = exr >= 0;
        AC_BND_TICK(0)
        AC_T0();
        const float ox = a.rays_o[3 * rin], oy = a.rays_o[3 * rin + 1], oz = a.rays_o[3 * rin + 2];
        const float dx = a.rays_d[3 * rin], dy = a.rays_d[3 * rin + 1], dz = a.rays_d[3 * rin + 2];
        float near, far;
        cube_near_far(ox, oy, oz, dx, dy, dz, bound, near, far);
        if (a.near_m) {                                          // :148-153 mesh-guided range where the ray passes the body
            const float nm = a.near_m[rin], fm = a.far_m[rin];
            if (!is_inf(nm)) near = nm;
            if (!is_inf(fm)) far = fm;
        }
        const float span = far - near;
        const float sample_dist = span / (float)T0;
        int cur = (MODE == MODE_FINAL) ? 0 : (nup & 1), cnt = T0;      // the buffers swap once per up-sampling iteration: start so that the last lands in zs0
        float *const zs_first = cur ? zs1 : zs0;

        if constexpr (MODE == MODE_UPSAMPLE) {
            // skip_masked: no sample of this ray can be unmasked (ray_cull_kernel) -- its pixel is the background whatever the field says, so neither
            // the coarse SDF nor the up-sampling runs; the z array is the coarse one padded with its last value (sorted, finite)
            if (a.ray_dead && a.ray_dead[ray]) {
                for (int i = lane; i < T; i += 64) {
                    const int ic = i < T0 ? i : T0 - 1;
                    float zi = near + span * lds[OFF_LIN + ic];
                    if (a.perturb) zi = zi + (a.noise[(size_t)ray * T0 + ic] - 0.5f) * sample_dist;
                    const size_t si = (size_t)ray * T + i;
                    a.zbuf[si] = zi;
                    if (a.mid_pts) { a.mid_pts[3 * si] = ox + dx * zi; a.mid_pts[3 * si + 1] = oy + dy * zi; a.mid_pts[3 * si + 2] = oz + dz * zi; }
                }
                wave_sync();
                continue;
            }
        }
        // ---- coarse samples :155-180 -------------------------------------------------------------
        if constexpr (MODE == MODE_FINAL) {
            for (int i = lane; i < T; i += 64) zs0[i] = a.zbuf[(size_t)ray * T + i];
        } else if (seg_first) {
            for (int c = 0; c < T0 / 16; ++c) {
                const int i = 16 * c + n;
                float zi = near + span * lds[OFF_LIN + i];
                if (a.perturb) zi = zi + (a.noise[(size_t)ray * T0 + i] - 0.5f) * sample_dist;
                if (nup > 0) {
                    float px, py, pz;
                    if (MODE == MODE_UPSAMPLE && a.ext_pts) {       // posed space: the warped coarse points (NULL: canonical sampling only)
                        const float *e = a.ext_pts + ((size_t)ray * T0 + i) * 3;
                        px = clampf(e[0], -bound, bound); py = clampf(e[1], -bound, bound); pz = clampf(e[2], -bound, bound);
                    } else {
                        px = clampf(ox + dx * zi, -bound, bound); py = clampf(oy + dy * zi, -bound, bound);
                        pz = clampf(oz + dz * zi, -bound, bound);
                    }
                    const f32x4 o2 = sdf_tile<AC_RENDER_H16>(lds, fc, lane, px, py, pz);
                    if (g == 0) sd[cur * MAXT + i] = o2[0];
                }
                if (g == 0) zs_first[i] = zi;
            }
        }
        wave_sync();
        AC_TICK(0)

        // ---- NeuS up-sampling :182-184, :410-475 -----------------------------------------------------
        for (int it = 0; it < ((MODE == MODE_FINAL || !seg_first) ? 0 : nup); ++it) {
            const float *zc = cur ? zs1 : zs0, *sc = sd + cur * MAXT;
            float *zn_ = cur ? zs0 : zs1, *sn_ = sd + (cur ^ 1) * MAXT;
            const int m = cnt - 1;
            const float inv_s = (float)(64 << it);
            float w[2];
            float carry = 1.0f; bool first = true;
            // pass 1: alpha, transmittance scan, weights (+1e-5)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const int i = 64 * ch + lane;
                float alpha = 0.0f, om = 1.0f;
                if (i < m) {
                    const float z0 = zc[i], z1 = zc[i + 1], s0 = sc[i], s1 = sc[i + 1];
                    const float p0x = ox + dx * z0, p0y = oy + dy * z0, p0z = oz + dz * z0;
                    const float p1x = ox + dx * z1, p1y = oy + dy * z1, p1z = oz + dz * z1;
                    const float r0 = __builtin_sqrtf((p0x * p0x + p0y * p0y) + p0z * p0z);
                    const float r1 = __builtin_sqrtf((p1x * p1x + p1y * p1y) + p1z * p1z);
                    const bool inside = (r0 < 1.0f) | (r1 < 1.0f);
                    const float mid = (s0 + s1) * 0.5f;
                    const float dist = z1 - z0;
                    const float cosv = (s1 - s0) / (dist + 1e-5f);
                    float prev_cos = 0.0f;
                    if (i > 0) { const float zm = zc[i - 1], sm = sc[i - 1]; prev_cos = (s0 - sm) / ((z0 - zm) + 1e-5f); }
                    float cmin = prev_cos < cosv ? prev_cos : cosv;
                    cmin = clampf(cmin, -1e3f, 0.0f) * (inside ? 1.0f : 0.0f);
                    const float half = cmin * dist * 0.5f;
                    const float pc = dv_sigmoid((mid - half) * inv_s), nc = dv_sigmoid((mid + half) * inv_s);
                    alpha = (pc - nc + 1e-5f) / (pc + 1e-5f);
                    om = 1.0f - alpha + 1e-7f;
                }
                float loc, row_in; bool row_first;
                (void)chunk_scan<true>(om, lane, carry, first, loc, row_in, row_first);
                // exclusive transmittance T_i = cp[i-1]: row-local inclusive value of lane n-1 times the row carry
                const float sh = dpp_shr<1>(1.0f, loc);                 // local[n-1], identity in lane n==0
                float Tex;
                if (n == 0) Tex = row_first ? 1.0f : row_in;
                else Tex = row_first ? sh : row_in * sh;
                w[ch] = (i < m) ? alpha * Tex + 1e-5f : 0.0f;
            }
            // pass 2: total = last element of the inclusive add tile-scan of w
            float total;
            {
                float c2 = 0.0f; bool f2 = true; float lc, ri; bool rf;
                float last = 0.0f;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const float incl = chunk_scan<false>(w[ch], lane, c2, f2, lc, ri, rf);
                    const int il = m - 1 - 64 * ch;                    // lane holding element m-1 (wave-uniform)
                    const float cand = __shfl(incl, il & 63);
                    if (il >= 0 && il < 64) last = cand;
                }
                total = last;
            }
            // pass 3: pdf, cdf
            {
                float c3 = 0.0f; bool f3 = true; float lc, ri; bool rf;
                if (lane == 0) cdf[0] = 0.0f;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const int i = 64 * ch + lane;
                    const float pdf = (i < m) ? w[ch] / total : 0.0f;
                    const float incl = chunk_scan<false>(pdf, lane, c3, f3, lc, ri, rf);
                    if (i < m) cdf[i + 1] = incl;
                }
            }
            wave_sync();
            // sample_pdf(det=True): one new sample per n (replicated over the 4 groups)
            float znew;
            int ind;
            {
                const float u = lds[OFF_LIN + 64 + n];
                int lo = 0, hi = cnt;
                while (lo < hi) { const int md = (lo + hi) >> 1; if (cdf[md] <= u) lo = md + 1; else hi = md; }
                ind = lo;
                const int below = lo - 1 > 0 ? lo - 1 : 0;
                const int above = lo < cnt - 1 ? lo : cnt - 1;
                const float cb = cdf[below], ca = cdf[above];
                float den = ca - cb;
                if (den < 1e-5f) den = 1.0f;
                const float t = (u - cb) / den;
                const float zb = zc[below], za = zc[above];
                znew = zb + t * (za - zb);
            }
            if (g == 0) {
                znl[n] = znew;
                if (EX && ex_on && a.out.ss_inds) a.out.ss_inds[((size_t)exr * nup + it) * 16 + n] = ind;
            }
            AC_TICK(1)
            const bool last_it = (it + 1 == nup);
            float sdf_new = 0.0f;
            if (!last_it) {
                const float px = clampf(ox + dx * znew, -bound, bound), py = clampf(oy + dy * znew, -bound, bound),
                            pz = clampf(oz + dz * znew, -bound, bound);
                const f32x4 o2 = sdf_tile<AC_RENDER_H16>(lds, fc, lane, px, py, pz);
                sdf_new = o2[0];
            }
            wave_sync();
            AC_TICK(2)
            // stable merge == torch.sort(cat([z, znew])) :466-473.  The old z are sorted except in the first iteration of a ray whose slab
            // test gave far < near (it misses the cube: its coarse z run from near DOWN to far): there the old elements are ranked too
            const bool old_sorted = !(it == 0 && span < 0.0f);         // wave-uniform
            int32_t *sidx = (EX && ex_on && a.out.sort_index) ? a.out.sort_index + ((size_t)exr * nup + it) * 128 : nullptr;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const int i = 64 * ch + lane;
                if (i < cnt) {
                    const float zi = zc[i];
                    int c = 0;
#pragma unroll
                    for (int j = 0; j < 16; ++j) c += (znl[j] < zi) ? 1 : 0;
                    int before = i;
                    if (!old_sorted) {
                        before = 0;
                        for (int k = 0; k < cnt; ++k) { const float zk = zc[k]; before += ((zk < zi) || (zk == zi && k < i)) ? 1 : 0; }
                    }
                    zn_[before + c] = zi; sn_[before + c] = sc[i];
                    if (sidx) sidx[before + c] = i;
                }
                if (sidx && i >= cnt + 16) sidx[i] = -1;
            }
            if (g == 0) {
                int lo = 0, hi = cnt;
                if (old_sorted) {
                    while (lo < hi) { const int md = (lo + hi) >> 1; if (zc[md] <= znew) lo = md + 1; else hi = md; }
                } else {
                    for (int k = 0; k < cnt; ++k) lo += (zc[k] <= znew) ? 1 : 0;
                }
                int c = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) { const float zj = znl[j]; c += ((zj < znew) || (zj == znew && j < n)) ? 1 : 0; }
                zn_[lo + c] = znew; sn_[lo + c] = sdf_new;
                if (sidx) sidx[lo + c] = cnt + n;
            }
            cnt += 16; cur ^= 1;
            wave_sync();
            AC_TICK(1)
        }

        // ---- render core :190-299 ---------------------------------------------------------------------
        const float *zf = zs0;                                  // cur == 0 here by construction
        if constexpr (MODE == MODE_UPSAMPLE) {                 // hand z and the posed-space mid points to the warp
            for (int i = lane; i < T; i += 64) {
                const float zi = zf[i];
                const float delta = (i < T - 1) ? zf[i + 1] - zi : sample_dist;
                const float zmid = (i < T - 1) ? zi + 0.5f * delta : zi;
                const size_t si = (size_t)ray * T + i;
                a.zbuf[si] = zi;
                if (a.mid_pts) { a.mid_pts[3 * si] = ox + dx * zmid; a.mid_pts[3 * si + 1] = oy + dy * zmid; a.mid_pts[3 * si + 2] = oz + dz * zmid; }
            }
            wave_sync();
            continue;
        }
        float cT = 1.0f;                                        // transmittance carry (cumprod)
        // the ten running sums of the ray (weights, colour, normal, depth, eikonal numerator / denominator) live in the wave's LDS slab, not in
        // registers: they are touched once per tile by one lane (lane 15, which holds the tile totals of the row scans), and ten registers less at the
        // peak of the stencil / MLP code is the difference between ~30 and ~10 spilled registers.  Slots: 1 s_w 2..4 rgb 5..7 normal 8 depth 9 10 eikonal
        float *const accs = zs0 + SLAB_ACC;
        // use_viewdirs: layer-1 bias of the colour network for THIS ray's direction, in the wave's slab: formed by the ray's first item (16 sh values + 64
        // dot products of 16 terms), handed to the later ones with the ray's state (64 floats: one store / one load per lane instead of the prologue again)
        if constexpr (SH && MODE != MODE_UPSAMPLE) { if (seg_first && !a.opacity_only) ray_sh_bias(zs0 + SLAB_SHB, a.Wsh, dx, dy, dz, lane); }
        if (!seg_first) {
            AC_BND_MARK();
            // continue a ray another wave (of this XCD) started: wait until its previous item is published, then take over z and the running sums.
            // All accesses to seg_flags / seg_state are agent-scope atomics = served by the XCD's L2, past the (incoherent) vector L1 caches.
            int timed_out = 0;
            if (lane == 0) {
                int spins = 0;
                // the flag of THIS launch: generation in the upper bits (a value left by an earlier launch in the same slot never matches)
                for (;;) {
                    const uint32_t f = __hip_atomic_load(a.seg_flags + ray, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((f >> 4) == a.gen && (f & 15u) >= (uint32_t)seq) || spins >= (1 << 21)) break;
                    __builtin_amdgcn_s_sleep(8); ++spins;       // (bounded: ~1 s; a ray's previous item takes ~100 us)
                }
                timed_out = spins >= (1 << 21);
                if (timed_out && a.handoff_timeouts) atomicAdd(a.handoff_timeouts, 1u);     // the host can ask (ac_render_handoff_timeouts): a lost hand-off is an ERROR, not only a NaN pixel
            }
            timed_out = __builtin_amdgcn_readfirstlane(timed_out);
            // NO acquire fence here, on purpose and measured (round 4): `fence acquire, agent` is `buffer_inv sc1` on gfx950 -- it empties the compute
            // unit's vector L1, i.e. the table lines all eight resident waves are gathering from, three times per ray: the 4096-ray launch went from
            // 0.744 to 1.087 ms with the acquire / release pair in place.  What makes the hand-off correct without it: the state and the
            // flag are written and read with agent-scope ATOMIC accesses only (they bypass the non-coherent L1 on both sides and meet at the device's
            // coherence point, whichever XCD either wave runs on); the publisher drains its state stores (s_waitcnt vmcnt(0)) before it issues the flag
            // store; the taker issues its state loads only after lane 0 has observed the flag (control dependence + the wave barrier below), and the
            // memory pipeline returns a wave's loads in issue order.  No ordinary (cached) access ever touches these words.
            // COMPILER ordering is pinned, not assumed: wave_sync() is `fence acq_rel, wavefront` + wave barrier (wave_ops.hpp) -- a wavefront-scope fence
            // costs no instruction (no cache maintenance) but forbids LLVM to move the relaxed state loads below above the flag load of the loop above
            // (ADVICE round 4); the publisher's side has the same fence between its state stores and its flag store.
            wave_sync();
            const uint32_t *st = reinterpret_cast<const uint32_t *>(a.seg_state + (size_t)ray * SEG_STATE);
            if constexpr (MODE != MODE_FINAL)
                for (int i = lane; i < T; i += 64) zs0[i] = __uint_as_float(__hip_atomic_load(st + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const float cv = __uint_as_float(__hip_atomic_load(st + MAXT + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            cT = lane_bcast(cv, 0);
            if (lane < 16) accs[lane] = cv;
            if constexpr (SH) zs0[SLAB_SHB + lane] = __uint_as_float(__hip_atomic_load(st + MAXT + 16 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (timed_out) {                                     // never observed; if the previous item was not published in ~1 s the ray's pixel must not
                cT = __builtin_nanf("");                         // look like a result: NaN, which the callers' finite checks and every parity test catch
                if (lane < 16) accs[lane] = cT;
            }
            wave_sync();
            AC_BND_TICK(1)
        }
        const float bxe = a.eps;
        const int c_hi = c_end < T / 16 ? c_end : T / 16;
        for (int c = c_begin; c < c_hi; ++c) {
            const int i = 16 * c + n;
            const float zi = zf[i];
            const float delta = (i < T - 1) ? zf[i + 1] - zi : sample_dist;
            const float zmid = (i < T - 1) ? zi + 0.5f * delta : zi;
            float px, py, pz;
            if constexpr (MODE == MODE_FINAL) {
                const float *e = a.ext_pts + ((size_t)ray * T + i) * 3;
                px = clampf(e[0], -bound, bound); py = clampf(e[1], -bound, bound); pz = clampf(e[2], -bound, bound);
            } else {
                px = clampf(ox + dx * zmid, -bound, bound); py = clampf(oy + dy * zmid, -bound, bound);
                pz = clampf(oz + dz * zmid, -bound, bound);
            }
            // centre + 6 finite-difference evaluations (:687-704): features of all 7 points first (shared corner
            // fetches), then 7 MLP passes as one loop body over a rotating feature register file.
            AC_TICK(7)
            // posed space: a tile whose 16 samples the warp masks out contributes alpha * 0 whatever the field says there (opt-in: skip_masked)
            bool skip = false;
            if constexpr (MODE == MODE_FINAL) {
                if (a.skip_masked) skip = __ballot(a.mask[(size_t)ray * T + i] != 0) == 0ull;       // wave-uniform
            }
            f32x4 oc = { 0.0f, 0.0f, 0.0f, 0.0f };
            float gr[3] = { 0.0f, 0.0f, 0.0f };
            uint32_t tk_v = 0;                                   // (LISTED, last tile of the item: the wave's next ticket on its way)
            if (!skip) {
            float fe0[4][2];
            encode_stencil<AC_RENDER_H16>(lds, fsl, fc, lane, px, py, pz, bxe, fe0);
            if (EX && ex_on && a.out.feat7) {                                     // training render: keep the 7 x 8 features of this lane (the backward streams them back)
                // layout [tile of 16 samples][14][lane][4]: float k = 8 e + q (evaluation e, slot q = 2 j + channel) of lane (n, g) sits in group k / 4,
                // component k % 4 -- every store (and every load of the backward) is one 16-byte access per lane, 1 KB contiguous per wave
                // (the lane term enters through an opaque copy: otherwise the per-lane base pointer is hoisted out of the tile loop and, at 256 registers, spilled -- a scratch
                // reload with a full wait in every tile; formed here it is one scalar product and one 64-bit add.  Round 6, profiles/r06_experiments.txt section 14)
                int lane_x = lane;
                asm volatile("" : "+v"(lane_x));
                f32x4 *dst = reinterpret_cast<f32x4 *>(a.out.feat7) + (((size_t)exr * (T / 16) + (i >> 4)) * 14) * 64 + lane_x;
                dst[0] = f32x4{ fe0[0][0], fe0[0][1], fe0[1][0], fe0[1][1] };
                dst[64] = f32x4{ fe0[2][0], fe0[2][1], fe0[3][0], fe0[3][1] };
#pragma unroll 1
                for (int e = 0; e < 6; ++e) {
                    const float *sp = fsl + (e * 8) * 64 + lane;
                    dst[(2 * e + 2) * 64] = f32x4{ sp[0], sp[64], sp[128], sp[192] };
                    dst[(2 * e + 3) * 64] = f32x4{ sp[256], sp[320], sp[384], sp[448] };
                }
            }
            AC_TICK(3)
            // (the stencil stays inline here, in render_long.hip and in field_tile.hpp's fd_forward: as one shared helper it changes the generated code)
            const float pc0 = sel4(g, px, py, pz, 0.0f);
            float spos = 0.0f;
            if constexpr (FAST) {
                // precision 1: the centre evaluation exactly (fp32 MFMA), the six offset evaluations as corrections of its layer 1 on the
                // bf16 matrix pipe (sdf_l1_delta): 12 short MFMA + ~50 VALU per evaluation instead of 36 fp32 MFMA of 32 clocks each
                const Acc4 acc0 = sdf_l1(lds, lane, pc0, fe0);
                oc = sdf_l2(lds, lane, acc0);
#pragma unroll 1
                for (int e = 0; e < 6; ++e) {
                    const int kn = e >> 1;
                    float fe[4][2];
#pragma unroll
                    for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fsl[(e * 8 + q_) * 64 + lane];
                    const float pk = kn == 0 ? px : (kn == 1 ? py : pz);
                    const float poff = clampf(pk + ((e & 1) ? -bxe : bxe), -bound, bound);
                    const Acc4 acc = sdf_l1_delta(lds, lane, acc0, fe, fe0, kn, poff - pk);
                    const float s_e = sdf_l2_sdf(lds, acc, w2r0);
                    if (!(e & 1)) spos = s_e;
                    else {
                        const float gk = 0.5f * (spos - s_e) / bxe;
                        if (kn == 0) gr[0] = gk; else if (kn == 1) gr[1] = gk; else gr[2] = gk;
                    }
                }
            } else {
            // 7 MLP passes, software-pipelined: layer 1 of evaluation e+1 (MFMA) is issued next to the softplus +
            // layer 2 of evaluation e (VALU), so the matrix and vector pipes of the SIMD overlap inside one wave.
            Acc4 acc = sdf_l1(lds, lane, pc0, fe0);
#pragma unroll 1
            for (int e = 0; e < 7; ++e) {
                Acc4 accn = acc;
                if (e < 6) {                                       // layer 1 of the next evaluation
                    const int kn = e >> 1;
                    float fe[4][2];
#pragma unroll
                    for (int q_ = 0; q_ < 8; ++q_) fe[q_ >> 1][q_ & 1] = fsl[(e * 8 + q_) * 64 + lane];
                    const float pk = kn == 0 ? px : (kn == 1 ? py : pz);
                    const float poff = clampf(pk + ((e & 1) ? -bxe : bxe), -bound, bound);
                    accn = sdf_l1(lds, lane, g == kn ? poff : pc0, fe);
                }
                if (e == 0) oc = sdf_l2(lds, lane, acc);           // the centre needs all 16 outputs
                else {                                             // the six offset points only their sdf
                    const float s_e = sdf_l2_sdf(lds, acc, w2r0);
                    const int k = (e - 1) >> 1;
                    if (e & 1) spos = s_e;
                    else {
                        const float gk = 0.5f * (spos - s_e) / bxe;
                        if (k == 0) gr[0] = gk; else if (k == 1) gr[1] = gk; else gr[2] = gk;
                    }
                }
                acc = accn;
            }
            }
            }
            AC_TICK(4)
            // The wave's NEXT ticket is taken here, in the item's last tile behind its SDF evaluations, and consumed a few microseconds later, behind the
            // colour network and the compositing of the same tile -- so neither the ticket's round trip to the counter nor the fetch of the next item
            // stands between two items.  Not earlier: a wave that takes a ticket commits the hand-out, and at the head of the tile (~35 us before it can
            // start the item) that cost the launch 1.5 % -- near its end another wave is free first (profiles/worklist_experiments.txt).
            // A wave holds at most ONE ticket ahead, and only while it is working on an item it needs nobody for any more (whatever this item waited for
            // was consumed before its first tile).  So every wait in the launch still points from a ticket to a SMALLER one, and the holder of the
            // smallest unfinished ticket is always running it: no cycle, the same no-deadlock argument as with tickets taken at the boundary.  (A
            // ticket past the end of the list obliges to nothing.)
            if constexpr (LISTED) {
                if (c + 1 == c_hi && lane == 0) {
                    // (the counter's address enters through an opaque vector-register copy: on a wave-uniform address LLVM's atomic optimizer rewrites the add
                    //  into its one-lane-per-wave form, which waits for the returned value right behind the instruction -- the wait this is here to move)
                    __attribute__((address_space(1))) uint32_t *tk_p = (__attribute__((address_space(1))) uint32_t *)tk_counter;
                    asm volatile("" : "+v"(tk_p));
                    tk_v = __hip_atomic_fetch_add(tk_p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            const float gx = gr[0], gy = gr[1], gz = gr[2];        // every lane of a sample holds the same finite-difference gradient
            const FdNormal nrm = fd_normal(gx, gy, gz);
            const float gn = nrm.gn, nx = nrm.nx, ny = nrm.ny, nz = nrm.nz;
            float rgb[3] = { 0.0f, 0.0f, 0.0f };
            if (!skip && !a.opacity_only) {                      // (wave-uniform)
                if constexpr (FC) color_tile_fast(lds, lane, px, py, pz, nx, ny, nz, oc, rgb, nullptr, 16, SH ? zs0 + SLAB_SHB : nullptr);
                else color_tile(lds, lane, px, py, pz, nx, ny, nz, oc, rgb, nullptr, 16, SH ? zs0 + SLAB_SHB : nullptr);
            }
            AC_TICK(5)
            // NeuS alpha :219-248
            const float sdf0 = oc[0];
            float alpha = neus_alpha(lds, a, (dx * nx + dy * ny) + dz * nz, sdf0, delta, inv_s_core);
            if constexpr (MODE == MODE_FINAL) alpha = alpha * (a.mask[(size_t)ray * T + i] ? 1.0f : 0.0f);      // :246-249
            const float om = 1.0f - alpha + 1e-7f;
            // transmittance: exclusive tile scan with carry  :250
            const float loc = row_scan<true>(om);
            const float sh = dpp_shr<1>(1.0f, loc);
            float Tex;
            if (n == 0) Tex = (c == 0) ? 1.0f : cT;
            else Tex = (c == 0) ? sh : cT * sh;
            const float tot = lane_bcast(loc, 15);
            cT = (c == 0) ? tot : cT * tot;
            const float wgt = alpha * Tex;
            const float zn01 = clampf((zi - near) / span, 0.0f, 1.0f);
            const float pn = __builtin_sqrtf((px * px + py * py) + pz * pz);
            const float relax = (pn < 1.2f && !skip) ? 1.0f : 0.0f;
            const float eerr = relax * ((gn - 1.0f) * (gn - 1.0f));
            // reductions (lane 15 of row 0 holds the tile totals)
            // reductions: lane 15 holds the tile totals of the row scans and adds them to the ray's running sums (sequential over the tiles, like the oracle)
            {
                const float t1 = row_scan<false>(wgt), t2 = row_scan<false>(rgb[0] * wgt), t3 = row_scan<false>(rgb[1] * wgt), t4 = row_scan<false>(rgb[2] * wgt),
                            t5 = row_scan<false>(nx * wgt), t6 = row_scan<false>(ny * wgt), t7 = row_scan<false>(nz * wgt), t8 = row_scan<false>(wgt * zn01),
                            t9 = row_scan<false>(eerr), t10 = row_scan<false>(relax);
                if (lane == 15) {
#define AC_ACC(K, T_) accs[K] = (c == 0) ? T_ : accs[K] + T_;
                    AC_ACC(1, t1) AC_ACC(2, t2) AC_ACC(3, t3) AC_ACC(4, t4) AC_ACC(5, t5) AC_ACC(6, t6) AC_ACC(7, t7) AC_ACC(8, t8) AC_ACC(9, t9) AC_ACC(10, t10)
#undef AC_ACC
                }
            }
            AC_TICK(6)
            if constexpr (LISTED) {
                if (c + 1 == c_hi) { tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk_v); AC_FETCH_ITEM(tk, it_ray, it_meta) tk_ahead = true; }
            }
            if (g == 0) {
                const size_t si = (size_t)exr * T + i;
                if (EX && ex_on && a.out.z_vals) a.out.z_vals[si] = zi;
                if (EX && ex_on && a.out.weights) a.out.weights[si] = wgt;
                if (EX && ex_on && a.out.alpha) a.out.alpha[si] = alpha;
                if (EX && ex_on && a.out.sdf) a.out.sdf[si] = sdf0;
                if (EX && ex_on && a.out.color) { a.out.color[3 * si] = rgb[0]; a.out.color[3 * si + 1] = rgb[1]; a.out.color[3 * si + 2] = rgb[2]; }
                if (EX && ex_on && a.out.gradient) { a.out.gradient[3 * si] = gx; a.out.gradient[3 * si + 1] = gy; a.out.gradient[3 * si + 2] = gz; }
                if (EX && ex_on && a.out.pts) { a.out.pts[3 * si] = px; a.out.pts[3 * si + 1] = py; a.out.pts[3 * si + 2] = pz; }
            }
            if (EX && ex_on && a.out.sdf_out16) {                                 // lane (n, g) holds outputs 4g..4g+3
                int g_x = g;
                asm volatile("" : "+v"(g_x));                                   // (see feat7 above)
                *reinterpret_cast<f32x4 *>(a.out.sdf_out16 + ((size_t)exr * T + i) * 16 + 4 * g_x) = oc;
            }
        }
        AC_BND_MARK();
        if (!seg_last) {
            // hand the ray to its next item: z values (once), the running sums, then the flag -- in that order (the stores are complete in L2
            // before the flag leaves: s_waitcnt vmcnt(0); the reader's loads are issued after it has seen the flag)
            uint32_t *st = reinterpret_cast<uint32_t *>(a.seg_state + (size_t)ray * SEG_STATE);
            if (MODE != MODE_FINAL && seg_first)
                for (int i = lane; i < T; i += 64) __hip_atomic_store(st + i, __float_as_uint(zf[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wave_sync();
            if (lane < 11) {
                const float cv = lane == 0 ? cT : accs[lane];
                __hip_atomic_store(st + MAXT + lane, __float_as_uint(cv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if constexpr (SH) { if (seg_first) __hip_atomic_store(st + MAXT + 16 + lane, __float_as_uint(zs0[SLAB_SHB + lane]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every lane's state stores have left the wave ...
            wave_sync();
            // ... before the flag store is issued (relaxed, agent scope: see the taker's side for why no release / acquire pair is used)
            if (lane == 0) __hip_atomic_store(a.seg_flags + ray, (a.gen << 4) | (uint32_t)(seq + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wave_sync();
            if constexpr (LISTED) { if (!tk_ahead) { AC_TAKE_TICKET(tk) AC_FETCH_ITEM(tk, it_ray, it_meta) } }       // (an item without tiles: the builder makes none)
            continue;
        }
        wave_sync();
        if (lane == 0) {
            const float s_w = accs[1], s_r = accs[2], s_g = accs[3], s_b = accs[4], s_nx = accs[5], s_ny = accs[6], s_nz = accs[7], s_d = accs[8], s_en = accs[9], s_ed = accs[10];
            const float b0 = a.bg ? a.bg[3 * ray] : 1.0f, b1 = a.bg ? a.bg[3 * ray + 1] : 1.0f, b2 = a.bg ? a.bg[3 * ray + 2] : 1.0f;
            a.out.image[3 * ray] = s_r + (1.0f - s_w) * b0;
            a.out.image[3 * ray + 1] = s_g + (1.0f - s_w) * b1;
            a.out.image[3 * ray + 2] = s_b + (1.0f - s_w) * b2;
            a.out.normal_map[3 * ray] = s_nx; a.out.normal_map[3 * ray + 1] = s_ny; a.out.normal_map[3 * ray + 2] = s_nz;
            a.out.weights_sum[ray] = s_w;
            a.out.depth[ray] = s_d;
            a.out.eik[2 * ray] = s_en; a.out.eik[2 * ray + 1] = s_ed;
        }
        wave_sync();
#ifdef AC_PROFILE               // per-ray wall time (100 MHz ticks) behind the per-wave records: [n_rays * 10 + ray]
        if (a.prof && lane == 0) a.prof[(size_t)a.n_rays * 10 + ray] = __builtin_amdgcn_s_memrealtime() - ray_r0_;
#endif
        if constexpr (LISTED) { if (!tk_ahead) { AC_TAKE_TICKET(tk) AC_FETCH_ITEM(tk, it_ray, it_meta) } }
    }
#undef AC_TAKE_TICKET
#undef AC_FETCH_ITEM
    // ---- epilogue: the last workgroup to finish reduces gradient_error and re-arms the slot's work counters (RenderArgs::done_counter) --------------------
    // (the arguments used here are read from the kernel-argument segment again, behind an opaque barrier: kept in scalar registers from the start of the kernel
    //  they cost the work loops two spilled vector registers)
    const __attribute__((address_space(4))) RenderArgs *ka = (const __attribute__((address_space(4))) RenderArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    uint32_t *const k_done = ka->done_counter;
    if (k_done) {
        __syncthreads();                                         // every wave of this workgroup has left the work loops: the weights in LDS are free
        uint32_t *ldsu = reinterpret_cast<uint32_t *>(lds);
        if (threadIdx.x == 0) {
            __threadfence();                                     // this workgroup's per-ray results are visible device-wide before its ticket is
            ldsu[0] = atomicAdd(k_done, 1u) == gridDim.x - 1u ? 1u : 0u;
        }
        __syncthreads();
        const bool last = ldsu[0] != 0u;
        __syncthreads();
        if (last) {
            __threadfence();                                     // ... and every other workgroup's are visible here
            float *const k_red = ka->eik_red;
            const int k_pair = ka->pair_n, k_n = ka->n_rays;
            const float *const k_eik = ka->out.eik;
            uint32_t *const k_cnt = ka->ray_counter;
            if (k_red) {
                // gradient_error (:270-272) of the batch -- of each copy of a pair launch -- in eikonal_reduce_kernel's order (oracle: orc_eikonal_reduce):
                // 1024 strided sequential partial sums (two per thread here), then a halving tree
                const int nred = k_pair ? 2 : 1, nper = k_pair ? k_pair : k_n;
                float *pn = lds, *pd = lds + 1024;
                for (int q = 0; q < nred; ++q) {
                    const float *e = k_eik + (size_t)q * nper * 2;
                    for (int t = (int)threadIdx.x; t < 1024; t += BLOCK) {
                        float sa = 0.0f, sb = 0.0f;
                        for (int r = t; r < nper; r += 1024) { sa += e[2 * r]; sb += e[2 * r + 1]; }
                        pn[t] = sa; pd[t] = sb;
                    }
                    __syncthreads();
                    for (int st = 512; st > 0; st >>= 1) {
                        for (int t = (int)threadIdx.x; t < st; t += BLOCK) { pn[t] += pn[t + st]; pd[t] += pd[t + st]; }
                        __syncthreads();
                    }
                    if (threadIdx.x == 0) { k_red[2 * q] = pn[0] / (pd[0] + 1e-5f); k_red[2 * q + 1] = pd[0] + 1e-5f; }
                    __syncthreads();
                }
            }
            if (threadIdx.x < 64) k_cnt[threadIdx.x] = 0u;       // the slot's next launch starts from zero again
            if (threadIdx.x == 64) *k_done = 0u;
        }
    }
#ifdef AC_PROFILE
    if (a.prof && lane == 0) { const int w_ = blockIdx.x * WAVES_PER_BLOCK + wave; for (int i = 0; i < 8; ++i) a.prof[w_ * 10 + i] = prof_acc[i];
        a.prof[(size_t)a.n_rays * 11 + 2 * w_] = prof_bnd[0]; a.prof[(size_t)a.n_rays * 11 + 2 * w_ + 1] = prof_bnd[1];
        a.prof[w_ * 10 + 8] = __builtin_amdgcn_s_memtime() - prof_t0; a.prof[w_ * 10 + 9] = __builtin_amdgcn_s_memrealtime() - prof_r0; }   // shader clock vs 100 MHz
#endif
}
