/*
 * include/avatarcraft_hip.h -- C ABI of libavatarcraft_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary of the AvatarCraft hot path: every entry point replaces one
 * function that the reference binds through pybind11 from its JIT-built CUDA extensions, with
 * the same argument meaning and order, plus (a) an explicit stream and (b) an int status
 * instead of a C++ exception (0 = ok; non-zero = bad arguments / launch failure, message in
 * ac_last_error(); the Python wrappers raise RuntimeError exactly where the reference's
 * TORCH_CHECK / std::runtime_error would).
 *
 * Conventions (same as the reference):
 *   - the CALLER allocates every buffer; the library never allocates user-visible memory and
 *     keeps no pointer after the call returns (small internal scratch is per-call);
 *   - all pointers are DEVICE pointers unless the parameter is documented "host";
 *   - all float data is fp32, all index data int32/uint32;
 *   - kernels are enqueued on `stream` (a hipStream_t; NULL = the null stream) and the call
 *     returns without synchronising.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   encoder/hashencoder/src/hashencoder.h:13-14   hash_encode_forward / hash_encode_backward
 *   encoder/shencoder/src/shencoder.h:11,14       sh_encode_forward / sh_encode_backward
 *   raymarching/src/raymarching.h:8-17            march_rays_train, composite_rays_train_forward/
 *                                                 _backward, march_rays, composite_rays, compact_rays
 *   models/instant_nsr.py:133-299,358-408         NeRFRenderer.run / render (the fused path:
 *                                                 ac_render_rays; the reference has no native
 *                                                 entry for it -- `run_cuda` is missing)
 */
#ifndef AVATARCRAFT_HIP_H
#define AVATARCRAFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ac_stream_t; /* hipStream_t */

#define AC_OK 0
#define AC_ERR_BAD_ARG 1
#define AC_ERR_LAUNCH 2
#define AC_MAX_LEVELS 32

/* library identification / diagnostics */
int ac_version(void);                /* ABI version, currently 10 (round 6, second half: ac_sdf_stencil_backward_inputs, ac_hash_stencil_input_backward -- the position gradient
                                      * of the stencil query, for the curvature term; 9, round 6: ac_warp_mesh.seed_faces / seed_stride -- the struct grew --, ac_set_occupancy_barrier_ms, ac_debug_hold_cus; the phased occupancy launches are cooperative launches sized by the runtime's
                                      * occupancy figure; 7, round 5, second half: ac_render_rays_occupancy_phased, ac_render_rays_occupancy_train, ac_march_rays_train_scratch -- the
                                      * marcher's scratch grew --; 6, round 5: ac_render_rays_occupancy's max_steps, ac_field_sdf_grid, ac_marching_cubes*,
                                      * ac_density_grid_update, the SH colour input of ac_field; round 4 = 5: ac_render_opts.opacity_only -- the struct grew from 64 to 72 bytes --,
                                      * ac_field_samples, ac_render_rays_occupancy, the measurement / liveness accessors, the *_typed encoder entries) */
const char *ac_last_error(void);     /* message of the last failing call on this thread */
/* test utility: `blocks` workgroups of 1024 threads + lds_bytes of LDS each spin for `millis` ms of wall clock on `stream` -- a FOREIGN workload that holds
 * compute units (no memory traffic), for the liveness tests of the kernels that wait for each other (tests/test_gpu_run_cuda.py, tests/test_gpu_render.py) */
int ac_debug_hold_cus(uint32_t blocks, uint32_t lds_bytes, uint32_t millis, ac_stream_t stream);
/* test utility: the division-free unit coordinate (q = a * RN(1 / d); r = fma(-q, d, a); u = fma(r, RN(1 / d), q)) against the IEEE quotient a / d
 * on the device, for EVERY fp32 dividend whose bit pattern lies in [lo_bits, hi_bits]: *mismatches (device, zeroed by the caller) += the number that differ in a
 * bit (two NaNs count as equal).  tests/test_gpu_ops.py sweeps the renderer's whole dividend domain for the divisors the library accepts. */
int ac_debug_unit_div_check(uint32_t lo_bits, uint32_t hi_bits, float d, unsigned long long *mismatches, ac_stream_t stream);

/* ---- hash-grid encoder -------------------------------------------------------------------
 * replaces hash_encode_forward (encoder/hashencoder/src/hashencoder.cu:413-436)
 *   inputs  [B,D] in [0,1]; embeddings [sum_l T_l, C]; offsets [L+1] int32 (device);
 *   outputs [L,B,C] (level major); dy_dx [B, L*D*C] (only written if calc_grad_inputs).
 *   D in {2,3}, C in {1,2,4,8}, L <= AC_MAX_LEVELS, else AC_ERR_BAD_ARG
 *   ("GridEncoding: C must be 1, 2, 4, or 8." in the reference).
 *   S = log2(per_level_scale) as float, H = base resolution.
 *   offsets_host: the same L+1 offsets in HOST memory (the reference reads them on the device
 *   only; the MI355X kernels take the level table as launch constants). */
int ac_hash_encode_forward(const float *inputs, const float *embeddings, const int32_t *offsets,
                           const int32_t *offsets_host, float *outputs, uint32_t B, uint32_t D, uint32_t C,
                           uint32_t L, float S, uint32_t H, int calc_grad_inputs, float *dy_dx,
                           ac_stream_t stream);

/* replaces hash_encode_backward (hashencoder.cu:438-468): grad [L,B,C]; grad_embeddings is
 * accumulated into (caller zero-fills, hashgrid.py:61); grad_inputs [B,D] written iff
 * calc_grad_inputs. */
int ac_hash_encode_backward(const float *grad, const float *inputs, const float *embeddings,
                            const int32_t *offsets, const int32_t *offsets_host, float *grad_embeddings,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                            int calc_grad_inputs, const float *dy_dx, float *grad_inputs, ac_stream_t stream);

/* debugging / parity: table entry index (before *C) of every trilinear corner, [L,B,2^D] uint32,
 * 0xffffffff for out-of-range inputs */
int ac_hash_corner_indices(const float *inputs, const int32_t *offsets_host, uint32_t *corner_idx, uint32_t B,
                           uint32_t D, uint32_t L, float S, uint32_t H, ac_stream_t stream);

/* host helper: the per-level (scale, resolution) table every kernel uses
 * (hashencoder.cu:122-123), computed once on the host */
void ac_hash_level_table(uint32_t L, float S, uint32_t H, float *scale_host, uint32_t *res_host);

/* ---- spherical-harmonics encoder -----------------------------------------------------------
 * replaces sh_encode_forward / sh_encode_backward (encoder/shencoder/src/shencoder.cu:403-441)
 *   inputs [B,3]; outputs [B, C*C] (C = degree, 1..8); dy_dx [B, 3*C*C]. */
int ac_sh_encode_forward(const float *inputs, float *outputs, uint32_t B, uint32_t D, uint32_t C,
                         int calc_grad_inputs, float *dy_dx, ac_stream_t stream);
int ac_sh_encode_backward(const float *grad, const float *inputs, uint32_t B, uint32_t D, uint32_t C,
                          const float *dy_dx, float *grad_inputs, ac_stream_t stream);

/* ---- half / double tensors of the two encoders ------------------------------------------------
 * The reference dispatches both extensions over the dtype of their tensors (AT_DISPATCH_FLOATING_TYPES_AND_HALF: hashencoder.cu:352,391,
 * shencoder.cu:337,380; `CHECK_IS_FLOATING` accepts Float, Half, Double).  Same arguments as the fp32 entry points above with `dtype` in front and
 * untyped pointers: AC_DTYPE_F32 is the fp32 entry points' call (they pass it); AC_DTYPE_F16 / AC_DTYPE_F64 are every tensor of the call (inputs, embeddings, outputs, dy_dx, grad,
 * grad_embeddings, grad_inputs) in that type.  Arithmetic: cell positions and interpolation weights in fp32 whatever the dtype (`float pos[D]`,
 * hashencoder.cu:125-133); half tensors are widened on load, accumulated in fp32 and rounded once on store (the table gradient: packed half2 atomics,
 * hashencoder.cu:293-299); double tensors accumulate in double.  Any other code: AC_ERR_BAD_ARG ("... must be a floating tensor"). */
#define AC_DTYPE_F32 0
#define AC_DTYPE_F16 1
#define AC_DTYPE_F64 2
int ac_hash_encode_forward_typed(int dtype, const void *inputs, const void *embeddings, const int32_t *offsets, const int32_t *offsets_host,
                                 void *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                                 void *dy_dx, ac_stream_t stream);
int ac_hash_encode_backward_typed(int dtype, const void *grad, const void *inputs, const void *embeddings, const int32_t *offsets,
                                  const int32_t *offsets_host, void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                  uint32_t H, int calc_grad_inputs, const void *dy_dx, void *grad_inputs, ac_stream_t stream);
int ac_sh_encode_forward_typed(int dtype, const void *inputs, void *outputs, uint32_t B, uint32_t D, uint32_t C, int calc_grad_inputs,
                               void *dy_dx, ac_stream_t stream);
int ac_sh_encode_backward_typed(int dtype, const void *grad, const void *inputs, uint32_t B, uint32_t D, uint32_t C, const void *dy_dx,
                                void *grad_inputs, ac_stream_t stream);

/* ---- raymarching operators (raymarching/src/raymarching.cu) ---------------------------------
 * Same arguments as the reference wrappers.  Slot reservation is deterministic: packed samples
 * are laid out in ray order (an exclusive prefix sum replaces the reference's atomicAdd), so
 * rays[N,3] = (ray id, offset, n_steps) is reproducible.  counter[2] (device) is incremented by
 * (total steps, N) as in the reference.  scratch: device int32 buffer of ac_march_rays_train_scratch(N)
 * elements (ABI 7: 36 N + 2 -- counts, offsets and, new, the positions of every ray's samples as a bit mask over its
 * step recurrence, which the counting pass records and the writing pass replays instead of walking the grid a second
 * time; before: 2N+2). */
size_t ac_march_rays_train_scratch(uint32_t N);
int ac_march_rays_train(const float *rays_o, const float *rays_d, const float *grid, float mean_density,
                        int iter_density, float bound, uint32_t N, uint32_t H, uint32_t M, float *xyzs,
                        float *dirs, float *deltas, int32_t *rays, int32_t *counter, uint32_t perturb,
                        int32_t *scratch, ac_stream_t stream);
int ac_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                    const int32_t *rays, float bound, uint32_t M, uint32_t N,
                                    float *weights_sum, float *image, ac_stream_t stream);
int ac_composite_rays_train_backward(const float *grad_weights_sum, const float *grad, const float *sigmas,
                                     const float *rgbs, const float *deltas, const int32_t *rays,
                                     const float *weights_sum, const float *image, float bound, uint32_t M,
                                     uint32_t N, float *grad_sigmas, float *grad_rgbs, ac_stream_t stream);
int ac_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t,
                  const float *rays_o, const float *rays_d, float bound, uint32_t H, const float *grid,
                  float mean_density, const float *near, const float *far, float *xyzs, float *dirs,
                  float *deltas, uint32_t perturb, ac_stream_t stream);
int ac_composite_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, float *rays_t,
                      const float *sigmas, const float *rgbs, const float *normals, const float *deltas,
                      float *weights_sum, float *depth, float *image, float *normal_map, ac_stream_t stream);
/* order-preserving compaction; scratch: >= n_alive+2 int32 */
int ac_compact_rays(uint32_t n_alive, int32_t *rays_alive, const int32_t *rays_alive_old, float *rays_t,
                    const float *rays_t_old, int32_t *alive_counter, int32_t *scratch, ac_stream_t stream);

/* ---- fused Instant-NSR renderer --------------------------------------------------------------
 * One launch = NeRFRenderer.run for a batch of rays (models/instant_nsr.py:133-299,
 * render_can=True): cube near/far, uniform(+jitter) z, 4x NeuS up-sampling (up_sample,
 * sample_pdf, cat_z_vals), hash-grid SDF MLP, finite-difference normals, colour MLP, NeuS
 * alpha, transmittance scan and compositing, eikonal partials.  Default model only:
 * L=16, C=2, D=3 hash grid; SDF MLP 35-64-16; colour MLP 21-64-64-3. */
typedef struct ac_field {
    const float *table;       /* embeddings [offsets[16], 2]                           (device) */
    int32_t offsets[17];      /* level offsets, entries                                (host values) */
    float S;                  /* log2(per_level_scale)  (hashgrid.py:27)                         */
    uint32_t H;               /* base resolution                                                  */
    const float *W1, *b1;     /* effective sdf_net.0 weight [64,35] row-major, bias [64] (device) */
    const float *W2, *b2;     /* effective sdf_net.1 weight [16,64], bias [16]                    */
    const float *Wc1;         /* effective color_net.0 weight [64,21]                             */
    const float *Wc2;         /* effective color_net.1 weight [64,64]                             */
    const float *Wc3;         /* effective color_net.2 weight [3,64]                              */
    const void *prepared;     /* optional: AC_FIELD_PREPARED_BYTES of device memory filled by ac_field_prepare() for THESE
                                 parameters (the weights in the order the renderer keeps them in LDS: its workgroups then
                                 copy 52 KB linearly instead of re-deriving the layout from the row-major matrices, 512 times
                                 per launch).  NULL = derive it in every workgroup.  Must be re-prepared when a parameter changes. */
    const float *Wc1_sh;      /* optional (ABI 6): NeRFNetwork(use_viewdirs=True) -- the colour network's first layer reads
                                 h = cat[x, sh(d), n, geo_feat] (models/instant_nsr.py:565-569, 644-653; sh = degree-4 real spherical harmonics of the RAW
                                 ray direction, encoder/shencoder: 16 values).  Wc1_sh = the 16 columns of the effective color_net.0 weight that multiply
                                 sh(d), [64,16] row-major (columns 3..18 of the [64,37] matrix); Wc1 keeps the other 21 (x, n, geo_feat).  The view
                                 direction is constant along a ray: the renderer folds Wc1_sh sh(d) into a per-ray bias of layer 1 (fp32 fma chain over
                                 the 16 terms in order, then the 21 inputs as without view directions) -- no per-sample cost.  NULL = no view directions. */
} ac_field;
#define AC_FIELD_PREPARED_BYTES 98304
/* fills `prepared` (device, AC_FIELD_PREPARED_BYTES) from the other members of `field`; enqueue on `stream` before the launches that use it */
int ac_field_prepare(const ac_field *field, void *prepared, ac_stream_t stream);

typedef struct ac_render_opts {
    int32_t n_rays;
    int32_t num_steps;        /* coarse samples per ray: 16,32,48 or 64                           */
    int32_t upsample_steps;   /* multiple of 16, num_steps + upsample_steps <= 128                */
    float bound;
    float inv_s;              /* forward_variance() = exp(10*variance).clip(1e-6,1e6)             */
    float cos_anneal_ratio;
    float fd_eps;             /* 0.005 * (1 - normal_epsilon_ratio)                               */
    int32_t perturb;          /* 1: z += (noise-0.5)*sample_dist (training && perturb_overwrite)  */
    const float *inv_s_dev;   /* optional: inv_s as ONE float in device memory (then `inv_s` above is ignored): the trainable
                                 variance stays on the device, no host read-back per render                                */
    const float *near_m, *far_m; /* optional [N]: per-ray sampling range that replaces the cube's where finite (+-inf = keep the cube's):
                                 the mesh-guided range of run(render_can=True, verts=..., use_mesh_guide=True), instant_nsr.py:147-153,
                                 as produced by ac_mesh_near_far.  NULL = cube only.  (ac_render_rays_warped computes its own.)       */
    int32_t precision;        /* 0 = exact: every product an fp32 fma in a stated order (bit-identical to the CPU oracle);
                                 1 = fast: layer 1 of the six finite-difference evaluations of a sample as
                                     l1(x +- eps e_k) = l1(x) [exact fp32] + W1 (h(x +- eps e_k) - h(x)) + W1[:,k] (+-eps)
                                 with the middle product on the bf16 matrix pipe, both factors split into hi + lo bf16 (3 products, fp32
                                 accumulate): the correction term is ~1e-2 of l1, its 2^-16 relative error is below fp32 round-off of l1
                                 itself (normals within 6e-5 of the exact mode), and the colour network (21-64-64-3) in split bf16 as well
                                 (hi + lo, 3 products per layer; colours move by ~1e-6).  Sample positions (everything that feeds
                                 searchsorted / the sort) and the centre SDF evaluation are unaffected: z_vals, indices and sdf stay
                                 bit-identical.  The product's default is 0. */
    int32_t skip_masked;      /* posed-space rendering (ac_render_rays_warped) only: 1 = tiles of 16 samples that the warp masks out entirely
                                 (alpha * 0, instant_nsr.py:246-249) are not evaluated.  image, weights_sum, depth, normal_map and the per-sample
                                 weights / alpha are unchanged bit for bit (their contribution is exactly zero; the transmittance factor
                                 1 + 1e-7 of a masked sample is kept); the per-sample sdf / color / gradient of skipped samples are 0 and
                                 gradient_error covers the evaluated samples only.  0 = evaluate everything like the reference (default). */
    int32_t opacity_only;     /* 1 = the caller wants weights_sum / depth / normal_map / gradient_error only (the frozen avatar of the opacity loss,
                                 stylize.py:176-190, is rendered for its weight_sum alone): the colour network is not evaluated and `image` is the
                                 background blend of a black body.  Every other output is unchanged bit for bit (alpha does not depend on the
                                 colour).  0 = default. */
} ac_render_opts;

typedef struct ac_render_out {
    float *image;             /* [N,3]  rgb incl. background blend                                */
    float *weights_sum;       /* [N]                                                              */
    float *depth;             /* [N]                                                              */
    float *normal_map;        /* [N,3]                                                            */
    float *eik;               /* [N,2]  per-ray (sum relax*(|g|-1)^2, sum relax)                  */
    /* optional (NULL = not written); T = num_steps + upsample_steps */
    float *z_vals;            /* [N,T]                                                            */
    float *weights;           /* [N,T]                                                            */
    float *alpha;             /* [N,T]                                                            */
    float *color;             /* [N,T,3]                                                          */
    float *sdf;               /* [N,T]                                                            */
    float *gradient;          /* [N,T,3]                                                          */
    int32_t *ss_inds;         /* [N, upsample_steps/16, 16]  searchsorted indices of sample_pdf   */
    int32_t *sort_index;      /* [N, upsample_steps/16, 128] sort permutation of cat_z_vals, -1 pad */
    float *sdf_out16;         /* [N,T,16] forward_sdf at the mid points: sdf + the 15 geometry features   */
    float *pts;               /* [N,T,3]  the mid points themselves (clamped to the bound)                */
    float *feat7;             /* [N*T/16,14,64,4] the hash features of the 7 points of every sample's finite-difference stencil, in the kernel's own
                               * lane order: tile of 16 consecutive samples, then float k = 8 e + 2 j + c (evaluation e, level 4 j + g, channel c) of
                               * lane n + 16 g (sample n of the tile, level group g) at [k / 4][lane][k % 4] -- opaque to callers, produced by the
                               * forward and consumed by ac_render_core_backward, which would otherwise gather the table again (0.9 KB per
                               * sample; training renders only)                                                                                */
    float *eik_reduced;       /* optional [2] ([2][2] for ac_render_rays_pair: one pair per copy): (gradient_error, its denominator) =
                               * (sum relax * err / (sum relax + 1e-5), sum relax + 1e-5) over the batch (instant_nsr.py:270-272), reduced by the
                               * render launch itself in ac_eikonal_reduce2's fixed order (bit-identical to calling it on `eik` afterwards);
                               * not written for an empty batch (ABI version 4)                                                               */
} ac_render_out;

/* rays_o, rays_d [N,3]; bg [N,3] or NULL (= white, bg_color None -> 1); noise [N,num_steps] U[0,1)
 * (read iff opts->perturb); lin_z [num_steps] = torch.linspace(0,1,num_steps) and lin_u [16] =
 * torch.linspace(0.5/16, 1-0.5/16, 16) as DEVICE arrays made by the host (instant_nsr.py:155,:34). */
int ac_render_rays(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                   const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                   const ac_render_out *out, ac_stream_t stream);

/* The same N = opts->n_rays rays rendered TWICE in one launch, with two draws of the jitter noise and two backgrounds: the two renders of
 * net_style in one stylisation step -- stylize.py:98-116 (render_val, no_grad) and :143-152 (the differentiable render of the same rays) are two
 * calls of NeRFRenderer.run (instant_nsr.py:133-299) in the reference.  The two copies of a ray are neighbours in the hand-out order and meet in
 * their XCD's L2 (-11 % against two launches on the stride-4 training view); every value is bit-identical to two ac_render_rays calls.
 * rays_o, rays_d [N,3]; bg2 [2,N,3] or NULL; noise2 [2,N,num_steps]; out: image, weights_sum, depth, normal_map, eik hold 2N rows (rows [0,N) = the
 * copy rendered with noise2[0] / bg2[0], rows [N,2N) = the other); the optional per-sample arrays are written for the SECOND copy only, N rows. */
int ac_render_rays_pair(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                        const float *bg2, const float *noise2, const float *lin_z, const float *lin_u,
                        const ac_render_out *out, ac_stream_t stream);

/* ac_render_rays for any sample count the reference accepts: num_steps >= 2 (any value, not only multiples of 16), upsample_steps >= 0 and a
 * multiple of 16, num_steps + upsample_steps <= 512 (anything else: AC_ERR_BAD_ARG naming the rule).  Canonical space (posed: ac_render_rays_long_warped); same arguments and
 * outputs as ac_render_rays (lin_z [num_steps]), except: sort_index is [N, upsample_steps/16, T] (T = num_steps + upsample_steps, -1 pad);
 * feat7 (optional, the layout documented at ac_render_out) needs T a multiple of 16 -- any other count with feat7 set is AC_ERR_BAD_ARG naming the
 * rule, and ac_render_core_backward gathers again there --; opts->skip_masked must be 0 (a posed-space option); opts->opacity_only is taken as by
 * ac_render_rays (no colour network, image = the background over a black body, every other output unchanged bit for bit).  Where both accept the
 * counts, every output (feat7 included) is bit-identical to ac_render_rays'.  Needs no scratch; gradient_error (eik_reduced) is formed by
 * ac_eikonal_reduce2 on the same stream. */
int ac_render_rays_long(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                        const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                        const ac_render_out *out, ac_stream_t stream);
/* ac_render_rays_pair for the sample counts of ac_render_rays_long, same contract: the N = opts->n_rays rays rendered twice in ONE launch; bg2 [2,N,3]
 * or NULL, noise2 [2,N,num_steps]; image, weights_sum, depth, normal_map, eik hold 2N rows (rows [0,N) = the copy of noise2[0] / bg2[0]); the optional
 * per-sample arrays and feat7 (16 | T, as above) are written for the SECOND copy only, N rows; eik_reduced [2][2], one pair per copy.  The 2N work items
 * keep the long renderer's static hand-out (chunks of 512 items, chunk c to XCD c % 8) with the two copies of a ray as consecutive items of one chunk,
 * so they meet in one XCD's L2.  Every value is bit-identical to two ac_render_rays_long calls.  No scratch. */
int ac_render_rays_long_pair(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                             const float *bg2, const float *noise2, const float *lin_z, const float *lin_u,
                             const ac_render_out *out, ac_stream_t stream);
/* the sampling stage of ac_render_rays_long alone -> z_vals [N, num_steps + upsample_steps]: the long counterpart of ac_sample_rays */
int ac_sample_rays_long(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d, const float *noise,
                        const float *lin_z, const float *lin_u, float *z_vals, ac_stream_t stream);

/* gradient_error = sum(relax*err) / (sum(relax) + 1e-5) over the per-ray partials, fixed order
 * (instant_nsr.py:270-272); result: 1 float (device) */
int ac_eikonal_reduce(const float *eik, int32_t n_rays, float *result, ac_stream_t stream);
/* same, result: 2 floats (device) = { gradient_error, sum(relax) + 1e-5 } -- the denominator is what the backward of the term needs */
int ac_eikonal_reduce2(const float *eik, int32_t n_rays, float *result2, ac_stream_t stream);

/* SDF-only / field queries used by density(), extract_geometry() and the unit tests:
 * out16 [B,16] = forward_sdf(x) (instant_nsr.py:627-642), x [B,3] in [-bound,bound] */
int ac_field_sdf(const ac_field *field, const float *x, uint32_t B, float bound, float *out16, ac_stream_t stream);
/* rgb [B,3] = forward_color(x, -, n, feat) (instant_nsr.py:644-663); sdfout [B,16] as returned above */
int ac_field_color(const ac_field *field, const float *x, const float *n, const float *sdfout, uint32_t B,
                   float *rgb, ac_stream_t stream);

/* ---- SMPL-guided animation path (render_warp.py, NeRFRenderer.run with render_can=False) ---------------------
 * replaces geometry_guided_near_far_torch (utils/ray_utils.py:277-294): per ray, over V vertex spheres of radius
 * geo_threshold; near/far [N], +inf / -inf where the ray misses every sphere (the caller substitutes the cube bounds,
 * models/instant_nsr.py:152-153). */
int ac_mesh_near_far(const float *rays_o, const float *rays_d, const float *verts, uint32_t N, uint32_t V, float geo_threshold,
                     float *near, float *far, ac_stream_t stream);

/* replaces warp_samples_to_canonical (utils/ray_utils.py:62-90; CPU libigl + numpy in the reference): for every sample
 * pts[P,3] (fp32): exact closest point on the triangle mesh (verts[V,3] fp32, faces[F,3] int32), mask = dist^2 < threshold
 * (the reference compares the SQUARED distance with DEFAULT_GEO_THRESH), barycentric blend of the per-vertex transforms
 * T[V',4,4] (fp64, V' >= max vertex index + 1), 4x4 inverse and application, all in fp64.
 * Outputs: can_pts [P,3] fp64 and/or can_pts_f32 [P,3] (at least one non-NULL); optional closest [P,3] fp64, dist2 [P] fp64,
 * face_id [P]; mask [P] uint8. */
int ac_warp_samples(const float *pts, const float *verts, const int32_t *faces, const double *T, uint32_t P, uint32_t V, uint32_t F,
                    double threshold, double *can_pts, float *can_pts_f32, double *closest, double *dist2, int32_t *face_id,
                    uint8_t *mask, ac_stream_t stream);

/* Accelerated form of ac_warp_samples: identical outputs bit for bit (same fp64 point-triangle arithmetic, ties -> lowest face id).
 * ac_warp_accel_build (once per frame / mesh) sorts the faces along a space-filling curve and cuts them into tiles of 32 with
 * bounding boxes; ac_warp_samples_accel then tests only the tiles whose box can contain the closest face (exact culling).
 * F <= 16384 (SMPL: 13776); ac_warp_accel_bytes returns 0 for meshes outside that range. */
size_t ac_warp_accel_bytes(uint32_t F);
/* Measurement accessors (bench.py's posed-frame roofline; no effect on results):
 * ac_warp_accel_work: the work the searches have done on this structure since its last build -- out[0] exact fp64 point-triangle tests,
 *   out[1] bounding-disc tests, out[2] sub-box tests, out[3] tile-box tests (counted per wave, one atomic each; waits for `stream`).
 * ac_debug_warped_phases(1): ac_render_rays_warped records HIP events at its phase boundaries; ac_debug_warped_phase_ms returns the five intervals of
 *   the last call in ms: near / far + coarse points + ray cull | first search | up-sampling pass | second search | final pass. */
int ac_warp_accel_work(const void *accel, unsigned long long out[4], ac_stream_t stream);
void ac_debug_warped_phases(int enable);
int ac_debug_warped_phase_ms(float out[5]);
int ac_warp_accel_build(const float *verts, const int32_t *faces, uint32_t V, uint32_t F, void *accel, size_t accel_bytes,
                        ac_stream_t stream);
int ac_warp_samples_accel(const float *pts, const float *verts, const int32_t *faces, const double *T, uint32_t P, uint32_t V, uint32_t F,
                          double threshold, const void *accel, double *can_pts, float *can_pts_f32, double *closest, double *dist2,
                          int32_t *face_id, uint8_t *mask, ac_stream_t stream);

/* ac_hash_encode_backward with caller scratch: for D = 3, C = 2 and levels of at most 2^19 entries (the default model) the table
 * gradient goes through the binned two-pass scatter (see ac_hash_stencil_backward) instead of one float atomic per corner and
 * channel; any other configuration, a NULL / too small scratch or calc_grad_inputs falls back to ac_hash_encode_backward.
 * ac_hash_encode_backward_scratch returns the bytes needed (0 = not coverable). */
size_t ac_hash_encode_backward_scratch(const int32_t *offsets_host, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t B);
int ac_hash_encode_backward_ws(const float *grad, const float *inputs, const float *embeddings, const int32_t *offsets,
                               const int32_t *offsets_host, float *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                               uint32_t H, int calc_grad_inputs, const float *dy_dx, float *grad_inputs, void *scratch, size_t scratch_bytes,
                               ac_stream_t stream);

/* ---- hash-grid encoder on the 7-point finite-difference stencil (training path)
 * One SDF query of the render core is 7 HashEncoder calls in the reference: forward_sdf at x (models/instant_nsr.py:627-642) and at
 * clamp(x +- eps e_k) (finite_difference_normals_approximator, :687-704), each through encoder/hashencoder/hashgrid.py:11-73.
 * These two entry points evaluate / back-propagate the seven points of every sample in one launch; the backward combines the
 * table gradients of the seven points in registers before its atomics (same sums as 7 x ac_hash_encode_backward).
 * x [B,3] world space, clamped to [-bound, bound]; point order x, +x, -x, +y, -y, +z, -z; outputs / grad [7, L, B, C], C = 2, D = 3;
 * grad_embeddings is accumulated into (zero it first).
 */
int ac_hash_stencil_forward(const float *x, const float *embeddings, const int32_t *offsets_host, float *outputs, uint32_t B,
                            uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, ac_stream_t stream);
/* scratch (optional, NULL = none = every level through hardware float atomics):
 * ac_hash_stencil_backward_scratch(offsets_host, L, S, H, n_copies, B) bytes hold (a) n_copies >= 2 private copies of the small dense
 * levels, which otherwise take bursts of same-address atomics from neighbouring rays, and (b) for B > 0 the per-bucket record queues of
 * the hashed levels (binned two-pass scatter: records are queued by destination bucket with one global atomic per flush and bucket,
 * then every bucket is summed in LDS by one workgroup and added to the table without atomics); ~4 GB for B = 524288. */
size_t ac_hash_stencil_backward_scratch(const int32_t *offsets_host, uint32_t L, float S, uint32_t H, uint32_t n_copies, uint32_t B);
int ac_hash_stencil_backward(const float *grad, const float *x, const int32_t *offsets_host, float *grad_embeddings, uint32_t B,
                             uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, void *scratch, size_t scratch_bytes,
                             ac_stream_t stream);

/* The stencil's gradient w.r.t. the sample POSITIONS through the encodings: what the reference obtains from dy_dx (kernel_grid's derivative branch,
 * hashencoder.cu:177-220, + kernel_input_backward, :311-337) when the encoder's input requires grad -- the curvature term's perturbed points
 * (models/instant_nsr.py:276-288).  gfeat [7, L, B, C] as ac_sdf_stencil_backward writes it; the corners are gathered again, nothing is stored.
 * gx_part [(L + 3) / 4][B][3]: one partial per group of four levels (the caller sums them: a fixed order); an offset coordinate passes through its
 * clamp to [-bound, bound] with torch.clamp's rule (inclusive), an out-of-range point contributes nothing (hashencoder.cu:95-119). */
int ac_hash_stencil_input_backward(const float *gfeat, const float *x, const float *embeddings, const int32_t *offsets_host, float *gx_part,
                                   uint32_t B, uint32_t C, uint32_t L, float S, uint32_t H, float eps, float bound, ac_stream_t stream);

/* The sampling stage of run() alone: coarse z (+ jitter), coarse SDF, 4x NeuS up-sampling -> z_vals [N, num_steps + upsample_steps]
 * (models/instant_nsr.py:155-184; the reference runs it under no_grad before the differentiable render core).  Same z as
 * ac_render_rays bit for bit, at a fraction of its cost. */
int ac_sample_rays(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d, const float *noise,
                   const float *lin_z, const float *lin_u, float *z_vals, ac_stream_t stream);

/* ---- fused SDF query of the differentiable render core (training path): forward_sdf(x) (models/instant_nsr.py:627-642) and
 * finite_difference_normals_approximator(x) (:687-704), i.e. 7 hash-encoder + MLP evaluations per sample, in one kernel each way.
 * forward : x [B,3] (clamped to the bound) -> out16 [B,16] = forward_sdf(x), grad [B,3] = the finite-difference gradient (eps > 0);
 *           bit-identical to the values ac_render_rays computes internally.
 * backward: (x, g_out16 [B,16], g_grad [B,3]) -> gfeat [7,16,B,2]: the gradient w.r.t. the hash features of the 7 stencil points in
 *           the layout ac_hash_stencil_backward consumes (the table scatter stays there), and gparams [3344] =
 *           dW1 [64][36] (column 35 = db1, columns 0..34 = the 35 input columns of sdf_net.0) | dW2 [16][64] | db2 [16]
 *           w.r.t. the EFFECTIVE (weight-normed) matrices of `field`.  The forward is recomputed per tile; no activations are stored.
 *           scratch: ac_sdf_stencil_backward_scratch(B) bytes (per-wave partial sums, reduced deterministically). */
int ac_sdf_stencil_forward(const ac_field *field, const float *x, uint32_t B, float bound, float eps, float *out16, float *grad,
                           ac_stream_t stream);
size_t ac_sdf_stencil_backward_scratch(uint32_t B);
int ac_sdf_stencil_backward(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                            float eps, float *gfeat, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* The same backward for positions that carry a gradient themselves (x.requires_grad in the reference: the curvature term's perturbed points,
 * models/instant_nsr.py:276-288): additionally g_x [B,3] = the share of d loss / d x that enters through the MLP's own xyz inputs (include_input,
 * :632-633; the offset coordinate of an offset evaluation through its clamp, :690-702).  The share through the encodings: ac_hash_stencil_input_backward
 * on the gfeat this call wrote; the caller adds the two. */
int ac_sdf_stencil_backward_inputs(const ac_field *field, const float *x, const float *g_out16, const float *g_grad, uint32_t B, float bound,
                                   float eps, float *gfeat, float *gparams, float *g_x, void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* Liveness of the renderer's segment hand-off (a ray's final pass is cut into segments that different waves may take; a taker waits, bounded to ~1 s,
 * for the previous segment's state).  A timed-out hand-off poisons the pixel with NaN AND is counted here, per (device, stream), over the life of the
 * launch scratch of that stream: 0 on a healthy run.  Waits for `stream`.  The render launches tag their scratch with a host-side generation number
 * baked into the kernel arguments: they must NOT be captured into a hipGraph (a replay would match the flags of its previous run). */
int ac_render_handoff_timeouts(ac_stream_t stream, uint32_t *count);

/* ---- field evaluation on PACKED samples: the body of NeRFRenderer.run_cuda between raymarching.march_rays[_train] and
 * raymarching.composite_rays[_train].  The reference dispatches cuda_ray=True renders to `run_cuda` (models/instant_nsr.py:362-363) but never defines it
 * (SURVEY 0.1); the per-sample arithmetic is run()'s render core (:205-243) with the marcher's step as the section length:
 *   p = clamp(xyz, +-bound); out16 = forward_sdf(p) (:627-642); g = finite-difference gradient (:687-704, eps); n = g / (1e-5 + |g|);
 *   rgb = forward_color(p, n, out16[1:]) (:644-663); alpha = NeuS alpha of (out16[0], dot(dir, n), delta, inv_s, cos_anneal_ratio) (:219-243), clipped to [0, 1].
 * xyzs, dirs [M,3]; deltas [M * delta_stride] (column 0 is used: march_rays_train writes stride 1, march_rays stride 2).
 * inv_s_dev (optional) = forward_variance() as one float on the device, else inv_s.  sdf [M], gradient [M,3] optional.
 * Bit-identical, per sample, to what ac_render_rays computes for the same point / direction / section length (same tile code). */
int ac_field_samples(const ac_field *field, const float *xyzs, const float *dirs, const float *deltas, uint32_t delta_stride, uint32_t M,
                     float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio, float *alpha, float *rgb, float *normal,
                     float *sdf, float *gradient, ac_stream_t stream);

/* The inference form of run_cuda as ONE launch: per ray, march through the occupancy grid (the arithmetic of ac_march_rays), evaluate the field on the
 * samples (the arithmetic of ac_field_samples, samples of a wave's 64 rays packed into tiles of 16) and composite them in order (the arithmetic of
 * ac_composite_rays: T = 1 - weights_sum, a ray stops at T < 1e-2 or at `far`) -- what the reference-shaped loop compact_rays / march_rays / field /
 * composite_rays computes in rounds with one host read-back each, bit for bit, without the rounds.  near / far = near_far_from_bound(type = 'cube')
 * (models/instant_nsr.py:58-77).  Outputs are the accumulators as composite_rays leaves them: weights_sum [N], depth [N] (sum of w * t: the caller normalises,
 * like run_cuda's last lines), image [N,3] (no background), normal_map [N,3]; n_samples (optional, device, [1]): samples evaluated, accumulated.
 * max_steps (ABI 6): a ray stops after that many samples (0 = only at `far` / T < 1e-2).  The loop of rounds stops at the first round that brings its
 * step count to >= max_steps -- after max_steps .. max_steps + 7 samples per ray, depending on how many rays were alive in its last rounds; this entry
 * stops at exactly max_steps.  The two forms are bit-identical for every ray that needs fewer than max_steps samples (all of them at the default 1024
 * unless a ray crosses > 1024 occupied cells: ~1600 steps of dt_min fit the diagonal of a bound-1.6 cube). */
int ac_render_rays_occupancy(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                             float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                             float *weights_sum, float *depth, float *image, float *normal_map, uint32_t *n_samples, uint32_t max_steps,
                             ac_stream_t stream);

/* The same inference render, the same bits, as rounds of march | field | composite INSIDE one launch with grid barriers between the phases (ABI 7): every lane
 * walks a ray, the samples of a round are evaluated on tiles dealt to all waves, and the rays that go on (not at `far`, T >= 1e-2, below max_steps) form the
 * next round's list -- the reference's loop without its host read-backs; faster than ac_render_rays_occupancy on whole views, where that kernel keeps a
 * quarter of a wave's lanes walking and every wave evaluating its own tiles one after the other.  n_step = 16 samples per ray and round; results do not
 * depend on it.  scratch: ac_render_rays_occupancy_phased_scratch(N) bytes (64 B per ray and round sample: 67 MB for a
 * 256 x 256 view), ZERO-FILLED by the caller before its first use, re-armed by every call, one buffer per stream; a call with fewer rays may reuse it.
 * A launch needs every workgroup resident: the grid is min(what the rays want, hipOccupancyMaxActiveBlocksPerMultiprocessor x compute units) and goes
 * through hipLaunchCooperativeKernel where the device supports it (a plain launch of the same grid where it does not) -- a grid that cannot be co-resident is
 * refused AT LAUNCH (AC_ERR_LAUNCH).  What remains: a foreign kernel holding compute units for longer than a barrier's bounded spin (two seconds;
 * ac_set_occupancy_barrier_ms / AC_OCC_BARRIER_MS override) -- then the phased kernel gives up, counts itself in the scratch's 32-bit word 8 (sticky) and sets
 * the launch's verdict word 9; the call has ALREADY queued the barrier-free kernel of ac_render_rays_occupancy behind it, conditional on that word: it
 * renders every ray again (the same bits) -- a few microseconds when not needed, no host round trip, and the outputs are complete whenever the stream
 * reaches the caller's next operation.  The reference's loop (raymarching/raymarching.py:136-188) never returns partial results either. */
size_t ac_render_rays_occupancy_phased_scratch(uint32_t N);
/* bound of a grid barrier's spin in the phased launches (inference and training form), milliseconds; 0 = back to the default (2000, or AC_OCC_BARRIER_MS).
 * Returns the value in force before the call.  Process-wide. */
uint32_t ac_set_occupancy_barrier_ms(uint32_t ms);
int ac_render_rays_occupancy_phased(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                                    float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                                    float *weights_sum, float *depth, float *image, float *normal_map, uint32_t *n_samples, uint32_t max_steps,
                                    void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* The training form of run_cuda WITHOUT autograd as ONE launch (ABI 7) -- stylize.py's render_val of a cuda_ray network, which never leaves train() mode
 * (stylize.py:46-215 never calls eval()): what ac_march_rays_train (count, scan, write) -> ac_field_samples -> ac_composite_rays_train_forward twice (colour,
 * normal) -> the eikonal term and the background in torch compute, as four phases of one persistent launch separated by grid barriers: the walk of
 * kernel_march_rays_train per ray (raymarching.cu:56-222; perturb: t0 = near + dt_min * pcg32(ray).next_float()), counting and recording the samples'
 * positions; offsets in ray order, the reference's budget rule and the packed samples (replayed from the records, no second walk); the field on tiles of
 * 16 packed samples dealt to all waves (the arithmetic of ac_field_samples with the marcher's step as the section length); kernel_composite_rays_train_forward's
 * loop per ray (:232-301: T < 1e-4 ends the sums) for image and normal map on the same weights.  A BUDGETED call only -- the packed layout lives in the scratch:
 *   capacity            M of ac_march_rays_train (> 0): a ray whose samples would end at or beyond it (offset + count >= M, offsets in ray order from
 *                       counter[0]) is not marched (:133);
 *   composite_capacity  M of ac_composite_rays_train_forward (> 0; the same number in run_cuda): such a ray gets weights_sum = image = 0 (:249);
 *   counter             optional [2] int32 (device): [0] += samples of all rays, [1] += N, like the stand-alone marcher.
 * bg_mode: image += (1 - weights_sum) * bg (run_cuda's last line; torch's three operations in torch's order): 0 none, 1 the scalar bg_value, 2 bg[3],
 * 3 bg[N][3].  gradient_error [1] (device): sum(relax * (|gradient| - 1)^2) / (sum(relax) + 1e-5) over the marched samples, relax = |x| < 1.2
 * (models/instant_nsr.py:266-272), summed in double in a fixed order (run to run identical; torch's fp32 tree differs from it by ~1e-6 relative);
 * NaN if a grid barrier timed out (it cannot with one workgroup per compute unit; the bound exists so that a mis-sized launch fails instead of hanging).
 * weights_sum / image / normal_map are the bits of the chain of operators.  scratch: ac_render_rays_occupancy_train_scratch(N, capacity) bytes, ZERO-FILLED
 * by the caller before its first use (every call leaves it re-armed for calls with the SAME N and capacity: the layout depends on both), one buffer per stream. */
size_t ac_render_rays_occupancy_train_scratch(uint32_t N, uint32_t capacity);
int ac_render_rays_occupancy_train(const ac_field *field, const float *rays_o, const float *rays_d, uint32_t N, const float *grid, uint32_t H,
                                   float mean_density, float bound, float eps, float inv_s, const float *inv_s_dev, float cos_anneal_ratio,
                                   uint32_t perturb, uint32_t capacity, uint32_t composite_capacity, int32_t *counter, const float *bg,
                                   uint32_t bg_mode, float bg_value, float *weights_sum, float *image, float *normal_map, float *gradient_error,
                                   void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* ---- geometry of the learned surface: mesh export and the marcher's density grid ----------------------------------------
 * ac_field_sdf_grid replaces extract_fields (models/instant_nsr.py:728-745): forward_sdf(x)[0] (:627-642) on the grid axis_x x axis_y x axis_z
 * (three DEVICE arrays of nx / ny / nz coordinates: what torch.linspace(bound_min, bound_max, resolution) holds -- the kernel forms the points itself,
 * no meshgrid / cat tensors, no 256^3 blocks, nothing goes to the host); volume [nx,ny,nz] (z fastest, like the reference's `u`), negate != 0 stores
 * -sdf (the `u = -1.0 * u` of extract_geometry :752-753).  Values are bit-identical to ac_field_sdf at the same points. */
int ac_field_sdf_grid(const ac_field *field, const float *axis_x, const float *axis_y, const float *axis_z, uint32_t nx, uint32_t ny, uint32_t nz,
                      float bound, int negate, float *volume, ac_stream_t stream);
/* Marching cubes on a device volume: replaces mcubes.marching_cubes(u, threshold) (models/instant_nsr.py:757; PyMCubes is a third-party package, not
 * vendored in the reference and absent from this image: the algorithm is restated from its definition -- Lorensen & Cline's 256 cases, table generated
 * by tools/gen_mc_table.py; corner flagged <=> u <= iso; one vertex per sign-changing grid edge at the linear zero crossing, formed in double; shared
 * by every triangle that touches the edge; triangle normals point towards u <= iso).  Two calls because the caller owns the output buffers:
 *   ac_marching_cubes_count: classify + scan; counts (DEVICE, [2]) = { vertices, triangles }.  scratch: ac_marching_cubes_scratch(nx, ny, nz) bytes
 *                            (5 bytes per grid point), kept unchanged until the emit call.
 *   ac_marching_cubes_emit : vertices [n_vertices,3] double = index / den * span + lo per axis (the reference's scaling to world units, :760-762, in its
 *                            order of operations; den = resolution - 1, span / lo HOST arrays [3]; den = 1, span = 1, lo = 0 gives PyMCubes' index space),
 *                            triangles [n_triangles,3] int32.  Deterministic order: vertices by owning grid point (linear index, z fastest) then axis
 *                            x, y, z; triangles by cell (linear index) then table position.
 * nx, ny, nz >= 2 and fewer than 2^31 grid points. */
size_t ac_marching_cubes_scratch(uint32_t nx, uint32_t ny, uint32_t nz);
int ac_marching_cubes_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *scratch, size_t scratch_bytes,
                            uint32_t *counts, ac_stream_t stream);
int ac_marching_cubes_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *scratch, size_t scratch_bytes,
                           double den, const double span[3], const double lo[3], double *vertices, uint32_t n_vertices, int32_t *triangles,
                           uint32_t n_triangles, ac_stream_t stream);
/* The same mesh from a grid that is never whole: marching cubes on a WINDOW of x layers, so that a grid of NX x ny x nz points is meshed slab by slab in the
 * memory of one window (the volume costs 4 bytes and the scratch 5 per grid point: 77 GB at 2048^3), and NX x ny x nz may pass 2^31 points.
 *   window [n][ny][nz] floats (DEVICE, z fastest) = grid layers [x0, x0 + n).  first != 0: x0 == 0.  last != 0: x0 + n == NX.  Consecutive windows overlap by
 *   exactly two layers: x0' = x0 + n - 2 (a grid point's owned x edge needs the next layer, a cell the vertex indices of two owner layers).
 *   A window emits the vertices owned by the grid points of its layers 1 .. n-2 (and 0 if first, and n-1 if last) and the triangles of its cell layers
 *   0 .. n-3 (and n-2 if last): the windows tile the grid without gap or repeat, and their outputs CONCATENATED in window order are, bit for bit and in
 *   order, what ac_marching_cubes_emit gives for the whole grid (same flag rule, table, double arithmetic on the global index x0 + i, same order).
 *   ac_marching_cubes_slab_count: flag + classify + scan over the window; counts (DEVICE, [4]) = { vertices emitted, triangles emitted, vertices of layer 0
 *                            (emitted by the previous window; by this one only if first), vertices of the last emitted layer }.  counts[3] of a window ==
 *                            counts[2] of the next: the caller's check that the carry holds.  scratch: ac_marching_cubes_slab_scratch(n, ny, nz) bytes
 *                            (0 for an unsupported window and for n = 2, which runs in the scratch of any larger window), unchanged until the emit call.
 *   ac_marching_cubes_slab_emit : vertices [n_vertices,3] double and triangles [n_triangles,3] int32 of THIS window (n_vertices = counts[0], n_triangles =
 *                            counts[1]).  vertex_base = the global index of the first vertex this window emits = the sum of counts[0] over the windows
 *                            before it; triangle entries are global indices (the carried layer 0 has [vertex_base - counts[2], vertex_base)).
 *                            den, span, lo as for ac_marching_cubes_emit.
 * AC_ERR_BAD_ARG before any launch: n < 3 (n == 2 is allowed for a window both first and last), ny < 2, nz < 2, n ny nz >= 2^31, a NULL buffer, den == 0, a
 * scratch that is too short, x0 + n beyond 32 bits, first with x0 != 0.  No atomics and no waits between workgroups: a deterministic mesh. */
size_t ac_marching_cubes_slab_scratch(uint32_t n, uint32_t ny, uint32_t nz);
int ac_marching_cubes_slab_count(const float *window, uint32_t n, uint32_t ny, uint32_t nz, float iso, uint32_t first, uint32_t last,
                                 void *scratch, size_t scratch_bytes, uint32_t *counts /* DEVICE [4] */, ac_stream_t stream);
int ac_marching_cubes_slab_emit(const float *window, uint32_t n, uint32_t ny, uint32_t nz, float iso, uint32_t first, uint32_t last,
                                void *scratch, size_t scratch_bytes, uint32_t x0, uint32_t vertex_base,
                                double den, const double span[3], const double lo[3],
                                double *vertices, uint32_t n_vertices, int32_t *triangles, uint32_t n_triangles, ac_stream_t stream);
/* ac_mesh_vertex_attrs stands in for nothing: the reference's export is utils.save_mesh(vert, face, ...) (stylize.py:263-269), geometry only -- the avatar's
 * colours never reach the file.  One launch over the vertices ac_marching_cubes_emit wrote (DEVICE doubles, read as they are): per vertex, all in fp32,
 *   p = clamp((float)vertex, +-bound); p0 = p; at most refine_steps times: the seven-point stencil at p exactly as ac_field_samples evaluates it (fd_eps) ->
 *   s = sdf, g = raw finite-difference gradient; r = s - target_sdf; |r| <= tol: stop; gg = (gx gx + gy gy) + gz gz; not gg > 1e-12: stop (status 2);
 *   t = r / gg; q = clamp(p - t g, +-bound); max_k |q_k - p0_k| > max_move: stop and keep p (status 3); p = q.
 * At the final p: positions = p, normals = g / (1e-5 + |g|), rgb = the colour network on (p, normal, geometry features) with the view direction dirs[v], or
 * -normal where dirs is NULL (it matters for a field with Wc1_sh only), sdf = s there, status = why the steps ended: 0 a step's test |r| <= tol was met (the
 * vertex is at a position with |sdf - target_sdf| <= tol) | 1 refine_steps steps taken (the last one is not tested: read sdf) | 2 degenerate gradient |
 * 3 stopped by max_move.  The Newton steps of a wave run while any of its 64 lanes still moves, at most refine_steps: bounded, no atomics, no waits.
 * rgb == NULL skips the colour network (a field whose colour matrices are placeholders is then enough); sdf, status and dirs are optional too.
 * Every value is bit-identical to the CPU oracle's orc_field_samples chained by the same fp32 arithmetic (tests/test_gpu_mesh_attrs.py). */
typedef struct ac_mesh_attr_opts {
    float bound, fd_eps;        /* as ac_field_samples: clamp, finite-difference step            */
    float target_sdf;           /* level the vertices are projected onto (0; -threshold of extract_geometry) */
    int32_t refine_steps;       /* 0 = leave the vertices where they are; at most 16             */
    float tol;                  /* |sdf - target| <= tol: converged                              */
    float max_move;             /* largest |coordinate change| from the input vertex, > 0        */
} ac_mesh_attr_opts;
int ac_mesh_vertex_attrs(const ac_field *field, const double *vertices /*[V,3], as ac_marching_cubes_emit writes them*/, uint32_t V,
                         const float *dirs /*optional [V,3]; NULL: -normal*/, const ac_mesh_attr_opts *opts,
                         float *positions /*[V,3]*/, float *normals /*[V,3]*/, float *rgb /*optional [V,3]*/,
                         float *sdf /*optional [V]: value at the final position*/, uint8_t *status /*optional [V]*/, ac_stream_t stream);
/* ac_mesh_bake_texture: the same per-point work over the TEXELS of a closed-form atlas instead of the vertices -- colour detail no longer tied to vertex density
 * (an added entry, no struct of an existing call changes: ac_version() stays 10).  The size x size image (row 0 on top, [y][x]) is cut into R x R cells of
 * cell x cell texels, R = size / cell (texels beyond R cell belong to nobody); triangle t lives in cell k = t >> 1 at column k % R, row k / R, half t & 1.
 * Texel (i, j) of a cell (i along x) belongs to half 0 iff i + j <= cell - 2.  With L = cell - 5, in fp32, every operation rounded once:
 *   half 0: w1 = (i - 1) / L, w2 = (j - 1) / L;   half 1: w1 = (cell - 2 - i) / L, w2 = (cell - 2 - j) / L;   w1 = max(w1, 0); w2 = max(w2, 0); s = w1 + w2;
 *   s > 1: w1 /= s, w2 /= s, w0 = 0; else w0 = 1 - s        (a texel outside its UV triangle takes a point ON the triangle: the gutter needs no dilation pass)
 *   p = clamp((w0 P0 + w1 P1) + w2 P2, +-bound) per coordinate, P* = positions[triangles[t][*]]
 * then ac_mesh_vertex_attrs's loop from p, unchanged (refine_steps, tol, max_move from the texel's starting point, the same status 0..3), and normal, sdf and colour at the
 * final point with the view direction -normal.  The UV corners sit on the texel centres (1, 1), (cell - 4, 1), (1, cell - 4) of half 0 and (cell - 2, cell - 2),
 * (3, cell - 2), (cell - 2, 3) of half 1: their weights are exactly (1,0,0), (0,1,0), (0,0,1), and a bilinear lookup inside a UV triangle reads its own texels only.
 * Per owned texel: rgb, owner = t, normals, sdf, status.  Per unowned texel: owner = -1, every other output 0, no field evaluation.
 * PRECONDITION: every triangle index lies in [0, V) -- the kernel reads positions through them unchecked (nsr_ops.mesh_bake_texture checks on the device first).
 * AC_ERR_BAD_ARG: a NULL required buffer, cell < 8, size < cell (or > 32768), T > 2 (size / cell)^2, opts outside what ac_mesh_vertex_attrs accepts.
 * The field needs its colour side.  Bit-identical to the CPU oracle's orc_field_samples chained by the same fp32 arithmetic (tests/test_gpu_texture_bake.py). */
typedef struct ac_atlas_opts { uint32_t size, cell; } ac_atlas_opts;
int ac_mesh_bake_texture(const ac_field *field, const float *positions /*[V,3]*/, uint32_t V, const int32_t *triangles /*[T,3]*/, uint32_t T,
                         const ac_atlas_opts *atlas, const ac_mesh_attr_opts *opts,
                         float *rgb /*[S,S,3]*/, int32_t *owner /*[S,S]*/, float *normals /*optional [S,S,3]*/, float *sdf /*optional [S,S]*/,
                         uint8_t *status /*optional [S,S]*/, ac_stream_t stream);
/* ac_field_occlusion: ambient occlusion at points of the level set -- how open the space above a point is, asked of the SDF itself by taps along a cone of directions
 * around the normal (added entries, no struct of an existing call changes: ac_version() stays 10).  It stands in for nothing in the reference.  A kit is K local
 * directions l_k = (lx, ly, lz) in the frame whose z axis is the normal, K weights w_k, J distances t_j, a gain and a level.  All fp32, every operation rounded once,
 * no contraction; fmax / fmin are fmaxf / fminf (a NaN operand is dropped).  Per point, with p = clamp(point, +-bound) per coordinate and n its unit normal:
 *   sg = copysignf(1, nz); a = -1 / (sg + nz); b = (nx ny) a                                   (|sg + nz| >= 1)
 *   T = (1 + sg ((nx nx) a), sg b, -(sg nx));  U = (b, sg + (ny ny) a, -ny)
 *   acc = 0
 *   for k = 0 .. K-1:
 *       w_c = (lx T_c + ly U_c) + lz n_c                                  per coordinate c
 *       v = 1
 *       for j = 0 .. J-1:
 *           q_c = fmin(fmax(p_c + t_j w_c, -bound), bound)                (a NaN coordinate becomes -bound)
 *           s = forward_sdf(q)[0] - level                                 (the bits of ac_field_sdf)
 *           h = t_j lz                                                    (the free distance a flat ground would leave at this tap)
 *           r = fmin(fmax((gain s) / h, 0), 1)                            (a NaN value counts as fully occluded)
 *           v = fmin(v, r)
 *       acc = acc + w_k v
 *   occlusion = fmin(acc, 1)
 * so a plane under a true distance field scores 1, and anything that closes the cone scores less.  A point is ACTIVE if active[i] != 0 (active == NULL: every
 * point) and its three coordinates and its three normal components are finite.  An inactive point stores 0 and is never evaluated: it rides along at the first
 * active point of its tile of 16, and a tile without an active point evaluates nothing.  The taps left of a direction are skipped once v is 0 in every active lane
 * of the wave, which changes no bit.  Nothing else depends on the data: K J evaluations per tile, no atomics, no waits.  N == 0 launches nothing.
 * The kit's tables are HOST pointers; the entry checks them on the host, before any launch, and copies them into the kernel's arguments.
 * AC_ERR_BAD_ARG: NULL opts or a NULL table, n_dirs outside 1..32, n_steps outside 1..16, a number that is not finite, an lz < 0.05, a direction whose length is not
 * within 1e-3 of 1, a negative weight, weights whose sum (in double, in order) is not within 1e-5 of 1, distances not > 0 or not strictly ascending, gain not > 0,
 * bound not > 0, a NULL buffer with N > 0.  The field's SDF side alone is used.
 * Bit-identical to the numpy fp32 restatement around the CPU oracle's Field.sdf (tests/mesh_occlusion_cases.py, tests/test_gpu_mesh_occlusion.py). */
typedef struct ac_occlusion_opts {
    int32_t n_dirs, n_steps;    /* K in 1..32, J in 1..16                                         */
    const float *dirs;          /* HOST [K,3] unit directions in the normal's frame, lz >= 0.05   */
    const float *weights;       /* HOST [K] >= 0, summing to 1                                    */
    const float *dists;         /* HOST [J] > 0, strictly ascending                               */
    float gain;                 /* > 0: r = gain s / h                                            */
    float level;                /* the level set the points lie on (0; -threshold of the export)  */
} ac_occlusion_opts;
int ac_field_occlusion(const ac_field *field, const float *points /*[N,3]*/, const float *normals /*[N,3]*/, const uint8_t *active /*optional [N]*/, uint32_t N,
                       float bound, const ac_occlusion_opts *opts, float *occlusion /*[N]*/, ac_stream_t stream);
/* ac_mesh_bake_maps: ac_mesh_bake_texture with more maps out of the same launch.  Per texel, in order: the texel -> triangle -> point prologue of ac_mesh_bake_texture,
 * unchanged; its refine loop and the normal, sdf and (only when out->rgb is given) colour at the final point, unchanged; then, with occ_opts, ac_field_occlusion's
 * procedure at that final point and normal, active = the texel is owned (and the six numbers are finite).  Colour and occlusion share the texel's refine.
 * out: every pointer may be NULL except owner; positions = the final point.  Unowned texels: owner = -1, every other output 0, no field evaluation.
 * out->occlusion must be NULL exactly when occ_opts is NULL (AC_ERR_BAD_ARG otherwise); the other refusals are ac_mesh_bake_texture's and ac_field_occlusion's.
 * Every output it shares with ac_mesh_bake_texture has the same bits; occlusion has the bits of ac_field_occlusion on (positions, normals, owner >= 0). */
typedef struct ac_bake_out {
    float *rgb;                 /* [S,S,3] */
    int32_t *owner;             /* [S,S], required */
    float *normals, *positions; /* [S,S,3] each */
    float *sdf;                 /* [S,S] */
    uint8_t *status;            /* [S,S] */
    float *occlusion;           /* [S,S] */
} ac_bake_out;
int ac_mesh_bake_maps(const ac_field *field, const float *positions /*[V,3]*/, uint32_t V, const int32_t *triangles /*[T,3]*/, uint32_t T,
                      const ac_atlas_opts *atlas, const ac_mesh_attr_opts *attr_opts, const ac_occlusion_opts *occ_opts /*optional*/,
                      const ac_bake_out *out, ac_stream_t stream);
/* ac_render_rays_surface: the image of the level set itself -- per ray the FIRST point with sdf = level, the field's normal and colour there, its metric distance
 * and a hit mask; one launch, about 18 SDF evaluations per ray where the volumetric render takes 1008 (an added entry, no struct of an existing call changes:
 * ac_version stays 10).  It stands in for nothing in the reference.  All fp32, every operation rounded once (t*d then the add; correctly rounded division); per ray:
 *   near, far = the cube's slab test exactly as ac_render_rays forms it (near >= 0.05)
 *   if not (far > near): status 2, iters 0, t = near, no evaluation
 *   t = near; have_lo = bracketed = false
 *   for it = 1 .. max_iters:
 *       p = clamp(o + t d, +-bound) per coordinate;  s = forward_sdf(p)[0] - level (the bits of ac_field_sdf);  iters = it
 *       s not finite            -> status 5, stop
 *       |s| <= tol              -> status 0, stop
 *       if not bracketed:
 *           if s > 0:
 *               t >= far        -> status 2, stop
 *               (t_lo, s_lo) = (t, s); have_lo = true
 *               t_next = min(t + max(step_scale s, min_step), far);  goto advance
 *           not have_lo         -> status 3, stop                         (the first evaluation is already inside)
 *           bracketed = true; (t_hi, s_hi) = (t, s)
 *       else: s > 0 ? (t_lo, s_lo) = (t, s) : (t_hi, s_hi) = (t, s)
 *       w = t_hi - t_lo; q = s_lo / (s_lo - s_hi); f = t_lo + w q; g = guard w
 *       t_next = min(max(f, t_lo + g), t_hi - g)                          (guarded false position)
 *     advance:
 *       it == max_iters -> status bracketed ? 1 : 4, stop                 (t stays the last EVALUATED t)
 *       t = t_next
 * status: 0 hit | 1 out of iterations inside a bracket | 2 miss (left or never entered the cube) | 3 starts inside | 4 out of iterations without a bracket |
 * 5 value not finite.  SHADED rays are those with status 0, 1 or 3: one seven-point stencil at p = clamp(o + t d) with fd_eps, exactly what ac_mesh_vertex_attrs
 * does with refine_steps = 0: sdf = the centre's raw output 0, normal = g / (1e-5 + |g|), rgb = the colour network on (p, normal, features) with the ray's
 * rays_d row AS GIVEN as view direction (a field with Wc1_sh; none otherwise) -- the bits ac_field_samples returns for that point and direction.
 * Outputs ([N] or [N,3]; each optional except status): image = rgb where shaded, else bg (bg == NULL: white, as in ac_render_rays; image == NULL: the colour
 * network is skipped and a field whose colour matrices are placeholders is enough) | weights_sum = 1 or 0 | depth = t for shaded rays, 0 elsewhere -- METRIC, where
 * the depth of NeRFNetwork.run is normalised to the near/far range | position = p, normal_map, sdf: 0 where not shaded | status, iters: uint8.
 * A wave serves 16 rays and runs while any of them is active, at most max_iters trips: bounded, no atomics, no waits.  N == 0 launches nothing.
 * AC_ERR_BAD_ARG before any launch: a NULL field, rays or status, max_iters outside 1..255, tol not >= 0, fd_eps, step_scale, min_step or bound not > 0, guard
 * outside [0, 0.5).  Bit-identical to the CPU oracle's orc_field_sdf / orc_field_samples chained by the same fp32 arithmetic (tests/test_gpu_surface_render.py). */
typedef struct ac_surface_opts {
    float bound, fd_eps;        /* as ac_field_samples: clamp, finite-difference step of the shading stencil */
    float level;                /* the level set that is rendered (0)                                         */
    float tol;                  /* |sdf - level| <= tol: hit (1e-4)                                           */
    int32_t max_iters;          /* evaluations per ray at most, 1..255 (64)                                   */
    float step_scale, min_step; /* outside step = max(step_scale s, min_step) (1, 1e-3)                       */
    float guard;                /* the false-position point keeps guard * width from both bracket ends (1/8)  */
} ac_surface_opts;
typedef struct ac_surface_out {
    float *image, *weights_sum, *depth, *position, *normal_map, *sdf;
    uint8_t *status, *iters;
} ac_surface_out;
int ac_render_rays_surface(const ac_field *field, const ac_surface_opts *opts, const float *rays_o /*[N,3]*/, const float *rays_d /*[N,3]*/, uint32_t N,
                           const float *bg /*optional [N,3]*/, const ac_surface_out *out, ac_stream_t stream);
/* ac_density_grid_update replaces the grid update of NeRFRenderer.update_extra_state (models/instant_nsr.py:303-346) in two launches (round 6: the densities on
 * ac_field_sdf_grid's x-tiles into the scratch, then one pooling / merging pass; round 5's single launch evaluated a halo per brick and was 3 x slower): forward_sdf on
 * the H^3 grid axis x axis x axis (axis [H], device: torch.linspace(-bound, bound, H)) -> density = inv_s e^(-inv_s |sdf|) / (1 + e^(-inv_s |sdf|)) in the
 * reference's two branches (:331-337; inv_s = 512) -> zero pad by one at the far ends + 2x2x2 max pool, stride 1 (:341-342) -> grid = max(grid * decay,
 * new) IN PLACE (:345) -> mean_out (DEVICE, 1 double) = mean(grid) (:346; accumulated in double, fixed order).  grid [H,H,H].
 * mean: in double where torch.mean reduces in fp32 -- equal to ~1e-7 relative, not bit for bit (a marcher threshold: values it is compared with differ by orders of magnitude).
 * scratch: ac_density_grid_update_scratch(H) bytes (4 H^3 + a few KB), ZEROED once by the caller before its first use (the launch re-arms it).  2 <= H <= 1024. */
size_t ac_density_grid_update_scratch(uint32_t H);
int ac_density_grid_update(const ac_field *field, const float *axis, uint32_t H, float bound, float inv_s, float decay, float *grid,
                           double *mean_out, void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* ---- shading of PACKED samples under autograd (ABI 9, round 6): what NeRFRenderer.run_cuda's train() branch computes between the fused SDF query
 * (ac_sdf_stencil_forward: sdf16 [M,16], gradient [M,3]) and the packed compositor (ac_composite_rays_train_*), one launch each way instead of ~40 torch kernels:
 *   normal = g / (1e-5 + |g|); alpha = the cos-annealed NeuS alpha of ac_field_samples with the marcher's step (deltas, stride 1 | 2) as section length;
 *   eik [M,2] = (relax (|g| - 1)^2, relax), relax = [|xyz| < 1.2][row < *n_valid] -- the two sums of gradient_error (models/instant_nsr.py:266-272).
 * backward: g_alpha [M], g_normal [M,3] (the colour network's), g_eik [M,2] (column 0 is read), any of them NULL = zero -> g_sdf16 [M,16] (column 0 WRITTEN, the
 * caller zero-fills the rest), g_gradient [M,3], g_inv_s_rows [M] (d / d inv_s = their sum).  n_valid: a DEVICE int32. */
int ac_packed_shading_forward(const float *sdf16, const float *gradient, const float *xyzs, const float *dirs, const float *deltas, uint32_t delta_stride,
                              uint32_t M, const int32_t *n_valid, float inv_s, const float *inv_s_dev, float cos_anneal_ratio, float *alpha, float *normal,
                              float *eik, ac_stream_t stream);
int ac_packed_shading_backward(const float *sdf16, const float *gradient, const float *xyzs, const float *dirs, const float *deltas, uint32_t delta_stride,
                               uint32_t M, const int32_t *n_valid, float inv_s, const float *inv_s_dev, float cos_anneal_ratio, const float *g_alpha,
                               const float *g_normal, const float *g_eik, float *g_sdf16, float *g_gradient, float *g_inv_s_rows, ac_stream_t stream);

/* use_viewdirs: the per-ray layer-1 bias of the colour network the renderer forms in its prologue, bias[r][u] = fma chain over j = 0..15 of
 * Wc1_sh[u][j] sh_j(rays_d[r]) (sh = the degree-4 values of ac_sh_encode_forward on the raw direction), as its own launch: bias [N,64], sh [N,16] or NULL.
 * What ac_render_core_backward needs beside the forward's outputs (ac_core_saved.sh_bias) and what turns its g_sh_tiles into d Wc1_sh. */
int ac_sh_bias(const ac_field *field, const float *rays_d, uint32_t N, float *bias, float *sh, ac_stream_t stream);
/* ac_field_color with the view direction of every point: dirs [B,3] (required when field->Wc1_sh is set, ignored otherwise) */
int ac_field_color_dirs(const ac_field *field, const float *x, const float *dirs, const float *n, const float *sdfout, uint32_t B, float *rgb,
                        ac_stream_t stream);

/* ---- colour MLP of the render core (training path): forward_color (models/instant_nsr.py:644-663, use_viewdirs = False)
 * rgb = sigmoid(Wc3 relu(Wc2 relu(Wc1 [x, normal, feat]))) with feat = sdf16[:, 1:16].
 * forward : same values as ac_field_color / ac_render_rays.   backward: recomputes the forward per tile of 16 samples and returns
 * g_normal [B,3], g_sdf16 [B,16] (column 0 = 0: the sdf itself is not an input of the colour net) and
 * gparams [7168] = dWc1 [64][32] (columns 0..20 = x(3), normal(3), feat(15)) | dWc2 [64][64] | dWc3 [16][64] (rows 0..2)
 * w.r.t. the EFFECTIVE matrices of `field`.  scratch: ac_color_backward_scratch(B) bytes. */
int ac_color_forward(const ac_field *field, const float *x, const float *normal, const float *sdf16, uint32_t B, float *rgb, ac_stream_t stream);
size_t ac_color_backward_scratch(uint32_t B);
int ac_color_backward(const ac_field *field, const float *x, const float *normal, const float *sdf16, const float *g_rgb, uint32_t B,
                      float *g_normal, float *g_sdf16, float *gparams, void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* ---- NeuS alpha + compositing of the render core (training path): models/instant_nsr.py:219-263,290-299 for rays in canonical space.
 * Inputs per sample: z_vals, sdf, normal (= gradient / (1e-5 + |gradient|)), colour, [N,T] / [N,T,3]; per ray: origin, direction
 * (near/far of the cube and sample_dist = (far - near) / num_steps are recomputed), optional background [N,3] (NULL = white).
 * forward : image [N,3], weights_sum [N], depth [N], normal_map [N,3], weights [N,T], alpha [N,T] -- the arithmetic of ac_render_rays.
 * backward: (d image, d weights_sum, d depth, d normal_map) -> d sdf [N,T], d normal [N,T,3], d colour [N,T,3] and the per-ray partial
 *           sums of d inv_s [N] (the caller adds them up).  T = num_steps + upsample_steps: a multiple of 16, <= 128 (ac_render_rays' counts), or
 *           ac_render_rays_long's: num_steps >= 2, upsample_steps >= 0 a multiple of 16, T <= 512 -- the weights are then that renderer's, bit for bit
 *           (its last tile of 16 samples masked when 16 does not divide T). */
int ac_composite_forward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf, const float *normal, const float *color,
                         const float *bg, int32_t n_rays, int32_t num_steps, int32_t T, float bound, float inv_s, float cos_anneal_ratio,
                         float *image, float *weights_sum, float *depth, float *normal_map, float *weights, float *alpha, ac_stream_t stream);
int ac_composite_backward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf, const float *normal, const float *color,
                          const float *bg, int32_t n_rays, int32_t num_steps, int32_t T, float bound, float inv_s, float cos_anneal_ratio,
                          const float *g_image, const float *g_weights_sum, const float *g_depth, const float *g_normal_map,
                          float *g_sdf, float *g_normal, float *g_color, float *g_inv_s_per_ray, ac_stream_t stream);

/* ---- the whole differentiable render core (models/instant_nsr.py:190-299) backward in one call (training path).
 * The forward is ac_render_rays itself with the per-sample outputs kept (z_vals, pts, sdf, sdf_out16, gradient, color and the
 * eikonal denominator of ac_eikonal_reduce2): the training render and the inference render are the same launch, bit for bit.
 * At the long renderer's counts (T = num_steps + upsample_steps > 128 or not a multiple of 16; the envelope of ac_composite_forward) the forward is
 * ac_render_rays_long (or ac_render_rays_long_pair) with the same outputs; saved->feat7 must then be NULL when 16 does not divide T (that renderer
 * writes it for whole tiles only: at other counts the stencil features are gathered again), and a field with view directions needs T a multiple of 16 (AC_ERR_BAD_ARG naming the rule otherwise).
 * The backward chains, on `stream`: normals from the finite-difference gradients -> NeuS alpha / compositing backward ->
 * colour MLP backward -> normalisation + eikonal backward -> fused SDF-query backward -> table-gradient scatter.
 * Every argument rule is checked before the first of them: a call refused with AC_ERR_BAD_ARG has queued nothing and written nothing.
 *   upstream: d image [N,3], d weights_sum [N], d depth [N], d normal_map [N,3] (any may be NULL = 0), d gradient_error (1 float, device, or NULL)
 *   results : g_table [offsets[16],2] ACCUMULATED into (like hash_encode_backward); g_sdf_params [3344] and g_color_params [7168]
 *             (layouts of ac_sdf_stencil_backward / ac_color_backward, w.r.t. the EFFECTIVE matrices); g_inv_s_per_ray [N].
 *   scratch : ac_render_core_backward_scratch(field, n_rays, T) bytes (~9 KB per sample, dominated by the scatter queues). */
typedef struct ac_core_saved {
    const float *z_vals, *pts, *sdf, *sdf_out16, *gradient, *color;      /* per-sample outputs of the forward launch */
    const float *eik_den;                                                 /* result2[1] of ac_eikonal_reduce2          */
    const float *feat7;                                                   /* ac_render_out.feat7 of the forward, or NULL: gather again */
    const uint8_t *mask;                                                  /* posed space only (the forward was ac_render_rays_warped): the warp's
                                                                           * alpha mask [N,T] (instant_nsr.py:246-249), with opts->near_m / far_m =
                                                                           * the forward's mesh-guided range and `pts` = the warped points the
                                                                           * forward kept; NULL = canonical space (ABI version 4)                  */
    const float *sh_bias;                                                 /* a field with view directions (ac_field.Wc1_sh) only: ac_sh_bias of the
                                                                           * forward's rays, [N,64]; NULL otherwise (ABI version 6)                  */
} ac_core_saved;
typedef struct ac_core_upstream {
    const float *g_image, *g_weights_sum, *g_depth, *g_normal_map, *g_eik;
    /* ABI 9 (round 6): SEVERAL patches of a view in one backward (stylize.py:143-199 back-propagates a 256 x 256 view as 16 patches of 4096 rays whose
     * gradients add up before the one optimizer.step()).  The eikonal term is a RATIO per patch (instant_nsr.py:266-272), so with eik_group_rays > 0 the
     * rays [k * eik_group_rays, (k + 1) * eik_group_rays) form patch k, whose upstream is g_eik[k] and whose denominator is
     * saved->eik_den[k * eik_den_stride]; 0 = the whole launch is one patch (g_eik[0], eik_den[0]). */
    int32_t eik_group_rays, eik_den_stride;
} ac_core_upstream;
typedef struct ac_core_grads {
    float *g_table, *g_sdf_params, *g_color_params, *g_inv_s_per_ray;
    /* data-parallel training (stylize.py under torch.distributed: one all-reduce of the flat gradient per step): with side_stream != NULL the table
     * scatter finishes levels >= split_level first and makes side_stream wait for exactly that; the caller enqueues the all-reduce of that slice of
     * g_table (entries [offsets[split_level], offsets[16])) on side_stream right after this call returns, and it overlaps the rest of the backward.
     * The slice is final at that point; results are bit-identical to the unsplit call.  NULL / 0 = off (ABI version 4). */
    ac_stream_t side_stream;
    int32_t split_level;
    int32_t reserved;
    float *g_sh_tiles;        /* a field with view directions only: [N * T / 16, 64], per tile of 16 samples the sum of d (layer-1 pre-activation of the colour
                               * network) = the gradient of that tile's share of its ray's view-direction bias.  d Wc1_sh [64,16] = sum over rays r of
                               * (sum of the ray's T / 16 rows) (x) sh(rays_d[r]) (sh from ac_sh_bias): the caller's [N,64]^T x [N,16] product (ABI version 6) */
} ac_core_grads;
size_t ac_render_core_backward_scratch(const ac_field *field, int32_t n_rays, int32_t T);
int ac_render_core_backward(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d, const float *bg,
                            const ac_core_saved *saved, const ac_core_upstream *upstream, const ac_core_grads *grads,
                            void *scratch, size_t scratch_bytes, ac_stream_t stream);

/* ---- the per-step pieces around the training render (stylize.py:95-199), so that a stylisation step runs no framework kernel between the
 * guidance gradient and the optimizer.
 * ac_weight_norm_forward: w[r, :] = v[r, :] * g[r] / ||v[r, :]|| for every layer in ONE launch -- torch.nn.utils.weight_norm(dim = 0) of the
 *   sdf_net / color_net layers (models/instant_nsr.py:557-590).  w may be a strided view (row stride w_stride >= cols). */
#define AC_WN_MAX_LAYERS 8
typedef struct ac_wn_layer { const float *v, *g; float *w; uint32_t rows, cols, w_stride, reserved_; } ac_wn_layer;
int ac_weight_norm_forward(const ac_wn_layer *layers, uint32_t n_layers, ac_stream_t stream);
/* ac_param_grads: gradients w.r.t. the EFFECTIVE matrices (g_sdf_params / g_color_params of ac_render_core_backward) -> the parameters' own
 *   gradient buffers, ACCUMULATED (+=, like autograd's), one launch for up to AC_PG_MAX_ENTRIES entries:
 *   AC_PG_WEIGHT_NORM: src = d W [rows, cols] (row stride src_stride), v, g -> dst = d weight_v [rows, cols], dst2 = d weight_g [rows]
 *   AC_PG_ADD        : dst[i] += src[i * src_stride], i < rows                              (biases)
 *   AC_PG_VARIANCE   : dst[0] += 10 * inv_s * sum_{i < rows} src[i] if 1e-6 < inv_s < 1e6;  g = device pointer to inv_s = exp(10 variance)
 *                      (SingleVarianceNetwork + clip, models/instant_nsr.py:35-45, 666-667; src = g_inv_s_per_ray) */
#define AC_PG_MAX_ENTRIES 12
enum { AC_PG_WEIGHT_NORM = 0, AC_PG_ADD = 1, AC_PG_VARIANCE = 2 };
/* optimizer.step() of the stylisation / reconstruction step (stylize.py:199 over torch.optim.Adam, :355-363; no amsgrad, weight decay or maximize): every
 * parameter tensor of the network in ONE launch, m = m + (1 - beta1)(g - m), v = beta2 v + (1 - beta2) g g, p -= step_size m / (sqrt(v) / sqrt(bc2) + eps);
 * step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t), 1 - beta1 and 1 - beta2 are formed by the caller in double.  zero_grad != 0 also clears the gradients
 * (the next step's optimizer.zero_grad(), stylize.py:143) while they are in registers.  HBM-bound: 28 (32) bytes per element. */
#define AC_ADAM_MAX_TENSORS 16
typedef struct ac_adam_entry { float *param, *grad, *exp_avg, *exp_avg_sq; uint64_t n; } ac_adam_entry;
int ac_adam_step(const ac_adam_entry *tensors, uint32_t n_tensors, float step_size, float beta1, float one_minus_beta1, float beta2,
                 float one_minus_beta2, float eps, float bias_correction2_sqrt, int zero_grad, ac_stream_t stream);

/* forward_variance() of the model (models/instant_nsr.py:35-45, 666-667): inv_s[0] = clip(exp(10 * variance[0]), 1e-6, 1e6), the value
 * ac_render_opts.inv_s_dev points at -- one launch instead of torch's five (ones, mul, exp, mul, clip); same bits (the device library's expf). */
int ac_variance_forward(const float *variance, float *inv_s, ac_stream_t stream);

typedef struct ac_pg_entry { const float *src, *v, *g; float *dst, *dst2; uint32_t rows, cols, src_stride; int32_t kind; } ac_pg_entry;
int ac_param_grads(const ac_pg_entry *entries, uint32_t n_entries, ac_stream_t stream);
/* ac_sds_upstream: the opacity term of the stylisation loss (stylize.py:183-193): loss = sum_i smooth_l1(clamp(ws_i, 0, 1), clamp(ws_gt_i, 0, 1)) *
 *   scale (scale = 1e5 / n_rays for F.smooth_l1_loss(...) * 1e5); g_weights_sum [n_rays] = d loss / d ws (or NULL), loss = 1 float (device, or NULL) */
int ac_sds_upstream(const float *weights_sum, const float *weights_sum_gt, uint32_t n_rays, float scale, float *g_weights_sum, float *loss,
                    ac_stream_t stream);

/* ---- posed-space rendering: NeRFRenderer.run(render_can=False, verts, faces, Ts, use_mesh_guide)
 * models/instant_nsr.py:147-172 (mesh-guided near/far, warp of the coarse samples), :198-203 (warp of the mid points),
 * :246-249 (alpha mask).  The reference moves the samples to the CPU for libigl twice per batch; here the whole sequence
 * (near/far -> coarse points -> warp -> coarse sdf + up-sampling -> warp -> render core) is enqueued on `stream`.
 * As in the reference, the up-sampling queries the field at the UNwarped new samples (cat_z_vals, :464-469). */
typedef struct ac_warp_mesh {
    const float *verts;        /* [V,3]  posed SMPL vertices of the frame */
    const int32_t *faces;      /* [F,3] */
    const double *T;           /* [V',4,4] rest->scene transform per vertex (V' >= V; render_warp.py passes V+24) */
    uint32_t V, F;
    double threshold;          /* mask: squared distance < threshold   (DEFAULT_GEO_THRESH = 0.05) */
    float geo_threshold;       /* radius of the vertex spheres of the near/far guide (DEFAULT_GEO_THRESH) */
    int32_t use_mesh_guide;
    const void *accel;         /* ac_warp_accel_build output for (verts, faces), or NULL = brute-force search */
    /* ABI 9 (round 6) -- temporal seeds of the closest-face searches, or NULL: [n_rays][seed_stride] int32 owned by the caller and kept ACROSS FRAMES, row r =
     * ray r of the launch, columns [0, num_steps) the faces the first search found for the ray's coarse samples, [num_steps, num_steps + T) those of the
     * second search; -1 = none (fill a new buffer with -1).  A search starts every sample from the exact distance of the face stored for its (ray, slot)
     * -- the previous frame's answer, a real face of THIS frame's mesh and therefore a valid bound -- and stores what it finds.  Results are unchanged
     * bit for bit; only the culling gets tighter (an animation's body moves little between frames).  seed_stride >= num_steps + T.  Needs accel. */
    int32_t *seed_faces;
    uint32_t seed_stride;
} ac_warp_mesh;

/* bytes of device scratch ac_render_rays_warped needs for n_rays rays of T = num_steps + upsample_steps samples; if offs is not
 * NULL it receives the byte offsets of {near_m[N] f32, far_m[N] f32, posed pts[N,T,3] f32, canonical pts[N,T,3] f32,
 * mask[N,T] u8, z[N,T] f32} (valid after the call; exposed for tests). */
size_t ac_render_rays_warped_scratch(int32_t n_rays, int32_t T, size_t offs[6]);

/* same arguments and outputs as ac_render_rays, plus the mesh and the scratch buffer */
int ac_render_rays_warped(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                          const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                          const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out,
                          ac_stream_t stream);

/* ac_render_rays_warped for the sample counts of ac_render_rays_long (num_steps >= 2, upsample_steps >= 0 and a multiple of 16, at most 512 samples): the
 * same sequence -- mesh near / far, coarse points, first closest-face search, up-sampling at the warped coarse points, second search, render core at the
 * warped mid points with alpha * mask -- on the long renderer's kernel.  Same arguments, outputs and scratch (ac_render_rays_warped_scratch(n_rays, T, offs))
 * as ac_render_rays_warped; honours opts->skip_masked, mesh->accel, mesh->seed_faces and mesh->use_mesh_guide; sort_index is [N, upsample_steps/16, T];
 * gradient_error (eik_reduced) is formed by ac_eikonal_reduce2 on the same stream.  feat7 must be NULL and opts->opacity_only 0 (AC_ERR_BAD_ARG).  Where
 * both accept the counts, every output is bit-identical to ac_render_rays_warped's. */
int ac_render_rays_long_warped(const ac_field *field, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                               const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                               const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out,
                               ac_stream_t stream);

/* ---- posing the exported mesh: forward SMPL warp of its vertices (csrc/mesh_pose.hip; added entries, no struct of an existing call changes: ABI stays 10)
 * The posed renderer draws { p : sdf(W^-1(p)) = 0 } with W^-1 the inverse warp of ac_warp_samples, so the posed position of a canonical vertex c is the p
 * with W^-1(p) = c -- a fixed point of p <- fwd(M(p), c).  The mesh keeps its triangles, UVs and texture; only its vertices move.  fp64 unless stated:
 *   Blended transform: a face with corners i0, i1, i2 and a point q on it; barycentrics bu, bv, bw by the formula of ac_warp_samples (d00 .. d21, den, bv, bw,
 *     bu = 1 - bv - bw); M = T[i0] bu + T[i1] bv + T[i2] bw element by element in that order; M = [[A, t], [., kappa]], kappa = M[3][3].
 *   Forward application: fwd(M, c) = A c + t / kappa, each coordinate (A[r][0] c0 + A[r][1] c1) + A[r][2] c2 + t[r] / kappa left to right, rounded to fp32:
 *     the p that solves (M^-1 (p, 1))[:3] = c (it includes the reference's quirk that the Ts carry eye(4) / SMPL_SCALE).
 *   Normal: n' = C n with C the cofactor matrix of A (the transposed adjugate), then n' / (1e-30 + |n'|), rounded to fp32.
 *
 * ac_mesh_bind, once per exported mesh (pose independent): for points [V,3] the closest face of the guide IN CANONICAL SPACE (guide_verts [Vg,3], faces [F,3];
 *   the search of ac_warp_samples unchanged -- the culled form when accel, an ac_warp_accel_build of (guide_verts, faces), is given and F <= 16384, else the
 *   exhaustive one; both give the same bits) -> face_id [V], bary [V,3] fp64 of the closest point (bu, bv, bw), optional dist2 [V] fp64.
 *   scratch: ac_mesh_bind_scratch(V, Vg) bytes.
 * ac_mesh_pose, once per frame: points [V,3] (c), optional canonical normals [V,3], the binding, the frame's mesh (posed verts, faces, T, accel, threshold as
 *   ac_render_rays_warped takes them; near/far guide and seeds are not used), on one stream:
 *     p_0 = fwd(M_bind, c), M_bind blended from the frame's T with the binding's face and barycentrics;
 *     for k = 0 .. iters: search at p_k -> can_k = W^-1(p_k), closest point, face, dist^2;  r_k = max_j |can_k[j] - c[j]|;
 *       a difference that is not finite: status 2, stop, keep p_k  |  r_k <= tol: status 0, stop  |  k == iters: status 1, stop  |  else p_{k+1} = fwd(M(p_k), c),
 *       M(p_k) blended at the search's closest point and face.
 *   A stopped vertex keeps its outputs and rides along: every launch covers all V vertices (lane = vertex), no atomics, no waits, iters + 1 searches.
 *   Outputs: positions [V,3] (also the iteration's working buffer); optional normals_out [V,3] = Normal with the A of M(p) at the returned p (needs normals;
 *   0 with status 2); optional residual [V] fp32 = the r of the returned position (+inf with status 2); optional status [V] u8; optional mask [V] u8 =
 *   dist^2 < mesh.threshold at the returned position -- a vertex with mask 0 lies where the renderer draws nothing; it is kept and flagged.
 *   scratch: ac_mesh_pose_scratch(V) bytes.  AC_ERR_BAD_ARG: iters outside 0 .. 16, tol not >= 0, a NULL required buffer, normals_out without normals.
 *   PRECONDITION: every binding face lies in [0, F) and every face index in [0, V') -- nsr_ops.mesh_pose checks the binding on the device first (a binding
 *   face outside the range is not read through: its vertex stays at c with status 2).
 * Every value is bit-identical to the same arithmetic in numpy fp64 around the CPU oracle's orc_warp_samples (tests/test_gpu_mesh_pose.py). */
typedef struct ac_mesh_pose_opts { int32_t iters; float tol; } ac_mesh_pose_opts;
size_t ac_mesh_bind_scratch(uint32_t V, uint32_t Vg);
int ac_mesh_bind(const float *points /*[V,3]*/, uint32_t V, const float *guide_verts /*[Vg,3]*/, uint32_t Vg, const int32_t *faces /*[F,3]*/, uint32_t F,
                 const void *accel /*or NULL*/, int32_t *face_id /*[V]*/, double *bary /*[V,3]*/, double *dist2 /*optional [V]*/,
                 void *scratch, size_t scratch_bytes, ac_stream_t stream);
size_t ac_mesh_pose_scratch(uint32_t V);
int ac_mesh_pose(const float *points /*[V,3]*/, const float *normals /*optional [V,3]*/, uint32_t V, const int32_t *face_id /*[V]*/, const double *bary /*[V,3]*/,
                 const ac_warp_mesh *mesh, const ac_mesh_pose_opts *opts, void *scratch, size_t scratch_bytes,
                 float *positions /*[V,3]*/, float *normals_out /*optional [V,3]*/, float *residual /*optional [V]*/, uint8_t *status /*optional [V]*/,
                 uint8_t *mask /*optional [V]*/, ac_stream_t stream);

/* ---- first-hit render of the POSED level set (csrc/surface_rays.hip; added entries and one new struct, no struct of an existing call changes: ABI stays 10)
 * ac_render_rays_surface_warped: ac_render_rays_surface through the SMPL warp -- per ray the first point p of { p : sdf(W^-1(p)) = level, p inside the mask },
 * W^-1 the inverse warp of ac_warp_samples for the frame's mesh: the set ac_render_rays_warped draws (alpha * mask) and ac_mesh_pose moves a mesh onto.  It
 * stands in for nothing in the reference.  Inputs: those of ac_render_rays_surface, plus w_tol (1e-4) and an ac_warp_mesh of which verts, faces, T, V, F,
 * threshold and accel are used (near/far guide and seeds are not).  rt = sqrtf((float)threshold).  All fp32, every operation rounded once (t*d then the add;
 * correctly rounded division and square root), in this order, unless marked fp64; per ray:
 *   near, far = the cube's slab test exactly as ac_render_rays_surface forms it
 *   if not (far > near): status 2, iters 0, no search, no evaluation
 *   t = near; have_lo = bracketed = lo_masked = false
 *   for it = 1 .. max_iters:
 *       p = clamp(o + t d, +-bound) per coordinate                                      (posed space)
 *       search at p: the bits of ac_warp_samples -> can (its can_pts_f32), dist2 (fp64), m = mask (dist2 < threshold);  iters = it
 *       if m:  c = clamp(can, +-bound);  s = forward_sdf(c)[0] - level (the bits of ac_field_sdf);  k = step_scale
 *       else:  e = sqrtf((float)dist2) - rt;  e not finite -> status 5, stop;  s = max(e, min_step);  k = 1
 *       s not finite            -> status 5, stop
 *       m and |s| <= tol        -> status 0, stop                                       (a masked point is never a hit)
 *       if not bracketed:
 *           if s > 0:
 *               t >= far        -> status 2, stop
 *               (t_lo, s_lo, lo_masked) = (t, s, !m); have_lo = true
 *               t_next = min(t + max(k s, min_step), far);  goto advance
 *           not have_lo         -> status 3, stop                                       (the first evaluation is already inside; necessarily unmasked)
 *           bracketed = true; (t_hi, s_hi) = (t, s)
 *       else: s > 0 ? (t_lo, s_lo, lo_masked) = (t, s, !m) : (t_hi, s_hi) = (t, s)
 *       w = t_hi - t_lo
 *       w <= w_tol              -> status 6, stop                                       (the bracket closed on a jump: the mask boundary cuts the body here)
 *       q = lo_masked ? 0.5 : s_lo / (s_lo - s_hi);  f = t_lo + w q;  g = guard w
 *       t_next = min(max(f, t_lo + g), t_hi - g)
 *     advance:
 *       it == max_iters -> status bracketed ? 1 : 4, stop
 *       t = t_next
 * Outside the mask (dist2 >= threshold) the posed renderer draws nothing; the traced function there is the Euclidean gap to the drawable region, an exact safe
 * step for a unit direction up to the fp32 rounding of the gap (about 1e-7): a gap step never jumps over the body, and a ray far from it reaches it, or far,
 * in a few trips.  Inside the mask the traced function is the canonical SDF scaled by step_scale, as in ac_render_rays_surface.  t_hi is always an unmasked
 * point (s <= 0 implies m: masked values are >= min_step > 0).  When the bracket's positive end is a masked point the function jumps at the mask boundary and
 * false position would crawl: the rule bisects instead.  t is the ray PARAMETER: for |d| != 1 a gap step of e moves the point by e |d| (safe only for
 * |d| <= 1); directions are used as given, never normalised.
 * status 0 .. 5 as in ac_render_rays_surface; 6 = the bracket closed on the mask boundary.  SHADED rays are those with status 0, 1, 3 and 6; their parameter
 * t_s is t for status 0 and 3, t_hi for status 1 and 6.  Shading: one more search at p_s = clamp(o + t_s d); c = clamp(can); one seven-point stencil at c with
 * fd_eps exactly as ac_render_rays_surface shades (sdf, the canonical normal n_c, rgb with the ray's rays_d row AS GIVEN as view direction); the posed normal
 * by ac_mesh_pose's rules: M blended from T at the search's closest point and face with the barycentrics of ac_warp_samples, n = cofactor(A) n_c / (1e-30 +
 * length) in fp64, rounded to fp32.
 * Outputs ([N] or [N,3]; each optional except out->status; each 0 where the ray is not shaded, except image): out->image = rgb, else bg (NULL: white; image ==
 * NULL skips the colour network) | weights_sum = 1 or 0 | depth = t_s | position = p_s (posed) | normal_map = the posed normal | sdf = the centre's raw
 * output 0 at c | status, iters (searches of the root finder) uint8 | out_w (optional) -> canonical = c | normal_can = n_c | face_id = the closest face at
 * p_s (int32, -1 where not shaded).
 * One C call enqueues, on one stream: a prologue, max_iters x (the closest-face search, unchanged: the culled form when accel is given and F <= 16384, else
 * the exhaustive one, same bits; then a trip kernel that evaluates the field once per tile of 16 rays that has an active unmasked ray), one search at the
 * shaded points and the shading kernel.  A ray that has stopped is flagged to the culled search and is not searched again.  No atomics, no waits.  N == 0
 * launches nothing.  scratch: ac_render_rays_surface_warped_scratch(N) bytes (90 N + a few KB).
 * AC_ERR_BAD_ARG before any launch: everything ac_render_rays_surface refuses; w_tol not >= 0; a NULL mesh or a mesh with NULL verts, faces or T; F == 0;
 * a scratch smaller than ac_render_rays_surface_warped_scratch(N).  PRECONDITION, as for ac_mesh_pose: every face index lies in [0, V').
 * Bit-identical to the same fp32 arithmetic in numpy around the CPU oracle's orc_warp_samples / orc_field_sdf / orc_field_samples
 * (tests/test_gpu_surface_posed.py). */
typedef struct ac_surface_warped_out {
    float *canonical, *normal_can;      /* [N,3] each */
    int32_t *face_id;                   /* [N] */
} ac_surface_warped_out;
size_t ac_render_rays_surface_warped_scratch(uint32_t N);
int ac_render_rays_surface_warped(const ac_field *field, const ac_surface_opts *opts, float w_tol, const float *rays_o /*[N,3]*/, const float *rays_d /*[N,3]*/,
                                  uint32_t N, const float *bg /*optional [N,3]*/, const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes,
                                  const ac_surface_out *out, const ac_surface_warped_out *out_w /*optional*/, ac_stream_t stream);

/* ---- cleaning the exported mesh: connected components and compaction on the device (csrc/mesh_components.hip; added entries, no struct of an existing call
 * changes: ABI stays 10).  It stands in for nothing in the reference, whose export writes every detached blob ("floater") the field has.
 * A mesh is triangles [T,3] int32 over V vertices.  Definitions:
 *   Valid triangle: its three indices lie in [0, V).  An invalid triangle joins nothing, is counted in n_bad, belongs to no component and is never emitted by
 *     the compaction.  A degenerate triangle (a, a, b) or a duplicate triangle is valid: it counts as a triangle and joins what it names.
 *   Connectivity: two vertices are connected iff a chain of edges of valid triangles joins them.  A vertex that no valid triangle names is a component of its
 *     own, of size (1 vertex, 0 triangles).
 *   root[v]: the smallest vertex index in v's component -- a canonical labelling: it depends on neither triangle order nor scheduling, so the result is the same
 *     from run to run and equal to any CPU union-find although the kernel hooks with atomics.
 *   component[v]: the rank of root[v] among the roots in ascending order; C = the number of components.  The component of a valid triangle is that of its first
 *     vertex (all three agree).
 *   sizes[c] = { vertices, triangles }: two uint32 per component.
 *   Compaction with keep [C] uint8: a vertex is kept iff keep[component[v]] != 0, a valid triangle iff its component is kept; kept vertices and kept triangles
 *     keep their relative order.  vertex_map [V] int32 = new index or -1; kept_vertices [V'] = old indices, ascending; triangles_out [T',3] = the kept triangles
 *     re-indexed through vertex_map; kept_triangles [T'] = old triangle indices, ascending.
 * ac_mesh_components: a union-find over parent[V] in scratch (initialise; ONE hooking launch over the triangles that always links the larger root under the
 *   smaller, every access of parent[] an agent-scope atomic; flatten), then is_root -> exclusive scan -> component, then the sizes by integer adds aggregated in
 *   the wave (one add per component a wave holds, for its first four; a wave that agrees does one add).  No wave waits for another one (every retry is a lock-free retry whose observed value strictly decreased), no floating-point atomics.
 *   counts (DEVICE, [2]) = { C, n_bad }.  sizes rows [C, max_components) are left untouched; max_components = V always suffices, and then the call does not
 *   synchronise.  With max_components < V the call reads C back (it waits for the stream) and, if C > max_components, returns AC_ERR_BAD_ARG saying so AFTER
 *   writing counts, root, component and the rows that fit.  V == 0 (then T must be 0): C = 0, no launch.  T == 0 with V > 0: V singleton components.
 *   scratch: the _scratch function of (V, T) bytes (4 per vertex and a little).
 * ac_mesh_compact_count: keep flags + scan; counts (DEVICE, [2]) = { V', T' }.  The scratch (its own _scratch function) is kept unchanged until the emit call.
 * ac_mesh_compact_emit : the four outputs, n_kept_vertices = V', n_kept_triangles = T' of the count call (nothing is written past them).  Flags -> scans ->
 *   ordered writes, no atomics.  V' = T' = 0 is legal (vertex_map is all -1; kept_vertices, triangles_out and kept_triangles may be NULL).
 * AC_ERR_BAD_ARG before any launch, with the rule in the message: a NULL required buffer (triangles may be NULL when T == 0, keep when C == 0, sizes when
 * max_components == 0), V or T above 2^31 - 1, triangles over V == 0, a scratch that is too short, C > V, n_kept_vertices > V or n_kept_triangles > T.
 * PRECONDITION of the compaction: component is the labelling of THESE triangles (values outside [0, C) are treated as not kept, never read through). */
size_t ac_mesh_components_scratch(uint32_t V, uint32_t T);
int ac_mesh_components(const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, int32_t *root /*[V]*/, int32_t *component /*[V]*/,
                       uint32_t *sizes /*[max_components][2]*/, uint32_t max_components, uint32_t *counts /* DEVICE [2] = { C, n_bad } */,
                       void *scratch, size_t scratch_bytes, ac_stream_t stream);
size_t ac_mesh_compact_scratch(uint32_t V, uint32_t T);
int ac_mesh_compact_count(const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, const int32_t *component /*[V]*/, const uint8_t *keep /*[C]*/, uint32_t C,
                          void *scratch, size_t scratch_bytes, uint32_t *counts /* DEVICE [2] = { V', T' } */, ac_stream_t stream);
int ac_mesh_compact_emit(const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, const int32_t *component /*[V]*/, const uint8_t *keep /*[C]*/, uint32_t C,
                         void *scratch, size_t scratch_bytes, int32_t *vertex_map /*[V]*/, int32_t *kept_vertices /*[V']*/, uint32_t n_kept_vertices,
                         int32_t *triangles_out /*[T',3]*/, int32_t *kept_triangles /*[T']*/, uint32_t n_kept_triangles, ac_stream_t stream);

/* ---- decimating the exported mesh: vertex clustering on a grid, on the device (csrc/mesh_cluster.hip; added entries and one added struct, no struct of an
 * existing call changes: ABI stays 10).  It stands in for nothing in the reference, whose export writes every marching-cubes triangle.  The step only decides
 * WHICH vertices merge and gives a starting point near the surface; position, normal and colour are restored from the field by ac_mesh_vertex_attrs and
 * ac_mesh_bake_texture, which pull every point onto the level set.  Everything computed here is an integer or a function of exact integer sums: the result
 * depends on neither scheduling nor any hash and equals a numpy restatement exactly (tests/mesh_decimate_cases.py).
 * A mesh is vertices [V,3] float64 (as ac_marching_cubes_emit writes them) and triangles [T,3] int32.  Definitions:
 *   Cluster grid: lo[3], a cell edge h > 0 and n[3] cells per axis, each in [1, 2^21].  For a vertex v, per axis:
 *     t = (v - lo) / h, an fp64 subtraction then an fp64 division.  The vertex is VALID iff, on every axis, t is finite and 0 <= t < n + 1 (the slack of one
 *       cell keeps a vertex at the upper bound, whose t may round just above n, inside the grid).
 *     c = min(floor(t), n - 1);  f = t - (double)c;  q = (int64) floor(f 2^30), so 0 <= q < 2^31.
 *     Key of the cell = (cx n_y + cy) n_z + cz, in 64 bits.
 *     An invalid vertex belongs to no cluster (cluster[v] = -1) and is counted.
 *   Leader of a cell: the smallest index among its valid vertices.  Clusters are numbered by ascending leader.
 *   cluster[v]: the rank of its cell's leader; leader[c]: the leader's old index (ascending in c); members[c]: the member count;
 *   positions[c], per axis: lo + ((double)c_axis + (double)S / ((double)members 2^30)) h, S the int64 sum of the members' q -- evaluated in exactly that order in
 *     fp64, no contraction, correctly rounded division: the mean of the members up to the 2^-30 of a cell their offsets are rounded to.
 *   Triangles: INVALID if an index lies outside [0, V) or names an invalid vertex: counted, never emitted.  A valid triangle maps to (cluster[a], cluster[b],
 *     cluster[c]); it is COLLAPSED, and dropped, iff two of the three are equal.  Surviving triangles keep their relative order and their vertex order
 *     (orientation); kept_triangles [T'] = their old indices, ascending.  Duplicate triangles are NOT removed, back-to-back pairs of a collapsed thin sheet
 *     included: vertex clustering does not preserve manifoldness and this step does not repair it -- ac_mesh_weld_count / _emit (below) remove them
 *     afterwards, and ac_mesh_topology says what is left.
 * ac_mesh_cluster_count: an open-addressing table in scratch with a power-of-two capacity >= 2 V, slots keyed by the cell key and claimed with a 64-bit
 *   compare-exchange under linear probing; a slot holds the leader (integer atomic min), the member count and the three sums (integer atomic adds); then
 *   is_leader -> the ordered scans -> cluster, and the triangle flags through the same scan.  No wave waits for another one (every retry is a lock-free retry:
 *   a slot's key changes once, from empty to a key), no floating-point atomics.  counts (DEVICE, [4]) = { V', T', invalid vertices, invalid triangles }.
 *   The scratch (the _scratch function of (V, T) bytes: 44 per table slot, 8 per vertex and a little) is kept unchanged until the emit call.
 * ac_mesh_cluster_emit : the same head, then the outputs with n_clusters = V' and n_kept_triangles = T' of the count call (nothing is written past them; an
 *   output of length 0 may be NULL).  Ordered writes, no atomics.  It reads the scratch, the triangles and the grid, not the vertices.
 * AC_ERR_BAD_ARG before any launch, with the rule in the message: a NULL required buffer (triangles may be NULL when T == 0, vertices and cluster when V == 0),
 * V or T above 2^31 - 1, h not finite or <= 0, an n outside [1, 2^21], a scratch that is too short, n_clusters > V or n_kept_triangles > T.
 * V == 0 with T == 0 is legal and launches nothing (counts = 0). */
typedef struct ac_cluster_grid {
    double lo[3];                       /* the grid's lower corner */
    double h;                           /* cell edge */
    uint32_t n[3];                      /* cells per axis */
} ac_cluster_grid;
size_t ac_mesh_cluster_scratch(uint32_t V, uint32_t T);
int ac_mesh_cluster_count(const double *vertices /*[V,3]*/, uint32_t V, const int32_t *triangles /*[T,3]*/, uint32_t T, const ac_cluster_grid *grid,
                          void *scratch, size_t scratch_bytes, int32_t *cluster /*[V]*/,
                          uint32_t *counts /* DEVICE [4] = { V', T', invalid vertices, invalid triangles } */, ac_stream_t stream);
int ac_mesh_cluster_emit(const double *vertices /*[V,3]*/, uint32_t V, const int32_t *triangles /*[T,3]*/, uint32_t T, const ac_cluster_grid *grid,
                         void *scratch, size_t scratch_bytes, int32_t *leader /*[V']*/, uint32_t *members /*[V']*/, double *positions /*[V',3]*/,
                         uint32_t n_clusters, int32_t *triangles_out /*[T',3]*/, int32_t *kept_triangles /*[T']*/, uint32_t n_kept_triangles,
                         ac_stream_t stream);

/* ---- welding the decimated mesh and reporting its topology, on the device (csrc/mesh_weld.hip; added entries only, no struct changes: ABI stays 10).  It
 * stands in for nothing in the reference.  The weld removes what ac_mesh_cluster_emit leaves behind where a thin part collapses onto itself: repeated
 * triangles, back-to-back pairs, and the vertices no surviving triangle names.  Everything is integer work on index buffers -- no vertex positions are read --
 * and every output is a function of the input alone: it depends on neither scheduling nor any hash and equals a numpy restatement exactly
 * (tests/mesh_weld_cases.py).  A mesh is triangles [T,3] int32 over V vertices.  Definitions of the weld:
 *   INVALID triangle: an index outside [0, V).  Counted, never emitted.  DEGENERATE triangle: valid, two equal corners.  Counted, never emitted.
 *   Group: all remaining triangles with the same SET of three vertices.  Sign of a member: rotated so that its smallest corner comes first, (a, b, c), it is
 *     + iff b < c.  net = n+ - n-.
 *   Kept triangle of a group: none if net == 0 (the group cancels: a fin of zero thickness); otherwise exactly one, the member with the smallest triangle
 *     index among those of the majority sign, its corner order unchanged.  Kept triangles keep their relative order; kept_triangles [T'] = their old
 *     indices, ascending.
 *   Kept vertex: named by at least one kept triangle.  Kept vertices keep their order.  vertex_map [V] int32 = new index or -1; kept_vertices [V'] = old
 *     indices, ascending; triangles_out [T',3] = the kept triangles re-indexed through vertex_map.
 *   counts (DEVICE, [8]) = { V', T', invalid, degenerate, cancelled, repeated, excess, 0 }: cancelled = the members of groups with net == 0; repeated = the
 *     members dropped from groups with net != 0; excess = the sum of |net| - 1 over the groups.  T = T' + invalid + degenerate + cancelled + repeated.
 *   For the triangles of a closed, consistently oriented mesh after ac_mesh_cluster_emit: if excess == 0, the welded mesh has every directed edge u -> v as
 *   often as v -> u (the weld removes whole cancelling pairs, and same-sign copies of a chain whose boundary is zero).
 * ac_mesh_weld_count: an open-addressing table of int32 in scratch with a power-of-two capacity >= 2 T.  The vertex set needs 93 bits, so a slot holds a
 *   triangle INDEX, claimed with a 32-bit compare-exchange from "empty" under linear probing; equality at an occupied slot is decided by reading the occupant's
 *   corners from the (immutable) input and comparing sorted triples.  A slot holds the smallest + member and the smallest - member (integer atomic mins) and
 *   the two member counts (integer atomic adds); then one flag pass (kept triangles, referenced vertices) and the ordered scans.  No wave waits for another
 *   one (a slot's occupant changes once, from empty to an index), no floating-point atomics.  The scratch (the _scratch function of (V, T) bytes: 20 per table
 *   slot, 5 per triangle, 1 per vertex and a little) is kept unchanged until the emit call.
 * ac_mesh_weld_emit : the same head, then the outputs with n_kept_vertices = V' and n_kept_triangles = T' of the count call (nothing is written past them;
 *   an output of length 0 may be NULL; vertex_map is written whole).  Ordered writes, no atomics.
 * ac_mesh_topology: the report.  An EDGE is the unordered pair of two corners of a valid, non-degenerate triangle; fwd = its uses in the direction
 *   min -> max, bwd = its uses in the other direction.  counts (DEVICE, [8]) = { E distinct edges, boundary (fwd + bwd == 1), nonmanifold (fwd + bwd > 2),
 *   misoriented (fwd + bwd == 2 and fwd != bwd), referenced vertices (named by a valid non-degenerate triangle), F valid non-degenerate triangles, invalid,
 *   degenerate }.  A closed oriented 2-manifold (up to non-manifold VERTICES, which are not looked for) has boundary = nonmanifold = misoriented = 0.
 *   The table of ac_mesh_cluster_count, keyed by (min << 31) | max, with a power-of-two capacity >= 6 T and two uint32 use counters per slot (integer
 *   atomic adds); a pass over the slots reduces them, aggregated in the wave, by integer adds.  scratch: 16 bytes per slot, 1 per vertex and a little.
 * AC_ERR_BAD_ARG before any launch, with the rule in the message: a NULL required buffer (triangles may be NULL when T == 0, everything but counts when
 * V == 0), V or T above 2^31 - 1, triangles over V == 0, a scratch that is too short, n_kept_vertices > V or n_kept_triangles > T.
 * V == 0 with T == 0 is legal and launches nothing (counts = 0).  Splitting non-manifold vertices
 * and edges: ac_mesh_repair_count / _emit (below).  Not built: filling holes. */
size_t ac_mesh_weld_scratch(uint32_t V, uint32_t T);
int ac_mesh_weld_count(const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes,
                       uint32_t *counts /* DEVICE [8] = { V', T', invalid, degenerate, cancelled, repeated, excess, 0 } */, ac_stream_t stream);
int ac_mesh_weld_emit(const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes, int32_t *vertex_map /*[V]*/,
                      int32_t *kept_vertices /*[V']*/, uint32_t n_kept_vertices, int32_t *triangles_out /*[T',3]*/, int32_t *kept_triangles /*[T']*/,
                      uint32_t n_kept_triangles, ac_stream_t stream);
size_t ac_mesh_topology_scratch(uint32_t V, uint32_t T);
int ac_mesh_topology(const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes,
                     uint32_t *counts /* DEVICE [8] = { E, boundary, nonmanifold, misoriented, referenced, F, invalid, degenerate } */, ac_stream_t stream);

/* ---- making the mesh manifold, on the device (csrc/mesh_repair.hip; added entries only, no struct changes: ABI stays 10).  It stands in for nothing in the
 * reference.  Vertex clustering pushes two sheets of the surface onto one edge or one vertex; the repair tells the sheets apart again and gives every sheet its
 * own copy of the vertex.  Every output is a function of the input alone and equals a numpy restatement exactly (tests/mesh_repair_cases.py).
 * Input: vertices [V,3] fp32, triangles [T,3] int32.  INVALID triangle: an index outside [0, V); counted, copied as it stands, takes no part (the Python
 * front end raises).  DEGENERATE triangle: valid, two equal corners; counted, copied as it stands, takes no part.  The others are MEMBERS.
 *   Uses.  Corner k of triangle t has the corner id 3 t + k.  Side k runs from corner k to corner (k + 1) % 3; its use id is 3 t + k and its opposite vertex
 *     is corner (k + 2) % 3.  The uses of the edge (a, b), a < b, are the member sides over { a, b }; a use is FORWARD if it runs a -> b.
 *   Joining, per edge, by its number of uses n.  n = 1: nothing.  n = 2: the two uses are joined, whatever their directions.  3 <= n <= 8: the edge is
 *     NON-MANIFOLD; its uses are ordered around it and paired (below); paired uses are joined, the others are CUT.  n > 8: the edge is CROWDED: it counts as
 *     non-manifold and all its uses are cut.
 *   Order around an edge.  All arithmetic is fp64 on the fp32 positions widened, every operation rounded on its own (no fused multiply-add).  The cross
 *     product is (y z' - z y', z x' - x z', x y' - y x'), the dot product (x x' + y y') + z z'.  e = P[b] - P[a]; d_i = P[c_i] - P[a] with c_i the opposite
 *     vertex of use i; w = e x d_r with r the use of smallest id; u = w x e; X_i = d_i . u, Y_i = d_i . w, s = |X_i| + |Y_i|.  The key of use i is 0 if
 *     s == 0; otherwise, with q = Y_i / s: q if X_i >= 0 and Y_i >= 0, 2 - q if X_i < 0, and 4 + q otherwise -- a monotone stand-in for the angle, in [0, 4).
 *     If any key of the edge is not finite, the edge is treated as crowded.  The uses are sorted by (key, use id) into a cyclic list.
 *   Pairing.  A backward use has the solid on its increasing-angle side, a forward use on its decreasing side.  From the start of the list, find the first
 *     position whose use is backward and whose cyclic successor is forward and a different use; join the two, remove both from the list, and start again from
 *     the beginning; stop when no such position is left.  (Cyclic bracket matching: with as many forward as backward uses it pairs every use, and each pair
 *     bounds one wedge of solid, so two bodies that touch along an edge come apart as two bodies.)
 *   Fans.  Joining two uses of the edge (a, b) unites the two triangles' corners at a, and their corners at b.  A FAN is a set of united member corners; its
 *     root is its smallest corner id.  Every vertex v keeps the index v for the fan whose root is smallest among its fans; every other fan gets a new index
 *     V + j, j = the rank of its root among all such extra roots in ascending order.  source [V'] = the original vertex of every output vertex (the identity
 *     on the first V).  triangles_out [T,3]: the same T, order and orientation, member corners rewritten to their fan's index.  Vertices nobody names keep
 *     their index: the repair never removes anything.  Non-manifold VERTICES are split by the same rule: two cones that meet in a point are two fans.
 *   counts (DEVICE, [8]) = { V', split (vertices with more than one fan), nonmanifold (edges, crowded ones included), paired (uses), cut (uses), crowded
 *     (edges), invalid, degenerate }.  Repairing the output again adds nothing.  What stays non-manifold afterwards are pinches -- an edge where the surface
 *     touches itself while both end points keep a single fan --, which no vertex duplication can separate: ac_mesh_topology counts them.
 * ac_mesh_repair_count: the table of ac_mesh_topology, keyed by (min << 31) | max, capacity >= 6 T, with a use counter and the smallest and largest use id
 *   per slot (integer atomic add / min / max); the slots with 3 to 8 uses get their use ids into a side list, and the lane that owns the edge computes the
 *   keys, sorts (key, use id) and matches the brackets in registers; the joins go through the lock-free union-find of ac_mesh_components over the 3 T corner
 *   ids; then a flatten pass, an integer atomic min of the roots per vertex, the extra-root flags and the ordered scans.  No wave waits for another one, no
 *   floating-point atomics.  The scratch (the _scratch function of (V, T) bytes: 24 per table slot, 36 per triangle, 8 per vertex and a little) is kept
 *   unchanged until the emit call.
 * ac_mesh_repair_emit : the same head, then the outputs with n_vertices = V' of the count call (source is written below n_vertices only, triangles_out
 *   whole).  Ordered writes, no atomics.
 * AC_ERR_BAD_ARG before any launch, with the rule in the message: a NULL required buffer (triangles and triangles_out may be NULL when T == 0, everything
 * but counts when V == 0), V or T above 2^31 - 1, 3 T above 2^31 - 1 (corner ids are int32), triangles over V == 0, a scratch that is too short,
 * n_vertices outside [V, V + 3 T].  V == 0 with T == 0 is legal and launches nothing (counts = 0).  Not built: re-pairing pinched edges, filling holes. */
size_t ac_mesh_repair_scratch(uint32_t V, uint32_t T);
int ac_mesh_repair_count(const float *vertices /*[V,3]*/, const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes,
                         uint32_t *counts /* DEVICE [8] = { V', split, nonmanifold, paired, cut, crowded, invalid, degenerate } */, ac_stream_t stream);
int ac_mesh_repair_emit(const float *vertices /*[V,3]*/, const int32_t *triangles /*[T,3]*/, uint32_t T, uint32_t V, void *scratch, size_t scratch_bytes,
                        int32_t *triangles_out /*[T,3]*/, int32_t *source /*[V']*/, uint32_t n_vertices, ac_stream_t stream);

/* ---- rendering from a half-precision hash table (opt-in, inference only) ----------------------------------------------------------------------------
 * The half table holds ONE dword per entry of the fp32 table [n_entries][2] (n_entries = field->offsets[16]): channel 0 as an IEEE binary16 in the low
 * half, channel 1 in the high half -- 4 bytes per entry instead of 8, the same level offsets.  ac_table_to_half makes it: every value is rounded to
 * nearest even, subnormals are kept, NaN stays NaN, |v| > 65504 that rounds up becomes +-inf.  *n_bad (a device word the caller zeroes; the call adds
 * to it) counts the entries in which a FINITE fp32 value became +-inf: a field that does not fit binary16 must not be rendered from the half table.
 *
 * ac_render_rays_h16 / ac_render_rays_warped_h16 are ac_render_rays / ac_render_rays_warped with every table gather one dword from table_h16, widened to
 * fp32 exactly (binary16 -> binary32 loses nothing); all other arithmetic is the same code.  Contract: every output is BIT-IDENTICAL to the fp32 entry
 * given the widened table (each half converted back to fp32) as field->table.  How close that is to a render from the unrounded table is a property
 * of the field, not of these entries.  field->table is not read (it may be NULL); the other members of the field, the options,
 * the trailing arguments, the outputs and the scratch (ac_render_rays_warped_scratch) are those of the fp32 entries.
 * AC_ERR_BAD_ARG, with the rule in the message: table_h16 NULL; opts->opacity_only; out->feat7, out->sdf_out16 or out->pts (the training extras: nothing
 * trains from the half table); sample counts outside the window of ac_render_rays.  There is no half-table form of the pair launch, the long renderer,
 * the occupancy, geometry or training entries. */
int ac_table_to_half(const float *table, uint32_t n_entries, void *table_h16, uint32_t *n_bad, ac_stream_t stream);
int ac_render_rays_h16(const ac_field *field, const void *table_h16, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                       const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                       const ac_render_out *out, ac_stream_t stream);
int ac_render_rays_warped_h16(const ac_field *field, const void *table_h16, const ac_render_opts *opts, const float *rays_o, const float *rays_d,
                              const float *bg, const float *noise, const float *lin_z, const float *lin_u,
                              const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_render_out *out,
                              ac_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AVATARCRAFT_HIP_H */
