// avatarcraft_amd/csrc/surface_rays.hip -- the first-hit renders of the level set: per ray the first point with sdf = level, shaded there.
//   ac_render_rays_surface         in canonical space: one kernel, the root finder's loop inside it;
//   ac_render_rays_surface_warped  in posed space, through the SMPL warp: the closest-face search of warp.hip before every evaluation, so the loop is unrolled
//                                  on the host over three kernels.
// Both trace with the same scalar rule (root_step), shade through refine_shade_tile (shade_tile.hpp) and write the rows of ac_surface_out through one epilogue.
#include "shade_tile.hpp"
#include "field_host.hpp"
#include "mesh_blend.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------- what both renderers share
// The root finder's scalar update after one evaluation of the traced function at parameter r.t (the procedure, operation by operation:
// include/avatarcraft_hip.h, ac_render_rays_surface and ac_render_rays_surface_warped).  In order: non-finite value, hit, update of an open bracket, outside
// step, first evaluation already inside, the bracket opens, guarded false position in the bracket, out of iterations.
//   in : s = traced value - level | k: the outside step is max(k s, min_step) | masked: s is the gap to the mask, not an SDF value | it: this evaluation, 1 ..
//   out: true = the ray stops with status st (r.t stays the evaluated parameter); false = r.t is the next parameter
// POSED adds what the mask needs: a masked point is never a hit, PF_LO_MASKED (bisection while the bracket's positive end is a masked point) and the stop on a
// bracket no wider than w_tol (status 6).  Operands and order of every float operation are part of the contract (tests/surface_cases.py: restate and
// tests/surface_posed_cases.py: restate_posed state them independently, bit for bit).
enum : uint32_t { PF_HAVE_LO = 1, PF_BRACKETED = 2, PF_LO_MASKED = 4 };
struct TraceOpts { int max_iters; float level, tol, step_scale, min_step, guard, w_tol; };     // of ac_surface_opts | w_tol: POSED only
struct RootState { float t, t_lo, s_lo, t_hi, s_hi, far; uint32_t fl; };                      // fl: PF_*

template <bool POSED>
__device__ __forceinline__ bool root_step(RootState &r, float s, float k, bool masked, int it, const TraceOpts &o, uint32_t &st)
{
    auto set_lo = [&] { r.t_lo = r.t; r.s_lo = s; if (POSED) r.fl = masked ? (r.fl | PF_LO_MASKED) : (r.fl & ~(uint32_t)PF_LO_MASKED); };
    float t_next = r.t;
    bool in_bracket = false;
    if (!(__builtin_fabsf(s) < __builtin_inff())) { st = 5u; return true; }
    if (!masked && __builtin_fabsf(s) <= o.tol) { st = 0u; return true; }
    if (r.fl & PF_BRACKETED) {
        if (s > 0.0f) set_lo(); else { r.t_hi = r.t; r.s_hi = s; }
        in_bracket = true;
    } else if (s > 0.0f) {                                                       // still outside: a sphere-tracing step, never past far
        if (r.t >= r.far) { st = 2u; return true; }
        set_lo(); r.fl |= PF_HAVE_LO;
        t_next = __builtin_fminf(r.t + __builtin_fmaxf(k * s, o.min_step), r.far);
    } else if (!(r.fl & PF_HAVE_LO)) { st = 3u; return true; }                   // the first evaluation is already inside
    else { r.fl |= PF_BRACKETED; r.t_hi = r.t; r.s_hi = s; in_bracket = true; }
    if (in_bracket) {
        const float w = r.t_hi - r.t_lo;
        if (POSED && w <= o.w_tol) { st = 6u; return true; }                     // the bracket closed on a jump: the mask boundary cuts the body here
        // guarded false position; bisection while the positive end is a masked point
        const float q = (POSED && (r.fl & PF_LO_MASKED)) ? 0.5f : r.s_lo / (r.s_lo - r.s_hi), f = r.t_lo + w * q, gd = o.guard * w;
        t_next = __builtin_fminf(__builtin_fmaxf(f, r.t_lo + gd), r.t_hi - gd);
    }
    if (it == o.max_iters) { st = (r.fl & PF_BRACKETED) ? 1u : 4u; return true; }
    r.t = t_next;
    return false;
}

// The rows of ac_surface_out for ray b (its lane g == 0 calls this): each "value if shaded else 0", the image the colour, the background or white.
// t, (hx, hy, hz), (nx, ny, nz): the ray's depth, position and normal_map rows; rgb and sdf come from r.
__device__ __forceinline__ void store_surface_out(const ac_surface_out &o, const float *bg, uint32_t b, bool shaded, const TileShade &r, float t,
                                                  float hx, float hy, float hz, float nx, float ny, float nz, uint32_t st, uint32_t iters)
{
    const size_t b3 = 3 * (size_t)b;
    if (o.image) {
        float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
        if (shaded) { c0 = r.rgb[0]; c1 = r.rgb[1]; c2 = r.rgb[2]; }
        else if (bg) { c0 = bg[b3]; c1 = bg[b3 + 1]; c2 = bg[b3 + 2]; }
        o.image[b3] = c0; o.image[b3 + 1] = c1; o.image[b3 + 2] = c2;
    }
    if (o.weights_sum) o.weights_sum[b] = shaded ? 1.0f : 0.0f;
    if (o.depth) o.depth[b] = shaded ? t : 0.0f;
    if (o.position) { o.position[b3] = shaded ? hx : 0.0f; o.position[b3 + 1] = shaded ? hy : 0.0f; o.position[b3 + 2] = shaded ? hz : 0.0f; }
    if (o.normal_map) { o.normal_map[b3] = shaded ? nx : 0.0f; o.normal_map[b3 + 1] = shaded ? ny : 0.0f; o.normal_map[b3 + 2] = shaded ? nz : 0.0f; }
    if (o.sdf) o.sdf[b] = shaded ? r.s : 0.0f;
    o.status[b] = (uint8_t)st;
    if (o.iters) o.iters[b] = (uint8_t)iters;
}

struct RayArgs {
    const float *rays_o, *rays_d, *bg;     // [N,3] [N,3] [N,3] | NULL: white
    uint32_t N;
    TraceOpts o;
};

// ---------------------------------------------------------------------------------------------------------------- first-hit render of the level set
// The image of the surface the export writes: per ray the first point with sdf = level, found by sphere-tracing steps until the sign changes and guarded false
// position inside the bracket (the procedure, operation by operation: include/avatarcraft_hip.h, ac_render_rays_surface), then refine_shade_tile with steps = 0
// at that point -- normal, sdf and colour as ac_field_samples gives them.  A wave owns tiles of 16 consecutive rays, lane (n, g) serves ray n of the tile (the
// four lanes of a ray hold the same state).  Every trip of the root-finder loop is ONE sdf_tile call at every lane's current point, then the scalar update in the
// lanes still active; stopped lanes ride along at their point.  The loop ends when no lane of the wave is active or after max_iters trips: wave-uniform, bounded.
// A tile without a shaded ray (status 0, 1 or 3) skips the stencil and the colour network; in a tile with some, the other lanes ride along at the first shaded
// lane's point.  No atomics, no waits on other waves, plain vector stores.
__global__ __launch_bounds__(FBLOCK) void surface_rays_kernel(const RenderArgs a, const RayArgs m, const ac_surface_out out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (out.image) fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const RefineOpts ro{ 0, 0.0f, 0.0f, 0.0f, out.image != nullptr };
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const float *po = m.rays_o + 3 * (size_t)bb, *pd = m.rays_d + 3 * (size_t)bb;
        const float ox = po[0], oy = po[1], oz = po[2], dx = pd[0], dy = pd[1], dz = pd[2];
        float near;
        RootState rs{};                                                          // in registers across the loop
        cube_near_far(ox, oy, oz, dx, dy, dz, bound, near, rs.far);
        rs.t = near;
        uint32_t st = 2u, iters = 0u;
        bool active = rs.far > near;
        float px = clampf(ox + rs.t * dx, -bound, bound), py = clampf(oy + rs.t * dy, -bound, bound), pz = clampf(oz + rs.t * dz, -bound, bound);
#pragma unroll 1
        for (int it = 1; it <= m.o.max_iters; ++it) {
            if (__ballot(active) == 0ull) break;                                 // (wave-uniform)
            const f32x4 o = sdf_tile(lds, fc, lane, px, py, pz);
            const float s = __shfl(o[0], n) - m.o.level;                         // output 0 lives in the lanes g == 0
            if (active) {
                iters = (uint32_t)it;
                if (root_step<false>(rs, s, m.o.step_scale, false, it, m.o, st)) active = false;       // (t stays the last evaluated t)
                else { px = clampf(ox + rs.t * dx, -bound, bound); py = clampf(oy + rs.t * dy, -bound, bound); pz = clampf(oz + rs.t * dz, -bound, bound); }
            }
        }
        const bool shaded = st == 0u || st == 1u || st == 3u;
        TileShade r{};
        const float hx = px, hy = py, hz = pz;                                   // this ray's own point
        if (ride_along(shaded, px, py, pz))                                      // (wave-uniform)
            r = refine_shade_tile(lds, fsl, fc, a, ro, lane, m.rays_d, (size_t)bb, false, px, py, pz);
        if (b < m.N && g == 0) store_surface_out(out, m.bg, b, shaded, r, rs.t, hx, hy, hz, r.fn.nx, r.fn.ny, r.fn.nz, st, iters);
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------- first-hit render of the POSED level set
// The image of { p : sdf(W^-1(p)) = level, p inside the mask }: the set the posed renderer draws and net.pose_mesh moves the exported mesh onto (the procedure,
// operation by operation: include/avatarcraft_hip.h, ac_render_rays_surface_warped).  Every evaluation of the traced function needs the closest-face search of
// warp.hip (over the mesh's culling structure: warp_accel.hpp, built by warp_accel_build.hip) at the ray's posed point first.  That search is wave-cooperative and compiled for <= 128 VGPRs, the sdf_tile code needs about 226: they stay separate
// kernels and the root finder's loop is unrolled on the HOST -- a sequence on one stream, the per-ray state kept in the scratch between the launches:
//   posed_start_kernel: near / far, the ray state, the first posed point;
//   max_iters times: the search (unchanged, through its internal launcher; the per-ray `stopped` byte is its ray_dead with one sample per ray), then
//     posed_trip_kernel: ONE sdf_tile call per tile of 16 rays at the clamped canonical points -- only for a tile with an active unmasked ray (ballot) -- and the
//     scalar update; it writes the state, the next posed point (the shaded point of a ray that stops) and the stopped byte;
//   one search at the shaded points (ray_dead = the `noshade` byte), then posed_shade_kernel: refine_shade_tile with steps = 0 at the clamped canonical point behind
//     surface_rays_kernel's ride-along rule, then the blended transform and the cofactor normal of mesh_blend.hpp in fp64, lane = ray.
// The host cannot know when every ray has stopped: all max_iters trips are enqueued, a trip without an active ray reads 16 bytes per tile and evaluates nothing.
// No atomics, no grid barrier, no waits on other waves, plain vector stores; a short last tile reads ray N - 1 and stores nothing for its padding lanes.
struct PosedState {                        // the scratch of ac_render_rays_surface_warped, one row per ray
    float *pts, *can;                      // [N,3] the posed point the next search reads | its canonical point (the search's can_pts_f32)
    double *closest, *dist2;               // [N,3], [N] of the search
    int32_t *face;                         // [N]
    uint8_t *smask;                        // [N] the search's mask
    uint8_t *stopped, *noshade;            // [N] ray_dead of the trips' searches | of the shading search
    uint8_t *st, *iters, *flags;           // [N] status, evaluations, PF_*
    float *t, *t_lo, *s_lo, *t_hi, *s_hi, *far;      // [N] each; t = the shaded parameter once the ray has stopped
};
struct PosedArgs : RayArgs {
    float rt;                              // the mask's radius: sqrt(threshold)
    PosedState s;
};

__global__ __launch_bounds__(256) void posed_start_kernel(const PosedArgs m, float bound)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= m.N) return;
    const float *po = m.rays_o + 3 * (size_t)b, *pd = m.rays_d + 3 * (size_t)b;
    float near, far;
    cube_near_far(po[0], po[1], po[2], pd[0], pd[1], pd[2], bound, near, far);
    const PosedState &s = m.s;
    s.t[b] = near; s.far[b] = far;
    s.t_lo[b] = 0.0f; s.s_lo[b] = 0.0f; s.t_hi[b] = 0.0f; s.s_hi[b] = 0.0f;
    s.flags[b] = 0; s.st[b] = 2; s.iters[b] = 0;
    s.stopped[b] = far > near ? 0 : 1;
    s.noshade[b] = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.pts[3 * (size_t)b + k] = clampf(po[k] + near * pd[k], -bound, bound);
}

__global__ __launch_bounds__(FBLOCK) void posed_trip_kernel(const RenderArgs a, const PosedArgs m, int it)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const PosedState &s = m.s;
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const bool active = s.stopped[bb] == 0;                                  // a stopped ray was not searched: nothing of the search is read for it
        const bool unmasked = active && s.smask[bb] != 0;
        float sv = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
        if (unmasked) {
            const float *c = s.can + 3 * (size_t)bb;
            cx = clampf(c[0], -bound, bound); cy = clampf(c[1], -bound, bound); cz = clampf(c[2], -bound, bound);
        }
        if (ride_along(unmasked, cx, cy, cz)) {                                  // (wave-uniform) one evaluation at the clamped canonical points
            const f32x4 o = sdf_tile(lds, fc, lane, cx, cy, cz);
            sv = __shfl(o[0], n) - m.o.level;                                    // output 0 lives in the lanes g == 0
        }
        if (active && b < m.N && g == 0) {
            RootState rs{ s.t[b], s.t_lo[b], s.s_lo[b], s.t_hi[b], s.s_hi[b], s.far[b], s.flags[b] };
            uint32_t st = 2u;
            bool stop = false;
            float sc = sv, k = m.o.step_scale;
            if (!unmasked) {                                                     // outside the mask: the gap to the drawable region, an exact safe step
                const float e = __builtin_sqrtf((float)s.dist2[b]) - m.rt;
                if (!(__builtin_fabsf(e) < __builtin_inff())) { st = 5u; stop = true; }
                sc = __builtin_fmaxf(e, m.o.min_step); k = 1.0f;
            }
            if (!stop) stop = root_step<true>(rs, sc, k, !unmasked, it, m.o, st);
            bool shaded = false;
            if (stop) {
                shaded = st == 0u || st == 1u || st == 3u || st == 6u;
                if (st == 1u || st == 6u) rs.t = rs.t_hi;                        // the shaded parameter: the bracket's inner end
                s.stopped[b] = 1; s.noshade[b] = shaded ? 0 : 1; s.st[b] = (uint8_t)st;
            }
            s.iters[b] = (uint8_t)it;
            s.t[b] = rs.t; s.t_lo[b] = rs.t_lo; s.s_lo[b] = rs.s_lo; s.t_hi[b] = rs.t_hi; s.s_hi[b] = rs.s_hi; s.flags[b] = (uint8_t)rs.fl;
            if (!stop || shaded) {                                               // the next search's point | the shading search's point
                const float *po = m.rays_o + 3 * (size_t)b, *pd = m.rays_d + 3 * (size_t)b;
#pragma unroll
                for (int c = 0; c < 3; ++c) s.pts[3 * (size_t)b + c] = clampf(po[c] + rs.t * pd[c], -bound, bound);
            }
        }
    }
}

struct PosedOut {
    ac_surface_warped_out w;                                                     // all NULL without the caller's out_w
    const float *verts; const int32_t *faces; const double *T;                   // the frame's guide
};

__global__ __launch_bounds__(FBLOCK) void posed_shade_kernel(const RenderArgs a, const PosedArgs m, const ac_surface_out out, const PosedOut po)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fill_lds_sdf(lds, a);
    if (out.image) fill_lds_color(lds, a);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    float *fsl = lds + OFF_WAVE + wave * FE_SLAB;
    const FieldCtx fc = make_ctx(a);
    const float bound = a.bound;
    const PosedState &s = m.s;
    const RefineOpts ro{ 0, 0.0f, 0.0f, 0.0f, out.image != nullptr };
    const uint32_t ntiles = (m.N + 15) / 16;
    for (uint32_t tile = blockIdx.x * FW + wave; tile < ntiles; tile += gridDim.x * FW) {
        const uint32_t b = tile * 16 + n, bb = b < m.N ? b : m.N - 1;
        const bool shaded = s.noshade[bb] == 0;
        TileShade r{};
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;
        if (shaded) {
            const float *c = s.can + 3 * (size_t)bb;
            cx = clampf(c[0], -bound, bound); cy = clampf(c[1], -bound, bound); cz = clampf(c[2], -bound, bound);
        }
        const float hx = cx, hy = cy, hz = cz;                                   // this ray's own point
        if (ride_along(shaded, cx, cy, cz))                                      // (wave-uniform)
            r = refine_shade_tile(lds, fsl, fc, a, ro, lane, m.rays_d, (size_t)bb, false, cx, cy, cz);
        if (b < m.N && g == 0) {
            const size_t b3 = 3 * (size_t)b;
            float nm[3] = { 0.0f, 0.0f, 0.0f };
            if (out.normal_map && shaded) {                                      // ac_mesh_pose's rules: M blended at the search's closest point and face
                const size_t f = (size_t)s.face[b];                              // the search's own answer: always a face of the mesh
                const int32_t f0v = po.faces[3 * f], f1v = po.faces[3 * f + 1], f2v = po.faces[3 * f + 2];
                const double q[3] = { s.closest[b3], s.closest[b3 + 1], s.closest[b3 + 2] };
                double bc[3];
                face_bary(q, po.verts, f0v, f1v, f2v, bc);
                const Blend M = blend3(po.T, f0v, f1v, f2v, bc);
                const float nc[3] = { r.fn.nx, r.fn.ny, r.fn.nz };
                normal_store(M, nc, nm);
            }
            store_surface_out(out, m.bg, b, shaded, r, s.t[b], s.pts[b3], s.pts[b3 + 1], s.pts[b3 + 2], nm[0], nm[1], nm[2], s.st[b], s.iters[b]);
            if (po.w.canonical) { po.w.canonical[b3] = shaded ? hx : 0.0f; po.w.canonical[b3 + 1] = shaded ? hy : 0.0f; po.w.canonical[b3 + 2] = shaded ? hz : 0.0f; }
            if (po.w.normal_can) { po.w.normal_can[b3] = shaded ? r.fn.nx : 0.0f; po.w.normal_can[b3 + 1] = shaded ? r.fn.ny : 0.0f; po.w.normal_can[b3 + 2] = shaded ? r.fn.nz : 0.0f; }
            if (po.w.face_id) po.w.face_id[b] =shaded ? s.face[b] : -1;
        }
        wave_sync();
    }
}

size_t posed_state(PosedState *s, void *scratch, uint32_t N)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    char *b = static_cast<char *>(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = b ? b + o : nullptr; o += up(bytes); return p; };
    const size_t n = N;
    double *closest = reinterpret_cast<double *>(take(n * 24)), *dist2 = reinterpret_cast<double *>(take(n * 8));
    float *pts = reinterpret_cast<float *>(take(n * 12)), *can = reinterpret_cast<float *>(take(n * 12));
    int32_t *face = reinterpret_cast<int32_t *>(take(n * 4));
    float *f[6];
    for (auto &p : f) p = reinterpret_cast<float *>(take(n * 4));
    uint8_t *u[6];
    for (auto &p : u) p = reinterpret_cast<uint8_t *>(take(n));
    if (s) *s = PosedState{ pts, can, closest, dist2, face, u[0], u[1], u[2], u[3], u[4], u[5], f[0], f[1], f[2], f[3], f[4], f[5] };
    return o;
}

// the refusals of ac_surface_opts that both entries make, in this order
int check_surface_opts(const char *who, const ac_surface_opts *opts)
{
    if (opts->max_iters < 1 || opts->max_iters > 255) { ac::set_error("%s: max_iters %d outside 1..255", who, opts->max_iters); return AC_ERR_BAD_ARG; }
    if (!(opts->tol >= 0.0f) || !(opts->fd_eps > 0.0f) || !(opts->step_scale > 0.0f) || !(opts->min_step > 0.0f) || !(opts->bound > 0.0f)) {
        ac::set_error("%s: tol not >= 0, or fd_eps, step_scale, min_step or bound not > 0", who); return AC_ERR_BAD_ARG;
    }
    if (!(opts->guard >= 0.0f && opts->guard < 0.5f)) { ac::set_error("%s: guard outside [0, 0.5)", who); return AC_ERR_BAD_ARG; }
    return AC_OK;
}

RayArgs ray_args(const ac_surface_opts *opts, float w_tol, const float *rays_o, const float *rays_d, const float *bg, uint32_t N)
{
    return RayArgs{ rays_o, rays_d, bg, N, { opts->max_iters, opts->level, opts->tol, opts->step_scale, opts->min_step, opts->guard, w_tol } };
}

}  // namespace

AC_API int ac_render_rays_surface(const ac_field *field, const ac_surface_opts *opts, const float *rays_o, const float *rays_d, uint32_t N, const float *bg,
                                  const ac_surface_out *out, ac_stream_t stream)
{
    const char *who = "render_rays_surface";
    if (!field || !opts || !out) { ac::set_error("%s: NULL field, opts or out", who); return AC_ERR_BAD_ARG; }
    if (int rc = check_surface_opts(who, opts)) return rc;
    if (N == 0) return AC_OK;
    if (!rays_o || !rays_d || !out->status) { ac::set_error("%s: NULL rays or status", who); return AC_ERR_BAD_ARG; }
    if (N > 0xffffffe0u) { ac::set_error("%s: more than 2^32 - 32 rays", who); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    launch_tiles<surface_rays_kernel>((N + 15) / 16, FWD_LDS_FLOATS * sizeof(float), (hipStream_t)stream, a, ray_args(opts, 0.0f, rays_o, rays_d, bg, N), *out);
    return ac::check_launch(who);
}

AC_API size_t ac_render_rays_surface_warped_scratch(uint32_t N) { return posed_state(nullptr, nullptr, N); }

AC_API int ac_render_rays_surface_warped(const ac_field *field, const ac_surface_opts *opts, float w_tol, const float *rays_o, const float *rays_d, uint32_t N,
                                         const float *bg, const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, const ac_surface_out *out,
                                         const ac_surface_warped_out *out_w, ac_stream_t stream)
{
    const char *who = "render_rays_surface_warped";
    if (!field || !opts || !out) { ac::set_error("%s: NULL field, opts or out", who); return AC_ERR_BAD_ARG; }
    if (int rc = check_surface_opts(who, opts)) return rc;
    if (!(w_tol >= 0.0f)) { ac::set_error("%s: w_tol not >= 0", who); return AC_ERR_BAD_ARG; }
    if (!mesh || !mesh->verts || !mesh->faces || !mesh->T || mesh->F == 0) { ac::set_error("%s: NULL mesh, verts, faces or T, or a mesh without faces", who); return AC_ERR_BAD_ARG; }
    if (N == 0) return AC_OK;
    if (!rays_o || !rays_d || !out->status) { ac::set_error("%s: NULL rays or status", who); return AC_ERR_BAD_ARG; }
    if (N > 0xffffffe0u) { ac::set_error("%s: more than 2^32 - 32 rays", who); return AC_ERR_BAD_ARG; }
    const size_t need = ac_render_rays_surface_warped_scratch(N);
    if (!scratch || scratch_bytes < need) { ac::set_error("%s: scratch smaller than %zu bytes", who, need); return AC_ERR_BAD_ARG; }
    RenderArgs a{};
    if (int rc = prep_args(a, field, opts->bound, opts->fd_eps)) return rc;
    PosedArgs m{ ray_args(opts, w_tol, rays_o, rays_d, bg, N), sqrtf((float)mesh->threshold), {} };
    posed_state(&m.s, scratch, N);
    const PosedState &s = m.s;
    const hipStream_t st = (hipStream_t)stream;
    // the culled search where the structure covers the mesh (it skips the rays flagged in `dead`), else the exhaustive one: the same bits
    const bool culled = mesh->accel && ac_warp_accel_bytes(mesh->F) != 0;
    auto search = [&](const uint8_t *dead, double *closest, int32_t *face) {
        if (culled)
            return ac::warp_samples_accel_impl(s.pts, mesh->verts, mesh->faces, mesh->T, N, mesh->V, mesh->F, mesh->threshold, mesh->accel, nullptr, s.can, closest,
                                               s.dist2, face, s.smask, stream, 0, dead, 1);
        return ac_warp_samples(s.pts, mesh->verts, mesh->faces, mesh->T, N, mesh->V, mesh->F, mesh->threshold, nullptr, s.can, closest, s.dist2, face, s.smask, stream);
    };
    hipLaunchKernelGGL(posed_start_kernel, dim3((N + 255) / 256), dim3(256), 0, st, m, opts->bound);
    if (int rc = ac::check_launch(who)) return rc;
    const uint32_t ntiles = (N + 15) / 16, blocks = tile_blocks(ntiles);
    for (int it = 1; it <= opts->max_iters; ++it) {
        if (int rc = search(s.stopped, nullptr, nullptr)) return rc;
        hipLaunchKernelGGL(posed_trip_kernel, dim3(blocks), dim3(FBLOCK), OFF_WAVE * sizeof(float), st, a, m, it);
        if (int rc = ac::check_launch(who)) return rc;
    }
    if (int rc = search(s.noshade, s.closest, s.face)) return rc;
    const PosedOut po{ out_w ? *out_w : ac_surface_warped_out{}, mesh->verts, mesh->faces, mesh->T };
    launch_tiles<posed_shade_kernel>(ntiles, FWD_LDS_FLOATS * sizeof(float), st, a, m, *out, po);
    return ac::check_launch(who);
}
