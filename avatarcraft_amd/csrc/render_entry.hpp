// avatarcraft_amd/csrc/render_entry.hpp -- the host side that the C entries of the two ray renderers share (render_fused.hip, render_long.hip; included
// behind render_slab.hpp): what an entry is (RenderEntry), the one check of its options and buffers, the RenderArgs fill, the view of the posed
// scratch and the posed sequence.  An entry is: its descriptor, check_render_entry, fill_entry_args, its launch.
#pragma once
#include "render_slab.hpp"

namespace {

constexpr int SHORT_MAX_T = 128, LONG_MAX_T = 512;      // samples per ray of the two windows (each renderer's MAXT)

// the rules that differ between the entries are functions of these switches (check_render_entry)
enum : unsigned {
    K_LONG = 1,               // the long window: num_steps >= 2, upsample_steps a multiple of 16, at most 512 samples; else multiples of 16, num_steps <= 64, at most 128
    K_POSED = 2,              // posed space: takes a mesh and a scratch, runs render_posed
    K_PAIR = 4,               // the same rays twice in one launch
    K_H16 = 8,                // gathers from the half table (an inference path: no training option)
    K_SAMPLING = 16,          // the sampling stage alone: z_vals is the only output, there is no ac_render_out
};
struct RenderEntry {
    const char *name;       // names the entry in every error
    bool lng, posed, pair, h16, sampling;
    constexpr RenderEntry(const char *n, unsigned kind) : name(n), lng(kind & K_LONG), posed(kind & K_POSED), pair(kind & K_PAIR), h16(kind & K_H16), sampling(kind & K_SAMPLING) {}
};

struct RayInputs { const float *rays_o, *rays_d, *bg, *noise, *lin_z, *lin_u; };

bool wants_samples(const ac_render_out &o)
{
    return o.z_vals || o.weights || o.alpha || o.color || o.sdf || o.gradient || o.ss_inds || o.sort_index || o.sdf_out16 || o.pts || o.feat7;
}

// Everything an entry refuses, before any device work; an empty batch (n_rays <= 0) is held to the options' rules, its buffers are not looked at.
// out: NULL for a sampling entry (z_vals instead); table_h16 / mesh: read for h16 / posed entries only.
int check_render_entry(const RenderEntry &d, const ac_field *field, const void *table_h16, const ac_render_opts *op, const RayInputs &in,
                       const ac_warp_mesh *mesh, const ac_render_out *out, const float *z_vals = nullptr)
{
    const char *who = d.name;
    if (!op || (d.sampling ? !z_vals : !out) || (d.posed && !mesh)) {
        ac::set_error("%s: NULL opts/%s%s", who, d.sampling ? "z_vals" : "out", d.posed ? "/mesh" : ""); return AC_ERR_BAD_ARG;
    }
    const int T = op->num_steps + op->upsample_steps;
    if (d.lng) {
        if (op->num_steps < 2 || op->upsample_steps < 0 || op->upsample_steps % 16 || T > LONG_MAX_T) {
            ac::set_error("%s: num_steps=%d upsample_steps=%d unsupported (num_steps >= 2, upsample_steps >= 0 and a multiple of 16, "
                          "num_steps + upsample_steps <= %d)", who, op->num_steps, op->upsample_steps, LONG_MAX_T);
            return AC_ERR_BAD_ARG;
        }
    } else if (op->num_steps % 16 || op->upsample_steps % 16 || op->num_steps < 16 || op->num_steps > 64 || op->upsample_steps < 0 || T > SHORT_MAX_T) {
        ac::set_error("%s: num_steps=%d upsample_steps=%d unsupported (multiples of 16, num_steps<=64, sum<=128)", who, op->num_steps, op->upsample_steps);
        return AC_ERR_BAD_ARG;
    }
    if (!(op->fd_eps > 0.0f)) {      // the reference stops here too: `assert (gradient == gradient).all()` after dividing by eps = 0 (instant_nsr.py:274)
        ac::set_error("%s: fd_eps = %g (normal_epsilon_ratio >= 1): the finite-difference normals divide by it, it must be positive", who, (double)op->fd_eps);
        return AC_ERR_BAD_ARG;
    }
    if (d.h16) {
        if (!field) { ac::set_error("%s: NULL field", who); return AC_ERR_BAD_ARG; }
        if (!table_h16) { ac::set_error("%s: NULL half table (ac_table_to_half makes it: one dword per entry)", who); return AC_ERR_BAD_ARG; }
        if (op->opacity_only) { ac::set_error("%s: opacity_only is not built for the half table (it serves the frozen avatar of a training step: fp32 entries)", who); return AC_ERR_BAD_ARG; }
        if (out->feat7 || out->sdf_out16 || out->pts) {
            ac::set_error("%s: feat7 / sdf_out16 / pts are the training extras: the half table is an inference path (nothing trains from it)", who);
            return AC_ERR_BAD_ARG;
        }
    }
    if (op->precision != 0 && op->precision != 1) { ac::set_error("%s: precision %d unknown (0 = exact, 1 = fast)", who, op->precision); return AC_ERR_BAD_ARG; }
    if (op->opacity_only != 0 && op->opacity_only != 1) { ac::set_error("%s: opacity_only must be 0 or 1", who); return AC_ERR_BAD_ARG; }
    if (op->opacity_only && d.posed && d.lng) {
        ac::set_error("%s: opacity_only is a canonical-space option of the long renderer (ac_render_rays_long); the posed entry evaluates the colour network", who);
        return AC_ERR_BAD_ARG;
    }
    if (op->skip_masked != 0 && op->skip_masked != 1) { ac::set_error("%s: skip_masked must be 0 or 1", who); return AC_ERR_BAD_ARG; }
    if (op->skip_masked && d.lng && !d.posed) {      // (the canonical entries of the short window accept it and ignore it)
        ac::set_error("%s: skip_masked is a posed-space option; this entry is canonical (posed: ac_render_rays_long_warped)", who); return AC_ERR_BAD_ARG;
    }
    if ((op->near_m != nullptr) != (op->far_m != nullptr)) { ac::set_error("%s: near_m and far_m go together", who); return AC_ERR_BAD_ARG; }
    if (d.lng && out && out->feat7) {
        if (d.posed) { ac::set_error("%s: feat7 (the fused training backward's features) is not produced by the long renderer", who); return AC_ERR_BAD_ARG; }
        // the stencil features exist per tile of 16 samples of one ray: only a count 16 divides has them (other counts gather again in the backward)
        if (T % 16) {
            ac::set_error("%s: feat7 needs T = num_steps + upsample_steps a multiple of 16 (T = %d); at other counts pass NULL: ac_render_core_backward gathers again", who, T);
            return AC_ERR_BAD_ARG;
        }
    }
    if (op->n_rays <= 0) return AC_OK;
    if (!in.rays_o || !in.rays_d || !in.lin_z || (op->upsample_steps && !in.lin_u) || (op->perturb && !in.noise) ||
        (out && (!out->image || !out->weights_sum || !out->depth || !out->normal_map || !out->eik))) {
        ac::set_error("%s: NULL buffer", who); return AC_ERR_BAD_ARG;
    }
    if (d.pair && op->n_rays > (1 << 29)) { ac::set_error("%s: too many rays", who); return AC_ERR_BAD_ARG; }
    if (d.posed && d.lng && (size_t)op->n_rays * (size_t)T > 0x7fffffffu) {
        ac::set_error("%s: %d rays x %d samples: too many samples for one launch", who, op->n_rays, T); return AC_ERR_BAD_ARG;
    }
    return AC_OK;
}

// RenderArgs of one launch over op->n_rays rays.  table_h16 non-NULL: the half table in the table's place (field->table is not read); the descriptor then
// covers n_entries dwords: the hardware bounds check in the half table's unit.  out: NULL leaves a.out empty (the sampling entries).
int fill_entry_args(RenderArgs &a, const ac_field *field, const void *table_h16, const ac_render_opts *op, const RayInputs &in, const ac_render_out *out)
{
    ac_field f;
    if (table_h16) { f = *field; f.table = static_cast<const float *>(table_h16); field = &f; }
    if (int rc = fill_render_common(a, field, op, in.rays_o, in.rays_d, in.bg, in.noise, in.lin_z, in.lin_u)) return rc;
    if (table_h16) a.table_bytes = (uint32_t)f.offsets[16] * 4u;
    if (out) a.out = *out;
    a.pair_n = 0; a.ex_from = 0; a.ex_rows = op->n_rays;
    a.skip_masked = op->skip_masked;
    a.opacity_only = op->opacity_only;
    return AC_OK;
}
// ... over the same rays twice (the pair entries): 2 n_rays work items, the per-sample outputs kept for copy b
void make_pair_args(RenderArgs &a) { a.pair_n = a.n_rays; a.ex_from = a.n_rays; a.ex_rows = a.n_rays; a.n_rays *= 2; }

// byte offsets of the segments of the posed scratch, 256-byte aligned: near_m, far_m [N] f32; pts, can [N,T,3] f32; mask [N,T] u8; zbuf [N,T] f32;
// ray_dead [N] u8 (skip_masked) -> the size.  ac_render_rays_warped_scratch documents the first six.
size_t warped_scratch_offsets(int32_t n_rays, int32_t T, size_t offs[7])
{
    const size_t N = n_rays > 0 ? (size_t)n_rays : 0, NT = N * (size_t)(T > 0 ? T : 0);
    const size_t sz[7] = { N * 4, N * 4, NT * 12, NT * 12, NT, NT * 4, N };
    size_t o = 0;
    for (int i = 0; i < 7; ++i) { offs[i] = o; o += (sz[i] + 255) & ~(size_t)255; }
    return o;
}
struct WarpedScratch {
    size_t need;
    float *near_m, *far_m, *pts, *can;
    uint8_t *mask;
    float *zbuf;
    uint8_t *ray_dead;
    WarpedScratch(void *scratch, int n_rays, int T)
    {
        size_t o[7];
        need = warped_scratch_offsets(n_rays, T, o);
        char *sc = static_cast<char *>(scratch);
        near_m = reinterpret_cast<float *>(sc + o[0]); far_m = reinterpret_cast<float *>(sc + o[1]);
        pts = reinterpret_cast<float *>(sc + o[2]); can = reinterpret_cast<float *>(sc + o[3]);
        mask = reinterpret_cast<uint8_t *>(sc + o[4]); zbuf = reinterpret_cast<float *>(sc + o[5]); ray_dead = reinterpret_cast<uint8_t *>(sc + o[6]);
    }
};

// The posed sequence of ac_render_rays_warped, ac_render_rays_warped_h16 and ac_render_rays_long_warped: mesh near / far -> coarse posed points -> (ray cull)
// -> first closest-face search -> launch_upsample(a): MODE_UPSAMPLE (coarse sdf at the warped coarse points, up-sampling, z and the posed mid points) ->
// second search -> launch_final(a): MODE_FINAL (field at the warped mid points, alpha * mask, optional skipping of fully masked tiles), with the phase
// marks of ac_debug_warped_phases between them.  a: the entry's filled arguments; this adds what the sequence itself produces.
template <class Up, class Fin>
int render_posed(const RenderEntry &d, RenderArgs &a, const ac_warp_mesh *mesh, void *scratch, size_t scratch_bytes, ac_stream_t stream,
                 Up &&launch_upsample, Fin &&launch_final)
{
    if (!mesh->verts || !mesh->faces || !mesh->T || mesh->V == 0 || mesh->F == 0) { ac::set_error("%s: NULL mesh buffer or empty mesh", d.name); return AC_ERR_BAD_ARG; }
    const int N = a.n_rays, T0 = a.T0, T = T0 + 16 * a.nup;
    const WarpedScratch s(scratch, N, T);
    if (!scratch || scratch_bytes < s.need) { ac::set_error("%s: scratch of %zu bytes needed, %zu given", d.name, s.need, scratch_bytes); return AC_ERR_BAD_ARG; }
    char step[96];
    const uint8_t *ray_dead = nullptr;
    hipStream_t st = (hipStream_t)stream;
    ac::warped_phase_mark(0, st);
    if (mesh->use_mesh_guide) {
        if (int rc = ac_mesh_near_far(a.rays_o, a.rays_d, mesh->verts, (uint32_t)N, mesh->V, mesh->geo_threshold, s.near_m, s.far_m, stream)) return rc;
        a.near_m = s.near_m; a.far_m = s.far_m;
    }
    a.zbuf = s.zbuf; a.mid_pts = s.pts;
    if (a.nup > 0) {                                              // coarse samples -> canonical space (:166-172)
        snprintf(step, sizeof step, "%s (coarse points)", d.name);
        if (int rc = ac::warped_coarse_pts(step, a.rays_o, a.rays_d, a.near_m, a.far_m, a.lin_z, a.noise, N, T0, a.bound, a.perturb, s.pts, st)) return rc;
        if (a.skip_masked && mesh->accel) {                       // rays that cannot hold an unmasked sample: no search, no field evaluation
            if (int rc = ac::warp_ray_cull(s.pts, (uint32_t)N, (uint32_t)T0, mesh->threshold, mesh->accel, s.ray_dead, stream)) return rc;
            ray_dead = s.ray_dead;
        }
        ac::warped_phase_mark(1, st);
        if (int rc = ac::warp_any(mesh, s.pts, (uint32_t)(N * T0), s.can, s.mask, stream, 0, ray_dead, (uint32_t)T0, 0u)) return rc;
    } else ac::warped_phase_mark(1, st);
    ac::warped_phase_mark(2, st);
    a.ext_pts = s.can;
    a.ray_dead = ray_dead;
    launch_upsample(a);                                           // coarse sdf, up-sampling, mid points (posed space)
    snprintf(step, sizeof step, "%s (up-sampling)", d.name);
    if (int rc = ac::check_launch(step)) return rc;
    ac::warped_phase_mark(3, st);
    // (skip_masked: the final pass does not evaluate masked-out samples, so the search may leave out those the cell grids prove masked)
    if (int rc = ac::warp_any(mesh, s.pts, (uint32_t)(N * T), s.can, s.mask, stream, a.skip_masked, ray_dead, (uint32_t)T, (uint32_t)T0)) return rc;     // :198-203
    ac::warped_phase_mark(4, st);
    a.mask = s.mask;
    launch_final(a);
    ac::warped_phase_mark(5, st);
    return ac::check_launch(d.name);
}

}  // namespace
